"""What XeGTAO costs: the headline 4K frame (Bistro-class, bench.py's default workload) with an environment bound, with and without GTAO, and the three stages
alone -- HIP events around runs of frames / stage calls.

    python tools/gtao_cost.py [--frames 50] [--repeats 3] [--size 3840x2160] [--quality high] [--lib PATH] [--step-timeout 300]

Every GPU step (one build of the library, one setting) runs in a child process of its own under `timeout`; a step that fails or runs out of time ends the
script with its status -- nothing more is started on the device behind it.  --lib (BRMI_LIB_PATH) measures the frame of another build of the library, e.g. the
parent commit's: one that lacks brmi_set_gtao gives its `off` frame with the same environment.  Prints one JSON line per step.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step(a):
    """One child: frames with GTAO off / on (alternating repeats), then the stages alone."""
    import torch
    from basicrenderer_amd import Scene
    from basicrenderer_amd.environment import Environment
    from basicrenderer_amd.renderer import VisibilityRenderer
    W, H = (int(x) for x in a.size.lower().split("x"))
    sc = Scene("bistro", W, H, point_lights=256, directional=True, unique_budget=True, lod_builder="own", relief_slope=1.5)
    r = VisibilityRenderer(sc, occlusion=True)
    r.set_environment(Environment.procedural(64))
    can = hasattr(r.lib, "brmi_set_gtao")

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record(); e1.synchronize()
        return round(e0.elapsed_time(e1) / n, 4)

    res = {"off": [], "on": []}
    for setting in (["off", "on"] if can else ["off"]) * a.repeats:
        if can:
            r.set_gtao(a.quality if setting == "on" else None, denoise=a.denoise, max_depth_lod=a.max_depth_lod)
        for _ in range(10):
            r.execute()
        torch.cuda.synchronize()
        res[setting].append(timed(r.execute, a.frames))
    out = {"scene": "bistro_4k_env", "size": [W, H], "frames_per_repeat": a.frames, "lib": os.environ.get("BRMI_LIB_PATH", "in-tree"), "frame_ms": res}
    if can:
        r.set_gtao(a.quality, denoise=a.denoise, max_depth_lod=a.max_depth_lod)
        r.execute()
        out["quality"], out["denoise"], out["max_depth_lod"] = a.quality, a.denoise, a.max_depth_lod
        out["stage_ms"] = {name: [timed(lambda: r.stage(name), a.frames) for _ in range(a.repeats)] for name in ("gtao_prefilter", "gtao_main", "gtao_denoise")}
    print(json.dumps(out), flush=True)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50); ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", default="3840x2160"); ap.add_argument("--quality", default="high"); ap.add_argument("--denoise", type=int, default=1)
    ap.add_argument("--max-depth-lod", type=int, default=0)
    ap.add_argument("--lib", action="append", default=None, help="another build of libbrmi.so to measure as well (repeatable)")
    ap.add_argument("--step-timeout", type=int, default=300); ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return step(a)
    base = [sys.executable, os.path.abspath(__file__), "--child", "--frames", str(a.frames), "--repeats", str(a.repeats), "--size", a.size, "--quality", a.quality,
            "--denoise", str(a.denoise), "--max-depth-lod", str(a.max_depth_lod)]
    for lib in [None] + [os.path.abspath(p) for p in (a.lib or [])]:
        env = dict(os.environ)
        if lib:
            env["BRMI_LIB_PATH"] = lib
        rc = subprocess.call(["timeout", "-k", "10", str(a.step_timeout)] + base, env=env)
        if rc != 0:      # a fault, an abort or the time limit: nothing more on the device
            print(json.dumps({"failed_step": lib or "in-tree", "status": rc}), flush=True)
            sys.exit(rc)


if __name__ == "__main__":
    main()
