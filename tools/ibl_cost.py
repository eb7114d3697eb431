"""What image-based lighting costs: the shading stage (brmi_stage_times, HIP events) of the headline 4K frame (Bistro-class, bench.py's default workload)
with the environment off and on (with and without the specular part), serial (brmi_execute) and with the shading half on a stream of its own
(brmi_execute_split, the k_shade<0, 3> / k_shade_ibl<0, 3> variants).

    python tools/ibl_cost.py [--frames 100] [--repeats 3] [--size 3840x2160] [--lib PATH]

`off` is measured before and after the others: the spread of its repeats is what a difference has to exceed.  --lib (BRMI_LIB_PATH) runs the same script on
another build of the library, e.g. the parent commit's; one that lacks brmi_set_environment measures `off` only.  Run the two builds in turn, several times
each, on one machine.  Prints one JSON line per mode: per setting, a (shading ms, sum of all stages ms) pair per repeat.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100); ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", default="3840x2160"); ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        os.environ["BRMI_LIB_PATH"] = os.path.abspath(a.lib)
    import torch
    from basicrenderer_amd import Scene
    from basicrenderer_amd.environment import Environment
    from basicrenderer_amd.renderer import VisibilityRenderer
    W, H = (int(x) for x in a.size.lower().split("x"))
    sc = Scene("bistro", W, H, point_lights=256, directional=True, unique_budget=True, lod_builder="own", relief_slope=1.5)
    env = Environment.procedural(64)
    for mode in ("serial", "in_flight"):
        r = VisibilityRenderer(sc, occlusion=True, stats=True)
        can = hasattr(r.lib, "brmi_set_environment")
        other = torch.cuda.Stream(device=r.device) if mode == "in_flight" else None

        def run(setting):
            if can:
                r.set_environment(None if setting is None else env, specular=setting != "diffuse_only")
            for _ in range(10):
                r.execute(other)
            torch.cuda.synchronize()
            r.stage_times()
            out = []
            for _ in range(a.repeats):
                for _ in range(a.frames):
                    r.execute(other)
                torch.cuda.synchronize()
                t = r.stage_times()
                out.append((round(t["shade"], 4), round(sum(t.values()), 4)))
            return out

        res = {"off": run(None)}
        if can:
            res["on"] = run("on")
            res["diffuse_only"] = run("diffuse_only")
            res["off_again"] = run(None)
        torch.cuda.synchronize()
        print(json.dumps({"scene": "bistro_4k", "mode": mode, "size": [W, H], "frames_per_repeat": a.frames, "lib": os.environ.get("BRMI_LIB_PATH", "in-tree"), "shade_ms_frame_ms": res}), flush=True)
        r.close()


if __name__ == "__main__":
    main()
