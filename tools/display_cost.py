"""What the display chain costs: the headline 4K frame (Bistro-class, bench.py's default workload) with and without the chain bound, and the three stages
alone -- HIP events around runs of frames / stage calls, all from one run.

    python tools/display_cost.py [--frames 50] [--repeats 3] [--size 3840x2160] [--tonemap lpm] [--no-bloom] [--step-timeout 300] [--write profiles/display_cost.md]

The GPU step runs in a child process of its own under `timeout`; one that fails or runs out of time ends the script with its status -- nothing more is started
on the device behind it.  Prints one JSON line; --write also records it as a table.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ("display_exposure", "display_bloom", "display_resolve")


def step(a):
    """The child: frames with the chain off / on (alternating repeats), then the stages alone."""
    import torch
    from basicrenderer_amd import Scene
    from basicrenderer_amd.renderer import VisibilityRenderer
    W, H = (int(x) for x in a.size.lower().split("x"))
    sc = Scene("bistro", W, H, point_lights=256, directional=True, unique_budget=True, lod_builder="own", relief_slope=1.5)
    r = VisibilityRenderer(sc, occlusion=True)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record(); e1.synchronize()
        return round(e0.elapsed_time(e1) / n, 4)

    res = {"off": [], "on": []}
    for setting in ["off", "on"] * a.repeats:
        r.set_display(a.tonemap if setting == "on" else None, bloom=not a.no_bloom, time_coefficient=1.0 / 60.0)
        for _ in range(10):
            r.execute()
        torch.cuda.synchronize()
        res[setting].append(timed(r.execute, a.frames))
    r.set_display(a.tonemap, bloom=not a.no_bloom, time_coefficient=1.0 / 60.0)
    r.execute()
    stages = [s for s in STAGES if not (a.no_bloom and s == "display_bloom")]
    out = {"scene": "bistro_4k", "size": [W, H], "frames_per_repeat": a.frames, "tonemap": a.tonemap, "bloom": not a.no_bloom, "frame_ms": res,
           "stage_ms": {name: [timed(lambda: r.stage(name), a.frames) for _ in range(a.repeats)] for name in stages}}
    print(json.dumps(out), flush=True)
    r.close()


def table(out):
    med = lambda v: sorted(v)[len(v) // 2]
    off, on = med(out["frame_ms"]["off"]), med(out["frame_ms"]["on"])
    lines = ["# Display chain: cost at %d x %d on an MI355X (tools/display_cost.py)\n" % tuple(out["size"]),
             f"Bistro-class frame of the benchmark, tone map `{out['tonemap']}`, bloom {'on' if out['bloom'] else 'off'}; HIP events around {out['frames_per_repeat']} frames or stage calls,",
             f"{len(out['frame_ms']['off'])} repeats, one run.  Medians; every repeat in brackets.\n", "| what | ms |", "|---|---|",
             f"| frame, chain off | {off:.4f} ({', '.join('%.4f' % x for x in out['frame_ms']['off'])}) |",
             f"| frame, chain on | {on:.4f} ({', '.join('%.4f' % x for x in out['frame_ms']['on'])}) |", f"| difference | {on - off:.4f} |"]
    for name, v in out["stage_ms"].items():
        lines.append(f"| brmi_{name} alone | {med(v):.4f} ({', '.join('%.4f' % x for x in v)}) |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50); ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", default="3840x2160"); ap.add_argument("--tonemap", default="lpm"); ap.add_argument("--no-bloom", action="store_true")
    ap.add_argument("--write", default=None, metavar="FILE.md"); ap.add_argument("--step-timeout", type=int, default=300); ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return step(a)
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--frames", str(a.frames), "--repeats", str(a.repeats),
           "--size", a.size, "--tonemap", a.tonemap] + (["--no-bloom"] if a.no_bloom else [])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:      # a fault, an abort or the time limit: nothing more on the device
        print(json.dumps({"failed_step": "display_cost", "status": p.returncode}), flush=True)
        sys.exit(p.returncode)
    line = [x for x in p.stdout.splitlines() if x.startswith("{")][-1]
    print(line, flush=True)
    if a.write:
        with open(a.write, "w") as f:
            f.write(table(json.loads(line)))


if __name__ == "__main__":
    main()
