"""What the temporal resolve costs: brmi_temporal_resolve alone on the headline 4K frame (Bistro-class, bench.py's default workload) -- HIP events around runs of
stage calls, with a history -- and the frame with and without the stage bound, all from one run.

    python tools/temporal_cost.py [--frames 50] [--repeats 3] [--size 3840x2160] [--step-timeout 300] [--write profiles/temporal_cost.md]

The GPU step runs in a child process of its own under `timeout`; one that fails or runs out of time ends the script with its status -- nothing more is started
on the device behind it.  Prints one JSON line; --write also records it as a table beside the display chain's figure and the ideal byte time.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BYTES_PER_PIXEL = 8 + 4 + 4 + 8 + 8      # HDR, depth, motion, about one history texel (four taps shared with the neighbours), the output
PEAK_GB_S = 8000.0                       # MI355X HBM3E
DISPLAY_CHAIN_MS = 0.6941                # profiles/display_cost.md: the frame's difference with the display chain bound


def step(a):
    """The child: frames with the stage off / on (alternating repeats), then the stage alone."""
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
        r.set_temporal(0.1 if setting == "on" else None)
        for _ in range(10):
            r.execute()
        torch.cuda.synchronize()
        res[setting].append(timed(r.execute, a.frames))      # (a still jitter phase: update() is host work and not part of the stage)
    r.set_temporal(0.1)
    r.execute(); r.execute()
    out = {"scene": "bistro_4k", "size": [W, H], "frames_per_repeat": a.frames, "frame_ms": res,
           "stage_ms": [timed(lambda: r.stage("temporal_resolve"), a.frames) for _ in range(a.repeats)]}
    print(json.dumps(out), flush=True)
    r.close()


def table(out):
    med = lambda v: sorted(v)[len(v) // 2]
    W, H = out["size"]
    off, on, stage = med(out["frame_ms"]["off"]), med(out["frame_ms"]["on"]), med(out["stage_ms"])
    ideal = W * H * BYTES_PER_PIXEL / (PEAK_GB_S * 1e9) * 1e3
    lines = ["# Temporal resolve: cost at %d x %d on an MI355X (tools/temporal_cost.py)\n" % (W, H),
             f"Bistro-class frame of the benchmark, blend 0.1, a valid history; HIP events around {out['frames_per_repeat']} frames or stage calls,",
             f"{len(out['stage_ms'])} repeats, one run.  Medians; every repeat in brackets.\n", "| what | ms |", "|---|---|",
             f"| frame, stage off | {off:.4f} ({', '.join('%.4f' % x for x in out['frame_ms']['off'])}) |",
             f"| frame, stage on | {on:.4f} ({', '.join('%.4f' % x for x in out['frame_ms']['on'])}) |", f"| difference | {on - off:.4f} |",
             f"| brmi_temporal_resolve alone | {stage:.4f} ({', '.join('%.4f' % x for x in out['stage_ms'])}) |",
             f"| the display chain, for scale (profiles/display_cost.md: frame difference) | {DISPLAY_CHAIN_MS:.4f} |\n",
             f"Bytes alone: {BYTES_PER_PIXEL} B per pixel ({W * H * BYTES_PER_PIXEL / 1e6:.0f} MB) at {PEAK_GB_S / 1000:.0f} TB/s is {ideal:.4f} ms; the stage alone reaches "
             f"{100.0 * ideal / stage:.0f} % of that rate.  No pass/fail threshold hangs on these numbers."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50); ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--write", default=None, metavar="FILE.md"); ap.add_argument("--step-timeout", type=int, default=300); ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return step(a)
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--frames", str(a.frames), "--repeats", str(a.repeats), "--size", a.size]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:      # a fault, an abort or the time limit: nothing more on the device
        print(json.dumps({"failed_step": "temporal_cost", "status": p.returncode}), flush=True)
        sys.exit(p.returncode)
    line = [x for x in p.stdout.splitlines() if x.startswith("{")][-1]
    print(line, flush=True)
    if a.write:
        with open(a.write, "w") as f:
            f.write(table(json.loads(line)))


if __name__ == "__main__":
    main()
