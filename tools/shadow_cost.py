"""What shadow maps cost: `brmi_shade` of the headline 4K frame (Bistro-class, bench.py's default workload) with shadows unbound and with 1, 8 and 32 shadowed
point lights bound, and one 1024 x 1024 light view (geometry stages + brmi_shadow_capture) -- HIP events around runs of stage calls, all from one run.

    python tools/shadow_cost.py [--calls 50] [--repeats 3] [--size 3840x2160] [--step-timeout 400] [--write profiles/shadow_cost.md]

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
COUNTS = (1, 8, 32)


def step(a):
    import numpy as np
    import torch
    from basicrenderer_amd import Scene, shadows
    from basicrenderer_amd.renderer import VisibilityRenderer
    W, H = (int(x) for x in a.size.lower().split("x"))
    sc = Scene("bistro", W, H, point_lights=256, directional=True, unique_budget=True, lod_builder="own", relief_slope=1.5)
    r = VisibilityRenderer(sc, occlusion=True)
    points = [int(i) for i in np.flatnonzero(sc.arrays["lights"].view(shadows.LIGHT_DTYPE)["type"] == shadows.LIGHT_POINT)]

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record(); e1.synchronize()
        return round(e0.elapsed_time(e1) / n, 4)

    def shade_times():
        for _ in range(3):
            r.execute()
        torch.cuda.synchronize()
        return [timed(lambda: r.stage("shade"), a.calls) for _ in range(a.repeats)]

    out = {"scene": "bistro_4k", "size": [W, H], "calls_per_repeat": a.calls, "shade_ms": {"unbound": shade_times()}}
    for n in COUNTS:
        r.set_shadows(points[:n], point_resolution=256)
        r.render_shadow_maps()
        out["shade_ms"][str(n)] = shade_times()
    r.set_shadows(points[:1], point_resolution=1024)
    r.render_shadow_maps()
    out["light_view_1024_ms"] = [timed(lambda: r.render_shadow_view(0), 20) for _ in range(a.repeats)]
    r.set_shadows(None)
    out["shade_ms"]["unbound_again"] = shade_times()
    print(json.dumps(out), flush=True)
    r.close()


def table(out):
    med = lambda v: sorted(v)[len(v) // 2]
    lines = ["# Shadow maps: cost at %d x %d on an MI355X (tools/shadow_cost.py)\n" % tuple(out["size"]),
             f"Bistro-class frame of the benchmark, 256 point lights + 1 directional; shadowed lights are the first point lights of the scene, cube faces 256 x 256.",
             f"HIP events around {out['calls_per_repeat']} calls of `brmi_shade`, {len(out['shade_ms']['unbound'])} repeats, one run.  Medians; every repeat in brackets.\n",
             "| `brmi_shade` with | ms |", "|---|---|"]
    names = {"unbound": "shadows unbound (`k_shade`, the parent's kernels)", "1": "1 shadowed light", "8": "8 shadowed lights", "32": "32 shadowed lights", "unbound_again": "unbound again"}
    for k, v in out["shade_ms"].items():
        lines.append(f"| {names[k]} | {med(v):.4f} ({', '.join('%.4f' % x for x in v)}) |")
    v = out["light_view_1024_ms"]
    lines += ["", f"One 1024 x 1024 light view (camera upload, brmi_update, clear, cull, raster, depth copy, brmi_shadow_capture; host-issued, 20 in a row): {med(v):.4f} ms ({', '.join('%.4f' % x for x in v)})."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50); ap.add_argument("--repeats", type=int, default=3); ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--write", default=None, metavar="FILE.md"); ap.add_argument("--step-timeout", type=int, default=400); ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return step(a)
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--repeats", str(a.repeats), "--size", a.size]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:      # a fault, an abort or the time limit: nothing more on the device
        print(json.dumps({"failed_step": "shadow_cost", "status": p.returncode}), flush=True)
        sys.exit(p.returncode)
    line = [x for x in p.stdout.splitlines() if x.startswith("{")][-1]
    print(line, flush=True)
    if a.write:
        with open(a.write, "w") as f:
            f.write(table(json.loads(line)))


if __name__ == "__main__":
    main()
