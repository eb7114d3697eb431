"""What anisotropic filtering costs: the G-buffer stage and the frame (brmi_stage_times, HIP events) of the San-Miguel-class 4K frame (material features 24)
and the Sponza-class textured frame (features 8), with the feature off, every sampler at 1 (the ANISO kernels with one tap), 4 and 16.

    python tools/aniso_cost.py [--frames 100] [--repeats 3] [--size 3840x2160] [--lib PATH]

`off` is measured before and after the others: the spread of its repeats is what a difference has to exceed.  --lib (BRMI_LIB_PATH) runs the same
script on another build of the library, e.g. the parent commit's; one that lacks brmi_set_sampler_anisotropy measures `off` only.  Run the two builds in
turn, several times each, on one machine.  Prints one JSON line per scene: per setting, a (G-buffer ms, sum of all stages ms) pair per repeat.
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
    from basicrenderer_amd.renderer import VisibilityRenderer
    W, H = (int(x) for x in a.size.lower().split("x"))
    for label, preset, features, lights in (("san_miguel_4k", "san_miguel", 24, 256), ("sponza_textured_4k", "sponza", 8, 64)):
        sc = Scene(preset, W, H, point_lights=lights, directional=True, material_features=features)
        r = VisibilityRenderer(sc, occlusion=True, stats=True)
        can = hasattr(r.lib, "brmi_set_sampler_anisotropy")

        def run(setting):
            if can:
                r.set_anisotropy(setting)
            for _ in range(10):
                r.execute()
            r.stage_times()
            out = []
            for _ in range(a.repeats):
                for _ in range(a.frames):
                    r.execute()
                t = r.stage_times()
                out.append((round(t["gbuffer"], 4), round(sum(t.values()), 4)))
            return out

        res = {"off": run(None)}
        if can:
            for k in (1, 4, 16):
                res[str(k)] = run(k)
            res["off_again"] = run(None)
        torch.cuda.synchronize()
        print(json.dumps({"scene": label, "size": [W, H], "frames_per_repeat": a.frames, "lib": os.environ.get("BRMI_LIB_PATH", "in-tree"), "gbuffer_ms_frame_ms": res}), flush=True)
        r.close()


if __name__ == "__main__":
    main()
