"""What the sky and the environment build cost (HIP events around the calls, medians over repeats).

    python tools/envbuild_cost.py [--frames 50] [--repeats 5] [--size 3840x2160] [--faces 512]

* the skybox stage (brmi_skybox alone, on the surfaces of the frame just rendered) on the headline 4K frame (Bistro-class, bench.py's default workload), which has
  few empty pixels, and on a frame that is half sky: the same frame with the depth plane's upper half set to "empty";
* the whole frame (brmi_execute) with the environment bound, skybox off and on;
* the three build stages at `--faces`^2 faces from a 4 * faces x 2 * faces RGBA16F panorama, full prefiltered chain.
Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50); ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", default="3840x2160"); ap.add_argument("--faces", type=int, default=512)
    a = ap.parse_args()
    import numpy as np
    import torch
    from basicrenderer_amd import Scene, capi
    from basicrenderer_amd import environment as E
    from basicrenderer_amd.renderer import VisibilityRenderer
    W, H = (int(x) for x in a.size.lower().split("x"))
    out = {"size": [W, H], "faces": a.faces}

    def timed(fn, n):
        """median over the repeats of (ms per call) of n calls between two events"""
        res = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record(); torch.cuda.synchronize()
            res.append(e0.elapsed_time(e1) / n)
        return round(statistics.median(res), 5)

    # ---- the build at faces^2
    n = a.faces
    lib = capi.brmi_lib()
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    rng = np.random.default_rng(1)
    pano = np.concatenate([rng.uniform(0, 4, size=(2 * n, 4 * n, 3)), np.ones((2 * n, 4 * n, 1))], -1).astype(np.float16)
    t_src = up(pano)
    d_src = up(E.descriptor_words(t_src.data_ptr(), 4 * n, 2 * n, 1, capi.TEXTURE_FORMAT_RGBA16_FLOAT))
    t_cube = torch.zeros(6 * n * n * 8, dtype=torch.uint8, device=dev)
    d_cube = up(np.stack([E.descriptor_words(t_cube.data_ptr() + f * n * n * 8, n, n, 1, capi.TEXTURE_FORMAT_RGBA16_FLOAT) for f in range(6)]))
    levels = min(16, int(np.log2(n)) + 1)
    per = E.chain_texels(n, levels)
    t_chain = torch.zeros(6 * per * 4, dtype=torch.uint8, device=dev)
    d_chain = up(np.stack([E.descriptor_words(t_chain.data_ptr() + f * per * 4, n, n, levels, capi.TEXTURE_FORMAT_RGBA8_UNORM) for f in range(6)]))
    t_info = up(np.zeros(32, dtype=np.uint32))
    s = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    stages = {"convert": lambda: lib.brmi_env_convert(d_src.data_ptr(), d_cube.data_ptr(), n, capi.TEXTURE_FORMAT_RGBA16_FLOAT, s()),
              "project_sh": lambda: lib.brmi_env_project_sh(d_cube.data_ptr(), 1, t_info.data_ptr(), 1, 0, n, s()),
              "prefilter": lambda: lib.brmi_env_prefilter(d_cube.data_ptr(), d_chain.data_ptr(), n, levels, capi.TEXTURE_FORMAT_RGBA8_UNORM, s())}
    for name, fn in stages.items():
        assert fn() == 0
        torch.cuda.synchronize()
        out["build_" + name + "_ms"] = timed(fn, 10)
    out["build_levels"] = levels

    # ---- the sky on the headline frame
    sc = Scene("bistro", W, H, point_lights=256, directional=True, unique_budget=True, lod_builder="own", relief_slope=1.5)
    env = E.Environment.procedural(64)
    r = VisibilityRenderer(sc, occlusion=True)
    for skybox in (False, True):
        r.set_environment(env, skybox=skybox)
        for _ in range(5):
            r.execute()
        torch.cuda.synchronize()
        out["frame_ms_skybox_%s" % ("on" if skybox else "off")] = timed(r.execute, a.frames)
    depth = r.depth().view(np.uint32)
    out["empty_pixel_share"] = round(float((depth == 0x7F7FFFFF).mean()), 5)
    sky = lambda: r.stage("skybox")
    out["skybox_stage_ms"] = timed(sky, a.frames)
    # half sky: the upper half of the tiled depth plane (whole tile rows) set to "empty"
    d = r.res[capi.RES["LINEAR_DEPTH"]].view(torch.int32)
    tiles_x, tile_rows = (W + 7) // 8, (H + 7) // 8
    d[: (tile_rows // 2) * tiles_x * 64] = 0x7F7FFFFF
    torch.cuda.synchronize()
    out["skybox_stage_half_sky_ms"] = timed(sky, a.frames)
    r.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
