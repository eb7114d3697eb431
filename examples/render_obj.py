#!/usr/bin/env python3
"""Render a Wavefront OBJ or a glTF 2.0 file (.gltf / .glb) through the whole path on an MI355X and write the lit frame as a PNG
(Reinhard + sRGB), or -- with --tonemap -- the RGBA8 picture of the library's display chain (auto-exposure, bloom, tone mapping).

    python examples/render_obj.py model.obj|scene.glb out.png [--size 1920x1080] [--lights 32] [--features 0] [--environment sky] [--gtao] [--shadows] [--view NAME]
                                  [--tonemap reinhard|neutral|aces|lpm|none] [--bloom] [--exposure-frames 8] [--taa N]

--view NAME writes a debug view of the frame instead (perFrame.outputType: normal, albedo, metallic, roughness, emissive, ao, depth, meshlets,
geometry_group, light_cluster_id, light_cluster_light_count, motion_vectors); pixels without geometry are black.
"""
import argparse
import os
import struct
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_png(path, rgb8):
    h, w, _ = rgb8.shape
    raw = b"".join(b"\x00" + rgb8[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("obj"); ap.add_argument("png")
    ap.add_argument("--size", default="1920x1080"); ap.add_argument("--lights", type=int, default=32); ap.add_argument("--features", type=int, default=0)
    ap.add_argument("--anisotropy", type=int, default=0, metavar="N", help="maxAnisotropy of every sampler, 1..16 (default: off, the isotropic sampler)")
    ap.add_argument("--environment", default=None, metavar="sky|FILE.hdr", help="image-based lighting from the procedural environment `sky` or from a Radiance .hdr panorama, built on the GPU (default: off, punctual lights only)")
    ap.add_argument("--skybox", action="store_true", help="show the environment behind the model (pixels without geometry)")
    ap.add_argument("--gtao", nargs="?", const="high", default=None, metavar="QUALITY", help="screen-space ambient occlusion (XeGTAO) in the environment term: low, medium, high (default) or ultra; "
                    "`--gtao --view ao` shows the visibility the shading takes")
    ap.add_argument("--view", default=None, metavar="NAME", help="write this debug view (e.g. meshlets) instead of the tone-mapped frame")
    ap.add_argument("--tonemap", default=None, choices=["reinhard", "neutral", "aces", "lpm", "none"], help="write the RGBA8 of the library's display chain with this curve (default: off, the file as before)")
    ap.add_argument("--bloom", action="store_true", help="with --tonemap: the bloom pyramid blended into the frame (both sides of the frame at least 32 pixels)")
    ap.add_argument("--exposure-frames", type=int, default=8, metavar="N", help="with --tonemap: render N frames, the last N - 2 with time coefficient 1, so the auto-exposure has settled")
    ap.add_argument("--taa", type=int, default=0, metavar="N", help="temporal anti-aliasing: render N jittered frames of the still camera and write the last resolved one (with --tonemap: through the display chain)")
    ap.add_argument("--shadows", action="store_true", help="shadow maps for every spot and point light of the scene (rendered once, from each light's own views)")
    ap.add_argument("--shadow-size", type=int, default=1024, metavar="N", help="with --shadows: a spot map is N x N, a cube face N/2 x N/2")
    ap.add_argument("--procedural-materials", action="store_true", help="a glTF file's own materials and textures are used by default; this keeps the procedural stand-ins (--features)")
    a = ap.parse_args()
    from basicrenderer_amd import Scene
    from basicrenderer_amd.obj import frame_view, load_obj
    from basicrenderer_amd.renderer import VisibilityRenderer
    w, h = (int(x) for x in a.size.lower().split("x"))
    if a.obj.lower().endswith((".gltf", ".glb")):
        from basicrenderer_amd import gltf
        meshes, instances = gltf.load_gltf(a.obj)
        view = gltf.frame_view(meshes, instances)
        materials = None if a.procedural_materials else gltf.load_gltf_materials(a.obj)
    else:
        materials = None
        meshes = load_obj(a.obj)
        instances, view = [(k, np.eye(4, dtype=np.float32)) for k in range(len(meshes))], frame_view(meshes)
    sc = Scene(width=w, height=h, point_lights=a.lights, material_features=a.features, meshes=meshes, instances=instances, view=view, materials=materials)
    r = VisibilityRenderer(sc, occlusion=True)
    if a.anisotropy > 0:
        r.set_anisotropy(a.anisotropy)
    if a.environment == "sky":
        from basicrenderer_amd.environment import Environment
        r.set_environment(Environment.procedural(64), skybox=a.skybox)
    elif a.environment:
        from basicrenderer_amd.environment import Environment, read_hdr
        r.set_environment(Environment.from_equirect(read_hdr(a.environment)), skybox=a.skybox)
    if a.gtao:
        r.set_gtao(a.gtao)
    if a.shadows:
        from basicrenderer_amd import shadows
        kinds = sc.arrays["lights"].view(shadows.LIGHT_DTYPE)["type"]
        casters = [int(i) for i in np.flatnonzero((kinds == shadows.LIGHT_SPOT) | (kinds == shadows.LIGHT_POINT))]
        r.set_shadows(casters, resolution=a.shadow_size, point_resolution=max(32, a.shadow_size // 2))
        r.render_shadow_maps()      # a still scene: once
    if a.view:
        r.set_debug_view(a.view)
    if a.bloom and not a.tonemap:
        ap.error("--bloom needs --tonemap")
    if a.tonemap and a.view:
        ap.error("--tonemap and --view write different pictures: give one of them")
    if a.taa and a.view:
        ap.error("--taa and --view write different pictures: give one of them")
    if a.taa:
        r.set_temporal()

    def frame(k):      # with --taa: frame k's jitter; without a skybox the shading pass leaves pixels without geometry alone, so the target is cleared here
        if a.taa:
            if not a.skybox:
                r.hdr_tensor().zero_()
            r.update(k)
        r.execute()
    if a.tonemap:
        frames = max(a.exposure_frames, a.taa, 1)
        for k in range(frames):      # the first two frames bring the path's own history up; from then on the adaptation jumps to the frame's average
            r.set_display(a.tonemap, bloom=a.bloom, time_coefficient=1.0 if k >= min(2, frames - 1) else 0.0)
            frame(k)
        write_png(a.png, np.ascontiguousarray(r.ldr()[..., :3]))
        print(f"{a.obj}: {a.tonemap}{' + bloom' if a.bloom else ''}, adapted luminance {r.adapted_luminance():.4g} after {frames} frames -> {a.png}")
        return
    for k in range(max(a.taa, 2)):
        frame(k)
    if a.view:
        write_png(a.png, np.ascontiguousarray(r.debug_image()[..., :3]))
        print(f"{a.obj}: debug view {a.view} -> {a.png}")
        return
    hdr = (r.resolved_hdr() if a.taa else r.hdr()).view(np.float16).reshape(h, w, 4)[..., :3].astype(np.float32)
    ldr = hdr / (1.0 + hdr)
    srgb = np.where(ldr <= 0.0031308, 12.92 * ldr, 1.055 * np.power(np.maximum(ldr, 1e-8), 1 / 2.4) - 0.055)
    write_png(a.png, (np.clip(srgb, 0, 1) * 255 + 0.5).astype(np.uint8))
    print(f"{a.obj}: {sc.stats['uniqueTriangles']} triangles, {sc.stats['meshletsTotal']} meshlets, {sc.stats['lodLevelsMax']} LOD levels -> {a.png}")


if __name__ == "__main__":
    main()
