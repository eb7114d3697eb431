"""numpy restatement of the debug views (TEST INFRASTRUCTURE): the payload perFrame.outputType asks for and its resolve to colour.

Written from the shader text -- BR/shaders/gbuffer.hlsl:63-111, deferred.hlsl:65-103, Include/debugPayload.hlsli, Include/lighting.hlsli:166-196 and
:502-511, PostProcessing/debugResolve.hlsl:50-106 -- on UNTILED planes, independently of basicrenderer_amd/csrc/brmi_debugview.hip.  The one
definition that is the project's own: the material modes pack what the G-buffer planes hold, not the material inputs in front of them.

A `frame` is a dict of arrays: vis [H,W] u64, clusters [n,4] u32, depth [H,W] f32, normals [H,W,4] f32, albedo / mr / motion [H,W] u32,
emissive [H,W] u64, light_clusters [m,12] u32, camera and per_frame (the bytes of brmi_camera / brmi_per_frame); optionally tri_counts [n], the
triangle count of every listed cluster (tri_counts_from_oracle).
"""
import ctypes as C

import numpy as np

MODES = {"NORMAL": 1, "ALBEDO": 2, "METALLIC": 3, "ROUGHNESS": 4, "EMISSIVE": 5, "AO": 6, "DEPTH": 7, "MESHLETS": 10, "LIGHT_CLUSTER_ID": 12,
         "LIGHT_CLUSTER_LIGHT_COUNT": 13, "MOTION_VECTORS": 14, "GEOMETRY_GROUP": 35}
HASHED = (10, 12, 13, 35)
SENTINEL = 0xFFFFFFFF
DEPTH_EMPTY_BITS = 0x7F7FFFFF
VIS_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
f32 = np.float32


def frame_of(o, scene):
    """The frame dict of an orc.OracleFrame that has run, or of anything with the same attributes."""
    return dict(vis=o.vis, clusters=o.clusters[: o.count], depth=o.depth, normals=o.normals, albedo=o.albedo, emissive=o.emissive, mr=o.mr, motion=o.motion,
                light_clusters=o.light_clusters, camera=scene.arrays["cameras"], per_frame=scene.arrays["perFrame"])


def frame_of_renderer(r, camera=None, per_frame=None):
    """The same from a VisibilityRenderer's read-back surfaces (camera: the bytes the frame was rendered with, default the scene's)."""
    g = r.gbuffer()
    return dict(vis=r.visibility(), clusters=r.visible_clusters(), depth=r.depth(), normals=g["normals"], albedo=g["albedo"], emissive=g["emissive"], mr=g["mr"],
                motion=g["motion"], light_clusters=r.light_clusters()[0], camera=r.scene.arrays["cameras"] if camera is None else camera,
                per_frame=r.scene.arrays["perFrame"] if per_frame is None else per_frame)


def half_bits(x):
    """f32tof16: round to nearest even (numpy's float16 conversion)."""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=f32).astype(np.float16).view(np.uint16).astype(np.uint32)


def pack_float3(x, y, z):
    """PackDebugFloat3: (f16(x) | f16(y) << 16, f16(z))."""
    return np.stack([half_bits(x) | (half_bits(y) << np.uint32(16)), half_bits(z)], axis=-1)


def pack_uint(v):
    """PackDebugUint: (v, 0)."""
    v = np.asarray(v, dtype=np.uint32)
    return np.stack([v, np.zeros_like(v)], axis=-1)


def tri_counts_from_oracle(scene, clusters):
    """Triangle count of every cluster of the list, asked of the oracle's G-buffer pass (which leaves a pixel alone when its key names a triangle the
    cluster does not have): an image whose pixel k holds the key (cluster k / 128, triangle k % 128)."""
    import orc
    clusters = np.asarray(clusters, dtype=np.uint32).reshape(-1, 4)
    n, (W, H) = len(clusters), (scene.width, scene.height)
    counts = np.zeros(n, dtype=np.uint32)
    depth_bits = np.uint64(int(f32(1.0).view(np.uint32)) >> 1)
    per = (W * H) // 128      # clusters per probe image
    for first in range(0, n, per):
        m = min(per, n - first)
        k = np.arange(m * 128, dtype=np.uint64)
        vis = np.full(W * H, VIS_EMPTY, dtype=np.uint64)
        vis[: m * 128] = (depth_bits << np.uint64(33)) | (((k >> np.uint64(7)) + np.uint64(first)) << np.uint64(7)) | (k & np.uint64(127))
        o = orc.OracleFrame(scene)
        o.clusters[:n], o.count, o.vis = clusters, n, vis.reshape(H, W)
        o.gbuffer()
        written = ((o.normals.view(np.uint32).reshape(-1, 4) != 0).any(axis=1) | (o.albedo.reshape(-1) != 0))[: m * 128].reshape(m, 128)
        counts[first: first + m] = written.sum(axis=1)
        assert all(written[i, : counts[first + i]].all() for i in range(m))      # the written triangles are 0 .. count - 1
    return counts


def key_fields(frame):
    """(valid, cluster index, record) per pixel: a key is empty when it is the clear value, names no cluster of the frame's list or -- where the frame
    carries tri_counts -- no triangle of its cluster (clodResolveCommon's bounds checks, as k_gbuffer has them)."""
    vis, clusters = frame["vis"], np.asarray(frame["clusters"], dtype=np.uint32).reshape(-1, 4)
    ci = ((vis >> np.uint64(7)) & np.uint64(0x3FFFFFF)).astype(np.int64)
    valid = (vis != VIS_EMPTY) & (ci < len(clusters))
    if frame.get("tri_counts") is not None:
        tri = (vis & np.uint64(0x7F)).astype(np.int64)
        valid &= tri < np.asarray(frame["tri_counts"], dtype=np.int64)[np.where(valid, ci, 0)]
    rec = clusters[np.where(valid, ci, 0)] if len(clusters) else np.zeros(vis.shape + (4,), dtype=np.uint32)
    return valid, ci, rec


def view_depth(frame):
    """|positionVS.z| as deferred.hlsl:43-46 has it: clipPos = (uv * 2 - 1, 1, 1) with uv.y flipped, mul(clipPos, projectionInverse).z * depth, all fp32."""
    cam, pf = np.frombuffer(bytes(frame["camera"]), dtype=f32), np.frombuffer(bytes(frame["per_frame"]), dtype=np.uint32)
    ip = cam[52:68].reshape(4, 4)      # brmi_camera::projectionInverse
    H, W = frame["depth"].shape
    px, py = np.arange(W, dtype=f32)[None, :], np.arange(H, dtype=f32)[:, None]
    uvx = (px + f32(0.5)) / f32(pf[13])
    uvy = f32(1.0) - (py + f32(0.5)) / f32(pf[14])
    cx, cy = uvx * f32(2.0) - f32(1.0), uvy * f32(2.0) - f32(1.0)
    vz = ((cx * ip[0, 2] + cy * ip[1, 2]) + f32(1.0) * ip[2, 2]) + f32(1.0) * ip[3, 2]
    return np.abs((vz * frame["depth"]).astype(f32))


def light_cluster_ids(frame):
    """ComputeClusterID (lighting.hlsli:166-196): (tile x, tile y, slice) per pixel; the slice through the oracle's orc_cluster_slice hook, and -- like the
    table of slice starts the library looks it up in -- never beyond gridZ, the first slice behind the grid."""
    import orc
    cam, pf = np.frombuffer(bytes(frame["camera"]), dtype=f32), np.frombuffer(bytes(frame["per_frame"]), dtype=np.uint32)
    gx, gy, gz, near = int(pf[15]), int(pf[16]), int(pf[17]), int(pf[18])
    z_split = float(np.frombuffer(bytes(frame["per_frame"]), dtype=f32)[19])
    H, W = frame["depth"].shape
    tsx, tsy = f32(pf[13]) / f32(gx), f32(pf[14]) / f32(gy)
    tx = (np.arange(W, dtype=f32) / tsx).astype(np.uint32)[None, :].repeat(H, 0)
    ty = (np.arange(H, dtype=f32) / tsy).astype(np.uint32)[:, None].repeat(W, 1)
    z = np.ascontiguousarray(view_depth(frame).reshape(-1))
    out = np.zeros(z.size, dtype=np.uint32)
    fn = orc.lib().orc_cluster_slice
    fn.argtypes = [C.c_void_p, C.c_uint64, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p]
    fn(z.ctypes.data, z.size, float(cam[174]), float(cam[175]), z_split, near, gz, out.ctypes.data)
    return tx, ty, np.minimum(out, np.uint32(gz)).reshape(H, W), (gx, gy, gz)


def payload(mode, frame):
    """[H, W, 2] uint32: the debug payload of `mode` for every pixel, the sentinel where the pixel has no geometry."""
    mode = MODES[mode.upper()] if isinstance(mode, str) else int(mode)
    if mode not in MODES.values():
        raise ValueError(f"outputType {mode} is not a debug view of this path")
    depth = frame["depth"]
    if mode in (10, 35):
        covered, _, rec = key_fields(frame)
        if mode == 10:
            out = pack_uint(rec[..., 1] & np.uint32(0x3FFF))                                                                      # localMeshlet
        else:
            out = pack_uint(((rec[..., 1] >> np.uint32(14)) & np.uint32(0x3FFFF)) | ((rec[..., 2] & np.uint32(3)) << np.uint32(18)))   # group id, 20 bits
    else:
        covered = depth.view(np.uint32) != np.uint32(DEPTH_EMPTY_BITS)
        half, tenth = f32(0.5), f32(0.1)
        unorm = lambda w, shift: ((w >> np.uint32(shift)) & np.uint32(0xFF)).astype(f32) / f32(255.0)      # noqa: E731
        if mode == 1:
            n = frame["normals"].astype(f32)
            out = pack_float3(n[..., 0] * half + half, n[..., 1] * half + half, n[..., 2] * half + half)
        elif mode == 2:
            out = pack_float3(unorm(frame["albedo"], 0), unorm(frame["albedo"], 8), unorm(frame["albedo"], 16))
        elif mode in (3, 4):
            v = unorm(frame["mr"], 0 if mode == 3 else 8)
            out = pack_float3(v, v, v)
        elif mode == 5:
            e = np.ascontiguousarray(frame["emissive"]).view(np.float16).reshape(depth.shape + (4,)).astype(f32)
            out = pack_float3(e[..., 0], e[..., 1], e[..., 2])
        elif mode == 6:
            v = unorm(frame["albedo"], 24)
            out = pack_float3(v, v, v)
        elif mode == 7:
            v = np.abs(depth).astype(f32) * tenth
            out = pack_float3(v, v, v)
        elif mode == 14:
            mv = np.ascontiguousarray(frame["motion"]).view(np.float16).reshape(depth.shape + (2,)).astype(f32)
            out = pack_float3(mv[..., 0] * half + half, mv[..., 1] * half + half, np.full(depth.shape, half, dtype=f32))
        else:
            tx, ty, sl, (gx, gy, gz) = light_cluster_ids(frame)
            if mode == 12:
                out = pack_uint(sl)      # lighting.hlsli:509 overwrites clusterIndex with clusterID.z
            else:
                ci = (tx.astype(f32) + ty.astype(f32) * f32(gx) + sl.astype(f32) * f32(gx) * f32(gy)).astype(np.int64)
                lc = np.asarray(frame["light_clusters"], dtype=np.uint32).reshape(-1, 12)
                inside = ci < gx * gy * gz
                out = pack_uint(np.where(inside, lc[np.where(inside, ci, 0), 8], 0))      # brmi_light_cluster::numLights
    out = np.array(out, dtype=np.uint32)
    out[~covered] = SENTINEL
    return out


def hash_to_color_codes(v):
    """HashToColor's three 8-bit channels (debugPayload.hlsli:70-82), 32-bit wrap-around arithmetic."""
    h = np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    m, mask = np.uint64(0x45D9F3B), np.uint64(0xFFFFFFFF)
    h = (((h >> np.uint64(16)) ^ h) * m) & mask
    h = (((h >> np.uint64(16)) ^ h) * m) & mask
    h = (h >> np.uint64(16)) ^ h
    return np.stack([h & np.uint64(0xFF), (h >> np.uint64(8)) & np.uint64(0xFF), (h >> np.uint64(16)) & np.uint64(0xFF)], axis=-1).astype(np.uint32)


def resolve_values(mode, pay):
    """(written [H,W] bool, x [H,W,3] float64): sat(LinearToSRGB(colour)) * 255 + 0.5 before the conversion to an integer; NaN where the colour is NaN."""
    mode = MODES[mode.upper()] if isinstance(mode, str) else int(mode)
    pay = np.asarray(pay, dtype=np.uint32)
    written = ~((pay[..., 0] == SENTINEL) & (pay[..., 1] == SENTINEL))
    if mode in HASHED:
        c = hash_to_color_codes(pay[..., 0]).astype(np.float64) / 255.0
    else:
        halves = np.stack([pay[..., 0] & np.uint32(0xFFFF), pay[..., 0] >> np.uint32(16), pay[..., 1] & np.uint32(0xFFFF)], axis=-1).astype(np.uint16)
        c = halves.view(np.float16).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.power(c, np.float64(f32(1.0 / 2.2)))      # pow(c, 1 / 2.2) with the shader's fp32 exponent; negative -> NaN
    x = np.clip(s, 0.0, 1.0) * 255.0 + 0.5               # (clip keeps NaN)
    return written, x


def resolve(mode, pay, background=None):
    """[H, W, 4] uint8 in float64: the resolved image; sentinel pixels keep `background` (zeros without one).  A negative or NaN channel stores 0."""
    written, x = resolve_values(mode, pay)
    codes = np.where(np.isnan(x), 0.0, np.floor(x)).astype(np.uint8)
    out = np.zeros(pay.shape[:2] + (4,), dtype=np.uint8) if background is None else np.array(background, dtype=np.uint8, copy=True)
    out[written, :3] = codes[written]
    out[written, 3] = 255
    return out
