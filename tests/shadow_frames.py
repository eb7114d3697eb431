"""The frame cases of the shadow tests (TEST INFRASTRUCTURE): scenes, the two shadowed lights of each, their light-view maps rendered by the CPU oracle from
the light's own cameras, the receivers of a frame (world position and shading normal per covered pixel, float64, from the oracle's depth and G-buffer the way
shade_pixel derives them) and, from the restatement alone, each pixel's shadow decision for both lights with its fragile flag.

tests/test_shadow_cpu.py judges the cases with this (fragile share, lit / shadowed shares); tests/test_shadow_gpu.py selects each pixel's candidate with it."""
import functools

import numpy as np

import orc
import shadow_cases as cases
import shadow_ref as ref
from basicrenderer_amd import shadows as sh

SPOT_RES, FACE_RES = 128, 64
MIN_N_DOT_V = 1e-4      # BRMI_MIN_N_DOT_V
# name -> (preset, W, H, kwargs, (spot light, point light)): the lights are picked so that each case meets test_shadow_cpu's conditions
FRAME_SCENES = {
    "tiny": ("tiny", 256, 144, dict(point_lights=6, spot_every=2), (4, 1)),
    "sponza": ("sponza", 320, 180, dict(point_lights=32, size_scale=0.15, spot_every=2, material_features=3), (24, 7)),
}
# The generator hangs its lights a short range (3.2) above the surfaces they light, so in the Sponza-class frame nothing stands between a light and the pixels
# it reaches.  The two shadowed lights of that scene are therefore raised (first number) and given (second number) x the range (intensity x RANGE_SCALE^2, far plane and
# bounding sphere to match): columns and arches then stand in their light.
# Both scenes' shadowed lights get NEAR as their near plane instead of the generator's 0.01: unprojectDepth turns an fp32 rounding of the map value into z^2 / near
# roundings of depth, and the spot / point tests compare clip z = far (z - near) / (far - near) with the view depth, which puts every lit surface within
# ~near of the threshold -- at 0.01 most decisions of a frame would sit inside any honest margin.
RETUNE = {"tiny": (0.0, 1.0, 0.1), "sponza": (1.0, 4.0, 0.2)}


def _retune(rec, li, raise_y, scale, near):
    l = rec[li]
    l["posWorldSpace"][1] += np.float32(raise_y)
    R = float(l["maxRange"]) * scale
    l["maxRange"], l["farPlane"], l["nearPlane"] = R, R, near
    l["color"][3] *= np.float32(scale * scale)
    if int(l["type"]) == sh.LIGHT_SPOT:      # ComputeConeBoundingSphere(origin, direction, height = maxRange, halfAngle = outer), as the generator has it
        r = R * np.tan(np.arccos(float(l["outerConeAngle"])))
        l["boundingSphere"][:3] = l["posWorldSpace"][:3] + l["dirWorldSpace"][:3] * np.float32(0.5 * R)
        l["boundingSphere"][3] = np.sqrt(R * R + r * r)
    else:
        l["boundingSphere"][:3], l["boundingSphere"][3] = l["posWorldSpace"][:3], R


@functools.lru_cache(maxsize=None)
def scene(name):
    from conftest import Scene
    preset, W, H, kw, lights = FRAME_SCENES[name]
    sc = Scene(preset, W, H, **kw)
    if name in RETUNE:
        rec = sc.arrays["lights"].view(sh.LIGHT_DTYPE)
        for li in lights:
            _retune(rec, li, *RETUNE[name])
    return sc


def shadowed_lights(name):
    return FRAME_SCENES[name][4]


def light_records(sc):
    return sc.arrays["lights"].view(sh.LIGHT_DTYPE)


@functools.lru_cache(maxsize=None)
def oracle_maps(name):
    """[spot map, six point faces]: the oracle's linear depth from each light camera through the capture conversion (bit-exact with the kernels' maps), and the
    views' camera records."""
    sc = scene(name)
    rec = light_records(sc)
    maps, cams = [], []
    for li, res in zip(shadowed_lights(name), (SPOT_RES, FACE_RES)):
        l = rec[li]
        for cam, cull in sh.light_views(l, res):
            o = orc.OracleFrame(sc.light_view(cam, cull, res))
            o.cull(); o.raster()
            maps.append(ref.capture_depth(o.depth_copy(), float(l["nearPlane"]), float(l["farPlane"])))
            cams.append(cam)
    return maps, cams


@functools.lru_cache(maxsize=None)
def oracle_frame(name):
    """The oracle's frame up to the light grid (what no candidate changes)."""
    o = orc.OracleFrame(scene(name))
    o.cull(); o.raster(); o.depth_copy(); o.gbuffer(); o.light_cluster()
    return o


def candidates(name, clustered):
    """The oracle's four frames: [neither, spot only, point only, both] of the two shadowed lights with intensity 0 (index = spot shadowed | point shadowed << 1)."""
    sc, o = scene(name), oracle_frame(name)
    rec = light_records(sc)
    spot, point = shadowed_lights(name)
    keep = rec["color"].copy()
    out = []
    try:
        for k in range(4):
            rec["color"][:] = keep
            if k & 1:
                rec["color"][spot, 3] = 0.0
            if k & 2:
                rec["color"][point, 3] = 0.0
            out.append(o.shade(clustered=bool(clustered)).copy())
    finally:
        rec["color"][:] = keep
    return out


@functools.lru_cache(maxsize=None)
def receivers(name):
    """(covered mask, posWS [n, 3], shading normal [n, 3]) in float64: shade_pixel's own derivation -- clip position from the pixel centre, the camera's
    projectionInverse scaled by the linear depth, viewInverse; N = normalize(n + max(0, MIN_N_DOT_V - n.V) V) with V towards the eye."""
    sc, o = scene(name), oracle_frame(name)
    c = sc.arrays["cameras"].view(np.float32)[:184].astype(np.float64)
    inv_proj, view_inv, eye = c[52:68].reshape(4, 4), c[20:36].reshape(4, 4), c[0:3]
    H, W = o.depth.shape
    covered = o.depth.view(np.uint32) != ref.EMPTY_DEPTH_BITS
    py, px = np.nonzero(covered)
    u = (px.astype(np.float32) + np.float32(0.5)) / np.float32(W)
    v = np.float32(1.0) - (py.astype(np.float32) + np.float32(0.5)) / np.float32(H)
    clip = np.stack([u.astype(np.float64) * 2 - 1, v.astype(np.float64) * 2 - 1, np.ones(len(px)), np.ones(len(px))], 1)
    pvs = (clip @ inv_proj)[:, :3] * o.depth[covered].astype(np.float64)[:, None]
    pos = np.concatenate([pvs, np.ones((len(px), 1))], 1) @ view_inv
    pos = pos[:, :3]
    V = eye - pos
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    n = o.normals[covered][:, :3].astype(np.float64)
    ndv = np.sum(n * V, axis=1)
    N = n + np.maximum(0.0, -ndv + MIN_N_DOT_V)[:, None] * V
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    return covered, pos, N


def decisions(name, maps=None, dt=np.float64):
    """Per covered pixel: (spot result dict, point result dict) of the restatement with `maps` (default: the oracle's)."""
    sc = scene(name)
    rec = light_records(sc)
    spot, point = shadowed_lights(name)
    omaps, cams = oracle_maps(name)
    maps = omaps if maps is None else maps
    _, pos, N = receivers(name)
    ls, lp = rec[spot], rec[point]
    rs = ref.spot_shadow(pos, N, ls["dirWorldSpace"][:3], float(ls["nearPlane"]), float(ls["farPlane"]), cases.view_projection(cams[0]), maps[0], dt)
    rp = ref.point_shadow(pos, N, lp["posWorldSpace"], float(lp["nearPlane"]), float(lp["farPlane"]), [cases.view_projection(c) for c in cams[1:7]], maps[1:7], dt)
    return rs, rp


@functools.lru_cache(maxsize=None)
def frame_margin():
    """The margin of shadow_cases.margin() with the frames' own receivers taken in: 4 x the largest fp32 - float64 difference over every input the tests use.
    A frame's receivers are the pixels the light reaches: beyond its range no decision is taken (and unprojectDepth's error grows with z^2 / near)."""
    worst = cases.margin()[0]
    for name in FRAME_SCENES:
        (s32, p32), (s64, p64) = decisions(name, dt=np.float32), decisions(name, dt=np.float64)
        reach_s, reach_p = reached(name, 1)
        pick = lambda r, m: {k: v[m] for k, v in r.items()}
        worst = max(worst, ref.measured_difference(pick(s32, reach_s), pick(s64, reach_s)),
                    ref.measured_difference(pick(p32, reach_p), pick(p64, reach_p), discrete=("face", "cam", "early")))
    return worst, 4.0 * worst


def reached(name, clustered):
    """Per covered pixel: does the spot / the point light change the oracle's unshadowed frame there (the pixels the light reaches)?"""
    covered = receivers(name)[0]
    c = candidates(name, clustered)
    return (c[0] != c[1])[covered], (c[0] != c[2])[covered]


def judged(name, clustered, margin, maps=None):
    """Per covered pixel: (spot shadowed, point shadowed, fragile).  A pixel is fragile when a light that reaches it has a fragile decision there; where a light
    does not reach a pixel its candidates are the same frame, so its decision there selects nothing."""
    rs, rp = decisions(name, maps)
    reach_s, reach_p = reached(name, clustered)
    fragile = (reach_s & ref.spot_fragile(rs, margin)) | (reach_p & ref.point_fragile(rp, margin))
    return rs["shadow"] != 0, rp["shadow"] != 0, fragile, reach_s, reach_p
