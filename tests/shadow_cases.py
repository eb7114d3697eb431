"""The made-up inputs of the shadow tests (tests/test_shadow_cpu.py decides on the CPU that they are fit to judge with, tests/test_shadow_gpu.py runs the
kernels on them): synthetic maps -- a plane, a step, a plane inside a border of 1.0 -- and receivers at a spread of offsets around them, few of them near zero.
Everything is derived from the `tiny` scene's first spot and first point light and the light views basicrenderer_amd.shadows makes for them."""
import functools

import numpy as np

import shadow_ref as ref
from basicrenderer_amd import shadows as sh

SPOT_SIZES = [(64, 64), (50, 36)]      # (width, height) of the spot maps
CUBE_RES = 32
MAP_KINDS = ["plane", "step", "border"]


@functools.lru_cache(maxsize=None)
def scene():
    from conftest import Scene
    return Scene("tiny", 256, 144, point_lights=6, spot_every=2)


@functools.lru_cache(maxsize=None)
def lights():
    """(records, index of the first spot light, index of the first point light)"""
    rec = scene().arrays["lights"].view(sh.LIGHT_DTYPE).copy()
    spot = int(np.flatnonzero(rec["type"] == sh.LIGHT_SPOT)[0])
    point = int(np.flatnonzero(rec["type"] == sh.LIGHT_POINT)[0])
    return rec, spot, point


def camera_floats(cam_bytes):
    return np.frombuffer(bytes(cam_bytes), dtype=np.float32)


def view_projection(cam_bytes):
    return camera_floats(cam_bytes)[68:84].reshape(4, 4).copy()


def plane_depth(light):
    return min(3.0, 0.3 * float(light["farPlane"]))


def synthetic_map(kind, w, h, light):
    near, far, z0 = float(light["nearPlane"]), float(light["farPlane"]), plane_depth(light)
    d0 = ref.capture_depth(np.float32(z0), near, far)
    m = np.full((h, w), d0, dtype=np.float32)
    if kind == "step":
        m[:, w // 2:] = ref.capture_depth(np.float32(1.6 * z0), near, far)
    if kind == "border":
        m[:3], m[-3:], m[:, :3], m[:, -3:] = 1.0, 1.0, 1.0, 1.0
    return m


def _offsets(rng, n):
    off = rng.uniform(-0.6, 0.6, n)
    off[:8] = rng.uniform(-1e-3, 1e-3, 8)      # the few near the surface
    return off


@functools.lru_cache(maxsize=None)
def spot_case():
    """dict(light, camera, vp, pos, nrm): 2048 receivers in and around the spot light's frustum, 64 of them behind the light."""
    rec, spot, _ = lights()
    l = rec[spot]
    cam, _cull = sh.light_views(l, 64)[0]
    c = camera_floats(cam)
    world = c[20:36].reshape(4, 4).astype(np.float64)
    fov = float(c[172])
    rng = np.random.default_rng(1234)
    n = 2048
    z = plane_depth(l) * (1.0 + _offsets(rng, n))
    z[-64:] = -z[-64:]                                        # behind the light
    ndc = rng.uniform(-1.3, 1.3, (n, 2))                      # some project outside the map
    t = np.tan(0.5 * fov)
    pv = np.stack([ndc[:, 0] * z * t, ndc[:, 1] * z * t, -z, np.ones(n)], 1)
    pos = (pv @ world)[:, :3].astype(np.float32)
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return dict(light=l, index=spot, camera=cam, vp=view_projection(cam), pos=pos, nrm=nrm.astype(np.float32))


@functools.lru_cache(maxsize=None)
def point_case():
    """dict(light, cameras, vps, pos, nrm): 2048 receivers around the point light, 16 of them exactly on cube face edges."""
    rec, _, point = lights()
    l = rec[point]
    views = sh.light_views(l, CUBE_RES)
    rng = np.random.default_rng(4321)
    n = 2048
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    e = rng.uniform(0.1, 0.9, 16)
    d[-16:] = np.stack([np.ones(16), np.where(np.arange(16) % 2 == 0, 1.0, -1.0), e], 1)[:, [[0, 1, 2], [2, 0, 1], [1, 2, 0], [0, 1, 2]][0]]
    d[-8:] = d[-8:][:, [2, 0, 1]]                             # edges between other pairs of faces
    depth = plane_depth(l) * (1.0 + _offsets(rng, n))         # along the major axis: what the face's camera sees as view depth
    pos = np.asarray(l["posWorldSpace"][:3], dtype=np.float64) + d * (depth / np.max(np.abs(d), axis=1))[:, None]
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return dict(light=l, index=point, cameras=[v[0] for v in views], vps=[view_projection(v[0]) for v in views], pos=pos.astype(np.float32), nrm=nrm.astype(np.float32))


def cube_maps(kind, light):
    faces = [synthetic_map("plane" if kind == "step" else kind, CUBE_RES, CUBE_RES, light) for _ in range(6)]
    if kind == "step":      # three faces further away
        far = ref.capture_depth(np.float32(1.6 * plane_depth(light)), float(light["nearPlane"]), float(light["farPlane"]))
        for f in (1, 3, 5):
            faces[f][:] = far
    return faces


def spot_results(kind, size, dt):
    c = spot_case()
    l = c["light"]
    m = synthetic_map(kind, size[0], size[1], l)
    return ref.spot_shadow(c["pos"], c["nrm"], l["dirWorldSpace"][:3], float(l["nearPlane"]), float(l["farPlane"]), c["vp"], m, dt)


def point_results(kind, dt):
    c = point_case()
    l = c["light"]
    return ref.point_shadow(c["pos"], c["nrm"], l["posWorldSpace"], float(l["nearPlane"]), float(l["farPlane"]), c["vps"], cube_maps(kind, l), dt)


@functools.lru_cache(maxsize=None)
def margin():
    """(measured, margin): the largest |fp32 - float64| of currentDepth - bias - closestDepth over every made-up input set, and 4 x that (the rule of
    profiles/display_accuracy.md; the figures are recorded in profiles/shadow_accuracy.md)."""
    worst = 0.0
    for kind in MAP_KINDS:
        for size in SPOT_SIZES:
            worst = max(worst, ref.measured_difference(spot_results(kind, size, np.float32), spot_results(kind, size, np.float64)))
        worst = max(worst, ref.measured_difference(point_results(kind, np.float32), point_results(kind, np.float64), discrete=("face", "cam", "early")))
    return worst, 4.0 * worst
