"""numpy restatement of the spot / point shadow path, from the shader text: BR/shaders/Include/shadows.hlsli:416-464 (calculatePointShadow),
:934-950 (calculateSpotShadow), utilities.hlsli:2807-2810 (unprojectDepth).  TEST INFRASTRUCTURE: independent of the kernels; every function takes the dtype it
computes in (float64: the reference the GPU is held to; float32: only to MEASURE how far fp32 can move the compared quantity -- the fragile margin).

A receiver is fragile when |currentDepth - bias - closestDepth| is below the margin, or when a discrete choice sits within the margin of flipping: the cube
lookup's face (its two largest |components| within the margin: faces are not filtered across), a sample within the margin of the `== 1.0` early-out without being
1.0, a spot receiver whose clip w is within the margin of 0.  The bilinear footprint itself is continuous in uv (a tap that changes carries a weight near 0; the
border value enters with weight near 0 too), so it adds no discrete choice."""
import numpy as np

EMPTY_DEPTH_BITS = 0x7F7FFFFF


def capture_depth(z, near, far):
    """brmi_shadow_capture's conversion in fp32, in its order: d = zFar * (z - zNear) / (z * (zFar - zNear)); the "empty" depth word -> 1.0."""
    z = np.asarray(z, dtype=np.float32)
    n, f = np.float32(near), np.float32(far)
    empty = z.view(np.uint32) == np.uint32(EMPTY_DEPTH_BITS)
    zz = np.where(empty, np.float32(1.0), z)
    with np.errstate(all="ignore"):
        d = (f * (zz - n)) / (zz * (f - n))
    return np.where(empty, np.float32(1.0), d.astype(np.float32))


def unproject_depth(d, near, far, dt=np.float64):
    d, n, f = np.asarray(d, dtype=dt), dt(near), dt(far)
    with np.errstate(all="ignore"):
        return n * f / (f - d * (f - n))


def bilinear(smap, u, v, border, dt=np.float64):
    """Level 0 of an R32F map at (u, v): the project's software bilinear (footprint around u * w - 0.5, a + t * (b - a) along x then y).  border: a tap outside
    the map reads 1.0; otherwise taps are clamped to the map (the cube faces' edge rule)."""
    h, w = smap.shape
    m = smap.astype(dt)
    fx, fy = np.asarray(u, dtype=dt) * dt(w) - dt(0.5), np.asarray(v, dtype=dt) * dt(h) - dt(0.5)
    x0f, y0f = np.floor(fx), np.floor(fy)
    tx, ty = fx - x0f, fy - y0f
    x0 = np.clip(np.nan_to_num(x0f, nan=0.0), -2.0 ** 31, 2.0 ** 31 - 2).astype(np.int64)
    y0 = np.clip(np.nan_to_num(y0f, nan=0.0), -2.0 ** 31, 2.0 ** 31 - 2).astype(np.int64)

    def tap(x, y):
        inside = (x >= 0) & (y >= 0) & (x < w) & (y < h)
        val = m[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
        return np.where(inside, val, dt(1.0)) if border else val
    c00, c10, c01, c11 = tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)
    a, b = c00 + tx * (c10 - c00), c01 + tx * (c11 - c01)
    return a + ty * (b - a)


def cube_face_uv(d, dt=np.float64):
    """The environment cube lookup's face and face coordinates: -> face, u, v, gap (the difference of the two largest |components|)."""
    d = np.asarray(d, dtype=dt)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    isx = (ax >= ay) & (ax >= az)
    isy = ~isx & (ay >= az)
    face = np.where(isx, np.where(x < 0, 1, 0), np.where(isy, np.where(y < 0, 3, 2), np.where(z < 0, 5, 4)))
    ma = np.where(isx, ax, np.where(isy, ay, az))
    sc = np.where(isx, np.where(x < 0, z, -z), np.where(isy, x, np.where(z < 0, -x, x)))
    tc = np.where(isx, -y, np.where(isy, np.where(y < 0, -z, z), -y))
    with np.errstate(all="ignore"):
        u, v = (sc / ma + dt(1.0)) * dt(0.5), (tc / ma + dt(1.0)) * dt(0.5)
    s = np.sort(np.stack([ax, ay, az], 1), axis=1)
    return face, u, v, s[:, 2] - s[:, 1]


def _mul_point(p, m, dt):
    p, m = np.asarray(p, dtype=dt), np.asarray(m, dtype=dt).reshape(4, 4)
    return np.stack([((p[:, 0] * m[0, c] + p[:, 1] * m[1, c]) + p[:, 2] * m[2, c]) + m[3, c] for c in range(4)], 1)


def spot_shadow(pos, nrm, light_dir, near, far, view_projection, smap, dt=np.float64):
    """calculateSpotShadow -> dict(shadow 0/1, diff = currentDepth - bias - closestDepth, w = clip w)."""
    clip = _mul_point(pos, view_projection, dt)
    with np.errstate(all="ignore"):
        u, v = clip[:, 0] / clip[:, 3], clip[:, 1] / clip[:, 3]
        u, v = u * dt(0.5) + dt(0.5), v * dt(0.5) + dt(0.5)
        v = dt(1.0) - v
        closest = unproject_depth(bilinear(smap, u, v, True, dt), near, far, dt)
        n, ld = np.asarray(nrm, dtype=dt), np.asarray(light_dir, dtype=dt)
        ndl = (n[:, 0] * ld[0] + n[:, 1] * ld[1]) + n[:, 2] * ld[2]
        bias = np.maximum(dt(0.0005), dt(0.01) * (dt(1.0) - ndl))
        diff = clip[:, 2] - bias - closest
    return dict(shadow=(clip[:, 2] - bias > closest).astype(np.float32), diff=diff, w=clip[:, 3])


def point_shadow(pos, nrm, light_pos, near, far, face_view_projections, faces, dt=np.float64):
    """calculatePointShadow -> dict(shadow, diff, gap (cube face margin), sample, early (the == 1.0 return), face).  faces: six (res, res) maps +X -X +Y -Y +Z -Z;
    face_view_projections: the six light cameras' viewProjection."""
    p, lp = np.asarray(pos, dtype=dt), np.asarray(light_pos, dtype=dt)[:3]
    l2f = p - lp
    l2f[:, 2] = -l2f[:, 2]
    with np.errstate(all="ignore"):
        wd = l2f * (dt(1.0) / np.sqrt((l2f[:, 0] * l2f[:, 0] + l2f[:, 1] * l2f[:, 1]) + l2f[:, 2] * l2f[:, 2]))[:, None]
    face, u, v, gap = cube_face_uv(wd, dt)
    sample = np.zeros(len(p), dtype=dt)
    for f in range(6):
        sel = face == f
        if sel.any():
            sample[sel] = bilinear(faces[f], u[sel], v[sel], False, dt)
    early = sample == dt(1.0)
    max_dir = np.maximum(np.maximum(np.abs(wd[:, 0]), np.abs(wd[:, 1])), np.abs(wd[:, 2]))
    cam = np.full(len(p), 0)
    chain = [(wd[:, 0] == max_dir), (wd[:, 0] == -max_dir), (wd[:, 1] == max_dir), (wd[:, 1] == -max_dir), (wd[:, 2] == max_dir), (wd[:, 2] == -max_dir)]
    for f in reversed(range(6)):
        cam = np.where(chain[f], f, cam)
    closest = unproject_depth(sample, near, far, dt)
    lsd = np.zeros(len(p), dtype=dt)
    for f in range(6):
        sel = cam == f
        if sel.any():
            lsd[sel] = _mul_point(p[sel], face_view_projections[f], dt)[:, 2]
    n = np.asarray(nrm, dtype=dt)
    ndl = (n[:, 0] * wd[:, 0] + n[:, 1] * wd[:, 1]) + n[:, 2] * wd[:, 2]
    bias = np.maximum(dt(0.0005), dt(0.02) * (dt(1.0) - ndl))
    with np.errstate(all="ignore"):
        diff = lsd - bias - closest
        shadow = np.where(early, 0.0, (lsd - bias > closest)).astype(np.float32)
    return dict(shadow=shadow, diff=diff, gap=gap, sample=sample, early=early, face=face, cam=cam)


def spot_fragile(r64, margin):
    return ~np.isfinite(r64["diff"]) | (np.abs(r64["diff"]) < margin) | (np.abs(r64["w"]) < margin)


def point_fragile(r64, margin):
    near_one = ~r64["early"] & (np.abs(r64["sample"] - 1.0) < margin)
    return ~np.isfinite(r64["diff"]) | (~r64["early"] & (np.abs(r64["diff"]) < margin)) | (r64["gap"] < margin) | near_one


def measured_difference(r32, r64, discrete=()):
    """max |fp32 - float64| of the compared quantity over the receivers whose discrete choices agree in both evaluations (the others are fragile as they stand)."""
    same = np.isfinite(r32["diff"]) & np.isfinite(r64["diff"])
    for k in discrete:
        same &= r32[k] == r64[k]
    return float(np.max(np.abs(r32["diff"][same].astype(np.float64) - r64["diff"][same]))) if same.any() else 0.0
