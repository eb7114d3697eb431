"""XeGTAO restated in numpy from the shader text (BR/shaders/GTAO.hlsl, BR/shaders/Intel/XeGTAO.hlsli, BR/include/ThirdParty/XeGTAO.h:165-202), with no call into
any library of the project.  DESIGN.md 4.12 lists the restatement decisions; the kernels (brmi_gtao.hip) were written from the same lines, separately.

  * prefilter(), edges(), denoise(): fp32 under the arithmetic contract (IEEE binary32, no contraction, correctly rounded / and sqrt, operations in the shader's
    order).  The kernels are held to them bit for bit.
  * main_pass(dtype=np.float64): exact-ish arithmetic on the fp32 inputs and the fp32 constants of the text.  It rounds to fp32 only where the definition IS an
    fp32 bit pattern: XeGTAO_FastSqrt's bit trick, and the spatio-temporal noise -- an R2 sequence evaluated in fp32 at indices up to 2 * 10^4, where the product
    keeps ten fractional bits: that quantised value is the noise, not an approximation of something finer.
    Returns per pixel the pre-rounding value saturate(v / 1.5) * 255, a `fragile` flag and `covered` (the centre is not empty).
  * main_pass(dtype=np.float32): the same statement in fp32, used only to MEASURE the margin M between an fp32 evaluation and the float64 one.

Fragile pixels: the working term is a discontinuous function of its inputs at a few decisions; a pixel within rounding distance of one may legitimately land on
either side.  The bounds are (operations upstream of the decision) x 2^-24 x (the float64 magnitudes at hand) -- counted below, not tuned:
  * a component of a tap's offset near a `round` cut (k + 0.5).  Upstream of s * omega: viewspaceZ (1), its product with NDCToViewMul_x_PixelSize (1), the
    radius quotient (1), slice + noise, / sliceCount, * pi (3), cos or sin (2, with the argument's error), * radius (1), noise + base, frac (2), step + noise,
    / steps (2), s * s (1), 1.3 / radius, + minS (2), s * omega (1): 18, taken as 24 with the rotation of the direction by the angle's error; the magnitude is
    the offset's length (an angle error moves a component by up to that) or 1.
  * with maxDepthLod > 0: the level near a k + 0.5 cut (the 24 above, a square root and a log2: 28; magnitude max(|log2 length|, 3.3)), or a texel coordinate on
    a level >= 1 near an integer ((p + 0.5) * pixelSize (2), r * pixelSize (1), + (1), * level size (1): 5, taken as 6; magnitude the coordinate or 1).
  * |dot(orthoDirectionVec, projectedNormalVec)| near 0 (its sign multiplies the normal's angle).  Upstream: the centre position (3), normalize (5), the
    view-space normal (5 + 5), orthoDirectionVec (6), axisVec (9 + 5), projectedNormalVec (8), the dot (5): 51, taken as 56; magnitudes are unit vectors: 1.
"""
import math

import numpy as np

F = np.float32
FLT_MAX = np.array([0x7F7FFFFF], dtype=np.uint32).view(np.float32)[0]      # the "empty" depth
EPS = 2.0 ** -24
N_OFFSET, N_LEVEL, N_TEXEL, N_SIGN = 24, 28, 6, 56
QUALITY = {0: (1, 2), 1: (2, 2), 2: (3, 3), 3: (9, 3)}


def mip_size(size, level):
    return max((size + (1 << level) - 1) >> level, 1)


def constants(width, height, fov, aspect, radius=0.5):
    """GTAOUpdateConstants and the folded falloff terms, every value fp32 (tan through the double function, rounded once)."""
    c = {}
    c["psx"], c["psy"] = F(1.0) / F(width), F(1.0) / F(height)
    ty = F(math.tan(float(F(fov) * F(0.5))))
    tx = F(ty * F(aspect))
    c["mulx"], c["muly"], c["addx"], c["addy"] = F(tx * F(2.0)), F(ty * F(-2.0)), F(tx * F(-1.0)), F(ty * F(1.0))
    c["mulPixX"] = F(c["mulx"] * c["psx"])
    for key, scale in (("", F(1.0)), ("mip", F(0.75))):
        er = F(F(radius) * F(1.457)) if key == "" else F(F(scale * F(radius)) * F(1.457))
        rng = F(F(0.615) * er)
        frm = F(er * F(F(1.0) - F(0.615)))
        c[key + "effectRadius"], c[key + "falloffMul"], c[key + "falloffAdd"] = er, F(F(-1.0) / rng), F(F(frm / rng) + F(1.0))
    return c


def _max0(x):
    return np.where(x > 0, x, x.dtype.type(0))


def _sat(x):
    a = _max0(x)
    return np.where(a < 1, a, x.dtype.type(1))


# ---------------------------------------------------------------- prefilter (fp32, exact) ----------------------------------------------------------------
def _mip_filter(d0, d1, d2, d3, mul, add):
    mx = np.maximum(np.maximum(d0, d1), np.maximum(d2, d3))
    with np.errstate(all="ignore"):
        w = [_sat((mx - d) * mul + add) for d in (d0, d1, d2, d3)]
        ws = ((w[0] + w[1]) + w[2]) + w[3]
        r = (((w[0] * d0 + w[1] * d1) + w[2] * d2) + w[3] * d3) / ws
    return np.where(mx == FLT_MAX, mx, r).astype(F)      # a quad with an empty texel stays empty


def prefilter(depth, c):
    """depth: [H, W] fp32 linear view depth ("empty" = FLT_MAX).  Returns the five levels, level m of mip_size(., m) pixels."""
    H, W = depth.shape
    d = np.where(depth > 0, depth, F(0)).astype(F)
    d = np.where(d < FLT_MAX, d, FLT_MAX).astype(F)                       # XeGTAO_ClampDepth, FP32 range
    gx, gy = (W + 15) // 16 * 8, (H + 15) // 16 * 8                     # threads: every workgroup is whole
    cx = np.minimum(np.arange(gx) * 2, W - 1); cx1 = np.minimum(cx + 1, W - 1)
    cy = np.minimum(np.arange(gy) * 2, H - 1); cy1 = np.minimum(cy + 1, H - 1)
    mul, add = c["mipfalloffMul"], c["mipfalloffAdd"]
    full = _mip_filter(d[np.ix_(cy, cx)], d[np.ix_(cy, cx1)], d[np.ix_(cy1, cx)], d[np.ix_(cy1, cx1)], mul, add)
    levels = [d, full[:mip_size(H, 1), :mip_size(W, 1)]]
    for m in (2, 3, 4):
        full = _mip_filter(full[0::2, 0::2], full[0::2, 1::2], full[1::2, 0::2], full[1::2, 1::2], mul, add)
        levels.append(full[:mip_size(H, m), :mip_size(W, m)])
    return [np.ascontiguousarray(l, dtype=F) for l in levels]


def _shift(img, dx, dy):
    """img at (x + dx, y + dy) with clamped coordinates."""
    H, W = img.shape[:2]
    ys = np.clip(np.arange(H) + dy, 0, H - 1); xs = np.clip(np.arange(W) + dx, 0, W - 1)
    return img[np.ix_(ys, xs)]


# ---------------------------------------------------------------- edges (fp32, exact) --------------------------------------------------------------------
def edges(level0):
    """XeGTAO_CalculateEdges + XeGTAO_PackEdges + the R8_UNORM store: uint8 codes."""
    z = level0.astype(F)
    with np.errstate(all="ignore"):
        e = [(_shift(z, -1, 0) - z), (_shift(z, 1, 0) - z), (_shift(z, 0, -1) - z), (_shift(z, 0, 1) - z)]
        slope_lr, slope_tb = (e[1] - e[0]) * F(0.5), (e[3] - e[2]) * F(0.5)
        adj = [e[0] + slope_lr, e[1] + -slope_lr, e[2] + slope_tb, e[3] + -slope_tb]
        den = z * F(0.011)
        packed = []
        for k in range(4):
            m = np.minimum(np.abs(e[k]), np.abs(adj[k]))
            packed.append(np.rint(_sat(_sat(F(1.25) - m / den)) * F(2.9)).astype(F))
        v = ((packed[0] * F(64.0 / 255.0) + packed[1] * F(16.0 / 255.0)) + packed[2] * F(4.0 / 255.0)) + packed[3] * F(1.0 / 255.0)
        return (_sat(v) * F(255.0) + F(0.5)).astype(np.uint32).astype(np.uint8)


# ---------------------------------------------------------------- denoise (fp32, exact) ------------------------------------------------------------------
def _unpack_edges(code):
    pv = ((code.astype(F) / F(255.0)) * F(255.5)).astype(np.uint32)
    return [_sat(((pv >> s) & 3).astype(F) / F(3.0)) for s in (6, 4, 2, 0)]      # L R T B


def denoise_pass(term, edge, blur, final):
    """One XeGTAO_Denoise pass over uint8 working term and edge codes."""
    v = term.astype(F) / F(255.0)
    C, L, R = _unpack_edges(edge), _unpack_edges(_shift(edge, -1, 0)), _unpack_edges(_shift(edge, 1, 0))
    T, B = _unpack_edges(_shift(edge, 0, -1)), _unpack_edges(_shift(edge, 0, 1))
    C = [C[0] * L[1], C[1] * R[0], C[2] * T[3], C[3] * B[2]]
    edginess = (_sat(F(1.5) - (((C[0] + C[1]) + C[2]) + C[3])) / F(1.5)) * F(0.5)
    C = [_sat(ck + edginess) for ck in C]
    dw = F(0.425)
    wTL, wTR = dw * (C[0] * L[2] + C[2] * T[0]), dw * (C[2] * T[1] + C[1] * R[2])
    wBL, wBR = dw * (C[3] * B[0] + C[0] * L[3]), dw * (C[1] * R[3] + C[3] * B[1])
    sw = np.full(v.shape, F(blur), dtype=F)
    s = v * sw
    for val, w in ((_shift(v, -1, 0), C[0]), (_shift(v, 1, 0), C[1]), (_shift(v, 0, -1), C[2]), (_shift(v, 0, 1), C[3]),
                   (_shift(v, -1, -1), wTL), (_shift(v, 1, -1), wTR), (_shift(v, -1, 1), wBL), (_shift(v, 1, 1), wBR)):
        s = s + w * val
        sw = sw + w
    ao = s / sw
    if final:
        ao = ao * F(1.5)
    return np.minimum((ao * F(255.0) + F(0.5)).astype(np.uint32), 255).astype(np.uint8)


def denoise(term, edge, passes):
    """denoisePasses 0..3 as brmi_gtao_denoise runs them: 0 = one final pass with beta 1e4; n >= 1 = n - 1 passes with beta / 5, then the final one with 1.2."""
    beta = F(1e4) if passes == 0 else F(1.2)
    for _ in range(max(passes, 1) - 1):
        term = denoise_pass(term, edge, F(beta / F(5.0)), False)
    return denoise_pass(term, edge, beta, True)


# ---------------------------------------------------------------- main pass -----------------------------------------------------------------------------
def hilbert_index(x, y):
    """HilbertIndex (XeGTAO.h:121-143) on uint32 arrays; only the low six bits of a coordinate take part."""
    x = (np.asarray(x, dtype=np.uint32) & 63).copy(); y = (np.asarray(y, dtype=np.uint32) & 63).copy()
    index = np.zeros(x.shape, dtype=np.uint32)
    lvl = 32
    while lvl > 0:
        rx = ((x & lvl) > 0).astype(np.uint32); ry = ((y & lvl) > 0).astype(np.uint32)
        index += np.uint32(lvl * lvl) * ((np.uint32(3) * rx) ^ ry)
        flip = (ry == 0) & (rx == 1)
        x = np.where(flip, np.uint32(63) - x, x); y = np.where(flip, np.uint32(63) - y, y)
        swap = ry == 0
        x, y = np.where(swap, y, x), np.where(swap, x, y)
        lvl //= 2
    return index


def noise(px, py, noise_index):
    """SpatioTemporalNoise, fp32 (the definition: see the module text)."""
    idx = (hilbert_index(px, py) + np.uint32(288 * (noise_index % 64))).astype(F)
    a = F(0.5) + idx * F(0.75487766624669276005); b = F(0.5) + idx * F(0.5698402909980532659114)
    return a - np.floor(a), b - np.floor(b)


def fast_sqrt(x):
    bits = x.astype(F).view(np.int32) >> 1                                 # asint(x) >> 1, arithmetic
    return (np.uint32(0x1fbd1df5) + bits.view(np.uint32)).view(F).astype(x.dtype)


def fast_acos(v):
    T = v.dtype.type
    x = np.abs(v)
    res = T(F(-0.156583)) * x + T(F(1.570796))
    res = res * fast_sqrt(T(1.0) - x)
    return np.where(v >= 0, res, T(F(3.141593)) - res)


def _normalize(v):
    d = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    inv = d.dtype.type(1.0) / np.sqrt(d)
    return [v[0] * inv, v[1] * inv, v[2] * inv]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _fetch(level, x, y):
    h, w = level.shape
    return level[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]


def main_pass(levels, normals, view3, c, quality=2, noise_index=0, max_depth_lod=0, dtype=np.float64):
    """levels: prefilter()'s output; normals: [H, W, 3] fp32 world normals; view3: the 3x3 of the camera's view matrix (row vector x matrix).
    Returns (value, fragile, covered): value = saturate(v / 1.5) * 255 before the + 0.5 and the truncation (170 at empty pixels)."""
    T = np.dtype(dtype).type
    slices, steps = QUALITY[quality]
    k = {name: T(v) for name, v in c.items()}
    z0 = levels[0]
    H, W = z0.shape
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    covered = z0 != FLT_MAX
    fragile = np.zeros((H, W), dtype=bool)
    with np.errstate(all="ignore"):
        nw = [normals[..., i].astype(T) for i in range(3)]
        V = view3.astype(T)
        vn = _normalize([(nw[0] * V[0, j] + nw[1] * V[1, j]) + nw[2] * V[2, j] for j in range(3)])
        vn[2] = -vn[2]
        n_slice, n_sample = (a.astype(T) for a in noise(px, py, noise_index))
        nspx, nspy = (px.astype(T) + T(0.5)) * k["psx"], (py.astype(T) + T(0.5)) * k["psy"]
        vz = z0.astype(T) * T(F(0.99999))
        pc = [(k["mulx"] * nspx + k["addx"]) * vz, (k["muly"] * nspy + k["addy"]) * vz, vz]
        vv = _normalize([-pc[0], -pc[1], -pc[2]])
        ssr = k["effectRadius"] / (vz * k["mulPixX"])
        visibility = _sat((T(10.0) - ssr) / T(100.0)) * T(0.5)
        min_s = T(F(1.3)) / ssr
        PI, PI_HALF = T(F(3.1415926535897932)), T(F(1.5707963267948966))

        def tap(rx, ry, sign, level, low, horizon):
            nonlocal fragile
            spx, spy = nspx + T(sign) * (rx * k["psx"]), nspy + T(sign) * (ry * k["psy"])
            sz = _fetch(levels[0], px + (sign * rx).astype(np.int64), py + (sign * ry).astype(np.int64))
            for m in range(1, max_depth_lod + 1):
                lw, lh = mip_size(W, m), mip_size(H, m)
                tx, ty = np.clip(spx * T(lw), -1.0, 65536.0), np.clip(spy * T(lh), -1.0, 65536.0)
                on = level == m
                # (only the cuts between two texels of the level: beyond its first and last one both sides of a cut clamp to the same texel)
                fragile |= covered & on & (((np.abs(tx - np.rint(tx)) < N_TEXEL * EPS * np.maximum(np.abs(tx), 1.0)) & (np.rint(tx) >= 1) & (np.rint(tx) <= lw - 1)) |
                                           ((np.abs(ty - np.rint(ty)) < N_TEXEL * EPS * np.maximum(np.abs(ty), 1.0)) & (np.rint(ty) >= 1) & (np.rint(ty) <= lh - 1)))
                sz = np.where(on, _fetch(levels[m], np.floor(tx).astype(np.int64), np.floor(ty).astype(np.int64)), sz)
            empty = sz == FLT_MAX
            szt = np.where(empty, T(1.0), sz.astype(T))
            sp = [(k["mulx"] * spx + k["addx"]) * szt, (k["muly"] * spy + k["addy"]) * szt, szt]
            delta = [sp[0] - pc[0], sp[1] - pc[1], sp[2] - pc[2]]
            dist = np.sqrt(_dot(delta, delta))
            hv = [delta[0] / dist, delta[1] / dist, delta[2] / dist]
            weight = _sat(dist * k["falloffMul"] + k["falloffAdd"])
            shc = _dot(hv, vv)
            shc = low + weight * (shc - low)
            return np.where(empty, horizon, np.maximum(horizon, shc))

        for sl in range(slices):
            slice_k = (T(sl) + n_slice) / T(slices)
            phi = slice_k * PI
            cos_phi, sin_phi = np.cos(phi), np.sin(phi)
            omx, omy = cos_phi * ssr, -sin_phi * ssr
            dvv = cos_phi * vv[0] + sin_phi * vv[1]
            ortho = [cos_phi - dvv * vv[0], sin_phi - dvv * vv[1], T(0.0) - dvv * vv[2]]
            cr = [ortho[1] * vv[2] - ortho[2] * vv[1], ortho[2] * vv[0] - ortho[0] * vv[2], ortho[0] * vv[1] - ortho[1] * vv[0]]
            axis = _normalize(cr)
            nda = _dot(vn, axis)
            proj = [vn[0] - axis[0] * nda, vn[1] - axis[1] * nda, vn[2] - axis[2] * nda]
            sd = _dot(ortho, proj)
            fragile |= covered & (np.abs(sd) < N_SIGN * EPS)
            sign_norm = np.sign(sd)
            proj_len = np.sqrt(_dot(proj, proj))
            cos_norm = _sat(_dot(proj, vv) / proj_len)
            n = sign_norm * fast_acos(cos_norm)
            low0, low1 = np.cos(n + PI_HALF), np.cos(n - PI_HALF)
            h0c, h1c = low0, low1
            for st in range(steps):
                base = T(sl + st * steps) * T(F(0.6180339887498948482))
                t = n_sample + base
                step_noise = t - np.floor(t)
                s = (T(st) + step_noise) / T(steps)
                s = s * s
                s = s + min_s
                sox, soy = s * omx, s * omy
                length = np.sqrt(sox * sox + soy * soy)
                bound = N_OFFSET * EPS * np.maximum(length, 1.0)
                for comp in (sox, soy):
                    fragile |= covered & (np.abs(np.abs(comp - np.floor(comp)) - 0.5) < bound)
                level = np.zeros((H, W), dtype=np.int64)
                if max_depth_lod > 0:
                    lg = np.log2(length)
                    mip = np.minimum(np.clip(lg - T(F(3.30)), 0.0, 5.0), T(max_depth_lod))
                    level = np.floor(mip + T(0.5)).astype(np.int64)
                    fragile |= covered & (np.abs((mip + 0.5) - np.rint(mip + 0.5)) < N_LEVEL * EPS * np.maximum(np.abs(lg), 3.3))
                rx, ry = np.clip(np.rint(sox), -65536.0, 65536.0), np.clip(np.rint(soy), -65536.0, 65536.0)
                rx, ry = np.where(covered, rx, 0.0).astype(T), np.where(covered, ry, 0.0).astype(T)
                h0c = tap(rx, ry, 1, level, low0, h0c)
                h1c = tap(rx, ry, -1, level, low1, h1c)
            proj_len = proj_len + T(F(0.05)) * (T(1.0) - proj_len)
            h0, h1 = -fast_acos(h1c), fast_acos(h0c)
            sin_n = np.sin(n)
            iarc0 = ((cos_norm + (T(2.0) * h0) * sin_n) - np.cos(T(2.0) * h0 - n)) / T(4.0)
            iarc1 = ((cos_norm + (T(2.0) * h1) * sin_n) - np.cos(T(2.0) * h1 - n)) / T(4.0)
            visibility = visibility + proj_len * (iarc0 + iarc1)
        visibility = visibility / T(slices)
        visibility = np.where(visibility > 0, np.power(np.where(visibility > 0, visibility, T(1.0)), T(F(2.2))), T(0.0))
        visibility = np.maximum(T(F(0.03)), visibility)
        value = _sat(visibility / T(1.5)) * T(255.0)
    value = np.where(covered, value, T(170.0))
    return value, fragile & covered, covered


def code_of(value):
    """The stored working term of a pre-rounding value: uint(value + 0.5)."""
    return np.floor(np.asarray(value, dtype=np.float64) + 0.5).astype(np.int64)


# ---------------------------------------------------------------- test inputs ---------------------------------------------------------------------------
def look_at_view():
    """The camera of the analytic inputs: at the origin looking down -z, y up; view = identity (row vector x matrix)."""
    return np.eye(3, dtype=F)


def height_field(kind, width, height, fov=1.0, aspect=None):
    """Analytic inputs written straight into the depth and normals planes: (depth [H, W] fp32, world normals [H, W, 3] fp32, fov, aspect).  The right third of
    every frame is empty.  The camera sits at the origin and looks down -z (view = identity): a pixel's eye ray is (ndc * tanHalfFov, -1) * depth.
      floor   a ground plane seen from 1.2 above, tilted into the picture
      box     a wall at depth 3 with a box 0.4 nearer in the middle: a step edge all round
      sphere  a sphere cap of radius 1.2 in front of a wall at depth 4
      wall    a wall seen at a grazing angle (10 degrees off the view axis)"""
    aspect = width / height if aspect is None else aspect
    ty = math.tan(fov * 0.5); tx = ty * aspect
    ys, xs = np.meshgrid((np.arange(height) + 0.5) / height, (np.arange(width) + 0.5) / width, indexing="ij")
    dx, dy = (xs * 2.0 - 1.0) * tx, (1.0 - ys * 2.0) * ty                  # the ray through the pixel is (dx, dy, -1) * depth
    depth = np.full((height, width), np.inf); nrm = np.zeros((height, width, 3))
    nrm[..., 2] = 1.0

    def plane(n, d0):                                                        # points p with n . p = d0; depth along (dx, dy, -1)
        n = np.asarray(n, dtype=np.float64); n = n / np.linalg.norm(n)
        den = n[0] * dx + n[1] * dy - n[2]
        t = np.where(np.abs(den) > 1e-9, d0 / den, np.inf)
        return np.where(t > 0.05, t, np.inf), n
    if kind == "floor":
        t, n = plane((0.0, 1.0, 0.25), -1.2)
        depth = t; nrm[...] = n                                              # (the eye is on n's side of the plane: n faces it)
    elif kind == "box":
        depth[...] = 3.0
        inside = (np.abs(dx * 2.6) < 0.45) & (np.abs(dy * 2.6) < 0.3)
        depth[inside] = 2.6
    elif kind == "sphere":
        depth[...] = 4.0
        cz, r = 3.2, 1.2                                                     # centre (0, 0, -cz)
        a = dx * dx + dy * dy + 1.0; b = -2.0 * cz; cc = cz * cz - r * r
        disc = b * b - 4 * a * cc
        t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
        hit = np.isfinite(t)
        depth[hit] = t[hit]
        tf = np.where(hit, t, 0.0)
        p = np.stack([dx * tf, dy * tf, -tf + cz], axis=-1)
        nrm[hit] = (p / r)[hit]
    elif kind == "wall":
        t, n = plane((1.0, 0.0, math.tan(math.radians(10.0))), -0.6)      # x + z tan(10 deg) = -0.6: on the left, receding into the picture
        depth = t; nrm[...] = n
    else:
        raise ValueError(kind)
    depth = np.where(np.isfinite(depth) & (depth < 60.0), depth, np.inf)
    depth[:, (2 * width) // 3:] = np.inf
    out = np.where(np.isfinite(depth), depth, FLT_MAX).astype(F)
    nrm = nrm / np.maximum(np.linalg.norm(nrm, axis=-1, keepdims=True), 1e-12)
    return out, nrm.astype(F), fov, aspect


def camera_fields(camera_bytes):
    """(fov, aspectRatio, the 3x3 of view) out of a brmi_camera's bytes (include/brmi_types.h: position (4 floats), view (16), eight more matrices, six planes)."""
    f = np.frombuffer(np.ascontiguousarray(camera_bytes).tobytes()[:736], dtype=F)
    return float(f[172]), float(f[173]), f[4:20].reshape(4, 4)[:3, :3].copy()


def case_inputs(kind, width, height, camera_bytes, radius=0.5):
    """The inputs of one case as the GPU test writes them for a pass whose camera is `camera_bytes`: (depth, WORLD normals, constants, view 3x3).  The height field
    is laid out in view space with the camera's own fov and aspect; its normals go to world space through the transpose of the view rotation."""
    fov, aspect, view3 = camera_fields(camera_bytes)
    depth, n_view, _, _ = height_field(kind, width, height, fov, aspect)
    n_world = (n_view.astype(np.float64) @ view3.astype(np.float64).T).astype(F)
    return depth, n_world, constants(width, height, fov, aspect, radius), view3


MAIN_CONFIGS = [(2, 0), (2, 4), (3, 0)]      # (qualityLevel, maxDepthLod) of the main-pass checks; Ultra on the 64 x 40 frames only
NOISE_INDEX = 5                               # the frame index the GPU tests update with
_cache = {}


def main_configs(width):
    return [cfg for cfg in MAIN_CONFIGS if cfg[0] != 3 or width == 64]


def reference(kind, width, height, camera_bytes, quality, max_depth_lod):
    """Everything the tests share about one case and configuration, computed once: inputs, levels, edge codes, the float64 main pass (value, fragile, covered)
    and the largest |fp32 - float64| of the pre-rounding value over non-fragile covered pixels."""
    key = (kind, width, height, quality, max_depth_lod, np.ascontiguousarray(camera_bytes).tobytes())
    if key not in _cache:
        depth, normals, c, view3 = case_inputs(kind, width, height, camera_bytes)
        levels = prefilter(depth, c)
        v64, fragile, covered = main_pass(levels, normals, view3, c, quality, NOISE_INDEX, max_depth_lod)
        v32, _, _ = main_pass(levels, normals, view3, c, quality, NOISE_INDEX, max_depth_lod, dtype=np.float32)
        ok = covered & ~fragile
        _cache[key] = dict(depth=depth, normals=normals, constants=c, view3=view3, levels=levels, edges=edges(levels[0]), value=v64, fragile=fragile, covered=covered,
                           fp32_error=float(np.abs(v32.astype(np.float64) - v64)[ok].max()) if ok.any() else 0.0)
    return _cache[key]


def margin(camera_of):
    """M = 4 x the largest |fp32 numpy - float64| of the pre-rounding value over the non-fragile pixels of every case and configuration.  camera_of(width, height)
    gives the camera bytes of the pass of that size."""
    return 4.0 * max(reference(kind, w, h, camera_of(w, h), q, lod)["fp32_error"] for kind, w, h in CASES for q, lod in main_configs(w))


CASES = [("floor", 101, 53), ("box", 101, 53), ("sphere", 101, 53), ("wall", 101, 53), ("floor", 64, 40), ("box", 64, 40), ("sphere", 64, 40), ("wall", 64, 40)]
