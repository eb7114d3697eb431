"""The display chain restated in numpy from the reference's shader text: luminance histogram and average, LpmSetup / LpmMap for the one
configuration the reference uses, the other tone curves, gamma and the UNORM store, the bloom pyramid.  Written from the HLSL, not from the kernels.

Two arithmetic modes, chosen by the dtype F every function takes:
    np.float32   every operation rounds to fp32 in the kernels' order (what brmi_display_math.h computes, up to the math library's log2 / exp2 / pow);
    np.float64   the same formulas in double: the value the decisions are judged by.
Constants are the fp32 constants of the text in both modes (they are part of the definition, not of the rounding).

A decision (a histogram bin, an 8-bit code, a half store, the downsample's length cut) is FRAGILE where the float64 value lies within a margin of the decision's
boundary; margins() measures those margins as the largest fp32-against-float64 difference over the inputs, times FACTOR.
"""
import numpy as np

FACTOR = 4.0      # for the GPU's log2, exp2 and pow, which are within 1-2 ULP of numpy's
MIN_LOG = np.float32(0.001)
LOG_RANGE = np.float32(np.log2(np.float32(10.0)) - np.log2(np.float32(0.1)))
HDR_MAX, BLOOM_RADIUS = 10.0, 0.001
SIZES = [(64, 40), (101, 53)]
CURVES = ["reinhard", "neutral", "aces", "lpm", "none"]


def k(F, v):
    return F(np.float32(v))


def sat(x):
    return np.fmin(np.fmax(x, x.dtype.type(0)), x.dtype.type(1))


def to_half(x):
    """What an RGBA16F store keeps (round to nearest even), as float16."""
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float16)


def halves_to_u64(rgb16, alpha=1.0):
    """(H, W, 3) float16 + alpha -> (H, W) uint64 as the surfaces hold a pixel."""
    a = np.full(rgb16.shape[:2] + (1,), alpha, dtype=np.float16)
    return np.ascontiguousarray(np.concatenate([rgb16, a], axis=-1)).view(np.uint64)[..., 0]


def u64_to_halves(img):
    return np.ascontiguousarray(img).view(np.float16).reshape(img.shape + (4,))


# ---------------------------------------------------------------- histogram and average ------------------------------------------------------------------
def luminance(rgb, F):
    r, g, b = (rgb[..., i].astype(F) for i in range(3))
    return (r * k(F, 0.2125) + g * k(F, 0.7154)) + b * k(F, 0.0721)


def bin_value(rgb, F, min_log=MIN_LOG, inv_range=None):
    """(luminance, logLum * 254 + 1, the logarithm's term before the saturate): the bin is 0 below 0.005, otherwise the value truncated."""
    inv_range = np.float32(1.0) / LOG_RANGE if inv_range is None else inv_range
    lum = luminance(rgb, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        raw = (np.log2(lum) - F(min_log)) * F(inv_range)
        v = sat(raw) * F(254.0) + F(1.0)
    return lum, v, raw


def bins_of(rgb, F, **kw):
    lum, v, _ = bin_value(rgb, F, **kw)
    return np.where(lum < k(F, 0.005), 0, np.nan_to_num(v, nan=1.0).astype(np.int64))


def histogram(rgb, F=np.float64, **kw):
    return np.bincount(bins_of(rgb, F, **kw).reshape(-1), minlength=256).astype(np.uint32)


def weighted_sum(hist):
    return int((hist.astype(np.uint64) * np.arange(256, dtype=np.uint64)).sum() & np.uint64(0xFFFFFFFF))      # uint32, wrapping as the shader's sum


def average_luminance(hist, num_pixels, F, min_log=MIN_LOG, log_range=LOG_RANGE):
    n = np.float32(num_pixels)      # NUM_PIXELS is passed as a float
    wla = F(np.float32(weighted_sum(hist))) / np.fmax(F(n) - F(np.float32(hist[0])), F(1.0)) - F(1.0)
    return np.exp2(wla / F(254.0) * F(log_range) + F(min_log))


def adapt(last, average, tc, F):
    return F(last) + (F(average) - F(last)) * F(np.float32(tc))


# ---------------------------------------------------------------- LpmSetup / LpmMap ---------------------------------------------------------------------------
def _luma_of_rec709(F):
    def z(s):
        return np.array([s[0], s[1], F(1.0) - (s[0] + s[1])], dtype=F)
    r, g, b, w = ([k(F, x), k(F, y)] for x, y in ((0.64, 0.33), (0.30, 0.60), (0.15, 0.06), (0.3127, 0.3290)))
    rz, gz, bz = z(r), z(g), z(b)
    ix, iy, iz = (np.array([rz[i], gz[i], bz[i]], dtype=F) for i in range(3))      # the transpose
    w3 = z(w) * (F(1.0) / w[1])
    i = F(1.0) / ((ix[0] * (iy[1] * iz[2] - iz[1] * iy[2]) - ix[1] * (iy[0] * iz[2] - iy[2] * iz[0])) + ix[2] * (iy[0] * iz[1] - iy[1] * iz[0]))
    ox = np.array([(iy[1] * iz[2] - iz[1] * iy[2]) * i, (ix[2] * iz[1] - ix[1] * iz[2]) * i, (ix[1] * iy[2] - ix[2] * iy[1]) * i], dtype=F)
    oy = np.array([(iy[2] * iz[0] - iy[0] * iz[2]) * i, (ix[0] * iz[2] - ix[2] * iz[0]) * i, (iy[0] * ix[2] - ix[0] * iy[2]) * i], dtype=F)
    oz = np.array([(iy[0] * iz[1] - iz[0] * iy[1]) * i, (iz[0] * ix[1] - ix[0] * iz[1]) * i, (ix[0] * iy[1] - iy[0] * ix[1]) * i], dtype=F)

    def dot(a, c):
        return (a[0] * c[0] + a[1] * c[1]) + a[2] * c[2]
    s = np.array([dot(ox, w3), dot(oy, w3), dot(oz, w3)], dtype=F)
    y = iy * s
    return y * (F(1.0) / ((y[0] + y[1]) + y[2]))


def exposure_of(adapted, F):
    return np.log2(k(F, HDR_MAX) * k(F, 0.18) / np.fmax(F(adapted), k(F, 1e-5)))


def lpm_params(adapted, F):
    """The fp32 words of the control block LpmSetup writes for shoulder 1, con 0, soft 0, con2 0, clip 1, scaleOnly 0, Rec.709 / D65 three times."""
    exposure = exposure_of(adapted, F)
    contrast, shoulder, hdr_max, mid_out = F(1.0), F(1.0), k(F, HDR_MAX), k(F, 0.18)
    mid_in = (hdr_max * k(F, 0.18)) * np.exp2(-exposure)
    cs = contrast * shoulder
    z0 = -np.power(mid_in, contrast)
    z1 = np.power(hdr_max, cs) * np.power(mid_in, contrast)
    z2 = (np.power(hdr_max, contrast) * np.power(mid_in, cs)) * mid_out
    z3 = np.power(hdr_max, cs) * mid_out
    z4 = np.power(mid_in, cs) * mid_out
    tsb0 = -((z0 + (mid_out * (z1 - z2)) * (F(1.0) / (z3 - z4))) * (F(1.0) / z4))
    tsb1 = (z1 - z2) * (F(1.0) / (z3 - z4))
    luma = _luma_of_rec709(F)
    return dict(saturation=np.full(3, contrast, dtype=F), contrast=contrast, shoulderContrast=shoulder, toneScaleBias=np.array([tsb0, tsb1], dtype=F),
                lumaT=luma, rcpLumaT=F(1.0) / luma, crosstalk=np.ones(3, dtype=F), exposure=exposure, midIn=mid_in)


def lpm_control(p):
    """The 96 words in the reference's packing, as floats of the params' dtype (the packed-half words 16-20 and the reserved ones are zero)."""
    w = np.zeros(96, dtype=p["lumaT"].dtype)
    w[0:3], w[3], w[4:6], w[6:9], w[9:12], w[12:15] = p["saturation"], p["contrast"], p["toneScaleBias"], p["lumaT"], p["crosstalk"], p["rcpLumaT"]
    w[24], w[25:28] = p["shoulderContrast"], p["lumaT"]
    return w


def lpm_map(rgb, p, F):
    r, g, b = (rgb[..., i].astype(F) for i in range(3))
    lt, ct, rl = p["lumaT"], p["crosstalk"], p["rcpLumaT"]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rcp_max = F(1.0) / np.fmax(np.fmax(r, g), b)
        rr, rg, rb = (np.power(c * rcp_max, s) for c, s in zip((r, g, b), p["saturation"]))
        luma = g * lt[1] + (r * lt[0] + (b * lt[2]))
        luma = np.power(luma, p["contrast"])
        shoulder = np.power(luma, p["shoulderContrast"])
        luma = luma * (F(1.0) / (shoulder * p["toneScaleBias"][0] + p["toneScaleBias"][1]))
        luma_ratio = (rr * lt[0] + rg * lt[1]) + rb * lt[2]
        scale = sat(luma * (F(1.0) / luma_ratio))
        cr, cg, cb = sat(rr * scale), sat(rg * scale), sat(rb * scale)
        kr, kg, kb = -ct[0] * cr + ct[0], -ct[1] * cg + ct[1], -ct[2] * cb + ct[2]
        add = sat((-cb) * lt[2] + ((-cr) * lt[0] + ((-cg) * lt[1] + luma)))
        t = add * (F(1.0) / (kg * lt[1] + (kr * lt[0] + (kb * lt[2]))))
        cr, cg, cb = sat(t * kr + cr), sat(t * kg + cg), sat(t * kb + cb)
        add = sat((-cb) * lt[2] + ((-cr) * lt[0] + ((-cg) * lt[1] + luma)))
        cr, cg, cb = sat(add * rl[0] + cr), sat(add * rl[1] + cg), sat(add * rl[2] + cb)
    return np.stack([cr, cg, cb], axis=-1)


# ---------------------------------------------------------------- the other curves, gamma, the store -----------------------------------------------------
def reinhard_jodie(rgb, F):
    c = rgb.astype(F)
    lum = ((c[..., 0] * k(F, 0.2126) + c[..., 1] * k(F, 0.7152)) + c[..., 2] * k(F, 0.0722))[..., None]
    pc, lm = c / (F(1.0) + c), c / (F(1.0) + lum)
    return lm + pc * (pc - lm)


def khronos_neutral(rgb, F):
    c = rgb.astype(F)
    start, desat = k(F, 0.8) - k(F, 0.04), k(F, 0.15)
    x = np.fmin(c[..., 0], np.fmin(c[..., 1], c[..., 2]))
    offset = np.where(x < k(F, 0.08), x - (k(F, 6.25) * x) * x, k(F, 0.04))
    c = c - offset[..., None]
    peak = np.fmax(c[..., 0], np.fmax(c[..., 1], c[..., 2]))
    d = F(1.0) - start
    with np.errstate(divide="ignore", invalid="ignore"):
        new_peak = F(1.0) - (d * d) / ((peak + d) - start)
        scaled = c * (new_peak / peak)[..., None]
        g = F(1.0) - F(1.0) / (desat * (peak - new_peak) + F(1.0))
        out = scaled + g[..., None] * (new_peak[..., None] - scaled)
    return np.where((peak < start)[..., None], c, out)


ACES_IN = np.array([[0.59719, 0.07600, 0.02840], [0.35458, 0.90834, 0.13383], [0.04823, 0.01566, 0.83777]], dtype=np.float32)
ACES_OUT = np.array([[1.60475, -0.10208, -0.00327], [-0.53108, 1.10813, -0.07276], [-0.07367, -0.00605, 1.07602]], dtype=np.float32)


def _mul_row(c, m, F):      # mul(color, M): out[j] = (c0 M[0][j] + c1 M[1][j]) + c2 M[2][j]
    m = m.astype(F)
    return np.stack([(c[..., 0] * m[0, j] + c[..., 1] * m[1, j]) + c[..., 2] * m[2, j] for j in range(3)], axis=-1)


def aces_hill(rgb, F):
    v = _mul_row(rgb.astype(F), ACES_IN, F)
    a = v * (v + k(F, 0.0245786)) - k(F, 0.000090537)
    b = v * (k(F, 0.983729) * v + k(F, 0.4329510)) + k(F, 0.238081)
    return sat(_mul_row(a / b, ACES_OUT, F))


def tone_map(curve, rgb, F, lpm=None):
    curve = CURVES.index(curve) if isinstance(curve, str) else int(curve)
    if curve == 0:
        return reinhard_jodie(rgb, F)
    if curve == 1:
        return khronos_neutral(rgb, F)
    if curve == 2:
        return aces_hill(rgb, F)
    if curve == 3:
        return lpm_map(rgb, lpm, F)
    return rgb.astype(F)


def code_value(mapped, F):
    """saturate(pow(c, 1 / 2.2)) * 255 + 0.5: the 8-bit code is this value truncated; a NaN stores 0."""
    with np.errstate(invalid="ignore"):
        g = np.power(mapped.astype(F), F(np.float32(1.0) / np.float32(2.2)))
    return sat(g) * F(255.0) + F(0.5)


def codes_of(value):
    return np.nan_to_num(value, nan=0.0).astype(np.int64)


def resolve(curve, rgb, F, lpm=None):
    """(H, W, 3) code values of a frame of (already blended) halves."""
    return code_value(tone_map(curve, rgb, F, lpm), F)


# ---------------------------------------------------------------- bloom ------------------------------------------------------------------------------------
def level_count(w, h):
    return min(5, int(np.floor(np.log2(max(w, h)))) + 1)


def level_size(w, h, level):
    return w >> level, h >> level


def bloom_possible(w, h):
    return min(w, h) >= 32


def _uv(w, h, F):
    u = (np.arange(w, dtype=np.float32).astype(F) + F(0.5)) / F(np.float32(w))
    v = (np.arange(h, dtype=np.float32).astype(F) + F(0.5)) / F(np.float32(h))
    return np.broadcast_to(u[None, :], (h, w)), np.broadcast_to(v[:, None], (h, w))


def bilinear(src, u, v, F):
    """SampleLevel(g_linearClamp, uv, 0) of an (H, W, 3) level: fp32 (or float64) weights, clamped texel coordinates."""
    h, w = src.shape[:2]
    x, y = u * F(np.float32(w)) - F(0.5), v * F(np.float32(h)) - F(0.5)
    x0f, y0f = np.floor(x), np.floor(y)
    fx, fy = (x - x0f)[..., None], (y - y0f)[..., None]
    x0, x1 = np.clip(x0f, 0, w - 1).astype(np.int64), np.clip(x0f + 1, 0, w - 1).astype(np.int64)
    y0, y1 = np.clip(y0f, 0, h - 1).astype(np.int64), np.clip(y0f + 1, 0, h - 1).astype(np.int64)
    s = src.astype(F)
    t00, t10, t01, t11 = s[y0, x0], s[y0, x1], s[y1, x0], s[y1, x1]
    r0, r1 = t00 + fx * (t10 - t00), t01 + fx * (t11 - t01)
    return r0 + fy * (r1 - r0)


DOWN_TAPS = [(-2, 2), (0, 2), (2, 2), (-2, 0), (0, 0), (2, 0), (-2, -2), (0, -2), (2, -2), (-1, 1), (1, 1), (-1, -1), (1, -1)]      # a .. m
TENT_TAPS = [(-1, 1), (0, 1), (1, 1), (-1, 0), (0, 0), (1, 0), (-1, -1), (0, -1), (1, -1)]      # a .. i


def downsample(src, F):
    """bloomDownsample.hlsl from an (H, W, 3) level to the next: (value before the store with the cut applied, length, kept)."""
    sh, sw = src.shape[:2]
    w, h = sw >> 1, sh >> 1
    u, v = _uv(w, h, F)
    x, y = F(np.float32(1.0) / np.float32(sw)), F(np.float32(1.0) / np.float32(sh))
    t = [bilinear(src, u + F(ox) * x, v + F(oy) * y, F) for ox, oy in DOWN_TAPS]
    d = t[4] * F(0.125)
    d = d + (((t[0] + t[2]) + t[6]) + t[8]) * F(0.03125)
    d = d + (((t[1] + t[3]) + t[5]) + t[7]) * F(0.0625)
    d = d + (((t[9] + t[10]) + t[11]) + t[12]) * F(0.125)
    d = np.fmax(d, k(F, 0.00001))
    length = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    kept = ~(length < F(1.0))
    return np.where(kept[..., None], d, F(0.0)), length, kept


def tent(src, w, h, F):
    """sample_for_upsample of an (h, w) destination: radius 0.001 in u, 0.001 * (w / h) in v."""
    u, v = _uv(w, h, F)
    x = k(F, BLOOM_RADIUS)
    y = F(np.float32(BLOOM_RADIUS) * (np.float32(w) / np.float32(h)))      # the host's fp32 product
    t = [bilinear(src, u + F(ox) * x, v + F(oy) * y, F) for ox, oy in TENT_TAPS]
    up = t[4] * F(4.0)
    up = up + (((t[1] + t[3]) + t[5]) + t[7]) * F(2.0)
    up = up + (((t[0] + t[2]) + t[6]) + t[8])
    return up * F(np.float32(1.0) / np.float32(16.0))


def upsample(src, dst, F):
    """The additive blend into the RGBA16F level: float(dst) + float(tent), before the store."""
    h, w = dst.shape[:2]
    return dst.astype(F) + tent(src, w, h, F)


def blend(hdr, level1, F):
    """bloomBlend.hlsl: lerp(existing, tent(level 1), 0.04), before the store."""
    h, w = hdr.shape[:2]
    e = hdr.astype(F)
    return e + k(F, 0.04) * (tent(level1, w, h, F) - e)


def half_distance(value):
    """Distance of a float64 value from the nearest rounding boundary of the half grid, in units of the half spacing there (0.5 = as far as can be)."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.abs(np.asarray(value, dtype=np.float64))
        h = v.astype(np.float16).astype(np.float64)
        spacing = np.maximum(np.spacing(np.minimum(h, 65504.0).astype(np.float16)).astype(np.float64), 2.0 ** -24)
        return 0.5 - np.abs(v - h) / spacing


def bloom_chain(hdr16, F=np.float64):
    """The whole pyramid in one mode, each store rounded to half: levels after the downsamples, after the upsamples, and the blended level 0 (float16)."""
    down = [hdr16]
    for _ in range(5):
        down.append(to_half(downsample(down[-1], F)[0]))
    up = list(down)
    for i in range(4, 0, -1):
        up[i] = to_half(upsample(up[i + 1], up[i], F))
    return down, up, to_half(blend(hdr16, up[1], F))


# ---------------------------------------------------------------- inputs ---------------------------------------------------------------------------------------
def _hash(a):
    a = (a ^ (a >> np.uint32(16))) * np.uint32(0x7FEB352D)
    a = (a ^ (a >> np.uint32(15))) * np.uint32(0x846CA68B)
    return a ^ (a >> np.uint32(16))


def frame(kind, w, h, seed=1):
    """(H, W, 3) float16 HDR inputs.  "ramp": a smooth log-luminance ramp from 1e-3 to 50 with per-pixel hashed colour, a few saturated texels above 10, the
    right third exactly zero; "halfzero": the ramp with the lower half zero; "dark": everything below the histogram's 0.005 (bin 0); "bright": 2 .. 60;
    "glow": 0.25 .. 24 with smooth colour, the bloom's input (the downsample's cut keeps about half of it)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.uint32)
    with np.errstate(over="ignore"):
        hsh = _hash(xx * np.uint32(9781) + yy * np.uint32(6271) + np.uint32(seed * 7919))
    col = np.stack([((hsh >> np.uint32(s)) & np.uint32(255)).astype(np.float64) / 255.0 for s in (0, 8, 16)], axis=-1) * 0.8 + 0.2
    t = (xx.astype(np.float64) / max(w - 1, 1) + yy.astype(np.float64) / max(h - 1, 1)) * 0.5
    if kind == "glow":      # smooth in luminance and in colour: the bloom taps' fp32 weights meet no steep gradient
        fx, fy = xx.astype(np.float64) / w, yy.astype(np.float64) / h
        col = np.stack([0.6 + 0.3 * np.sin(2.1 * fx + 1.3 * fy), 0.6 + 0.3 * np.cos(1.7 * fx - 0.9 * fy), 0.6 + 0.3 * np.sin(0.8 * fx + 2.3 * fy + 1.0)], axis=-1)
        lum = 0.25 * np.exp2(t * np.log2(24.0 / 0.25)) * (1.0 + 0.1 * np.sin(seed + 3.0 * fx + 2.0 * fy))
    elif kind == "dark":
        lum = 1e-4 + 2e-3 * t
    elif kind == "bright":
        lum = 2.0 * np.exp2(t * np.log2(30.0))
    else:
        lum = 1e-3 * np.exp2(t * np.log2(50.0 / 1e-3))
    img = col * (lum / (col @ np.array([0.2125, 0.7154, 0.0721])))[..., None]
    if kind in ("ramp", "halfzero"):
        hot = (hsh % np.uint32(97)) == 0
        img[hot] = img[hot] * 0.0 + np.array([14.0, 11.0, 30.0]) * (1.0 + col[hot])
        img[:, w - w // 3:] = 0.0
    if kind == "halfzero":
        img[h // 2:] = 0.0
    return to_half(img)


HISTOGRAM_KINDS = ("ramp", "halfzero", "dark", "bright")      # what each stage's tests use: the margins and fragile shares are measured over exactly these
RESOLVE_KINDS = ("ramp", "halfzero", "dark")
BLOOM_KINDS = ("glow",)
SEEDS = {}      # (kind, w, h) -> the seed test_display_cpu.py settled on; 1 where it is not listed


def case(kind, w, h):
    return frame(kind, w, h, SEEDS.get((kind, w, h), 1))


UP_SOURCE_SCALE = np.float32(1.0 / 32.0)


def upsample_case(w, h, i):
    """(level i + 1, level i) as the test writes them before upsample i: two glow fields of their own, the source a thirty-second of the destination's size of
    number.  Where a level is exactly half its source's size the tent's weights are sixteenths, so float(dst) + tent is a multiple of a sixteenth of the
    source's half spacing: with the pyramid's own levels (source as large as the destination, or the destination cut to zero) that sum IS a rounding boundary
    for one texel in five, whatever the seed.  A source 32 times smaller puts 512 such multiples between two halves of the sum, and one of them is the
    boundary."""
    dst = frame("glow", w >> i, h >> i, 10 + i)
    src = frame("glow", w >> (i + 1), h >> (i + 1), 20 + i).astype(np.float32) * UP_SOURCE_SCALE
    return to_half(src), dst


def blend_case(w, h):
    """(HDR, level 1) of the blend's test: level 1 is a glow field as bright as the frame.  (At 64 x 40 a level 1 eight times brighter, as the additive
    pyramid leaves it, makes tent - existing a multiple of half a spacing and 0.04 of it a near-boundary for 3 % of the pixels.)"""
    return case("glow", w, h), frame("glow", w >> 1, h >> 1, 30)


# ---------------------------------------------------------------- margins and fragile masks ----------------------------------------------------------------------
def _maxdiff(a32, a64):
    with np.errstate(invalid="ignore"):
        d = np.abs(a32.astype(np.float64) - a64)
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


_margins = None


def margins():
    """FACTOR x the largest fp32-against-float64 difference over the test inputs, per decision: `bin` and `code` in steps of the decision, `lum` and `length`
    absolute, `half_*` (the stores of the downsample, the upsample and the blend) in units of the half spacing, `adapted` and `control` relative."""
    global _margins
    if _margins is not None:
        return _margins
    m = dict(bin=0.0, lum=0.0, code=0.0, half_down=0.0, half_up=0.0, half_blend=0.0, length=0.0, adapted=0.0, control=0.0)
    for w, h in SIZES:
        for kind in HISTOGRAM_KINDS:
            img = case(kind, w, h)
            l32, v32, _ = bin_value(img, np.float32)
            l64, v64, _ = bin_value(img, np.float64)
            m["lum"] = max(m["lum"], _maxdiff(l32, l64)); m["bin"] = max(m["bin"], _maxdiff(v32, v64))
        for kind in RESOLVE_KINDS:
            img = case(kind, w, h)
            hist = histogram(img)
            a32, a64 = (average_luminance(hist, w * h, F) for F in (np.float32, np.float64))
            m["adapted"] = max(m["adapted"], abs(float(a32) - float(a64)) / float(a64))
            p32 = lpm_params(a32, np.float32)
            c32, c64 = lpm_control(p32).astype(np.float64), lpm_control(lpm_params(np.float32(a32), np.float64))
            m["control"] = max(m["control"], float(np.max(np.abs(c32 - c64) / np.maximum(np.abs(c64), 1e-30))))
            for curve in CURVES:
                m["code"] = max(m["code"], _maxdiff(resolve(curve, img, np.float32, p32), resolve(curve, img, np.float64, lpm_params(np.float32(a32), np.float64))))
        for kind in BLOOM_KINDS:
            img = case(kind, w, h)
            down, up, _ = bloom_chain(img)
            for i in range(5):
                d32, n32, _ = downsample(down[i], np.float32)
                d64, n64, _ = downsample(down[i], np.float64)
                m["length"] = max(m["length"], _maxdiff(n32, n64))
                m["half_down"] = max(m["half_down"], _half_units(d32, d64))
        for i in range(4, 0, -1):
            src, dst = upsample_case(w, h, i)
            m["half_up"] = max(m["half_up"], _half_units(upsample(src, dst, np.float32), upsample(src, dst, np.float64)))
        img, level1 = blend_case(w, h)
        m["half_blend"] = max(m["half_blend"], _half_units(blend(img, level1, np.float32), blend(img, level1, np.float64)))
    _margins = {key: FACTOR * v for key, v in m.items()}
    return _margins


def _half_units(a32, a64):
    with np.errstate(over="ignore", invalid="ignore"):
        h = np.abs(a64).astype(np.float16)
        spacing = np.maximum(np.spacing(np.minimum(h, np.float16(65504.0))).astype(np.float64), 2.0 ** -24)
        d = np.abs(a32.astype(np.float64) - a64) / spacing
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


def fragile_bins(img, m=None):
    """Pixels whose float64 luminance is within the margin of the 0.005 cut, or whose bin value is within the margin of an integer (on the saturate's two
    plateaus the value is exactly 1 or 255 in both modes: not fragile)."""
    m = m or margins()
    lum, v, raw = bin_value(img, np.float64)
    with np.errstate(invalid="ignore"):
        near_cut = np.abs(lum - np.float64(np.float32(0.005))) <= m["lum"]
        near_step = (lum >= 0.005) & (raw > 0.0) & (raw < 1.0) & (np.abs(v - np.rint(v)) <= m["bin"])
    return near_cut | near_step


def fragile_codes(value, m=None):
    """Per channel: the float64 code value within the margin of an integer (the truncation's boundary)."""
    m = m or margins()
    with np.errstate(invalid="ignore"):
        return (np.abs(value - np.rint(value)) <= m["code"]) & (np.rint(value) >= 1) & (np.rint(value) <= 255)


def fragile_halves(value, stage, m=None):
    """Per channel: the float64 value within the margin of a half rounding boundary; stage is "down", "up" or "blend" (each store has its own margin)."""
    m = m or margins()
    return half_distance(value) <= m["half_" + stage]


def fragile_cut(length, m=None):
    m = m or margins()
    return np.abs(length - 1.0) <= m["length"]
