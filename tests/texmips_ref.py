"""Texture mip chains, restated in numpy from the reference's shader text: Utilities/mipmapping.hlsl over FidelityFX/ffx_spd.h (the Float4, non-array
variant of MipmapCSMain), Utilities/alphaCoverageMipmapping.hlsl and the job loop of TextureFactory.cpp.  No call into any library of this
repository.  fp32 with the shaders' operand order wherever bytes depend on it; float64 beside that for the one transcendental, the sRGB encode.

What the text says, as restated here:
  * level sizes max(1, w >> l) x max(1, h >> l), tightly packed RGBA8;
  * SpdLoadSourceImage clamps to the image; a source texel is code / 255 (fp32), rgb of an sRGB texture through the 256-entry decode table (the view's
    format decodes: DESIGN.md 2);
  * SpdReduce4 is ((v0 + v1) + v2) + v3) * 0.25f.  The four loads of SpdReduceLoadSourceImage and of SpdReduceLoad4 come in the order (0,0) (0,1) (1,0) (1,1)
    of (x, y) -- y first; SpdReduceQuad reads lanes quad|0..3, which ARmpRed8x8 lays out (0,0) (1,0) (0,1) (1,1) -- x first.  So levels 1 and 7 add y first,
    every other level x first;
  * levels 1..6 of a 64 x 64 tile come from fp32 intermediates; every thread of a tile computes, whether or not its texel is inside the level, and a store
    outside the level is dropped;
  * level 6 is stored; levels 7.. start from SpdLoad of the STORED level 6: code / 255 with no decode (an sRGB chain is encoded a second time from there
    on: the text's behaviour, kept), over the 64 x 64 region the last workgroup reads; levels 8.. come from fp32 intermediates again.  SpdLoad does not
    clamp, and what a typed UAV load gives outside the level is the API's business (zero on the reference's: the last levels of every texture that is not a
    power-of-two square would darken by halves).  Restatement decision: the re-read clamps to the level as SpdLoadSourceImage clamps to the image;
  * EncodeForOutput applies LinearToSrgb to rgb with the flag; the store is UNORM8: (uint)(saturate(x) * 255 + 0.5).

The sRGB encode is the only inexact step: pow(c, 1/2.4) differs in the last place between a GPU and libm.  encode_codes() returns, beside the codes, which
texels are DECIDED: the float64 value before rounding is farther than ENCODE_BOUND from a rounding cut.  Decided texels must match bit for bit, the others
may differ by one code.  Linear chains, alpha channels, statistics words and scales are exact.
"""
import numpy as np

f32 = np.float32
MAX_MIPS = 16
STATS_WORDS = 260
PREV_COVERED, PREV_TOTAL, DST_TOTAL, HIST_BASE = 0, 1, 2, 3

# ---- the bound of the encode, from the fp32 error of its operations (in units of one 8-bit code) ----------------------------------------------------------
# hi = 1.055f * pow(c, 1/2.4f) - 0.055f; lerp(lo, hi, 1) = lo + (hi - lo); store = x * 255 + 0.5.  u = 2^-24 is the relative error of one fp32 rounding.
#   pow as exp2(y * log2(c)) (HLSL) or the device library's powf: with c >= 0.0031308, |y * log2 c| <= 8.32 / 2.4 < 3.5.  log2 (<= 2 ulp = 4u relative), the
#   product's rounding (u): the exponent is off by at most 3.5 * 5u absolute, which is 3.5 * 5u * ln 2 < 12.2u relative in the power; exp2 adds <= 2 ulp = 4u.
#   pow <= 1, so: pow 16.2u, times 1.055f (u * 1.055), minus 0.055f (u), hi - lo (u), lo + .. (u), lo itself (u), * 255 (u), + 0.5 (u at 256: 2u of 128..256)
#   every term relative to a value <= 1.055 (or, after * 255, <= 256):
_U = 2.0 ** -24
ENCODE_BOUND = (16.2 * 1.055 + 1.055 + 4.0) * _U * 255.0 + 3.0 * _U * 256.0      # ~ 3.8e-4 of a code
_C_EDGE, _C_LO, _C_A, _C_B, _C_P = (float(f32(x)) for x in (0.0031308, 12.92, 1.055, 0.055, f32(1.0) / f32(2.4)))


def srgb_table():
    """The scene's 256-entry decode table (scene_gen.cpp: float64 formula, rounded to fp32)."""
    x = np.arange(256, dtype=np.float64) / 255.0
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4).astype(f32)


def level_sizes(w, h, mips):
    return [(max(1, w >> l), max(1, h >> l)) for l in range(mips)]


def full_mip_count(w, h):
    return int(max(w, h)).bit_length()


def mip_offsets(w, h, mips):
    """Texel offsets of a tightly packed chain, and its total texel count."""
    offs, o = [], 0
    for lw, lh in level_sizes(w, h, mips):
        offs.append(o); o += lw * lh
    return offs, o


def unorm_decode(codes):
    return codes.astype(f32) / f32(255.0)


def unorm_store(x):
    """(uint)(saturate(x) * 255.0f + 0.5f) in fp32."""
    x = np.asarray(x, f32)
    return (np.clip(x, f32(0), f32(1)) * f32(255.0) + f32(0.5)).astype(np.uint32).astype(np.uint8)


def encode_codes(v, srgb):
    """fp32 RGBA (.., 4) -> (uint8 codes, decided mask).  Alpha and linear rgb are exact (decided everywhere)."""
    v = np.asarray(v, f32)
    codes = unorm_store(v)
    decided = np.ones(v.shape, bool)
    if srgb:
        c = np.clip(v[..., :3], f32(0), f32(1)).astype(np.float64)
        hi = _C_A * np.power(c, _C_P) - _C_B
        e = np.where(v[..., :3] >= f32(0.0031308), hi, c * _C_LO)      # step(edge, c): the fp32 comparison, exact on both sides
        t = np.clip(e, 0.0, 1.0) * 255.0 + 0.5
        codes[..., :3] = np.floor(t).astype(np.uint8)
        decided[..., :3] = np.abs(t - np.round(t)) > ENCODE_BOUND
    return codes, decided


def _reduce(a, y_first):
    """SpdReduce4 over the 2x2 blocks of an (H, W, 4) fp32 array; operand order per the header."""
    v00, v10, v01, v11 = a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2]       # v<x><y>
    s = ((v00 + v01) + v10) + v11 if y_first else ((v00 + v10) + v01) + v11
    return (s * f32(0.25)).astype(f32)


def plain_chain(level0, srgb, mips, table=None):
    """level0: (h, w, 4) uint8.  Returns (levels, decided): lists of (h_l, w_l, 4) arrays for l = 0 .. mips - 1 (level 0 as given)."""
    h, w = level0.shape[:2]
    assert 1 <= mips <= min(MAX_MIPS, full_mip_count(w, h), 13)
    table = srgb_table() if table is None else table
    src = unorm_decode(level0)
    if srgb:
        src[..., :3] = table[level0[..., :3]]
    sizes = level_sizes(w, h, mips)
    levels, decided = [level0.copy()], [np.ones(level0.shape, bool)]
    tx, ty = (w + 63) // 64, (h + 63) // 64
    ix, iy = np.minimum(np.arange(64 * tx), w - 1), np.minimum(np.arange(64 * ty), h - 1)
    cur = src[iy][:, ix]                                     # every tile's 64 x 64 loads, clamped to the image

    def store(v, l):
        lw, lh = sizes[l]
        c, d = encode_codes(v[:lh, :lw], srgb)
        levels.append(c); decided.append(d)

    for l in range(1, min(mips, 7)):
        cur = _reduce(cur, y_first=(l == 1))
        store(cur, l)
    if mips > 7:
        w6, h6 = sizes[6]
        jx, jy = np.minimum(np.arange(64), w6 - 1), np.minimum(np.arange(64), h6 - 1)
        cur = unorm_decode(levels[6])[jy][:, jx]             # SpdLoad(imgDst5): the stored codes, no decode; clamped to the level
        for l in range(7, mips):
            cur = _reduce(cur, y_first=(l == 7))
            store(cur, l)
    return levels, decided


# ---- alphaCoverageMipmapping.hlsl -------------------------------------------------------------------------------------------------------------------------
def resolve_scale(stats):
    """AlphaMipResolveScaleCS on the 260 words of one level."""
    prev_total, prev_covered, dst_total = int(stats[PREV_TOTAL]), int(stats[PREV_COVERED]), int(stats[DST_TOTAL])
    if prev_total == 0 or dst_total == 0 or prev_covered == 0:
        return f32(1.0)
    target_coverage = f32(prev_covered) / f32(prev_total)
    target = min(dst_total, max(1, int(np.rint(target_coverage * f32(dst_total)))))       # HLSL round: half to even
    acc, selected = 0, 255
    for b in range(255, 0, -1):
        acc += int(stats[HIST_BASE + b])
        if acc >= target:
            selected = b
            break
    alpha = max(f32(selected) / f32(255.0), f32(1.0) / f32(255.0))
    return f32(min(max(f32(0.55) / alpha, f32(0.25)), f32(16.0)))


def _dilated_rgb(rgb, a):
    """DilatedRgb for every texel of a level (rgb, a: decoded fp32, (h, w, 3) and (h, w))."""
    h, w = a.shape
    out = rgb.copy()
    for y, x in zip(*np.nonzero(a < f32(0.5))):
        best_a, best = a[y, x], rgb[y, x]
        done = False
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)
                if a[qy, qx] > best_a:
                    best_a, best = a[qy, qx], rgb[qy, qx]
                if a[qy, qx] >= f32(0.5):
                    best, done = rgb[qy, qx], True
                    break
            if done:
                break
        out[y, x] = best
    return out


def alpha_chain(level0, srgb, mips, table=None):
    """Returns (levels, decided, stats, scales): stats uint32 (mips * 260), scales fp32 (mips); words of level 0 are not written (returned as zero)."""
    h, w = level0.shape[:2]
    assert 1 <= mips <= min(MAX_MIPS, full_mip_count(w, h))
    table = srgb_table() if table is None else table
    sizes = level_sizes(w, h, mips)
    levels, decided = [level0.copy()], [np.ones(level0.shape, bool)]
    stats, scales = np.zeros(mips * STATS_WORDS, np.uint32), np.zeros(mips, f32)
    for l in range(1, mips):
        prev = levels[l - 1]
        (sw, sh), (dw, dh) = sizes[l - 1], sizes[l]
        val = unorm_decode(prev)
        if srgb:
            val[..., :3] = table[prev[..., :3]]
        dil = _dilated_rgb(val[..., :3], val[..., 3])
        ix, iy = np.minimum(np.arange(2 * dw), sw - 1), np.minimum(np.arange(2 * dh), sh - 1)      # LoadSource clamps
        inx, iny = np.arange(2 * dw) < sw, np.arange(2 * dh) < sh
        rgb, a = dil[iy][:, ix], val[..., 3][iy][:, ix]
        inb = iny[:, None] & inx[None, :]
        rgb_sum, a_sum = np.zeros((dh, dw, 3), f32), np.zeros((dh, dw), f32)
        for oy in range(2):
            for ox in range(2):
                rgb_sum = rgb_sum + rgb[oy::2, ox::2]
                a_sum = a_sum + a[oy::2, ox::2]
        out = np.concatenate([rgb_sum * f32(0.25), (a_sum * f32(0.25))[..., None]], axis=2).astype(f32)
        s = stats[l * STATS_WORDS:(l + 1) * STATS_WORDS]
        s[PREV_TOTAL] = inb.sum()
        s[PREV_COVERED] = (inb & (a >= f32(0.5))).sum()
        s[DST_TOTAL] = dw * dh
        bins = np.minimum(255, np.rint(np.clip(out[..., 3], f32(0), f32(1)) * f32(255.0)).astype(np.int64))
        s[HIST_BASE:HIST_BASE + 256] = np.bincount(bins.ravel(), minlength=256)
        codes, dec = encode_codes(out, srgb)
        scales[l] = resolve_scale(s)
        codes[..., 3] = unorm_store(np.clip(unorm_decode(codes[..., 3]) * scales[l], f32(0), f32(1)))      # AlphaMipApplyScaleCS
        levels.append(codes); decided.append(dec)
    return levels, decided, stats, scales


def pack(levels):
    return np.concatenate([l.reshape(-1, 4) for l in levels])


def assert_mostly_decided(decided, limit=0.01):
    """The restatement's own condition on a test input: undecided texels are at most 1 % of each level."""
    for l, d in enumerate(decided):
        und = int((~d.all(axis=-1)).sum())
        assert und <= limit * d.shape[0] * d.shape[1], f"level {l}: {und} of {d.shape[0] * d.shape[1]} texels within the encode's bound of a rounding cut"


def assert_chain_matches(got, levels, decided, what=""):
    """got: list of (h_l, w_l, 4) uint8.  Decided channels bit for bit, the others within one code."""
    for l, (g, r, d) in enumerate(zip(got, levels, decided)):
        assert g.shape == r.shape, f"{what} level {l}: shape {g.shape} != {r.shape}"
        diff = np.abs(g.astype(np.int32) - r.astype(np.int32))
        bad = (d & (diff != 0)) | (diff > 1)
        assert not bad.any(), f"{what} level {l}: {int(bad.sum())} channel values differ (first at {np.argwhere(bad)[0].tolist()}: {g[tuple(np.argwhere(bad)[0])]} vs {r[tuple(np.argwhere(bad)[0])]})"


# ---- the test inputs (fixed seeds; chosen so that assert_mostly_decided holds) ---------------------------------------------------------------------------
def noise_image(w, h, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


# (w, h, mipCount, seed) of the plain-chain shape tests: nothing to build; an odd size on the clamp; a column; exactly one tile; a tile edge on a non-square
# image; several workgroups and the re-read of the stored level 6; a chain shorter than the size allows
PLAIN_CASES = [(1, 1, 1, 100), (2, 2, 2, 101), (5, 3, 3, 102), (1, 37, 6, 103), (64, 64, 7, 104), (65, 33, 7, 105), (130, 70, 8, 106), (256, 256, 4, 107)]


def soft_holes(w, h, pitch=16, seed=7):
    """Round holes with a soft rim, radius growing across the image: level-1 alphas land on many bins, exact halves among them.  (The GPU comparison takes
    these and not hard-edged holes: a hard mask gives level 1 five bins and no exact half, so the histogram, the half-to-even rounding and the scan would
    hardly be exercised; the hard-edged holes are in test_texmips_cpu.py, where the coverage property is about them.)"""
    rng = np.random.default_rng(seed)
    img = rng.integers(32, 224, (h, w, 4), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    r = 2.0 + 5.0 * (x / max(1, w - 1)) * (0.5 + 0.5 * y / max(1, h - 1))
    d = np.hypot((x % pitch) - (pitch - 1) / 2.0, (y % pitch) - (pitch - 1) / 2.0)
    img[..., 3] = np.rint(np.clip((d - r) * 0.8 + 0.5, 0.0, 1.0) * 255.0)
    return img


def alpha_inputs():
    """The alpha-chain inputs.  The resolve's clamps cannot be reached by an image: a covered source texel (code >= 128) puts its destination texel at bin >= 32
    and the target never exceeds the number of such destination texels, so the selected bin is >= 32 (scale <= 0.55 * 255 / 32 < 4.39) whenever the scan
    succeeds, and 0.55 / selectedAlpha >= 0.55 always.  scale_high and scale_low are the two extremes an image does reach."""
    rng = np.random.default_rng(21)
    opaque = rng.integers(0, 256, (16, 16, 4), dtype=np.uint8); opaque[..., 3] = 255
    transparent = rng.integers(0, 256, (32, 32, 4), dtype=np.uint8); transparent[..., 3] = rng.integers(0, 128, (32, 32))
    high = rng.integers(0, 256, (16, 16, 4), dtype=np.uint8); high[..., 3] = 0; high[5, 9, 3] = 128
    return {"holes": soft_holes(64, 64), "odd": noise_image(37, 21, 108), "opaque": opaque, "transparent": transparent, "scale_high": high, "scale_low": opaque[:4, :4].copy()}
