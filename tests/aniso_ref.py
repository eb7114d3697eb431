"""The anisotropic SampleGrad of DESIGN.md 4.7, restated for tests in numpy float32 from the written definition.

Steps 1-4 and 6 (squared axis lengths, fallback, tap count, level of detail, the sum) are float32 arithmetic here; the taps of step 5 are the
oracle's SampleLevel (`orc_sample_level`) and the isotropic fallback is the oracle's SampleGrad (`orc_sample_grad`).  Nothing comes from the
library under test.  Every float32 operation is a single numpy operation on float32 operands: correctly rounded, never fused.
"""
import ctypes as C

import numpy as np

f32 = np.float32
MIN_NORMAL = f32(1.17549435e-38)
MAX_MAJOR2 = f32(3.0e38)


def log2_poly(x):
    """exponent + degree-5 polynomial of the mantissa, Horner from the innermost term, float32"""
    x = np.ascontiguousarray(x, dtype=f32)
    b = x.view(np.uint32)
    e = ((b >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int32) - 127
    t = ((b & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(f32) - f32(1.0)
    p = t * f32(0.05827096104621887)
    for c in (-0.2247820496559143, 0.44070422649383545, -0.7168022990226746, 1.442609190940857):
        p = t * (f32(c) + p)
    return e.astype(f32) + p


def clamp_anisotropy(a):
    return np.clip(np.asarray(a, dtype=np.int64), 1, 16)


def plan(width, height, ddx, ddy, A):
    """Steps 1-4 for n samples: (N, lod, major axis in uv units).  N == 1 marks the samples that are today's SampleGrad (A == 1, a NaN axis, major2 out
    of range, or no n > 1 needed); their lod / axis entries are not used."""
    ddx, ddy = np.ascontiguousarray(ddx, dtype=f32), np.ascontiguousarray(ddy, dtype=f32)
    A = np.broadcast_to(clamp_anisotropy(A), (len(ddx),))
    W, H = f32(width), f32(height)
    with np.errstate(all="ignore"):
        dxx, dxy, dyx, dyy = ddx[:, 0] * W, ddx[:, 1] * H, ddy[:, 0] * W, ddy[:, 1] * H
        lx2, ly2 = dxx * dxx + dxy * dxy, dyx * dyx + dyy * dyy
        x_major = lx2 >= ly2
        major2, minor2 = np.where(lx2 > ly2, lx2, ly2), np.where(lx2 < ly2, lx2, ly2)
        iso = (A == 1) | np.isnan(lx2) | np.isnan(ly2) | ~(major2 >= MIN_NORMAL) | ~(major2 <= MAX_MAJOR2)
        N = A.copy()
        for n in range(16, 0, -1):      # the smallest n in [1, A] that satisfies the comparison; A if none does
            ok = (n <= A) & (f32(n * n) * minor2 >= major2)
            N = np.where(ok, n, N)
        N = np.where(iso, 1, N)
        lod = f32(0.5) * log2_poly(np.where(iso, f32(1.0), major2)) - log2_poly(N.astype(f32))
    m = np.where(x_major[:, None], ddx, ddy)
    return N, lod, m


class Sampler:
    """A host scene's texture / sampler tables behind the oracle's two sampler hooks."""

    def __init__(self, sb):
        import orc
        self.sb, self.lib = sb, orc.lib()

    def sample_level(self, t, s, uv, lod):
        uv, lod = np.ascontiguousarray(uv, dtype=f32), np.ascontiguousarray(lod, dtype=f32)
        out = np.zeros((len(uv), 4), dtype=f32)
        self.lib.orc_sample_level(C.byref(self.sb), C.c_uint32(t), C.c_uint32(s), uv.ctypes.data_as(C.c_void_p), lod.ctypes.data_as(C.c_void_p), C.c_uint64(len(uv)), out.ctypes.data_as(C.c_void_p))
        return out

    def sample_grad(self, t, s, uv, ddx, ddy):
        uv, ddx, ddy = (np.ascontiguousarray(a, dtype=f32) for a in (uv, ddx, ddy))
        out = np.zeros((len(uv), 4), dtype=f32)
        self.lib.orc_sample_grad(C.byref(self.sb), C.c_uint32(t), C.c_uint32(s), uv.ctypes.data_as(C.c_void_p), ddx.ctypes.data_as(C.c_void_p), ddy.ctypes.data_as(C.c_void_p), C.c_uint64(len(uv)), out.ctypes.data_as(C.c_void_p))
        return out

    def sample_grad_aniso(self, t, s, width, height, uv, ddx, ddy, A, return_n=False):
        """Steps 1-6.  width / height: level 0 of texture `t`.  An unbound slot reads opaque white through both hooks."""
        uv, ddx, ddy = (np.ascontiguousarray(a, dtype=f32) for a in (uv, ddx, ddy))
        N, lod, m = plan(width, height, ddx, ddy, A)
        out = self.sample_grad(t, s, uv, ddx, ddy)              # N == 1: today's SampleGrad, bit for bit
        for n in np.unique(N[N > 1]):
            sel = np.flatnonzero(N == n)
            fn = f32(n)
            acc = None
            for i in range(int(n)):
                ti = (f32(i) + f32(0.5)) / fn - f32(0.5)
                uvi = uv[sel] + m[sel] * ti
                tap = self.sample_level(t, s, uvi, lod[sel])
                acc = tap if acc is None else acc + tap
            out[sel] = acc * (f32(1.0) / fn)
        return (out, N) if return_n else out


def make_scene_buffers(textures, samplers):
    """A host SceneBuffers holding only what the sampler reads.  textures: list of dict(levels=[uint8 array (h, w, 4), ...], srgb=bool), the chain in the
    scene library's layout (levels tightly packed, mipOffset in texels); samplers: list of (addressU, addressV, min, mag, mip, bias, minLod, maxLod).
    Returns (sb, arrays): arrays = dict(texels, descs (texel field = byte offset), samplers, srgb), kept alive by the caller."""
    from basicrenderer_amd import capi
    blob, descs = [], np.zeros((len(textures), 24), dtype=np.uint32)
    offset = 0
    for k, tx in enumerate(textures):
        h, w = tx["levels"][0].shape[:2]
        descs[k, 0], descs[k, 1] = offset & 0xFFFFFFFF, offset >> 32
        descs[k, 2:6] = (w, h, len(tx["levels"]), 1 if tx.get("srgb") else 0)
        at = 0
        for l, lv in enumerate(tx["levels"]):
            assert lv.shape == (max(1, h >> l), max(1, w >> l), 4) and lv.dtype == np.uint8
            descs[k, 6 + l] = at
            at += lv.shape[0] * lv.shape[1]
            blob.append(lv.reshape(-1))
        offset += at * 4
    texels = np.ascontiguousarray(np.concatenate(blob))
    samp = np.zeros((len(samplers), 8), dtype=np.uint32)
    for k, s in enumerate(samplers):
        samp[k, :5] = s[:5]
        samp[k, 5:8] = np.array(s[5:8], dtype=f32).view(np.uint32)
    c = np.arange(256, dtype=np.float64) / 255.0
    srgb = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(f32)
    host = descs.copy()
    ptr = host.view(np.uint64).reshape(len(textures), 12)
    ptr[:, 0] += np.uint64(texels.ctypes.data)
    sb = capi.SceneBuffers()
    sb.textures, sb.textureCount = host.ctypes.data, len(textures)
    sb.samplers, sb.samplerCount = samp.ctypes.data, len(samplers)
    sb.srgbToLinear = srgb.ctypes.data
    return sb, dict(texels=texels, descs=descs, host_descs=host, samplers=samp, srgb=srgb)


def box_chain(level0, levels=None):
    """2x2 box averages (rounded to nearest) down to 1x1, or `levels` levels"""
    out = [np.ascontiguousarray(level0, dtype=np.uint8)]
    while (out[-1].shape[0] > 1 or out[-1].shape[1] > 1) and (levels is None or len(out) < levels):
        a = out[-1].astype(np.uint32)
        h, w = a.shape[:2]
        nh, nw = max(1, h >> 1), max(1, w >> 1)
        ys, xs = np.minimum(np.arange(nh) * 2, h - 1), np.minimum(np.arange(nw) * 2, w - 1)
        ys1, xs1 = np.minimum(ys + 1, h - 1), np.minimum(xs + 1, w - 1)
        s = a[ys][:, xs] + a[ys][:, xs1] + a[ys1][:, xs] + a[ys1][:, xs1]
        out.append(((s + 2) // 4).astype(np.uint8))
    return out
