"""Anisotropic filtering, CPU side (`-m "not gpu"`): the reference of tests/aniso_ref.py held to the oracle's isotropic sampler and to cases whose
answer follows from the definition, so that it cannot hide a failure of the kernels it judges; and the C-ABI surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aniso_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


@pytest.fixture(scope="module")
def noise():
    """a 64 x 32 sRGB noise texture with its chain and a 100 x 60 UNORM one; wrap trilinear, clamp/mirror with a bias, all point"""
    rng = np.random.default_rng(11)
    tex = [dict(levels=aniso_ref.box_chain(rng.integers(0, 256, (32, 64, 4), dtype=np.uint8)), srgb=True),
           dict(levels=aniso_ref.box_chain(rng.integers(0, 256, (60, 100, 4), dtype=np.uint8)), srgb=False)]
    samplers = [(0, 0, 1, 1, 1, 0.0, 0.0, 1000.0), (2, 1, 1, 1, 1, 0.75, 0.0, 1000.0), (0, 0, 0, 0, 0, 0.0, 0.0, 1000.0)]
    sb, keep = aniso_ref.make_scene_buffers(tex, samplers)
    return aniso_ref.Sampler(sb), keep, [(64, 32), (100, 60)]


def test_isotropic_cases_are_the_oracles_sample_grad(noise):
    """A = 1 is orc_sample_grad bit for bit; so is any A where the two axes have exactly the same length (N = 1)."""
    sm, _, sizes = noise
    rng = np.random.default_rng(3)
    n = 600
    uv = rng.uniform(-2.0, 3.0, (n, 2)).astype(f32)
    ddx = (rng.normal(0, 1, (n, 2)) * np.exp2(rng.uniform(-9, -1, (n, 1)))).astype(f32)
    ddy = (rng.normal(0, 1, (n, 2)) * np.exp2(rng.uniform(-9, -1, (n, 1)))).astype(f32)
    for t, (w, h) in enumerate(sizes):
        for s in range(3):
            want = sm.sample_grad(t, s, uv, ddx, ddy)
            got, N = sm.sample_grad_aniso(t, s, w, h, uv, ddx, ddy, 1, return_n=True)
            assert (N == 1).all() and np.array_equal(_bits(got), _bits(want))
    # |dx| == |dy| exactly: the same vector, its negation, its components swapped on a square footprint in texels (64 x 32: (a, 2b) <-> (b, 2a) in uv)
    for A in (2, 5, 16):
        for ddy2 in (ddx, -ddx, np.stack([ddx[:, 1] * f32(0.5), ddx[:, 0] * f32(2.0)], 1)):
            got, N = sm.sample_grad_aniso(0, 0, 64, 32, uv, ddx, ddy2, A, return_n=True)
            assert (N == 1).all()
            assert np.array_equal(_bits(got), _bits(sm.sample_grad(0, 0, uv, ddx, ddy2)))


def test_tap_count_follows_the_ratio_of_the_axes():
    """Axis-aligned footprints with dyy / dxx = r: N = min(A, ceil(r)).  r = 4 and 16 are exact squares in fp32 (r^2 * dxx^2 == dyy^2 with no rounding for the
    power-of-two dxx used here): the definition's own comparison `n^2 * minor2 >= major2` decides them, n = r."""
    W = H = 64
    dxx = f32(2.0) ** -3      # texels
    for r in (1, 1.5, 2, 3.99, 4, 4.01, 16, 1000):
        ddx = np.array([[dxx / f32(W), 0.0]], dtype=f32)
        ddy = np.array([[0.0, f32(r) * dxx / f32(H)]], dtype=f32)
        for A in (1, 2, 5, 16, 0, 99):
            a = min(16, max(1, A))
            N, lod, m = aniso_ref.plan(W, H, ddx, ddy, A)
            assert int(N[0]) == min(a, int(np.ceil(r))), (r, A, int(N[0]))
            Nt, _, mt = aniso_ref.plan(W, H, ddy, ddx, A)      # the axes the other way round: same count, the major axis is still the long one
            assert int(Nt[0]) == int(N[0])
            if N[0] > 1:
                assert np.array_equal(m[0], ddy[0]) and np.array_equal(mt[0], ddy[0])
    # a zero minor axis: N = A;  zero gradients, NaN and out-of-range major axes: isotropic
    N, _, _ = aniso_ref.plan(W, H, np.array([[0.0, 0.0]], dtype=f32), np.array([[0.0, 0.01]], dtype=f32), 7)
    assert int(N[0]) == 7
    for g in (0.0, np.nan, np.inf, 1.0e18, 1.0e-22):
        N, _, _ = aniso_ref.plan(W, H, np.array([[g, 0.0]], dtype=f32), np.array([[0.0, 0.0]], dtype=f32), 16)
        assert int(N[0]) == 1, g


def test_level_of_detail_is_that_of_the_minor_axis_when_n_reaches_the_ratio():
    """lod = 0.5 * log2(major2) - log2(N): a footprint 8 x 1 texels with A = 16 is sampled at level 0, 32 x 4 at level 2 (powers of two: the polynomial is exact)"""
    for minor, want in ((1.0, 0.0), (4.0, 2.0)):
        N, lod, _ = aniso_ref.plan(128, 128, np.array([[minor / 128.0, 0.0]], dtype=f32), np.array([[0.0, 8.0 * minor / 128.0]], dtype=f32), 16)
        assert int(N[0]) == 8 and float(lod[0]) == want


def test_stripes_seen_along_their_length_keep_their_contrast():
    """A derived exact case.  64 x 64 vertical stripes, 2 texels on, 2 off, the chain 2x2 box averages: levels >= 2 are one grey.  Wrap, linear / linear /
    linear; a footprint of 1 texel along u and 16 along v.  A = 1 samples level 4: the grey, for every u.  A = 16: N = 16, lod = 0, and the sixteen taps
    differ in v only, where the stripes do not vary, so all sixteen are the one value x = orc_sample_level(uv, 0).  The running sums 2x, 3x .. 16x are exact
    when x has at most 20 significant bits, and * 0.0625f always is: with u on a sixteenth-of-a-texel grid (x = q / 16 or 1 - q / 16) every sample IS
    orc_sample_level(uv, 0) bit for bit.  For any other u the sums k * x round (3x needs up to two bits more than x), so there the sample is the rounded
    sum of sixteen copies of the oracle's x, stated here in float32 from the oracle's value, and within 16 half-ulps of it."""
    x = np.arange(64)
    row = np.where((x // 2) % 2 == 0, 255, 0).astype(np.uint8)
    level0 = np.repeat(np.repeat(row[None, :, None], 64, 0), 4, 2)
    chain = aniso_ref.box_chain(level0)
    assert len(chain) == 7 and all(len(np.unique(l)) == 1 for l in chain[2:])
    sb, keep = aniso_ref.make_scene_buffers([dict(levels=chain, srgb=False)], [(0, 0, 1, 1, 1, 0.0, 0.0, 1000.0)])
    sm = aniso_ref.Sampler(sb)
    n = 512
    rng = np.random.default_rng(2)
    grid_u = ((16 * rng.integers(-64, 128, n) + 8 + rng.integers(0, 16, n)) / 1024.0).astype(f32)      # u * 64 - 0.5 = j + q / 16, exactly
    ddx = np.tile(np.array([[1.0 / 64.0, 0.0]], dtype=f32), (n, 1))
    ddy = np.tile(np.array([[0.0, 16.0 / 64.0]], dtype=f32), (n, 1))
    grey = f32(chain[4][0, 0, 0]) / f32(255.0)
    for u, exact in ((grid_u, True), (rng.uniform(-1.0, 2.0, n).astype(f32), False)):
        uv = np.stack([u, rng.uniform(-1.0, 2.0, n).astype(f32)], 1)
        iso = sm.sample_grad_aniso(0, 0, 64, 64, uv, ddx, ddy, 1)
        assert np.array_equal(_bits(iso), _bits(np.full((n, 4), grey, dtype=f32)))
        got, N = sm.sample_grad_aniso(0, 0, 64, 64, uv, ddx, ddy, 16, return_n=True)
        assert (N == 16).all()
        want = sm.sample_level(0, 0, uv, np.zeros(n, dtype=f32))
        assert len(np.unique(want[:, 0])) > 8 and want[:, 0].min() == 0.0 and want[:, 0].max() == 1.0      # the stripes are there
        if exact:
            assert np.array_equal(_bits(got), _bits(want))
        else:
            acc = want.copy()
            for _ in range(15):
                acc = acc + want
            assert np.array_equal(_bits(got), _bits(acc * f32(0.0625)))
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 16 * 2.0 ** -24 * np.abs(want.astype(np.float64))).all()


def test_abi_exports_the_anisotropy_entry_points():
    from basicrenderer_amd import capi
    header = open(os.path.join(ROOT, "include", "brmi.h")).read()
    names = ("brmi_set_sampler_anisotropy", "brmi_debug_sample_grad")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.BRMI_EXPORTS
    lib_path = os.path.join(ROOT, "basicrenderer_amd", "lib", "libbrmi.so")
    if not os.path.exists(lib_path):
        pytest.skip("libbrmi.so not built")
    lib = C.CDLL(lib_path)      # (loading it needs no GPU)
    for name in names:
        assert hasattr(lib, name), f"libbrmi.so does not export {name}"
