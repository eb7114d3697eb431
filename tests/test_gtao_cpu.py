"""XeGTAO without a GPU: the C ABI's structs, exports and layout; the numpy restatement's own anchors; and -- from the float64 side alone -- the
fragile share of every input tests/test_gtao_gpu.py uses (cap: 5 % of the covered pixels; a scene that exceeds it is changed, not the cap) and the margin M.

    python tests/test_gtao_cpu.py      writes the measured shares and M to profiles/gtao_accuracy.md
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gtao_ref as g      # noqa: E402

FRAGILE_CAP = 0.05
_scenes = {}


def camera_of(width, height):
    """The camera of the pass the GPU tests create for a frame of this size (the tiny preset's; host-side scene library only)."""
    if (width, height) not in _scenes:
        from basicrenderer_amd import Scene
        _scenes[(width, height)] = Scene("tiny", width, height, point_lights=2)
    return _scenes[(width, height)].camera_host()


def test_struct_sizes_and_exports():
    from basicrenderer_amd import capi
    assert C.sizeof(capi.GtaoSettings) == 32 and C.sizeof(capi.GtaoPlane) == 16 and C.sizeof(capi.GtaoLayout) == 144 and C.sizeof(capi.GtaoBuffers) == 72
    assert capi.GtaoBuffers.settings.offset == 8 and capi.GtaoBuffers.scratch.offset == 40 and capi.GtaoBuffers.aoTerm.offset == 56
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "brmi.h")).read()
    for name in ("brmi_gtao_default_settings", "brmi_gtao_get_layout", "brmi_set_gtao", "brmi_gtao_prefilter", "brmi_gtao_main", "brmi_gtao_denoise"):
        assert name in capi.BRMI_EXPORTS and name + "(" in header
    assert "brmi_gtao_settings" in header and "brmi_gtao_layout" in header and "brmi_gtao_buffers" in header


def _library():
    from basicrenderer_amd import capi
    return capi.brmi_lib(), capi


FAKE = 0x10000      # a non-null, 16 B aligned "device" address: every call below is refused, or stores the pointer, before anything could read it


def _buffers(capi, lib, width, height, **over):
    lay = capi.GtaoLayout()
    assert lib.brmi_gtao_get_layout(width, height, C.byref(lay)) == 0
    b = capi.GtaoBuffers()
    b.structSize = C.sizeof(capi.GtaoBuffers)
    lib.brmi_gtao_default_settings(C.byref(b.settings))
    b.scratch, b.scratchBytes, b.aoTerm, b.aoTermBytes = FAKE, lay.scratchBytes, FAKE * 2, lay.outputBytes
    for k, v in over.items():
        setattr(b.settings if k in ("qualityLevel", "denoisePasses", "radius", "maxDepthLod") else b, k, v)
    return b


def test_set_gtao_refusals_need_no_device():
    """Every refusal of brmi_set_gtao is host state; a good binding is kept; the stages answer BRMI_ERR_STATE before setup."""
    lib, capi = _library()
    INVALID, STATE = -1, -4

    def make(**cfg_over):
        cfg = capi.Config()
        lib.brmi_default_config(C.byref(cfg), 64, 32)
        for k, v in cfg_over.items():
            setattr(cfg, k, v)
        h = capi.vp()
        assert lib.brmi_create(C.byref(cfg), C.byref(h)) == 0
        return h
    h = make()
    try:
        assert lib.brmi_set_gtao(h, C.byref(_buffers(capi, lib, 64, 32))) == 0
        assert lib.brmi_set_gtao(h, None) == 0
        for over in (dict(structSize=71), dict(qualityLevel=4), dict(denoisePasses=4), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
                     dict(maxDepthLod=5), dict(scratch=None), dict(aoTerm=None), dict(scratch=FAKE + 8), dict(aoTerm=FAKE + 4)):
            assert lib.brmi_set_gtao(h, C.byref(_buffers(capi, lib, 64, 32, **over))) == INVALID, over
        b = _buffers(capi, lib, 64, 32); b.scratchBytes -= 1
        assert lib.brmi_set_gtao(h, C.byref(b)) == INVALID
        b = _buffers(capi, lib, 64, 32); b.aoTermBytes -= 1
        assert lib.brmi_set_gtao(h, C.byref(b)) == INVALID
        b = _buffers(capi, lib, 64, 32); b.settings.structSize = 28
        assert lib.brmi_set_gtao(h, C.byref(b)) == INVALID
        for stage in (lib.brmi_gtao_prefilter, lib.brmi_gtao_main, lib.brmi_gtao_denoise):
            assert stage(h, None) == STATE
    finally:
        lib.brmi_destroy(h)
    for cfg_over in (dict(bandY0=8, bandY1=24), dict(bandY1=16), dict(dynamicBand=1), dict(height=16, stripeRows=16, stripeCount=2, stripeIndex=0, fullHeight=32)):
        h = make(**cfg_over)
        try:
            assert lib.brmi_set_gtao(h, C.byref(_buffers(capi, lib, 64, 16 if "height" in cfg_over else 32))) == INVALID, cfg_over
            assert b"band" in lib.brmi_last_error(h)
        finally:
            lib.brmi_destroy(h)


@pytest.mark.parametrize("size,widths", [((101, 53), [101, 51, 26, 13, 7]), ((16, 16), [16, 8, 4, 2, 1]), ((1, 1), [1, 1, 1, 1, 1])])
def test_layout_against_the_size_formulas(size, widths):
    lib, capi = _library()
    W, H = size
    lay = capi.GtaoLayout()
    assert lib.brmi_gtao_get_layout(W, H, C.byref(lay)) == 0
    tiles = lambda w, h: ((w + 7) // 8) * ((h + 7) // 8) * 64
    end = 0
    planes = [(lay.depth[m], 4) for m in range(5)] + [(lay.edges, 1), (lay.term[0], 1), (lay.term[1], 1)]
    for m in range(5):
        assert (lay.depth[m].width, lay.depth[m].height) == (g.mip_size(W, m), g.mip_size(H, m)) and lay.depth[m].width == widths[m]
    for p in (lay.edges, lay.term[0], lay.term[1]):
        assert (p.width, p.height) == (W, H)
    for p, bpp in planes:      # in order, 16 B aligned, not overlapping, inside the scratch
        assert p.offset % 16 == 0 and p.offset >= end
        end = p.offset + tiles(p.width, p.height) * bpp
    assert lay.scratchBytes >= end and lay.outputBytes == tiles(W, H)
    assert lib.brmi_gtao_get_layout(0, 4, C.byref(lay)) != 0 and lib.brmi_gtao_get_layout(4, 4, None) != 0
    s = capi.GtaoSettings()
    lib.brmi_gtao_default_settings(C.byref(s))
    assert (s.structSize, s.qualityLevel, s.denoisePasses, s.maxDepthLod) == (32, 2, 1, 0) and s.radius == 0.5


def test_hilbert_index_is_a_bijection():
    y, x = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    idx = g.hilbert_index(x, y)
    assert sorted(idx.ravel().tolist()) == list(range(4096))
    assert (g.hilbert_index(x + 64, y + 128) == idx).all()      # only the low six bits take part
    # a Hilbert curve: consecutive indices are neighbouring pixels
    order = np.argsort(idx.ravel())
    step = np.abs(np.diff(x.ravel()[order])) + np.abs(np.diff(y.ravel()[order]))
    assert (step == 1).all()


def test_fast_acos_within_its_published_error():
    """XeGTAO_FastACos is Lagarde's degree-1 fit acos(x) ~ (-0.156583 x + pi / 2) sqrt(1 - x), x >= 0, with the square root replaced by the bit trick.
      * the fit with an exact square root: Lagarde publishes a maximum error of 9.0e-3 rad (the figure is rounded to two digits: anything below 9.05e-3);
      * the bit trick: its relative error repeats with every factor of 4 of the operand (the exponent's low bit and the mantissa are all it looks at), so
        its maximum R is found by evaluating every fp32 pattern of [1, 4) -- an enumeration, not a sample;
      * together: fast = fit * (1 + r), |r| <= R, and fit <= acos + 9.05e-3 <= pi / 2 + 9.05e-3 on [0, 1], so
        |fast - acos| <= 9.05e-3 + (pi / 2 + 9.05e-3) * R; the branch for x < 0 is pi - fast(|x|) and has the same error."""
    x = np.linspace(-1, 1, 20001)
    a = np.abs(x)
    fit = (np.float64(np.float32(-0.156583)) * a + np.float64(np.float32(1.570796))) * np.sqrt(1.0 - a)
    fit = np.where(x >= 0, fit, np.float64(np.float32(3.141593)) - fit)
    published = 9.05e-3
    assert np.abs(fit - np.arccos(x)).max() < published, np.abs(fit - np.arccos(x)).max()
    every = np.arange(0x3F800000, 0x40800000, dtype=np.uint32).view(np.float32)      # [1, 4)
    R = float(np.abs(g.fast_sqrt(every).astype(np.float64) / np.sqrt(every.astype(np.float64)) - 1.0).max())
    assert 0.03 < R < 0.05, R      # (the trick is a few per cent off, not exact and not broken)
    err = np.abs(g.fast_acos(x) - np.arccos(x))
    assert err.max() <= published + (math.pi / 2 + published) * R, (err.max(), R)
    assert np.abs(g.fast_acos(x.astype(np.float32)).astype(np.float64) - g.fast_acos(x)).max() < 1e-5


def _flat(width, height, depth_value):
    depth = np.full((height, width), depth_value, dtype=np.float32)
    normals = np.zeros((height, width, 3), dtype=np.float32); normals[..., 2] = 1.0
    return depth, normals


def test_flat_plane_facing_the_eye_is_unoccluded():
    """A plane at constant view depth with its normal towards the eye: every horizon is the surface itself; pre-denoise code 170 (visibility 1)."""
    W, H = 64, 40
    depth, normals = _flat(W, H, 3.0)
    c = g.constants(W, H, 0.2, W / H)      # a narrow view: the plane is "facing the eye" at every pixel to within 6 degrees
    levels = g.prefilter(depth, c)
    value, fragile, covered = g.main_pass(levels, normals, g.look_at_view(), c, 2, 0, 0)
    assert covered.all() and fragile.mean() < FRAGILE_CAP
    ok = ~fragile
    assert (g.code_of(value)[ok] == 170).all(), (g.code_of(value)[ok].min(), g.code_of(value)[ok].max())
    assert (g.edges(levels[0]) == 255).all()      # no edge anywhere: 3 in every two-bit field


def test_step_edge_darkens_the_low_side_only():
    W, H = 64, 40
    depth, normals = _flat(W, H, 3.0)
    depth[:, 32:] = 2.7      # the right half is a step 0.3 nearer: the left (far, low) side sees a wall, the right side sees nothing above it
    c = g.constants(W, H, 0.2, W / H)
    levels = g.prefilter(depth, c)
    value, fragile, _ = g.main_pass(levels, normals, g.look_at_view(), c, 2, 0, 0)
    code = g.code_of(value)
    low, high = code[8:32, 24:32], code[:, 32:][~fragile[:, 32:]]
    assert low.min() < 150 and (high == 170).all(), (low.min(), high.min(), high.max())      # the high half, every non-fragile pixel of it: untouched
    assert low.mean() < 170 - 10
    e = g.edges(levels[0])
    assert ((e[:, 31] >> 4) & 3 == 0).all() and ((e[:, 32] >> 6) & 3 == 0).all()      # the right edge of column 31 and the left edge of column 32 are hard
    assert (e[:, :30] == 255).all()


def test_empty_depth_survives_the_prefilter():
    W, H = 37, 21
    depth = np.full((H, W), 2.0, dtype=np.float32)
    depth[:, 20:] = g.FLT_MAX; depth[5, 3] = g.FLT_MAX
    levels = g.prefilter(depth, g.constants(W, H, 1.0, W / H))
    assert [l.shape for l in levels] == [(g.mip_size(H, m), g.mip_size(W, m)) for m in range(5)]
    for m in range(1, 5):
        assert np.isfinite(levels[m]).all() and (levels[m][:, -1] == g.FLT_MAX).all()
    assert levels[1][2, 1] == g.FLT_MAX and levels[1][0, 0] == np.float32(2.0)


def _shares():
    rows = []
    for kind, W, H in g.CASES:
        for q, lod in g.main_configs(W):
            ref = g.reference(kind, W, H, camera_of(W, H), q, lod)
            rows.append((kind, W, H, q, lod, int(ref["covered"].sum()), int(ref["fragile"].sum()), ref["fp32_error"]))
    return rows


def test_fragile_share_and_margin_of_the_gpu_inputs():
    rows = _shares()
    for kind, W, H, q, lod, covered, fragile, err in rows:
        print(f"{kind} {W}x{H} quality {q} maxDepthLod {lod}: covered {covered}, fragile {fragile} ({100.0 * fragile / covered:.2f} %), max |fp32 - float64| {err:.3g}")
        assert covered > W * H // 4 and covered <= (2 * W * H) // 3 + H, (kind, covered)      # a third of the frame is empty
        assert fragile <= FRAGILE_CAP * covered, (kind, W, H, q, lod, fragile, covered)
    M = g.margin(camera_of)
    print(f"M = {M:.4g} codes")
    assert 0.0 < M < 0.25, M      # an fp32 evaluation stays well inside half a code of the float64 one: most pixels are decided, not merely "within 1"


def _write_profile(path):
    rows = _shares()
    M = g.margin(camera_of)
    with open(path, "w") as f:
        f.write("# XeGTAO main pass: fragile shares and the margin M\n\n")
        f.write("Measured by `python tests/test_gtao_cpu.py` from the float64 restatement alone (tests/gtao_ref.py), on the inputs tests/test_gtao_gpu.py writes\n"
                "(analytic height fields, camera of the `tiny` preset at that size, frame index 5).  Cap on the fragile share: 5 % of the covered pixels.\n\n")
        f.write("| input | size | quality | maxDepthLod | covered | fragile | share | max abs(fp32 numpy - float64), codes |\n|---|---|---|---|---|---|---|---|\n")
        for kind, W, H, q, lod, covered, fragile, err in rows:
            f.write(f"| {kind} | {W}x{H} | {q} | {lod} | {covered} | {fragile} | {100.0 * fragile / covered:.2f} % | {err:.4g} |\n")
        f.write(f"\nM = 4 x the largest of the last column = **{M:.4g}** codes of the pre-rounding value `saturate(v / 1.5) * 255`.\n")


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gtao_accuracy.md")
    _write_profile(out)
    print(open(out).read())
