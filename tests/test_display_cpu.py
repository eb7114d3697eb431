"""The display chain without a GPU: brmi_display_math.h, compiled into tests/display_main.cpp, against tests/display_ref.py; properties of the
curves that do not depend on who wrote the restatement; the C ABI; and -- from the float64 side alone -- the margins and the fragile share of every input
tests/test_display_gpu.py uses (cap: 2 % of a case's pixels; an input that exceeds it is changed, not the cap).

    python tests/test_display_cpu.py      writes the measured margins and shares to profiles/display_accuracy.md

Measured (margins are FACTOR = 4 times the largest fp32-against-float64 difference): bin 1.0e-4 steps, luminance 2.1e-5, code 8.0e-4 codes, half stores
1.6e-3 / 2.7e-4 / 3.1e-4 of the spacing (down / up / blend), length 1.7e-5; fragile shares, exact ties included: bins <= 0.04 %, codes <= 0.55 %,
downsample <= 1.2 %, upsample <= 0.9 %, blend <= 1.1 %.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import display_ref as d      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAGILE_CAP = 0.02
ADAPTED = [0.18, 1.0, 0.02, 4.0, 1e-7]


def _inputs():
    rng = np.random.default_rng(11)
    lum = np.exp2(rng.uniform(np.log2(1e-3), np.log2(50.0), size=400))
    col = rng.uniform(0.2, 1.0, size=(400, 3))
    colours = (col * (lum / (col @ np.array([0.2125, 0.7154, 0.0721])))[:, None])
    colours = np.concatenate([colours, [[0, 0, 0], [12, 14, 30], [1e-4, 2e-4, 1e-4], [0.18, 0.18, 0.18], [10, 10, 10], [65504, 0, 0]]]).astype(np.float16).astype(np.float32)
    hist = rng.integers(0, 900, size=256).astype(np.uint32)
    taps = rng.uniform(0.0, 8.0, size=(30, 13)).astype(np.float32)
    taps[:6] *= np.float32(0.02)      # below the cut
    tent = rng.uniform(0.0, 8.0, size=(30, 9)).astype(np.float32)
    return colours, np.array(ADAPTED, np.float32), hist, np.float32(101 * 53), taps, tent


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """display_main.cpp built with the library's floating-point rules: (directory, program)."""
    tmp = tmp_path_factory.mktemp("display")
    exe = str(tmp / "display_main")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", os.path.join(ROOT, "tests", "display_main.cpp"), "-o", exe])
    return tmp, exe


PROP_ADAPTED = [0.02, 0.18, 1.0, 4.0]
PROP_CONSTANTS = [3.0, 0.7, 0.5]      # length = c sqrt(3): kept, kept, cut


def _property_inputs():
    rng = np.random.default_rng(3)
    greys = np.exp2(np.linspace(-12, np.log2(10.0), 600)).astype(np.float32)
    wide = np.exp2(rng.uniform(-14, 15, size=(4000, 3))).astype(np.float32)
    hand = np.zeros(256, np.uint32); hand[0], hand[100], hand[200] = 50, 30, 20
    big = np.zeros(256, np.uint32); big[255] = 7680 * 4320      # an 8K frame of bright pixels: 255 * 33177600 = 8460288000 wraps past 2^32
    empty = np.zeros(256, np.uint32); empty[0] = 64
    hists = [(hand, 100.0), (big, float(7680 * 4320)), (empty, 64.0)]
    # fp32 values no half holds: every binade of the half range and beyond, subnormals, the overflow threshold, exact ties on even and odd halves, both signs
    halves = np.arange(0, 0x7C00, 37, dtype=np.uint16).view(np.float16).astype(np.float32)
    step = np.spacing(halves.astype(np.float16)).astype(np.float32)
    unrounded = np.concatenate([np.exp2(rng.uniform(-30, 18, size=3000)).astype(np.float32) * rng.choice([-1.0, 1.0], size=3000).astype(np.float32),
                                halves + step * np.float32(0.5), halves + step * np.float32(0.5) * (1 + np.float32(2.0 ** -12)), halves + step * np.float32(0.25),
                                np.array([65504.0, 65519.996, 65520.0, 70000.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 2.0 ** -26, 0.0, -0.0, np.inf, -np.inf, 6.1e-5, 6.1035e-5],
                                         dtype=np.float32)]).astype(np.float32)
    return greys, wide, hists, unrounded


@pytest.fixture(scope="module")
def props(built):
    """display_main --properties on the property tests' inputs: (the header's outputs, inputs)."""
    tmp, exe = built
    greys, wide, hists, unrounded = _property_inputs()
    with open(str(tmp / "props.bin"), "wb") as f:
        for arr in (np.array(PROP_ADAPTED, np.float32), greys):
            f.write(np.uint32(len(arr)).tobytes() + arr.tobytes())
        f.write(np.uint32(len(wide)).tobytes() + wide.tobytes())
        f.write(np.uint32(len(PROP_CONSTANTS)).tobytes() + np.array(PROP_CONSTANTS, np.float32).tobytes())
        f.write(np.uint32(len(hists)).tobytes())
        for hist, npx in hists:
            f.write(hist.tobytes() + np.float32(npx).tobytes())
        f.write(np.uint32(len(unrounded)).tobytes() + unrounded.tobytes())
    r = subprocess.run([exe, "--properties", str(tmp / "props.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout), (greys, wide, hists, unrounded)


@pytest.fixture(scope="module")
def header(built):
    """display_main on the fixed inputs: (outputs, inputs)."""
    tmp, exe = built
    colours, adapted, hist, npx, taps, tent = _inputs()
    with open(str(tmp / "in.bin"), "wb") as f:
        f.write(np.uint32(len(colours)).tobytes() + colours.tobytes() + np.uint32(len(adapted)).tobytes() + adapted.tobytes() + hist.tobytes() + npx.tobytes())
        f.write(np.uint32(len(taps)).tobytes() + taps.tobytes() + tent.tobytes())
    r = subprocess.run([exe, str(tmp / "in.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout), (colours, adapted, hist, npx, taps, tent)


def _close(got, want64, rel, what):
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    err = np.abs(got - want64) / np.maximum(np.abs(want64), 1e-3)
    print(f"{what}: largest relative difference {np.nanmax(err):.3g} (bound {rel:.3g})")
    assert np.nanmax(err) <= rel, (what, float(np.nanmax(err)))
    assert np.array_equal(np.isnan(got), np.isnan(want64)), what


def test_header_against_numpy(header):
    """Integers exact outside fragile inputs; floats within FACTOR x the fp32-against-float64 difference of the restatement on the same inputs."""
    out, (colours, adapted, hist, npx, taps, tent) = header
    m = d.margins()
    bins64 = d.bins_of(colours, np.float64)
    fragile = d.fragile_bins(colours)
    assert fragile.mean() <= FRAGILE_CAP
    assert np.array_equal(np.asarray(out["bins"])[~fragile], bins64[~fragile]) and (np.abs(np.asarray(out["bins"]) - bins64) <= 1).all()
    assert out["weightedSum"][0] == d.weighted_sum(hist)
    avg64 = d.average_luminance(hist, npx, np.float64)
    _close(out["average"], [avg64, d.adapt(0.5, np.float32(avg64), 0.25, np.float64)], max(m["adapted"], 4e-6), "average")
    for k, a in enumerate(adapted):
        c64, c32 = d.lpm_control(d.lpm_params(a, np.float64)), d.lpm_control(d.lpm_params(a, np.float32)).astype(np.float64)
        rel = d.FACTOR * float(np.max(np.abs(c32 - c64) / np.maximum(np.abs(c64), 1e-30)))
        got = np.asarray(out["control"][96 * k: 96 * k + 96])
        assert np.max(np.abs(got - c64) / np.maximum(np.abs(c64), 1e-30)) <= max(rel, 4e-6), (a, got[4:6], c64[4:6])
        assert (got[15:24] == 0).all() and (got[28:] == 0).all()      # con2, softGap, con and the packed-half words stay zero
    lpm64 = d.lpm_params(adapted[0], np.float64)
    for curve in d.CURVES:
        v32, v64 = d.tone_map(curve, colours, np.float32, d.lpm_params(adapted[0], np.float32)).astype(np.float64), d.tone_map(curve, colours, np.float64, lpm64)
        with np.errstate(invalid="ignore"):
            bound = d.FACTOR * np.nanmax(np.abs(v32 - v64) / np.maximum(np.abs(v64), 1e-3))
        _close(np.asarray(out[curve]).reshape(-1, 3), v64, max(bound, 4e-6), curve)
    value = d.code_value(colours, np.float64)
    codes = np.asarray(out["codes"]).reshape(-1, 4)
    ok = ~d.fragile_codes(value)
    assert np.array_equal(codes[:, :3][ok], d.codes_of(value)[ok]) and (codes[:, 3] == 255).all()
    assert np.array_equal(np.asarray(out["halves"], dtype=np.uint16), colours.astype(np.float16).view(np.uint16).reshape(-1))
    t64 = taps.astype(np.float64)
    down64 = t64[:, 4] * 0.125 + (t64[:, 0] + t64[:, 2] + t64[:, 6] + t64[:, 8]) * 0.03125 + (t64[:, 1] + t64[:, 3] + t64[:, 5] + t64[:, 7]) * 0.0625 + t64[:, 9:].sum(1) * 0.125
    _close(out["down"], down64, 4e-6, "downsample")
    e64 = tent.astype(np.float64)
    _close(out["tent"], (e64[:, 4] * 4 + (e64[:, 1] + e64[:, 3] + e64[:, 5] + e64[:, 7]) * 2 + e64[:, 0] + e64[:, 2] + e64[:, 6] + e64[:, 8]) / 16, 4e-6, "tent")
    tails = np.asarray(out["tail"]).reshape(-1, 4)
    v = np.maximum(down64.reshape(-1, 3), 1e-5)
    kept = np.sqrt((v * v).sum(1)) >= 1.0
    assert np.array_equal(tails[:, 0] == 1.0, kept) and (~kept).sum() >= 2 and (tails[~kept, 1:] == 0).all()
    want = [float(np.float16(np.float32(1.5) + np.float32(0.04) * np.float32(1.75))), float(np.float16(np.float32(0.333251953125) + np.float32(1.0009765625)))]
    assert np.array_equal(np.asarray(out["blend"], dtype=np.float16), np.asarray(want, dtype=np.float16))      # (printed with nine digits: halves survive)


def test_levels_and_refusal(header):
    out, _ = header
    lv = np.asarray(out["levels"]).reshape(3, 12)
    for row, (w, h) in zip(lv, [(64, 40), (101, 53), (40, 24)]):
        assert row[0] == 5 == d.level_count(w, h) and row[1] == (1 if min(w, h) >= 32 else 0)
        assert [tuple(x) for x in row[2:].reshape(5, 2)] == [(w >> l, h >> l) for l in range(1, 6)]
    assert lv[2][1] == 0 and not d.bloom_possible(40, 24)
    assert d.level_count(8, 4) == 4 and d.level_count(1, 1) == 1


def test_lpm_contract_and_curve_properties(props):
    """On brmi_display_math.h's own output.  toneScaleBias's contract: grey hdrMax * 0.18 * 2^-exposure maps to 0.18 and grey hdrMax to 1 (fp32: the curve is
    luma / (luma * tsb0 + tsb1) with tsb of a few fp32 operations; 2e-6 absolute is a dozen ULP of 0.18); every curve is monotone on greys (to one ULP of the
    output: fp32 rounds each step of the ramp on its own); ACES lies in [0, 1]; type 4 is gamma only.  The restatement is held to the same properties."""
    out, (greys, wide, _, _) = props
    mid, lo, hi = np.asarray(out["midIn"]), np.asarray(out["lpmMid"]).reshape(-1, 3), np.asarray(out["lpmMax"]).reshape(-1, 3)
    assert np.allclose(mid, PROP_ADAPTED, rtol=4e-6)      # midIn = hdrMax * 0.18 * 2^-log2(hdrMax * 0.18 / adapted) is the adapted luminance
    assert np.allclose(lo, 0.18, atol=2e-6) and np.allclose(hi, 1.0, atol=2e-6), (lo, hi)
    for name in ("rampReinhard", "rampNeutral", "rampAces", "rampLpm", "rampNone"):
        y = np.asarray(out[name], dtype=np.float32)
        assert len(y) == len(greys) and (np.diff(y) >= -np.spacing(y[1:])).all(), name
        assert y[-1] > y[0]
    a = np.asarray(out["aces"])
    assert len(a) == wide.size and a.min() >= 0.0 and a.max() <= 1.0 and a.max() > 0.9
    assert np.array_equal(np.asarray(out["none"], dtype=np.float32).reshape(-1, 3), wide)
    value = d.code_value(wide, np.float64)
    codes, ok = np.asarray(out["noneCodes"]).reshape(-1, 4), ~d.fragile_codes(value)
    assert np.array_equal(codes[:, :3][ok], d.codes_of(value)[ok]) and (np.abs(codes[:, :3] - d.codes_of(value)) <= 1).all() and (codes[:, 3] == 255).all()
    for adapted in PROP_ADAPTED:
        p = d.lpm_params(np.float64(adapted), np.float64)
        m64 = float(p["midIn"])
        assert abs(m64 - adapted) < 1e-9 * adapted
        o = d.lpm_map(np.array([[m64] * 3, [d.HDR_MAX] * 3]), p, np.float64)
        assert np.allclose(o[0], 0.18, atol=1e-9) and np.allclose(o[1], 1.0, atol=1e-9)
    g64 = np.repeat(greys.astype(np.float64)[:, None], 3, axis=1)
    p = d.lpm_params(np.float64(0.5), np.float64)
    for curve in d.CURVES:
        assert (np.diff(d.tone_map(curve, g64, np.float64, p)[:, 1]) >= -1e-12).all(), curve
    black = d.lpm_map(np.zeros((1, 3)), p, np.float64)      # rcp(0) * 0 = NaN, which the saturates turn into 0
    assert (black == 0).all() and (d.codes_of(d.code_value(np.array([np.nan, -1.0, 2.0]), np.float64)) == [0, 0, 255]).all()


def test_constant_images_pass_the_filters(props):
    """The header's 13-tap and 9-tap sums of a constant are that constant (weights sum to 1 in fp32: powers of two), and the tail cuts length < 1 to zero;
    the restatement's whole-image filters likewise."""
    out, _ = props
    down, tent = np.asarray(out["constDown"], dtype=np.float32).reshape(-1, 4), np.asarray(out["constTent"], dtype=np.float32)      # (nine digits: fp32 survives)
    for row, t, c, kept in zip(down, tent, PROP_CONSTANTS, (True, True, False)):
        assert t == np.float32(c) and row[0] == float(kept)
        assert (row[1:] == np.float32(c)).all() if kept else (row[1:] == 0).all()
    for c, kept in zip(PROP_CONSTANTS, (True, True, False)):
        src = np.full((20, 32, 3), c, dtype=np.float16)
        v, length, k = d.downsample(src, np.float64)
        assert (k == kept).all() and (np.allclose(v, float(np.float16(c))) if kept else (v == 0).all())
        assert np.allclose(d.tent(src, 64, 40, np.float64), float(np.float16(c)), rtol=1e-12)
        assert np.allclose(d.upsample(src, np.zeros((40, 64, 3), np.float16), np.float32), float(np.float16(c)), rtol=1e-6)


def test_average_on_hand_made_histograms(props):
    """weighted_sum and average_luminance of the header on hand-made histograms, one whose weighted sum exceeds 2^32, against figures worked out here."""
    out, (_, _, hists, _) = props
    sums, averages = out["histSums"], np.asarray(out["histAverages"])
    rng_, mlog = float(d.LOG_RANGE), float(d.MIN_LOG)
    assert sums == [7000, (255 * 7680 * 4320) % (1 << 32), 0] and sums[1] == 4165320704
    wla_big = float(np.float32(4165320704)) / float(np.float32(7680 * 4320)) - 1.0
    want = [2.0 ** ((7000.0 / 50.0 - 1.0) / 254.0 * rng_ + mlog), 2.0 ** (wla_big / 254.0 * rng_ + mlog), 2.0 ** (-1.0 / 254.0 * rng_ + mlog)]      # (max(0, 1) = 1, then - 1)
    assert np.allclose(averages, want, rtol=4e-6), (averages, want)      # a few fp32 operations and exp2f
    for (hist, npx), s, w in zip(hists, sums, want):
        assert d.weighted_sum(hist) == s
        assert abs(float(d.average_luminance(hist, npx, np.float64)) - w) < 1e-9 * max(w, 1.0)


def test_half_bits_of_unrounded_values(props):
    """The host's half_bits on fp32 values that are no halves: round to nearest even, subnormals, overflow to infinity, both signs -- numpy's float16 cast."""
    out, (_, _, _, unrounded) = props
    with np.errstate(over="ignore"):
        want = unrounded.astype(np.float16).view(np.uint16)
    got = np.asarray(out["halfBits"], dtype=np.uint16)
    assert np.array_equal(got, want), (unrounded[got != want][:5], got[got != want][:5], want[got != want][:5])


# ---------------------------------------------------------------- the C ABI --------------------------------------------------------------------------------------
def test_struct_sizes_and_exports():
    from basicrenderer_amd import capi
    assert C.sizeof(capi.DisplaySettings) == 48 and C.sizeof(capi.DisplayPlane) == 24 and C.sizeof(capi.DisplayLayout) == 176 and C.sizeof(capi.DisplayBuffers) == 104
    assert capi.DisplayBuffers.settings.offset == 8 and capi.DisplayBuffers.scratch.offset == 56 and capi.DisplayBuffers.blendedHdr.offset == 88
    header = open(os.path.join(ROOT, "include", "brmi.h")).read()
    for name in ("brmi_display_default_settings", "brmi_display_get_layout", "brmi_set_display", "brmi_display_exposure", "brmi_display_bloom", "brmi_display_resolve"):
        assert name in capi.BRMI_EXPORTS and name + "(" in header
    assert "#define BRMI_ABI_MINOR 1u" in header
    lib = capi.brmi_lib()
    s = capi.DisplaySettings()
    lib.brmi_display_default_settings(C.byref(s))
    assert (s.structSize, s.tonemapType, s.bloom, s.autoExposure) == (48, 3, 1, 1)
    assert s.minLogLuminance == d.MIN_LOG and s.logLuminanceRange == d.LOG_RANGE
    for w, h in d.SIZES + [(40, 24)]:
        lay = capi.DisplayLayout()
        assert lib.brmi_display_get_layout(w, h, C.byref(lay)) == 0
        assert lay.ldrBytes == w * h * 4 and lay.blendedHdrBytes == ((w + 7) // 8) * ((h + 7) // 8) * 512 and lay.controlBlockOffset % 128 == 0
        assert lay.bloomLevels == (5 if min(w, h) >= 32 else 0)
        end = max(lay.histogramOffset + 1024, lay.adaptedLuminanceOffset + 4, lay.controlBlockOffset + 384)
        for k in range(lay.bloomLevels):
            p = lay.bloom[k]
            assert (p.width, p.height) == (w >> (k + 1), h >> (k + 1)) and p.offset >= end and p.offset % 256 == 0 and p.bytes == ((p.width + 7) // 8) * ((p.height + 7) // 8) * 512
            end = p.offset + p.bytes
        assert lay.scratchBytes >= end
    assert lib.brmi_display_get_layout(0, 4, C.byref(lay)) == -1 and lib.brmi_display_get_layout(4, 4, None) == -1


FAKE = 0x10000      # a non-null, aligned "device" address: every call below is refused, or stores the pointer, before anything could read it


def test_set_display_refusals_need_no_device():
    from basicrenderer_amd import capi
    lib = capi.brmi_lib()
    INVALID, STATE = -1, -4

    def make(w=64, h=40, **over):
        cfg = capi.Config()
        lib.brmi_default_config(C.byref(cfg), w, h)
        for key, v in over.items():
            setattr(cfg, key, v)
        hnd = capi.vp()
        assert lib.brmi_create(C.byref(cfg), C.byref(hnd)) == 0
        return hnd

    def buffers(w=64, h=40, **over):
        lay = capi.DisplayLayout()
        lib.brmi_display_get_layout(w, h, C.byref(lay))
        b = capi.DisplayBuffers()
        b.structSize = C.sizeof(capi.DisplayBuffers)
        lib.brmi_display_default_settings(C.byref(b.settings))
        b.scratch, b.scratchBytes, b.ldr, b.ldrBytes, b.blendedHdr, b.blendedHdrBytes = FAKE, lay.scratchBytes, 2 * FAKE, lay.ldrBytes, 3 * FAKE, lay.blendedHdrBytes
        for key, v in over.items():
            setattr(b if hasattr(b, key) else b.settings, key, v)
        return b
    hnd = make()
    try:
        assert lib.brmi_set_display(hnd, C.byref(buffers())) == 0
        assert lib.brmi_set_display(hnd, C.byref(buffers(blendedHdr=None))) == 0
        assert lib.brmi_display_resolve(hnd, None) == STATE      # bound, but before brmi_setup
        assert lib.brmi_set_display(hnd, None) == 0
        for over in (dict(structSize=100), dict(scratch=None), dict(ldr=None), dict(scratch=FAKE + 8), dict(ldr=FAKE + 2), dict(blendedHdr=FAKE + 8), dict(reserved=1)):
            assert lib.brmi_set_display(hnd, C.byref(buffers(**over))) == INVALID, over
        for field in ("scratchBytes", "ldrBytes", "blendedHdrBytes"):
            b = buffers(); setattr(b, field, getattr(b, field) - 1)
            assert lib.brmi_set_display(hnd, C.byref(b)) == INVALID, field
        for key, v in (("structSize", 44), ("tonemapType", 5), ("bloom", 2), ("autoExposure", 2), ("minLogLuminance", float("nan")), ("logLuminanceRange", float("inf")),
                       ("logLuminanceRange", 0.0), ("timeCoefficient", float("nan")), ("fixedAdaptedLuminance", float("inf"))):
            b = buffers(); setattr(b.settings, key, v)
            assert lib.brmi_set_display(hnd, C.byref(b)) == INVALID, key
            assert lib.brmi_last_error(hnd)
        for stage in ("brmi_display_exposure", "brmi_display_bloom", "brmi_display_resolve"):
            assert getattr(lib, stage)(hnd, None) == STATE
    finally:
        lib.brmi_destroy(hnd)
    small = make(40, 24)
    try:
        b = buffers(40, 24)
        assert lib.brmi_set_display(small, C.byref(b)) == INVALID      # bloom below 32 pixels a side
        b.settings.bloom = 0
        assert lib.brmi_set_display(small, C.byref(b)) == 0
    finally:
        lib.brmi_destroy(small)
    for over in (dict(bandY0=8, bandY1=24), dict(dynamicBand=1), dict(h=64, stripeRows=16, stripeCount=2, stripeIndex=0, fullHeight=128)):
        hh = over.pop("h", 40)
        part = make(64, hh, **over)
        try:
            assert lib.brmi_set_display(part, C.byref(buffers(64, hh))) == INVALID, over
        finally:
            lib.brmi_destroy(part)


# ---------------------------------------------------------------- margins and fragile shares -----------------------------------------------------------------------
def shares():
    """{case: fragile share} for every input the GPU file uses; bloom stores count a texel once whichever channel is fragile."""
    out = {}
    for w, h in d.SIZES:
        for kind in d.HISTOGRAM_KINDS:
            out[f"histogram {kind} {w}x{h}"] = float(d.fragile_bins(d.case(kind, w, h)).mean())
        for kind in d.RESOLVE_KINDS:
            img = d.case(kind, w, h)
            p = d.lpm_params(np.float32(d.average_luminance(d.histogram(img), w * h, np.float32)), np.float64)
            for curve in d.CURVES:
                out[f"resolve {curve} {kind} {w}x{h}"] = float(d.fragile_codes(d.resolve(curve, img, np.float64, p)).any(-1).mean())
        for kind in d.BLOOM_KINDS:
            img = d.case(kind, w, h)
            down, up, _ = d.bloom_chain(img)
            n = f = 0
            for i in range(5):
                v, length, kept = d.downsample(down[i], np.float64)
                fr = (d.fragile_halves(v, "down").any(-1) & kept) | d.fragile_cut(length)
                n, f = n + fr.size, f + int(fr.sum())
            out[f"downsample {kind} {w}x{h}"] = f / n
        n = f = 0
        for i in range(4, 0, -1):
            fr = d.fragile_halves(d.upsample(*d.upsample_case(w, h, i), np.float64), "up").any(-1)
            n, f = n + fr.size, f + int(fr.sum())
        out[f"upsample {w}x{h}"] = f / n
        out[f"blend {w}x{h}"] = float(d.fragile_halves(d.blend(*d.blend_case(w, h), np.float64), "blend").any(-1).mean())
    return out


def test_fragile_share_of_every_gpu_input():
    """A condition on the inputs: at most 2 % of a case's pixels are fragile.  An exact rounding tie is fragile like any other value on a boundary; the
    upsample's and the blend's sources are chosen so that ties are rare (display_ref.upsample_case, blend_case)."""
    sh = shares()
    for case, v in sh.items():
        print(f"{case}: {100 * v:.3f} %")
    over = {c: v for c, v in sh.items() if v > FRAGILE_CAP}
    assert not over, over


if __name__ == "__main__":
    m, sh = d.margins(), shares()
    with open(os.path.join(ROOT, "profiles", "display_accuracy.md"), "w") as f:
        f.write("# Display chain: measured margins and fragile shares (tests/test_display_cpu.py)\n\n")
        f.write(f"Margins are {d.FACTOR:g} x the largest fp32-against-float64 difference of tests/display_ref.py over the inputs of the GPU tests; the factor is for the\n"
                "GPU's log2, exp2 and pow, which are within 1-2 ULP of numpy's.\n\n| decision | margin | unit |\n|---|---|---|\n")
        units = dict(bin="bin steps", lum="luminance (absolute; the 0.005 cut)", code="8-bit codes", half_down="half spacings (downsample store)", half_up="half spacings (upsample store)",
                     half_blend="half spacings (blend store)", length="length (absolute; the < 1 cut)", adapted="relative (adapted luminance)", control="relative (control block words)")
        for key, v in m.items():
            f.write(f"| {key} | {v:.3g} | {units[key]} |\n")
        f.write("\n| case | fragile share |\n|---|---|\n")
        for case, v in sh.items():
            f.write(f"| {case} | {100 * v:.3f} % |\n")
    print("wrote profiles/display_accuracy.md")
