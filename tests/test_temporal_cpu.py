"""Temporal anti-aliasing without a GPU: the C ABI's exports, struct sizes and host-side refusals; the jitter sequence and the jittered camera
record (basicrenderer_amd/temporal.py); brmi_temporal_math.h, compiled into tests/temporal_main.cpp, against tests/temporal_ref.py bit for bit; and, from the
oracle, the share of edge pixels in the frame tests/test_temporal_gpu.py measures the effect on.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import temporal_ref as t      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_and_exports():
    from basicrenderer_amd import capi
    assert C.sizeof(capi.TemporalSettings) == 32 and C.sizeof(capi.TemporalLayout) == 16 and C.sizeof(capi.TemporalBuffers) == 64
    assert capi.TemporalBuffers.settings.offset == 8 and capi.TemporalBuffers.history.offset == 40 and capi.TemporalBuffers.historyBytes.offset == 56
    header = open(os.path.join(ROOT, "include", "brmi.h")).read()
    for name in ("brmi_temporal_default_settings", "brmi_temporal_get_layout", "brmi_set_temporal", "brmi_temporal_resolve", "brmi_temporal_reset", "brmi_debug_temporal_resolve"):
        assert name in capi.BRMI_EXPORTS and name + "(" in header
    assert "brmi_set_history_source" in header.split("Temporal anti-aliasing")[1].split("typedef")[0]      # the several-passes limit is stated where the stage is
    lib = capi.brmi_lib()
    s = capi.TemporalSettings()
    lib.brmi_temporal_default_settings(C.byref(s))
    assert s.structSize == 32 and s.blend == np.float32(0.1) and s.phases == 16 and not any(s.reserved)
    lay = capi.TemporalLayout()
    assert lib.brmi_temporal_get_layout(100, 72, C.byref(lay)) == 0
    assert (lay.tilesX, lay.tilesY, lay.historyBytes) == (13, 9, 13 * 9 * 64 * 8)
    assert lib.brmi_temporal_get_layout(0, 72, C.byref(lay)) == -1 and lib.brmi_temporal_get_layout(100, 72, None) == -1


def test_refusals_need_no_device():
    """The debug entry point refuses before it launches: null surfaces, misaligned ones, bad settings; the pass entry points refuse a null pass."""
    from basicrenderer_amd import capi
    lib = capi.brmi_lib()
    INVALID, FAKE = -1, 0x10000
    s = capi.TemporalSettings()
    lib.brmi_temporal_default_settings(C.byref(s))

    def call(hdr=FAKE, depth=2 * FAKE, motion=3 * FAKE, history=None, out=4 * FAKE, settings=s, w=64, h=40):
        return lib.brmi_debug_temporal_resolve(w, h, hdr, depth, motion, history, out, C.byref(settings) if settings is not None else None, None)
    for over in (dict(hdr=None), dict(depth=None), dict(motion=None), dict(out=None), dict(settings=None), dict(w=0), dict(h=0), dict(hdr=FAKE + 4), dict(out=4 * FAKE + 2),
                 dict(depth=2 * FAKE + 1), dict(history=5 * FAKE + 4), dict(out=FAKE), dict(history=4 * FAKE)):
        assert call(**over) == INVALID, over
        assert lib.brmi_last_error(None)
    for field, value in (("blend", 0.0), ("blend", 1.25), ("blend", float("nan")), ("phases", 0), ("structSize", 28)):
        bad = capi.TemporalSettings()
        lib.brmi_temporal_default_settings(C.byref(bad))
        setattr(bad, field, value)
        assert call(settings=bad) == INVALID, field
    bad = capi.TemporalSettings()
    lib.brmi_temporal_default_settings(C.byref(bad))
    bad.reserved[4] = 7
    assert call(settings=bad) == INVALID
    assert lib.brmi_set_temporal(None, None) == INVALID and lib.brmi_temporal_resolve(None, None) == INVALID and lib.brmi_temporal_reset(None) == INVALID


# ---------------------------------------------------------------- jitter ---------------------------------------------------------------------------------
def _halton_here(i, b):
    """The radical inverse of i in base b, digit by digit in fp32 as the formula states it."""
    f, r = np.float32(1.0), np.float32(0.0)
    while i > 0:
        f = np.float32(f / np.float32(b))
        r = np.float32(r + np.float32(f * np.float32(i % b)))
        i //= b
    return r


def test_jitter_sequence():
    from basicrenderer_amd import temporal
    seq = [temporal.jitter_offset(k) for k in range(32)]
    for k, (jx, jy) in enumerate(seq):
        i = k % 16
        assert np.float32(jx) == np.float32(_halton_here(i + 1, 2) - np.float32(0.5)) and np.float32(jy) == np.float32(_halton_here(i + 1, 3) - np.float32(0.5))
        assert -0.5 <= jx < 0.5 and -0.5 <= jy < 0.5
        assert (jx, jy) == tuple(float(v) for v in t.jitter_offset(k))
    assert seq[:16] == seq[16:] and len(set(seq[:16])) == 16      # period 16, no shorter
    assert all(seq[k] != seq[k + 8] for k in range(8))
    assert temporal.jitter_offset(9, phases=8) == temporal.jitter_offset(1, phases=8) == seq[1]
    # base 2 by hand: 1/2, 1/4, 3/4, 1/8 ...
    assert [seq[k][0] + 0.5 for k in range(4)] == [0.5, 0.25, 0.75, 0.125]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """temporal_main.cpp built with the library's floating-point rules: (directory, program)."""
    tmp = tmp_path_factory.mktemp("temporal")
    exe = str(tmp / "temporal_main")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", os.path.join(ROOT, "tests", "temporal_main.cpp"), "-o", exe])
    return tmp, exe


def test_header_jitter_equals_python(built):
    from basicrenderer_amd import temporal
    _, exe = built
    for phases in (16, 8):
        lines = subprocess.run([exe, "--jitter", "32", str(phases)], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")[:32]
        got = [tuple(float(np.array([int(w, 16)], dtype=np.uint32).view(np.float32)[0]) for w in line.split()) for line in lines]
        assert got == [temporal.jitter_offset(k, phases) for k in range(32)]


def test_jittered_camera(scenes):
    from basicrenderer_amd import temporal
    sc = scenes("tiny")
    W, H = sc.width, sc.height
    base_cam, base_cull = sc.arrays["cameras"], sc.arrays["cullingCameras"]
    keep = base_cam.copy()
    previous = None
    rng = np.random.default_rng(5)
    for k in range(4):
        j = temporal.jitter_offset(k)
        cam, cull = temporal.jitter_camera(base_cam, base_cull, W, H, j, previous=previous)
        assert np.array_equal(base_cam, keep)      # the input record is not written
        c, b, cc = cam.view(np.float32), base_cam.view(np.float32), cull.view(np.float32)
        unj, proj = c[132:148].reshape(4, 4), c[36:52].reshape(4, 4)
        assert np.array_equal(unj, b[132:148].reshape(4, 4))
        ndc = (np.float32(np.float32(2.0) * np.float32(j[0])) / np.float32(W), np.float32(np.float32(-2.0) * np.float32(j[1])) / np.float32(H))
        # only the translation: row 2 (the row w is made of: column 3 holds -1) gains -ndc in x and y, nothing else moves
        delta = proj.astype(np.float64) - unj.astype(np.float64)
        expect = np.zeros((4, 4)); expect[2, 0], expect[2, 1] = -np.float64(ndc[0]), -np.float64(ndc[1])
        assert np.array_equal(delta, expect)
        # a point projected by both differs by jitterNDC after the divide
        view = c[4:20].reshape(4, 4).astype(np.float64)
        for _ in range(8):
            p = np.append(rng.uniform(-2, 2, size=3) + [0.0, 0.5, -4.0], 1.0) @ view
            a, bb = p @ proj.astype(np.float64), p @ unj.astype(np.float64)
            assert bb[3] > 0 and np.allclose(a[:2] / a[3] - bb[:2] / bb[3], [ndc[0], ndc[1]], rtol=0, atol=1e-12)
        # what the scene code derives from `projection`
        assert np.array_equal(c[68:84].reshape(4, 4), (view @ proj.astype(np.float64)).astype(np.float32))
        assert np.allclose(c[52:68].reshape(4, 4).astype(np.float64) @ proj.astype(np.float64), np.eye(4), atol=1e-4)
        assert cc[4] == proj[0, 0] and cc[5] == proj[1, 1] and np.array_equal(cc[24:40], c[68:84]) and np.array_equal(cc[60:76], c[52:68])
        untouched = np.ones(len(c), dtype=bool)
        untouched[36:84] = False; untouched[100:132] = False
        assert np.array_equal(c.view(np.uint32)[untouched], b.view(np.uint32)[untouched])
        if previous is None:
            assert np.array_equal(c[100:132], b[100:132])
        else:
            pv = previous.view(np.float32)
            assert np.array_equal(c[100:116], pv[36:52]) and np.array_equal(c[116:132], pv[132:148])      # prev* of frame k + 1 = the current fields of frame k
        previous = cam
    # frame 0's x offset is zero (Halton(1, 2) = 1/2): its y is not
    assert temporal.jitter_offset(0)[0] == 0.0 and temporal.jitter_offset(0)[1] != 0.0


# ---------------------------------------------------------------- the header against the restatement ----------------------------------------------------
@pytest.mark.parametrize("width,height", t.SIZES)
@pytest.mark.parametrize("kind", t.CASES)
def test_header_equals_restatement(built, kind, width, height):
    tmp, exe = built
    case = t.case(kind, width, height)
    src, dst = str(tmp / f"{kind}_{width}.in"), str(tmp / f"{kind}_{width}.out")
    with open(src, "wb") as f:
        f.write(np.array([width, height, 0 if case["history"] is None else 1], dtype=np.uint32).tobytes() + np.float32(case["blend"]).tobytes())
        f.write(case["hdr"].tobytes() + case["depth"].tobytes() + case["motion"].tobytes())
        if case["history"] is not None:
            f.write(np.ascontiguousarray(case["history"]).tobytes())
    subprocess.run([exe, src, dst], check=True, timeout=60)
    got = np.fromfile(dst, dtype=np.uint64).reshape(height, width)
    want, present = t.resolve(case["hdr"], case["depth"], case["motion"], case["history"], case["blend"])
    assert np.array_equal(got, want), (kind, int((got != want).sum()))
    assert np.array_equal(got[~present], case["hdr"][~present])


def test_restatement_properties():
    """Properties that do not depend on who wrote the restatement: a constant frame with the same constant history settles on w^-1 of the half that holds w(c),
    within one half step of c, and stays there; the tie rule on a hand-made frame."""
    W, H = 24, 16
    grey = t.pack(np.full((H, W, 3), 0.5, dtype=np.float16), np.full((H, W), 0x3C00, dtype=np.uint16))
    depth = np.ones((H, W), dtype=np.float32)
    still = t.motion_of_pixels(0.0, 0.0, W, H)
    out, present = t.resolve(grey, depth, still, grey, 0.1)
    w16 = np.float32(np.float16(np.float32(0.5) / np.float32(1.5)))      # the neighbourhood holds w as halves: the box of a constant frame is that one value
    settled = np.float16(w16 / (np.float32(1.0) - w16))
    assert present.all() and (t.unpack(out)[0] == np.float32(settled)).all() and abs(float(settled) - 0.5) <= 2.0 ** -11
    again, _ = t.resolve(grey, depth, still, out, 0.1)
    assert np.array_equal(again, out)      # ... and there it stays
    # equal depths everywhere: the first of the nine in row-major order is the upper-left neighbour, whose motion (one pixel left, distinct from every other) is taken
    motion = t.motion_of_pixels(0.0, 0.0, W, H)
    motion[4, 6] = t.motion_of_pixels(-1.0, 0.0, W, H)[0, 0]
    hist = t.pack(np.random.default_rng(1).uniform(0.1, 0.9, size=(H, W, 3)).astype(np.float16), np.full((H, W), 0x3C00, dtype=np.uint16))
    ramp = t.pack(np.random.default_rng(2).uniform(0.1, 0.9, size=(H, W, 3)).astype(np.float16), np.full((H, W), 0x3C00, dtype=np.uint16))
    a, _ = t.resolve(ramp, depth, motion, hist, 0.5)
    b, _ = t.resolve(ramp, depth, still, hist, 0.5)
    differs = np.argwhere(a != b)
    assert len(differs) >= 1 and all((y, x) == (5, 7) for y, x in differs)      # only the pixel whose upper-left neighbour is (6, 4)
    # ... and a strictly closer pixel later in the order beats it
    depth2 = depth.copy(); depth2[5, 8] = 0.5
    motion2 = motion.copy(); motion2[5, 8] = t.motion_of_pixels(0.0, 1.0, W, H)[0, 0]
    c, _ = t.resolve(ramp, depth2, motion2, hist, 0.5)
    d_, _ = t.resolve(ramp, depth2, t.motion_of_pixels(0.0, 1.0, W, H), hist, 0.5)
    assert c[5, 7] == d_[5, 7] and c[5, 7] != a[5, 7]


def test_edge_pixels_of_the_effect_frame(scenes, oracle_frames):
    """The frame test_temporal_gpu.py measures the effect on has at least 2 % edge pixels (3 x 3 neighbourhoods of the visibility buffer with more than one cluster)."""
    import test_temporal_gpu as g
    share = g.edge_mask(oracle_frames("tiny").vis).mean()
    print(f"edge pixels: {share:.4f} of the frame")
    assert share >= 0.02
