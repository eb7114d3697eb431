"""Temporal anti-aliasing on the GPU (brmi_temporal.hip) against tests/temporal_ref.py, bit for bit.

1  the kernel alone on synthetic surfaces (brmi_debug_temporal_resolve) at 100 x 72 and 50 x 36: neither a multiple of 8, so partial tiles on both edges, the
   second smaller than a row of 16 x 16 blocks in places;  2  through the pass, "tiny" at 256 x 144: the geometry path under a jittered camera against the
   oracle, the resolved image against the restatement iterated over the pass's own surfaces, reset, unbinding, the display chain's input, split execution,
   refusals;  3  the effect, as a condition: on edge pixels the resolved frame is closer to the mean of 16 jittered oracle frames than the unjittered frame is.

Measured on an MI355X (32 frames, blend 0.1, "tiny" 256 x 144, w-space mean absolute error on edge pixels): see profiles/temporal_cost.md.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import display_ref as d
import temporal_ref as t

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, 0xCD
W0, H0 = 256, 144


# ---------------------------------------------------------------- 1: the kernel alone ------------------------------------------------------------------
def _run_kernel(case, W, H):
    """(out (H, W) uint64, the whole output tensor's bytes, bytes of one image) of brmi_debug_temporal_resolve on the case's surfaces."""
    import torch
    from basicrenderer_amd import capi
    from basicrenderer_amd.renderer import detile, tile
    lib = capi.brmi_lib()
    dev = torch.device("cuda:0")

    def up(a):
        return None if a is None else torch.from_numpy(tile(np.ascontiguousarray(a)).view(np.uint8).reshape(-1).copy()).to(dev)
    hdr, depth, motion, history = up(case["hdr"]), up(case["depth"]), up(case["motion"]), up(case["history"])
    nbytes = hdr.numel()
    out = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
    st = capi.TemporalSettings()
    lib.brmi_temporal_default_settings(C.byref(st))
    st.blend = case["blend"]
    rc = lib.brmi_debug_temporal_resolve(W, H, hdr.data_ptr(), depth.data_ptr(), motion.data_ptr(), history.data_ptr() if history is not None else None, out.data_ptr(),
                                         C.byref(st), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, lib.brmi_last_error(None)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    return detile(raw[:nbytes].view(np.uint64), W, H), raw, nbytes


@pytest.fixture(scope="module")
def kernel_runs():
    cache = {}

    def get(kind, W, H):
        if (kind, W, H) not in cache:
            case = t.case(kind, W, H)
            want, present = t.resolve(case["hdr"], case["depth"], case["motion"], case["history"], case["blend"])
            cache[(kind, W, H)] = (case, want, present) + _run_kernel(case, W, H)
        return cache[(kind, W, H)]
    return get


@pytest.mark.parametrize("width,height", t.SIZES)
@pytest.mark.parametrize("kind", t.CASES)
def test_kernel_equals_restatement(kernel_runs, kind, width, height):
    """Every output word equals the restatement; the guard bytes behind the output and the whole-tile padding inside it keep their fill."""
    from basicrenderer_amd.renderer import tile
    case, want, present, got, raw, nbytes = kernel_runs(kind, width, height)
    bad = np.argwhere(got != want)
    print(f"{kind} {width}x{height}: history present on {present.mean():.3f} of the pixels, {len(bad)} words differ")
    assert len(bad) == 0, (kind, len(bad), bad[:4], hex(int(got[tuple(bad[0])])), hex(int(want[tuple(bad[0])])), bool(present[tuple(bad[0])]))
    assert (raw[nbytes:] == FILL).all()
    inside = tile(np.ones((height, width), dtype=np.uint8)).astype(bool)
    assert (raw[:nbytes].reshape(-1, 8)[~inside] == FILL).all()      # no store outside W x H


def test_zero_motion_is_the_pure_blend(kernel_runs):
    for (W, H) in t.SIZES:
        case, want, present, got, _, _ = kernel_runs("zero_motion", W, H)
        assert present.all() and not np.array_equal(got, case["hdr"])
        assert np.array_equal(got >> np.uint64(48), case["hdr"] >> np.uint64(48))      # alpha: the current pixel's bits


def test_history_absent_at_the_border_the_motion_leaves_through(kernel_runs):
    """Absent there and only there: worked out here from the motion halves in float64, and there the output is the current pixel."""
    for (W, H) in t.SIZES:
        for kind in ("left", "right", "up", "down", "fractional"):
            case, want, present, got, _, _ = kernel_runs(kind, W, H)
            mv = np.ascontiguousarray(case["motion"]).view(np.float16).reshape(H, W, 2).astype(np.float64)
            ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            x, y = xs - 0.5 * mv[..., 0] * W, ys + 0.5 * mv[..., 1] * H
            expect = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
            assert np.array_equal(present, expect), kind
            assert not expect.all() and expect.mean() > 0.9
            assert np.array_equal(got[~expect], case["hdr"][~expect]) and (got[expect] != case["hdr"][expect]).mean() > 0.99


def test_no_history_and_non_finite_history_pass_the_current_frame(kernel_runs):
    for (W, H) in t.SIZES:
        case, _, present, got, _, _ = kernel_runs("no_history", W, H)
        assert not present.any() and np.array_equal(got, case["hdr"])
        case, _, present, got, _, _ = kernel_runs("non_finite", W, H)
        planted = ~np.isfinite(t.unpack(case["history"])[0]).all(axis=-1)
        assert planted.sum() >= 30 and not present[planted].any()
        assert np.isfinite(t.unpack(got)[0]).all() and np.array_equal(got[~present], case["hdr"][~present])


def test_fireflies_are_bounded(kernel_runs):
    """A firefly in the history is clamped into the neighbourhood box; one in the current frame is bounded by w: neither survives in the output."""
    for (W, H) in t.SIZES:
        case, _, present, got, _, _ = kernel_runs("fireflies", W, H)
        out, cur, hist = t.unpack(got)[0], t.unpack(case["hdr"])[0], t.unpack(case["history"])[0]
        assert present.all() and (hist.max(axis=-1) > 60000).sum() >= 3 and (cur.max(axis=-1) > 60000).sum() >= 3
        assert out.max() < 100.0      # (the ordinary content is below 16)


def test_velocity_is_the_closest_neighbours(kernel_runs):
    """The far side's column next to the step edge takes the near side's motion: there the output is that of a frame that moves as a whole, not of a still one."""
    for (W, H) in t.SIZES:
        case, want, _, got, _, _ = kernel_runs("dilated", W, H)
        edge = W // 2 + 3      # the first far column
        moving, _ = t.resolve(case["hdr"], case["depth"], t.motion_of_pixels(2.25, 0.0, W, H), case["history"], case["blend"])
        still, _ = t.resolve(case["hdr"], case["depth"], t.motion_of_pixels(0.0, 0.0, W, H), case["history"], case["blend"])
        assert np.array_equal(got[:, edge], moving[:, edge]) and not np.array_equal(got[:, edge], still[:, edge])
        assert np.array_equal(got[:, edge + 1:], still[:, edge + 1:]) and np.array_equal(got[:, :edge], moving[:, :edge])


# ---------------------------------------------------------------- 2: through the pass ----------------------------------------------------------------------
def _jittered_scene(scene, cam, cull):
    v = copy.copy(scene)
    v.arrays, v._keep = dict(scene.arrays), []
    v.arrays["cameras"], v.arrays["cullingCameras"] = cam, cull
    return v


def _surfaces(r):
    g = r.gbuffer()
    return dict(vis=r.visibility(), depth=r.depth().view(np.uint32), hdr=r.hdr(), **g)


@pytest.fixture(scope="module")
def tiny(scenes):
    return scenes("tiny")


def test_geometry_path_honours_the_jittered_projection(tiny):
    """Visibility keys, depth and the seven G-buffer planes of a jittered frame equal the oracle's for the same camera bytes: the rasteriser and the resolve use
    `projection`, the motion plane the unjittered matrices."""
    import orc
    from basicrenderer_amd import temporal
    from basicrenderer_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(tiny)
    try:
        r.set_temporal()
        r.update(5); r.execute()
        cam0, _ = temporal.jitter_camera(tiny.arrays["cameras"], tiny.arrays["cullingCameras"], W0, H0, temporal.jitter_offset(0))
        cam5, cull5 = temporal.jitter_camera(tiny.arrays["cameras"], tiny.arrays["cullingCameras"], W0, H0, temporal.jitter_offset(5), previous=cam0)
        assert np.array_equal(r.device_arrays["cameras"].cpu().numpy()[: len(cam5)], cam5) and np.array_equal(r.device_arrays["cullingCameras"].cpu().numpy()[: len(cull5)], cull5)
        o = orc.OracleFrame(_jittered_scene(tiny, cam5, cull5)).run()
        plain = orc.OracleFrame(tiny).run()
        assert not np.array_equal(o.vis, plain.vis)      # the jitter moves coverage
        s = _surfaces(r)
        covered = o.vis != np.uint64(0xFFFFFFFFFFFFFFFF)
        assert np.array_equal(s["vis"], o.vis) and np.array_equal(s["depth"], o.depth.view(np.uint32))
        assert np.array_equal(s["normals"].view(np.uint32)[covered], o.normals.view(np.uint32)[covered])
        for key, ref in (("albedo", o.albedo), ("mr", o.mr), ("motion", o.motion), ("coat", o.coat), ("emissive", o.emissive), ("fuzz", o.fuzz)):
            assert np.array_equal(s[key][covered], ref[covered]), key
        # a still camera and static geometry: the motion plane does not see the jitter
        mv = np.ascontiguousarray(s["motion"][covered]).view(np.float16).astype(np.float64)
        assert np.abs(mv).max() * max(W0, H0) * 0.5 < 0.01
    finally:
        r.close()


@pytest.fixture(scope="module")
def sequence(tiny):
    """Six jittered frames of one pass, a reset before the fifth: per frame (hdr, depth, motion, resolved)."""
    from basicrenderer_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(tiny)
    frames = []
    try:
        r.set_temporal(blend=0.1, fill=FILL, guard=GUARD)
        for k in range(6):
            if k == 4:
                r.temporal_reset()
            r.update(k); r.execute()
            frames.append((r.hdr(), r.depth(), r.gbuffer()["motion"], r.resolved_hdr()))
        intact = r.temporal_guard_intact()
    finally:
        r.close()
    return frames, intact


def test_resolved_image_is_the_restatement_iterated(sequence):
    frames, intact = sequence
    history = None
    for k, (hdr, depth, motion, resolved) in enumerate(frames):
        if k == 4:
            history = None      # brmi_temporal_reset
        want, present = t.resolve(hdr, depth, motion, history, 0.1)
        assert np.array_equal(resolved, want), (k, int((resolved != want).sum()))
        if history is None:
            assert np.array_equal(resolved, hdr)      # the first frame, and the first after a reset, is the raw frame
        else:
            assert present.mean() > 0.99 and not np.array_equal(resolved, hdr)
        history = resolved
    assert intact


def test_unbinding_gives_the_frames_of_a_pass_that_never_bound(tiny):
    """With a skybox, so that a frame writes every pixel of the HDR target and the motion plane (the shading pass leaves pixels without geometry alone, and the
    jittered frames before covered other pixels): keys, depth, HDR, motion and ldr() byte for byte, the other planes wherever there is geometry."""
    from basicrenderer_amd.environment import Environment
    from basicrenderer_amd.renderer import VisibilityRenderer
    a, b = VisibilityRenderer(tiny), VisibilityRenderer(tiny)
    try:
        for r in (a, b):
            r.set_environment(Environment.procedural(16), skybox=True)
            r.set_display("lpm", bloom=True, time_coefficient=1.0)
        b.set_temporal()
        for k in range(2):
            b.update(k); b.execute()
        b.set_temporal(None)
        assert np.array_equal(b.device_arrays["cameras"].cpu().numpy(), a.device_arrays["cameras"].cpu().numpy())
        for r in (a, b):
            r.reset_exposure(); r.update(2); r.execute()
        sa, sb = _surfaces(a), _surfaces(b)
        covered = sa["vis"] != np.uint64(0xFFFFFFFFFFFFFFFF)
        assert covered.any() and not covered.all()
        for key in sa:
            every = key in ("vis", "depth", "hdr", "motion")
            assert np.array_equal(sa[key] if every else sa[key][covered], sb[key] if every else sb[key][covered]), key
        assert np.array_equal(a.ldr(), b.ldr())
        with pytest.raises(Exception):
            b.resolved_hdr()
    finally:
        a.close(); b.close()


def _fragile_ok(got, value64):
    want, fragile = d.codes_of(value64), d.fragile_codes(value64)
    diff = np.abs(got[..., :3].astype(np.int64) - want)
    return int(((diff != 0) & ~fragile).sum()), int(diff.max())


def test_display_chain_reads_the_resolved_image(tiny):
    from basicrenderer_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(tiny)
    try:
        r.set_display("aces", bloom=False, auto_exposure=False)
        r.set_temporal()
        for k in range(3):
            r.update(k); r.execute()
        resolved, raw = d.u64_to_halves(r.resolved_hdr())[..., :3], d.u64_to_halves(r.hdr())[..., :3]
        bad, worst = _fragile_ok(r.ldr(), d.resolve(2, resolved, np.float64))
        assert bad == 0 and worst <= 1
        bad_raw, _ = _fragile_ok(r.ldr(), d.resolve(2, raw, np.float64))
        assert bad_raw > 100      # ... and not the one-sample frame
    finally:
        r.close()


def test_split_execution_gives_the_same_bytes(tiny, sequence):
    from basicrenderer_amd.renderer import VisibilityRenderer
    frames, _ = sequence
    r = VisibilityRenderer(tiny)
    try:
        torch = r.torch
        other = torch.cuda.Stream(device=r.device)
        r.set_temporal(blend=0.1)
        for k in range(3):
            r.update(k); r.execute(shading_stream=other)
            other.synchronize()
            assert np.array_equal(r.hdr(), frames[k][0]) and np.array_equal(r.resolved_hdr(), frames[k][3]), k
    finally:
        r.close()


def test_refusals(tiny):
    from basicrenderer_amd import capi
    from basicrenderer_amd.renderer import VisibilityRenderer
    INVALID = -1
    r, other = VisibilityRenderer(tiny, occlusion=True), VisibilityRenderer(tiny, occlusion=True)
    try:
        lib, torch = r.lib, r.torch
        lay = r.temporal_layout()
        n = int(lay.historyBytes)
        assert n == ((W0 + 7) // 8) * ((H0 + 7) // 8) * 64 * 8
        mem = torch.zeros(2 * n + 64, dtype=torch.uint8, device=r.device)
        base = mem.data_ptr()

        def buffers(**over):
            b = capi.TemporalBuffers()
            b.structSize = C.sizeof(capi.TemporalBuffers)
            lib.brmi_temporal_default_settings(C.byref(b.settings))
            b.history[0], b.history[1], b.historyBytes = base, base + n, n
            for key, v in over.items():
                if key in ("blend", "phases"):
                    setattr(b.settings, key, v)
                elif key == "settings_reserved":
                    b.settings.reserved[2] = v
                elif key in ("h0", "h1"):
                    b.history[int(key[1])] = v
                else:
                    setattr(b, key, v)
            return b
        assert lib.brmi_set_temporal(r._h, C.byref(buffers())) == 0
        for over in (dict(h0=None), dict(h1=None), dict(h1=base + n + 8), dict(historyBytes=n - 1), dict(h1=base + n - 16), dict(h1=base), dict(blend=0.0), dict(blend=-0.5), dict(blend=1.5),
                     dict(blend=float("nan")), dict(blend=float("inf")), dict(phases=0), dict(settings_reserved=1), dict(reserved=1), dict(structSize=60)):
            assert lib.brmi_set_temporal(r._h, C.byref(buffers(**over))) == INVALID, over
        assert lib.brmi_set_temporal(r._h, C.byref(buffers(blend=1.0))) == 0
        # a binding belongs to one pass: no history source on a bound pass, either way round, and no binding on a linked pass
        assert lib.brmi_set_history_source(r._h, other._h) == INVALID and lib.brmi_set_history_source(other._h, r._h) == INVALID
        assert lib.brmi_set_temporal(r._h, None) == 0
        assert lib.brmi_set_history_source(r._h, other._h) == 0
        assert lib.brmi_set_temporal(r._h, C.byref(buffers())) == INVALID and lib.brmi_set_temporal(other._h, C.byref(buffers())) == INVALID
        assert lib.brmi_set_history_source(r._h, None) == 0
        assert lib.brmi_temporal_resolve(r._h, r._s()) != 0 and lib.brmi_temporal_reset(r._h) != 0      # nothing bound
        torch.cuda.synchronize()
        assert not mem.any()      # nothing was launched
    finally:
        r.close(); other.close()


# ---------------------------------------------------------------- 3: the effect ------------------------------------------------------------------------------
def _w64(hdr):
    c = t.unpack(hdr)[0].astype(np.float64)
    return c / (1.0 + c.max(axis=-1, keepdims=True))


def edge_mask(vis):
    """Pixels whose 3 x 3 neighbourhood in the visibility buffer holds more than one cluster (an empty pixel counts as a cluster of its own)."""
    ids = np.where(vis == np.uint64(0xFFFFFFFFFFFFFFFF), np.int64(-1), ((vis >> np.uint64(7)) & np.uint64(0x3FFFFFF)).astype(np.int64))
    p = np.pad(ids, 1, mode="edge")
    H, W = ids.shape
    edge = np.zeros((H, W), dtype=bool)
    for dy in range(3):
        for dx in range(3):
            edge |= p[dy: dy + H, dx: dx + W] != ids
    return edge


def jittered_truth(scene, phases=16):
    """(mean over the oracle's `phases` jittered HDR frames in w-space, float64; the unjittered oracle frame)."""
    import orc
    from basicrenderer_amd import temporal
    total, previous = 0.0, None
    for k in range(phases):
        cam, cull = temporal.jitter_camera(scene.arrays["cameras"], scene.arrays["cullingCameras"], scene.width, scene.height, temporal.jitter_offset(k, phases), previous=previous)
        total = total + _w64(orc.OracleFrame(_jittered_scene(scene, cam, cull)).run().hdr)
        previous = cam
    return total / phases, orc.OracleFrame(scene).run()


def test_resolved_edges_are_closer_to_the_supersampled_frame(tiny):
    """A still camera, 32 jittered frames.  Ground truth: the mean of the oracle's 16 jittered HDR frames (float64, w-space).  On the edge pixels the resolved frame's
    mean absolute error is smaller than the unjittered one-sample frame's."""
    from basicrenderer_amd.renderer import VisibilityRenderer
    truth, plain = jittered_truth(tiny)
    edges = edge_mask(plain.vis)
    assert edges.mean() >= 0.02
    from basicrenderer_amd import capi
    r = VisibilityRenderer(tiny)
    try:
        r.execute()
        single = _w64(r.hdr())
        r.set_temporal(blend=0.1, phases=16)
        for k in range(32):
            r.res[capi.RES["HDR_COLOR"]].zero_()      # (no skybox: the shading pass leaves pixels without geometry alone, and the oracle's are zero)
            r.update(k); r.execute()
        resolved = _w64(r.resolved_hdr())
    finally:
        r.close()
    err_resolved, err_single = np.abs(resolved - truth)[edges].mean(), np.abs(single - truth)[edges].mean()
    print(f"edge pixels {edges.mean():.4f} of the frame; w-space mean absolute error on them: resolved {err_resolved:.6f}, one sample {err_single:.6f}")
    assert err_resolved < err_single
