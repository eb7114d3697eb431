"""The display chain on the GPU through the C ABI (brmi_set_display and its stages), against tests/display_ref.py.

HDR inputs are poked into the HDR target of a small pass (no render), 64 x 40 and 101 x 53.  Every display buffer is the test's own tensor, pre-filled with
0xCD (the histogram and the adapted luminance zeroed, as the ABI asks), with guard bytes behind it.  A decision (bin, code, half store, length cut) is held
exactly wherever the float64 restatement is farther than the measured margin from the decision's boundary, and to one step elsewhere.

1  histogram;  2  average, adaptation over three frames, the control block;  3  bloom level by level from the test's own sources, the blended level 0, the
HDR target untouched;  4  resolve: five curves, with and without bloom, fixed exposure;  5  whole frames: bound == unbound in every surface, off is off;
6  refusals launch nothing.
"""
import ctypes as C

import numpy as np
import pytest

import display_ref as d

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, 0xCD


class Rig:
    """One small pass per frame size with the test's own display buffers."""

    def __init__(self, width, height):
        from basicrenderer_amd import Scene
        from basicrenderer_amd.renderer import VisibilityRenderer
        self.W, self.H = width, height
        self.r = VisibilityRenderer(Scene("tiny", width, height, point_lights=2))
        self.lay = self.r.display_layout()
        torch = self.r.torch
        self.scratch = torch.empty((int(self.lay.scratchBytes) + GUARD,), dtype=torch.uint8, device=self.r.device)
        self.ldr = torch.empty((int(self.lay.ldrBytes) + GUARD,), dtype=torch.uint8, device=self.r.device)
        self.blended = torch.empty((int(self.lay.blendedHdrBytes) + GUARD,), dtype=torch.uint8, device=self.r.device)
        self.refill()

    def refill(self, zero_state=True):
        self.r.torch.cuda.synchronize()
        self.scratch.fill_(FILL); self.ldr.fill_(FILL); self.blended.fill_(FILL)
        if zero_state:
            self.scratch[int(self.lay.histogramOffset): int(self.lay.histogramOffset) + 1024].zero_()
            self.scratch[int(self.lay.adaptedLuminanceOffset): int(self.lay.adaptedLuminanceOffset) + 4].zero_()

    def buffers(self, tonemap=3, bloom=1, auto=1, tc=1.0, fixed=0.18, blended=True):
        from basicrenderer_amd import capi
        b = capi.DisplayBuffers()
        b.structSize = C.sizeof(capi.DisplayBuffers)
        self.r.lib.brmi_display_default_settings(C.byref(b.settings))
        b.settings.tonemapType, b.settings.bloom, b.settings.autoExposure, b.settings.timeCoefficient, b.settings.fixedAdaptedLuminance = tonemap, bloom, auto, tc, fixed
        b.scratch, b.scratchBytes, b.ldr, b.ldrBytes = self.scratch.data_ptr(), int(self.lay.scratchBytes), self.ldr.data_ptr(), int(self.lay.ldrBytes)
        if blended:
            b.blendedHdr, b.blendedHdrBytes = self.blended.data_ptr(), int(self.lay.blendedHdrBytes)
        return b

    def bind(self, **kw):
        rc = self.r.lib.brmi_set_display(self.r._h, C.byref(self.buffers(**kw)))
        assert rc == 0, self.r.lib.brmi_last_error(self.r._h)

    def poke_hdr(self, rgb16):
        from basicrenderer_amd import capi
        from basicrenderer_amd.renderer import tile
        raw = self.r.torch.from_numpy(tile(d.halves_to_u64(rgb16)).view(np.uint8).reshape(-1)).to(self.r.device)
        self.r.res[capi.RES["HDR_COLOR"]][: raw.numel()].copy_(raw)

    def hdr_bytes(self):
        from basicrenderer_amd import capi
        self.r.torch.cuda.synchronize()
        return self.r.res[capi.RES["HDR_COLOR"]].cpu().numpy().copy()

    def words(self, off, n, dtype=np.uint32):
        self.r.torch.cuda.synchronize()
        return self.scratch[int(off): int(off) + 4 * n].cpu().numpy().view(dtype).copy()

    def level(self, k):
        """Bloom level k (1 .. 5) as (h, w, 4) float16."""
        from basicrenderer_amd.renderer import detile
        p = self.lay.bloom[k - 1]
        self.r.torch.cuda.synchronize()
        raw = self.scratch[int(p.offset): int(p.offset) + int(p.bytes)].cpu().numpy().view(np.uint64)
        return d.u64_to_halves(detile(raw, p.width, p.height))

    def write_level(self, k, rgb16):
        from basicrenderer_amd.renderer import tile
        p = self.lay.bloom[k - 1]
        raw = self.r.torch.from_numpy(tile(d.halves_to_u64(rgb16)).view(np.uint8).reshape(-1)).to(self.r.device)
        self.scratch[int(p.offset): int(p.offset) + raw.numel()].copy_(raw)

    def ldr_image(self):
        self.r.torch.cuda.synchronize()
        return self.ldr[: self.W * self.H * 4].cpu().numpy().reshape(self.H, self.W, 4)

    def blended_image(self):
        from basicrenderer_amd.renderer import detile
        self.r.torch.cuda.synchronize()
        return d.u64_to_halves(detile(self.blended[: int(self.lay.blendedHdrBytes)].cpu().numpy().view(np.uint64), self.W, self.H))

    def guards_intact(self):
        self.r.torch.cuda.synchronize()
        return all(bool((t[int(n):] == FILL).all()) for t, n in ((self.scratch, self.lay.scratchBytes), (self.ldr, self.lay.ldrBytes), (self.blended, self.lay.blendedHdrBytes)))

    def untouched(self):
        self.r.torch.cuda.synchronize()
        return bool((self.scratch == FILL).all()) and bool((self.ldr == FILL).all()) and bool((self.blended == FILL).all())

    def control(self):
        return self.words(self.lay.controlBlockOffset, 96, np.float32)

    def close(self):
        self.r.close()


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(width, height):
        if (width, height) not in made:
            made[(width, height)] = Rig(width, height)
        return made[(width, height)]
    yield get
    for rig in made.values():
        rig.close()


def _params_of(control):
    """display_ref's LPM parameters from the device's control block (float64 of the fp32 words): a stage is judged from the input it was given."""
    c = np.asarray(control, dtype=np.float64)
    return dict(saturation=c[0:3], contrast=c[3], toneScaleBias=c[4:6], lumaT=c[6:9], crosstalk=c[9:12], rcpLumaT=c[12:15], shoulderContrast=c[24])


def _check_halves(got16, value64, fragile, what):
    """Bit patterns equal outside fragile channels; fragile ones within one half step."""
    want = d.to_half(value64)
    gb, wb = got16.view(np.uint16).astype(np.int64), want.view(np.uint16).astype(np.int64)
    bad = np.argwhere((gb != wb) & ~fragile)
    print(f"{what}: {int((gb != wb).sum())} of {gb.size} halves differ, {int(fragile.sum())} are fragile")
    assert len(bad) == 0, (what, len(bad), bad[:4], got16[tuple(bad[0])], want[tuple(bad[0])])
    assert (np.abs(gb - wb) <= 1).all(), what


@pytest.mark.parametrize("width,height", d.SIZES)
@pytest.mark.parametrize("kind", d.HISTOGRAM_KINDS)
def test_histogram(rigs, kind, width, height):
    """1: the counts sum to W * H and equal the float64 histogram but for fragile pixels, each of which may sit one bin away."""
    rig = rigs(width, height)
    img = d.case(kind, width, height)
    rig.refill(); rig.poke_hdr(img); rig.bind(bloom=0)
    assert rig.r.lib.brmi_debug_display_histogram(rig.r._h, rig.r._s()) == 0, rig.r.lib.brmi_last_error(rig.r._h)
    got, want = rig.words(rig.lay.histogramOffset, 256).astype(np.int64), d.histogram(img).astype(np.int64)
    bins64, fragile = d.bins_of(img, np.float64), d.fragile_bins(img)
    sure = np.bincount(bins64[~fragile], minlength=256)
    reach = np.bincount(np.concatenate([np.clip(bins64[fragile] + k, 0, 255) for k in (-1, 0, 1)]), minlength=256) if fragile.any() else np.zeros(256, np.int64)
    print(f"{kind} {width}x{height}: {int(np.abs(got - want).sum())} counts differ, fragile pixels {int(fragile.sum())}, bin 0 holds {int(want[0])}")
    assert got.sum() == width * height
    assert (got >= sure).all() and (got <= sure + reach).all() and np.abs(got - want).sum() <= 2 * int(fragile.sum())
    if kind == "dark":
        assert got[0] == width * height
    if kind == "halfzero":
        assert got[0] >= width * height // 2
    assert rig.guards_intact()


@pytest.mark.parametrize("width,height", d.SIZES)
def test_average_adapts_over_three_frames(rigs, width, height):
    """2: time coefficients 1, 0.25 and 0 from a zeroed state, a different frame each time; the control block's fp32 words follow the adapted luminance."""
    rig = rigs(width, height)
    rig.refill()
    m = d.margins()
    last = 0.0
    for kind, tc in (("ramp", 1.0), ("halfzero", 0.25), ("ramp", 0.0)):
        img = d.case(kind, width, height)
        rig.poke_hdr(img); rig.bind(bloom=0, tc=tc)
        rig.r.stage("display_exposure")
        got = float(rig.words(rig.lay.adaptedLuminanceOffset, 1, np.float32)[0])
        hist = d.histogram(img)
        fragile = int(d.fragile_bins(img).sum())
        avg = float(d.average_luminance(hist, width * height, np.float64))
        want = float(d.adapt(last, avg, tc, np.float64))
        slack = (fragile * float(d.LOG_RANGE) / 254.0 / max(width * height - int(hist[0]), 1) * np.log(2.0) + m["adapted"] + 4e-7) * avg
        print(f"{width}x{height} tc {tc}: adapted {got:.9g}, float64 {want:.9g}")
        assert abs(got - want) <= slack + 4e-7 * abs(want)
        assert (rig.words(rig.lay.histogramOffset, 256) == 0).all()
        ctl = rig.control().astype(np.float64)
        c64 = d.lpm_control(d.lpm_params(np.float32(got), np.float64))
        rel = np.abs(ctl - c64) / np.maximum(np.abs(c64), 1e-30)
        assert rel.max() <= max(m["control"], 4e-6), (rel.argmax(), ctl[rel.argmax()], c64[rel.argmax()])
        assert (ctl[15:24] == 0).all() and (ctl[28:] == 0).all()
        last = got
    assert last == float(rig.words(rig.lay.adaptedLuminanceOffset, 1, np.float32)[0]) and rig.guards_intact()


@pytest.mark.parametrize("width,height", d.SIZES)
def test_bloom_level_by_level(rigs, width, height):
    """3: every BloomSamplePass from sources the test wrote (downsamples: the float64 chain's halves; upsamples and the blend: display_ref.upsample_case and
    blend_case, where rounding ties are rare), then the stage as a whole equals the passes one by one."""
    rig = rigs(width, height)
    img = d.case("glow", width, height)
    down, up, _ = d.bloom_chain(img)
    rig.refill(); rig.poke_hdr(img); rig.bind()
    before = rig.hdr_bytes()
    lib, h = rig.r.lib, rig.r._h
    cut = 0
    for i in range(5):
        if i:
            rig.write_level(i, down[i])
        assert lib.brmi_debug_display_bloom_pass(h, i, 0, rig.r._s()) == 0, lib.brmi_last_error(h)
        got = rig.level(i + 1)
        value, length, kept = d.downsample(down[i], np.float64)
        sure = ~d.fragile_cut(length)
        assert got.shape[:2] == (height >> (i + 1), width >> (i + 1))
        assert (got[..., 3] == 1.0).all()
        dropped = (got[..., :3].view(np.uint16) == 0).all(-1)
        assert np.array_equal(dropped[sure], ~kept[sure]), i      # the thresholded texels are exactly (0, 0, 0, 1)
        same = dropped == ~kept
        _check_halves(got[..., :3][same], value[same], d.fragile_halves(value, "down")[same], f"down {i}")
        cut += int(dropped.sum())
    assert cut > 0
    for i in range(4, 0, -1):
        src, dst = d.upsample_case(width, height, i)
        rig.write_level(i + 1, src); rig.write_level(i, dst)
        assert lib.brmi_debug_display_bloom_pass(h, i, 1, rig.r._s()) == 0, lib.brmi_last_error(h)
        value = d.upsample(src, dst, np.float64)
        got = rig.level(i)
        assert (got[..., 3] == 1.0).all()
        _check_halves(got[..., :3], value, d.fragile_halves(value, "up"), f"up {i}")
    blend_img, level1 = d.blend_case(width, height)
    assert np.array_equal(blend_img.view(np.uint16), img.view(np.uint16))      # the frame already poked
    rig.write_level(1, level1)
    rig.r.stage("display_resolve")
    value = d.blend(img, level1, np.float64)
    got = rig.blended_image()
    _check_halves(got[..., :3], value, d.fragile_halves(value, "blend"), "blend")
    assert (got[..., 3] == 1.0).all()      # the input's alpha
    # the stage as a whole: the same launches in the reference's order
    rig.r.stage("display_bloom")
    whole = [rig.level(k).copy() for k in range(1, 6)]
    for i in range(5):
        assert lib.brmi_debug_display_bloom_pass(h, i, 0, rig.r._s()) == 0
    for i in range(4, 0, -1):
        assert lib.brmi_debug_display_bloom_pass(h, i, 1, rig.r._s()) == 0
    for k in range(1, 6):
        assert np.array_equal(whole[k - 1].view(np.uint16), rig.level(k).view(np.uint16)), k
    assert np.array_equal(before, rig.hdr_bytes()) and rig.guards_intact()


@pytest.mark.parametrize("width,height", d.SIZES)
@pytest.mark.parametrize("curve", range(5))
def test_resolve(rigs, curve, width, height):
    """4: RGBA8 exact outside fragile channels, within one code inside them, alpha 255; without bloom from the HDR halves, with bloom from the blended halves
    the same launch wrote; autoExposure 0 with a fixed luminance."""
    rig = rigs(width, height)
    for kind in d.RESOLVE_KINDS:
        img = d.case(kind, width, height)
        rig.refill(); rig.poke_hdr(img); rig.bind(tonemap=curve, bloom=0)
        rig.r.stage("display_exposure"); rig.r.stage("display_resolve")
        _check_codes(rig.ldr_image(), d.resolve(curve, img, np.float64, _params_of(rig.control())), f"{d.CURVES[curve]} {kind}")
        assert (rig.blended_image().view(np.uint16) == 0xCDCD).all()      # not written without bloom
    img = d.case("glow", width, height)
    rig.refill(); rig.poke_hdr(img); rig.bind(tonemap=curve, bloom=1, auto=0, fixed=0.7)
    for stage in ("display_exposure", "display_bloom", "display_resolve"):
        rig.r.stage(stage)
    assert rig.words(rig.lay.adaptedLuminanceOffset, 1)[0] == 0      # autoExposure 0 leaves the adapted luminance alone
    ctl = rig.control().astype(np.float64)
    c64 = d.lpm_control(d.lpm_params(np.float32(0.7), np.float64))
    assert (np.abs(ctl - c64) / np.maximum(np.abs(c64), 1e-30)).max() <= max(d.margins()["control"], 4e-6)
    blended = rig.blended_image()[..., :3]
    _check_codes(rig.ldr_image(), d.resolve(curve, blended, np.float64, _params_of(ctl)), f"{d.CURVES[curve]} glow + bloom")
    _check_chain(blended, img, f"{d.CURVES[curve]} glow {width}x{height}")
    assert not np.array_equal(blended.view(np.uint16), img.view(np.uint16)) and rig.guards_intact()


def _check_chain(blended16, hdr16, what):
    """The blended level 0 a whole chain left, against the float64 chain from the same HDR.  The stated tolerance for nine compounded stores: each pyramid
    store may be one half step (2^-10 of its value) off where it is fragile; the filters are convex sums and the upsamples add, so level 1 is off by at most
    9 * 2^-10 of the pyramid's largest value; the blend takes 0.04 of that and stores once more (one half step of the result).  A length within the margin of
    the cut may drop a texel whose channels are at most 1, at each of five levels: 0.04 * 5 more, only where the float64 chain has such a texel."""
    down, up, want16 = d.bloom_chain(hdr16)
    want = want16.astype(np.float64)
    near_cut = any(bool(d.fragile_cut(d.downsample(down[i], np.float64)[1]).any()) for i in range(5))
    top = max(float(np.max(level.astype(np.float64))) for level in up[1:])
    spacing = np.maximum(np.spacing(np.abs(want16)).astype(np.float64), 2.0 ** -24)
    bound = spacing + 0.04 * 9 * 2.0 ** -10 * top + (0.04 * 5 if near_cut else 0.0)
    err = np.abs(blended16.astype(np.float64) - want)
    print(f"{what}: blended against the float64 chain: largest difference {err.max():.3g}, {float((err / spacing).max()):.3g} half steps; bound beyond one step "
          f"{0.04 * 9 * 2.0 ** -10 * top:.3g}, fragile cut {near_cut}; {int((blended16.view(np.uint16) != want16.view(np.uint16)).sum())} of {err.size} halves differ")
    assert (err <= bound).all(), (what, float(err.max()))


def _check_codes(got, value64, what):
    want, fragile = d.codes_of(value64), d.fragile_codes(value64)
    diff = np.abs(got[..., :3].astype(np.int64) - want)
    print(f"{what}: {int((diff != 0).sum())} of {diff.size} codes differ; fragile {int(fragile.sum())}")
    bad = np.argwhere((diff != 0) & ~fragile)
    assert len(bad) == 0, (what, len(bad), bad[:4], got[tuple(bad[0][:2])], value64[tuple(bad[0][:2])])
    assert (diff <= 1).all() and (got[..., 3] == 255).all(), what


def test_refusals_launch_nothing(rigs):
    """6: every refusal leaves the 0xCD buffers as they were, and so do the stages and the frame of a pass with nothing bound."""
    from basicrenderer_amd import Scene
    from basicrenderer_amd.renderer import VisibilityRenderer
    rig = rigs(64, 40)
    lib, INVALID, STATE = rig.r.lib, -1, -4
    rig.refill(zero_state=False)
    assert lib.brmi_set_display(rig.r._h, None) == 0
    for over in (dict(tonemap=5), dict(bloom=2), dict(auto=2), dict(tc=float("nan")), dict(fixed=float("inf"))):
        assert lib.brmi_set_display(rig.r._h, C.byref(rig.buffers(**over))) == INVALID, over
    for field in ("structSize", "scratchBytes", "ldrBytes", "blendedHdrBytes"):
        b = rig.buffers(); setattr(b, field, getattr(b, field) - 1)
        assert lib.brmi_set_display(rig.r._h, C.byref(b)) == INVALID, field
    b = rig.buffers(); b.scratch += 8
    assert lib.brmi_set_display(rig.r._h, C.byref(b)) == INVALID
    b = rig.buffers(); b.ldr = None
    assert lib.brmi_set_display(rig.r._h, C.byref(b)) == INVALID
    b = rig.buffers(); b.settings.logLuminanceRange = 0.0
    assert lib.brmi_set_display(rig.r._h, C.byref(b)) == INVALID
    for key, v in (("minLogLuminance", float("nan")), ("minLogLuminance", float("inf")), ("logLuminanceRange", float("nan"))):
        b = rig.buffers(); setattr(b.settings, key, v)
        assert lib.brmi_set_display(rig.r._h, C.byref(b)) == INVALID, key
    for field, by in (("ldr", 2), ("blendedHdr", 8)):      # misaligned
        b = rig.buffers()
        setattr(b, field, getattr(b, field) + by)
        assert lib.brmi_set_display(rig.r._h, C.byref(b)) == INVALID, field
    for stage in ("brmi_display_exposure", "brmi_display_bloom", "brmi_display_resolve"):
        assert getattr(lib, stage)(rig.r._h, rig.r._s()) == STATE
    assert lib.brmi_debug_display_bloom_pass(rig.r._h, 0, 0, rig.r._s()) == STATE
    rig.r.execute()      # a frame with nothing bound does not touch them either
    assert rig.untouched()
    for kw, size in ((dict(band=(8, 24)), (64, 40)), (dict(dynamicBand=1), (64, 40)), (dict(stripes=(16, 2, 0)), (64, 64)), (dict(), (40, 24))):
        r = VisibilityRenderer(Scene("tiny", size[0], size[1], point_lights=2), **kw)
        try:
            assert lib.brmi_set_display(r._h, C.byref(rig.buffers())) == INVALID, kw      # (larger than this pass needs: the refusal is about the partition, or the bloom's 32 pixels)
            assert lib.brmi_display_resolve(r._h, r._s()) == STATE
        finally:
            r.close()
    assert rig.untouched()


# ---------------------------------------------------------------- frames ---------------------------------------------------------------------------------
def test_frames_bound_is_unbound_plus_ldr():
    """5: the "tiny" scene with environment and skybox through brmi_execute and brmi_execute_split: visibility, depth, G-buffer planes and HDR byte for byte
    those of the unbound pass; the blended halves follow the float64 chain from that HDR and equal, like every level and ldr(), what the three stages leave
    one by one; ldr() is the restatement of the blended halves; after set_display(None) the frame leaves fresh 0xCD buffers alone."""
    from basicrenderer_amd import Scene
    from basicrenderer_amd.environment import Environment
    from basicrenderer_amd.renderer import VisibilityRenderer
    sc = Scene("tiny", 160, 90, point_lights=5, seed=3)
    r = VisibilityRenderer(sc)
    try:
        torch = r.torch
        r.set_environment(Environment.procedural(16), skybox=True)
        r.execute()

        def surfaces():
            torch.cuda.synchronize()
            g = r.gbuffer()
            return [r.visibility(), r.depth().view(np.uint32), r.hdr()] + [g[key] for key in sorted(g)]
        unbound = [a.copy() for a in surfaces()]
        for split in (False, True):
            r.set_display("lpm", bloom=True, time_coefficient=1.0, fill=FILL, guard=GUARD)
            other = torch.cuda.Stream(device=r.device) if split else None
            r.execute(shading_stream=other)
            if other is not None:
                other.synchronize()
            for a, b in zip(unbound, surfaces()):
                assert np.array_equal(a, b)
            hdr16 = d.u64_to_halves(r.hdr())[..., :3]
            hist = d.histogram(hdr16)
            assert abs(r.adapted_luminance() - float(d.average_luminance(hist, 160 * 90, np.float64))) <= 1e-3 * r.adapted_luminance()      # (fragile bins move it a little)
            blended = d.u64_to_halves(r.blended_hdr())[..., :3]
            lay = r._display["layout"]
            o = int(lay.controlBlockOffset)
            ctl = r._display["scratch"][o: o + 384].cpu().numpy().view(np.float32)
            _check_codes(r.ldr(), d.resolve("lpm", blended, np.float64, _params_of(ctl)), f"frame split={split}")
            _check_chain(blended, hdr16, f"frame split={split}")      # the frame's bloom ran, ahead of the resolve, from this HDR
            # ... and the frame's chain is the three stages one by one from the same HDR, byte for byte, into buffers filled afresh
            from basicrenderer_amd.renderer import detile
            dis = r._display

            def chain_bytes():
                torch.cuda.synchronize()
                levels = [dis["scratch"][int(p.offset): int(p.offset) + int(p.bytes)].cpu().numpy().view(np.uint64) for p in list(lay.bloom)[: int(lay.bloomLevels)]]
                return [detile(raw, p.width, p.height).copy() for raw, p in zip(levels, lay.bloom)] + [r.blended_hdr().copy(), r.ldr().copy(), ctl.copy()]
            frame = chain_bytes()
            for p in list(lay.bloom)[: int(lay.bloomLevels)]:
                dis["scratch"][int(p.offset): int(p.offset) + int(p.bytes)].fill_(FILL)
            dis["blended"][: int(lay.blendedHdrBytes)].fill_(FILL); dis["ldr"][: int(lay.ldrBytes)].fill_(FILL)
            for stage in ("display_exposure", "display_bloom", "display_resolve"):
                r.stage(stage)
            ctl = dis["scratch"][o: o + 384].cpu().numpy().view(np.float32)
            for k, (a, b) in enumerate(zip(frame, chain_bytes())):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (split, k)
            assert r.display_guards_intact()
            if split:
                first = r.ldr().copy()
                r.set_display("lpm", bloom=True, time_coefficient=1.0)      # settings only: the buffers and the adapted luminance stay
                r.execute()
                assert np.array_equal(r.ldr(), first)
            r.set_display(None)
        # off is off: the frame of the unbound pass again, and a stage finds nothing bound
        r.execute()
        for a, b in zip(unbound, surfaces()):
            assert np.array_equal(a, b)
        assert r.lib.brmi_display_resolve(r._h, r._s()) == -4
    finally:
        r.close()
