"""Debug views (perFrame.outputType) on the GPU: k_debug_payload and k_debug_resolve against tests/debug_view_ref.py.

The payload is held BIT FOR BIT to the numpy restatement evaluated on the renderer's own read-back surfaces (which the parity suite holds to the
oracle); the resolved image to the float64 restatement within one code, and exactly wherever the float64 value is not next to a rounding boundary."""
import ctypes as C

import numpy as np
import pytest

import debug_view_ref as ref

pytestmark = pytest.mark.gpu

# A generator scene with several instances, two LOD levels, textured, layered and constant-factor materials and 24 point lights + the sun, at a size that is
# no multiple of 8 in either direction (700 = 87.5 tiles, 420 = 52.5).  Chosen on the CPU with the oracle so that the guards below hold: 91 % covered,
# 79 meshlet indices, 13 groups, 16 slices, 5 light counts.
W, H = 700, 420
SCENE_KW = dict(point_lights=24, size_scale=0.1, lod_levels=2, material_features=8 | 3)
PLANES = ("normals", "albedo", "coat", "emissive", "fuzz", "mr", "motion")
FILL_WORD, FILL_BYTE = 0x5A5A5A5A, 0x2B


def make_scene(step=0, width=W, height=H):
    from conftest import Scene
    return Scene("bistro", width, height, camera_step=step, **SCENE_KW)


def surfaces(r):
    """Every image of the frame, untiled (uncovered pixels of the planes hold whatever they held: compare frames of the same pass, or covered pixels)."""
    out = dict(vis=r.visibility(), depth=r.depth().view(np.uint32), hdr=r.hdr())
    out.update(r.gbuffer())
    return out


def fill_targets(r):
    """What the test puts into the targets before a frame: pixels the library must not write keep it."""
    r.torch.cuda.synchronize()
    r._debug_view["payload"].view(r.torch.int32).fill_(FILL_WORD)
    r._debug_view["image"].fill_(FILL_BYTE)


@pytest.fixture(scope="module")
def scene():
    return make_scene()


@pytest.fixture(scope="module")
def renderer(scene):
    from basicrenderer_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(scene)
    yield r
    r.close()


@pytest.fixture(scope="module")
def plain(renderer):
    """The frame with outputType == 0 and nothing bound: its surfaces and the restatement's input made of them.  Computed once, never changed."""
    renderer.set_debug_view(None)
    renderer.execute()
    s = surfaces(renderer)
    fr = ref.frame_of_renderer(renderer)
    for a in list(s.values()) + [v for k, v in fr.items() if k not in ("camera", "per_frame")]:      # (those two are the scene's own arrays)
        a.setflags(write=False)
    return s, fr


@pytest.fixture(scope="module")
def views(renderer, plain):
    """One frame per mode, rendered on first use: (payload, image, surfaces of that frame)."""
    cache = {}

    def get(mode):
        if mode not in cache:
            renderer.set_debug_view(mode)
            fill_targets(renderer)
            renderer.execute()
            cache[mode] = (renderer.debug_payload(), renderer.debug_image(), surfaces(renderer))
        return cache[mode]

    return get


def test_the_scene_exercises_every_view(plain):
    """Coverage guards, from the reference side: the comparisons below cannot pass on an empty picture."""
    _, fr = plain
    covered = fr["vis"] != ref.VIS_EMPTY
    assert np.array_equal(covered, fr["depth"].view(np.uint32) != np.uint32(ref.DEPTH_EMPTY_BITS))
    share = covered.mean()
    print(f"covered {share:.3f}")
    assert 0.20 <= share <= 0.95
    meshlets, groups = ref.payload("MESHLETS", fr)[covered][:, 0], ref.payload("GEOMETRY_GROUP", fr)[covered][:, 0]
    slices, counts = ref.payload("LIGHT_CLUSTER_ID", fr)[covered][:, 0], ref.payload("LIGHT_CLUSTER_LIGHT_COUNT", fr)[covered][:, 0]
    print("meshlets", len(np.unique(meshlets)), "groups", len(np.unique(groups)), "slices", len(np.unique(slices)), "light counts", np.unique(counts))
    assert len(np.unique(meshlets)) >= 8 and len(np.unique(groups)) >= 2
    assert len(np.unique(slices)) >= 3 and len(np.unique(counts)) >= 3
    # textured and constant materials both show: the albedo plane is neither one value nor noise
    assert 8 <= len(np.unique(fr["albedo"][covered])) and len(np.unique(fr["emissive"][covered])) >= 1


@pytest.mark.parametrize("name", sorted(ref.MODES, key=ref.MODES.get))
def test_payload_equals_the_restatement_bit_for_bit(views, plain, name):
    base, _ = plain
    payload, _, s = views(ref.MODES[name])
    # the frame itself does not know about the mode: HDR and every plane are those of the outputType == 0 frame (same pass: all bytes)
    for k in base:
        assert np.array_equal(s[k], base[k]), f"{name}: {k} differs from the plain frame"
    fr = dict(plain[1])
    want = ref.payload(name, fr)
    sentinel = (want[..., 0] == ref.SENTINEL) & (want[..., 1] == ref.SENTINEL)
    diff = (payload != want).any(axis=-1)
    print(f"{name}: {int(diff.sum())} of {diff.size} pixels differ; {int(sentinel.sum())} sentinel pixels")
    assert np.array_equal(payload, want), (name, np.argwhere(diff)[:5].tolist(), payload[diff][:3].tolist(), want[diff][:3].tolist())


@pytest.mark.parametrize("name", sorted(ref.MODES, key=ref.MODES.get))
def test_resolved_image_against_the_float64_restatement(views, name):
    payload, image, _ = views(ref.MODES[name])
    written, x = ref.resolve_values(name, payload)
    want = ref.resolve(name, payload, np.full((H, W, 4), FILL_BYTE, dtype=np.uint8))
    # sentinel pixels keep the fill, written pixels are opaque
    assert (image[~written] == FILL_BYTE).all()
    assert (image[written][:, 3] == 255).all()
    got, exp = image[written][:, :3].astype(np.int32), want[written][:, :3].astype(np.int32)
    differ = got != exp
    print(f"{name}: {differ.mean():.2e} of the channels differ at all, max {np.abs(got - exp).max()} code")
    assert np.abs(got - exp).max() <= 1
    xs = x[written]
    away = np.isnan(xs) | (np.abs(xs - np.round(xs)) > 0.01)      # more than 0.01 of a code from the integer where floor() changes
    assert not differ[away].any()
    assert away.mean() > 0.9


def test_moving_camera_motion_vectors_and_light_views():
    from basicrenderer_amd.renderer import VisibilityRenderer
    sc0, sc1 = make_scene(0), make_scene(1)
    r = VisibilityRenderer(sc0)
    try:
        r.execute()
        for name in ("MOTION_VECTORS", "LIGHT_CLUSTER_ID", "LIGHT_CLUSTER_LIGHT_COUNT", "DEPTH"):
            r.set_debug_view(name)
            r.set_camera_from(sc1, frame_index=1)
            r.execute()
            fr = ref.frame_of_renderer(r, camera=sc1.arrays["cameras"], per_frame=sc1.arrays["perFrame"])
            covered = fr["vis"] != ref.VIS_EMPTY
            if name == "MOTION_VECTORS":
                moving = int(((fr["motion"] != 0) & covered).sum())
                print("pixels with a non-zero motion vector:", moving)
                assert moving > 0
            assert 0.20 <= covered.mean() <= 0.95
            assert np.array_equal(r.debug_payload(), ref.payload(name, fr)), name
    finally:
        r.close()


def test_poked_surfaces_empty_keys_and_colours_that_store_zero():
    """What no rendered frame holds, written into the surfaces behind a frame and seen through the stage entry: keys that name a cluster beyond the list or a
    triangle beyond the cluster's count are empty (a scene from the library's own LOD builder: two of its clusters have 127 triangles, so triangle id 127
    is the case); negative, NaN, -0 and infinite colour channels resolve to 0 / 0 / 0 / 255."""
    from conftest import Scene
    from basicrenderer_amd import capi
    from basicrenderer_amd.renderer import VisibilityRenderer, tile
    w, h = 256, 144
    sc = Scene("tiny", w, h, point_lights=4, lod_builder="own")
    r = VisibilityRenderer(sc)
    try:
        torch = r.torch
        r.execute()

        def poke(rid, img):
            raw = torch.from_numpy(tile(img).view(np.uint8).reshape(-1)).to(r.device)
            r.res[capi.RES[rid]][: raw.numel()].copy_(raw)

        # -- colours: every covered pixel's emissive word becomes one of five patterns of halves
        fr = ref.frame_of_renderer(r)
        covered = fr["vis"] != ref.VIS_EMPTY
        assert covered.sum() > 1000
        minus, nan, half, inf, mzero = 0xBC00, 0x7E00, 0x3800, 0x7C00, 0x8000
        words = np.array([minus | (nan << 16) | (half << 32), inf | (mzero << 16) | (minus << 32), nan | (nan << 16) | (nan << 32),
                          half | (inf << 16) | (mzero << 32), mzero | (half << 16) | (inf << 32)], dtype=np.uint64)
        yy, xx = np.mgrid[0:h, 0:w]
        fr["emissive"] = words[(xx + 3 * yy) % 5]
        poke("GBUF_EMISSIVE", fr["emissive"])
        r.set_debug_view("EMISSIVE")
        fill_targets(r)
        r.stage("debug_view")
        payload, image = r.debug_payload(), r.debug_image()
        assert np.array_equal(payload, ref.payload("EMISSIVE", fr))
        want = ref.resolve("EMISSIVE", payload, np.full((h, w, 4), FILL_BYTE, dtype=np.uint8))
        assert np.array_equal(image, want)      # every channel is 0, 255 or pow(0.5, 1 / 2.2) * 255 + 0.5 = 186.6: nowhere near a rounding boundary
        seen = {tuple(c) for c in image[covered].reshape(-1, 4).tolist()}
        m = 186
        assert seen == {(0, 0, m, 255), (255, 0, 0, 255), (0, 0, 0, 255), (m, 255, 0, 255), (0, m, 255, 255)}, seen

        # -- keys: pixel k names (cluster k / 128, triangle k % 128) for every listed cluster, then clusters beyond the list, then nothing
        clusters = r.visible_clusters()
        n = len(clusters)
        counts = ref.tri_counts_from_oracle(sc, clusters)
        assert n * 128 + 256 < w * h and (counts < 128).any() and (counts == 128).any()
        k = np.arange(n * 128 + 256, dtype=np.uint64)
        depth_bits = np.uint64(int(np.float32(2.0).view(np.uint32)) >> 1)
        vis = np.full(w * h, ref.VIS_EMPTY, dtype=np.uint64)
        vis[: len(k)] = (depth_bits << np.uint64(33)) | ((k >> np.uint64(7)) << np.uint64(7)) | (k & np.uint64(127))      # (k / 128 >= n for the last 256)
        vis[len(k) - 1] = (depth_bits << np.uint64(33)) | (np.uint64(0x3FFFFFF) << np.uint64(7))                          # the largest index a key can name
        fr = dict(fr, vis=vis.reshape(h, w), clusters=clusters, tri_counts=counts)
        poke("VISIBILITY", fr["vis"])
        for name in ("MESHLETS", "GEOMETRY_GROUP"):
            r.set_debug_view(name)
            fill_targets(r)
            r.stage("debug_view")
            want = ref.payload(name, fr)
            empty = (want[..., 0] == ref.SENTINEL) & (want[..., 1] == ref.SENTINEL)
            assert int((~empty).sum()) == int(counts.sum()) and int(counts.sum()) < n * 128      # some keys are empty by the triangle rule alone
            assert np.array_equal(r.debug_payload(), want), name
    finally:
        r.close()


def test_band_writes_its_rows_only(scene, plain):
    """A band whose ends split a tile row (rows 100 .. 300: 12.5 and 37.5 tiles), and a band moved with brmi_set_band: the band's rows equal the
    unbanded frame's, every other pixel of both targets keeps the test's fill."""
    from basicrenderer_amd.renderer import VisibilityRenderer
    _, fr = plain
    for make, (y0, y1) in ((lambda: VisibilityRenderer(scene, band=(100, 300)), (100, 300)), (lambda: VisibilityRenderer(scene, dynamicBand=1), (104, 296))):
        r = make()
        try:
            if r.cfg.dynamicBand:
                r.set_band(y0, y1)
            for name in ("MESHLETS", "NORMAL", "LIGHT_CLUSTER_LIGHT_COUNT"):
                r.set_debug_view(name)
                fill_targets(r)
                r.execute()
                raw = r._debug_view["payload"].cpu().numpy().view(np.uint32)
                payload, image = r.debug_payload(), r.debug_image()
                want = ref.payload(name, fr)
                assert np.array_equal(payload[y0:y1], want[y0:y1]), (name, y0, y1)
                outside = np.ones(H, dtype=bool)
                outside[y0:y1] = False
                assert (payload[outside] == FILL_WORD).all() and (image[outside] == FILL_BYTE).all()
                # ... the padding of the tiled target included: exactly the band's pixels were written
                assert int((raw.reshape(-1, 2) != FILL_WORD).any(axis=1).sum()) == (y1 - y0) * W
                colour = ref.resolve(name, want, np.full((H, W, 4), FILL_BYTE, dtype=np.uint8))
                assert np.abs(image[y0:y1].astype(np.int32) - colour[y0:y1].astype(np.int32)).max() <= 1
        finally:
            r.close()


def test_three_frames_in_flight_give_the_serial_payload():
    """A ring of three linked passes (brmi_set_history_source + brmi_execute_split), each with its own targets, light-count view: the last frame's payload
    is the one a single pass rendering the same frames in order writes."""
    import torch
    from basicrenderer_amd.renderer import VisibilityRenderer
    steps, ring = 4, 3
    scenes = [make_scene(s) for s in range(steps)]
    serial = VisibilityRenderer(make_scene(0), occlusion=True)
    passes = [VisibilityRenderer(make_scene(0), occlusion=True) for _ in range(ring)]
    try:
        serial.set_debug_view("LIGHT_CLUSTER_LIGHT_COUNT")
        for s in range(steps):
            serial.set_camera_from(scenes[s], frame_index=s)
            serial.execute()
        want = serial.debug_payload()
        assert np.array_equal(want, ref.payload(13, ref.frame_of_renderer(serial, camera=scenes[-1].arrays["cameras"], per_frame=scenes[-1].arrays["perFrame"])))
        for k in range(ring):
            passes[k].set_history_source(passes[(k - 1) % ring])
            passes[k].set_debug_view("LIGHT_CLUSTER_LIGHT_COUNT")
        geometry, shading = torch.cuda.Stream(priority=-1), torch.cuda.Stream()
        torch.cuda.synchronize()
        for s in range(steps):
            with torch.cuda.stream(geometry):
                passes[s % ring].set_camera_from(scenes[s], frame_index=s)
                passes[s % ring].execute(shading)
        torch.cuda.synchronize()
        last = passes[(steps - 1) % ring]
        assert np.array_equal(last.visibility(), serial.visibility())
        got = last.debug_payload()
        covered = (want[..., 0] != ref.SENTINEL) | (want[..., 1] != ref.SENTINEL)
        assert 0.20 <= covered.mean() <= 0.95 and len(np.unique(want[covered][:, 0])) >= 3
        assert np.array_equal(got, want)
    finally:
        for p in passes + [serial]:
            p.close()


def test_refusals_and_unbinding(renderer, plain, views):
    from basicrenderer_amd import Scene, capi
    from basicrenderer_amd.renderer import BrmiError, VisibilityRenderer
    base, _ = plain
    lib = renderer.lib
    # modes outside the table: the frame's debug stage refuses them by number
    for mode in (11, 15, 33, 99):
        with pytest.raises(BrmiError, match=rf"set_debug_view: outputType {mode} is not a debug view"):
            renderer.set_debug_view(mode)
        renderer.set_debug_view(mode, check=False)      # the library's own refusal: before the frame launches anything
        before = renderer.counters()
        renderer.res[capi.RES["VISIBILITY"]][:64].fill_(0x11)
        with pytest.raises(BrmiError, match=rf"brmi_debug_view: outputType {mode} is not a debug view"):
            renderer.execute()
        assert (renderer.res[capi.RES["VISIBILITY"]][:64] == 0x11).all().item()      # not even the visibility clear ran
        assert renderer.counters().visibleClusters == before.visibleClusters
    with pytest.raises(BrmiError, match="no debug view named"):
        renderer.set_debug_view("model_normals")
    # a short struct, a null payload
    b = capi.DebugViewBuffers()
    b.structSize = C.sizeof(capi.DebugViewBuffers) - 8
    b.payload, b.payloadBytes = renderer.res[capi.RES["HDR_COLOR"]].data_ptr(), int(lib.brmi_debug_view_bytes(W, H))
    assert lib.brmi_set_debug_view(renderer._h, C.byref(b)) == -1 and b"structSize" in lib.brmi_last_error(renderer._h)
    b.structSize, b.payload = C.sizeof(capi.DebugViewBuffers), None
    assert lib.brmi_set_debug_view(renderer._h, C.byref(b)) == -1 and b"payload pointer is null" in lib.brmi_last_error(renderer._h)
    b.payload, b.payloadBytes = renderer.res[capi.RES["HDR_COLOR"]].data_ptr(), int(lib.brmi_debug_view_bytes(W, H)) - 8
    assert lib.brmi_set_debug_view(renderer._h, C.byref(b)) == -1 and b"payload holds" in lib.brmi_last_error(renderer._h)
    # the interleaved partition
    striped = VisibilityRenderer(Scene("tiny", 256, 160, point_lights=2), stripes=(16, 2, 0))
    try:
        with pytest.raises(BrmiError, match="interleaved partition"):
            striped.set_debug_view("MESHLETS")
    finally:
        striped.close()
    # a call before brmi_setup
    cfg, h = capi.Config(), capi.vp()
    lib.brmi_default_config(C.byref(cfg), 64, 64)
    assert lib.brmi_create(C.byref(cfg), C.byref(h)) == 0
    try:
        assert lib.brmi_debug_view(h, None) == -4 and b"brmi_setup first" in lib.brmi_last_error(h)
    finally:
        lib.brmi_destroy(h)
    # the stage on its own, without a target: refused; with outputType == 0: nothing to do
    renderer.set_debug_view("MESHLETS")
    assert lib.brmi_set_debug_view(renderer._h, None) == 0
    assert lib.brmi_debug_view(renderer._h, renderer._s()) == -4 and b"no debug target bound" in lib.brmi_last_error(renderer._h)
    # NULL unbinds: with outputType still set, the frame is byte for byte the unbound one and the old targets are not touched
    fill_targets(renderer)
    renderer.execute()
    s = surfaces(renderer)
    for k in base:
        assert np.array_equal(s[k], base[k]), k
    assert (renderer.debug_payload() == FILL_WORD).all() and (renderer.debug_image() == FILL_BYTE).all()
    renderer.set_debug_view(None)
    assert lib.brmi_debug_view(renderer._h, renderer._s()) == 0
    # the stage entry on its own, behind a finished frame, writes what the frame's own call wrote
    renderer.set_debug_view("GEOMETRY_GROUP")
    renderer.execute()
    first = renderer.debug_payload()
    fill_targets(renderer)
    renderer.stage("debug_view")
    assert np.array_equal(renderer.debug_payload(), first) and np.array_equal(first, views(35)[0])
