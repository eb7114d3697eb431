"""Residency-aware cut and streaming feedback on the GPU (brmi_set_streaming / brmi_streaming_feedback).

Frame reference: the existing oracle on the transformed scene of tests/clod_residency.py.  Feedback reference: that module's numpy restatement.

Which case reaches which culling kernel (every one that carries the residency branch):
  * k_cull_hierarchy, eight draws to a wave (hierarchies of <= 8 nodes) and one draw to a wave (<= 256 nodes), and k_cull_clusters: the default
    frames of tiny_lod / tiny_ownlod / sponza_ownlod (test_frame_*, test_feedback_*);
  * k_cull_hierarchy's level walk: BRMI_TUNING flat_traversal=0 (phase 1) and every phase 2 of the occlusion test (replayed nodes);
  * k_traverse (with k_cull_instances in front): BRMI_TUNING cull_level_kernels=1;
  * k_cull_flat_level: BRMI_TUNING flat_levels_min_draws=1;
  * k_cull_flat_wide: the 686-node hierarchies of the `tiny`, lod_levels=7 scene.
The tuning keys are read by brmi_create / brmi_set_scene, so they are set around the construction of the renderer, as tests/test_parity_gpu.py does.
"""
import os

import numpy as np
import pytest

import clod_residency as cr
from conftest import SCENE_CASES, Scene
from test_residency_cpu import CASES, SETS, make_scene, residency_set

pytestmark = pytest.mark.gpu
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
COUNTER_FIELDS = ("instancesTested", "instancesVisible", "nodesVisited", "bucketRecords", "meshletsTested", "visibleClusters")


class _Tuning:
    def __init__(self, text):
        self.text, self.old = text, None

    def __enter__(self):
        self.old = os.environ.get("BRMI_TUNING")
        if self.text:
            os.environ["BRMI_TUNING"] = self.text

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("BRMI_TUNING", None)
        else:
            os.environ["BRMI_TUNING"] = self.old


def _half_ulp_distance(a_bits, b_bits):
    def key(h):
        h = h.astype(np.int32)
        return np.where(h & 0x8000, -(h & 0x7FFF), h & 0x7FFF)
    return np.abs(key(a_bits) - key(b_bits))


def _renderer(scene, tuning="", **kw):
    from basicrenderer_amd.renderer import VisibilityRenderer
    with _Tuning(tuning):
        return VisibilityRenderer(scene, stats=True, **kw)


@pytest.fixture(scope="module")
def references(scenes):
    """(case, set) -> (oracle frame of the transformed scene, restatement), computed once and left unchanged."""
    import orc
    cache = {}

    def get(name, which, maker=None, scene=None):
        if (name, which) not in cache:
            sc = scene if scene is not None else scenes(name)
            n, active = residency_set(sc, which)
            o = orc.OracleFrame(cr.transformed_scene(maker or make_scene(name), n, active)).run()
            cache[(name, which)] = (o, cr.restate(sc, n, active), n, active)
        return cache[(name, which)]

    return get


def _assert_frame(r, o, surfaces=True):
    gc = r.counters()
    assert gc.droppedRecords == 0 and gc.droppedClusters == 0
    for field in COUNTER_FIELDS:
        print(field, getattr(gc, field), getattr(o.counters, field))
        assert getattr(gc, field) == getattr(o.counters, field), field
    assert np.array_equal(r.visible_clusters(), o.clusters[: o.count])
    if not surfaces:
        return
    _assert_surfaces(r, o)


def _assert_surfaces(r, o):
    assert np.array_equal(r.visibility(), o.vis)
    assert np.array_equal(r.depth().view(np.uint32), o.depth.view(np.uint32))
    covered = o.vis != EMPTY
    gb = r.gbuffer()
    for key, ref in (("normals", o.normals), ("albedo", o.albedo), ("coat", o.coat), ("emissive", o.emissive), ("fuzz", o.fuzz), ("mr", o.mr), ("motion", o.motion)):
        a, b = gb[key][covered], ref[covered]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), key
    if covered.any():
        a = r.hdr().view(np.uint16).reshape(o.H, o.W, 4)[covered]
        b = o.hdr.view(np.uint16).reshape(o.H, o.W, 4)[covered]
        d = _half_ulp_distance(a, b)
        assert d.max() <= 1, f"max fp16 ULP distance {int(d.max())}"
        assert float((d > 0).mean()) < 0.02


def _assert_feedback(r, want):
    req, touched, counts = r.streaming_feedback()
    print("counts", counts, "expected", want["counts"])
    assert np.array_equal(counts, want["counts"])
    assert np.array_equal(touched, want["touched"])
    assert np.array_equal(req, want["requests"])


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("name", CASES)
def test_frame_and_feedback_equal_the_references(name, which, scenes, references):
    """1 + 2: list, counters and every surface equal the oracle's frame of the transformed scene; requests, touched groups and counts equal the
    restatement's reduced output exactly (occlusion off)."""
    o, want, n, active = references(name, which)
    r = _renderer(scenes(name))
    r.set_streaming(n, active)
    r.execute()
    _assert_frame(r, o)
    _assert_feedback(r, want)
    # what the reference asks for is what the rule allows: every touched group that is not resident and lies under activeGroupScanCount (in the
    # two 6- and 7-group scenes set (e) leaves none of those: [3, 4] and [4, 5] under a scan count of 3); the larger scene asks in every set but (a)
    groups = r.group_count()
    requestable = cr.effective_mask(groups, n, None) & (np.arange(groups) < (groups if active is None else active))
    assert len(want["touched"]) > 0
    assert np.array_equal(np.sort(want["requests"][:, 0]), want["touched"][requestable[want["touched"]]])
    if name == "sponza_ownlod" and which != "none":
        assert len(want["requests"]) > 0
        if which == "third_half_scan":
            assert len(want["requests"]) < len(references(name, "third")[1]["requests"])
    if which == "none":     # ... and equals a renderer that never heard of streaming, byte for byte on every surface
        from basicrenderer_amd import capi
        plain = _renderer(scenes(name))
        plain.execute()
        assert np.array_equal(plain.visible_clusters(), r.visible_clusters())
        plain.torch.cuda.synchronize()
        n_vis = plain.counters().visibleClusters
        for key in ("VISIBILITY", "LINEAR_DEPTH", "GBUF_NORMALS", "GBUF_ALBEDO", "GBUF_COAT", "GBUF_EMISSIVE", "GBUF_FUZZ", "GBUF_METALLIC_ROUGHNESS",
                    "GBUF_MOTION_VECTORS", "HDR_COLOR", "VISIBLE_CLUSTERS"):
            a, b = plain.res[capi.RES[key]], r.res[capi.RES[key]]
            if key == "VISIBLE_CLUSTERS":
                a, b = a[: n_vis * 16], b[: n_vis * 16]
            assert plain.torch.equal(a, b), key
        plain.close()
    r.close()


@pytest.mark.parametrize("tuning,name", [("flat_traversal=0", "sponza_ownlod"), ("cull_level_kernels=1", "sponza_ownlod"), ("flat_levels_min_draws=1", "sponza_ownlod"),
                                         ("flat_packed=0", "tiny_ownlod")])
@pytest.mark.parametrize("which", ["finest", "third_half_scan"])
def test_every_traversal_form_follows_the_rule(tuning, name, which, scenes, references):
    """6: the level walk, the level kernels, the level-synchronous flat traversal and the one-draw-per-wave flat evaluation give the same frame
    and the same feedback as the default launches."""
    o, want, n, active = references(name, which)
    r = _renderer(scenes(name), tuning)
    r.set_streaming(n, active)
    r.execute()
    _assert_frame(r, o, surfaces=False)
    _assert_feedback(r, want)
    r.close()


@pytest.mark.parametrize("which", ["third", "all"])
def test_wide_flat_hierarchies_follow_the_rule(which, references):
    """6: k_cull_flat_wide (hierarchies of 257 .. 8192 nodes: 686 here).  At this size the frame's cut touches the six coarsest of the 1029 groups:
    set (d) holds two of them, so the cut changes and four touched groups stay unrequested; set (b) asks for all six, at two priorities."""
    maker = lambda: Scene("tiny", 256, 144, point_lights=2, lod_levels=7)
    sc = maker()
    o, want, n, active = references("tiny_lod7", which, maker, sc)
    assert 0 < len(want["requests"]) and len(want["touched"]) > 2
    if which == "third":
        assert len(want["requests"]) < len(want["touched"])
    else:
        assert len(np.unique(want["requests"][:, 3] >> 16)) > 1
    r = _renderer(sc)
    r.set_streaming(n, active)
    r.execute()
    _assert_frame(r, o, surfaces=False)
    _assert_feedback(r, want)
    r.close()


def test_request_list_truncates_to_the_first_of_the_ordering(scenes, references):
    """4: request_capacity=8 on a case whose set (d) asks for more: the first 8 of the full ordering, counts[0] the full number."""
    o, want, n, active = references("sponza_ownlod", "third")
    assert len(want["requests"]) > 8
    r = _renderer(scenes("sponza_ownlod"))
    r.set_streaming(n, active, request_capacity=8, touched_capacity=4)
    r.execute()
    req, touched, counts = r.streaming_feedback()
    assert np.array_equal(counts, want["counts"])
    assert np.array_equal(req, want["requests"][:8]) and np.array_equal(touched, want["touched"][:4])
    r.close()


def test_occlusion_two_frames(references):
    """3: bistro_small with the library's own LOD builder, occlusion on, two frames: list and surfaces equal the oracle's two-phase frames of the
    transformed scene; what the frame asked for and touched is a subset of the occlusion-off frame's of the same camera."""
    import orc
    preset, W, H, kw = SCENE_CASES["bistro_small"]
    maker = lambda: Scene(preset, W, H, **dict(kw, lod_builder="own"))
    sc = maker()
    n, active = residency_set(sc, "finest")
    o = orc.OracleFrame(cr.transformed_scene(maker, n, active))
    r = _renderer(sc, occlusion=True)
    r.set_streaming(n, active)
    hz = None
    for _ in range(2):
        r.execute()
        hz = o.run_occlusion(hz)
    o.gbuffer(); o.light_cluster(); o.shade()
    assert np.array_equal(r.visible_clusters(), o.clusters[: o.count])
    _assert_surfaces(r, o)
    req, touched, counts = r.streaming_feedback()
    free = _renderer(sc)
    free.set_streaming(n, active)
    free.execute()
    freq, ftouched, _ = free.streaming_feedback()
    assert len(req) > 0 and set(req[:, 0].tolist()) <= set(freq[:, 0].tolist()) and set(touched.tolist()) <= set(ftouched.tolist())
    r.close(); free.close()


def test_three_frames_in_flight_keep_their_own_feedback(scenes, references):
    """5: two linked passes, frames on a geometry and a shading stream, N changed between frames: every frame's feedback is that frame's alone."""
    import torch
    name = "sponza_ownlod"
    sc = scenes(name)
    order = ["finest", "third", "all"]
    wants = [references(name, w) for w in order]
    pair = [_renderer(sc, occlusion=True), _renderer(sc, occlusion=True)]
    pair[0].set_history_source(pair[1]); pair[1].set_history_source(pair[0])
    geometry, shading = torch.cuda.Stream(priority=-1), torch.cuda.Stream()
    torch.cuda.synchronize()
    kept = []
    with torch.cuda.stream(geometry):
        for k, (o, want, n, active) in enumerate(wants):
            p = pair[k & 1]
            p.invalidate_hzb()                      # (no occlusion history: the restatement's frame)
            p.set_streaming(n, active)              # the residency bits are rewritten in stream order
            p.execute(shading)
            kept.append([t.clone() for t in p.streaming_tensors()])
    torch.cuda.synchronize()
    for k, (o, want, n, active) in enumerate(wants):
        req, touched, counts = pair[0].unpack_feedback(*[t.cpu().numpy() for t in kept[k]])
        assert np.array_equal(counts, want["counts"]), order[k]
        assert np.array_equal(req, want["requests"]) and np.array_equal(touched, want["touched"]), order[k]
    for p in pair:
        p.close()


def test_switching_off_and_refusals(scenes, oracle_frames):
    """7: brmi_set_streaming(NULL) after a streaming frame restores the plain frame; undersized scratch and a null nonResidentBits are refused."""
    import ctypes as C
    from basicrenderer_amd import capi
    from basicrenderer_amd.renderer import BrmiError
    name = "tiny_lod"
    sc = scenes(name)
    r = _renderer(sc)
    r.set_streaming(np.arange(r.group_count()))
    r.execute()
    assert r.counters().visibleClusters == 0
    r.set_streaming(None)
    r.execute()
    _assert_frame(r, oracle_frames(name))
    with pytest.raises(BrmiError):
        r.streaming_feedback()
    assert r.lib.brmi_streaming_feedback(r._h, None) != 0
    r.set_streaming([0])
    st = r._streaming
    b = capi.StreamingBuffers()
    b.structSize = C.sizeof(capi.StreamingBuffers)
    b.activeGroupScanCount = r.group_count()
    b.nonResidentBits, b.loadRequests, b.requestCapacity = st["bits"].data_ptr(), st["requests"].data_ptr(), 16
    b.touchedGroups, b.touchedCapacity, b.counts = st["touched"].data_ptr(), 16, st["counts"].data_ptr()
    b.scratch, b.scratchBytes = st["scratch"].data_ptr(), int(r.lib.brmi_streaming_scratch_bytes(r.group_count())) - 1
    assert r.lib.brmi_set_streaming(r._h, C.byref(b)) == -3 and b"scratch" in r.lib.brmi_last_error(r._h)
    b.scratchBytes += 1
    b.nonResidentBits = None
    assert r.lib.brmi_set_streaming(r._h, C.byref(b)) == -1
    b.nonResidentBits = st["bits"].data_ptr()
    assert r.lib.brmi_set_streaming(r._h, C.byref(b)) == 0
    r.close()
