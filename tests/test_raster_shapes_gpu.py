"""The two register shapes of the opaque direct rasteriser: k_raster<false, false> (the general one) and
k_raster_slim (the slim one: at most 104 VGPRs, launched for frames issued on two streams).  BRMI_TUNING raster_slim=0|1 forces either.
Both must write the same visibility keys bit for bit, and the CPU oracle's."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = (0, 1)


class _Tuning:
    """BRMI_TUNING around the creation of one pass (the library reads it in brmi_create)."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = os.environ.get("BRMI_TUNING")
        os.environ["BRMI_TUNING"] = ",".join(f"{k}={v}" for k, v in self.kv.items())

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("BRMI_TUNING", None)
        else:
            os.environ["BRMI_TUNING"] = self.old


def _pass(sc, slim, tuning=None, **kw):
    from basicrenderer_amd.renderer import VisibilityRenderer
    with _Tuning(raster_slim=slim, **(tuning or {})):
        return VisibilityRenderer(sc, **kw)


@pytest.fixture(scope="module")
def adversarial():
    """tests/raster64.py's scene, 700 x 420 (no multiple of 8 either way): triangles across 8 x 8 tile borders and the right and bottom screen edges, triangles
    the near plane clips, clusters of one triangle, large triangles that leave k_raster as bin records beside small ones of the same cluster, mirrored instances.
    With the oracle's frame."""
    import orc
    import raster64
    sc, _, _ = raster64.adversarial_scene()
    o = orc.OracleFrame(sc); o.cull(); o.raster(); o.depth_copy()
    return sc, o


@pytest.mark.parametrize("tuning", [dict(), dict(big_tri_area=1 << 30), dict(big_tri_area=1), dict(wide_capacity=0, bin_capacity=3, bin_overflow=2)],
                         ids=["default", "nothing binned", "everything binned", "whole-wave emission, bins of three"])
def test_both_shapes_write_the_oracles_keys_on_the_adversarial_scene(tuning, adversarial):
    """Every triangle through the row walk, every triangle through the records, and the default mix of both; without the wide queue the triangles of many
    bins are emitted by the whole wave (the slim shape requests four slots at a time there, the general one eight), and a full bin's record is
    rasterised inside k_raster."""
    sc, o = adversarial
    for slim in SHAPES:
        r = _pass(sc, slim, tuning)
        r.execute()
        assert r.raster_shape() == slim
        vis, depth = r.visibility(), r.depth()
        r.close()
        assert np.array_equal(vis, o.vis), f"raster_slim={slim}: keys differ from the oracle's"
        assert np.array_equal(depth.view(np.uint32), o.depth.view(np.uint32)), f"raster_slim={slim}: depth"


def test_both_shapes_in_a_row_band_and_in_interleaved_stripes(adversarial):
    """bandY0 / bandY1 and the stripe map: a band cut through the scene's stack of triangles, and chunks of 16 rows for two ranks (at a height the
    stripes divide).  What the keys name and the depth bits are the oracle's full frame's on the rank's rows, for both shapes."""
    import orc
    import raster64
    sc, o = adversarial
    want = orc.canonical_ids(o.vis, o.clusters[: o.count])
    for slim in SHAPES:
        for y0, y1 in ((0, raster64.ADVERSARIAL_SPLIT), (raster64.ADVERSARIAL_SPLIT, sc.height)):
            r = _pass(sc, slim, band=(y0, y1))
            r.execute()
            assert r.raster_shape() == slim
            for got, ref in zip(orc.canonical_ids(r.visibility(), r.visible_clusters()), want):
                assert np.array_equal(got[y0:y1], ref[y0:y1]), (slim, y0, y1)
            assert np.array_equal(r.depth().view(np.uint32)[y0:y1], o.depth.view(np.uint32)[y0:y1]), (slim, y0, y1)
            r.close()
    sc2, _, _ = raster64.adversarial_scene(size=(700, 416))
    o2 = orc.OracleFrame(sc2); o2.cull(); o2.raster(); o2.depth_copy()
    want = orc.canonical_ids(o2.vis, o2.clusters[: o2.count])
    for slim in SHAPES:
        for index in range(2):
            r = _pass(sc2, slim, stripes=(16, 2, index))
            r.execute()
            fr = r.frame_rows()
            for got, ref in zip(orc.canonical_ids(r.visibility(), r.visible_clusters()), want):
                assert np.array_equal(got, ref[fr]), (slim, index)
            assert np.array_equal(r.depth().view(np.uint32), o2.depth.view(np.uint32)[fr]), (slim, index)
            r.close()


@pytest.mark.parametrize("case", ["tiny_skinned", "bistro_skinned", "bistro_mirrored"])
def test_both_shapes_on_skinned_and_mirrored_instances(case, scenes, oracle_frames):
    """Compute skinning in the vertex stage (the slim shape requests two bone matrices at a time, the general one as many as fit) and reversed winding.
    The generator's meshlets are grids of 81 vertices and 128 triangles: two passes of 64 triangles per cluster, one full and one partial round of the
    vertex stage.  (The cluster of 128 vertices is the last test's.)"""
    sc, o = scenes(case), oracle_frames(case)
    for slim in SHAPES:
        r = _pass(sc, slim)
        r.execute()
        vis = r.visibility()
        r.close()
        assert np.array_equal(vis, o.vis), f"raster_slim={slim}: keys differ from the oracle's"


def test_split_frames_launch_the_slim_shape_and_one_stream_frames_the_general_one():
    """The selection itself (launch_raster): brmi_execute_split picks the slim shape, brmi_execute and a forced raster_slim=0 the general one, a forced
    raster_slim=1 the slim one on one stream too -- read back with brmi_debug_raster_shape."""
    import torch
    from basicrenderer_amd import Scene
    from basicrenderer_amd.renderer import VisibilityRenderer
    sc = Scene("tiny", 200, 120, point_lights=2)
    geometry, shading = torch.cuda.Stream(priority=-1), torch.cuda.Stream()
    seen = {}
    for name, tuning in (("auto", None), ("forced general", dict(raster_slim=0)), ("forced slim", dict(raster_slim=1))):
        if tuning is None:
            r = VisibilityRenderer(sc, occlusion=True)
        else:
            with _Tuning(**tuning):
                r = VisibilityRenderer(sc, occlusion=True)
        r.execute()
        torch.cuda.synchronize()
        one = r.raster_shape()
        with torch.cuda.stream(geometry):
            r.execute(shading)
        torch.cuda.synchronize()
        seen[name] = (one, r.raster_shape())
        r.close()
    assert seen == {"auto": (0, 1), "forced general": (0, 0), "forced slim": (1, 1)}, seen


def test_split_ring_with_the_slim_shape_renders_the_serial_frames_of_the_general_one():
    """Two-phase occlusion culling over three frames of a moving camera on a ring of two passes with brmi_execute_split: the launcher, not the tuning
    key, picks the slim shape, for phase 1, phase 2 and the late launches alike.  Every frame's keys and depth are those of one pass that renders the
    path serially with the general shape, and the oracle's."""
    import orc
    import torch
    from conftest import Scene
    from basicrenderer_amd.renderer import VisibilityRenderer
    preset, W, H, kw = "bistro", 640, 360, dict(point_lights=8, size_scale=0.3)
    steps = 3
    scs = [Scene(preset, W, H, camera_step=s, **kw) for s in range(steps)]
    serial, oracle, hz = [], [], None
    hold = dict(hold_min_clusters=0)      # the draw list on: phase 1 holds clusters back, re-tests them and draws the late ones (a second launch of k_raster)
    one = _pass(scs[0], 0, hold, occlusion=True)
    phase2 = 0
    for s in range(steps):
        if s:
            one.set_camera_from(scs[s], frame_index=s)
        one.execute()
        torch.cuda.synchronize()
        assert one.raster_shape() == 0
        phase2 += one.counters().visibleClustersPhase2
        serial.append((one.visibility().copy(), one.depth().copy()))
        o = orc.OracleFrame(scs[s])
        hz = o.run_occlusion(hz)
        oracle.append(o.vis.copy())
    one.close()
    assert phase2 > 0, "the path leaves phase 2 nothing to draw"
    with _Tuning(**hold):      # (no raster_slim: the launcher picks)
        passes = [VisibilityRenderer(Scene(preset, W, H, camera_step=0, **kw), occlusion=True) for _ in range(2)]
    passes[0].set_history_source(passes[1]); passes[1].set_history_source(passes[0])
    geometry, shading = torch.cuda.Stream(priority=-1), torch.cuda.Stream()
    torch.cuda.synchronize()
    for s in range(steps):
        r = passes[s % 2]
        with torch.cuda.stream(geometry):
            r.set_camera_from(scs[s], frame_index=s)
            r.execute(shading)
        torch.cuda.synchronize()
        assert r.raster_shape() == 1, f"frame {s}: the split frame did not launch the slim shape"
        vis, depth = r.visibility(), r.depth()
        assert np.array_equal(vis, serial[s][0]), f"frame {s}: keys differ from the serial frame of the general shape"
        assert np.array_equal(depth.view(np.uint32), serial[s][1].view(np.uint32)), f"frame {s}: depth"
        assert np.array_equal(vis, oracle[s]), f"frame {s}: keys differ from the oracle's"
    for r in passes:
        r.close()


def _full_meshlet_scene():
    """A caller's scene of two meshes, each one meshlet: a ring of 64 inner and 64 outer vertices joined by 128 triangles -- BRMI_MESHLET_MAX_VERTS vertices and the most
    triangles a meshlet holds, so the vertex stage runs two full rounds of 64 lanes and every triangle of both passes reads a staged vertex of index 64 or more -- and a
    single triangle.  The ring's triangles are about 14 x 50 px: some walked directly, some binned, across tile borders.  Camera on the z axis as in tests/raster64.py."""
    from basicrenderer_amd import Scene as RawScene
    W, H, eye_z, fov, d = 300, 203, 4.0, 90.0, 2.0
    h = 1.0 / np.tan(np.radians(fov) / 2)
    w = h / (W / H)
    aim = lambda sx, sy: [(sx / (W / 2) - 1.0) * d / w, (1.0 - sy / (H / 2)) * d / h, eye_z - d]

    def front(tri):      # (screen positions) wound so that the rasteriser keeps it: twice the screen area negative, y down
        (ax, ay), (bx, by), (cx, cy) = tri
        return tri if (bx - ax) * (cy - ay) - (by - ay) * (cx - ax) < 0 else [tri[0], tri[2], tri[1]]

    ang = 2.0 * np.pi * (np.arange(64) + 0.37) / 64
    ring = [(150.3 + 45.0 * np.cos(a), 101.7 + 45.0 * np.sin(a)) for a in ang] + [(150.3 + 95.0 * np.cos(a), 101.7 + 95.0 * np.sin(a)) for a in ang]
    idx = []
    for k in range(64):
        i0, i1, o0, o1 = k, (k + 1) % 64, 64 + k, 64 + (k + 1) % 64
        for tri in ((i0, o0, i1), (i1, o0, o1)):
            keep = front([ring[v] for v in tri])
            idx += tri if keep[1] == ring[tri[1]] else (tri[0], tri[2], tri[1])
    one = front([(20.5, 20.5), (20.5, 33.5), (41.5, 20.5)])
    meshes = [dict(positions=np.array([aim(*p) for p in ring], dtype=np.float32), indices=np.array(idx, dtype=np.uint32), material=0),
              dict(positions=np.array([aim(*p) for p in one], dtype=np.float32), indices=np.arange(3, dtype=np.uint32), material=1)]
    eye = np.eye(4, dtype=np.float32)
    return RawScene(width=W, height=H, meshes=meshes, instances=[(0, eye), (1, eye)], view=dict(eye=(0.0, 0.0, eye_z), yaw=0.0, pitch=0.0, fov=fov, near=0.01, far=100.0))


def _meshlet_counts(sc, clusters):
    """(vertices, triangles) of every listed cluster, read from the scene's pages as the rasteriser reads them"""
    import raster64
    out = []
    for c in np.asarray(clusters, dtype=np.uint32).reshape(-1, 4):
        pos, tri = raster64._decode_meshlet(sc.slabs[int((c[2] >> 2) & 0xFFFFF)], int(c[2] >> 22) << raster64.PAGE_SHIFT, int(c[1] & 0x3FFF))
        out.append((len(pos), len(tri)))
    return out


def test_both_shapes_on_a_meshlet_of_128_vertices_and_128_triangles_beside_one_of_one_triangle():
    """The largest cluster the format allows and the smallest, in one frame: the visible list read back holds a cluster of exactly BRMI_MESHLET_MAX_VERTS = 128
    vertices and 128 triangles and one of one triangle, and both shapes write the oracle's keys for them."""
    import orc
    sc = _full_meshlet_scene()
    o = orc.OracleFrame(sc); o.cull(); o.raster(); o.depth_copy()
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    assert int((o.vis != empty).sum()) > 15000, "the ring is not on screen"
    for slim in SHAPES:
        r = _pass(sc, slim)
        r.execute()
        assert r.raster_shape() == slim
        vis, depth, clusters = r.visibility(), r.depth(), r.visible_clusters()
        r.close()
        counts = _meshlet_counts(sc, clusters)
        assert (128, 128) in counts and (3, 1) in counts, counts
        # every triangle of the full meshlet owns pixels: both 64-triangle passes drew, from vertices of both rounds of the vertex stage
        full = counts.index((128, 128))
        keys = vis[vis != empty]
        owners = np.unique(keys[((keys >> np.uint64(7)) & np.uint64(0x3FFFFFF)) == np.uint64(full)] & np.uint64(0x7F))
        assert len(owners) == 128, f"raster_slim={slim}: {len(owners)} of the full meshlet's 128 triangles own a pixel"
        assert np.array_equal(vis, o.vis), f"raster_slim={slim}: keys differ from the oracle's"
        assert np.array_equal(depth.view(np.uint32), o.depth.view(np.uint32)), f"raster_slim={slim}: depth"
