"""The draw list's prediction runs in the cluster cull (brmi_cull.hip: k_cull_clusters_hold) and reaches the scatter in the TempVisible record.

Small frames, the draw list forced on (hold_min_clusters=0, as test_parity_gpu forces it), a ring of two passes linked by set_history_source, four frames: two of
the scene's own camera, then two of the camera path.  Every frame is held against the CPU oracle (visible list, keys, depth, depth chain: bit-exact).  On every
frame the held list (brmi_debug_read_held) and the draw list (brmi_debug_read_draw_list) partition the placed phase-1 clusters: no index twice, none on both, together
every index below the placed count and nothing else; no held cluster belongs to a skinned mesh; every held record names a box of the table (a cluster of a page
without boxes has none: its record would carry 0xFFFFFFFF and the re-test would read beyond the table); clusters are held from the second frame on, late ones are
among the held.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OCCLUDERS = dict(unique_budget=True, lod_builder="own", relief_slope=1.5)
SCENES = {
    "small": ("bistro", 256, 144, OCCLUDERS),
    "mid": ("bistro", 640, 360, OCCLUDERS),
    "skinned": ("bistro", 256, 144, dict(skinned_fraction=0.3, **OCCLUDERS)),
    "alpha": ("san_miguel", 256, 144, dict(material_features=24)),
}
FRAMES = 4
VERTEX_SKINNED = 1 << 3


@pytest.fixture(scope="module")
def oracle_frames():
    """Per scene: (Scene, cameras of frames 3-4, per frame the oracle's clusters / phase-1 count / keys / depth / chain) -- computed once, shared, never written to."""
    from conftest import Scene
    from test_parity_gpu import _OracleRun
    cache = {}

    def get(name):
        if name not in cache:
            preset, W, H, kw = SCENES[name]
            sc = Scene(preset, W, H, point_lights=4, **kw)
            cams = [sc.camera_at(0.1 * (j + 1), 0.1 * j) for j in range(2)]
            own = (sc.arrays["cameras"].copy(), sc.arrays["cullingCameras"].copy())
            run, frames = _OracleRun(sc), []
            for f in range(FRAMES):
                o = run.frame(None if f < 2 else cams[f - 2], shade=False)
                data, offs, n = o.hzb
                frames.append(dict(clusters=o.clusters[: o.count].copy(), count1=o.count1, vis=o.vis.copy(), depth=o.depth.copy(), hzb=(data.copy(), np.array(offs).copy(), n), W=o.W, H=o.H))
            sc.arrays["cameras"][:] = own[0]; sc.arrays["cullingCameras"][:] = own[1]
            cache[name] = (sc, cams, frames)
        return cache[name]

    return get


def _skinned_cluster(sc, clusters):
    inst = sc.arrays["perMeshInstance"].view(np.uint32).reshape(-1, 8)
    mesh = sc.arrays["perMesh"].view(np.uint32).reshape(-1, 16)
    return (mesh[inst[(clusters[:, 0] >> 8).astype(np.int64), 0].astype(np.int64), 2] & VERTEX_SKINNED) != 0


def _run(sc, cams, frames, what, exact=True, **renderer_kw):
    """The four frames on the ring; returns (held, late, draw) index arrays per frame."""
    import torch
    from basicrenderer_amd.renderer import VisibilityRenderer
    from test_parity_gpu import _Env
    with _Env(hold_min_clusters=0):
        passes = [VisibilityRenderer(sc, occlusion=True, stats=True, **renderer_kw) for _ in range(2)]
    passes[0].set_history_source(passes[1]); passes[1].set_history_source(passes[0])
    dev = torch.device("cuda:0")
    lists = []
    for f, ref in enumerate(frames):
        p = passes[f % 2]
        if f < 2:
            p.update()
        else:
            cam, cull = cams[f - 2]
            p.set_camera_device(torch.from_numpy(cam).to(dev), torch.from_numpy(cull).to(dev), cam)
        p.execute()
        torch.cuda.synchronize()
        c = p.counters()
        held, late = p.held_clusters()
        lists.append((held.copy(), late.copy()))
        print(f"[prediction] {what} frame {f}: phase-1 clusters {c.visibleClusters}, held {len(held)}, late {len(late)}")
        assert (c.reserved[1], c.reserved[3]) == (len(held), len(late)), f"{what} frame {f}"
        placed1 = min(int(c.visibleClusters), int(p.cfg.maxVisibleClusters))
        assert len(np.unique(held)) == len(held) and (held < placed1).all(), f"{what} frame {f}: a held index twice, or outside the {placed1} placed clusters"
        draw, held_boxes, box_count = p.draw_list()
        lists[-1] += (draw.copy(),)
        if f == 0:
            assert len(draw) == 0 and len(held) == 0, "no previous chain: nothing to predict from, every cluster is drawn in list order"
        else:
            assert len(np.intersect1d(draw, held)) == 0, f"{what} frame {f}: a cluster on both lists"
            both = np.sort(np.concatenate([draw, held]))
            assert np.array_equal(both, np.arange(placed1, dtype=np.uint32)), f"{what} frame {f}: draw list ({len(draw)}) and held list ({len(held)}) are not the {placed1} placed clusters"
            assert len(held_boxes) == len(held) and (held_boxes < box_count).all(), f"{what} frame {f}: a held record without a box of the table ({box_count} boxes)"
        assert np.isin(late, held).all(), f"{what} frame {f}: a late cluster that was not held"
        if exact:
            got = p.visible_clusters()
            assert np.array_equal(got, ref["clusters"]), f"{what} frame {f}: visible-cluster list"
            assert not _skinned_cluster(sc, got[held]).any(), f"{what} frame {f}: a cluster of a skinned mesh was held"
            assert np.array_equal(p.visibility(), ref["vis"]), f"{what} frame {f}: visibility keys"
            assert np.array_equal(p.depth().view(np.uint32), ref["depth"].view(np.uint32)), f"{what} frame {f}: depth"
            data, offs, n = ref["hzb"]
            pw, ph = 1 << (ref["W"] - 1).bit_length(), 1 << (ref["H"] - 1).bit_length()
            mips = p.hzb_mips()
            assert len(mips) == n - 1
            for mip in range(1, n):
                w, h = max(1, pw >> mip), max(1, ph >> mip)
                assert np.array_equal(mips[mip - 1].view(np.uint32), data[int(offs[mip]): int(offs[mip]) + w * h].reshape(h, w).view(np.uint32)), f"{what} frame {f}: chain mip {mip}"
    for p in passes:
        p.close()
    return lists


@pytest.mark.parametrize("name", list(SCENES))
def test_frames_are_the_oracles_and_clusters_are_held(name, oracle_frames):
    sc, cams, frames = oracle_frames(name)
    lists = _run(sc, cams, frames, name)
    if name != "alpha":      # (the occluder scenes: the case must not pass with the draw list silently off)
        for f in range(1, FRAMES):
            assert len(lists[f][0]) > 0, f"{name} frame {f}: nothing held"


def test_ragged_last_wave(oracle_frames):
    """maxVisibleClusters just above the list: the phase-1 count is no multiple of 64, so the scatter's last wave is ragged."""
    sc, cams, frames = oracle_frames("small")
    assert all(fr["count1"] % 64 != 0 for fr in frames[1:]), [fr["count1"] for fr in frames]
    lists = _run(sc, cams, frames, "ragged", max_clusters=max(len(fr["clusters"]) for fr in frames) + 37, maxTraversalRecords=1 << 16)
    assert all(len(l[0]) > 0 for l in lists[1:])


def test_capacity_below_the_visible_count(oracle_frames):
    """maxVisibleClusters below the phase-1 count: a cluster that found no place is on neither list -- _run holds the two lists to exactly the indices below the
    capacity -- and the frames do overflow (the oracle's phase-1 count is above the capacity)."""
    sc, cams, frames = oracle_frames("small")
    cap = min(fr["count1"] for fr in frames) * 3 // 4
    lists = _run(sc, cams, frames, "capacity", exact=False, max_clusters=cap, maxTraversalRecords=1 << 16)
    assert all(fr["count1"] > cap for fr in frames)
    for held, _, draw in lists[1:]:
        assert (held < cap).all() and (draw < cap).all() and len(held) + len(draw) == cap
