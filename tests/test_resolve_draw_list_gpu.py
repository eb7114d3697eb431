"""The resolve tables follow the draw list (brmi_resolve.hip: k_resolve_setup_listed).

On a frame that holds clusters back the setup builds tables for the draw list, the late list and the phase-2 clusters only; a held cluster that is never
released keeps whatever its place in the arena held.  Every frame here is held against the CPU oracle (tests/orc.py), never against the code under test:
visible-cluster list, keys, depth and the seven G-buffer planes exact, HDR within one fp16 ULP (test_parity_gpu's rule and helper).

Small frames where this can still go wrong: the `bistro` preset with the library's own LOD builder at 256 x 144 and 640 x 360, occlusion culling on, a ring of
two passes linked by set_history_source, the draw list forced onto them (hold_min_clusters=0); one scene with skinned instances (never held: they are on the
draw list) and one with material features 24 (texcoord tables, alpha test).  One sequence per scene and arrangement: five frames of the still camera, then
four of the camera path on the same ring.  Frames this small have more than a quarter of a cluster triangle per pixel and would resolve without any table
(resolve_inline_frame), so the setup would never be launched: resolve_inline=0 keeps the tables, as the 4K frames the draw list is meant for have them.

Not checked: that stale arena entries are never read, by filling the arena with a NaN pattern between two frames.  The arena is not a resource of its own
(brmi_declare): it is a range of the workspace at an offset only the library knows.  What the moving frames check instead: a released cluster's entries were
last written, if ever, under another frame's camera.
"""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCENES = {
    "small": (256, 144, dict()),
    "mid": (640, 360, dict()),
    "skinned": (256, 144, dict(skinned_fraction=0.3)),
    "textured": (256, 144, dict(material_features=24)),
}
STILL_FRAMES, MOVING_FRAMES = 5, 4


def _scene(name):
    from conftest import Scene
    W, H, kw = SCENES[name]
    return Scene("bistro", W, H, point_lights=8, lod_builder="own", **kw)


def _cameras(sc):
    """Frame j of the moving part sees the path's position 0.1 (j + 1); its culling camera is the frame before's."""
    return [sc.camera_at(0.1 * (j + 1), 0.1 * j) for j in range(MOVING_FRAMES)]


def _snapshot(o):
    """What _assert_frame_is_the_oracles reads of an OracleFrame (which reuses its cluster buffer frame after frame; the images are new arrays per frame)."""
    return types.SimpleNamespace(W=o.W, H=o.H, count=o.count, count1=o.count1, count2=o.count2, clusters=o.clusters[: o.count].copy(), vis=o.vis, depth=o.depth,
                                 normals=o.normals, albedo=o.albedo, mr=o.mr, motion=o.motion, coat=o.coat, emissive=o.emissive, fuzz=o.fuzz, hdr=o.hdr)


@pytest.fixture(scope="module")
def oracle_sequences():
    """Per scene: (the Scene, the oracle's last still frame, its four moving frames) -- computed once, shared by every arrangement, never written to."""
    from test_parity_gpu import _OracleRun
    cache = {}

    def get(name):
        if name not in cache:
            sc = _scene(name)
            cams = _cameras(sc)
            still_cam = (sc.arrays["cameras"].copy(), sc.arrays["cullingCameras"].copy())
            run = _OracleRun(sc)
            for _ in range(STILL_FRAMES - 1):
                run.frame(shade=False)
            still = _snapshot(run.frame())
            moving = [_snapshot(run.frame(cam)) for cam in cams]
            sc.arrays["cameras"][:] = still_cam[0]; sc.arrays["cullingCameras"][:] = still_cam[1]      # (the renderers are created from the scene's own camera)
            cache[name] = (sc, still, moving, cams)
        return cache[name]

    return get


def _render(sc, cams, split=True, **tuning):
    """The sequence on a ring of two passes (frame k on pass k % 2).  split: the bench's arrangement, one geometry stream and a shading stream per pass
    (brmi_execute_split: the phase-1 setup beside the rasteriser, the late list and phase 2 at the end of the geometry half); else brmi_execute, whose one setup
    launch finds every list final.  Returns (captures of the last still frame and of every moving frame, (held, late) counts per frame, the late list per frame)."""
    import torch
    from basicrenderer_amd.renderer import VisibilityRenderer
    from test_parity_gpu import _Env, _capture
    with _Env(resolve_inline=0, **tuning):
        passes = [VisibilityRenderer(sc, occlusion=True, band=(0, sc.height)) for _ in range(2)]
    passes[0].set_history_source(passes[1]); passes[1].set_history_source(passes[0])
    geometry, shading = torch.cuda.Stream(priority=-1), [torch.cuda.Stream() for _ in passes]
    dev = torch.device("cuda:0")
    cam_dev = [(torch.from_numpy(c).to(dev), torch.from_numpy(cc).to(dev)) for c, cc in cams]
    torch.cuda.synchronize()
    captures, counts, lists = [], [], []
    for f in range(STILL_FRAMES + len(cams)):
        k = f % 2
        p = passes[k]
        with torch.cuda.stream(geometry):
            if f < STILL_FRAMES:
                p.update()
            else:
                j = f - STILL_FRAMES
                p.set_camera_device(cam_dev[j][0], cam_dev[j][1], cams[j][0])
            p.execute(shading[k] if split else None)
        if f >= STILL_FRAMES - 1:
            with torch.cuda.stream(shading[k] if split else geometry):
                captures.append(_capture(p))
        held, late = p.held_clusters()      # (waits for the device: the counts of this frame have reached the host before the next one chooses its launches)
        counts.append((len(held), len(late))); lists.append(late)
    for p in passes:
        p.close()
    return captures, counts, lists


def _check_sequence(name, oracle_sequences, what, **kw):
    from test_parity_gpu import _assert_frame_is_the_oracles
    sc, still, moving, cams = oracle_sequences(name)
    captures, counts, lists = _render(sc, cams, **kw)
    # pixels of the oracle's frame whose key names a cluster of the late list (key: depth | cluster index << 7 | triangle): tables the first setup launch did not make
    late_px = [int(np.isin((o.vis[o.vis != np.uint64(0xFFFFFFFFFFFFFFFF)] >> np.uint64(7)) & np.uint64(0x3FFFFFF), lists[STILL_FRAMES + j]).sum()) for j, o in enumerate(moving)]
    print(f"[draw list] {name} {what}: (held, late) per frame {counts}, pixels of late clusters per moving frame {late_px}")
    held, late = counts[STILL_FRAMES - 1]
    assert held > 0 and late == 0, f"{name} {what}: last still frame held {held} clusters, {late} late: nothing was skipped, or the prediction is not exact with a still camera"
    _assert_frame_is_the_oracles(captures[0], still, f"{name} {what}: still frame {STILL_FRAMES - 1}")
    assert any(l > 0 for _, l in counts[STILL_FRAMES:]), f"{name} {what}: no moving frame released a held cluster {counts[STILL_FRAMES:]}"
    assert sum(late_px) > 0, f"{name} {what}: no late cluster owns a pixel: the moving frames would pass without the late list's tables"
    for j, o in enumerate(moving):      # (a released cluster that reached the pixel pass without tables fails here)
        _assert_frame_is_the_oracles(captures[1 + j], o, f"{name} {what}: moving frame {j}, (held, late) = {counts[STILL_FRAMES + j]}")
    return captures


@pytest.mark.parametrize("name", list(SCENES))
def test_late_list_walked_directly(name, oracle_sequences):
    """Still camera: clusters are held, none is late, the last frame is the oracle's.  Camera path: some frame draws late clusters (their tables come from the
    second setup launch), every frame is the oracle's.  The late pass walks its list directly (late_direct_max at its default)."""
    _check_sequence(name, oracle_sequences, "direct", hold_min_clusters=0)


@pytest.mark.parametrize("name", list(SCENES))
def test_late_list_through_the_bins(name, oracle_sequences):
    """The same with the late pass through records, plan and bins (late_direct_max=0)."""
    _check_sequence(name, oracle_sequences, "bins", hold_min_clusters=0, late_direct_max=0)


@pytest.mark.parametrize("late_direct", [None, 0])
def test_one_stream_sets_up_behind_the_rasteriser(late_direct, oracle_sequences):
    """brmi_execute on one stream: the setup runs once, in front of the pixel pass, with the draw, late and phase-2 lists all final."""
    tuning = dict(hold_min_clusters=0) if late_direct is None else dict(hold_min_clusters=0, late_direct_max=late_direct)
    _check_sequence("small", oracle_sequences, f"one stream, late_direct_max={late_direct}", split=False, **tuning)


def test_draw_list_off_is_the_same_frame(oracle_sequences):
    """hold_min_clusters=1000000, hold_still_max=0: no frame makes a draw list and the setup is the launch it always was.  Nothing is held; the frames are the
    oracle's, and every plane of every captured frame has the bytes of the run with the draw list on."""
    from test_parity_gpu import _assert_frame_is_the_oracles
    sc, still, moving, cams = oracle_sequences("small")
    off, counts, _ = _render(sc, cams, hold_min_clusters=1000000, hold_still_max=0)
    assert all(c == (0, 0) for c in counts), counts
    _assert_frame_is_the_oracles(off[0], still, "draw list off: still frame")
    for j, o in enumerate(moving):
        _assert_frame_is_the_oracles(off[1 + j], o, f"draw list off: moving frame {j}")
    on, _, _ = _render(sc, cams, hold_min_clusters=0)
    for f, (a, b) in enumerate(zip(on, off)):
        covered = a["VISIBILITY"].cpu().numpy().view(np.uint64) != np.uint64(0xFFFFFFFFFFFFFFFF)
        for k in a:
            x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
            if k == "VISIBLE_CLUSTERS":
                n = (still if f == 0 else moving[f - 1]).count * 16
                x, y = x[:n], y[:n]
            elif k not in ("VISIBILITY", "LINEAR_DEPTH"):      # (byte planes in tile order, like the keys: compared where a key was drawn)
                per = x.size // covered.size
                x, y = x.reshape(covered.size, per)[covered], y.reshape(covered.size, per)[covered]
            assert np.array_equal(x, y), f"captured frame {f}: {k} differs between the draw list on and off"
