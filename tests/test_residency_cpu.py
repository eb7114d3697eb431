"""Residency-aware cut, CPU side: the numpy restatement of tests/clod_residency.py is anchored to the existing oracle before any GPU is involved."""
import numpy as np
import pytest

import clod_residency as cr
from conftest import SCENE_CASES, Scene

CASES = ["tiny_lod", "tiny_ownlod", "sponza_ownlod"]
SETS = ["none", "all", "finest", "third", "third_half_scan"]


def residency_set(scene, which):
    """(non-resident group indices, activeGroupScanCount or None) of the sets the GPU tests use."""
    groups = cr.SceneTables(scene).group_count
    third = np.sort(np.random.default_rng(5).choice(groups, size=max(1, groups // 3), replace=False))
    return {"none": (np.zeros(0, dtype=np.int64), None), "all": (np.arange(groups), None), "finest": (cr.finest_depth_groups(scene), None),
            "third": (third, None), "third_half_scan": (third, groups // 2)}[which]


def make_scene(name):
    preset, W, H, kw = SCENE_CASES[name]
    return lambda: Scene(preset, W, H, **kw)


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("name", CASES)
def test_restatement_counters_equal_the_oracle_on_the_transformed_scene(name, which, scenes):
    import orc
    sc = scenes(name)
    n, active = residency_set(sc, which)
    r = cr.restate(sc, n, active)
    o = orc.OracleFrame(cr.transformed_scene(make_scene(name), n, active))
    o.cull()
    for field in ("instancesVisible", "nodesVisited", "bucketRecords", "meshletsTested"):
        assert r["counters"][field] == getattr(o.counters, field), field
    # the reduction holds what the raw stream holds: the same groups, each once, the best priority of each
    assert set(r["requests"][:, 0].tolist()) == set(r["requests_raw"][:, 0].tolist())
    assert np.array_equal(r["touched"], np.unique(r["touched_raw"]))
    mask = cr.effective_mask(cr.SceneTables(sc).group_count, n, active)
    assert not mask[r["touched"]][~np.isin(r["touched"], r["requests"][:, 0])].any() or active is not None
    if len(r["requests"]) > 1:
        prio = (r["requests"][:, 3] >> 16).astype(np.int64)
        assert (np.diff(prio) <= 0).all() and (np.diff(r["requests"][:, 0].astype(np.int64))[np.diff(prio) == 0] > 0).all()
    if which == "none":
        assert len(r["requests"]) == 0 and len(r["touched"]) > 0
    if which == "third_half_scan":
        assert (r["requests"][:, 0] < active).all()


def test_pack_view_priority_edge_values():
    f = np.float32
    cases = [(f(0.0), 0), (f(1.0 / 2048.0), 1), (np.nextafter(f(1.0 / 2048.0), f(1.0)), 1),
             # one binary32 step below 1 / 2048: x * 1024 + 0.5 = 1 - 2^-25 is a tie between 1 - 2^-24 and 1.0 and rounds to even, 1.0: the shader's float sum gives 1
             (np.nextafter(f(1.0 / 2048.0), f(0.0)), 1), (f(0.499) / f(1024.0), 0),
             (np.nextafter(f(64.0), f(0.0)), 65535), (f(np.inf), 65535), (f(np.nan), 0), (f(-3.0), 0), (f(1.0), 1024)]
    for eod, want in cases:
        packed = cr.pack_view_priority(7, eod)
        assert packed >> 16 == want and packed & 0xFFFF == 7, (eod, packed)


def test_abi_exports_the_streaming_entry_points():
    import os
    import re
    from basicrenderer_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "brmi.h")).read()
    for name in ("brmi_streaming_scratch_bytes", "brmi_set_streaming", "brmi_streaming_feedback"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.BRMI_EXPORTS
    assert "brmi_streaming_request" in open(os.path.join(root, "include", "brmi_types.h")).read()
    assert re.search(r"#define BRMI_ABI_VERSION 1u", header)
    import ctypes
    assert ctypes.sizeof(capi.StreamingBuffers) == 72
    lib_path = os.path.join(root, "basicrenderer_amd", "lib", "libbrmi.so")
    if os.path.exists(lib_path):      # (built by __graft_entry__.build(); loading it needs no GPU)
        lib = ctypes.CDLL(lib_path)
        for name in ("brmi_streaming_scratch_bytes", "brmi_set_streaming", "brmi_streaming_feedback"):
            getattr(lib, name)
        lib.brmi_streaming_scratch_bytes.restype = ctypes.c_uint64
        assert lib.brmi_streaming_scratch_bytes(ctypes.c_uint32(1000)) >= 1000 // 8 + 1000 * 8
