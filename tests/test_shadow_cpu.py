"""Shadow maps of spot and point lights, the part that needs no GPU: the ABI, and whether the inputs of tests/test_shadow_gpu.py are fit to judge with --
decided by the float64 restatement (tests/shadow_ref.py) alone, before any kernel is looked at."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import shadow_cases as cases
import shadow_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAGILE_CAP = 0.02


def test_abi_exports_shadow_entry_points():
    """libbrmi.so exports the three entry points, the header declares them with the struct and the format, and brmi_light_info is still 128 B."""
    from basicrenderer_amd import capi, shadows
    lib = capi.brmi_lib()
    header = open(os.path.join(ROOT, "include", "brmi.h")).read()
    for name in ("brmi_set_shadows", "brmi_shadow_capture", "brmi_debug_shadow"):
        assert hasattr(lib, name), f"libbrmi.so does not export {name}"
        assert name in capi.BRMI_EXPORTS and name + "(" in header
    types = open(os.path.join(ROOT, "include", "brmi_types.h")).read()
    assert re.search(r"#define BRMI_TEXTURE_FORMAT_R32_FLOAT\s+3u", types) and capi.TEXTURE_FORMAT_R32_FLOAT == 3
    assert re.search(r"\}\s*brmi_light_info;\s*/\* 128 B \*/", types) and shadows.LIGHT_DTYPE.itemsize == 128
    assert C.sizeof(capi.ShadowBuffers) == 56 and "} brmi_shadow_buffers;" in header
    # the scene generator's record is the same 128 bytes: the light array divides into whole records
    assert cases.scene().arrays["lights"].size % 128 == 0 and cases.scene().arrays["lights"].size // 128 == cases.scene().counts["lights"]


def test_margin_is_measured_and_small():
    measured, margin = cases.margin()
    print(f"measured fp32 - float64 difference {measured:.3e}, margin {margin:.3e}")
    assert 0.0 < measured and margin == 4.0 * measured
    assert margin < 1e-2      # the offsets of the receivers are spread over +-0.6 x the plane's depth: a margin near that would judge nothing


@pytest.mark.parametrize("kind", cases.MAP_KINDS)
@pytest.mark.parametrize("size", cases.SPOT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_spot_inputs_fragile_share(kind, size):
    _, margin = cases.margin()
    r = cases.spot_results(kind, size, np.float64)
    fragile = ref.spot_fragile(r, margin)
    share, shadowed = fragile.mean(), r["shadow"][~fragile].mean()
    print(f"spot {kind} {size}: fragile {share:.4f}, shadowed {shadowed:.3f}")
    assert share <= FRAGILE_CAP
    assert 0.05 <= shadowed <= 0.95      # both answers are exercised
    # receivers that project outside the map and receivers behind the light are among them
    assert (r["w"] < 0).sum() >= 32


@pytest.mark.parametrize("kind", cases.MAP_KINDS)
def test_point_inputs_fragile_share(kind):
    _, margin = cases.margin()
    r = cases.point_results(kind, np.float64)
    fragile = ref.point_fragile(r, margin)
    share, shadowed = fragile.mean(), r["shadow"][~fragile].mean()
    print(f"point {kind}: fragile {share:.4f}, shadowed {shadowed:.3f}")
    assert share <= FRAGILE_CAP
    assert 0.05 <= shadowed <= 0.95
    assert (r["gap"] < margin).sum() >= 8 and len(np.unique(r["face"])) == 6      # receivers on face edges (up to the rounding of their fp32 positions); every face
    if kind == "border":
        assert r["early"].sum() >= 16      # the `== 1.0` early-out is taken


@pytest.mark.parametrize("clustered", [1, 0], ids=["clustered", "unclustered"])
@pytest.mark.parametrize("name", ["tiny", "sponza"])
def test_frame_cases_are_fit_to_judge_with(name, clustered):
    """The frame cases of tests/test_shadow_gpu.py, from the oracle-rendered light views and the restatement alone: at most 2 % of the covered pixels are fragile,
    and of the pixels each shadowed light reaches at least 5 % are shadowed and at least 5 % are lit."""
    import shadow_frames as frames
    measured, margin = frames.frame_margin()
    spot_sh, point_sh, fragile, reach_s, reach_p = frames.judged(name, clustered, margin)
    print(f"{name} clustered={clustered}: margin {margin:.3e} (measured {measured:.3e}), fragile {fragile.mean():.4f} of {len(fragile)} pixels")
    assert fragile.mean() <= FRAGILE_CAP
    for what, shadowed, reach in (("spot", spot_sh, reach_s), ("point", point_sh, reach_p)):
        ok = reach & ~fragile
        share = shadowed[ok].mean()
        print(f"  {what}: reaches {int(reach.sum())} pixels, {share:.3f} of them shadowed")
        assert reach.sum() >= 500
        assert 0.05 <= share <= 0.95
    # the maps hold geometry and background both
    maps, _ = frames.oracle_maps(name)
    assert len(maps) == 7 and maps[0].shape == (frames.SPOT_RES, frames.SPOT_RES) and maps[1].shape == (frames.FACE_RES, frames.FACE_RES)
    assert any((m < 1).any() for m in maps)


def test_capture_round_trip():
    """unprojectDepth(capture(z)) gives z back within the fp32 bound of the two expressions, and the background maps to 1.0.
    capture rounds d = f (z - n) / (z (f - n)) to fp32: relative error <= 3 ulp = 3 * 2^-24 of d (three roundings).  unprojectDepth divides n f by
    f - d (f - n) = n f / z: an error e of d moves the result by z^2 (f - n) / (n f) * e <= (z^2 / n) * e, so |z' - z| <= (z^2 / n) * 3 * 2^-24 (+ its own roundings)."""
    near, far = 0.01, 24.0
    z = np.geomspace(0.02, 23.0, 4096).astype(np.float32)
    d = ref.capture_depth(z, near, far)
    assert d.dtype == np.float32 and np.all((d > 0) & (d < 1))
    back = ref.unproject_depth(d.astype(np.float64), near, far)
    bound = (z.astype(np.float64) ** 2 / near) * 3 * 2.0 ** -24 + 4 * np.spacing(z).astype(np.float64)
    assert np.all(np.abs(back - z) <= bound)
    empty = np.array([ref.EMPTY_DEPTH_BITS], dtype=np.uint32).view(np.float32)
    assert ref.capture_depth(empty, near, far)[0] == np.float32(1.0)
    assert ref.unproject_depth(1.0, near, far) == pytest.approx(far, rel=1e-12)
