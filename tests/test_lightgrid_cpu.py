"""The oracle's clustered lighting (orc_light_cluster, orc_shade) held to tests/lightgrid_ref.py, the restatement written from the shader text alone.

Boxes, numLights, ptrFirstPage, every page word the shader stores and the pages-used count bit for bit (the oracle is built with -ffp-contract=off); the
host's slice planes within the bound derived in lightgrid_ref; the lit image by the indicator method of lightgrid_cases.  Every case asserts its own premise.
tests/test_lightgrid_gpu.py runs the same cases on the kernels.
"""
import numpy as np
import pytest

import lightgrid_cases as lc
import lightgrid_ref as ref

f32 = np.float32
GRIDS = [((12, 12, 24), 4, 6.0), ((1, 1, 1), 0, 6.0), ((5, 7, 3), 1, 6.0), ((16, 9, 62), 4, 6.0), ((3, 2, 4), 1, 6.0), ((3, 2, 4), 3, 6.0), ((3, 2, 4), 3, 2.5), ((12, 12, 24), 4, 11.0)]
COUNTS = [0, 1, 11, 12, 13, 63, 64, 65, 128, 129]


class OracleBackend:
    """geometry once per rig; lists and image for the rig's current lights, with a page pool of `pool` (set it before lists / render)"""

    def __init__(self, rig):
        import orc
        self.rig, self.pool = rig, 1
        self.o = o = orc.OracleFrame(rig.scene)
        o.cull(); o.raster(); o.depth_copy(); o.gbuffer()
        o.emissive[:] = 0
        self.depth = o.depth

    def planes(self):
        return self.o.cluster_planes()

    def set_roughness(self, mode, target):
        """every pixel's roughness code ROUGH_CODE ("rough"), but the target's SMOOTH_CODE ("exact"); asserts the premise on the G-buffer it leaves"""
        o = self.o
        o.mr[:] = (o.mr & np.uint32(0xFFFF00FF)) | np.uint32(lc.ROUGH_CODE << 8)
        if mode == "exact":
            o.mr[target] = (o.mr[target] & np.uint32(0xFFFF00FF)) | np.uint32(lc.SMOOTH_CODE << 8)
        lc.roughness_premise(o.mr, o.coat, lc.covered_of(self.depth), mode, target)

    def lists(self):
        self.o.light_cluster(pool=self.pool)
        return self.o.light_clusters, self.o.light_pages, self.o.pages_used

    def render(self, records, clustered):
        L = self.rig.scene.arrays["lights"].view(np.uint32).reshape(-1, 32)
        keep = L.copy()
        L[:len(records)] = records
        self.o.light_cluster(pool=self.pool)
        hdr = self.o.shade(clustered=clustered).copy()
        L[:] = keep
        return hdr


@pytest.fixture(scope="module")
def flat():
    rig = lc.Rig("tiny", material_features=3)
    return rig, OracleBackend(rig)


@pytest.fixture(scope="module")
def deep():
    rig = lc.Rig("sponza", size_scale=0.15)
    return rig, OracleBackend(rig)


@pytest.fixture(scope="module")
def plain():
    """a scene of plain materials only (the shading pass's MODE 0 pixels, the ones whose tiles choose between the two instantiations of the light loop)"""
    rig = lc.Rig("tiny")
    return rig, OracleBackend(rig)


@pytest.mark.parametrize("gz", [1, 3, 4, 24, 61, 62])
@pytest.mark.parametrize("near,z_split", [(0, 6.0), (1, 2.5), (4, 6.0), (3, 11.0)])
def test_host_slice_planes_within_the_derived_bound(flat, gz, near, z_split):
    rig, be = flat
    fr = rig.apply([], grid=(2, 2, gz), near=near, z_split=z_split)
    worst, bound = lc.planes_within_bound(fr, be.planes())
    assert worst <= bound, (worst, bound)
    assert bound < 4e-5


@pytest.mark.parametrize("grid,near,z_split", GRIDS)
def test_lists_against_the_restatement(flat, grid, near, z_split):
    """random light sets of every type at the ballot-word edges; the largest grids with two counts only (the allocator is a Python loop)"""
    rig, be = flat
    counts = COUNTS if grid[0] * grid[1] * grid[2] <= 3456 else [13, 65]
    for count in counts:
        lights = lc.random_lights(rig, count, seed=count)
        fr = rig.apply(lights, grid=grid, near=near, z_split=z_split)
        be.pool = fr.total * 12
        hit, al = lc.check_lists(fr, be.planes(), be.pool, *be.lists(), what=(grid, count))
        assert al["counter"] <= be.pool
        if count >= 11 and fr.total > 1:
            assert hit.any() and not hit.all()
        lo64, hi64 = ref.boxes(fr, be.planes(), np.float64)
        lo, hi = ref.boxes(fr, be.planes())
        assert np.allclose(lo, lo64, rtol=1e-4, atol=1e-4) and np.allclose(hi, hi64, rtol=1e-4, atol=1e-4)      # (information: the fp32 boxes are the float64 ones)


def permuted_case(rig, be):
    """23 of 40 lights near the surface (point and spot, the sphere no wider than the range: membership varies) through a non-monotone permutation"""
    lights = lc.surface_lights(rig, be.depth, 40, seed=77, sphere=2.5, spots=True)
    perm = np.random.default_rng(3).permutation(23)
    assert (np.diff(perm) < 0).any() and (perm != np.arange(23)).any()
    return lights, perm


def test_active_list_shorter_than_the_buffer_and_not_the_identity(flat):
    rig, be = flat
    rig.apply([])
    lights, perm = permuted_case(rig, be)
    for active, num in ((None, 7), (perm, 23)):
        fr = rig.apply(lights, active=active, num=num)
        assert fr.num_lights < len(lights)
        be.pool = fr.total * 4
        lc.check_lists(fr, be.planes(), be.pool, *be.lists(), what=("active", num))
    sub = lights[:23]
    fr = rig.apply(sub, active=perm, num=23)
    hit, al = lc.check_lists(fr, be.planes(), be.pool, *be.lists(), what="perm")
    lc.indicator_check(rig, fr, be.depth, al, sub, be.render, what="perm")


# hits per cluster, a missing light behind them, the list positions whose indicator frame is rendered (None: all)
PAGE_EDGES = {"12_last": (12, False, None), "12_more": (12, True, None), "24_last": (24, False, None), "24_more": (24, True, (0, 11, 12, 23)), "13": (13, False, None),
              "25_more": (25, True, (0, 11, 12, 23, 24)), "65": (65, False, (0, 11, 12, 23, 24, 47, 48, 59, 60, 63, 64)), "129_more": (129, True, (0, 63, 64, 65, 107, 108, 127, 128))}


def page_edge_case(rig, be, case, near):
    """Every cluster hits every light (bounding spheres of radius 1000), each light's range keeps it to a part of the frame.  With a missing light behind a full
    page the newest page is empty and the walk shades nothing.  25 hits are three pages, 65 and 129 cross the 64-light ballot words."""
    n, more, only = PAGE_EDGES[case]
    rig.apply([], grid=(3, 2, 4), near=near)
    lights = lc.surface_lights(rig, be.depth, n, seed=n) + ([lc.far_miss(rig)] if more else [])
    fr = rig.apply(lights, grid=(3, 2, 4), near=near)
    be.pool = 400
    hit, al = lc.check_lists(fr, be.planes(), be.pool, *be.lists(), what=case)
    assert (hit.sum(axis=1) == n).all() and (al["numLights"] == n).all()                       # premise: exactly n hits everywhere
    assert bool(hit[:, -1].all()) != more                                                       # ... and the last hit is / is not the last light
    walks = [ref.walk(fr, al["numLights"][c], al["first"][c], al["pages"])[1] for c in range(fr.total)]
    empty_newest = more and n % 12 == 0
    assert all(len(w) == (0 if empty_newest else n) for w in walks)
    if empty_newest:
        assert (al["pages"][al["first"], 1] == 0).all() and al["counter"] == fr.total * (n // 12 + 1)
    ks = list(range(n)) if only is None else list(only)
    lc.indicator_check(rig, fr, be.depth, al, lights, be.render, what=case, only=ks, none_lit=ks if empty_newest else ())


@pytest.mark.parametrize("near", [1, 3])
@pytest.mark.parametrize("case", list(PAGE_EDGES))
def test_page_edges(flat, case, near):
    page_edge_case(*flat, case, near)


# lights (all hit every cluster), pool: 13 lights ask for two pages a cluster, 37 for four
POOLS = {"demand": (13, 48), "one_short": (13, 47), "inside": (13, 11), "one": (13, 1, (1, 1, 1), 0), "fewer_than_clusters": (13, 19), "three_of_four": (37, 23), "two_of_four": (37, 4 * 7 + 2)}


def pool_case(rig, be, name):
    n, pool, grid, near = (POOLS[name] + ((3, 2, 4), 1))[:4]      # (a pool of 1 on the one-cluster grid: the only list there is covers the frame)
    rig.apply([], grid=grid, near=near)
    lights = lc.surface_lights(rig, be.depth, n, seed=100 + n)
    fr = rig.apply(lights, grid=grid, near=near)
    per = n // 12 + 1
    be.pool = pool
    hit, al = lc.check_lists(fr, be.planes(), pool, *be.lists(), what=name)
    assert (hit.sum(axis=1) == n).all()
    c, kept = pool // per, pool % per      # premise: clusters before c whole, c keeps `kept` full pages (the pool runs out inside it), every later one a null first page
    assert (al["numLights"][:c] == n).all() and (al["first"][c + 1:] == ref.NULL).all()
    if name == "demand":
        assert c == fr.total and al["counter"] == pool
    else:
        assert c < fr.total and al["numLights"][c] == 12 * kept and (al["first"][c] == pool - 1 if kept else al["first"][c] == ref.NULL)
    if name == "three_of_four":
        assert kept == 3
    cov = lc.covered_of(be.depth)
    ci = ref.pixel_cluster(fr, ref.world_position(fr, be.depth)[0][..., 2])[3]
    seen = np.unique(ci[cov])
    assert name == "one" or (seen < c).any()                                                     # a covered cluster that kept its lists ...
    assert name != "three_of_four" or c in seen                                                 # ... and the one the pool ran out in is on screen
    ks = list(range(n)) if n == 13 else [0, 11, 12, 23, 24, 35, 36]
    # A light beyond the pages the exhausted cluster kept is in the lists of the whole clusters only, and with a pool of 1 only cluster 0 has a list at all: whether
    # such a frame shows anything is a matter of which clusters are on screen.  The frames the restatement says are black are declared; the others must hold both.
    lit = lc.restated_lit(fr, be.depth, al, ks)
    none = [k for k in ks if not lit[k].any()]
    assert none == [12] if name == "one" else len(none) < len(ks) // 2, (name, none)
    lc.indicator_check(rig, fr, be.depth, al, lights, be.render, what=name, only=ks, none_lit=none)


@pytest.mark.parametrize("name", list(POOLS))
def test_pool_exhaustion(flat, name):
    pool_case(*flat, name)


@pytest.mark.parametrize("grid,near", [((12, 12, 24), 4), ((5, 7, 3), 1)])
def test_sphere_edges(flat, grid, near):
    rig, be = flat
    fr = rig.apply([], grid=grid, near=near)
    lights, c, at = lc.sphere_edge_lights(rig, fr, be.planes())
    fr = rig.apply(lights, grid=grid, near=near)
    be.pool = fr.total * 3
    hit, al = lc.check_lists(fr, be.planes(), be.pool, *be.lists(), what="spheres")
    for name, want in (("inside", True), ("zero_inside", True), ("zero_outside", False), ("negative", True), ("touch", True), ("touch_below", False), ("touch_above", True),
                       ("huge", True), ("spot_inside", True)):
        assert bool(hit[c, at[name]]) == want, name
    assert not hit[:, at["behind_eye"]].any() and not hit[:, at["beyond_far"]].any() and hit[:, at["huge"]].all()
    assert np.isfinite(fr.light_f()[:len(lights), 4:7]).all()


@pytest.mark.parametrize("which", ["flat", "deep"])
def test_types_range_and_cone_edges_through_the_image(flat, deep, which):
    rig, be = flat if which == "flat" else deep
    lc.types_range_cone_case(rig, be, lc.pick_target(be.depth), deep=which == "deep")


@pytest.mark.parametrize("mode", ["rough", "exact"])
def test_edges_and_ratio_on_plain_pixels_at_both_roughness_settings(plain, mode):
    """the frames test_lightgrid_gpu.py renders to reach both instantiations of the kernels' light loop; the oracle has one loop"""
    rig, be = plain
    target = lc.pick_target(be.depth)
    be.set_roughness(mode, target)
    lc.types_range_cone_case(rig, be, target, what="types " + mode)
    lc.ratio_case(rig, be, "oracle plain " + mode)


def test_attenuation_and_cone_by_linearity(flat):
    """on the scene with coat and fuzz materials"""
    lc.ratio_case(*flat, "oracle")
