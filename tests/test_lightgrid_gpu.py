"""Clustered lighting on the GPU held to tests/lightgrid_ref.py: the cases of tests/test_lightgrid_cpu.py on the kernels.

Lists (cluster boxes, numLights, ptrFirstPage, page words, CNT_LIGHT_PAGES) bit for bit through three routes that must also agree byte for byte: the stage
entry point brmi_light_clustering, brmi_execute (the clustering rides the culling launches) and brmi_execute_split on a second stream.  The flat lists
k_shade reads are workspace: the image is their only witness, through the indicator method of lightgrid_cases.indicator_check.  The cluster and page
buffers are filled with 0xCD before every route, and every route is held to the restatement on its own: a route that skips a cluster fails.
"""
import os

import numpy as np
import pytest

import lightgrid_cases as lc
import lightgrid_ref as ref
from test_lightgrid_cpu import COUNTS, GRIDS, PAGE_EDGES, POOLS, page_edge_case, permuted_case, pool_case

pytestmark = pytest.mark.gpu
f32 = np.float32


class _Pool:
    def __init__(self, pool):
        self.pool = pool

    def __enter__(self):
        self.old = os.environ.get("BRMI_TUNING")
        os.environ["BRMI_TUNING"] = f"light_page_pool={self.pool}"

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("BRMI_TUNING", None)
        else:
            os.environ["BRMI_TUNING"] = self.old


class GpuBackend:
    """Renderers of the rig's current grid with a page pool of `pool`, one with clustered lighting, one without, made when first asked for and again when the
    grid or the pool changes.  After every whole frame the emissive plane is zeroed and set_roughness's codes are written: the stages run on that G-buffer."""

    def __init__(self, rig, pool=3456 * 4):
        import orc
        self.rig, self._pool, self.r, self.key, self.rough = rig, pool, {}, None, None
        # The slice planes the restatement takes are orc_cluster_planes' (host logf / expf, the arithmetic of brmi_update): the library's own planes have no read
        # accessor.  A difference between the two would show in the bit-exact boxes; the float64 bound on the planes is applied to the oracle's only (CPU file).
        self._orc = orc.OracleFrame(rig.scene)
        self._depth = None

    @property
    def pool(self):
        return self._pool

    @pool.setter
    def pool(self, value):
        self._pool = int(value)

    @property
    def depth(self):
        if self._depth is None:
            self._depth = self.get(True).depth()
        return self._depth

    def _prepare(self, r):
        from basicrenderer_amd import capi
        r.torch.cuda.synchronize()
        r.res[capi.RES["GBUF_EMISSIVE"]].zero_()
        if self.rough is not None:
            mode, (y, x) = self.rough
            mr = r.res[capi.RES["GBUF_METALLIC_ROUGHNESS"]]
            mr.view(-1, 4)[:, 1] = lc.ROUGH_CODE
            if mode == "exact":
                tiles_x = (lc.W + 7) // 8      # tiled 8 x 8, column-major inside a tile (renderer.detile)
                mr.view(-1, 4)[((y // 8) * tiles_x + x // 8) * 64 + (x % 8) * 8 + (y % 8), 1] = lc.SMOOTH_CODE
            g = r.gbuffer()
            lc.roughness_premise(g["mr"], g["coat"], lc.covered_of(r.depth()), mode, (y, x))

    def set_roughness(self, mode, target):
        self.rough = (mode, target)
        for r in self.r.values():
            self._prepare(r)

    def get(self, clustered):
        from basicrenderer_amd import capi
        from basicrenderer_amd.renderer import VisibilityRenderer
        key = (self.rig.grid, self._pool)
        if key != self.key:
            self.close()
            self.key = key
        if clustered not in self.r:
            with _Pool(self._pool):
                r = VisibilityRenderer(self.rig.scene, lightClusterSize=(capi.u32 * 3)(*self.rig.grid), enableClusteredLighting=1 if clustered else 0)
            r.execute()
            self._prepare(r)
            self.r[clustered] = r
        return self.r[clustered]

    def planes(self):
        return self._orc.cluster_planes()

    def sync(self, r):
        """the rig's light buffer, active list and per-frame record as they are now, to this renderer's device copies; then brmi_update"""
        for name in ("lights", "activeLightIndices", "perFrame"):
            r.device_arrays[name].copy_(r.torch.from_numpy(np.ascontiguousarray(self.rig.scene.arrays[name])).to(r.device))
        r.update()

    def lists(self, route="stage"):
        from basicrenderer_amd import capi
        r = self.get(True)
        self.sync(r)
        r.res[capi.RES["LIGHT_CLUSTERS"]].fill_(0xCD)
        r.res[capi.RES["LIGHT_PAGES"]].fill_(0xCD)
        if route == "stage":
            r.stage("light_clustering")
        else:
            if route == "execute":
                r.execute()
            else:
                other = r.torch.cuda.Stream(device=r.device)
                r.execute(shading_stream=other)
                other.synchronize()
            self._prepare(r)
        c, p = r.light_clusters()
        return c.copy(), p.copy(), int(r.counters().lightPagesUsed)

    def render(self, records, clustered):
        r = self.get(clustered)
        L = self.rig.scene.arrays["lights"].view(np.uint32).reshape(-1, 32)
        keep = L.copy()
        L[:len(records)] = records
        try:
            self.sync(r)
            if clustered:
                r.stage("light_clustering")
            r.stage("shade")
            return r.hdr().copy()
        finally:
            L[:] = keep

    def close(self):
        for r in self.r.values():
            r.close()
        self.r = {}


@pytest.fixture(scope="module")
def flat():
    return lc.Rig("tiny", material_features=3)


@pytest.fixture(scope="module")
def deep():
    return lc.Rig("sponza", size_scale=0.15)


@pytest.fixture(scope="module")
def plain():
    return lc.Rig("tiny")


def _three_routes(be, fr, what):
    """each route writes into poisoned buffers and is held to the restatement on its own; then the three agree byte for byte"""
    got, out = {}, None
    for route in ("stage", "execute", "split"):
        got[route] = be.lists(route)
        out = lc.check_lists(fr, be.planes(), be.pool, *got[route], what=(what, route))
    n, used = fr.total, min(got["stage"][2], be.pool)
    for route in ("execute", "split"):
        assert np.array_equal(got[route][0][:n], got["stage"][0][:n]) and got[route][2] == got["stage"][2], (what, route, "clusters")
        assert np.array_equal(got[route][1][:used], got["stage"][1][:used]), (what, route, "pages")
    return out


@pytest.mark.parametrize("grid,near,z_split", GRIDS)
def test_lists_through_three_routes(flat, grid, near, z_split):
    rig = flat
    fr = rig.apply([], grid=grid, near=near, z_split=z_split)
    be = GpuBackend(rig, fr.total * 12)
    try:
        for count in (COUNTS if fr.total <= 3456 else [13, 65]):
            fr = rig.apply(lc.random_lights(rig, count, seed=count), grid=grid, near=near, z_split=z_split)
            _three_routes(be, fr, (grid, count))
    finally:
        be.close()


def test_active_list_shorter_than_the_buffer_and_not_the_identity(flat):
    """... and, through the image, that the light shaded for a page word is activeLightIndices[word] (lighting.hlsli:528)"""
    rig = flat
    fr = rig.apply([])
    be = GpuBackend(rig, fr.total * 4)
    try:
        lights, perm = permuted_case(rig, be)
        for active, num in ((None, 7), (perm, 23)):
            _three_routes(be, rig.apply(lights, active=active, num=num), ("active", num))
        sub = lights[:23]
        fr = rig.apply(sub, active=perm, num=23)
        hit, al = lc.check_lists(fr, be.planes(), be.pool, *be.lists(), what="perm")
        lc.indicator_check(rig, fr, be.depth, al, sub, be.render, what="perm")
    finally:
        be.close()


def test_grids_the_library_refuses():
    """(a scene of its own: a renderer whose constructor raised is closed whenever it is collected, and closing drops its scene's device arrays)"""
    import gc
    from basicrenderer_amd import capi
    from basicrenderer_amd.renderer import BrmiError, VisibilityRenderer
    rig = lc.Rig("tiny")
    rig.apply([], grid=(2, 2, 63))
    with pytest.raises(BrmiError, match="brmi_create"):
        VisibilityRenderer(rig.scene, lightClusterSize=(capi.u32 * 3)(2, 2, 63))
    rig.apply([], grid=(3, 2, 4))
    with pytest.raises(BrmiError, match="light cluster grid differs"):
        VisibilityRenderer(rig.scene, lightClusterSize=(capi.u32 * 3)(3, 2, 5))
    gc.collect()


@pytest.mark.parametrize("near", [1, 3])
@pytest.mark.parametrize("case", list(PAGE_EDGES))
def test_page_edges(flat, case, near):
    rig = flat
    rig.apply([], grid=(3, 2, 4), near=near)
    be = GpuBackend(rig, 400)
    try:
        page_edge_case(rig, be, case, near)
        _three_routes(be, ref.Frame(rig.scene.arrays), case)
    finally:
        be.close()


@pytest.mark.parametrize("name", list(POOLS))
def test_pool_exhaustion(flat, name):
    rig = flat
    grid, near = (POOLS[name] + ((3, 2, 4), 1))[2:4]
    rig.apply([], grid=grid, near=near)
    be = GpuBackend(rig, POOLS[name][1])
    try:
        pool_case(rig, be, name)
        _three_routes(be, ref.Frame(rig.scene.arrays), name)
    finally:
        be.close()


@pytest.mark.parametrize("grid,near", [((12, 12, 24), 4), ((5, 7, 3), 1)])
def test_sphere_edges(flat, grid, near):
    rig = flat
    fr = rig.apply([], grid=grid, near=near)
    be = GpuBackend(rig, fr.total * 3)
    try:
        lights, c, at = lc.sphere_edge_lights(rig, fr, be.planes())
        fr = rig.apply(lights, grid=grid, near=near)
        hit, al = _three_routes(be, fr, "spheres")
        assert hit[c, at["touch"]] and not hit[c, at["touch_below"]] and hit[c, at["negative"]] and not hit[c, at["zero_outside"]]
    finally:
        be.close()


@pytest.mark.parametrize("which", ["flat", "deep"])
def test_types_range_and_cone_edges_through_the_image(flat, deep, which):
    rig = flat if which == "flat" else deep
    rig.apply([])
    be = GpuBackend(rig)
    try:
        lc.types_range_cone_case(rig, be, lc.pick_target(be.depth), deep=which == "deep")
    finally:
        be.close()


@pytest.mark.parametrize("mode", ["rough", "exact"])
def test_edges_and_ratio_through_both_instantiations_of_the_light_loop(plain, mode):
    """k_shade<0> picks the light loop per 8 x 8 tile: the fast-directions form where every live pixel's roughness^2 is at least SHADE_FAST_ALPHA = 0.1, the exact
    form where one is below.  On a scene of plain materials only, with the G-buffer's roughness codes rewritten before the shading stage: "rough" = every covered
    pixel at code 200 (every tile fast), "exact" = the same but the target pixel at code 10 (its tile exact; the +-1 ulp range and cone lights are judged at that
    pixel).  The premise is asserted on the G-buffer read back (lightgrid_cases.roughness_premise)."""
    rig = plain
    rig.apply([])
    be = GpuBackend(rig)
    try:
        target = lc.pick_target(be.depth)
        be.set_roughness(mode, target)
        lc.types_range_cone_case(rig, be, target, what="types " + mode)
        lc.ratio_case(rig, be, "kernels plain " + mode)
    finally:
        be.close()


def test_attenuation_and_cone_by_linearity(flat):
    """on the scene with coat and fuzz materials (k_shade<1..3>); the worst error / bound is printed for profiles/lightgrid_accuracy.md"""
    rig = flat
    rig.apply([])
    be = GpuBackend(rig)
    try:
        lc.ratio_case(rig, be, "kernels")
    finally:
        be.close()
