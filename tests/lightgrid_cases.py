"""The cases of tests/test_lightgrid_cpu.py and tests/test_lightgrid_gpu.py, and the checks both run (TEST INFRASTRUCTURE).

A `Rig` is one 164 x 100 scene whose light buffer (160 records), active-light list and per-frame grid are rewritten in numpy before anything reads
them.  A backend (the oracle on the CPU, the kernels on the GPU) gives, for the rig's current state, the cluster and page buffers and the HDR image;
the checks hold them to tests/lightgrid_ref.py.  Nothing here looks at what a backend returns to choose a light, a target or a bound: targets come
from the depth plane (geometry, which neither backend's lighting touches) and from the restatement.
"""
import numpy as np

import lightgrid_ref as ref

f32 = np.float32
W, H, MAX_LIGHTS = 164, 100, 160
EMPTY_DEPTH = 0x7F7FFFFF
POINT, SPOT, DIRECTIONAL = 0, 1, 2


def light(kind, pos=(0, 0, 0), radius=1.0, direction=(0, -1, 0), attenuation=(1, 0, 0), color=(1, 1, 1), intensity=1.0, max_range=None, inner=1.0, outer=0.0, sphere=None):
    """one LightInfo record (32 words); the bounding sphere is (pos, radius) unless `sphere` = (x, y, z, r) says otherwise"""
    r = np.zeros(32, dtype=np.uint32)
    f = r.view(f32)
    r[0] = kind
    f[1], f[2] = inner, outer
    r[3] = 0xFFFFFFFF
    f[4:7], f[7] = pos, 1.0
    f[8:11] = direction
    f[12:15] = attenuation
    f[15] = radius if max_range is None else max_range
    f[16:19], f[19] = color, intensity
    r[22] = r[23] = 0xFFFFFFFF
    f[25:29] = sphere if sphere is not None else (pos[0], pos[1], pos[2], radius)
    f[29] = radius if max_range is None else max_range
    return r


class Rig:
    def __init__(self, preset, **kw):
        from conftest import Scene
        self.scene = Scene(preset, W, H, point_lights=MAX_LIGHTS, directional=False, **kw)
        a = self.scene.arrays
        assert a["lights"].nbytes == MAX_LIGHTS * 128 and self.scene.counts["lights"] == MAX_LIGHTS
        self.apply([])

    def apply(self, lights, grid=(12, 12, 24), near=4, z_split=6.0, active=None, num=None):
        """rewrite the scene in place; returns the restatement's Frame of the new state"""
        a = self.scene.arrays
        L = a["lights"].view(np.uint32).reshape(-1, 32)
        L[:] = 0
        for i, rec in enumerate(lights):
            L[i] = rec
        act = a["activeLightIndices"].view(np.uint32)
        assert len(act) >= MAX_LIGHTS
        act[:] = 0
        act[:MAX_LIGHTS] = np.arange(MAX_LIGHTS)
        if active is not None:
            act[:len(active)] = active
        pf = a["perFrame"].view(np.uint32)
        pf[9] = len(lights) if num is None else num
        pf[15:18] = grid
        pf[18] = near
        pf.view(f32)[19] = z_split
        self.grid = tuple(grid)
        return ref.Frame(a)

    def to_world(self, view_pos):
        """a view-space point as an fp32 world position (float64 through viewInverse, rounded once)"""
        fr = ref.Frame(self.scene.arrays)
        v = np.concatenate([np.asarray(view_pos, dtype=np.float64), [1.0]])
        return (v @ fr.view_inverse.astype(np.float64))[:3].astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# light sets
def random_lights(rig, count, seed, kinds=(POINT, POINT, POINT, SPOT, DIRECTIONAL, 3, 4, 5, 6, 7)):
    """`count` lights in and around the view frustum: spheres from a twentieth of a tile to several slices wide, every type"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        z = -float(np.exp(rng.uniform(np.log(0.3), np.log(80.0))))
        x, y = rng.uniform(-1.2, 1.2, size=2) * -z
        kind = kinds[int(rng.integers(0, len(kinds)))] if i % 3 else POINT
        d = rng.normal(size=3)
        out.append(light(kind, rig.to_world((x, y, z)), radius=float(np.exp(rng.uniform(np.log(0.05), np.log(12.0)))), direction=d, inner=0.95, outer=0.6,
                         attenuation=(1.0, 0.1, 0.02), intensity=float(rng.uniform(2, 20))))
    return out


def directional_set(count, tail=()):
    """`count` directional lights (every cluster hits every one of them), then `tail`"""
    rng = np.random.default_rng(count)
    out = []
    for _ in range(count):
        d = rng.normal(size=3)
        d[1] = -abs(d[1]) - 0.5
        out.append(light(DIRECTIONAL, direction=d / np.linalg.norm(d), intensity=float(rng.uniform(0.5, 2))))
    return out + list(tail)


def surface_lights(rig, depth, count, seed, sphere=1000.0, max_range=2.5, spots=False):
    """`count` point lights (every third a spot light aimed at its pixel with `spots`) one unit in front of randomly chosen covered pixels, towards the eye.  With the
    default bounding sphere of radius 1000 every cluster hits every one of them, as with directional lights, but `max_range` keeps each to a part of the frame: an
    indicator frame then holds lit pixels and exactly-zero ones.  With `sphere` = the range, membership varies from cluster to cluster as well."""
    fr = ref.Frame(rig.scene.arrays)
    cov = covered_of(depth)
    _, ws = ref.world_position(fr, depth)
    ys, xs = np.nonzero(cov)
    rng = np.random.default_rng(seed)
    out = []
    for i, j in enumerate(rng.choice(len(ys), size=count, replace=count > len(ys))):
        at = ws[ys[j], xs[j]].astype(np.float64)
        to_eye = fr.cam_pos[:3].astype(np.float64) - at
        pos = (at + to_eye / np.linalg.norm(to_eye)).astype(f32)
        kind = SPOT if spots and i % 3 == 2 else POINT
        out.append(light(kind, pos, radius=sphere, max_range=max_range, direction=-to_eye, inner=0.9, outer=0.5, intensity=8.0))
    return out


def far_miss(rig):
    """a point light that touches no cluster: a small sphere far beside the frustum"""
    return light(POINT, rig.to_world((500.0, 0.0, -3.0)), radius=0.25, intensity=5.0)


def sphere_edge_lights(rig, fr, planes):
    """Lights for one chosen cluster of the current grid: centre inside its box; radius 0 inside the box and outside it; a negative radius (r * r > 0: it
    hits, as in the shader); a sphere whose fp32 d^2 to the box equals r * r exactly, and the radii one ulp below and above; behind the eye; beyond zFar;
    radius 1e20.  Returns (lights, cluster index, dict of list positions)."""
    lo, hi = ref.boxes(fr, planes)
    c = fr.total // 2 + fr.gx // 2 if fr.total > 2 else 0
    mid = (lo[c].astype(np.float64) + hi[c].astype(np.float64)) / 2
    size = hi[c].astype(np.float64) - lo[c].astype(np.float64)
    lights, at = [], {}

    def add(name, rec):
        at[name] = len(lights)
        lights.append(rec)

    add("inside", light(POINT, rig.to_world(mid), radius=float(size.min()) / 8))
    add("zero_inside", light(POINT, rig.to_world(mid), radius=0.0, max_range=5.0))
    beside = mid + np.array([size[0], 0, 0])
    add("zero_outside", light(POINT, rig.to_world(beside), radius=0.0, max_range=5.0))
    add("negative", light(POINT, rig.to_world(beside), radius=-float(size[0]), max_range=5.0))
    # exact touch: look for a centre whose fp32 squared distance to the box is the fp32 square of some radius
    rng = np.random.default_rng(5)
    for _ in range(4000):
        p = rig.to_world(mid + np.array([size[0] * rng.uniform(0.8, 3.0), size[1] * rng.uniform(-0.3, 0.3), 0.0]))
        probe = rig.apply([light(POINT, p, radius=1.0)], grid=rig.grid, near=fr.near_slices, z_split=float(fr.z_split))
        cv, _ = ref.centres(probe)
        d = np.maximum(lo[c], np.minimum(cv[0], hi[c])) - cv[0]
        d2 = ref.dot3(d, d)
        r = np.sqrt(d2)
        if d2 > 0 and r * r == d2:
            break
    else:
        raise AssertionError("no exactly touching sphere found")
    add("touch", light(POINT, p, radius=float(r), max_range=5.0))
    add("touch_below", light(POINT, p, radius=float(np.nextafter(r, f32(0))), max_range=5.0))
    add("touch_above", light(POINT, p, radius=float(np.nextafter(r, f32(np.inf))), max_range=5.0))
    add("behind_eye", light(POINT, rig.to_world((0.0, 0.0, 5.0)), radius=2.0))
    add("beyond_far", light(POINT, rig.to_world((0.0, 0.0, -float(fr.z_far) * 1.5)), radius=2.0))
    add("huge", light(POINT, rig.to_world(mid), radius=1.0e20, max_range=2.0))
    add("spot_inside", light(SPOT, rig.to_world(mid), radius=float(size.min()) / 8, inner=0.9, outer=0.5))
    return lights, c, at


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# checks
def restated_lists(fr, planes, pool):
    lo, hi = ref.boxes(fr, planes)
    hit = ref.hits(fr, lo, hi)
    return lo, hi, hit, ref.allocate(fr, hit, pool)


def check_lists(fr, planes, pool, clusters, pages, used, what=""):
    """boxes, numLights, ptrFirstPage, every page word the shader stores and the pages-used count, bit for bit; returns the restatement's (hit, alloc)"""
    clusters, pages = np.asarray(clusters).view(np.uint32).reshape(-1, 12)[:fr.total], np.asarray(pages).view(np.uint32).reshape(-1, 14)[:pool]
    lo, hi, hit, al = restated_lists(fr, planes, pool)
    for k, (want, got) in enumerate(((lo, clusters[:, 0:3]), (hi, clusters[:, 4:7]))):
        bad = np.flatnonzero((want.view(np.uint32) != got).any(axis=1))
        assert len(bad) == 0, (what, "box min" if k == 0 else "box max", len(bad), bad[:4], want[bad[:2]], got[bad[:2]].view(f32))
    assert (clusters[:, 3] == 0).all() and (clusters[:, 7] == 0).all()
    assert np.array_equal(clusters[:, 8], al["numLights"]), (what, "numLights", np.flatnonzero(clusters[:, 8] != al["numLights"])[:8])
    assert np.array_equal(clusters[:, 9], al["first"]), (what, "ptrFirstPage", np.flatnonzero(clusters[:, 9] != al["first"])[:8])
    bad = al["written"] & (pages != al["pages"])
    assert not bad.any(), (what, "page words", np.argwhere(bad)[:8])
    assert used == min(al["counter"], pool), (what, "pages used", used, al["counter"], pool)
    return hit, al


def planes_within_bound(fr, planes):
    want, got = ref.planes64(fr), np.asarray(planes, dtype=np.float64).reshape(fr.gz, 2)
    err = np.abs(got - want) / np.abs(want)
    return float(err.max()), ref.planes_bound(fr)


def covered_of(depth):
    return np.ascontiguousarray(depth).view(np.uint32) != EMPTY_DEPTH


def expected_reach(fr, depth, alloc):
    """per pixel: the cluster index, and per cluster the list of lights the text's walk shades"""
    vs, ws = ref.world_position(fr, depth)
    _, _, sl, ci = ref.pixel_cluster(fr, vs[..., 2])
    walks = [ref.walk(fr, alloc["numLights"][c], alloc["first"][c], alloc["pages"])[1] for c in range(fr.total)]
    return ws, sl, ci, walks


def restated_lit(fr, depth, alloc, ks):
    """{k: [H, W] bool}: the covered pixels the restatement says list position k's light is shaded at (the walk reaches it, no fp32 decision rejects it)"""
    cov = covered_of(depth)
    ws, sl, ci, walks = expected_reach(fr, depth, alloc)
    out = {}
    for k in ks:
        lk = int(fr.active[k])
        reach = np.isin(ci, [c for c in np.unique(ci[cov]) if lk in walks[int(c)]])
        out[k] = reach & ~ref.pixel_light(fr, ws, lk)["rejected"] & cov
    return out


def indicator_check(rig, fr, depth, alloc, lights, render, deliberate=(), what="", frames=None, only=None, none_lit=()):
    """The indicator method.  `render(records, clustered)` -> HDR [H, W] uint64 of the rig with those light records.  In frame k only light k keeps its colour.
    A covered pixel's HDR must be exactly 0 where the walk of its cluster does not reach light k or an fp32 decision rejects it, and elsewhere the bits of
    the same frame without clustered lighting.  It sees a wrong list ORDER only where the order changes bits, which with one coloured light it never does:
    membership is what it pins.  `deliberate` = {list position: (y, x)}: the pairs placed on an edge on purpose, left out of the 1 % cap.  `frames`, a dict, receives
    {k: (clustered HDR, lit mask)}.  Both frames of a light come from the same backend, so a decision that is wrong in the same way with and without clustering is
    not seen here: the caller holds lights that differ in one field against each other for that.
    Every frame must hold an exactly-zero covered pixel and a non-zero one, or it proves nothing; the list positions in `none_lit` are the exception the caller
    declares -- lights the restatement says shade no pixel at all (a type the clustering ignores, a range no pixel is within, a cluster whose newest page is
    empty) -- and for those that premise is asserted on the restatement and the frame must be black.  `only`: the list positions to render (default: all)."""
    cov = covered_of(depth)
    ws, sl, ci, walks = expected_reach(fr, depth, alloc)
    assert cov.any() and (ci[cov] < fr.total).all(), (what, "a covered pixel lies behind the grid")
    n = fr.num_lights
    # the 1 % cap on pairs whose fp32 and float64 decisions differ, on the restatement alone
    edge, pairs = 0, 0
    facts = {}
    for li in sorted(set(int(v) for v in fr.active[:n])):
        facts[li] = ref.pixel_light(fr, ws, li)
        e = facts[li]["on_edge"] & cov
        for pos, (y, x) in dict(deliberate).items():
            if int(fr.active[pos]) == li:
                e[y, x] = False
        edge, pairs = edge + int(e.sum()), pairs + int(cov.sum())
    assert edge <= 0.01 * pairs, (what, "on the edge", edge, pairs)
    summary = []
    for k in (range(n) if only is None else only):
        lk = int(fr.active[k])
        recs = [np.array(r, copy=True) for r in lights]
        for j, r in enumerate(recs):
            if j != lk:
                r.view(f32)[16:20] = 0.0
        clustered = render(recs, True)
        plain = render(recs, False)
        reach = np.zeros((H, W), dtype=bool)
        for c in np.unique(ci[cov]):
            if lk in walks[int(c)]:
                reach |= ci == c
        lit = reach & ~facts[lk]["rejected"] & cov
        rgb = clustered.view(np.uint16).reshape(H, W, 4)[..., :3]
        dark = cov & ~lit
        assert (rgb[dark] == 0).all(), (what, "light", k, "shows where the walk or a decision excludes it", np.argwhere(dark & (rgb != 0).any(-1))[:4])
        assert (clustered[lit] == plain[lit]).all(), (what, "light", k, "differs from the unclustered frame", np.argwhere(lit & (clustered != plain))[:4])
        if frames is not None:
            frames[k] = (clustered, lit)
        zero, nonzero = int(((rgb == 0).all(-1) & cov).sum()), int(((rgb != 0).any(-1) & cov).sum())
        if k in none_lit:
            assert not lit.any() and nonzero == 0, (what, "light", k, "was declared to shade nothing", int(lit.sum()), nonzero)
        else:
            assert zero > 0 and nonzero > 0, (what, "light", k, "frame without an exactly-zero covered pixel or without a lit one", zero, nonzero)
        summary.append((zero, nonzero))
    return summary


def half_ulp16(x):
    """half an fp16 ulp at |x| (normal range; 2^-25 below it)"""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -14)))
    return 2.0 ** (e - 11)


def ratio_check(hdr_a, hdr_b, rho, cov, what=""):
    """HDR_B = HDR_A * rho per channel within 0.5 ulp16(HDR_A) rho + 0.5 ulp16(HDR_B) + 2^-18 |HDR_B|; pixels whose HDR_A is below the fp16 normal range
    are left out (at most 5 % of the lit pixels).  Returns the worst error / bound."""
    a = hdr_a.view(np.float16).reshape(H, W, 4)[..., :3].astype(np.float64)
    b = hdr_b.view(np.float16).reshape(H, W, 4)[..., :3].astype(np.float64)
    lit = cov & (a > 0).any(-1)
    normal = cov[..., None] & (a >= 2.0 ** -14)
    tiny = lit & ((a > 0) & (a < 2.0 ** -14)).any(-1)
    assert lit.any() and tiny.sum() <= 0.05 * lit.sum(), (what, int(tiny.sum()), int(lit.sum()))
    want = a * rho[..., None]
    bound = half_ulp16(a) * rho[..., None] + half_ulp16(b) + 2.0 ** -18 * np.abs(b)
    err = np.abs(b - want)
    worst = float((err[normal] / bound[normal]).max())
    zero_a = cov[..., None] & (a == 0)
    assert (b[zero_a] == 0).all(), (what, "light where frame A has none")
    return worst, int(normal.sum())


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# cases run through a backend: .depth, .pool (settable before lists / render), .planes(), .lists() -> (clusters, pages, used), .render(records, clustered)
def pick_target(depth, seed=9):
    ys, xs = np.nonzero(covered_of(depth))
    i = int(np.random.default_rng(seed).integers(0, len(ys)))
    return int(ys[i]), int(xs[i])


def types_range_cone_case(rig, be, target, deep=False, what="types"):
    """Types 0 - 7 clustered and not (the clustering ignores 3 - 7, the unclustered loop shades them as point lights); maxRange at the target pixel's fp32 distance
    and one ulp to each side, 0, negative, 1e-20, 1e20; the cone's outer and inner cosine at the target's cosine and one ulp to each side, inner == outer,
    outer < -1."""
    fr = rig.apply([])
    cov = covered_of(be.depth)
    vs, ws = ref.world_position(fr, be.depth)
    if deep:
        assert len(np.unique(ref.pixel_cluster(fr, vs[..., 2])[2][cov])) >= 3      # premise: depth across several slices
    ty, tx = target
    assert cov[ty, tx]
    lights, deliberate = [], {}
    p = (ws[ty, tx].astype(np.float64) + np.array([0.3, 1.5, 0.2])).astype(f32)
    aim = (0.1, -1.0, 0.05)
    for kind in range(8):
        lights.append(light(kind, p, radius=6.0, direction=aim, inner=0.9, outer=0.3, intensity=8.0))
    facts = ref.pixel_light(rig.apply([light(SPOT, p, radius=6.0, direction=aim)]), ws, 0)
    d, cosine = facts["distance"][ty, tx], facts["cos"][ty, tx]
    for rng_ in (d, np.nextafter(d, f32(0)), np.nextafter(d, f32(np.inf)), f32(0), f32(-1), f32(1e-20), f32(1e20)):
        deliberate[len(lights)] = (ty, tx)
        lights.append(light(POINT, p, radius=6.0, max_range=float(rng_), intensity=8.0))
    for outer in (cosine, np.nextafter(cosine, f32(-1)), np.nextafter(cosine, f32(1)), f32(-1.5)):
        deliberate[len(lights)] = (ty, tx)
        lights.append(light(SPOT, p, radius=6.0, direction=aim, inner=0.999, outer=float(outer), intensity=8.0))
    for inner in (cosine, np.nextafter(cosine, f32(-1)), np.nextafter(cosine, f32(1))):
        deliberate[len(lights)] = (ty, tx)
        lights.append(light(SPOT, p, radius=6.0, direction=aim, inner=float(inner), outer=0.1, intensity=8.0))
    deliberate[len(lights)] = (ty, tx)
    lights.append(light(SPOT, p, radius=6.0, direction=aim, inner=float(cosine), outer=float(cosine), intensity=8.0))
    fr = rig.apply(lights)
    be.pool = fr.total * 4
    hit, al = check_lists(fr, be.planes(), be.pool, *be.lists(), what=what)
    assert hit[:, :3].any() and not hit[:, 3:8].any()      # the clustering's switch has no case for types 3 - 7
    # premises on the restatement: the equal-range light reaches the target, one ulp below does not; likewise the cone
    r = {k: ref.pixel_light(fr, ws, k) for k in range(len(lights))}
    assert not r[8]["cut"][ty, tx] and r[9]["cut"][ty, tx] and not r[10]["cut"][ty, tx] and r[11]["cut"][cov].all() and r[12]["cut"][cov].all() and r[13]["cut"][cov].all() and not r[14]["cut"][cov].any()
    assert r[15]["outside"][ty, tx] and not r[16]["outside"][ty, tx] and r[17]["outside"][ty, tx] and not r[18]["outside"][cov].any()
    assert not r[19]["below_inner"][ty, tx] and not r[20]["below_inner"][ty, tx] and r[21]["below_inner"][ty, tx] and r[22]["outside"][ty, tx]
    frames = {}
    indicator_check(rig, fr, be.depth, al, lights, be.render, deliberate=deliberate, what=what, frames=frames, none_lit=(3, 4, 5, 6, 7, 11, 12, 13))
    # lights 8 - 14 differ in maxRange alone: where the fp32 decision keeps one of them it shows the bits of the light with a range of 1e20, and the target pixel,
    # which the equal-range light reaches, is lit there (a cone an ulp inside its outer cosine has a smoothstep of 0 in fp16: no such check for it)
    far, lit_far = frames[14]
    assert (far.view(np.uint16).reshape(H, W, 4)[ty, tx, :3] != 0).any() and lit_far[ty, tx]
    for k in (8, 10):
        img, lit = frames[k]
        assert lit[ty, tx] and (img[lit] == far[lit]).all(), k
    # clustering off: types 3 - 7 are shaded through `default:` exactly like the point light in their place
    recs = [np.array(x, copy=True) for x in lights]
    for x in recs:
        x.view(f32)[16:20] = 0.0
    images = []
    for k in (0, 3, 4, 5, 6, 7):
        one = [np.array(x, copy=True) for x in recs]
        one[k].view(f32)[16:20] = lights[k].view(f32)[16:20]
        images.append(be.render(one, False))
    assert all((im == images[0]).all() for im in images[1:]) and (images[0].view(np.uint16).reshape(H, W, 4)[..., :3] != 0).any()


def ratio_case(rig, be, label):
    """HDR_B = HDR_A x rho (ratio_check): frame A has attenuation (1, 0, 0) and no cone, frame B (c, l, q) and / or a cone.  Returns {name: worst error / bound}."""
    fr = rig.apply([])
    cov = covered_of(be.depth)
    vs, ws = ref.world_position(fr, be.depth)
    p = (ws[cov].astype(np.float64).mean(axis=0) + np.array([0.2, 2.0, 0.3])).astype(f32)
    aim = (0.05, -1, 0.1)
    a = light(POINT, p, radius=50.0, attenuation=(1, 0, 0), intensity=40.0)
    be.pool = fr.total * 2
    out = {}
    for name, b in (("attenuation", light(POINT, p, radius=50.0, attenuation=(1.5, 0.2, 0.05), intensity=40.0)),
                    ("cone", light(SPOT, p, radius=50.0, attenuation=(1, 0, 0), direction=aim, inner=0.95, outer=0.55, intensity=40.0)),
                    ("both", light(SPOT, p, radius=50.0, attenuation=(2.0, 0.5, 0.01), direction=aim, inner=0.95, outer=0.55, intensity=40.0))):
        fa = ref.pixel_light(rig.apply([a]), ws, 0)
        ha = be.render([a], True)
        fb = ref.pixel_light(rig.apply([b]), ws, 0)
        hb = be.render([b], True)
        with np.errstate(all="ignore"):
            rho = np.where(cov, fb["factor64"] / fa["factor64"], 0.0)
        assert (rho <= 1.0).all() and (rho[cov] > 0).any() and not fa["rejected"][cov].any()
        worst, n = ratio_check(ha, hb, rho, cov, what=name)
        print(f"[lightgrid] {label} {name}: worst error / bound {worst:.3f} over {n} channels")
        assert worst <= 1.0, (label, name, worst)
        out[name] = worst
    return out


ROUGH_CODE, SMOOTH_CODE = 200, 10      # (code / 255)^2 = 0.615 and 0.0015, on either side of the shading pass's fast-directions threshold of 0.1


def roughness_premise(mr, coat, cov, mode, target):
    """the G-buffer a backend shades after set_roughness: every covered pixel plain (no coat weight, no fuzz weight: the pass's MODE 0 pixels) and at ROUGH_CODE,
    but the target at SMOOTH_CODE in "exact" mode"""
    code = (np.asarray(mr) >> 8) & 0xFF
    assert (np.asarray(coat).view(np.uint16).reshape(H, W, 4)[..., 3][cov] == 0).all() and ((np.asarray(mr) >> 24)[cov] == 0).all(), "a layered pixel"
    want = np.full((H, W), ROUGH_CODE)
    if mode == "exact":
        want[target] = SMOOTH_CODE
    assert (code[cov] == want[cov]).all() and cov[target]
    assert (ROUGH_CODE / 255.0) ** 2 >= 0.1 > (SMOOTH_CODE / 255.0) ** 2
