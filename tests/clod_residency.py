"""Residency-aware cluster-LOD cut: test references (TEST INFRASTRUCTURE).

Two things live here.

* `transformed_scene`: the frame reference.  For a non-resident set N the existing oracle renders a second Scene of the same case whose host
  arrays say what N means for the cut: `maxParentError = 0` in every group of N (its boundary error is then below any threshold, so it never
  suppresses a parent) and `meshletCount = 0` in every segment of N's groups (the traversal emits nothing for them, computeCulling.hlsl:372).

* `restate`: the feedback reference.  A numpy float32 restatement of K1 + K2 + the per-meshlet condition 2 WITH the residency rule and the
  streaming requests, written from the shader text (computeCulling.hlsl:103-531, workGraphCulling.hlsl:1012-1018, 1522-1783, 2550-2561,
  2672-2696) in the operation order of oracle/orc_cull.cpp (every product and sum is one float32 operation, no contraction).  No occlusion, no
  skinning.  It returns the reference's raw stream (one entry per touching / requesting thread) and its reduction to the library's output
  contract (include/brmi.h: one record per requested group, descending priority then ascending group; touched groups ascending).
"""
import numpy as np

F = np.float32
NODE_INTERNAL = 0
VERTEX_SKINNED = 1 << 3


def _u32(a, words):
    return a.view(np.uint32).reshape(-1, words)


def _f32(a, words):
    return a.view(np.float32).reshape(-1, words)


class SceneTables:
    """Typed views of a Scene's host arrays (include/brmi_types.h layouts)."""

    def __init__(self, scene):
        A = scene.arrays
        self.scene = scene
        self.md = _u32(A["meshMetadata"], 10)            # groupsBase, segmentsBase, lodNodesBase, rootNode, .., .., pageMapBase
        self.offs = A["clodOffsets"].view(np.uint32)
        self.nodes_u, self.nodes_f = _u32(A["lodNodes"], 16), _f32(A["lodNodes"], 16)
        self.groups_u, self.groups_f = _u32(A["lodGroups"], 19), _f32(A["lodGroups"], 19)
        self.segs = _u32(A["lodSegments"], 4)            # refinedGroup, firstMeshletInPage, meshletCount, pageIndex
        self.pmap = _u32(A["groupPageMap"], 2)
        self.inst_u, self.inst_f = _u32(A["perMeshInstance"], 8), _f32(A["perMeshInstance"], 8)
        self.obj = _f32(A["perObject"], 52)
        self.permesh = _u32(A["perMesh"], 16)
        self.draws = A["activeDraws"].view(np.uint32)[: scene.counts["activeDraws"]]
        self.view_id = int(A["perFrame"].view(np.uint32)[8])
        cam = A["cameras"][self.view_id * 736: (self.view_id + 1) * 736]
        self.view = cam[16:80].view(np.float32).reshape(4, 4).copy()
        self.planes = cam[592:688].view(np.float32).reshape(6, 4).copy()
        self.ortho = int(cam[720:724].view(np.uint32)[0]) != 0
        cc = A["cullingCameras"][self.view_id * 304: (self.view_id + 1) * 304].view(np.float32)
        self.cam_pos, self.z_near, self.threshold = cc[0:3].copy(), F(cc[6]), F(cc[7])
        self.group_count = len(self.groups_u)

    def leaf_segments_of_groups(self):
        """(global group, global segment) of every leaf node of every mesh: the segments the traversal can emit for a group."""
        order = np.argsort(self.md[:, 2], kind="stable")
        ends = np.append(self.md[order, 2][1:], len(self.nodes_u))
        pairs = []
        for m, end in zip(order, ends):
            n = self.nodes_u[self.md[m, 2]: end]
            leaf = n[:, 0] != NODE_INTERNAL
            pairs.append(np.stack([self.md[m, 0] + n[leaf, 3], self.md[m, 1] + n[leaf, 1]], 1))
        return np.concatenate(pairs) if pairs else np.zeros((0, 2), dtype=np.uint32)

    def mesh_of_group(self):
        order = np.argsort(self.md[:, 0], kind="stable")
        starts = self.md[order, 0]
        idx = np.searchsorted(starts, np.arange(self.group_count), side="right") - 1
        return order[idx]


def effective_mask(group_count, non_resident, active_group_scan_count=None):
    """bool[group_count]: groups that are not resident (CLodGroupIsResident: the bit, or an index at / above activeGroupScanCount)."""
    mask = np.zeros(group_count, dtype=bool)
    nr = np.asarray(non_resident)
    if nr.dtype == bool:
        mask[:] = nr
    elif nr.size:
        mask[nr.astype(np.int64)] = True
    if active_group_scan_count is not None:
        mask[int(active_group_scan_count):] = True
    return mask


def finest_depth_groups(scene):
    """Set (c) of the tests: per mesh, the groups of the finest DAG depth (the depth whose groups have no refined group below them: depth 0)."""
    t = SceneTables(scene)
    depth = t.groups_u[:, 7].view(np.int32)
    mesh = t.mesh_of_group()
    out = []
    for m in np.unique(mesh):
        g = np.nonzero(mesh == m)[0]
        out.append(g[depth[g] == depth[g].min()])
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def transformed_scene(make_scene, non_resident, active_group_scan_count=None):
    """A fresh Scene (make_scene()) whose host arrays say "the groups of `non_resident` are not there" to a cut that knows nothing of residency."""
    sc = make_scene()
    t = SceneTables(sc)
    mask = effective_mask(t.group_count, non_resident, active_group_scan_count)
    t.groups_f[mask, 17] = 0.0                                   # maxParentError
    pairs = t.leaf_segments_of_groups()
    t.segs[pairs[mask[pairs[:, 0]], 1], 2] = 0                   # meshletCount
    return sc


def pack_view_priority(view_id, error_over_distance):
    """CLodPackViewPriority (workGraphCulling.hlsl:1012-1018) in float32: HLSL min / max drop a NaN operand."""
    e = F(error_over_distance) * F(1024.0)
    e = e if e > F(0.0) else F(0.0)                              # max(x, 0): NaN -> 0
    e = e if e < F(65535.0) else F(65535.0)
    q = int(F(e + F(0.5)))
    return ((q & 0xFFFF) << 16) | (int(view_id) & 0xFFFF)


# ---- float32 arithmetic in the oracle's association (orc_common.h) -------------------------------------------------
def _mul_point(p, m):      # mul(float4(p, 1), M), row-vector convention; p: [..., 3]
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([((x * m[0, k] + y * m[1, k]) + z * m[2, k]) + m[3, k] for k in range(4)], -1)


def _mul4(v, m):
    return np.stack([((v[..., 0] * m[0, k] + v[..., 1] * m[1, k]) + v[..., 2] * m[2, k]) + v[..., 3] * m[3, k] for k in range(4)], -1)


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _length(a):
    return np.sqrt(_dot3(a, a))


def _max_axis_scale(m):
    l = [_length(m[r, :3]) for r in range(3)]
    b = l[1] if l[1] > l[2] else l[2]
    return l[0] if l[0] > b else b


def _outside_frustum(c, r, planes):      # c: [..., 3], r: [...]
    out = np.zeros(np.shape(r), dtype=bool)
    for i in range(6):
        d = _dot3(planes[i, :3], c) + planes[i, 3]
        out |= d < -r
    return out


def _projected_error(center, radius, err_mesh, scale, cam_pos, z_near, ortho):
    ws = err_mesh * scale
    if ortho:
        return ws + np.zeros(np.shape(radius), dtype=F)
    dist = _length(center - cam_pos)
    a = dist - radius
    denom = np.where(a > z_near, a, z_near)
    return ws / denom


def restate(scene, non_resident=(), active_group_scan_count=None, factor=2):
    """K1 + K2 + condition 2 of one frame (phase 1, no occlusion) under the residency rule.  Returns a dict:
    counters (instancesVisible, nodesVisited, bucketRecords, meshletsTested), touched_raw (one group per touching thread), requests_raw (one
    (group, instance, meshBuffer, viewId) per requesting thread), and the reduction: requests [n, 4] uint32, touched uint32, counts (2,)."""
    with np.errstate(all="ignore"):
        return _restate(scene, non_resident, active_group_scan_count, factor)


def _restate(scene, non_resident, active_group_scan_count, factor):
    t = SceneTables(scene)
    assert not (t.permesh[:, 2] & VERTEX_SKINNED).any(), "the restatement does not cover skinned meshes"
    mask = effective_mask(t.group_count, non_resident, None)
    active = t.group_count if active_group_scan_count is None else min(int(active_group_scan_count), t.group_count)
    touched_raw, requests_raw = [], []
    cnt = dict(instancesTested=0, instancesVisible=0, nodesVisited=0, bucketRecords=0, meshletsTested=0)
    thr, cam_pos, z_near, ortho = t.threshold, t.cam_pos, t.z_near, t.ortho
    f = max(1, min(64, int(factor)))
    f = 1 << (f.bit_length() - 1)

    def touch(group, inst, eod):
        """CLodTouchAndRequestGroupResident"""
        touched_raw.append(group)
        if group < active and not mask[group]:
            return True
        if group < active:
            requests_raw.append((group, inst, int(t.inst_u[inst, 0]), pack_view_priority(t.view_id, eod)))
        return False

    def group_sphere(g, model, scale):
        c = _mul_point(t.groups_f[g, 0:3], model)[:3]
        return c, t.groups_f[g, 3] * scale

    def child_holds(child, model, scale):
        """the refined child's boundary error is at or above the threshold"""
        c, r = group_sphere(child, model, scale)
        ce = _projected_error(c, r, t.groups_f[child, 17], scale, cam_pos, z_near, ortho)
        return not (ce < thr)

    frontier, buckets = [], []
    for ii in t.draws:
        ii = int(ii)
        cnt["instancesTested"] += 1
        model = t.obj[t.inst_u[ii, 1], 0:16].reshape(4, 4)
        c = _mul4(_mul_point(t.inst_f[ii, 4:7], model), t.view)[:3]
        r = t.inst_f[ii, 7] * _max_axis_scale(model)
        if not (np.isfinite(c).all() and np.isfinite(r)) or _outside_frustum(c, r, t.planes):
            continue
        cnt["instancesVisible"] += 1
        frontier.append((ii, int(t.md[t.offs[ii], 3])))
    levels = 0
    while frontier and levels < 64:
        nxt = []
        for ii, node_id in frontier:
            cnt["nodesVisited"] += 1
            md = t.md[t.offs[ii]]
            model = t.obj[t.inst_u[ii, 1], 0:16].reshape(4, 4)
            scale = _max_axis_scale(model)
            nu, nf = t.nodes_u[md[2] + node_id], t.nodes_f[md[2] + node_id]
            cvs = _mul4(_mul_point(nf[4:7], model), t.view)[:3]
            if _outside_frustum(cvs, nf[7] * scale, t.planes):
                continue
            if nu[0] != NODE_INTERNAL:
                owner = int(md[0] + nu[3])
                gc, gr = group_sphere(owner, model, scale)
                eod = _projected_error(gc, gr, nf[12], scale, cam_pos, z_near, ortho)
                if not (eod >= thr):
                    continue
                can_render = touch(owner, ii, eod)
                if nu[2] != 0:
                    child = int(md[0] + nu[2] - 1)
                    if child_holds(child, model, scale) and touch(child, ii, eod):
                        continue
                if not can_render:
                    continue
                seg_index = int(md[1] + nu[1])
                seg = t.segs[seg_index]
                if seg[2] == 0:
                    continue
                pe = t.pmap[md[6] + seg[3]]
                if pe[0] == 0:
                    continue
                base, remaining = int(seg[1]), int(seg[2])
                while remaining > 0:
                    chunk = min(remaining, f)
                    buckets.append((ii, owner, base, chunk, int(pe[0]), int(pe[1])))
                    base += chunk
                    remaining -= chunk
                continue
            lc = _mul_point(nf[8:11], model)[:3]
            if not (_projected_error(lc, nf[11] * scale, nf[12], scale, cam_pos, z_near, ortho) >= thr):
                continue
            for k in range(min(int(nu[2]) + 1, 8)):
                child_id = int(nu[1]) + k
                cu, cf = t.nodes_u[md[2] + child_id], t.nodes_f[md[2] + child_id]
                ccvs = _mul4(_mul_point(cf[4:7], model), t.view)[:3]
                if _outside_frustum(ccvs, cf[7] * scale, t.planes):
                    continue
                if cu[0] == NODE_INTERNAL:
                    wc = _mul_point(cf[8:11], model)[:3]
                    if _projected_error(wc, cf[11] * scale, cf[12], scale, cam_pos, z_near, ortho) < thr:
                        continue
                nxt.append((ii, child_id))
        frontier = nxt
        levels += 1
    cnt["bucketRecords"] = len(buckets)
    for ii, owner, first, count, slab, page_off in buckets:
        md = t.md[t.offs[ii]]
        model = t.obj[t.inst_u[ii, 1], 0:16].reshape(4, 4)
        scale = _max_axis_scale(model)
        page = scene.slabs[slab][page_off:]
        hdr = page[:64].view(np.uint32)
        cnt["meshletsTested"] += count
        own_eod = None
        for lm in range(first, first + count):
            if lm >= hdr[0]:
                continue
            desc = page[hdr[4] + lm * 64: hdr[4] + lm * 64 + 64]
            bounds = desc[48:64].view(np.float32)
            cvs = _mul4(_mul_point(bounds[0:3], model), t.view)[:3]
            if _outside_frustum(cvs, bounds[3] * scale, t.planes):
                continue
            refined = int(desc[32:36].view(np.uint32)[0] >> 16) - 1
            if refined >= 0:
                child = int(md[0]) + refined
                if child_holds(child, model, scale):
                    if own_eod is None:      # the own group's error over distance from bounds.error (workGraphCulling.hlsl:2550-2561)
                        oc, orad = group_sphere(owner, model, scale)
                        own_eod = _projected_error(oc, orad, t.groups_f[owner, 4], scale, cam_pos, z_near, ortho)
                    touch(child, ii, own_eod)
    return dict(counters=cnt, touched_raw=np.asarray(touched_raw, dtype=np.uint32), requests_raw=np.asarray(requests_raw, dtype=np.uint32).reshape(-1, 4),
                **reduce_stream(touched_raw, requests_raw))


def reduce_stream(touched_raw, requests_raw):
    """The raw stream -> the output contract: per requested group the highest priority, among requests of that priority the lowest instance
    (and its mesh buffer); descending priority, then ascending group.  Touched groups ascending, once each."""
    best = {}
    for g, inst, mesh, view_id in requests_raw:
        key = (-(view_id >> 16), inst)
        if g not in best or key < best[g][0]:
            best[g] = (key, (g, inst, mesh, view_id))
    recs = sorted((v[1] for v in best.values()), key=lambda r: (-(r[3] >> 16), r[0]))
    requests = np.asarray(recs, dtype=np.uint32).reshape(-1, 4)
    touched = np.unique(np.asarray(touched_raw, dtype=np.uint32))
    return dict(requests=requests, touched=touched, counts=np.asarray([len(requests), len(touched)], dtype=np.uint32))
