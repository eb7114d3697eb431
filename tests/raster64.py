"""A float64 rasteriser and a checker of visibility images against it (TEST INFRASTRUCTURE, numpy only).

Written from the reference's shader text alone -- ClusterLOD/softwareRaster.hlsl:60-89 (SWDecodeTriangle), :262-288 (the scanline clip),
:290-612 (SWRasterCluster), Include/visibilityPacking.hlsli:11-37 (the key), Include/visibleClusterPacking.hlsli:83-122 (the packed
cluster), Include/clodStructs.hlsli:48-129 (page header, meshlet descriptor, CLodLoadPagePosition) and gbuffer.hlsl:114-143 (the depth
copy) -- and from the struct layouts of include/brmi_types.h, WITHOUT reading oracle/orc_raster.cpp or brmi_raster.hip and without a
call into liboracle.so: the oracle and the kernels share an author and a reading of that shader, this module does not.

What it states: for a Scene and a list of visible clusters, every triangle is DRAWN, CULLED or UNDECIDED and every pixel centre of a
drawn triangle's rectangle is INSIDE, OUTSIDE or UNDECIDED, with the screen-linear depth the shader interpolates there.  "Undecided" is
where the fp32 path of the shader, whichever scan strategy the wave vote picks and however its products and sums are contracted, may land
on either side; the width of that band is the rounding analysis of DESIGN.md section 2 ("the float64 rasteriser"), restated next to the
code that applies it, in units of U = 2^-24 (the relative error of one rounded fp32 operation).

Out of scope: clusters of skinned meshes and of alpha-tested materials are not restated; a pixel whose key names one is an unknown
occluder (check_visibility only asks that the key names a real triangle of it).  Every page the packer writes holds FLOAT3 positions
(CLodLoadPagePosition returns zero for any other format: so does this decode, by refusing the page).
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
DEPTH_EMPTY_BITS = 0x7F7FFFFF                                     # gbuffer.hlsl:132
PAGE_SHIFT = 18                                                   # visibleClusterPacking.hlsli:7
OBJECT_FLAG_REVERSE_WINDING, VERTEX_SKINNED, MATERIAL_ALPHA_TEST = 1 << 0, 1 << 3, 1 << 13
DRAWN, CULLED, UNDECIDED = 0, 1, 2                                # triangles
INSIDE, PIXEL_UNDECIDED = 1, 2                                    # stored pairs (OUTSIDE pairs are not kept)
PAIRS_PER_CHUNK = 1 << 21


def _decode_meshlet(slab, page, lm):
    """(positions [V,3] float32, triangles [T,3]) of one meshlet of one page."""
    hdr = slab[page:page + 64].view(np.uint32)
    assert int(hdr[1]) == 1, "not a FLOAT3 page"
    assert lm < int(hdr[0])
    d = slab[page + int(hdr[4]) + lm * 64: page + int(hdr[4]) + lm * 64 + 64].view(np.uint32)
    V, T = int(d[7] >> 24) & 0xFF, int(d[8] & 0xFFFF)
    p0 = page + int(hdr[6]) + int(d[0])
    pos = slab[p0:p0 + V * 12].view(np.float32).reshape(V, 3)
    t0 = page + int(hdr[12]) + int(d[2])                          # a byte stream: SWDecodeTriangle's word loads and shifts pick bytes 3t, 3t+1, 3t+2
    tri = slab[t0:t0 + 3 * T].reshape(T, 3).astype(np.int64)
    assert T == 0 or int(tri.max()) < V
    return pos, tri


class Raster64:
    """The float64 statement about `clusters` ([N,4] uint32, packed visible clusters) of `scene`; see the module docstring."""

    def __init__(self, scene, clusters):
        self.scene, self.W, self.H = scene, int(scene.width), int(scene.height)
        self.clusters = np.ascontiguousarray(clusters, dtype=np.uint32).reshape(-1, 4)
        self._decode()
        self._vertices()
        self._triangles()
        self._pixels()

    # -- geometry of the listed clusters ----------------------------------------------------------------------------------------------
    def _decode(self):
        sc, cl = self.scene, self.clusters
        inst = sc.arrays["perMeshInstance"].view(np.uint32).reshape(-1, 8)
        mesh = sc.arrays["perMesh"].view(np.uint32).reshape(-1, 16)
        obj = sc.arrays["perObject"].view(np.uint32).reshape(-1, 52)
        objf = sc.arrays["perObject"].view(np.float32).reshape(-1, 52)
        mat = sc.arrays["materials"].view(np.uint32).reshape(-1, 69)
        n = len(cl)
        self.view = (cl[:, 0] & 0xFF).astype(np.int64)
        self.instance = (cl[:, 0] >> 8).astype(np.int64)
        self.mesh_index = inst[self.instance, 0].astype(np.int64) if n else np.zeros(0, np.int64)
        o = inst[self.instance, 1].astype(np.int64) if n else np.zeros(0, np.int64)
        self.model = objf[o, :16].reshape(-1, 4, 4).astype(np.float64)
        self.reverse = (obj[o, 49] & OBJECT_FLAG_REVERSE_WINDING) != 0
        skinned = (mesh[self.mesh_index, 2] & VERTEX_SKINNED) != 0
        alpha = (mat[mesh[self.mesh_index, 0], 0] & MATERIAL_ALPHA_TEST) != 0
        self.skipped = skinned | alpha
        self.tri_count = np.zeros(n, dtype=np.int64)
        cache, vpos, vcl, tris, tcl, tti, vbase = {}, [], [], [], [], [], 0
        for c in range(n):
            key = (int((cl[c, 2] >> 2) & 0xFFFFF), int(cl[c, 2] >> 22) << PAGE_SHIFT, int(cl[c, 1] & 0x3FFF))
            if key not in cache:
                cache[key] = _decode_meshlet(sc.slabs[key[0]], key[1], key[2])
            pos, tri = cache[key]
            self.tri_count[c] = len(tri)
            if self.skipped[c] or not len(tri):
                continue
            vpos.append(pos); vcl.append(np.full(len(pos), c)); tris.append(tri + vbase); tcl.append(np.full(len(tri), c)); tti.append(np.arange(len(tri)))
            vbase += len(pos)
        cat = lambda parts, dt, shape: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dt)
        self.vpos, self.vcl = cat(vpos, np.float64, (0, 3)), cat(vcl, np.int64, (0,))
        self.tris, self.tcl, self.tti = cat(tris, np.int64, (0, 3)), cat(tcl, np.int64, (0,)), cat(tti, np.int64, (0,))

    # -- softwareRaster.hlsl:336-375, per vertex ----------------------------------------------------------------------------------------
    def _vertices(self):
        sc = self.scene
        cam = sc.arrays["cullingCameras"].view(np.float32).reshape(-1, 76).astype(np.float64)
        ri = sc.arrays["viewRasterInfo"].view(np.uint32).reshape(-1, 12).astype(np.int64)
        vp, vz = cam[self.view, 24:40].reshape(-1, 4, 4), cam[self.view, 40:44]
        self.scissor = ri[self.view, 3:7] if len(self.view) else np.zeros((0, 4), np.int64)      # minX, minY, maxX, maxY
        # modelViewProjection = mul(model, viewProjection); modelViewZ = mul(model, viewZ): entries are 4-term dot products.  A 4-term fp32 dot
        # product (4 products, 3 sums, fused or not) is off by at most 4 U times the sum of the |products|.
        mvp, mvp_abs = self.model @ vp, np.abs(self.model) @ np.abs(vp)
        mvz, mvz_abs = np.einsum("cik,ck->ci", self.model, vz), np.einsum("cik,ck->ci", np.abs(self.model), np.abs(vz))
        p4 = np.concatenate([self.vpos, np.ones((len(self.vpos), 1))], 1)
        c = self.vcl
        clip = np.einsum("vi,vij->vj", p4, mvp[c])
        # clipPos = mul(localPos4, mvp): another 4-term dot product over entries that already carry 4 U: (4 + 4) U sum |p_i| (|model| |vp|)_ij
        e_clip = 8 * U * np.einsum("vi,vij->vj", np.abs(p4), mvp_abs[c])
        self.vdepth = -np.einsum("vi,vi->v", p4, mvz[c])                                         # gs_linearDepth = -dot(localPos4, modelViewZ)
        self.e_vdepth = 8 * U * np.einsum("vi,vi->v", np.abs(p4), mvz_abs[c])
        with np.errstate(all="ignore"):
            w = clip[:, 3]
            rel_w = e_clip[:, 3] / np.abs(w)
            rel_inv = np.where(rel_w < 0.5, rel_w / (1 - rel_w), np.inf) + U                    # invW = 1 / w: the error of w, one rounding
            inv = 1.0 / w
            ndc = clip[:, :2] * inv[:, None]                                                     # one product
            e_ndc = e_clip[:, :2] * np.abs(inv)[:, None] * (1 + rel_inv)[:, None] + np.abs(ndc) * (rel_inv + U)[:, None]
            sz = self.scissor[c]
            vis_w, vis_h = (sz[:, 2] - sz[:, 0]).astype(np.float64), (sz[:, 3] - sz[:, 1]).astype(np.float64)
            ax, ay = ndc[:, 0] + 1.0, 1.0 - ndc[:, 1]                                            # one sum each
            e_ax, e_ay = e_ndc[:, 0] + U * np.abs(ax), e_ndc[:, 1] + U * np.abs(ay)
            bx, by = ax * 0.5 * vis_w, ay * 0.5 * vis_h                                          # * 0.5 is exact; one product
            e_bx, e_by = e_ax * 0.5 * vis_w + U * np.abs(bx), e_ay * 0.5 * vis_h + U * np.abs(by)
            sx, sy = bx + sz[:, 0], by + sz[:, 1]                                                # one sum
            self.vscreen = np.stack([sx, sy], 1)
            self.e_vscreen = np.maximum(e_bx + U * np.abs(sx), e_by + U * np.abs(sy))

    # -- softwareRaster.hlsl:416-470, per triangle ---------------------------------------------------------------------------------------
    def _triangles(self):
        t = self.tris.copy()
        rev = self.reverse[self.tcl]
        t[rev, 1], t[rev, 2] = self.tris[rev, 2], self.tris[rev, 1]                             # if (reverseWinding) swap(tri.y, tri.z)
        self.wound = t
        d, ed = self.vdepth[t], self.e_vdepth[t]
        self.d, self.ed = d, ed
        behind = (d < -ed).any(1)                                                                # depth <= 0 on any vertex: dropped whole
        in_front = (d > ed).all(1)
        with np.errstate(all="ignore"):
            s = self.vscreen[t]                                                                  # [T,3,2]
            es = self.e_vscreen[t].max(1)
            e01, e02, e12, e20 = s[:, 1] - s[:, 0], s[:, 2] - s[:, 0], s[:, 2] - s[:, 1], s[:, 0] - s[:, 2]
            longest = np.max(np.abs(np.concatenate([e01, e02, e12, e20], 1)), 1)
            ee = 2 * es + U * longest                                                            # an edge component: two screen errors, one difference
            area = e01[:, 0] * e02[:, 1] - e01[:, 1] * e02[:, 0]
            q = np.abs(e01[:, 0] * e02[:, 1]) + np.abs(e01[:, 1] * e02[:, 0])
            e_area = ee * np.abs(np.concatenate([e01, e02], 1)).sum(1) + 2 * ee * ee + 2 * U * q  # two products and a difference: <= 2 U q
            rel_area = e_area / np.abs(area)
        ok = in_front & np.isfinite(area) & np.isfinite(e_area)
        state = np.full(len(t), UNDECIDED)
        state[behind] = CULLED
        state[ok & (area > e_area)] = CULLED                                                     # else if (twiceArea >= 0) continue
        state[ok & (area < -e_area) & (rel_area <= 0.5)] = DRAWN
        self.state, self.s, self.es, self.ee, self.area, self.rel_area = state, s, es, ee, area, rel_area
        self.edges = (e12, e20)
        # a triangle whose vertex depth is undecided has no bounded rectangle (the screen position runs away as w -> 0): it is reported and
        # never enumerated; one whose area sign is undecided has a rectangle, and every pixel of it is an undecided pair
        self.unbounded = (state == UNDECIDED) & ~ok
        # minPx = floor(min), maxPx = floor(max), clamped to the scissor and to the image; the fp32 rectangle may start or end one pixel
        # beside the float64 one where a coordinate is within its error of an integer, so both candidates are walked
        sz = self.scissor[self.tcl]
        with np.errstate(all="ignore"):
            lo = np.floor(np.nan_to_num(s.min(1) - es[:, None], nan=0.0, posinf=1e9, neginf=-1e9)).astype(np.int64)
            hi = np.floor(np.nan_to_num(s.max(1) + es[:, None], nan=0.0, posinf=1e9, neginf=-1e9)).astype(np.int64)
        lo = np.maximum(np.maximum(lo, sz[:, 0:2]), 0)
        hi = np.minimum(np.minimum(hi, sz[:, 2:4] - 1), np.array([self.W - 1, self.H - 1]))
        live = (state != CULLED) & ~self.unbounded & (lo <= hi).all(1)
        self.lo, self.hi, self.live = lo, hi, live

    # -- softwareRaster.hlsl:484-610, per pixel centre of the rectangle ------------------------------------------------------------------
    def _pixels(self):
        idx = np.flatnonzero(self.live)
        wh = self.hi[idx] - self.lo[idx] + 1
        counts = wh[:, 0] * wh[:, 1]
        keep = {k: [] for k in ("tri", "pix", "verdict", "depth", "tol")}
        self.pairs_walked = int(counts.sum())
        # the largest uncertainty under which a pair was still called INSIDE (information).  It is large on thin triangles: there kappa, the
        # relative error of 1 / twiceArea, is up to 1 and enters b2's bound as kappa |b0 + b1|; such a pair is INSIDE because b2 exceeds even that
        self.largest_inside_bound = 0.0
        start = 0
        while start < len(idx):
            stop = start + max(1, int(np.searchsorted(np.cumsum(counts[start:]), PAIRS_PER_CHUNK, side="right")))
            self._chunk(idx[start:stop], wh[start:stop], counts[start:stop], keep)
            start = stop
        self.p_tri = np.concatenate(keep["tri"]) if keep["tri"] else np.zeros(0, np.int64)
        self.p_pix = np.concatenate(keep["pix"]) if keep["pix"] else np.zeros(0, np.int64)
        self.p_verdict = np.concatenate(keep["verdict"]) if keep["verdict"] else np.zeros(0, np.int64)
        self.p_depth = np.concatenate(keep["depth"]) if keep["depth"] else np.zeros(0)
        self.p_tol = np.concatenate(keep["tol"]) if keep["tol"] else np.zeros(0)
        # the nearest a pixel's key may be beaten by: min over drawn + inside pairs of depth + tolerance (inf: nothing certainly covers it)
        self.nearest = np.full(self.W * self.H, np.inf)
        sure = self.p_verdict == INSIDE
        np.minimum.at(self.nearest, self.p_pix[sure], (self.p_depth + self.p_tol)[sure])
        # shares (float64 side alone): undecided pairs over inside pairs; pixels whose winner an undecided pair could change over covered pixels
        und = ~sure
        could_win = und & (np.where(self.state[self.p_tri] == DRAWN, self.p_depth - self.p_tol, -np.inf) <= self.nearest[self.p_pix])
        covered = np.zeros(self.W * self.H, bool); covered[self.p_pix] = True
        shaky = np.zeros(self.W * self.H, bool); shaky[self.p_pix[could_win]] = True
        self.stats = dict(clusters=len(self.clusters), skipped_clusters=int(self.skipped.sum()), triangles=len(self.tris),
                          drawn=int((self.state == DRAWN).sum()), culled=int((self.state == CULLED).sum()), undecided_triangles=int((self.state == UNDECIDED).sum()),
                          unbounded_triangles=int(self.unbounded.sum()), pairs_walked=self.pairs_walked,
                          inside_pairs=int(sure.sum()), undecided_pairs=int(und.sum()), covered_pixels=int(covered.sum()), shaky_pixels=int(shaky.sum()))
        self.stats["undecided_pair_share"] = self.stats["undecided_pairs"] / max(self.stats["inside_pairs"], 1)
        self.stats["shaky_pixel_share"] = self.stats["shaky_pixels"] / max(self.stats["covered_pixels"], 1)

    def _chunk(self, idx, wh, counts, keep):
        n = int(counts.sum())
        rep = np.repeat(np.arange(len(idx)), counts)
        local = np.arange(n) - np.repeat(np.cumsum(counts) - counts, counts)
        wrep = wh[rep, 0]
        i, j = local % wrep, local // wrep                                                       # steps from the rectangle's origin
        lo, s, area = self.lo[idx], self.s[idx], self.area[idx]
        e12, e20 = self.edges[0][idx], self.edges[1][idx]
        es, ee = self.es[idx], self.ee[idx]
        decided = self.state[idx] == DRAWN
        with np.errstate(all="ignore"):
            inv = -1.0 / area                                                                    # invTwiceArea = -1 / twiceArea
            rel = np.where(decided, self.rel_area[idx], 0.5)
            k = rel / (1 - rel) + U                                                              # relative error of invTwiceArea: the area's, then one division
            ox, oy = lo[:, 0] + 0.5, lo[:, 1] + 0.5                                              # exact in fp32
            rows, steps_x, steps_y, e_rows, e_step = [], [], [], [], ee / np.abs(area)
            for a, e in ((s[:, 1], e12), (s[:, 2], e20)):
                dx, dy = ox - a[:, 0], oy - a[:, 1]
                e_d = es + U * np.maximum(np.abs(dx), np.abs(dy))                                # origin - vertex: the screen error, one difference
                num = dx * e[:, 1] - dy * e[:, 0]
                e_num = (np.abs(dx) + np.abs(dy)) * ee + np.abs(e).sum(1) * e_d + 2 * ee * e_d + 2 * U * (np.abs(dx * e[:, 1]) + np.abs(dy * e[:, 0]))
                rows.append(num * inv); e_rows.append(e_num / np.abs(area))
                steps_x.append(e[:, 1] * inv); steps_y.append(-e[:, 0] * inv)                    # dx_b = e.y * inv, dy_b = -e.x * inv
            # the largest |barycentric| any partial sum of the walk can reach: the corners of the rectangle, one pixel wider each way
            cx = np.stack([-1 * np.ones(len(idx)), wh[:, 0].astype(float)] * 2, 1)
            cy = np.stack([-1 * np.ones(len(idx))] * 2 + [wh[:, 1].astype(float)] * 2, 1)
            corner = [rows[m][:, None] + cx * steps_x[m][:, None] + cy * steps_y[m][:, None] for m in (0, 1)]
            corner.append(1.0 - corner[0] - corner[1])
            bmax = [np.abs(cn).max(1) for cn in corner]
            px, py = lo[rep, 0] + i, lo[rep, 1] + j
            b, e_sign = [], []
            for m, a, e in ((0, s[:, 1], e12), (1, s[:, 2], e20)):
                b.append(((px + 0.5 - a[rep, 0]) * e[rep, 1] - (py + 0.5 - a[rep, 1]) * e[rep, 0]) * inv[rep])
                # b0 and b1 at a pixel are (numerator at the origin + i edge.y - j edge.x) * invTwiceArea: the error of invTwiceArea is ONE factor common to
                # the row value and to both steps, so it scales b0 and b1 and cannot change their signs.  What can: the numerator's and the edges' errors,
                # and the roundings of the walk, each at a magnitude <= bmax: i + j sums; the row product and the step products (i |dx_b| + j |dy_b| <= 4 bmax):
                # 5; the scanline walk's start (one product, one sum): 2; an origin one pixel beside this one: 2; the scanline clip's own division
                # (ceil(-value / step), :276-280, moves a decision only where |value + k step| <= U |value|): 1.
                e_sign.append(e_rows[m][rep] + (i + j) * e_step[rep] + (i + j + 10) * U * bmax[m][rep])
            b.append(1.0 - b[0] - b[1])
            # b2 = 1 - b0 - b1 (in the clip: 1 - s0 - s1 stepped by -(dx0 + dx1)): here the common factor does count, against the exact 1
            e_sign.append(e_sign[0] + e_sign[1] + k[rep] * np.abs(b[0] + b[1]) + U * (1 + bmax[0] + 4 * bmax[2])[rep])
            b, e_sign = np.stack(b, 1), np.stack(e_sign, 1)
            # the values themselves, for the depth: b0 and b1 also carry the common factor
            e_value = e_sign + np.stack([k[rep] * np.abs(b[:, 0]), k[rep] * np.abs(b[:, 1]), np.zeros(n)], 1)
            inside = (b > e_sign).all(1) & decided[rep]
            outside = (b < -e_sign).any(1) & decided[rep]
            d, ed = self.d[idx][rep], self.ed[idx][rep]
            depth = (b * d).sum(1)                                                               # b0 * depth0 + b1 * depth1 + b2 * depth2
            e_depth = (np.abs(b) * ed + np.abs(d) * e_value + e_value * ed).sum(1) + 3 * U * np.abs(b * d).sum(1)
            tol = e_depth + 2 * U * np.abs(depth)                                                # + the bit the key drops (PackVisKey: asuint(depth) >> 1)
        kept = ~outside
        if inside.any():
            self.largest_inside_bound = max(self.largest_inside_bound, float(e_sign[inside].max()))
        keep["tri"].append(idx[rep][kept])
        keep["pix"].append((py * self.W + px)[kept])
        keep["verdict"].append(np.where(inside, INSIDE, PIXEL_UNDECIDED)[kept])
        keep["depth"].append(np.nan_to_num(depth[kept], nan=0.0))
        keep["tol"].append(np.where(decided[rep], np.nan_to_num(tol, nan=np.inf), np.inf)[kept])

    # -- bookkeeping --------------------------------------------------------------------------------------------------------------------
    def triangle_positions(self, mesh_index=None):
        """The triangles the restatement walks, as model-space vertex triples in the stream's order (before the winding swap)."""
        sel = np.ones(len(self.tris), bool) if mesh_index is None else self.mesh_index[self.tcl] == mesh_index
        return self.vpos[self.tris[sel]].astype(np.float32)

    def restricted_to_rows(self, y0, y1):
        """A copy that speaks of rows [y0, y1) only: what a pass that owns those rows must have drawn there."""
        import copy
        r = copy.copy(self)
        rows = self.p_pix // self.W
        keep = (rows >= y0) & (rows < y1)
        for name in ("p_tri", "p_pix", "p_verdict", "p_depth", "p_tol"):
            setattr(r, name, getattr(self, name)[keep])
        r.nearest = self.nearest.copy()
        r.nearest[: y0 * self.W] = np.inf
        r.nearest[y1 * self.W:] = np.inf
        return r

    def family_coverage(self, names_by_mesh):
        """{name: (decided inside pairs, decided outside pairs inside the rectangles)} per mesh name."""
        out = {}
        inside_per_tri = np.bincount(self.p_tri[self.p_verdict == INSIDE], minlength=len(self.tris))
        kept_per_tri = np.bincount(self.p_tri, minlength=len(self.tris))
        wh = np.where(self.live[:, None], self.hi - self.lo + 1, 0)
        walked = wh[:, 0] * wh[:, 1]
        mesh_of_tri = self.mesh_index[self.tcl]
        for m, name in names_by_mesh.items():
            sel = (mesh_of_tri == m) & (self.state == DRAWN)
            a, b = out.get(name, (0, 0))
            out[name] = (a + int(inside_per_tri[sel].sum()), b + int((walked - kept_per_tri)[sel].sum()))
        return out


def unpack(vis):
    """(empty, cluster, triangle, depth as float64, depth bits with the low bit clear) of a visibility image: UnpackVisKey."""
    empty = vis == EMPTY
    tri = (vis & np.uint64(0x7F)).astype(np.int64)
    cl = ((vis >> np.uint64(7)) & np.uint64(0x3FFFFFF)).astype(np.int64)
    bits = ((vis >> np.uint64(33)) << np.uint64(1)).astype(np.uint32)
    return empty, cl, tri, bits.view(np.float32).astype(np.float64), bits


def check_visibility(r, vis, depth_plane=None, what=""):
    """DESIGN.md section 2's assertions about a visibility image (the oracle's or the GPU's) of r's cluster list.  Returns measured figures."""
    W, H = r.W, r.H
    assert vis.shape == (H, W)
    empty, kcl, ktri, kdepth, kbits = (a.ravel() for a in unpack(np.ascontiguousarray(vis)))
    full = ~empty

    def where(mask):
        p = np.flatnonzero(mask)[:5]
        return ", ".join(f"({int(q % W)}, {int(q // W)}): cluster {int(kcl[q])} (mesh {int(r.mesh_index[min(kcl[q], len(r.mesh_index) - 1)]) if len(r.mesh_index) else -1}) triangle {int(ktri[q])} depth {kdepth[q]!r}" for q in p)

    # every key names a triangle of a listed cluster
    bad = full & (kcl >= len(r.clusters))
    assert not bad.any(), f"{what}: {int(bad.sum())} keys name a cluster beyond the list: {where(bad)}"
    bad = full & (ktri >= r.tri_count[np.where(full, kcl, 0)] if len(r.clusters) else full)
    assert not bad.any(), f"{what}: {int(bad.sum())} keys name a triangle beyond their cluster's count: {where(bad)}"
    opaque = full & ~(r.skipped[np.where(full, kcl, 0)] if len(r.clusters) else full)       # keys of restated clusters; the others are unknown occluders
    # the named triangle's own pair: it must exist among the pairs that are not OUTSIDE, of a triangle that is not CULLED
    named = opaque[r.p_pix] & (kcl[r.p_pix] == r.tcl[r.p_tri]) & (ktri[r.p_pix] == r.tti[r.p_tri])
    found = np.zeros(W * H, bool); found[r.p_pix[named]] = True
    tri_of_key = np.full(W * H, -1, np.int64)
    if len(r.tris):
        first = np.full(len(r.clusters) + 1, 0, np.int64)
        np.add.at(first, r.tcl + 1, 1); first = np.cumsum(first)                                # triangles are stored cluster by cluster, in stream order
        tri_of_key[opaque] = first[kcl[opaque]] + ktri[opaque]
    in_unbounded = np.zeros(W * H, bool)
    in_unbounded[opaque] = r.unbounded[tri_of_key[opaque]]
    stray = opaque & ~found & ~in_unbounded
    if stray.any():
        st = r.state[tri_of_key[stray]]
        raise AssertionError(f"{what}: {int(stray.sum())} stray writes: the named triangle is culled ({int((st == CULLED).sum())}) or the pixel centre is outside it "
                             f"({int((st != CULLED).sum())}): {where(stray)}")
    # depth of the named triangle
    nd, nt, npx = r.p_depth[named], r.p_tol[named], r.p_pix[named]
    with np.errstate(invalid="ignore"):
        off = np.abs(kdepth[npx] - nd)
        bad_depth = off > nt
    if bad_depth.any():
        m = np.zeros(W * H, bool); m[npx[bad_depth]] = True
        k = int(np.argmax(np.where(bad_depth, off / nt, 0)))
        raise AssertionError(f"{what}: {int(bad_depth.sum())} keys hold a depth beyond the bound of their own triangle (worst: {off[k]!r} against a bound of {nt[k]!r}, float64 depth {nd[k]!r}): {where(m)}")
    # nothing nearer was missed; an empty pixel has no drawn + inside triangle
    missed = empty & np.isfinite(r.nearest)
    assert not missed.any(), f"{what}: {int(missed.sum())} empty pixels are inside a drawn triangle, e.g. pixels {[(int(q % W), int(q // W)) for q in np.flatnonzero(missed)[:5]]}"
    nearer = opaque & (kdepth > r.nearest)
    assert not nearer.any(), f"{what}: {int(nearer.sum())} keys are farther than a triangle that certainly covers the pixel: {where(nearer)}"
    # the winner is the nearest: its own float64 depth, less its bound, does not exceed the nearest certain candidate's depth plus that one's bound
    lose = (nd - nt) > r.nearest[npx]
    if lose.any():
        m = np.zeros(W * H, bool); m[npx[lose]] = True
        raise AssertionError(f"{what}: {int(lose.sum())} pixels are won by a triangle that is not the nearest: {where(m)}")
    if depth_plane is not None:
        bits = np.ascontiguousarray(depth_plane).view(np.uint32).ravel()
        assert np.array_equal(bits[full], kbits[full]), f"{what}: the depth plane is not the key's depth with the low bit cleared"
        assert (bits[empty] == DEPTH_EMPTY_BITS).all(), f"{what}: the depth plane of an empty pixel is not the empty value"
    decided = np.isfinite(nt) & (nt > 0)
    return dict(covered=int(full.sum()), checked=int(named.sum()), unknown_occluder_pixels=int((full & ~opaque).sum()),
                worst_depth_over_bound=float((off[decided] / nt[decided]).max()) if decided.any() else 0.0)


def caps_hold(r, cap, what=""):
    """The caps that keep the checker from hiding a failure behind 'undecided' (float64 side alone, before any image is looked at)."""
    s = r.stats
    print(f"[raster64] {what}: {s['clusters']} clusters ({s['skipped_clusters']} skipped), {s['triangles']} triangles: {s['drawn']} drawn, {s['culled']} culled, "
          f"{s['undecided_triangles']} undecided ({s['unbounded_triangles']} without a rectangle); {s['inside_pairs']} inside pairs, {s['undecided_pairs']} undecided "
          f"({100 * s['undecided_pair_share']:.3f} %); {s['shaky_pixels']} of {s['covered_pixels']} covered pixels rest on an undecided pair ({100 * s['shaky_pixel_share']:.3f} %)")
    assert s["inside_pairs"] > 0
    assert s["undecided_pair_share"] <= cap, f"{what}: undecided pairs are {100 * s['undecided_pair_share']:.2f} % of the inside pairs (cap {100 * cap:.0f} %)"
    assert s["shaky_pixel_share"] <= cap, f"{what}: {100 * s['shaky_pixel_share']:.2f} % of the covered pixels rest on an undecided pair (cap {100 * cap:.0f} %)"


# -- exact arithmetic on the fp32 screen positions (the restatement checks itself) --------------------------------------------------------
def exact_verdicts(r, tri):
    """Triangle `tri` once more in rationals, from its float64 screen positions rounded to fp32: (sign of twiceArea, {pixel: inside}) for
    every pixel centre of its rectangle.  Inside = all three edge functions, divided by -twiceArea, are >= 0."""
    s = [[Fraction(float(np.float32(v))) for v in p] for p in r.s[tri]]
    e01, e02 = (s[1][0] - s[0][0], s[1][1] - s[0][1]), (s[2][0] - s[0][0], s[2][1] - s[0][1])
    area = e01[0] * e02[1] - e01[1] * e02[0]
    sign = (area > 0) - (area < 0)
    pixels = {}
    if sign < 0:
        e12, e20 = (s[2][0] - s[1][0], s[2][1] - s[1][1]), (s[0][0] - s[2][0], s[0][1] - s[2][1])
        for py in range(int(r.lo[tri, 1]), int(r.hi[tri, 1]) + 1):
            for px in range(int(r.lo[tri, 0]), int(r.hi[tri, 0]) + 1):
                cx, cy = Fraction(2 * px + 1, 2), Fraction(2 * py + 1, 2)
                n0 = (cx - s[1][0]) * e12[1] - (cy - s[1][1]) * e12[0]
                n1 = (cx - s[2][0]) * e20[1] - (cy - s[2][1]) * e20[0]
                b0, b1 = -n0 / area, -n1 / area
                pixels[py * r.W + px] = b0 >= 0 and b1 >= 0 and 1 - b0 - b1 >= 0
    return sign, pixels


# -- the adversarial scene ---------------------------------------------------------------------------------------------------------------
ADVERSARIAL_SIZE = (700, 420)              # no multiple of 8, 16, 32 or 64 either way: no bin, tile or band edge falls on the image's
ADVERSARIAL_SPLIT = 208                    # the row where the band-split runs cut the image (through family 10's stack)
_EYE_Z, _FOV = 4.0, 90.0


def adversarial_scene(size=ADVERSARIAL_SIZE, scissor=None, **kw):
    """(scene, {mesh index: family name}, {mesh index: intended triangles [T,3,3] float32}).  Camera on the z axis looking down -z, every
    family on planes z = const, so a target screen position inverts to a model position in two lines (aim below); positions are FLOAT3.
    `size`: the interleaved-stripe partition needs a height that is a multiple of 32, which the default is not on purpose.
    `scissor` = (minX, minY, maxX, maxY): written into the view's raster info.  The shader maps ndc onto the scissor rectangle, so the whole
    picture shrinks into it: the aimed positions move off the pixel centres, and the triangles of family 4 that straddle the image's sides
    straddle the scissor's sides instead."""
    from basicrenderer_amd import Scene as RawScene
    W, H = size
    h = 1.0 / np.tan(np.radians(_FOV) / 2)
    w = h / (W / H)

    def aim(sx, sy, d):
        """the model position whose screen position is (sx, sy) at view depth d (before its rounding to fp32: <= 2^-24 of the offset from the centre)"""
        return [(sx / (W / 2) - 1.0) * d / w, (1.0 - sy / (H / 2)) * d / h, _EYE_Z - d]

    meshes, names, intended = [], {}, {}

    def mesh(name, tris, facing="front"):
        """tris: lists of three (sx, sy, d), wound front-facing (twiceArea < 0 on screen, y down) unless told otherwise, or of three model positions ('raw', x, y, z), kept as given"""
        P = []
        for t in tris:
            pts = [list(v[1:]) if v[0] == "raw" else aim(*v) for v in t]
            if facing != "keep" and all(v[0] != "raw" for v in t):
                area = (t[1][0] - t[0][0]) * (t[2][1] - t[0][1]) - (t[1][1] - t[0][1]) * (t[2][0] - t[0][0])
                if (area > 0) == (facing == "front"):
                    pts[1], pts[2] = pts[2], pts[1]
            P.append(pts)
        P = np.array(P, dtype=np.float32)
        assert len(P) <= 42, "one meshlet: at most 126 vertices"
        names[len(meshes)] = name
        intended[len(meshes)] = P
        meshes.append(dict(positions=P.reshape(-1, 3), indices=np.arange(3 * len(P), dtype=np.uint32), material=len(meshes) % 3))
        return len(meshes) - 1

    # 1. vertices on pixel centres, on pixel corners, shared edges through rows and diagonals of pixel centres
    d = 2.0
    f1 = mesh("1 centres and corners", [
        [(12.5, 12.5, d), (12.5, 30.5, d), (30.5, 12.5, d)], [(30.5, 30.5, d), (30.5, 12.5, d), (12.5, 30.5, d)],
        [(40, 12, d), (40, 30, d), (58, 12, d)], [(58, 30, d), (58, 12, d), (40, 30, d)],
        [(62, 20.5, d), (88, 20.5, d), (75, 10.2, d)], [(62, 20.5, d), (75, 33.7, d), (88, 20.5, d)],
        [(12.5, 40.5, d), (12.5, 55.5, d), (40.5, 40.5, d)], [(70.5, 40, d), (70.5, 58, d), (90, 49.5, d)]])
    # 2. needles: a fan from one apex and a strip between two long lines, 1/50 to 1/5000 of a pixel wide at several angles
    d = 3.0
    fan = []
    # (a needle this long is decided down to about 1/50 of a pixel: the thinner ones are kept short or shallow, their whole rectangle is undecided)
    for ang, length, width in ((3.0, 380.0, 1 / 50), (11.0, 330.0, 1 / 50), (19.0, 300.0, 1 / 50), (27.0, 260.0, 1 / 20), (2.0, 200.0, 1 / 500), (1.5, 200.0, 1 / 5000), (45.0, 30.0, 1 / 500), (50.0, 30.0, 1 / 5000)):
        c, s_ = np.cos(np.radians(ang)), np.sin(np.radians(ang))
        fan.append([(120.3, 15.7, d), (120.3 + length * c + width * s_ / 2, 15.7 + length * s_ - width * c / 2, d), (120.3 + length * c - width * s_ / 2, 15.7 + length * s_ + width * c / 2, d)])
    strip = []
    for k in range(8):
        a0, b0, a1, b1 = (130.2, 150.1 + k / 50), (480.7, 175.3 + k / 50), (130.2, 150.1 + (k + 1) / 50), (480.7, 175.3 + (k + 1) / 50)
        strip += [[a0 + (d,), b0 + (d,), a1 + (d,)], [a1 + (d,), b0 + (d,), b1 + (d,)]]
    wedges = [[(140.3, 120.2, d), (440.9, 128.7, d), (140.1, 126.9, d)], [(150.3, 140.2, d), (150.9, 100.7, d), (153.1, 141.9, d)]]      # thin but decided: 6 and 3 pixels at the wide end
    f2 = mesh("2 needle fan", fan)
    f2s = mesh("2 needle strip", strip)
    f2w = mesh("2 wedges", wedges)
    # 3. sub-pixel triangles that do and do not contain a pixel centre
    d = 2.5
    tiny = []
    for gy in range(5):
        for gx in range(8):
            cx, cy = 14 + 10 * gx + (0.5 if (gx + gy) % 2 == 0 else 0.03), 75 + 10 * gy + (0.5 if (gx + gy) % 2 == 0 else 0.97)
            r_ = 0.12 + 0.02 * gx
            tiny.append([(cx, cy - r_, d), (cx - r_, cy + r_, d), (cx + r_, cy + r_, d)])
    f3 = mesh("3 sub-pixel", tiny)
    # 4. larger than the screen, clamped on each side (the scissor is the image)
    f4 = mesh("4 clamped", [
        [(-300, -100, 8.0), (900, -100, 8.0), (-300, 500, 8.0)],
        [(-20.3, 100.2, 7.0), (8.4, 90.1, 7.0), (8.4, 112.6, 7.0)], [(350.2, -15.3, 7.0), (340.1, 6.4, 7.0), (362.7, 6.4, 7.0)],
        [(720.3, 200.2, 7.0), (692.4, 190.1, 7.0), (692.4, 212.6, 7.0)], [(600.2, 440.3, 7.0), (590.1, 412.4, 7.0), (612.7, 412.4, 7.0)],
        [(690.2, 410.3, 7.0), (705.1, 400.4, 7.0), (704.7, 431.4, 7.0)], [(-3.2, -4.3, 7.0), (9.1, 2.4, 7.0), (2.7, 11.4, 7.0)]])
    # 5. rectangles 1 to 8 pixels wide: a wave of narrow ones, a wave of wide ones, one wide one among narrow ones (WaveActiveAnyTrue(rectWidth > 4))
    d = 2.25

    def row(widths, x0, y0):
        out, x = [], x0
        for wd in widths:
            out.append([(x + 0.1, y0 + 0.2, d), (x + wd - 0.1, y0 + 0.3, d), (x + 0.3, y0 + 8.6, d)])
            x += wd + 1
        return out
    f5n = mesh("5 narrow wave", row([1 + k % 4 for k in range(21)], 10, 190) + row([4 - k % 4 for k in range(21)], 10, 202))
    f5w = mesh("5 wide wave", row([5 + k % 4 for k in range(21)], 10, 214) + row([8 - k % 4 for k in range(21)], 10, 226))
    f5m = mesh("5 one wide among narrow", row([1 + k % 4 for k in range(21)], 10, 238) + row([4 - k % 4 if k != 13 else 7 for k in range(21)], 10, 250))
    # 6. vertices behind the eye and at view depth 0 (dropped whole, never clipped), a large triangle just in front of the eye
    x0, y0, _ = aim(40, 370, 2.0); x1, y1, _ = aim(90, 360, 2.0); x2, y2, _ = aim(70, 400, 2.0)
    near = 0.03125
    f6 = mesh("6 behind the eye", [
        [("raw", x0, y0, _EYE_Z - 2.0), ("raw", x1, y1, _EYE_Z - 2.0), ("raw", x2, y2, _EYE_Z + 1.0)],
        [("raw", x0, y0, _EYE_Z + 0.5), ("raw", x1, y1, _EYE_Z - 2.0), ("raw", x2, y2, _EYE_Z + 1.0)],
        [("raw", x0, y0, _EYE_Z - 2.0), ("raw", x1, y1, _EYE_Z), ("raw", x2, y2, _EYE_Z - 2.0)],
        [(100.2, 352.3, near), (330.4, 356.1, near), (180.7, 415.2, near)],
        [(110.2, 362.3, 2.0), (150.4, 366.1, 2.0), (120.7, 405.2, 2.0)]])
    # 7. exactly and nearly degenerate, back-facing
    d = 2.0
    f7 = mesh("7 degenerate", [
        [(20, 290, d), (40, 300, d), (60, 310, d)], [(20, 300, d), (20, 300, d), (50, 312, d)],
        [(110.2, 290.3, d), (130.2, 300.3, d), (150.2, 310.3 + 1e-6, d)], [(110.2, 300.3, d), (130.2, 310.3, d), (150.2, 320.3 - 1e-6, d)]], facing="keep")
    f7b = mesh("7 back-facing", [[(30.3, 315.2, d), (60.1, 318.4, d), (38.2, 338.9, d)], [(70.3, 312.2, d), (95.1, 300.4, d), (98.2, 338.9, d)]], facing="back")
    f7f = mesh("7 front-facing beside them", [[(130.3, 325.2, d), (160.1, 328.4, d), (138.2, 345.9, d)]])
    # 8. coplanar overlapping triangles; two with the same footprint one fp32 ULP of model z apart
    d = 2.0
    z_ulp = float(np.nextafter(np.float32(_EYE_Z - d), np.float32(10.0))) - (_EYE_Z - d)
    f8 = mesh("8 coplanar and one ULP apart", [
        [(215.3, 285.2, d), (265.1, 288.4, d), (228.2, 335.9, d)], [(225.3, 281.2, d), (275.1, 298.4, d), (218.2, 325.9, d)],
        [(285.3, 285.2, d), (325.1, 288.4, d), (298.2, 335.9, d)], [(285.3, 285.2, d - z_ulp), (325.1, 288.4, d - z_ulp), (298.2, 335.9, d - z_ulp)]])
    # 10. a stack of overlapping triangles at different depths across the row where the band-split runs cut the image
    f10 = mesh("10 stack across the band edge", [[(340.2 + 6 * k, 185.3 + 2 * k, 1.5 + 0.1 * k), (395.4 + 5 * k, 190.1 + k, 1.5 + 0.1 * k), (360.7 + 4 * k, 240.2 - 2 * k, 1.5 + 0.1 * k)] for k in range(6)])
    # 11. tilted: every vertex at its own depth (the families above lie on planes z = const, where any weighting of the corner depths gives the plane's)
    f11 = mesh("11 tilted", [[(430.3, 285.2, 1.5), (520.1, 300.4, 4.0), (445.2, 340.9, 2.5)], [(540.3, 290.2, 5.0), (600.1, 283.4, 1.25), (585.2, 345.9, 3.0)],
                             [(440.3, 350.2, 6.0), (590.1, 360.4, 2.0), (470.2, 405.9, 1.75)]])
    eye = np.eye(4, dtype=np.float32)

    def mirror(dx_px, dy_px, d_plane, dz=0.0):
        """x -> -x (the screen column c goes to W - c), then moved by whole pixels at the family's depth; drawn with reversed winding"""
        m = np.diag([-1.0, 1.0, 1.0, 1.0]).astype(np.float32)
        m[3, :3] = [dx_px / (W / 2) * d_plane / w, -dy_px / (H / 2) * d_plane / h, dz]
        return m
    instances = [(k, eye) for k in range(len(meshes))]
    # 9. mirrored instances of families 1, 2 and 5
    instances += [(f1, mirror(0, 0, 2.0), True), (f2, mirror(60, 190, 3.0, -0.5), True), (f2s, mirror(60, 190, 3.0, -0.5), True), (f2w, mirror(60, 190, 3.0, -0.5), True), (f5n, mirror(0, 0, 2.25), True), (f5w, mirror(0, 0, 2.25), True), (f5m, mirror(0, 0, 2.25), True)]
    kw.setdefault("point_lights", 4)
    sc = RawScene(width=W, height=H, meshes=meshes, instances=instances, view=dict(eye=(0.0, 0.0, _EYE_Z), yaw=0.0, pitch=0.0, fov=_FOV, near=0.01, far=100.0), **kw)
    if scissor is not None:
        info = sc.arrays["viewRasterInfo"].view(np.uint32)
        info[3:7] = scissor
    return sc, names, intended


ADVERSARIAL_SCISSOR = (37, 21, 655, 389)
