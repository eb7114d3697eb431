"""Clustered lighting restated from the shader text alone (numpy; TEST INFRASTRUCTURE).

A second reading of the light grid, the paged light lists and the part of the deferred pass that finds a pixel's cluster, walks its
list and applies range, attenuation and spot cone.  Written from the HLSL only; it opens nothing of oracle/ or of the kernels and
makes no call into liboracle.so.  What it needs of this repository is the byte layout of the scene buffers (include/brmi_types.h),
which is the reference's (structs.hlsli:148-176 Camera, :196-224 PerFrameBuffer, :229-250 LightInfo, :533-547 LightPage / Cluster).

Lines restated:

  clustering.hlsl:6-12      lineIntersectionWithZPlane                       -> _line_z
  clustering.hlsl:16-29     screenToView (the `- 1` of the flipped y kept)    -> _screen_to_view
  clustering.hlsl:55-66     tile size, tile corners on the far plane (z = 1)  -> boxes
  clustering.hlsl:68-92     slice planes: uniform below zSplit, log beyond    -> planes64
  clustering.hlsl:95-106    four intersections, component-wise min / max      -> boxes
  lightCulling.hlsl:7-20    sphereAABBIntersection, testSphereAABB            -> centres, hits
  lightCulling.hlsl:22-30   AllocatePage: the counter grows past the pool     -> allocate
  lightCulling.hlsl:68-125  the serial allocator, the `switch (light.type)`   -> allocate, hits
  lighting.hlsli:70-79      spotAttenuation                                   -> pixel_light
  lighting.hlsli:81-113     getLightParametersForFragment                     -> pixel_light
  lighting.hlsli:166-196    ComputeClusterID                                  -> pixel_cluster
  lighting.hlsli:502-526    cluster index, the page walk and its three exits  -> walk
  lighting.hlsli:528        `activeLightIndices[page.lightIndices[i]]`        -> walk (see below)
  lighting.hlsli:530-532    the loop over every active light (no clusters)    -> plain_list
  lighting.hlsli:607-610    `light.type != 2 && distance > light.maxRange`    -> pixel_light
  lighting.hlsli:617-621    remainingLights, ptrNextPage, pagesVisited        -> walk
  deferred.hlsl:25-27       uv from the pixel INDEX + 0.5, y flipped          -> world_position
  deferred.hlsl:41-49       positionVS = mul(clip, projectionInverse).xyz * depth, positionWS through viewInverse
  deferred.hlsl:54, utilities.hlsli:2640   `ret.pixelCoords = pixelCoordinates`, the uint2 `pixel` of deferred.hlsl:25

**pixelCoords is the pixel index, not the pixel centre.**  deferred.hlsl:25 has `uint2 pixel = dispatchThreadId.xy`, :54 passes `pixel` to
GetFragmentInfoScreenSpace, whose first line (utilities.hlsli:2640) stores it in `FragmentInfo::pixelCoords`; lighting.hlsli:502 hands that to
ComputeClusterID, which divides it by the tile size (:170).  The + 0.5 of deferred.hlsl:26 goes into `uv` only.  (The forward path differs:
utilities.hlsli:2777 / :2793 take `input.position.xy`, SV_Position, which is the centre.  Only the deferred path is restated here.)

**The page holds light indices, and the walk indexes activeLightIndices with them.**  lightCulling.hlsl:105 / :112 store `activeLightIndices[i]` in the
page; lighting.hlsli:528 reads `activeLightIndices[page.lightIndices[i]]`, a second indirection.  `walk` returns both readings: `slots` (the page words)
and `lights_text` (the words looked up in activeLightIndices once more, as :528 has it).  They are the same list wherever activeLightIndices is the
identity, which is every scene the reference's LightManager builds without removals.

Arithmetic (DESIGN.md section 2's contract): IEEE binary32, round to nearest even, nothing fused, `mul(v, M)` accumulated k = 0..3, dot products x, y, z in
order, correctly rounded `/` and `sqrt`, `normalize = v * (1 / sqrt(dot))`, float -> uint saturating (negative and NaN give 0).  numpy's float32
scalar and array operations are exactly that; every constant below is wrapped in np.float32 so that nothing is promoted.  The `log` of the slice lookup
is the correctly rounded fp32 logarithm (evaluated in float64 and rounded once), as DESIGN.md defines; the `log` / `exp` of the slice PLANES are the host's
and come in as an input to `boxes`.

**Bound on the host's slice planes** (planes_bound; u = 2^-24, L = max(|log(zSplit / zNear)|, |log(zFar / zNear)|), `log` and `exp` each taken to be within
4 ulp = 8 u relative of the true value of their fp32 argument).  Uniform slices: `(zSplit - zNear) / n`, one product and one sum of positive terms: 4 u
relative.  Log slices: each quotient carries u, so each log is off by 8 u L + u; their difference by twice that plus its rounding, 17 u L + 2 u; times
t <= 1 (t itself one rounding, the product another): 19 u L + 2 u; plus logStart and the sum's rounding: 28 u L + 3 u absolute in the exponent, which is the
relative error of the exponential; `exp` adds 8 u, the product with zNear u: (28 L + 12) u.  For zNear 0.1 and zFar 200 that is 1.3e-5.
"""
import numpy as np

f32 = np.float32
LIGHTS_PER_PAGE = 12
NULL = 0xFFFFFFFF
CAMERA_WORDS, LIGHT_WORDS, CLUSTER_WORDS, PAGE_WORDS = 184, 32, 12, 14
U = 2.0 ** -24


class Frame:
    """The inputs the three shaders read, decoded from the scene's byte arrays (`arrays`: name -> numpy array of bytes or words)."""

    def __init__(self, arrays):
        pf = np.ascontiguousarray(arrays["perFrame"]).view(np.uint32)
        pff = pf.view(f32)
        self.main_camera, self.num_lights = int(pf[8]), int(pf[9])
        self.W, self.H = int(pf[13]), int(pf[14])
        self.gx, self.gy, self.gz, self.near_slices = int(pf[15]), int(pf[16]), int(pf[17]), int(pf[18])
        self.z_split = f32(pff[19])
        cam = np.ascontiguousarray(arrays["cameras"]).view(f32).reshape(-1, CAMERA_WORDS)[self.main_camera]
        self.cam_pos = cam[0:4].copy()
        self.view, self.view_inverse = cam[4:20].reshape(4, 4).copy(), cam[20:36].reshape(4, 4).copy()
        self.projection_inverse = cam[52:68].reshape(4, 4).copy()
        self.z_near, self.z_far = f32(cam[174]), f32(cam[175])
        self.lights = np.ascontiguousarray(arrays["lights"]).view(np.uint32).reshape(-1, LIGHT_WORDS).copy()
        self.active = np.ascontiguousarray(arrays["activeLightIndices"]).view(np.uint32).copy()
        self.total = self.gx * self.gy * self.gz

    # LightInfo fields
    def light_type(self, li): return self.lights[li, 0]
    def light_f(self): return self.lights.view(f32)


def mul_v_m(v, M, dtype=f32):
    """mul(float4 v, matrix M): out_j = ((v0 M0j + v1 M1j) + v2 M2j) + v3 M3j; v [..., 4], M [4, 4]"""
    v, M = np.asarray(v, dtype=dtype), np.asarray(M, dtype=dtype)
    out = v[..., 0:1] * M[0]
    for k in (1, 2, 3):
        out = out + v[..., k:k + 1] * M[k]
    return out


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def to_uint(x):
    """float -> uint, saturating: negative and NaN give 0"""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isnan(x) | (x <= 0), 0, np.minimum(np.floor(np.where(np.isnan(x), 0, x)), 4294967295.0)).astype(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# clustering.hlsl
def planes64(fr):
    """[gz, 2] float64 (planeNear, planeFar), both negative (clustering.hlsl:76-92), from the fp32 camera and per-frame values"""
    zn, zf, zs = float(fr.z_near), float(fr.z_far), float(fr.z_split)
    out = np.zeros((fr.gz, 2))
    for s in range(fr.gz):
        if s < fr.near_slices:
            size = (zs - zn) / fr.near_slices
            out[s] = -(zn + s * size), -(zn + (s + 1) * size)
        else:
            a, b = np.log(zs / zn), np.log(zf / zn)
            d = float(fr.gz - fr.near_slices)
            t0, t1 = (s - fr.near_slices) / d, (s + 1 - fr.near_slices) / d
            out[s] = -zn * np.exp(a + t0 * (b - a)), -zn * np.exp(a + t1 * (b - a))
    return out


def planes_bound(fr):
    """relative bound on an fp32 evaluation of planes64 (module docstring)"""
    zn, zf, zs = float(fr.z_near), float(fr.z_far), float(fr.z_split)
    L = max(abs(np.log(zs / zn)), abs(np.log(zf / zn)))
    return (28.0 * L + 12.0) * U


def _screen_to_view(x, y, fr, dtype):
    """clustering.hlsl:16-29 with screenCoord.z = 1"""
    one, two = dtype(1.0), dtype(2.0)
    rx, ry = dtype(fr.W), dtype(fr.H)
    ndc = np.stack([two * x / rx - one, two * (ry - y - one) / ry - one, np.full_like(x, one), np.full_like(x, one)], -1)
    v = mul_v_m(ndc, fr.projection_inverse, dtype)
    return (v / v[..., 3:4])[..., :3]


def _line_z(end, z_distance, dtype):
    """clustering.hlsl:6-12 with startPoint = 0: direction = end - 0; t = (zDistance - dot(n, 0)) / dot(n, direction); 0 + t * direction"""
    zero, one = dtype(0.0), dtype(1.0)
    start = np.zeros_like(end)
    direction = end - start
    n_dot_start = (zero * start[..., 0] + zero * start[..., 1]) + one * start[..., 2]
    n_dot_dir = (zero * direction[..., 0] + zero * direction[..., 1]) + one * direction[..., 2]
    t = (z_distance - n_dot_start) / n_dot_dir
    return start + t[..., None] * direction


def boxes(fr, planes, dtype=f32):
    """(aabbMin, aabbMax) [clusters, 3] in index order x + y gx + z gx gy; `planes` [gz, 2] = (planeNear, planeFar) as the host hands them"""
    planes = np.asarray(planes, dtype=dtype).reshape(fr.gz, 2)
    gz_, gy_, gx_ = np.meshgrid(np.arange(fr.gz), np.arange(fr.gy), np.arange(fr.gx), indexing="ij")
    gx_, gy_, gz_ = gx_.ravel(), gy_.ravel(), gz_.ravel()
    tsx, tsy = dtype(fr.W) / dtype(fr.gx), dtype(fr.H) / dtype(fr.gy)
    fx, fy = gx_.astype(dtype), gy_.astype(dtype)
    mn = _screen_to_view(fx * tsx, fy * tsy, fr, dtype)
    mx = _screen_to_view((fx + dtype(1.0)) * tsx, (fy + dtype(1.0)) * tsy, fr, dtype)
    pn, pf = planes[gz_, 0], planes[gz_, 1]
    p = [_line_z(mn, pn, dtype), _line_z(mx, pn, dtype), _line_z(mn, pf, dtype), _line_z(mx, pf, dtype)]
    lo = np.minimum(np.minimum(p[0], p[1]), np.minimum(p[2], p[3]))
    hi = np.maximum(np.maximum(p[0], p[1]), np.maximum(p[2], p[3]))
    return lo, hi


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# lightCulling.hlsl
def centres(fr, dtype=f32):
    """view-space centre and radius of list position i (light activeLightIndices[i]): mul(float4(boundingSphere.xyz, 1), view).xyz, boundingSphere.w"""
    lf = fr.light_f()[fr.active[:fr.num_lights]]
    pos = np.concatenate([lf[:, 25:28], np.ones((len(lf), 1), dtype=f32)], 1)
    return mul_v_m(pos, fr.view, dtype)[:, :3], lf[:, 28].astype(dtype)


def hits(fr, lo, hi, dtype=f32):
    """[clusters, numLights] bool: list position i is written to the cluster's pages (lightCulling.hlsl:100-116).  Types 0 and 1 by the sphere test, type 2
    always, every other type never: the switch has no default."""
    c, r = centres(fr, dtype)
    types = fr.lights[fr.active[:fr.num_lights], 0]
    lo, hi = np.asarray(lo, dtype=dtype), np.asarray(hi, dtype=dtype)
    closest = np.maximum(lo[:, None, :], np.minimum(c[None, :, :], hi[:, None, :]))
    d = closest - c[None, :, :]
    with np.errstate(over="ignore"):      # (a radius of 1e20 squares to +inf, as in the shader)
        touch = dot3(d, d) <= (r * r)[None, :]
    return np.where(types[None, :] <= 1, touch, types[None, :] == 2)


def allocate(fr, hit, pool):
    """The serial allocator over clusters in index order (the canonical order).  Returns dict(numLights, first [clusters] uint32, pages [pool, 14] uint32,
    written [pool, 14] bool -- the words the shader stores --, counter: LinkedListCounter[0], which AllocatePage increments whether or not a page was left)."""
    n = hit.shape[0]
    num, first = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    pages, written = np.zeros((pool, PAGE_WORDS), dtype=np.uint32), np.zeros((pool, PAGE_WORDS), dtype=bool)
    counter = 0

    def alloc():
        nonlocal counter
        index = counter
        counter += 1
        return NULL if index >= pool else index

    def put(pg, word, value):
        pages[pg, word], written[pg, word] = value, True

    for c in range(n):
        page = alloc()
        count, first[c] = 0, page
        if page == NULL:
            continue
        put(page, 0, NULL)
        in_page = 0
        for i in range(fr.num_lights):
            if in_page >= LIGHTS_PER_PAGE:
                put(page, 1, LIGHTS_PER_PAGE)
                old = page
                page = alloc()
                if page == NULL:
                    break
                put(page, 0, old)
                first[c] = page
                in_page = 0
            if hit[c, i]:
                put(page, 2 + in_page, fr.active[i])
                in_page += 1
                count += 1
        if page != NULL:
            put(page, 1, in_page)
        num[c] = count
    return dict(numLights=num, first=first, pages=pages, written=written, counter=counter)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# lighting.hlsli
def walk(fr, num_lights, first, pages):
    """The lights a pixel of a cluster shades, in order (lighting.hlsli:511-526, :617-621): (slots, lights_text).  `slots` are the page words; `lights_text`
    is activeLightIndices[slot], the index :528 reads.  Exits: a null page, no lights remaining, the page budget max(1, ceil(numLights / 12)), and the `break`
    on a page of zero lights -- the empty newest page of a cluster whose twelfth (24th, ...) hit was not its last light."""
    slots = []
    page, remaining, visited = int(first), int(num_lights), 0
    budget = max(1, (int(num_lights) + LIGHTS_PER_PAGE - 1) // LIGHTS_PER_PAGE)
    while page != NULL and remaining > 0 and visited < budget:
        in_page = min(min(int(pages[page, 1]), LIGHTS_PER_PAGE), remaining)
        if in_page == 0:
            break
        slots.extend(int(v) for v in pages[page, 2:2 + in_page])
        remaining -= in_page
        page = int(pages[page, 0])
        visited += 1
    return slots, [int(fr.active[s]) for s in slots]


def plain_list(fr):
    """lighting.hlsli:530-532: without PSO_CLUSTERED_LIGHTING every list position, light activeLightIndices[i]"""
    return [int(v) for v in fr.active[:fr.num_lights]]


def log32(x):
    """the correctly rounded fp32 logarithm of fp32 x"""
    return np.log(np.asarray(x, dtype=np.float64)).astype(f32)


def world_position(fr, depth, dtype=f32):
    """deferred.hlsl:25-49: (positionVS, positionWS) [H, W, 3] from the linear depth plane"""
    H, W = depth.shape
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    half, one, two = dtype(0.5), dtype(1.0), dtype(2.0)
    uvx = (px.astype(dtype) + half) / dtype(W)
    uvy = one - (py.astype(dtype) + half) / dtype(H)
    clip = np.stack([uvx * two - one, uvy * two - one, np.full_like(uvx, one), np.full_like(uvx, one)], -1)
    with np.errstate(all="ignore"):      # (pixels without geometry hold the largest float)
        vh = mul_v_m(clip, fr.projection_inverse, dtype)
        vs = vh[..., :3] * np.asarray(depth, dtype=dtype)[..., None]
        ws = mul_v_m(np.concatenate([vs, np.ones_like(vs[..., :1])], -1), fr.view_inverse, dtype)[..., :3]
    return vs, ws


def pixel_cluster(fr, view_z):
    """ComputeClusterID + lighting.hlsli:503-505 in fp32: (tileX, tileY, slice, clusterIndex) per pixel of `view_z` [H, W] = positionVS.z"""
    H, W = view_z.shape
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    tsx, tsy = f32(fr.W) / f32(fr.gx), f32(fr.H) / f32(fr.gy)
    tx, ty = to_uint(px.astype(f32) / tsx), to_uint(py.astype(f32) / tsy)
    z = np.abs(np.asarray(view_z, dtype=f32))
    zn, zf, zs = fr.z_near, fr.z_far, fr.z_split
    with np.errstate(all="ignore"):
        t = (z - zn) / (zs - zn)
        near = to_uint(t * f32(fr.near_slices))
        a, b, lz = log32(zs / zn), log32(zf / zn), log32(z / zn)
        u = (lz - a) / (b - a)
        far = np.uint64(fr.near_slices) + to_uint(u * f32(np.uint32((fr.gz - fr.near_slices) & 0xFFFFFFFF)))
    sl = np.where(z < zs, near, far)
    return tx, ty, sl, tx + ty * np.uint64(fr.gx) + sl * np.uint64(fr.gx * fr.gy)


def _normalize(v):
    return v * (f32(1.0) / np.sqrt(dot3(v, v)))[..., None]


def pixel_light(fr, ws, li):
    """Light `li` at world positions `ws` [..., 3] (fp32, from world_position).  fp32 under the contract: `distance`, the decision `cut` (type != 2 and
    distance > maxRange, lighting.hlsli:607), `cos`, `outside` (not cos > outer) and `below_inner` (cos < inner).  float64 from the same fp32 inputs:
    `distance64`, `cut64`, `outside64`, `below_inner64`, `attenuation64`, `spot64` and `factor64` = attenuation x spot, 0 where the fp32 decisions reject."""
    L = fr.light_f()[li]
    kind = int(fr.lights[li, 0])
    ws = np.asarray(ws, dtype=f32)
    pos, direction = L[4:7], L[8:11]
    c, l, q, max_range, inner, outer = L[12], L[13], L[14], L[29], L[1], L[2]
    out = {}
    with np.errstate(all="ignore"):
        to_l = pos - ws
        to_l64 = pos.astype(np.float64) - ws.astype(np.float64)
        if kind == 2:
            shape = ws.shape[:-1]
            out.update(distance=np.zeros(shape, f32), distance64=np.zeros(shape), cut=np.zeros(shape, bool), cut64=np.zeros(shape, bool),
                       attenuation64=np.ones(shape))
        else:
            d = np.sqrt(dot3(to_l, to_l))
            d64 = np.sqrt(dot3(to_l64, to_l64))
            out.update(distance=d, distance64=d64, cut=d > max_range, cut64=d64 > float(max_range),
                       attenuation64=1.0 / ((float(c) + float(l) * d64 + float(q) * d64 * d64) + 0.0001))
        shape = ws.shape[:-1]
        if kind == 1:
            light_to_frag = _normalize(to_l)
            cos = dot3(_normalize(np.broadcast_to(direction, to_l.shape).copy()), _normalize(-light_to_frag))
            d64v = direction.astype(np.float64)
            cos64 = dot3(np.broadcast_to(d64v / np.sqrt(dot3(d64v, d64v)), to_l64.shape), -to_l64 / np.sqrt(dot3(to_l64, to_l64))[..., None])
            o64, i64 = float(outer), float(inner)
            t = np.clip((cos64 - o64) / (i64 - o64), 0.0, 1.0)
            smooth = t * t * (3.0 - 2.0 * t)
            outside, below = ~(cos > outer), cos < inner
            out.update(cos=cos, cos64=cos64, outside=outside, below_inner=below, outside64=~(cos64 > o64), below_inner64=cos64 < i64,
                       spot64=np.where(outside, 0.0, np.where(below, smooth, 1.0)))
        else:
            out.update(cos=np.ones(shape, f32), cos64=np.ones(shape), outside=np.zeros(shape, bool), below_inner=np.zeros(shape, bool),
                       outside64=np.zeros(shape, bool), below_inner64=np.zeros(shape, bool), spot64=np.ones(shape))
        out["rejected"] = out["cut"] | out["outside"]
        out["on_edge"] = (out["cut"] != out["cut64"]) | (out["outside"] != out["outside64"]) | (out["below_inner"] != out["below_inner64"])
        out["factor64"] = np.where(out["rejected"], 0.0, out["attenuation64"] * out["spot64"])
    return out
