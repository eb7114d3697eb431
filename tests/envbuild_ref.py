"""The environment build and the skybox stage, restated for tests in numpy from the shader text alone: BR/shaders/envToCubemap.hlsl,
sphericalHarmonics.hlsl, blurEnvironment.hlsl (+ the loop of EnvironmentFilterPass.h:99-127), skybox.hlsl.  Nothing here calls the library under test.

Every function takes the float type `dt`.  In float32 every operation is one numpy operation on float32 operands (correctly rounded, never fused) in the
shader's own order, with normalize(v) = v * (1 / sqrt(dot(v, v))) and dot = ((x x + y y) + z z): what the stages that are IEEE fp32 throughout (SH projection,
skybox, the fp16 lookup) must reproduce bit for bit.  In float64 the same text serves as the reference of the stages that call sin / cos / atan2 / asin.

A cube is either six RGBA8 mip chains (lists of (n, n, 4) uint8, what ibl_ref.sample_cube takes) or a (6, n, n, 4) float16 array (one level), or six lists of
float16 levels.
"""
import numpy as np

import ibl_ref

f32, f64 = np.float32, np.float64
PI = 3.14159265359            # the PI of the three build shaders
EMPTY_DEPTH = 0x7F7FFFFF


# ------------------------------------------------------------------------------------------------ lookups
def _bilinear16(level, u, v, dt):
    """ibl_ref._bilinear for a level of halves: a half decodes to the float of the same value."""
    h, w = level.shape[:2]
    tex = level.astype(dt)
    fx, fy = (u * dt(w)).astype(dt) - dt(0.5), (v * dt(h)).astype(dt) - dt(0.5)
    x0f, y0f = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0f).astype(dt)[:, None], (fy - y0f).astype(dt)[:, None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    xa, xb, ya, yb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1), np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    c00, c10, c01, c11 = tex[ya, xa], tex[ya, xb], tex[yb, xa], tex[yb, xb]
    top = (c00 + (tx * (c10 - c00)).astype(dt)).astype(dt)
    bot = (c01 + (tx * (c11 - c01)).astype(dt)).astype(dt)
    return (top + (ty * (bot - top)).astype(dt)).astype(dt)


def sample_face_level16(chain, u, v, lod, dt=f32):
    """ibl_ref.sample_face_level (the level choice of g_linearClamp, two levels blended where the fraction is not 0) on float16 levels."""
    n = len(u)
    lod = np.ascontiguousarray(lod, dtype=dt)
    with np.errstate(all="ignore"):
        lod = (lod + dt(0.0)).astype(dt)
        lod = np.where(lod > 0, lod, dt(0.0))
        lod = np.where(lod < dt(ibl_ref.FLT_MAX), lod, dt(ibl_ref.FLT_MAX))
        top = dt(len(chain) - 1)
        lod = np.where(lod < top, lod, top).astype(dt)
    l0 = np.floor(lod).astype(np.int64)
    frac = (lod - np.floor(lod)).astype(dt)
    l1 = np.minimum(l0 + 1, len(chain) - 1)
    out = np.zeros((n, 4), dtype=dt)
    for l in range(len(chain)):
        m = l0 == l
        if m.any():
            out[m] = _bilinear16(chain[l], u[m], v[m], dt)
    for l in range(len(chain)):
        m = (l1 == l) & (frac != 0)
        if m.any():
            b = _bilinear16(chain[l], u[m], v[m], dt)
            out[m] = (out[m] + (frac[m][:, None] * (b - out[m])).astype(dt)).astype(dt)
    return out


def is_rgba8(cube):
    return not isinstance(cube, np.ndarray) and np.asarray(cube[0][0]).dtype == np.uint8


def chains16(cube):
    return [[cube[f]] for f in range(6)] if isinstance(cube, np.ndarray) else cube


def sample_cube_any(cube, dirs, lod=0.0, dt=f32):
    """TextureCube::SampleLevel(g_linearClamp, dir, lod) of a cube of either format -> (n, 4)."""
    if is_rgba8(cube):
        return ibl_ref.sample_cube(cube, dirs, lod, dt)
    chains = chains16(cube)
    face, u, v = ibl_ref.cube_face_uv(dirs, dt)
    lod = np.broadcast_to(np.asarray(lod, dtype=dt), (len(u),))
    out = np.zeros((len(u), 4), dtype=dt)
    for f in range(6):
        m = face == f
        if m.any():
            out[m] = sample_face_level16(chains[f], u[m], v[m], lod[m], dt)
    return out


def sample_2d_any(level, uv, dt):
    """Texture2D::SampleLevel(g_linearClamp, uv, 0) of one level, (h, w, 4) float16 or uint8 -> (n, 4)"""
    u, v = uv[:, 0].astype(dt), uv[:, 1].astype(dt)
    if level.dtype == np.uint8:
        return ibl_ref._bilinear(level, u, v, dt)
    return _bilinear16(level, u, v, dt)


# ------------------------------------------------------------------------------------------------ vector helpers, one rounding per operation
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize(v):
    """v * (1 / sqrt(dot(v, v))): square root and reciprocal correctly rounded, as numpy computes them"""
    dt = v.dtype.type
    with np.errstate(all="ignore"):
        inv = dt(1.0) / np.sqrt(dot3(v, v))
    return v * inv[..., None]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def mul_vm(v, m):
    """mul(float4 v, M): row vector times row-major matrix, k accumulated 0..3 left to right"""
    return np.stack([((v[..., 0] * m[0, j] + v[..., 1] * m[1, j]) + v[..., 2] * m[2, j]) + v[..., 3] * m[3, j] for j in range(4)], -1)


def _texel_uv(size, dt):
    """((i + 0.5) / size) * 2 - 1 for every texel, as (x grid, y grid) of shape (size, size), row = y"""
    c = ((np.arange(size).astype(dt) + dt(0.5)) / dt(size)) * dt(2.0) - dt(1.0)
    return np.meshgrid(c, c, indexing="xy")


def face_uv_to_dir(face, u, v):
    """FaceUVToDir of envToCubemap.hlsl / blurEnvironment.hlsl (uv in [-1, 1], y already flipped), normalised"""
    one = np.ones_like(u)
    d = [(one, v, -u), (-one, v, u), (u, one, -v), (u, -one, v), (u, v, one), (-u, v, -one)][face]
    return normalize(np.stack(d, -1))


def sh_face_dir(face, u, v):
    """the face table of sphericalHarmonics.hlsl (no y flip: the signs are in the table), not normalised"""
    one = np.ones_like(u)
    d = [(one, -v, -u), (-one, -v, u), (u, one, v), (u, -one, -v), (u, -v, one), (-u, -v, -one)][face]
    return np.stack(d, -1)


# ------------------------------------------------------------------------------------------------ sphericalHarmonics.hlsl
SH_C = (0.28209479, 0.48860251, 1.09254843, 0.31539157, 0.54627422)


def sh_basis(d):
    """the nine basis values of a direction, in the shader's order of operations"""
    dt = d.dtype.type
    c0, c1, c2, c3, c4 = (dt(c) for c in SH_C)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, c0), c1 * y, c1 * z, c1 * x, (c2 * x) * y, (c2 * y) * z, c3 * (((dt(3.0) * z) * z) - dt(1.0)), (c2 * z) * x,
                     c4 * (x * x - y * y)], -1)


def project_sh(cube, size, dt=f32):
    """(27 integers as int32 (sums wrapped to 32 bits), scale as float32): (int)(L * sh[i] * 100) per texel and channel, truncating toward zero (saturating,
    NaN -> 0), summed; scale = 4 pi / (size^2 * 6) in float32 (Environment.cpp:31, XM_PI = 3.141592654f)."""
    total = np.zeros(27, dtype=np.int64)
    u, v = _texel_uv(size, dt)
    for face in range(6):
        d = normalize(sh_face_dir(face, u, v)).reshape(-1, 3)
        L = sample_cube_any(cube, d, 0.0, dt)[:, :3]
        contrib = (L[:, None, :] * sh_basis(d)[:, :, None]) * dt(100.0)          # (n, 9, 3)
        with np.errstate(all="ignore"):
            t = np.where(np.isnan(contrib), 0.0, np.clip(np.trunc(contrib.astype(f64)), -2.0 ** 31, 2.0 ** 31 - 1))
        total += t.astype(np.int64).reshape(-1, 27).sum(axis=0)
    wrapped = (total & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    scale = f32(f32(4.0) * f32(3.141592654)) / f32(size * size * 6)
    return wrapped, f32(scale)


def project_sh_float(cube, size):
    """the same sums without the integer step, float64: (9, 3) = sum over texels of L * basis (what the integers / 100 approximate)"""
    total = np.zeros((9, 3))
    u, v = _texel_uv(size, f64)
    for face in range(6):
        d = normalize(sh_face_dir(face, u, v)).reshape(-1, 3)
        L = sample_cube_any(cube, d, 0.0, f64)[:, :3]
        total += (L[:, None, :] * sh_basis(d)[:, :, None]).sum(axis=0)
    return total


# ------------------------------------------------------------------------------------------------ blurEnvironment.hlsl
def _reverse_bits(i):
    return int("{:032b}".format(i)[::-1], 2)


def prefilter_directions(size, level, dt=f64):
    """N of every texel of a level: (6, s, s, 3)"""
    s = max(1, size >> level)
    u, v = _texel_uv(s, dt)
    return np.stack([normalize(face_uv_to_dir(f, u, -v)) for f in range(6)])


def prefilter_level(cube, size, levels, level, dt=f64):
    """the unquantised rgb of level `level`: (6, s, s, 3) in dt"""
    s = max(1, size >> level)
    roughness = dt(level) / dt(levels - 1) if levels > 1 else dt(0.0)
    a = roughness * roughness
    N = prefilter_directions(size, level, dt).reshape(-1, 3)
    V = N
    up = np.where((np.abs(N[:, 2]) < dt(0.999))[:, None], np.array([0, 0, 1], dtype=dt), np.array([1, 0, 0], dtype=dt))
    T = normalize(cross3(up, N))
    B = cross3(N, T)
    acc, total = np.zeros((len(N), 3), dtype=dt), np.zeros(len(N), dtype=dt)
    for i in range(16):
        xi_x, xi_y = dt(i) / dt(16.0), dt(dt(_reverse_bits(i)) * dt(2.3283064365386963e-10))
        phi = (dt(2.0) * dt(PI)) * xi_x
        cos_t = np.sqrt((dt(1.0) - xi_y) / (dt(1.0) + (a * a - dt(1.0)) * xi_y))
        sin_t = np.sqrt(max(dt(0.0), dt(1.0) - cos_t * cos_t))
        hx, hy, hz = dt(np.cos(phi) * sin_t), dt(np.sin(phi) * sin_t), dt(cos_t)
        H = normalize((T * hx + B * hy) + N * hz)
        L = normalize(((dt(2.0) * dot3(V, H))[:, None] * H) - V)
        ndotl = np.maximum(dot3(N, L), dt(0.0))
        c = sample_cube_any(cube, L, 0.0, dt)[:, :3]
        hit = ndotl > 0
        acc = np.where(hit[:, None], acc + c * ndotl[:, None], acc)
        total = np.where(hit, total + ndotl, total)
    with np.errstate(all="ignore"):
        out = np.where((total > 0)[:, None], acc / total[:, None], dt(0.0))
    return out.reshape(6, s, s, 3).astype(dt)


def unorm_codes(v):
    """saturate, then the nearest code: (uint)(sat(x) * 255 + 0.5) in the value's own float type"""
    dt = v.dtype.type
    return (np.clip(v, dt(0.0), dt(1.0)) * dt(255.0) + dt(0.5)).astype(np.int64)


def prefilter(cube, size, levels, dt=f64):
    """[level] -> (6, s, s, 3) unquantised values"""
    return [prefilter_level(cube, size, levels, m, dt) for m in range(levels)]


def prefiltered_faces(values):
    """six RGBA8 chains (what Environment takes) of prefilter()'s values"""
    return [[np.concatenate([unorm_codes(v[f]), np.full(v[f].shape[:2] + (1,), 255)], -1).astype(np.uint8) for v in values] for f in range(6)]


# ------------------------------------------------------------------------------------------------ envToCubemap.hlsl
def convert(equirect, size, dt=f64):
    """(values (6, size, size, 3) in dt before the fp16 store, equirect uv (6, size, size, 2)) of an (H, W, 4) float16 / uint8 panorama"""
    u, v = _texel_uv(size, dt)
    vals, uvs = [], []
    for face in range(6):
        d = normalize(face_uv_to_dir(face, u, -v)).reshape(-1, 3)
        eu = np.arctan2(d[:, 2], d[:, 0]) / (dt(2.0) * dt(PI)) + dt(0.5)
        ev = dt(0.5) - np.arcsin(d[:, 1]) / dt(PI)
        uv = np.stack([eu, ev], -1).astype(dt)
        vals.append(sample_2d_any(equirect, uv, dt)[:, :3].reshape(size, size, 3)); uvs.append(uv.reshape(size, size, 2))
    return np.stack(vals), np.stack(uvs)


# ------------------------------------------------------------------------------------------------ skybox.hlsl
def camera_matrices(cam_words, dt):
    """the matrices skybox.hlsl reads from one brmi_camera given as 184 float32 words"""
    c = np.asarray(cam_words, dtype=f32).astype(dt)
    m = lambda o: c[o:o + 16].reshape(4, 4)
    return dict(view=m(4), viewInverse=m(20), projectionInverse=m(52), prevView=m(84), prevUnjitteredProjection=m(116), unjitteredProjection=m(132))


def skybox(cam_words, W, H, cube, dt=f32):
    """(rgb (H, W, 3), motion vector (H, W, 2)) of every pixel as skybox.hlsl computes an empty one, before the fp16 stores"""
    M = camera_matrices(cam_words, dt)
    ux = (np.arange(W).astype(dt) + dt(0.5)) / dt(W)
    uy = dt(1.0) - (np.arange(H).astype(dt) + dt(0.5)) / dt(H)
    nx, ny = np.meshgrid(ux * dt(2.0) - dt(1.0), uy * dt(2.0) - dt(1.0), indexing="xy")
    one, zero = np.ones_like(nx), np.zeros_like(nx)
    h = mul_vm(np.stack([nx, ny, one, one], -1), M["projectionInverse"])
    w = np.maximum(np.abs(h[..., 3]), dt(1e-6))
    view_dir = normalize(h[..., :3] / w[..., None])
    with0 = lambda v: np.concatenate([v, zero[..., None]], -1)
    with1 = lambda v: np.concatenate([v, one[..., None]], -1)
    world = normalize(mul_vm(with0(view_dir), M["viewInverse"])[..., :3])
    cur = mul_vm(with1(normalize(mul_vm(with0(world), M["view"])[..., :3])), M["unjitteredProjection"])
    prev = mul_vm(with1(normalize(mul_vm(with0(world), M["prevView"])[..., :3])), M["prevUnjitteredProjection"])
    cur_ndc = cur[..., :2] / np.maximum(np.abs(cur[..., 3]), dt(1e-6))[..., None]
    prev_ndc = prev[..., :2] / np.maximum(np.abs(prev[..., 3]), dt(1e-6))[..., None]
    rgb = sample_cube_any(cube, world.reshape(-1, 3), 0.0, dt)[:, :3].reshape(H, W, 3)
    return rgb.astype(dt), (cur_ndc - prev_ndc).astype(dt)


def half_ulp_of(x):
    """one fp16 ULP at |x| (2^-24 below the normal range)"""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -14)))
    return 2.0 ** (e - 10)
