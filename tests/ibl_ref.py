"""Image-based lighting (DESIGN.md 2 "cube lookup", 4.11), restated for tests in numpy from the written definition and the shader text
(BR/shaders/Include/IBL.hlsli, PBR.hlsli, utilities.hlsli:2590-2709).  Nothing here calls the library under test or the oracle.

* the cube lookup, generic over the float type: in float32 every operation is one numpy operation on float32 operands (correctly rounded, never fused), in the
  sampler's own order -- what brmi_debug_ibl_lookup must reproduce bit for bit; in float64 it serves the term below;
* evaluateIBL in float64, from the G-buffer words of a pixel, a view vector, the scene's OpenPBR records and lookup tables, and an environment.
"""
import numpy as np

f32, f64 = np.float32, np.float64
FLT_MAX = 3.4028234663852886e38
MIN_PERCEPTUAL_ROUGHNESS, MIN_N_DOT_V = 0.06, 1e-4
PREFILTER_LEVELS = 12
PI_SHADER = 3.1415926538      # the PI of the reference's shaders (constants.hlsli), what Fd_Lambert and the FON constants are made of


# ------------------------------------------------------------------------------------------------ the cube lookup
def cube_face_uv(d, dt=f32):
    """(face, u, v) of n directions: X if |x| >= |y| and |x| >= |z|, else Y if |y| >= |z|, else Z; the major component's sign picks the face;
    u = (sc / ma + 1) * 0.5, v = (tc / ma + 1) * 0.5.  All-zero and non-finite directions: face 0 at (0.5, 0.5)."""
    d = np.ascontiguousarray(d, dtype=dt).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        bad = ~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z)) | ((ax == 0) & (ay == 0) & (az == 0))
        isx = (ax >= ay) & (ax >= az)
        isy = ~isx & (ay >= az)
        isz = ~isx & ~isy
        face = np.where(isx, np.where(x < 0, 1, 0), np.where(isy, np.where(y < 0, 3, 2), np.where(z < 0, 5, 4)))
        ma = np.where(isx, ax, np.where(isy, ay, az))
        sc = np.where(isx, np.where(x < 0, z, -z), np.where(isy, x, np.where(z < 0, -x, x)))
        tc = np.where(isx, -y, np.where(isy, np.where(y < 0, -z, z), -y))
        one, half = dt(1.0), dt(0.5)
        u = ((sc / ma).astype(dt) + one) * half
        v = ((tc / ma).astype(dt) + one) * half
    face = np.where(bad, 0, face)
    u, v = np.where(bad, half, u).astype(dt), np.where(bad, half, v).astype(dt)
    return face.astype(np.int64), u, v


def direction_of(face, u, v):
    """The inverse, stated on its own from the cube layout (float64): the direction through (u, v) of a face, major component +-1."""
    face, sc, tc = np.asarray(face), 2.0 * np.asarray(u, dtype=f64) - 1.0, 2.0 * np.asarray(v, dtype=f64) - 1.0
    one = np.ones_like(sc)
    table = [(one, -tc, -sc), (-one, -tc, sc), (sc, one, tc), (sc, -one, -tc), (sc, -tc, one), (-sc, -tc, -one)]
    out = np.zeros(sc.shape + (3,))
    for f, (x, y, z) in enumerate(table):
        m = face == f
        out[m] = np.stack([x, y, z], -1)[m]
    return out


def _bilinear(level, u, v, dt):
    """One level of one face, linear filter, clamp addressing: the 2x2 footprint around u * w - 0.5, blended a + t * (b - a) along x, then y."""
    h, w = level.shape[:2]
    tex = (level.astype(dt) / dt(255.0)).astype(dt)
    fx, fy = (u * dt(w)).astype(dt) - dt(0.5), (v * dt(h)).astype(dt) - dt(0.5)
    x0f, y0f = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0f).astype(dt)[:, None], (fy - y0f).astype(dt)[:, None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    xa, xb, ya, yb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1), np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    c00, c10, c01, c11 = tex[ya, xa], tex[ya, xb], tex[yb, xa], tex[yb, xb]
    top = (c00 + (tx * (c10 - c00)).astype(dt)).astype(dt)
    bot = (c01 + (tx * (c11 - c01)).astype(dt)).astype(dt)
    return (top + (ty * (bot - top)).astype(dt)).astype(dt)


def sample_face_level(chain, u, v, lod, dt=f32):
    """SampleLevel of one 2D mip chain with g_linearClamp: lod + bias 0 clamped to [0, FLT_MAX] (a NaN reads 0), then to the chain; two levels blended
    a + frac * (b - a) where frac != 0."""
    n = len(u)
    lod = np.ascontiguousarray(lod, dtype=dt)
    with np.errstate(all="ignore"):
        lod = (lod + dt(0.0)).astype(dt)
        lod = np.where(lod > 0, lod, dt(0.0))                  # max2(x, 0) = x > 0 ? x : 0
        lod = np.where(lod < dt(FLT_MAX), lod, dt(FLT_MAX))
        top = dt(len(chain) - 1)
        lod = np.where(lod < top, lod, top).astype(dt)
    l0 = np.floor(lod).astype(np.int64)
    frac = (lod - np.floor(lod)).astype(dt)
    l1 = np.minimum(l0 + 1, len(chain) - 1)
    out = np.zeros((n, 4), dtype=dt)
    for l in range(len(chain)):
        m = l0 == l
        if m.any():
            out[m] = _bilinear(chain[l], u[m], v[m], dt)
    for l in range(len(chain)):
        m = (l1 == l) & (frac != 0)
        if m.any():
            b = _bilinear(chain[l], u[m], v[m], dt)
            out[m] = (out[m] + (frac[m][:, None] * (b - out[m])).astype(dt)).astype(dt)
    return out


def sample_cube(faces, dirs, lod, dt=f32):
    """TextureCube::SampleLevel(g_linearClamp, dir, lod): faces = six mip chains (lists of (n, n, 4) uint8).  No filtering across face edges."""
    face, u, v = cube_face_uv(dirs, dt)
    lod = np.broadcast_to(np.asarray(lod, dtype=dt), (len(u),))
    out = np.zeros((len(u), 4), dtype=dt)
    for f in range(6):
        m = face == f
        if m.any():
            out[m] = sample_face_level(faces[f], u[m], v[m], lod[m], dt)
    return out


# ------------------------------------------------------------------------------------------------ irradianceSH
def fold_sh(sh, scale):
    """(9, 3) float64 coefficients of an environment's integers: value * scale / SH_FLOAT_SCALE (the scale as the float32 the record holds)."""
    return np.asarray(sh, dtype=f64).reshape(9, 3) * f64(f32(scale)) / 100.0


def irradiance_sh(k, n):
    """irradianceSH (IBL.hlsli:8-23) for normals n (m, 3): the basis order is y, z, x as the shader writes it."""
    x, y, z = (n[:, i:i + 1] for i in range(3))
    return (k[0] + k[1] * y + k[2] * z + k[3] * x + k[4] * y * x + k[5] * y * z + k[6] * (3.0 * z * z - 1.0) + k[7] * z * x + k[8] * (x * x - y * y))


# ------------------------------------------------------------------------------------------------ OpenPBR tables (IBL.hlsli:132-139, 307-439)
def sat(x):
    return np.clip(x, 0.0, 1.0)


class Luts:
    """The scene's lookup tables as float64 texel values (UNORM16 / 65535; the fuzz LTC is float)."""

    def __init__(self, arrays):
        u16 = lambda name: arrays[name].view(np.uint16).astype(f64) / 65535.0
        self.od_e = u16("lutOdE").reshape(32, 32, 32)          # [ior slice][alpha row][cos column]
        self.od_avg = u16("lutOdAvg").reshape(32, 32)          # [ior row][alpha column]
        self.im_e = u16("lutImE").reshape(32, 32)              # [alpha row][cos column]
        self.ltc = arrays["lutFuzzLTC"].view(f32).astype(f64).reshape(32, 32, 4)      # [roughness row][cos column]


def _tex2d(t, u, v):
    """Texture2D::SampleLevel(g_linearClamp, (u, v), 0) of t[row, column(, channels)] in float64."""
    h, w = t.shape[:2]
    x, y = u * w - 0.5, v * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    if t.ndim == 3:
        fx, fy = fx[:, None], fy[:, None]
    xa, xb = np.clip(x0, 0, w - 1).astype(int), np.clip(x0 + 1, 0, w - 1).astype(int)
    ya, yb = np.clip(y0, 0, h - 1).astype(int), np.clip(y0 + 1, 0, h - 1).astype(int)
    top, bot = t[ya, xa] + fx * (t[ya, xb] - t[ya, xa]), t[yb, xa] + fx * (t[yb, xb] - t[yb, xa])
    return top + fy * (bot - top)


def ior_to_f0(ior):
    s = np.maximum(ior, 1.0)
    return ((s - 1.0) / (s + 1.0)) ** 2


def _ior_index(ior):
    s = np.maximum(ior, 1.0e-4)
    below = 15.0 - ((1.0 / s - 1.0) / 1.5) * 15.0
    above = 16.0 + ((s - 1.0) / 1.5) * 15.0
    return np.where(s < 1.0, below, above)


def _clamp_index(e):
    return np.clip(e, 0.0, 31.0)


def _remap(e):
    return np.clip(0.5 / 32.0 + e / 32.0, 0.5 / 32.0, 1.0 - 0.5 / 32.0)


def _extrapolate(value, ior):
    f0max = ior_to_f0(2.5)
    progress = (ior_to_f0(np.maximum(ior, 1.0e-4)) - f0max) / (1.0 - f0max)
    return np.where((ior > 2.5) | (ior < 1.0 / 2.5), (1.0 - progress) * value, value)


def od_average(L, ior, alpha):
    ei, ea = _clamp_index(_ior_index(ior)), _clamp_index(np.sqrt(sat(alpha)) * 31.0)
    return _extrapolate(_tex2d(L.od_avg, _remap(ea), _remap(ei)), ior)


def od_complement(L, ior, alpha, cos):
    ei, ea, ec = _clamp_index(_ior_index(ior)), _clamp_index(np.sqrt(sat(alpha)) * 31.0), _clamp_index(sat(cos) * 31.0)
    s0 = np.floor(ei).astype(int)
    s1 = np.minimum(s0 + 1, 31)
    t = ei - s0
    u, v = _remap(ec), _remap(ea)
    v0, v1 = np.zeros(len(u)), np.zeros(len(u))
    for s in np.unique(np.concatenate([s0, s1])):
        m0, m1 = s0 == s, s1 == s
        if m0.any():
            v0[m0] = _tex2d(L.od_e[s], u[m0], v[m0])
        if m1.any():
            v1[m1] = _tex2d(L.od_e[s], u[m1], v[m1])
    return _extrapolate(v0 + t * (v1 - v0), ior)


def im_complement(L, alpha, cos):
    ea, ec = _clamp_index(np.sqrt(sat(alpha)) * 31.0), _clamp_index(sat(cos) * 31.0)
    return _tex2d(L.im_e, _remap(ec), _remap(ea))


def fuzz_ltc(L, roughness, cos):
    return _tex2d(L.ltc, sat(cos) * (31.0 / 32.0) + 0.5 / 32.0, sat(roughness) * (31.0 / 32.0) + 0.5 / 32.0)[:, :3]


def average_fresnel(eta):
    s = np.maximum(eta, 1.0e-4)
    return np.where(s > 1.0, (s - 1.0) / (4.08567 + 1.00071 * s), 0.997118 + 0.1014 * s - 0.965241 * s * s - 0.130607 * s * s * s)


def fresnel_dielectric(eta, cos):
    c = sat(cos)
    s2 = np.maximum(0.0, 1.0 - c * c)
    st2 = s2 / np.maximum(eta * eta, 1.0e-6)
    ct = np.sqrt(np.maximum(0.0, 1.0 - st2))
    rs = (c - eta * ct) / np.maximum(c + eta * ct, 1.0e-6)
    rp = (ct - eta * c) / np.maximum(ct + eta * c, 1.0e-6)
    return np.where(np.abs(eta - 1.0) <= 1.0e-6, 0.0, np.where(st2 >= 1.0, 1.0, 0.5 * (rs * rs + rp * rp)))


def ggx_dir_albedo(NdotV, alpha, F0, F90):
    """mx_ggx_dir_albedo_analytic (PBR.hlsli:8-25)"""
    x, y = NdotV, alpha
    x2, y2 = x * x, y * y
    c = np.array([[0.1003, 0.9345, 1.0, 1.0], [-0.6303, -2.323, -1.765, 0.2281], [9.748, 2.229, 8.263, 15.94], [-2.038, -3.748, 11.53, -55.83],
                  [29.34, 1.424, 28.96, 13.08], [-8.245, -0.7684, -7.507, 41.26], [-26.44, 1.436, -36.11, 54.9], [19.99, 0.2913, 15.86, 300.2],
                  [-5.448, 0.6286, 33.37, -285.1]])
    terms = [np.ones_like(x), x, y, x * y, x2, y2, x2 * y, x * y2, x2 * y2]
    r = sum(c[i][None, :] * terms[i][:, None] for i in range(9))
    A, B = sat(r[:, 0] / r[:, 2]), sat(r[:, 1] / r[:, 3])
    return F0 * A[:, None] + F90 * B[:, None]


def gtao_multi_bounce(visibility, albedo):
    a, b, c = 2.0404 * albedo - 0.3324, -4.7951 * albedo + 0.6417, 2.7552 * albedo + 0.6903
    v = visibility[:, None]
    return np.maximum(v, ((v * a + b) * v + c) * v)


# ------------------------------------------------------------------------------------------------ the surface and the term
def half4(words):
    """(n,) uint64 -> (n, 4) float64: four IEEE halves, x in the low bits"""
    return np.ascontiguousarray(words, dtype=np.uint64).view(np.float16).reshape(-1, 4).astype(f64)


def unorm4(words):
    return np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8).reshape(-1, 4).astype(f64) / 255.0


def surfaces_from_gbuffer(normals, albedo, mr, coat, emissive, fuzz, view, openpbr):
    """GetFragmentInfoScreenSpace + PopulateFragmentInfoFromOpenPBR (utilities.hlsli:2590-2709) for n pixels: the stored words, the unit vector
    towards the eye (n, 3), and the scene's OpenPBR records as (m, 100) float32 words."""
    normals, view = np.asarray(normals, dtype=f64).reshape(-1, 4), np.asarray(view, dtype=f64).reshape(-1, 3)
    al, m4, ct, fz = unorm4(albedo), unorm4(mr), half4(coat), half4(fuzz)
    op = np.asarray(openpbr, dtype=f32).reshape(-1, 100).astype(f64)
    idx = (normals[:, 3] + 0.5).astype(np.int64)
    idx = np.where(idx >= len(op), 0, idx)
    rec = op[idx]
    s = dict()
    nrm = normals[:, :3]
    ndv = np.einsum("ij,ij->i", nrm, view)
    N = nrm + np.maximum(0.0, -ndv + MIN_N_DOT_V)[:, None] * view
    s["N"] = N / np.linalg.norm(N, axis=1, keepdims=True)
    s["V"], s["NdotV"] = view, np.maximum(MIN_N_DOT_V, ndv)
    s["reflected"] = -view - 2.0 * s["N"] * np.einsum("ij,ij->i", -view, s["N"])[:, None]
    s["ao"] = al[:, 3]
    pr = np.clip(m4[:, 1], MIN_PERCEPTUAL_ROUGHNESS, 1.0)
    s["perceptualRoughness"], s["roughness"] = pr, pr * pr
    metal = m4[:, 0]
    baseWeight, specularWeight, specularColor = sat(rec[:, 0]), sat(rec[:, 15]), sat(rec[:, 16:19])
    wbc = sat(al[:, :3] * baseWeight[:, None])
    f0 = np.minimum(ior_to_f0(rec[:, 21]) * sat(specularWeight), 0.9999)
    sq = np.sqrt(np.minimum(sat(f0), 0.9999))
    s["weightedSpecularIor"] = (1.0 + sq) / np.maximum(1.0 - sq, 1.0e-4)
    s["dielectricSpecularF0"] = sat(specularColor * ior_to_f0(s["weightedSpecularIor"])[:, None])
    cpr = np.clip(m4[:, 2], MIN_PERCEPTUAL_ROUGHNESS, 1.0)
    s["coatPerceptualRoughness"], s["coatRoughness"] = cpr, cpr * cpr
    s["dielectricSpecularWeight"], s["metalSpecularWeight"] = sat(1.0 - metal), sat(metal * specularWeight)
    s["metalSpecularF0"] = sat(wbc * specularColor)
    om = 1.0 - 1.0 / 7.0       # OpenPBRMetalAverageFresnelWithF82Tint
    bfac = (wbc + (1.0 - wbc) * om ** 5) * (1.0 - specularColor) / np.maximum((1.0 / 7.0) * om ** 6, 1.0e-6)
    s["metalAverageFresnel"] = sat(wbc + (1.0 - wbc) / 21.0 - bfac / 126.0)
    s["albedo"], s["diffuseColor"] = wbc, wbc * (1.0 - metal)[:, None]
    s["coatWeight"], s["coatColor"] = sat(ct[:, 3]), sat(ct[:, :3])
    s["coatIor"], s["coatDarkening"] = rec[:, 30], sat(rec[:, 31])
    s["coatF0"] = sat(s["coatColor"] * ior_to_f0(s["coatIor"])[:, None])
    s["fuzzWeight"], s["fuzzColor"], s["fuzzRoughness"] = sat(m4[:, 3]), sat(fz[:, :3]), sat(fz[:, 3])
    s["baseDiffuseRoughness"] = sat(rec[:, 4])
    s["emissive"] = half4(emissive)[:, :3]
    return s


def pixel_class(s):
    return (s["coatWeight"] != 0).astype(int) | ((s["fuzzWeight"] != 0).astype(int) << 1)


def coat_reflected(L, s, NdotX):
    presence, ior, alpha = sat(s["coatWeight"]), np.maximum(np.maximum(s["coatIor"], 1.0), 1.0e-4), sat(s["coatRoughness"])
    refl = np.where(alpha <= 0.0, fresnel_dielectric(ior, sat(NdotX)), 1.0 - od_complement(L, ior, alpha, sat(NdotX)))
    return sat(presence * refl)


def coat_scale_incoming(L, s, NdotV):
    """OpenPBRCoatBaseLayerScaleIncoming with MakeOpenPBRCoatLayerState / OpenPBRComputeCoatExtraBaseLayerScale (IBL.hlsli:576-654)"""
    tint, presence, ior = sat(s["coatColor"]), sat(s["coatWeight"]), np.maximum(s["coatIor"], 1.0)
    Ks = average_fresnel(ior)
    Kr = 1.0 - (1.0 - Ks) / np.maximum(ior * ior, 1.0e-4)
    ds = average_fresnel(np.maximum(s["weightedSpecularIor"], 1.0))
    dw, mw = sat(s["dielectricSpecularWeight"]), sat(s["metalSpecularWeight"])
    spec_base = sat(dw * ds + (1.0 - dw))
    eff = 1.0 + spec_base * (np.sqrt(sat(s["roughness"])) - 1.0)
    K = Ks + eff * (Kr - Ks)
    wbc = sat(s["albedo"])
    Eb = sat(mw[:, None] * sat(s["metalAverageFresnel"]) + dw[:, None] * (wbc + ds[:, None] * (1.0 - wbc)))
    Delta = (1.0 - K)[:, None] / np.maximum(1.0 - Eb * K[:, None], 1.0e-4)
    mod = (sat(presence) * sat(s["coatDarkening"]))[:, None]
    extra = 1.0 + mod * (sat(Delta) - 1.0)
    c = sat(NdotV)
    eta = 1.0 / ior
    rc = np.sqrt(np.maximum(0.0, 1.0 - (1.0 - c * c) / np.maximum(eta * eta, 1.0e-4)))
    dist = 1.0 / np.maximum(rc, 1.0e-4)
    with np.errstate(all="ignore"):
        along = np.power(np.sqrt(tint), dist[:, None])
    passage = 1.0 + presence[:, None] * (along - 1.0)
    passage = np.where(((c <= 0.0) | (tint.min(axis=1) >= 1.0))[:, None], 1.0, passage)
    return passage * (1.0 - coat_reflected(L, s, NdotV))[:, None] * extra


def evaluate_ibl(s, L, env_faces, sh_coefficients, specular):
    """evaluateIBL (IBL.hlsli:683-740) in float64 -> dict(Fd, Fr, coatFr, fuzzFr) of (n, 3): diffuseAO = albedo.a, bentNormal = normalWS,
    the specular ambient occlusion is SpecularAO_Lagarde (the `#if` at :65 compares two undefined names, 0 == 0)."""
    N, NdotV, alpha = s["N"], s["NdotV"], s["roughness"]
    r = s["reflected"] + (alpha * alpha)[:, None] * (N - s["reflected"])
    zero = np.zeros_like(N)
    lookup = lambda rough: sample_cube(env_faces, r, rough * float(PREFILTER_LEVELS - 1), f64)[:, :3]
    spec_rad = lookup(s["perceptualRoughness"]) if specular else zero
    fuzz_rad = lookup(s["fuzzRoughness"]) if specular else zero
    n2 = N + N
    n2 = n2 / np.linalg.norm(n2, axis=1, keepdims=True)
    irr = np.maximum(irradiance_sh(sh_coefficients, n2), 0.0) * (1.0 / PI_SHADER)
    ior = np.maximum(s["weightedSpecularIor"], 1.0)
    avg = od_average(L, ior, sat(alpha))
    cached = np.maximum(0.0, od_complement(L, ior, sat(alpha), sat(NdotV)) / np.maximum(avg, 1.0e-12))
    comp = np.maximum(0.0, cached * avg)
    fon_a = 0.5 - 2.0 / (3.0 * PI_SHADER)
    mc = 1.0 - sat(NdotV)
    g = mc * (0.0571085289 + mc * (0.491881867 + mc * (-0.332181442 + mc * 0.0714429953)))
    rough = sat(s["baseDiffuseRoughness"])
    dir_albedo = (1.0 + rough * g) / (1.0 + fon_a * rough)
    one = np.ones_like(N)
    dielE = ggx_dir_albedo(NdotV, sat(alpha), sat(s["dielectricSpecularF0"]), one)
    metalE = ggx_dir_albedo(NdotV, sat(alpha), sat(s["metalSpecularF0"]), one)
    mms = im_complement(L, sat(alpha), NdotV)
    dw, mw = sat(s["dielectricSpecularWeight"]), sat(s["metalSpecularWeight"])
    maf = sat(s["metalAverageFresnel"])
    ms_scale = mw[:, None] * maf * maf
    Fd = s["diffuseColor"] * irr * dir_albedo[:, None] * comp[:, None] * s["ao"][:, None]
    Fr = (dw[:, None] * dielE + mw[:, None] * metalE + ms_scale * mms[:, None]) * spec_rad
    view_reflected = sat(sat(s["fuzzWeight"]) * sat(fuzz_ltc(L, s["fuzzRoughness"], NdotV)[:, 2]))
    fuzz_scale = 1.0 - view_reflected
    coat_att = coat_scale_incoming(L, s, NdotV)
    fuzzFr = view_reflected[:, None] * sat(s["fuzzColor"]) * fuzz_rad
    coatFr = zero.copy()
    if specular:
        has = sat(s["coatWeight"]) > 0.0
        coatFr = np.where(has[:, None], coat_reflected(L, s, NdotV)[:, None] * lookup(s["coatPerceptualRoughness"]), 0.0)
    base_att = fuzz_scale[:, None] * coat_att
    Fd, Fr, coatFr = Fd * base_att, Fr * base_att, coatFr * fuzz_scale[:, None]
    Fd = Fd * gtao_multi_bounce(s["ao"], s["diffuseColor"])
    if specular:
        sao = sat(np.power(NdotV + s["ao"], np.exp2(-16.0 * alpha - 1.0)) - 1.0 + s["ao"])
        Fr, coatFr, fuzzFr = Fr * gtao_multi_bounce(sao, s["dielectricSpecularF0"]), coatFr * gtao_multi_bounce(sao, s["coatF0"]), fuzzFr * gtao_multi_bounce(sao, s["fuzzColor"])
    return dict(Fd=Fd, Fr=Fr, coatFr=coatFr, fuzzFr=fuzzFr)


def term(s, L, env, specular=True):
    """(diffuse, specular) = (Fd, Fr + coatFr + fuzzFr) for an environment.Environment"""
    t = evaluate_ibl(s, L, env.faces, fold_sh(env.sh, env.scale), specular)
    return t["Fd"], t["Fr"] + t["coatFr"] + t["fuzzFr"]
