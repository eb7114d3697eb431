"""Image-based lighting, CPU side (`-m "not gpu"`): the data contract, the refusals that need no GPU, and the restatement of tests/ibl_ref.py held
to independent statements -- the face mapping to its inverse, the generator's coefficients to closed forms and to a quadrature, the float64 term to
the cases whose answer is known."""
import ctypes as C
import os

import numpy as np

import ibl_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def special_directions():
    """The 26 axis, edge and corner directions of the cube"""
    g = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], dtype=np.float64)
    assert len(g) == 26
    return g


def test_environment_info_layout_and_exports():
    """brmi_environment_info is the reference's EnvironmentInfo byte for byte (ShaderBuffers.h:453-459), and the library exports the new entry points."""
    from basicrenderer_amd import capi
    E = capi.EnvironmentInfo
    assert C.sizeof(E) == 128
    assert (E.cubeMapDescriptorIndex.offset, E.prefilteredCubemapDescriptorIndex.offset, E.sphericalHarmonicsScale.offset, E.sphericalHarmonics.offset, E.pad.offset) == (0, 4, 8, 12, 120)
    header = open(os.path.join(ROOT, "include", "brmi_types.h")).read()
    body = header[header.index("typedef struct brmi_environment_info {"): header.index("} brmi_environment_info;")]
    fields = [l.split()[1].rstrip(";") for l in body.splitlines()[1:] if l.strip()]
    assert fields == ["cubeMapDescriptorIndex", "prefilteredCubemapDescriptorIndex", "sphericalHarmonicsScale", "sphericalHarmonics[27]", "pad[2]"]
    assert "#define BRMI_SH_FLOAT_SCALE 100" in header and capi.SH_FLOAT_SCALE == 100
    lib = capi.brmi_lib()
    for name in ("brmi_set_environment", "brmi_debug_ibl", "brmi_debug_ibl_lookup"):
        assert hasattr(lib, name), name
    assert capi.PER_FRAME_ACTIVE_ENVIRONMENT_WORD + 1 == capi.PER_FRAME_OUTPUT_TYPE_WORD      # activeEnvironmentIndex sits in front of outputType


def test_set_environment_refuses_bad_bindings_without_a_gpu():
    from basicrenderer_amd import capi
    lib = capi.brmi_lib()
    cfg, h = capi.Config(), capi.vp()
    lib.brmi_default_config(C.byref(cfg), 64, 64)
    assert lib.brmi_create(C.byref(cfg), C.byref(h)) == 0
    try:
        table = (C.c_uint8 * 1024)()      # host memory standing in for the tables: the binding itself reads nothing
        b = capi.EnvironmentBuffers()
        b.structSize, b.environments, b.environmentCount, b.cubemaps, b.cubemapCount = C.sizeof(capi.EnvironmentBuffers) - 8, C.addressof(table), 1, C.addressof(table), 1
        assert lib.brmi_set_environment(h, C.byref(b)) == -1 and b"structSize" in lib.brmi_last_error(h)
        b.structSize = C.sizeof(capi.EnvironmentBuffers)
        b.environments = None
        assert lib.brmi_set_environment(h, C.byref(b)) == -1 and b"null table" in lib.brmi_last_error(h)
        b.environments, b.cubemaps = C.addressof(table), None
        assert lib.brmi_set_environment(h, C.byref(b)) == -1 and b"null table" in lib.brmi_last_error(h)
        b.cubemaps, b.environmentCount = C.addressof(table), 0
        assert lib.brmi_set_environment(h, C.byref(b)) == -1 and b"environmentCount is 0" in lib.brmi_last_error(h)
        b.environmentCount = 1
        assert lib.brmi_set_environment(h, C.byref(b)) == 0
        assert lib.brmi_set_environment(h, None) == 0
        assert lib.brmi_set_environment(None, None) == -1
        assert lib.brmi_debug_ibl_lookup(None, 0, None, None, None, 1, None) == -1
    finally:
        lib.brmi_destroy(h)


def test_face_mapping_round_trips_and_ties_follow_the_rule():
    """direction -> (face, u, v) -> the direction through that texel -> the same face and (u, v) within fp32 rounding; on the 26 axis, edge and corner
    directions the tie rule (X over Y over Z on equal magnitudes) decides the face."""
    rng = np.random.default_rng(11)
    d = rng.normal(size=(10000, 3)) * np.exp(rng.uniform(-20, 20, size=(10000, 1)))
    d = np.concatenate([d, special_directions()]).astype(np.float32)
    face, u, v = ibl_ref.cube_face_uv(d)
    assert ((u >= 0) & (u <= 1) & (v >= 0) & (v <= 1)).all()
    back = ibl_ref.direction_of(face, u, v)
    # the same point of the cube: d / |major| is `back` up to the rounding of two divisions and two half-sums (2 ulp of a value in [0, 1] each)
    major = np.abs(d.astype(np.float64)).max(axis=1, keepdims=True)
    assert np.abs(d.astype(np.float64) / major - back).max() <= 4 * 2.0 ** -23
    face2, u2, v2 = ibl_ref.cube_face_uv(back.astype(np.float32))
    interior = (np.abs(back).max(axis=1, keepdims=True) - np.sort(np.abs(back), axis=1)[:, 1:2] > 1e-6)[:, 0]      # off the edges, where a rounding cannot change the face
    assert (face2 == face)[interior].all()
    assert np.abs(u2 - u)[interior].max() <= 2.0 ** -22 and np.abs(v2 - v)[interior].max() <= 2.0 ** -22
    for s, f in zip(special_directions(), ibl_ref.cube_face_uv(special_directions().astype(np.float32))[0]):
        a = np.abs(s)
        want = (1 if s[0] < 0 else 0) if a[0] >= a[1] and a[0] >= a[2] else (3 if s[1] < 0 else 2) if a[1] >= a[2] else (5 if s[2] < 0 else 4)
        assert f == want, (s, f, want)
    assert tuple(ibl_ref.cube_face_uv(np.float32([[1, 1, 1]]))[0]) == (0,) and tuple(ibl_ref.cube_face_uv(np.float32([[0, -1, 1]]))[0]) == (3,)
    # the directions the definition sets aside
    bad = np.float32([[0, 0, 0], [np.nan, 1, 0], [1, np.inf, 0], [0, 0, -np.inf], [-0.0, 0.0, -0.0]])
    face, u, v = ibl_ref.cube_face_uv(bad)
    assert (face == 0).all() and (u == 0.5).all() and (v == 0.5).all()
    # the generator's texel centres are the lookup's: every texel of every face reads back as itself
    from basicrenderer_amd import environment
    dirs = environment.face_directions(4)
    for f in range(6):
        ff, uu, vv = ibl_ref.cube_face_uv(dirs[f].reshape(-1, 3).astype(np.float32))
        assert (ff == f).all()
        centre = (np.arange(4) + 0.5) / 4
        assert np.abs(uu.reshape(4, 4) - centre[None, :]).max() < 1e-6 and np.abs(vv.reshape(4, 4) - centre[:, None]).max() < 1e-6


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def test_generator_coefficients_and_mips():
    """irradianceSH(n) / pi is the cosine-convolved radiance: the constant itself for a constant environment, the closed form of the polynomial for the
    procedural one (and a quadrature of the integral says the closed form is the integral), both within the quantisation 9 * 0.5 * scale / 100, which the
    generator keeps below 1e-4 of the largest radiance.  The mips of a constant environment are that constant."""
    from basicrenderer_amd import environment
    rng = np.random.default_rng(5)
    n = _unit(rng, 1000)
    c = np.array([0.25, 0.5, 0.75])
    env = environment.Environment.constant(c, size=8)
    bound = 9 * 0.5 * env.scale / 100
    assert bound < 1e-4 * c.max()
    assert np.abs(ibl_ref.irradiance_sh(ibl_ref.fold_sh(env.sh, env.scale), n) / np.pi - c).max() <= bound
    code = np.rint(c * 255).astype(np.uint8)
    for f in env.faces:
        assert len(f) == 4
        for level in f:
            assert (level[..., :3] == code).all() and (level[..., 3] == 255).all()

    env = environment.Environment.procedural(16)
    p = env.radiance
    L = p(environment.face_directions(16))
    assert L.min() > 0 and L.max() <= 1
    bound = 9 * 0.5 * env.scale / 100
    assert bound < 1e-4 * L.max()
    # the closed form, stated here on its own: bands 0, 1, 2 of L come through the clamped cosine times 1, 2/3, 1/4 (after the division by pi)
    tr = np.einsum("iic->c", p.Q)
    Qt = p.Q - np.eye(3)[:, :, None] * tr / 3
    want = p.c0 + tr / 3 + (2.0 / 3.0) * n @ p.a + 0.25 * np.einsum("ni,nj,ijc->nc", n, n, Qt)
    got = ibl_ref.irradiance_sh(ibl_ref.fold_sh(env.sh, env.scale), n) / np.pi
    assert np.abs(got - want).max() <= bound
    # ... and the integral itself for a few normals: (1 / pi) * integral of L(w) max(0, n.w) over the sphere, midpoint rule on a (theta, phi) grid
    T, P = 400, 800
    th, ph = (np.arange(T) + 0.5) * np.pi / T, (np.arange(P) + 0.5) * 2 * np.pi / P
    w = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones(P)), np.outer(np.sin(th), np.sin(ph))], -1).reshape(-1, 3)
    dw = (np.outer(np.sin(th), np.ones(P)) * (np.pi / T) * (2 * np.pi / P)).reshape(-1)
    Lw = p(w)
    for k in range(6):
        E = (Lw * (np.maximum(0.0, w @ n[k]) * dw)[:, None]).sum(axis=0) / np.pi
        assert np.abs(E - want[k]).max() < 2e-5, (k, E, want[k])
    # the faces are the radiance at the texel centres, the mips box filters of the linear values
    assert np.abs(env.faces[2][0][..., :3] / 255.0 - L[2]).max() <= 0.5 / 255 + 1e-12
    assert [l.shape[0] for l in env.faces[0]] == [16, 8, 4, 2, 1]
    lin = env.faces[4][0].astype(np.float64) / 255
    box = 0.25 * (lin[0::2, 0::2] + lin[1::2, 0::2] + lin[0::2, 1::2] + lin[1::2, 1::2])
    assert np.abs(env.faces[4][1] / 255.0 - box).max() <= 0.5 / 255 + 1e-12


def _surfaces(rng, n, scene, layered):
    """n made-up pixels over the scene's OpenPBR records; layered: give them coat and fuzz weights"""
    op = scene.arrays["openpbrMaterials"].view(np.float32).reshape(-1, 100)
    V = _unit(rng, n)
    nrm = _unit(rng, n)
    normals = np.concatenate([nrm, rng.integers(0, len(op), size=(n, 1)).astype(np.float64)], 1).astype(np.float32)
    albedo = rng.integers(0, 256, size=(n, 4), dtype=np.uint8).view(np.uint32).reshape(-1)
    mr = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    coat = rng.uniform(0, 1, size=(n, 4)).astype(np.float16)
    fuzz = rng.uniform(0, 1, size=(n, 4)).astype(np.float16)
    if not layered:
        mr[:, 3] = 0
        coat[:, 3] = 0
    emissive = np.zeros((n, 4), dtype=np.float16)
    return ibl_ref.surfaces_from_gbuffer(normals, albedo, mr.view(np.uint32).reshape(-1), coat.view(np.uint64).reshape(-1), emissive.view(np.uint64).reshape(-1),
                                         fuzz.view(np.uint64).reshape(-1), V.astype(np.float32), op)


def test_float64_term_sanity(scenes):
    from basicrenderer_amd import environment
    scene = scenes("tiny_coat_fuzz")
    L = ibl_ref.Luts(scene.arrays)
    rng = np.random.default_rng(3)
    sky = environment.Environment.procedural(16)
    s = _surfaces(rng, 512, scene, layered=True)
    # no ambient occlusion left: no diffuse term
    s0 = dict(s); s0["ao"] = np.zeros_like(s["ao"])
    assert (ibl_ref.evaluate_ibl(s0, L, sky.faces, ibl_ref.fold_sh(sky.sh, sky.scale), True)["Fd"] == 0).all()
    # a constant environment without the specular part: nothing depends on the reflection vector
    const = environment.Environment.constant([0.3, 0.6, 0.9])
    k = ibl_ref.fold_sh(const.sh, const.scale)
    a = ibl_ref.evaluate_ibl(s, L, const.faces, k, False)
    s1 = dict(s); s1["reflected"] = _unit(rng, 512)
    b = ibl_ref.evaluate_ibl(s1, L, const.faces, k, False)
    assert all((a[key] == b[key]).all() for key in a) and (a["Fr"] == 0).all() and (a["coatFr"] == 0).all() and (a["fuzzFr"] == 0).all()
    assert (a["Fd"] > 0).any()
    # ... and with it, the lookups of a constant cube return the constant whatever the direction
    a, b = (ibl_ref.evaluate_ibl(x, L, const.faces, k, True) for x in (s, s1))
    assert all(np.abs(a[key] - b[key]).max() <= 1e-15 for key in a) and (a["Fr"] > 0).any()
    # plain surfaces: the coat and fuzz addends are exactly 0 and their factors exactly 1
    p = _surfaces(rng, 512, scene, layered=False)
    assert (ibl_ref.pixel_class(p) == 0).all()
    t = ibl_ref.evaluate_ibl(p, L, sky.faces, ibl_ref.fold_sh(sky.sh, sky.scale), True)
    assert (t["coatFr"] == 0).all() and (t["fuzzFr"] == 0).all() and (t["Fr"] > 0).any()
    assert (ibl_ref.coat_scale_incoming(L, p, p["NdotV"]) == 1.0).all()
    assert (ibl_ref.fuzz_ltc(L, p["fuzzRoughness"], p["NdotV"])[:, 2] * p["fuzzWeight"] == 0).all()
    assert (ibl_ref.pixel_class(s) == 3).any()
