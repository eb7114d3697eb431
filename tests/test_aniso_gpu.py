"""Anisotropic filtering on the GPU (brmi_set_sampler_anisotropy / brmi_debug_sample_grad).

1  the sampler itself, through the debug entry point that calls the device function the G-buffer kernel calls, bit for bit against tests/aniso_ref.py;
2  the ANISO instantiations with every sampler at 1 (N = 1 in every lane): the oracle's frames, held as tests/test_parity_gpu.py holds them;
3  every sampler at 16: only texture-sampled pixels move, both G-buffer forms agree, switching it off or a second brmi_set_scene restores the oracle's frame;
4  refusals.
What no test here sees is a frame-level comparison of an A > 1 G-buffer with an oracle: the oracle is isotropic.
"""
import ctypes as C

import numpy as np
import pytest

import aniso_ref

pytestmark = pytest.mark.gpu
f32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
N_SAMPLES = 8192

# (addressU, addressV, min, mag, mip, mipLodBias, minLod, maxLod); 0 wrap 1 mirror 2 clamp; 0 point 1 linear
SAMPLERS = [(0, 0, 1, 1, 1, 0.0, 0.0, 1000.0),          # wrap, trilinear
            (1, 2, 1, 1, 1, 0.75, 0.0, 1000.0),         # mirror / clamp, biased up
            (2, 1, 1, 1, 0, -0.75, 0.0, 1000.0),        # clamp / mirror, nearest mip, biased down
            (0, 0, 0, 0, 0, 0.0, 0.0, 1000.0),          # all point
            (0, 1, 0, 1, 1, 0.0, 1.5, 3.25),            # point min, linear mag, a LOD window that clips
            (0, 0, 1, 1, 1, 0.0, 0.0, 1000.0)]
TABLES = {"1": [1] * 6, "2": [2] * 6, "5": [5] * 6, "16": [16] * 6, "mixed": [16, 5, 2, 16, 5, 1]}
TEXTURES = {"pow2_256x64_srgb": (256, 64, True), "npot_100x60_unorm": (100, 60, False), "pow2_16x16_unorm": (16, 16, False), "npot_37x21_srgb": (37, 21, True)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _major2(W, H, ddx, ddy):
    with np.errstate(all="ignore"):
        dxx, dxy, dyx, dyy = ddx[:, 0] * f32(W), ddx[:, 1] * f32(H), ddy[:, 0] * f32(W), ddy[:, 1] * f32(H)
        lx2, ly2 = dxx * dxx + dxy * dxy, dyx * dyx + dyy * dyy
        return np.where(lx2 > ly2, lx2, ly2), lx2, ly2


def _stream(W, H, seed):
    """8,192 samples = 128 waves of 64 consecutive lanes.  Waves 0-47: every lane its own tap count, N = 1 .. 16 inside one wave (equal axes, then ratios 1.6 .. 18.6 of a rotated
    footprint, widths from a hundredth of a texel to beyond the whole chain, so that the 1 x 1 level is reached); waves 48-63: every lane N = 1 (equal axes); waves 64-79:
    every lane at ratio >= 16; waves 80-119: random gradient pairs; waves 120-127: the guards' inputs mixed into ordinary lanes."""
    rng = np.random.default_rng(seed)
    n = N_SAMPLES
    uv = rng.uniform(-3.0, 4.0, (n, 2)).astype(f32)
    lane = np.arange(n) % 64
    wave = np.arange(n) // 64
    ang = rng.uniform(0, 2 * np.pi, n)
    width = np.exp2(rng.uniform(-6.0, 7.0, n))            # minor axis in texels
    ratio = np.where(wave < 48, 1.1 + (lane % 32) * 0.56 + rng.uniform(0, 0.2, n), rng.uniform(16.0, 40.0, n))
    minor = np.stack([np.cos(ang), np.sin(ang)], 1) * width[:, None]
    major = np.stack([-np.sin(ang), np.cos(ang)], 1) * (width * ratio)[:, None]
    swap = rng.integers(0, 2, n).astype(bool)[:, None]
    size = np.array([W, H], dtype=np.float64)
    ddx = (np.where(swap, major, minor) / size).astype(f32)
    ddy = (np.where(swap, minor, major) / size).astype(f32)
    eq = ((wave >= 48) & (wave < 64)) | ((wave < 48) & (lane % 32 == 0))
    ddy[eq] = np.where(rng.integers(0, 2, (int(eq.sum()), 1)).astype(bool), ddx[eq], -ddx[eq])
    rnd = (wave >= 80) & (wave < 120)
    k = int(rnd.sum())
    ddx[rnd] = (rng.normal(0, 1, (k, 2)) * np.exp2(rng.uniform(-12, 1, (k, 1)))).astype(f32)
    ddy[rnd] = (rng.normal(0, 1, (k, 2)) * np.exp2(rng.uniform(-12, 1, (k, 1)))).astype(f32)
    # the guards' inputs, in the lanes of the last eight waves that are a multiple of three
    slots = iter(np.flatnonzero((wave >= 120) & (lane % 3 == 0)))

    def put(gx, gy, at_uv=None):
        i = next(slots)
        ddx[i], ddy[i] = np.asarray(gx, dtype=f32), np.asarray(gy, dtype=f32)
        if at_uv is not None:
            uv[i] = np.asarray(at_uv, dtype=f32)

    for _ in range(4):
        put((0, 0), (0, 0))
        put((0, 0), (0.01, 0.003)); put((0.02, -0.01), (0, 0))                       # one zero axis
        put((1e-40, 0), (0, 3e-41)); put((1e-41, 2e-42), (0.05, 0.0))                # denormal gradients
        put((np.inf, 0), (0.01, 0)); put((0.01, 0.01), (0, -np.inf)); put((np.inf, np.inf), (np.inf, 0))
        put((np.nan, 0), (0.01, 0)); put((0.01, 0), (0, np.nan)); put((np.nan, np.nan), (np.nan, np.nan)); put((0.3, 0.01), (np.nan, 0.001))
    for bound in (1.17549435e-38, 3.0e38):                                           # major2 just inside and just outside both bounds: a run of consecutive floats across each
        g = f32(np.sqrt(bound) / W)
        lo = g
        for _ in range(24):
            lo = np.nextafter(lo, f32(0))
        v = lo
        for k in range(48):
            if k % 2:
                put((v, 0), (0, 0))
            else:
                put((0, 0), (v, 0))
            v = np.nextafter(v, f32(np.inf))
    for m in (1.0e6, -1.0e6, 65536.5, -99999.25, 1.0e5):                             # |uv| up to 1e6, with an anisotropic footprint
        put((2.0 / W, 0), (0, 11.0 / H), at_uv=(m, -m * 0.5))
        put((0.3 / W, 0.1 / H), (-0.4 / H, 1.9 / H), at_uv=(0.25, m))
    return uv, ddx, ddy


def _assert_stream_has_every_class(W, H, uv, ddx, ddy):
    major2, lx2, ly2 = _major2(W, H, ddx, ddy)
    N, _, _ = aniso_ref.plan(W, H, ddx, ddy, 16)
    per_wave = N.reshape(-1, 64)
    assert any(set(range(1, 17)) <= set(w.tolist()) for w in per_wave), "no wave holds lanes with N from 1 to 16"
    assert (per_wave == 1).all(axis=1).any() and (per_wave == 16).all(axis=1).any(), "waves with every lane at N = 1 and with every lane at N = 16"
    zero_x, zero_y = (ddx == 0).all(axis=1), (ddy == 0).all(axis=1)
    assert (zero_x & zero_y).any() and (zero_x & ~zero_y & np.isfinite(ddy).all(axis=1)).any() and (zero_y & ~zero_x & np.isfinite(ddx).all(axis=1)).any()
    g = np.concatenate([ddx, ddy], axis=1)
    tiny = f32(1.17549435e-38)
    assert ((np.abs(g) > 0) & (np.abs(g) < tiny)).any() and np.isinf(g).any() and np.isnan(g).any()
    assert np.isnan(lx2).any() and np.isnan(ly2).any()
    lo, hi = tiny, f32(3.0e38)
    with np.errstate(all="ignore"):
        assert ((major2 >= lo) & (major2 < lo * f32(1.0001))).any() and ((major2 < lo) & (major2 > lo * f32(0.9999))).any(), "major2 on both sides of the lower bound"
        assert ((major2 <= hi) & (major2 > hi * f32(0.9999))).any() and ((major2 > hi) & (major2 < hi * f32(1.0001))).any(), "major2 on both sides of the upper bound"
    assert (np.abs(uv).max(axis=1) >= 1.0e6).any() and (N[np.abs(uv).max(axis=1) >= 1.0e5] > 1).any()


@pytest.fixture(scope="module")
def sampler_rig():
    """the four textures and six samplers in host memory (for the oracle's hooks) and in HBM in the scene library's layout"""
    import torch
    from basicrenderer_amd import capi
    rng = np.random.default_rng(7)
    tex = [dict(levels=aniso_ref.box_chain(rng.integers(0, 256, (h, w, 4), dtype=np.uint8)), srgb=srgb) for (w, h, srgb) in TEXTURES.values()]
    assert tex[0]["levels"][-1].shape[:2] == (1, 1) and len(tex[0]["levels"]) == 9
    sb, keep = aniso_ref.make_scene_buffers(tex, SAMPLERS)
    dev = "cuda:0"
    texels = torch.from_numpy(keep["texels"]).to(dev)
    descs = keep["descs"].copy()
    descs.view(np.uint64).reshape(len(tex), 12)[:, 0] += np.uint64(texels.data_ptr())
    d_descs = torch.from_numpy(descs.view(np.int32)).to(dev)
    d_samp = torch.from_numpy(keep["samplers"].view(np.int32)).to(dev)
    d_srgb = torch.from_numpy(keep["srgb"]).to(dev)
    dsb = capi.SceneBuffers()
    dsb.textures, dsb.textureCount = d_descs.data_ptr(), len(tex)
    dsb.samplers, dsb.samplerCount = d_samp.data_ptr(), len(SAMPLERS)
    dsb.srgbToLinear = d_srgb.data_ptr()
    tables = {k: torch.from_numpy(np.array(v, dtype=np.uint32).view(np.int32)).to(dev) for k, v in TABLES.items()}
    yield dict(host=aniso_ref.Sampler(sb), keep=(keep, texels, d_descs, d_samp, d_srgb), dsb=dsb, tables=tables, lib=capi.brmi_lib(), torch=torch, dev=dev)


@pytest.mark.parametrize("texture", list(TEXTURES))
def test_sampler_is_the_reference_bit_for_bit(texture, sampler_rig):
    """brmi_debug_sample_grad against aniso_ref on 8,192 samples per (texture, sampler, maxAnisotropy table, binding form); four channels as bit patterns, no sample left out."""
    rig, torch = sampler_rig, sampler_rig["torch"]
    t = list(TEXTURES).index(texture)
    W, H, _ = TEXTURES[texture]
    uv, ddx, ddy = _stream(W, H, seed=100 + t)
    _assert_stream_has_every_class(W, H, uv, ddx, ddy)
    d_uv, d_dx, d_dy = (torch.from_numpy(a).to(rig["dev"]) for a in (uv, ddx, ddy))
    out = torch.zeros((N_SAMPLES, 4), dtype=torch.float32, device=rig["dev"])
    iso = {s: rig["host"].sample_grad(t, s, uv, ddx, ddy) for s in range(len(SAMPLERS))}
    ref = {}
    for s in range(len(SAMPLERS)):
        for uniform in (0, 1):      # no table: today's sample_grad
            out.fill_(-1.0)
            assert rig["lib"].brmi_debug_sample_grad(C.byref(rig["dsb"]), None, t, s, uniform, d_uv.data_ptr(), d_dx.data_ptr(), d_dy.data_ptr(), out.data_ptr(), N_SAMPLES, None) == 0
            bad = (_bits(out.cpu().numpy()) != _bits(iso[s])).any(axis=1)
            assert not bad.any(), f"{texture} sampler {s} no table uniform={uniform}: {int(bad.sum())} samples differ from the oracle's SampleGrad, first {np.flatnonzero(bad)[:8]}"
        for name, table in TABLES.items():
            A = table[s]
            if (s, A) not in ref:
                ref[(s, A)] = rig["host"].sample_grad_aniso(t, s, W, H, uv, ddx, ddy, A, return_n=True)
            want, N = ref[(s, A)]
            if A == 1:
                assert np.array_equal(_bits(want), _bits(iso[s]))
            for uniform in (0, 1):
                out.fill_(-1.0)
                rc = rig["lib"].brmi_debug_sample_grad(C.byref(rig["dsb"]), rig["tables"][name].data_ptr(), t, s, uniform, d_uv.data_ptr(), d_dx.data_ptr(), d_dy.data_ptr(), out.data_ptr(), N_SAMPLES, None)
                assert rc == 0
                got = out.cpu().numpy()
                bad = (_bits(got) != _bits(want)).any(axis=1)
                assert not bad.any(), (f"{texture} sampler {s} table {name} (A = {A}) uniform={uniform}: {int(bad.sum())} of {N_SAMPLES} samples differ; first {np.flatnonzero(bad)[:8]}, "
                                       f"their N {N[bad][:8]}, got {got[bad][:2]}, want {want[bad][:2]}")
    # an unbound slot reads opaque white with and without a table
    for table in (None, rig["tables"]["16"].data_ptr()):
        out.fill_(-1.0)
        assert rig["lib"].brmi_debug_sample_grad(C.byref(rig["dsb"]), table, 99, 0, 1, d_uv.data_ptr(), d_dx.data_ptr(), d_dy.data_ptr(), out.data_ptr(), N_SAMPLES, None) == 0
        assert (out.cpu().numpy() == 1.0).all()


# ---- frames ------------------------------------------------------------------------------------------------------------------------------
def _scene_and_oracle(name, scenes, oracle_frames, cache={}):
    if name != "tiny_uv_sets_3":
        return scenes(name), oracle_frames(name)
    if name not in cache:
        import orc
        from conftest import Scene
        sc = Scene("tiny", 256, 144, material_features=256 | 8, lod_levels=2)
        cache[name] = (sc, orc.OracleFrame(sc).run())
    return cache[name]


@pytest.mark.parametrize("inline", [0, 1])
@pytest.mark.parametrize("name", ["tiny_textured", "tiny_parallax", "tiny_layer_textures_only", "tiny_uv_sets_3"])
def test_all_ones_runs_the_aniso_kernels_and_renders_the_oracles_frame(name, inline, scenes, oracle_frames):
    """set_anisotropy(1): the ANISO instantiations with N = 1 in every lane.  Lists, keys, depth and the seven planes bit-exact, HDR within one fp16 ULP
    (test_parity_gpu's own check), with the per-cluster tables and resolved in place."""
    from basicrenderer_amd.renderer import VisibilityRenderer
    from test_parity_gpu import _Env, _assert_frame_is_the_oracles, _capture
    sc, o = _scene_and_oracle(name, scenes, oracle_frames)
    with _Env(BRMI_RESOLVE_INLINE=inline):
        r = VisibilityRenderer(sc, stats=True)
    r.set_anisotropy(1)
    r.execute()
    _assert_frame_is_the_oracles(_capture(r), o, f"{name} resolve_inline={inline} anisotropy 1")
    r.close()


def _layout(struct):
    """{field: (first 32-bit word, words)} and the size in words of a record of include/brmi_types.h whose members are all uint32_t / float (arrays included), read
    from the header itself so that a layout change moves these offsets with it"""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "brmi_types.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, at = {}, 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(uint32_t|float)\s+(.*)$", decl, re.S)
        assert m, f"{struct}: a member that is not a 32-bit scalar: {decl!r}"
        for item in m.group(2).split(","):
            name, dims = re.match(r"\s*(\w+)((?:\[\w+\])*)\s*$", item).groups()
            words = int(np.prod([int(d) for d in re.findall(r"\[(\d+)\]", dims)])) if dims else 1
            fields[name] = (at, words)
            at += words
    return fields, at


def _material_bit(name):
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "brmi_types.h")).read()
    if name == "BRMI_MATERIAL_ANY_TEXTURE":
        expr = re.search(r"#define BRMI_MATERIAL_ANY_TEXTURE \((.*?)\)\n", text.replace("\\\n", " "), re.S).group(1)
        return sum(_material_bit(n.strip()) for n in expr.split("|"))
    return 1 << int(re.search(r"#define %s\s+\(1u << (\d+)\)" % name, text).group(1))


def _textured_pixels(sc, o):
    """per pixel: does its material sample a texture in the G-buffer pass -- from the oracle's keys and cluster list and the scene's host tables"""
    inst_f, inst_w = _layout("brmi_per_mesh_instance")
    mesh_f, mesh_w = _layout("brmi_per_mesh")
    mat_f, mat_w = _layout("brmi_material_info")
    op_f, op_w = _layout("brmi_openpbr_material_info")
    bind0 = op_f["textureBindings"][0]
    covered = o.vis != EMPTY
    cluster = ((o.vis >> np.uint64(7)) & np.uint64(0x3FFFFFF)).astype(np.int64)
    cluster[~covered] = 0
    instance = (o.clusters[: max(1, o.count), 0] >> 8)[cluster]
    per_mesh = sc.arrays["perMeshInstance"].view(np.uint32).reshape(-1, inst_w)[instance, inst_f["perMeshBufferIndex"][0]]
    material = sc.arrays["perMesh"].view(np.uint32).reshape(-1, mesh_w)[per_mesh, mesh_f["materialDataIndex"][0]]
    mats = sc.arrays["materials"].view(np.uint32).reshape(-1, mat_w)
    op = sc.arrays["openpbrMaterials"].view(np.uint32).reshape(-1, op_w)[:, bind0:bind0 + 12].reshape(-1, 6, 2)      # the six coat / fuzz (texture, sampler) pairs
    layer = ((op[:, :, 0] != 0xFFFFFFFF) & (op[:, :, 1] != 0xFFFFFFFF)).any(axis=1)
    textured = ((mats[:, mat_f["materialFlags"][0]] & _material_bit("BRMI_MATERIAL_ANY_TEXTURE")) != 0) | layer[mats[:, mat_f["openPBRMaterialDataIndex"][0]]]
    return covered, covered & textured[material]


@pytest.mark.parametrize("name", ["tiny_textured", "sponza_textured"])
def test_sixteen_moves_only_texture_sampled_pixels_and_can_be_switched_off(name, scenes, oracle_frames):
    from basicrenderer_amd import capi
    from basicrenderer_amd.renderer import VisibilityRenderer
    from test_parity_gpu import _Env, _assert_frame_is_the_oracles, _capture
    sc, o = scenes(name), oracle_frames(name)
    covered, textured = _textured_pixels(sc, o)
    assert textured.any() and (name != "tiny_textured" or (covered & ~textured).any())      # (every material of the Sponza-class scene samples a texture)
    planes = {}
    for inline in (0, 1):
        with _Env(BRMI_RESOLVE_INLINE=inline):
            r = VisibilityRenderer(sc, stats=True)
        r.set_anisotropy(16)
        r.execute()
        assert np.array_equal(r.visibility(), o.vis) and np.array_equal(r.depth().view(np.uint32), o.depth.view(np.uint32))
        g = r.gbuffer()
        assert np.array_equal(g["motion"], o.motion), "motion vectors"
        plain = covered & ~textured
        for key, ref in (("normals", o.normals), ("albedo", o.albedo), ("coat", o.coat), ("emissive", o.emissive), ("fuzz", o.fuzz), ("mr", o.mr)):
            a, b = g[key][plain], ref[plain]
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), f"{key} of pixels whose material samples no texture"
        moved = covered & (g["albedo"] != o.albedo)
        assert moved.any(), "sixteen taps changed no albedo"
        assert not (moved & ~textured).any()
        planes[inline] = g
        if inline == 0:
            r.set_anisotropy(None)                              # off: the oracle's frame again
            r.execute()
            _assert_frame_is_the_oracles(_capture(r), o, f"{name} after set_anisotropy(None)")
            r.set_anisotropy(16)                                # ... and a second brmi_set_scene forgets the binding
            r._check(r.lib.brmi_set_scene(r._h, C.byref(r.sb)), "brmi_set_scene")
            binds = (capi.ResourceBinding * len(r.descs))()
            for i, (rid, d) in enumerate(sorted(r.descs.items())):
                binds[i].id, binds[i].ptr, binds[i].bytes = rid, r.res[rid].data_ptr(), r.res[rid].numel()
            r._check(r.lib.brmi_setup(r._h, binds, len(r.descs), r._s()), "brmi_setup")
            r.update()
            r.execute()
            _assert_frame_is_the_oracles(_capture(r), o, f"{name} after a second brmi_set_scene")
        r.close()
    for key in planes[0]:                                       # the tables form and the in-place form agree bit for bit
        a, b = planes[0][key][covered], planes[1][key][covered]
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), key


def test_refusals(scenes):
    import torch
    from basicrenderer_amd import capi
    from basicrenderer_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(scenes("tiny_textured"), stats=True)
    count = int(r.sb.samplerCount)
    table = torch.ones(count + 1, dtype=torch.int32, device=r.device)
    assert r.lib.brmi_set_sampler_anisotropy(r._h, table.data_ptr(), count + 1) == -1      # BRMI_ERR_INVALID
    assert b"count" in r.lib.brmi_last_error(r._h) and b"brmi_set_sampler_anisotropy" in r.lib.brmi_last_error(r._h)
    assert r.lib.brmi_set_sampler_anisotropy(r._h, table.data_ptr(), count) == 0
    assert r.lib.brmi_set_sampler_anisotropy(r._h, None, 0) == 0
    with pytest.raises(Exception):
        r.set_anisotropy([1] * (count + 1))
    r.close()
    # before brmi_set_scene: the status brmi_set_streaming gives there
    lib = capi.brmi_lib()
    cfg = capi.Config()
    lib.brmi_default_config(C.byref(cfg), 64, 64)
    h = capi.vp()
    assert lib.brmi_create(C.byref(cfg), C.byref(h)) == 0
    b = capi.StreamingBuffers()
    b.structSize = C.sizeof(capi.StreamingBuffers)
    want = lib.brmi_set_streaming(h, C.byref(b))
    assert want != 0 and lib.brmi_set_sampler_anisotropy(h, table.data_ptr(), count) == want
    lib.brmi_destroy(h)
