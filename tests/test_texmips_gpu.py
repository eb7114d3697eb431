"""brmi_texmips_build / brmi_texmips_build_alpha on the GPU against tests/texmips_ref.py.

Texels of a linear chain, alpha channels, statistics words and scales: bit for bit.  rgb of an sRGB chain: bit for bit where the restatement's float64 value
is farther from a rounding cut than its derived bound, within one code elsewhere (texmips_ref.assert_chain_matches).
"""
import ctypes as C

import numpy as np
import pytest

import texmips_ref as T

pytestmark = pytest.mark.gpu
FILL, GUARD = 0xCD, 256      # bytes of every destination before a build; guard texels behind the chain


class Dev:
    def __init__(self):
        import torch
        from basicrenderer_amd import capi
        self.torch, self.capi, self.lib = torch, capi, capi.brmi_lib()
        self.device = torch.device("cuda:0")
        self.table = torch.from_numpy(T.srgb_table()).to(self.device)
        self.scratch = torch.zeros(4, dtype=torch.uint8, device=self.device)      # cleared once, here

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def chain(self, img, srgb, mips, offsets=None):
        """(descriptor, texel tensor): level 0 filled, everything else FILL"""
        h, w = img.shape[:2]
        offs, total = T.mip_offsets(w, h, mips)
        t = self.torch.full(((total + GUARD) * 4,), FILL, dtype=self.torch.uint8, device=self.device)
        t[: w * h * 4] = self.torch.from_numpy(img.reshape(-1).copy()).to(self.device)
        d = self.capi.TextureDesc()
        d.texels, d.width, d.height, d.mipCount = t.data_ptr(), w, h, mips
        d.format = self.capi.TEXTURE_FORMAT_RGBA8_UNORM_SRGB if srgb else self.capi.TEXTURE_FORMAT_RGBA8_UNORM
        for l, o in enumerate(offs if offsets is None else offsets):
            d.mipOffset[l] = o
        return d, t

    def plain(self, d, scratch=None):
        scratch = self.scratch if scratch is None else scratch
        return self.lib.brmi_texmips_build(C.byref(d), self.table.data_ptr(), scratch.data_ptr(), scratch.numel(), self.stream())

    def levels_of(self, t, w, h, mips):
        raw = t.cpu().numpy()
        offs, total = T.mip_offsets(w, h, mips)
        out = [raw[o * 4:(o + lw * lh) * 4].reshape(lh, lw, 4) for o, (lw, lh) in zip(offs, T.level_sizes(w, h, mips))]
        return out, raw[total * 4:]


@pytest.fixture(scope="module")
def dev():
    return Dev()


@pytest.fixture(scope="module")
def plain_refs():
    cache = {}

    def get(case, srgb):
        if (case, srgb) not in cache:
            w, h, mips, seed = case
            img = T.noise_image(w, h, seed)
            levels, decided = T.plain_chain(img, srgb, mips)
            T.assert_mostly_decided(decided)
            cache[(case, srgb)] = (img, levels, decided)
        return cache[(case, srgb)]
    return get


@pytest.mark.parametrize("srgb", [0, 1], ids=["linear", "srgb"])
@pytest.mark.parametrize("case", T.PLAIN_CASES, ids=[f"{c[0]}x{c[1]}m{c[2]}" for c in T.PLAIN_CASES])
def test_plain_chain_equals_the_restatement(dev, plain_refs, case, srgb):
    w, h, mips, _ = case
    img, levels, decided = plain_refs(case, srgb)
    d, t = dev.chain(img, srgb, mips)
    assert dev.plain(d) == 0, dev.lib.brmi_last_error(None)
    dev.torch.cuda.synchronize()
    got, guard = dev.levels_of(t, w, h, mips)
    assert np.array_equal(got[0], img), "level 0 was written"
    assert (guard == FILL).all(), "the guard behind the chain was written"
    T.assert_chain_matches(got, levels, decided, f"{w}x{h}")
    # every texel of every requested level is written: a texel the build skipped would still hold FILL in all four bytes where the restatement does not
    for l in range(1, mips):
        skipped = (got[l] == FILL).all(axis=-1) & ~(levels[l] == FILL).all(axis=-1)
        assert not skipped.any(), f"level {l}: {int(skipped.sum())} texels not written"
    assert int(dev.scratch.view(dev.torch.int32)[0]) == 0, "the counter was not left at zero"
    # a second build into the same scratch, not cleared in between, gives the same bytes
    d2, t2 = dev.chain(img, srgb, mips)
    assert dev.plain(d2) == 0
    dev.torch.cuda.synchronize()
    assert dev.torch.equal(t, t2)


ALPHA_CASES = ["holes", "odd", "opaque", "transparent", "scale_high", "scale_low"]


@pytest.mark.parametrize("srgb", [0, 1], ids=["linear", "srgb"])
@pytest.mark.parametrize("name", ALPHA_CASES)
def test_alpha_chain_equals_the_restatement(dev, name, srgb):
    img = T.alpha_inputs()[name]
    h, w = img.shape[:2]
    mips = T.full_mip_count(w, h)
    levels, decided, stats, scales = T.alpha_chain(img, srgb, mips)
    T.assert_mostly_decided(decided)
    d, t = dev.chain(img, srgb, mips)
    d_stats = dev.torch.full((mips * T.STATS_WORDS,), 0x5A5A5A5A, dtype=dev.torch.int32, device=dev.device)
    d_scales = dev.torch.full((mips,), -7.0, dtype=dev.torch.float32, device=dev.device)
    assert dev.lib.brmi_texmips_build_alpha(C.byref(d), dev.table.data_ptr(), d_stats.data_ptr(), d_scales.data_ptr(), dev.stream()) == 0, dev.lib.brmi_last_error(None)
    dev.torch.cuda.synchronize()
    got, guard = dev.levels_of(t, w, h, mips)
    assert np.array_equal(got[0], img) and (guard == FILL).all()
    g_stats, g_scales = d_stats.cpu().numpy().view(np.uint32), d_scales.cpu().numpy()
    assert (g_stats[:T.STATS_WORDS] == 0x5A5A5A5A).all() and g_scales[0] == -7.0, "the words of level 0 were written"
    assert np.array_equal(g_stats[T.STATS_WORDS:], stats[T.STATS_WORDS:]), "statistics words differ"
    assert np.array_equal(g_scales[1:].view(np.uint32), scales[1:].view(np.uint32)), f"scales differ: {g_scales[1:]} vs {scales[1:]}"
    T.assert_chain_matches(got, levels, decided, name)
    for l in range(1, mips):
        assert np.array_equal(got[l][..., 3], levels[l][..., 3]), f"level {l}: alpha differs"


def test_refusals_launch_nothing(dev):
    capi, lib = dev.capi, dev.lib
    img = T.noise_image(16, 8, 5)
    cases = []

    def case(name, status, word, mutate, alpha=False, table=True, scratch="ok"):
        cases.append((name, status, word, mutate, alpha, table, scratch))

    case("null texels", -1, b"texels", lambda d: setattr(d, "texels", None))
    case("misaligned texels", -1, b"texels", lambda d: setattr(d, "texels", d.texels + 2))
    case("null table", -1, b"table", lambda d: None, table=False)
    case("null scratch", -1, b"scratch", lambda d: None, scratch=None)
    case("misaligned scratch", -1, b"scratch", lambda d: None, scratch="odd")
    case("short scratch", -3, b"scratch", lambda d: None, scratch="short")
    case("mipCount 0", -1, b"mipCount", lambda d: setattr(d, "mipCount", 0))
    case("mipCount 17", -1, b"mipCount", lambda d: setattr(d, "mipCount", capi.TEXTURE_MAX_MIPS + 1))
    case("mipCount longer than the size allows", -1, b"mipCount", lambda d: setattr(d, "mipCount", 6))
    case("float format", -1, b"format", lambda d: setattr(d, "format", capi.TEXTURE_FORMAT_RGBA16_FLOAT))
    case("unknown format", -1, b"format", lambda d: setattr(d, "format", 9))
    case("empty image", -1, b"empty", lambda d: setattr(d, "width", 0))
    case("overlapping offsets", -1, b"overlap", lambda d: d.mipOffset.__setitem__(2, d.mipOffset[1] + 3))
    case("level 1 inside level 0", -1, b"overlap", lambda d: d.mipOffset.__setitem__(1, 100))
    case("alpha: null stats", -1, b"stats", lambda d: None, alpha=True, scratch=None)
    case("alpha: overlapping offsets", -1, b"overlap", lambda d: d.mipOffset.__setitem__(3, d.mipOffset[2]), alpha=True)
    case("alpha: mipCount 0", -1, b"mipCount", lambda d: setattr(d, "mipCount", 0), alpha=True)
    big = dev.torch.zeros(64, dtype=dev.torch.uint8, device=dev.device)
    for name, status, word, mutate, alpha, table, scratch in cases:
        d, t = dev.chain(img, 0, 5)
        before = t.clone()
        mutate(d)
        tb = dev.table.data_ptr() if table else None
        if alpha:
            stats = dev.torch.zeros(5 * T.STATS_WORDS, dtype=dev.torch.int32, device=dev.device)
            scales = dev.torch.zeros(5, dtype=dev.torch.float32, device=dev.device)
            rc = lib.brmi_texmips_build_alpha(C.byref(d), tb, stats.data_ptr() if scratch else None, scales.data_ptr(), dev.stream())
        else:
            ptr, n = {None: (None, 4), "ok": (big.data_ptr(), 4), "odd": (big.data_ptr() + 1, 4), "short": (big.data_ptr(), 3)}[scratch]
            rc = lib.brmi_texmips_build(C.byref(d), tb, ptr, n, dev.stream())
        dev.torch.cuda.synchronize()
        assert rc == status, f"{name}: returned {rc}"
        assert word in lib.brmi_last_error(None), f"{name}: {lib.brmi_last_error(None)}"
        assert dev.torch.equal(t, before), f"{name}: the chain was written"
    assert lib.brmi_texmips_build(None, dev.table.data_ptr(), big.data_ptr(), 4, dev.stream()) == -1 and b"descriptor" in lib.brmi_last_error(None)
    d, _ = dev.chain(T.noise_image(4100, 1, 1), 0, 2)
    assert lib.brmi_texmips_build(C.byref(d), dev.table.data_ptr(), big.data_ptr(), 4, dev.stream()) == -3 and b"4096" in lib.brmi_last_error(None)
    s, st, sc = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert lib.brmi_texmips_bytes(5, C.byref(s), C.byref(st), C.byref(sc)) == 4 + 5 * 1040 + 20 and (s.value, st.value, sc.value) == (4, 5200, 20)
    assert lib.brmi_texmips_bytes(0, None, None, None) == 0 and lib.brmi_texmips_bytes(17, None, None, None) == 0


def test_a_scene_whose_chains_were_rebuilt_on_the_device_renders_as_the_chains_of_the_restatement(dev, scenes):
    """The pattern of test_a_device_built_environment_renders_as_the_tables_of_the_restatement: the textured tiny scene, every texture's levels 1.. wiped and
    rebuilt by brmi_texmips_build in the pass's own texel buffer, against the same scene with the restatement's chains uploaded (where the restatement leaves a
    code undecided, the device's code, checked to be within one)."""
    from basicrenderer_amd.renderer import VisibilityRenderer
    scene = scenes("tiny_textured")
    descs = scene.arrays["textureDescs"].view(np.uint8).reshape(-1, 96)
    frames = []
    r = VisibilityRenderer(scene)
    try:
        texels = r.texels()
        assert texels.numel() == scene.arrays["texels"].size
        table = r.torch.from_numpy(scene.arrays["srgbToLinear"].view(np.float32).copy()).to(r.device)
        host = np.ascontiguousarray(scene.arrays["texels"]).view(np.uint8).reshape(-1).copy()
        wiped, expected, built = host.copy(), host.copy(), 0
        jobs = []
        for i in range(len(descs)):
            base = int(descs[i, :8].view(np.uint64)[0])
            w, h, mips, fmt = (int(x) for x in descs[i, 8:24].view(np.uint32))
            offs = [int(x) for x in descs[i, 24:24 + 4 * mips].view(np.uint32)]
            if fmt > 1 or mips < 2:
                continue
            level0 = host[base:base + w * h * 4].reshape(h, w, 4)
            levels, decided = T.plain_chain(level0, fmt, mips, scene.arrays["srgbToLinear"].view(np.float32))
            for l in range(1, mips):
                lw, lh = T.level_sizes(w, h, mips)[l]
                wiped[base + offs[l] * 4: base + (offs[l] + lw * lh) * 4] = FILL
            jobs.append((base, w, h, mips, fmt, offs, levels, decided))
        texels.copy_(r.torch.from_numpy(wiped).to(r.device))
        for base, w, h, mips, fmt, offs, levels, decided in jobs:
            d = dev.capi.TextureDesc()
            d.texels, d.width, d.height, d.mipCount, d.format = texels.data_ptr() + base, w, h, mips, fmt
            for l, o in enumerate(offs):
                d.mipOffset[l] = o
            assert dev.lib.brmi_texmips_build(C.byref(d), table.data_ptr(), dev.scratch.data_ptr(), 4, r._s()) == 0, dev.lib.brmi_last_error(None)
            built += 1
        r.torch.cuda.synchronize()
        device = texels.cpu().numpy()
        for base, w, h, mips, fmt, offs, levels, decided in jobs:
            got = [device[base + o * 4: base + (o + lw * lh) * 4].reshape(lh, lw, 4) for o, (lw, lh) in zip(offs, T.level_sizes(w, h, mips))]
            T.assert_chain_matches(got, levels, decided, "scene texture")
            for l in range(1, mips):
                lw, lh = T.level_sizes(w, h, mips)[l]
                expected[base + offs[l] * 4: base + (offs[l] + lw * lh) * 4] = np.where(decided[l], levels[l], got[l]).reshape(-1)
        assert built > 0
        r.execute()
        frames.append({k: v.copy() for k, v in r.gbuffer().items()})
        texels.copy_(r.torch.from_numpy(expected).to(r.device))
        r.execute()
        frames.append({k: v.copy() for k, v in r.gbuffer().items()})
    finally:
        r.close()
    for k in frames[0]:
        assert np.array_equal(frames[0][k].view(np.uint8), frames[1][k].view(np.uint8)), f"G-buffer plane {k} differs"
    assert not np.array_equal(wiped, expected)


def test_a_glb_renders_its_own_materials_as_the_cpu_oracle_does(tmp_path):
    """The default path of a glTF file with materials: tables from gltf.load_gltf_materials, the scene entry for the caller's materials, chains built on the
    device by VisibilityRenderer, one frame -- against the CPU oracle on the same scene arrays (which then hold the device-built chains), under the tolerances
    of test_parity_gpu.py: keys, depth and G-buffer bit for bit, HDR within one fp16 ULP.  The masked quad's hole shows no geometry: empty visibility keys."""
    import gltf_fixture as G
    import orc
    from basicrenderer_amd import Scene, gltf
    from basicrenderer_amd.renderer import VisibilityRenderer
    glb = G.write_glb(str(tmp_path / "two_quads.glb"))
    meshes, instances = gltf.load_gltf(glb)
    mats = gltf.load_gltf_materials(glb)
    view = dict(eye=(0.0, 0.0, 3.2), yaw=0.0, pitch=0.0, fov=60.0, near=0.1, far=50.0)
    sc = Scene(width=256, height=144, point_lights=2, meshes=meshes, instances=instances, view=view, materials=mats)
    r = VisibilityRenderer(sc)
    try:
        assert sc.pending_chains == []
        # the chains the device built are the restatement's (alpha chain for the mask, plain chains for the rest)
        descs = sc.arrays["textureDescs"].view(np.uint8).reshape(-1, 96)
        tx = np.ascontiguousarray(sc.arrays["texels"]).view(np.uint8).reshape(-1)
        for i, t in enumerate(mats["textures"]):
            h, w = t["texels"].shape[:2]
            mips = T.full_mip_count(w, h)
            base = int(descs[i, :8].view(np.uint64)[0])
            offs = [int(x) for x in descs[i, 24:24 + 4 * mips].view(np.uint32)]
            got = [tx[base + o * 4: base + (o + lw * lh) * 4].reshape(lh, lw, 4) for o, (lw, lh) in zip(offs, T.level_sizes(w, h, mips))]
            levels, decided = (T.alpha_chain(t["texels"], int(t["srgb"]), mips)[:2] if t["alpha_coverage"] else T.plain_chain(t["texels"], int(t["srgb"]), mips))
            T.assert_chain_matches(got, levels, decided, t["name"])
        r.execute()
        o = orc.OracleFrame(sc)
        o.run(); o.gbuffer(); o.light_cluster(); o.shade()
        empty = np.uint64(0xFFFFFFFFFFFFFFFF)
        assert np.array_equal(r.visibility(), o.vis), "visibility keys differ"
        assert np.array_equal(r.depth().view(np.uint32), o.depth.view(np.uint32))
        covered = o.vis != empty
        gb = r.gbuffer()
        for key, ref in (("normals", o.normals), ("albedo", o.albedo), ("coat", o.coat), ("emissive", o.emissive), ("fuzz", o.fuzz), ("mr", o.mr), ("motion", o.motion)):
            x, y = gb[key][covered], ref[covered]
            if x.dtype == np.float32:
                x, y = x.view(np.uint32), y.view(np.uint32)
            assert np.array_equal(x, y), f"G-buffer plane {key}: {int((x != y).sum())} of {x.size} values differ"
        # the opaque quad's planes are not constant: its metallic-roughness and emissive textures reached them
        right = covered & (np.arange(covered.shape[1])[None, :] >= 128)
        assert len(np.unique(gb["mr"][right])) > 4 and len(np.unique(gb["emissive"][right].reshape(-1))) > 4
        assert np.abs(r.hdr().view(np.uint16).astype(np.int32) - o.hdr.view(np.uint16).astype(np.int32)).max() <= 1
        # the left quad spans x in [-2.1, -0.1], its hole the middle half of it: the pixel at its centre is empty, one at its rim is not
        vis = r.visibility()
        ys, xs = np.nonzero(covered[:, : 128])
        cy, cx = int(round(ys.mean())), int(round((xs.min() + xs.max()) / 2))
        assert vis[cy, cx] == empty and vis[cy, xs.min() + 2] != empty and covered.sum() > 2000
    finally:
        r.close()
