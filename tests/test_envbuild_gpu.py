"""The environment build (brmi_env_convert / brmi_env_project_sh / brmi_env_prefilter), the RGBA16F lookup and the skybox stage on the GPU, against
tests/envbuild_ref.py (DESIGN.md 2 "cube lookup", 4.11).

1  the lookup of the new format, bit for bit;
2  the SH projection: 27 integers and the scale equal to the fp32 restatement;
3  the prefilter: RGBA8 codes against the float64 restatement, with the margin of an fp32 restatement measured on the CPU;
4  the conversion of a panorama, per half against float64;
5  frames: off is off, pixels with geometry untouched, empty pixels equal to the fp32 restatement, bands, frames in flight, a device-built environment.
"""
import ctypes as C

import numpy as np
import pytest

import envbuild_ref as ref
from test_ibl_gpu import _lookup_samples

pytestmark = pytest.mark.gpu
FILL = 0x5A
CANARY = np.uint64(int.from_bytes(bytes([FILL] * 8), "little"))


# ------------------------------------------------------------------------------------------------ device helpers
class Dev:
    def __init__(self):
        import torch
        from basicrenderer_amd import capi, environment
        self.torch, self.capi, self.env, self.lib = torch, capi, environment, capi.brmi_lib()
        self.device = torch.device("cuda:0")

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.device)

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def cube(self, cube):
        """(descriptor tensor of six faces, tensors to keep) of a (6, n, n, 4) float16 array or of six chains (lists of levels, uint8 or float16)"""
        chains = [[cube[f]] for f in range(6)] if isinstance(cube, np.ndarray) else cube
        fmt = self.capi.TEXTURE_FORMAT_RGBA8_UNORM if chains[0][0].dtype == np.uint8 else self.capi.TEXTURE_FORMAT_RGBA16_FLOAT
        keep, descs = [], []
        for chain in chains:
            t = self.up(np.concatenate([np.ascontiguousarray(l).view(np.uint8).reshape(-1) for l in chain]))
            offs, at = [], 0
            for l in chain:
                offs.append(at); at += l.shape[0] * l.shape[1]
            keep.append(t)
            descs.append(self.env.descriptor_words(t.data_ptr(), chain[0].shape[1], chain[0].shape[0], len(chain), fmt, offs))
        d = self.up(np.stack(descs))
        return d, keep

    def empty_chain(self, size, levels, fill=0x33):
        """a destination RGBA8 chain of six faces: (descriptor tensor, texel tensor, texels per face)"""
        per = self.env.chain_texels(size, levels)
        t = self.torch.full((6 * per * 4,), fill, dtype=self.torch.uint8, device=self.device)
        d = self.up(np.stack([self.env.descriptor_words(t.data_ptr() + f * per * 4, size, size, levels, self.capi.TEXTURE_FORMAT_RGBA8_UNORM) for f in range(6)]))
        return d, t, per


@pytest.fixture(scope="module")
def dev():
    return Dev()


def _sky16(n):
    from basicrenderer_amd import environment
    L = environment.sky_polynomial()(environment.face_directions(n))
    return np.concatenate([L, np.ones((6, n, n, 1))], -1).astype(np.float16)


def _checker16(n, spot=1000.0):
    """a checker of values in [0, 1] with negative entries on one face and one HDR texel"""
    rng = np.random.default_rng(700 + n)
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    c = np.zeros((6, n, n, 4), dtype=np.float32)
    for f in range(6):
        on = ((x // max(1, n // 4) + y // max(1, n // 4) + f) & 1).astype(np.float32)
        c[f, ..., :3] = on[..., None] * rng.uniform(0.2, 1.0, size=3) + rng.uniform(0.0, 0.1, size=(n, n, 3))
    c[1, ..., :3] -= 0.6      # negatives
    c[2, n // 2, n // 3, :3] = (spot, 0.5 * spot, 0.25)
    c[..., 3] = 1.0
    return c.astype(np.float16)


def _octant_checker16(n, spot=40.0):
    """a checker of the direction's octant (eight colours, the cell borders on the faces' centre lines) with one HDR texel inside a face.  Why this checker: the
    cube lookup does not filter across face edges, so a cube whose faces disagree along their common edge is DISCONTINUOUS there, and the prefilter's sample
    directions land on such edges exactly (N at a texel centre, H at multiples of pi / 8: |x| = |y| ties by symmetry), where the last bit of the arithmetic
    picks the face.  Cells that span the face edges make the cube continuous across them, so float32 and float64 agree to rounding."""
    from basicrenderer_amd import environment
    D = environment.face_directions(n)
    palette = np.random.default_rng(77).uniform(0.05, 1.0, size=(8, 3))
    cell = (D[..., 0] > 0).astype(int) + 2 * (D[..., 1] > 0) + 4 * (D[..., 2] > 0)
    c = np.concatenate([palette[cell], np.ones((6, n, n, 1))], -1).astype(np.float32)
    c[2, n // 4, n // 4 + 1, :3] = (spot, 0.5 * spot, 0.25)
    return c.astype(np.float16)


# ------------------------------------------------------------------------------------------------ 1  the fp16 lookup
def test_fp16_lookup_bit_for_bit(dev):
    """brmi_debug_env_lookup on the 4,096 samples of test_ibl_gpu._lookup_samples per cube, faces 1, 4 and 16: a one-level RGBA16F cube (what the build and the
    skybox read: every lod reads level 0) and, for 4 and 16, a chain of RGBA16F levels (the lods pick and blend levels as for RGBA8).  Four channels as bit
    patterns, no sample left out.  An RGBA8 cube through the same entry point takes the existing path: equal to ibl_ref.sample_cube."""
    import ibl_ref
    rng = np.random.default_rng(31)
    for n in (1, 4, 16):
        one = (_checker16(n, spot=60000.0).astype(np.float32) * rng.uniform(0.5, 1.0, size=(6, n, n, 4))).astype(np.float16)
        levels = int(np.log2(n)) + 1
        chain = [[(rng.normal(size=(max(1, n >> l), max(1, n >> l), 4)) * 4.0 ** rng.integers(-6, 6)).astype(np.float16) for l in range(levels)] for _ in range(6)]
        rgba8 = [[rng.integers(0, 256, size=(max(1, n >> l), max(1, n >> l), 4), dtype=np.uint8) for l in range(levels)] for _ in range(6)]
        for cube, sampler in ((one, ref.sample_cube_any), (chain, ref.sample_cube_any), (rgba8, ibl_ref.sample_cube)):
            nl = 1 if isinstance(cube, np.ndarray) else levels
            dirs, lods = _lookup_samples(n, nl)
            d, keep = dev.cube(cube)
            out = dev.torch.zeros((len(dirs), 4), dtype=dev.torch.float32, device=dev.device)
            t_dirs, t_lods = dev.up(dirs), dev.up(lods)
            assert dev.lib.brmi_debug_env_lookup(d.data_ptr(), 1, 0, t_dirs.data_ptr(), t_lods.data_ptr(), out.data_ptr(), len(dirs), dev.stream()) == 0
            got = out.cpu().numpy()
            want = sampler(cube, dirs, lods)
            assert np.isfinite(want).all()
            bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
            assert len(bad) == 0, (n, nl, len(bad), dirs[bad[:3]], lods[bad[:3]], got[bad[:3]], want[bad[:3]])


# ------------------------------------------------------------------------------------------------ 2  SH projection
@pytest.mark.parametrize("n", [1, 4, 16, 24])
@pytest.mark.parametrize("fmt", ["rgba16f", "rgba8"])
def test_sh_projection_equals_the_fp32_restatement(dev, n, fmt):
    """All 27 integers and the scale's bits EQUAL envbuild_ref.project_sh (24 is not a multiple of the 16-wide tile: edge guard, partial waves); negatives in
    fp16 and an HDR texel of 1000; run twice into a record full of garbage: the same result (the stage zeroes the record itself); the second environment of
    the table, and the other words of the first, are untouched; the cube is the one cubeMapDescriptorIndex of the record names (the second of the table)."""
    rng = np.random.default_rng(n)
    cube = _checker16(n) if fmt == "rgba16f" else [[rng.integers(0, 256, size=(n, n, 4), dtype=np.uint8)] for _ in range(6)]
    decoy = _sky16(4)
    d_decoy, k0 = dev.cube(decoy)
    d_cube, k1 = dev.cube(cube)
    table = dev.torch.cat([d_decoy, d_cube])
    info = rng.integers(0, 2 ** 32, size=(2, 32), dtype=np.uint32)
    info[0, 0] = 1
    t_info = dev.up(info)
    want, scale = ref.project_sh(cube, n)
    for _ in range(2):
        assert dev.lib.brmi_env_project_sh(table.data_ptr(), 2, t_info.data_ptr(), 2, 0, n, dev.stream()) == 0
        got = t_info.cpu().numpy().view(np.uint32).reshape(2, 32)
        assert np.array_equal(got[0, 3:30].view(np.int32), want), (got[0, 3:30].view(np.int32), want)
        assert got[0, 2] == np.array([scale], dtype=np.float32).view(np.uint32)[0]
        assert np.array_equal(got[1], info[1]) and np.array_equal(got[0, :2], info[0, :2]) and np.array_equal(got[0, 30:], info[0, 30:])
    assert np.abs(want).max() > 10
    if fmt == "rgba16f" and n > 1:
        assert (want < 0).any() and np.abs(want).max() > 1000


# ------------------------------------------------------------------------------------------------ 3  prefilter
PREFILTER_CASES = {"sky_16x5": ("sky", 16, 5), "checker_16x5": ("checker", 16, 5), "sky_8x12": ("sky", 8, 12), "checker_8x12": ("checker", 8, 12)}


@pytest.fixture(scope="module")
def prefilter_refs():
    """float64 and float32 restatements of every case, computed once"""
    cache = {}

    def get(case):
        if case not in cache:
            kind, n, levels = PREFILTER_CASES[case]
            cube = _sky16(n) if kind == "sky" else _octant_checker16(n)
            cache[case] = (cube, ref.prefilter(cube, n, levels, np.float64), ref.prefilter(cube, n, levels, np.float32))
        return cache[case]
    return get


@pytest.mark.parametrize("case", list(PREFILTER_CASES))
def test_prefilter_codes_against_float64(dev, prefilter_refs, case):
    """Base 16 with 5 levels and base 8 with 12 requested levels (the levels below 1 x 1 stay 1 x 1), the procedural sky and a checker with an HDR spot, RGBA16F.
    Every code within 1 of the float64 restatement; equal wherever the float64 value lies further from a rounding boundary than the margin = 4 x the largest
    deviation, in code units, of the fp32 numpy restatement from float64 on these same inputs; at most 2 % of the codes differ by 1, and the fp32 restatement
    alone stays within that share.  Measured on the CPU: the checker deviates 4.8e-3 (base 16) and 1.8e-3 (base 8) code units, its HDR spot setting the
    scale -- margins 1.9e-2 and 7.3e-3; the sky deviates 0.48 and 0.89 code units at its roughest levels, margins 1.9 and 3.6, which leaves the equality
    clause nothing to hold for it: the sky's faces disagree along their edges (texel centres of two faces are different directions), the lookup does not
    filter across edges, and sample directions land on them exactly (_octant_checker16 says more); 8 / 6138 and 10 / 1674 of its fp32 codes differ.
    No texel is excluded: for these sizes no texel centre has |N.z| within 2e-3 of the 0.999 frame switch (asserted from the float64 directions).  Alpha is 255."""
    kind, n, levels = PREFILTER_CASES[case]
    cube, v64, v32 = prefilter_refs(case)
    for m in range(levels):
        nz = np.abs(ref.prefilter_directions(n, m, np.float64)[..., 2])
        assert ((np.abs(nz - 0.999) > 2e-3) | (nz == 1.0)).all(), (m, nz[np.abs(nz - 0.999) <= 2e-3])      # (the 1 x 1 level sits at exactly 1)
    d_src, k0 = dev.cube(cube)
    d_dst, t_dst, per = dev.empty_chain(n, levels)
    assert dev.lib.brmi_env_prefilter(d_src.data_ptr(), d_dst.data_ptr(), n, levels, dev.capi.TEXTURE_FORMAT_RGBA8_UNORM, dev.stream()) == 0
    got_all = t_dst.cpu().numpy().reshape(6, per, 4)
    to_units = lambda v: np.clip(v.astype(np.float64), 0.0, 1.0) * 255.0
    deviation = max(np.abs(to_units(a) - to_units(b)).max() for a, b in zip(v32, v64))
    margin = 4.0 * deviation
    print(f"prefilter {case}: fp32 restatement deviates {deviation:.3e} code units from float64, margin {margin:.3e}")
    total = differ = differ32 = 0
    at = 0
    for m in range(levels):
        s = max(1, n >> m)
        got = got_all[:, at:at + s * s].reshape(6, s, s, 4).astype(np.int64); at += s * s
        assert (got[..., 3] == 255).all()
        x = to_units(v64[m])
        want = np.floor(x + 0.5).astype(np.int64)
        dist = np.abs(x - (np.floor(x) + 0.5))
        diff = np.abs(got[..., :3] - want)
        assert diff.max() <= 1, (m, diff.max())
        safe = dist > margin
        assert (diff[safe] == 0).all(), (m, np.argwhere(safe & (diff != 0))[:4])
        total += diff.size; differ += int((diff != 0).sum()); differ32 += int((ref.unorm_codes(v32[m]) != want).sum())
    print(f"prefilter {case}: {differ} of {total} codes differ by 1 from float64 ({differ32} for the fp32 restatement)")
    assert differ <= 0.02 * total and differ32 <= 0.02 * total
    assert at == per


def test_prefilter_level_0_of_an_rgba8_source_is_the_source(dev):
    """roughness 0: the lookup at N, quantised -- bit for bit the source's codes, alpha 255; a destination descriptor of another format, or without texels, is
    skipped (its canary stays), and texels outside a face's own size are not written."""
    rng = np.random.default_rng(12)
    n = 16
    src = [[rng.integers(0, 256, size=(n, n, 4), dtype=np.uint8)] for _ in range(6)]
    d_src, k0 = dev.cube(src)
    d_dst, t_dst, per = dev.empty_chain(n, 3)
    words = d_dst.cpu().numpy().view(np.uint32).reshape(6, 24).copy()
    words[4, 5] = dev.capi.TEXTURE_FORMAT_RGBA16_FLOAT      # face 4: not the format the stage writes
    words[5, 0:2] = 0                                        # face 5: no texels
    d_dst = dev.up(words)
    assert dev.lib.brmi_env_prefilter(d_src.data_ptr(), d_dst.data_ptr(), n, 3, dev.capi.TEXTURE_FORMAT_RGBA8_UNORM, dev.stream()) == 0
    got = t_dst.cpu().numpy().reshape(6, per, 4)
    for f in range(4):
        assert np.array_equal(got[f, :n * n, :3].reshape(n, n, 3), src[f][0][..., :3]) and (got[f, :, 3] == 255).all()
    assert (got[4:] == 0x33).all()


# ------------------------------------------------------------------------------------------------ 4  convert
def _sky_panorama(W, H):
    from basicrenderer_amd import environment
    u, v = np.meshgrid((np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H, indexing="xy")
    theta, y = (u - 0.5) * 2 * np.pi, np.sin((0.5 - v) * np.pi)
    c = np.sqrt(np.maximum(0.0, 1 - y * y))
    return environment.sky_polynomial()(np.stack([np.cos(theta) * c, y, np.sin(theta) * c], -1))


def test_convert_against_float64(dev):
    """A 64 x 32 panorama of the procedural sky (RGBA16F) to faces of 16: each half within 1 fp16 ULP of the float64 restatement plus W * 2^-20 * (the largest
    difference between neighbouring source texels of that channel) -- the uv budget: the documented 2 ULP of atan2f / asinf and the roundings behind them move
    u * W by less than 2^-20 * W texels, and a bilinear sample moves by at most one neighbour difference per texel.  Alpha is exactly 1.0; the canary of a
    texel the face's own descriptor does not hold stays."""
    W, H, n = 64, 32, 16
    pano = np.concatenate([_sky_panorama(W, H), np.ones((H, W, 1))], -1).astype(np.float16)
    t_src = dev.up(pano)
    d_src = dev.up(dev.env.descriptor_words(t_src.data_ptr(), W, H, 1, dev.capi.TEXTURE_FORMAT_RGBA16_FLOAT))
    t_cube = dev.torch.full((6 * n * n * 8 + 64,), FILL, dtype=dev.torch.uint8, device=dev.device)
    d_cube = dev.up(np.stack([dev.env.descriptor_words(t_cube.data_ptr() + f * n * n * 8, n, n, 1, dev.capi.TEXTURE_FORMAT_RGBA16_FLOAT) for f in range(6)]))
    assert dev.lib.brmi_env_convert(d_src.data_ptr(), d_cube.data_ptr(), n, dev.capi.TEXTURE_FORMAT_RGBA16_FLOAT, dev.stream()) == 0
    raw = t_cube.cpu().numpy()
    assert (raw[6 * n * n * 8:] == FILL).all()
    got = raw[:6 * n * n * 8].view(np.float16).reshape(6, n, n, 4).astype(np.float64)
    want, _ = ref.convert(pano, n, np.float64)
    assert (got[..., 3] == 1.0).all()
    p = pano.astype(np.float64)[..., :3]
    neighbour = np.maximum(np.abs(np.diff(p, axis=0)).max(axis=(0, 1)), np.abs(p - np.roll(p, 1, axis=1)).max(axis=(0, 1)))
    tol = ref.half_ulp_of(want) + W * 2.0 ** -20 * neighbour
    err = np.abs(got[..., :3] - want)
    print(f"convert: worst error {np.max(err / tol):.3f} of the bound")
    assert (err <= tol).all(), np.argwhere(err > tol)[:4]
    assert np.ptp(got[..., :3]) > 0.3


# ------------------------------------------------------------------------------------------------ 5  frames
@pytest.fixture(scope="module")
def sky_env():
    """the procedural environment the IBL frame tests use, with a sky cube of its own: RGBA16F, HDR in places"""
    from basicrenderer_amd import environment
    e = environment.Environment.procedural(16)
    cube = _sky16(16).astype(np.float32)
    cube[2, 3:6, 4:9, :3] *= 40.0
    cube[[0, 1, 4, 5], 5:8, 2:11, :3] *= 40.0      # (side faces, the rows above the horizon: what this scene's cameras see)
    return environment.Environment(e.faces, e.sh, e.scale, e.radiance, cube16=cube.astype(np.float16))


def _capture(r):
    return dict(hdr=r.hdr(), depth=r.depth(), **r.gbuffer())


def _frame(scene, env, skybox, camera=None, split=False, in_flight=0, **kw):
    from basicrenderer_amd import capi
    from basicrenderer_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(scene, **kw)
    try:
        if camera is not None:
            cam, cull = camera
            r.set_camera_device(r.torch.from_numpy(cam).to(r.device), r.torch.from_numpy(cull).to(r.device), cam)
        if env is not None:
            r.set_environment(env, skybox=skybox)
        r.res[capi.RES["HDR_COLOR"]].fill_(FILL)
        if split:
            other = r.torch.cuda.Stream(device=r.device)
            for _ in range(max(1, in_flight)):
                r.execute(shading_stream=other)
            other.synchronize()
        else:
            r.execute()
        return _capture(r)
    finally:
        r.close()


def _on_face_edge(words, W, H, eps=1e-6):
    """pixels whose float64 view ray has its two largest |components| within eps of each other (relative)"""
    M = ref.camera_matrices(words, np.float64)
    nx, ny = np.meshgrid(((np.arange(W) + 0.5) / W) * 2 - 1, (1 - (np.arange(H) + 0.5) / H) * 2 - 1, indexing="xy")
    h = ref.mul_vm(np.stack([nx, ny, np.ones_like(nx), np.ones_like(nx)], -1), M["projectionInverse"])
    v = ref.normalize(h[..., :3] / np.maximum(np.abs(h[..., 3]), 1e-6)[..., None])
    w = np.sort(np.abs(ref.normalize(ref.mul_vm(np.concatenate([v, np.zeros_like(nx)[..., None]], -1), M["viewInverse"])[..., :3])), axis=-1)
    return (w[..., 2] - w[..., 1]) <= eps * w[..., 2]


def _camera_words(scene, camera):
    pf = scene.arrays["perFrame"].view(np.uint32)
    cams = (camera[0] if camera is not None else scene.arrays["cameras"]).view(np.float32).reshape(-1, 184)
    return cams[pf[8]]


@pytest.fixture(scope="module")
def frame_cases(scenes):
    """the 256 x 144 scene of the IBL frame tests from a camera one step along its path, at rest and with a previous frame half a step back (motion); both look
    more than half at empty sky, and neither has a view ray along a cube face edge (test_frames_show_the_sky_behind_the_geometry)"""
    scene = scenes("tiny_coat_fuzz")
    return scene, {"still": scene.camera_at(1.0, 1.0), "moved": scene.camera_at(1.0, 0.5)}


@pytest.mark.parametrize("which", ["still", "moved"])
def test_frames_show_the_sky_behind_the_geometry(frame_cases, sky_env, which):
    """skybox off: HDR and every plane equal, byte for byte, those of a pass that bound the environment the old way (the canary of the empty pixels included).
    On: every pixel with geometry unchanged byte for byte in every plane; every empty pixel's HDR halves and motion-vector halves equal the fp32 restatement
    bit for bit and lie within 1 fp16 ULP of float64; alpha 1."""
    scene, cams = frame_cases
    camera = cams[which]
    old = _frame(scene, sky_env, False, camera)
    on = _frame(scene, sky_env, True, camera)
    from basicrenderer_amd import environment
    plain = environment.Environment(sky_env.faces, sky_env.sh, sky_env.scale)      # no sky cube: the tables of before
    oldest = _frame(scene, plain, False, camera)
    for k in old:
        assert (old[k].view(np.uint8) == oldest[k].view(np.uint8)).all(), k
    H, W = old["depth"].shape
    empty = old["depth"].view(np.uint32) == ref.EMPTY_DEPTH
    print(f"skybox frame '{which}': {empty.mean():.2%} of the pixels are sky")
    assert 0.05 < empty.mean() < 0.95
    assert (old["hdr"][empty] == CANARY).all()
    for k in old:
        assert (old[k][~empty].view(np.uint8) == on[k][~empty].view(np.uint8)).all(), k
        if k not in ("hdr", "motion"):
            assert (old[k].view(np.uint8) == on[k].view(np.uint8)).all(), k
    words = _camera_words(scene, camera)
    rgb32, mv32 = ref.skybox(words, W, H, sky_env.cube16, np.float32)
    rgb64, mv64 = ref.skybox(words, W, H, sky_env.cube16, np.float64)
    got = on["hdr"][empty].view(np.uint16).reshape(-1, 4)
    want = np.concatenate([rgb32[empty], np.ones((int(empty.sum()), 1), dtype=np.float32)], 1).astype(np.float16).view(np.uint16)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    got_mv = on["motion"][empty].view(np.uint16).reshape(-1, 2)
    assert np.array_equal(got_mv, mv32[empty].astype(np.float16).view(np.uint16)), np.argwhere(got_mv != mv32[empty].astype(np.float16).view(np.uint16))[:4]
    g = got.view(np.float16).astype(np.float64)[:, :3]
    # float64, every empty pixel.  (The cameras are chosen so that no view ray runs along a face edge of the cube, where the lookup -- which does not filter
    # across edges, DESIGN.md 2 -- is discontinuous and the last bit of the direction picks the face: asserted here as a property of the inputs.  The scene's
    # own camera is yawed so that one pixel column lies 6e-8 from the |x| = |z| edge.)
    assert not _on_face_edge(words, W, H).any()
    assert (np.abs(g - rgb64[empty]) <= ref.half_ulp_of(rgb64[empty])).all()
    # the motion vector: 1 fp16 ULP of the float64 value + 2^-20, the bound DESIGN.md 4.11 derives for a difference of two fp32 NDC positions
    gm = got_mv.view(np.float16).astype(np.float64)
    assert (np.abs(gm - mv64[empty]) <= ref.half_ulp_of(mv64[empty]) + 2.0 ** -20).all()
    assert g.max() > 2.0 and np.ptp(g) > 0.3
    assert (np.abs(gm).max() > 1e-3) == (which == "moved")


def test_skybox_of_an_environment_without_a_sky_cube_shows_its_prefiltered_level_0(frame_cases, sky_env):
    """cubeMapDescriptorIndex then names the RGBA8 cube: the lookup takes the existing path"""
    from basicrenderer_amd import environment
    scene, _ = frame_cases
    plain = environment.Environment(sky_env.faces, sky_env.sh, sky_env.scale)
    on = _frame(scene, plain, True)
    empty = on["depth"].view(np.uint32) == ref.EMPTY_DEPTH
    H, W = empty.shape
    rgb32, _ = ref.skybox(_camera_words(scene, None), W, H, [f[:] for f in plain.faces], np.float32)
    got = on["hdr"][empty].view(np.uint16).reshape(-1, 4)[:, :3]
    assert np.array_equal(got, rgb32[empty].astype(np.float16).view(np.uint16))


def test_frame_modes_reproduce_the_whole_frame(frame_cases, sky_env):
    """a band of rows 16-56 equals those rows of the whole frame (and writes no other row); brmi_execute_split on two streams, three frames in flight, gives
    the serial frame; the interleaved partition renders its rows of the frame."""
    from basicrenderer_amd.renderer import VisibilityRenderer
    scene, _ = frame_cases
    whole = _frame(scene, sky_env, True)
    band = _frame(scene, sky_env, True, band=(16, 56))
    for k in ("hdr", "motion"):
        assert (band[k][16:56] == whole[k][16:56]).all(), k
    assert (band["hdr"][:16] == CANARY).all() and (band["hdr"][56:] == CANARY).all()
    split = _frame(scene, sky_env, True, split=True, in_flight=3)
    for k in whole:
        assert (split[k].view(np.uint8) == whole[k].view(np.uint8)).all(), k
    from conftest import Scene
    tall = Scene("tiny", 256, 160, point_lights=2)      # (chunks of 16 rows for two GPUs need a height that is a multiple of 32)
    whole = _frame(tall, sky_env, True)
    r = VisibilityRenderer(tall, stripes=(16, 2, 1))
    try:
        r.set_environment(sky_env, skybox=True)
        r.execute()
        rows = r.frame_rows()
        empty = whole["depth"][rows].view(np.uint32) == ref.EMPTY_DEPTH
        assert empty.any() and (r.hdr() == whole["hdr"][rows]).all() and (r.gbuffer()["motion"][empty] == whole["motion"][rows][empty]).all()
    finally:
        r.close()


def test_a_device_built_environment_renders_as_the_tables_of_the_restatement(dev, frame_cases):
    """Environment.from_equirect (convert + project + prefilter on the device) against an Environment made of envbuild_ref's results for the device's own cube:
    the same SH integers and scale, prefiltered codes within 1, and frames whose bytes agree wherever the prefilter codes agree -- here: every empty pixel
    (the sky cube is the same), and every pixel when no code differs."""
    from basicrenderer_amd import environment
    scene, _ = frame_cases
    pano = _sky_panorama(64, 32)
    pano[4:8, 10:14] *= 30.0
    built = environment.Environment.from_equirect(pano, size=16, levels=5)
    assert built.cube16.shape == (6, 16, 16, 4) and built.levels == 5 and built.cube16.astype(np.float32).max() > 5.0
    ints, scale = ref.project_sh(built.cube16, 16)
    assert np.array_equal(built.sh.reshape(-1), ints) and np.float32(built.scale) == scale
    want = ref.prefiltered_faces(ref.prefilter(built.cube16, 16, 5, np.float64))
    diffs = sum(int((np.abs(a.astype(np.int64) - b.astype(np.int64)) != 0).sum()) for fa, fb in zip(built.faces, want) for a, b in zip(fa, fb))
    assert all(np.abs(a.astype(np.int64) - b.astype(np.int64)).max() <= 1 for fa, fb in zip(built.faces, want) for a, b in zip(fa, fb))
    restated = environment.Environment(want, ints, float(scale), cube16=built.cube16)
    a, b = _frame(scene, built, True), _frame(scene, restated, True)
    empty = a["depth"].view(np.uint32) == ref.EMPTY_DEPTH
    for k in a:
        assert (a[k][empty].view(np.uint8) == b[k][empty].view(np.uint8)).all(), k
        if diffs == 0 or k != "hdr":
            assert (a[k].view(np.uint8) == b[k].view(np.uint8)).all(), k
    print(f"device-built environment: {diffs} prefiltered codes differ from the float64 restatement")
    # with the device's own codes in the restated tables the frames agree everywhere
    same = environment.Environment(built.faces, ints, float(scale), cube16=built.cube16)
    c = _frame(scene, same, True)
    for k in a:
        assert (a[k].view(np.uint8) == c[k].view(np.uint8)).all(), k


def test_procedural_ggx_and_from_cube_run_the_build(dev):
    """Environment.procedural(prefilter="ggx"): level 0 is the procedural level 0 (an RGBA8 source comes back bit for bit), the chain below it is not the box
    chain, the integers and the scale are the projection of that level 0; the default stays the box chain.  Environment.from_cube keeps the cube it was given
    (as halves) and projects it."""
    from basicrenderer_amd import environment
    box = environment.Environment.procedural(8)
    ggx = environment.Environment.procedural(8, prefilter="ggx")
    assert ggx.levels == box.levels == 4 and ggx.cube16 is None
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(ggx.faces, box.faces))
    assert any((a[2] != b[2]).any() for a, b in zip(ggx.faces, box.faces))
    ints, scale = ref.project_sh([f[:1] for f in box.faces], 8)
    assert np.array_equal(ggx.sh.reshape(-1), ints) and np.float32(ggx.scale) == scale
    want = ref.prefiltered_faces(ref.prefilter([f[:1] for f in box.faces], 8, 4, np.float64))
    assert all(np.abs(a.astype(np.int64) - b.astype(np.int64)).max() <= 1 for fa, fb in zip(ggx.faces, want) for a, b in zip(fa, fb))
    cube = _checker16(8)
    env = environment.Environment.from_cube(cube.astype(np.float32)[..., :3], levels=2)
    assert np.array_equal(env.cube16.view(np.uint16), cube.view(np.uint16)) and env.levels == 2
    ints, scale = ref.project_sh(cube, 8)
    assert np.array_equal(env.sh.reshape(-1), ints) and np.float32(env.scale) == scale
