"""Shadow maps of spot and point lights on the GPU: the capture kernel against the oracle's depth from the light's camera, the two shadow
functions against the float64 restatement on the made-up inputs tests/test_shadow_cpu.py has judged, off is off, and frames in flight."""
import ctypes as C

import numpy as np
import pytest

import shadow_cases as cases
import shadow_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer():
    from basicrenderer_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(cases.scene())
    yield r
    r.close()


def _bind(r, spot_size=(64, 64)):
    """Shadows for the first spot and the first point light; the maps are then this file's own tensors (a spot map need not be square)."""
    from basicrenderer_amd import capi
    _, spot, point = cases.lights()
    r.set_shadows([spot, point], resolution=64, point_resolution=cases.CUBE_RES)
    sd = r._shadows
    if spot_size != (64, 64):
        v = sd["views"][0]
        v["map"] = r.torch.zeros((spot_size[1], spot_size[0]), dtype=r.torch.float32, device=r.device)
        v["desc"].texels, v["desc"].width, v["desc"].height = v["map"].data_ptr(), spot_size[0], spot_size[1]
        table = np.frombuffer(b"".join(bytes(x["desc"]) for x in sd["views"]), dtype=np.uint8).copy()
        t = r.torch.from_numpy(table).to(r.device)
        sd["keep"].append(t)
        sd["buffers"].maps = t.data_ptr()
        r._check(r.lib.brmi_set_shadows(r._h, C.byref(sd["buffers"])), "brmi_set_shadows")
    return sd


def _load(r, view, array):
    view["map"].copy_(r.torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32)).to(r.device))


# ---- 1. capture ---------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(100, 72), (128, 128)], ids=["100x72", "128x128"])
def test_capture_matches_oracle_depth(size):
    """brmi_shadow_capture of a light-view pass == the fp32 conversion of the oracle's linear depth from the same camera, bit for bit, background included."""
    import orc
    from basicrenderer_amd import capi, shadows as sh
    from basicrenderer_amd.renderer import VisibilityRenderer
    from conftest import Scene
    W, H = size
    s = Scene("tiny", W, H, point_lights=6, spot_every=2)
    rec = s.arrays["lights"].view(sh.LIGHT_DTYPE)
    l = rec[int(np.flatnonzero(rec["type"] == sh.LIGHT_SPOT)[0])]
    # the light's view at the scene's own size: the spot camera's matrices with the aspect of the frame folded into the projection's x scale
    cam, cull = sh.light_views(l, max(W, H))[0]
    c, cc = np.frombuffer(cam, dtype=np.float32).copy(), np.frombuffer(cull, dtype=np.float32).copy()
    view, proj = c[4:20].reshape(4, 4).astype(np.float64), c[36:52].reshape(4, 4).astype(np.float64)
    proj[0, 0] *= H / W
    for off, m in ((36, proj), (52, np.linalg.inv(proj)), (68, view @ proj), (100, proj), (116, proj), (132, proj)):
        c[off: off + 16] = m.reshape(-1)
    c.view(np.uint32)[177:179] = [W, H]
    cc[4], cc[24:40], cc[60:76] = c[36], c[68:84], c[52:68]
    s.arrays["cameras"], s.arrays["cullingCameras"] = c.view(np.uint8), cc.view(np.uint8)
    near, far = float(l["nearPlane"]), float(l["farPlane"])
    o = orc.OracleFrame(s)
    o.cull(); o.raster(); depth = o.depth_copy()
    want = ref.capture_depth(depth, near, far)
    r = VisibilityRenderer(s)
    try:
        for st in (("clear_visibility",), ("cull", 1), ("raster", 1), ("depth_copy",)):
            r.stage(*st)
        out = r.torch.full((H, W), -7.0, dtype=r.torch.float32, device=r.device)
        d = capi.TextureDesc()
        d.texels, d.width, d.height, d.mipCount, d.format = out.data_ptr(), W, H, 1, capi.TEXTURE_FORMAT_R32_FLOAT
        r._check(r.lib.brmi_shadow_capture(r._h, capi.f32(near), capi.f32(far), C.byref(d), r._s()), "brmi_shadow_capture")
        r.torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(r.depth().view(np.uint32), depth.view(np.uint32))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        background = depth.view(np.uint32) == ref.EMPTY_DEPTH_BITS
        assert background.any() and (~background).sum() > 0.05 * W * H and np.all(got[background] == 1.0)
        d.width = W + 1
        assert r.lib.brmi_shadow_capture(r._h, capi.f32(near), capi.f32(far), C.byref(d), r._s()) != 0      # not the pass's size
    finally:
        r.close()


# ---- 2. the two functions -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cases.MAP_KINDS)
@pytest.mark.parametrize("size", cases.SPOT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_spot_function(renderer, kind, size):
    _, margin = cases.margin()
    c = cases.spot_case()
    sd = _bind(renderer, size)
    _load(renderer, sd["views"][0], cases.synthetic_map(kind, size[0], size[1], c["light"]))
    got = renderer.debug_shadow(c["index"], c["pos"], c["nrm"])
    want = cases.spot_results(kind, size, np.float64)
    fragile = ref.spot_fragile(want, margin)
    print(f"spot {kind} {size}: {int(fragile.sum())} fragile, {int((got != want['shadow'])[~fragile].sum())} of {int((~fragile).sum())} differ")
    assert np.all((got == 0.0) | (got == 1.0))
    assert np.array_equal(got[~fragile], want["shadow"][~fragile])


@pytest.mark.parametrize("kind", cases.MAP_KINDS)
def test_point_function(renderer, kind):
    _, margin = cases.margin()
    c = cases.point_case()
    sd = _bind(renderer)
    for f, m in enumerate(cases.cube_maps(kind, c["light"])):
        _load(renderer, sd["views"][1 + f], m)
    got = renderer.debug_shadow(c["index"], c["pos"], c["nrm"])
    want = cases.point_results(kind, np.float64)
    fragile = ref.point_fragile(want, margin)
    print(f"point {kind}: {int(fragile.sum())} fragile, {int((got != want['shadow'])[~fragile].sum())} of {int((~fragile).sum())} differ")
    assert np.all((got == 0.0) | (got == 1.0))
    assert np.array_equal(got[~fragile], want["shadow"][~fragile])


# ---- 3. frames ------------------------------------------------------------------------------------------
def _half_ulp_distance(a_bits, b_bits):
    """fp16 ULP distance of two arrays of half bit patterns (the project's HDR bound, test_parity_gpu.py)"""
    def key(h):
        h = h.astype(np.int32)
        return np.where(h & 0x8000, -(h & 0x7FFF), h & 0x7FFF)
    return np.abs(key(a_bits) - key(b_bits))


def _halves(hdr, mask):
    return hdr[mask].view(np.uint16).reshape(-1, 4)


@pytest.mark.parametrize("env", [0, 1], ids=["punctual", "environment"])
@pytest.mark.parametrize("clustered", [1, 0], ids=["clustered", "unclustered"])
@pytest.mark.parametrize("name", ["tiny", "sponza"])
def test_frames_select_the_restatements_candidate(name, clustered, env):
    """One shadowed spot and one shadowed point light among the unshadowed rest; 128 x 128 spot map and 64 x 64 faces from render_shadow_maps().  A shadow is
    binary, so a pixel of the shadowed frame is one of four frames: the one without shadows in which each subset of the two lights has intensity 0.  The float64
    restatement (from the frame's own depth and normals and the oracle-rendered maps) says which; the kernels' pixel must be within one fp16 ULP of that
    candidate, a fragile pixel within one ULP of any of the four.  Without an environment the candidates are the ORACLE's frames.  The oracle knows no environment:
    there (the clustered sponza case also with XeGTAO bound) the candidates are the same pass's frames without shadows, which tests/test_ibl_gpu.py and
    test_gtao_gpu.py hold.  Depth and the seven G-buffer surfaces equal the oracle's bit for bit, and the rendered maps equal the oracle's light views through
    the fp32 conversion.  The sponza scene has coated and fuzzy materials: every MODE of the three shadowed kernel families runs."""
    import shadow_frames as frames
    from basicrenderer_amd import shadows as sh
    from basicrenderer_amd.renderer import VisibilityRenderer
    sc = frames.scene(name)
    spot, point = frames.shadowed_lights(name)
    _, margin = frames.frame_margin()
    o = frames.oracle_frame(name)
    covered = frames.receivers(name)[0]
    r = VisibilityRenderer(sc, enableClusteredLighting=clustered)
    try:
        if env:
            from basicrenderer_amd.environment import Environment
            r.set_environment(Environment.procedural(16))
            if name == "sponza" and clustered:
                r.set_gtao("low")
            rec = sc.arrays["lights"].view(sh.LIGHT_DTYPE).copy()
            cand = []
            for k in range(4):
                sub = rec.copy()
                if k & 1:
                    sub["color"][spot, 3] = 0.0
                if k & 2:
                    sub["color"][point, 3] = 0.0
                r.device_arrays["lights"].copy_(r.torch.from_numpy(sub.view(np.uint8)).to(r.device))
                cand.append(_frame(r))
            r.device_arrays["lights"].copy_(r.torch.from_numpy(rec.view(np.uint8)).to(r.device))
        else:
            cand = frames.candidates(name, clustered)
        r.set_shadows([spot, point], resolution=frames.SPOT_RES, point_resolution=frames.FACE_RES)
        r.render_shadow_maps()
        maps, want_maps = r.shadow_maps(), frames.oracle_maps(name)[0]
        for k, (a, b) in enumerate(zip(maps, want_maps)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"map {k}"
        hdr = _frame(r)
        spot_sh, point_sh, fragile, reach_s, reach_p = frames.judged(name, clustered, margin, maps)
        pick = spot_sh.astype(np.int64) | (point_sh.astype(np.int64) << 1)
        got = _halves(hdr, covered)
        dist = np.stack([_half_ulp_distance(got, _halves(c, covered)).max(axis=1) for c in cand], 0)      # [candidate, pixel]
        chosen = dist[pick, np.arange(len(pick))]
        moved = (_halves(cand[0], covered) != got).any(axis=1)
        print(f"{name} clustered={clustered} env={env}: {len(pick)} pixels, {int(fragile.sum())} fragile, {int(moved.sum())} differ from the unshadowed frame, "
              f"{int((chosen[~fragile] > 1).sum())} miss their candidate, worst {int(chosen[~fragile].max())} ULP; candidates picked {np.bincount(pick, minlength=4).tolist()}")
        assert chosen[~fragile].max() <= 1
        assert dist.min(axis=0).max() <= 1
        assert moved.mean() > 0.01
        assert np.array_equal(hdr[~covered], cand[0][~covered])
        assert np.array_equal(r.depth().view(np.uint32), o.depth.view(np.uint32))
        g = r.gbuffer()
        for key, want in (("normals", o.normals), ("albedo", o.albedo), ("coat", o.coat), ("emissive", o.emissive), ("fuzz", o.fuzz), ("mr", o.mr), ("motion", o.motion)):
            assert np.array_equal(g[key].view(np.uint8), want.view(np.uint8)), key
    finally:
        r.close()


# ---- 4. off is off, 5. frames in flight -------------------------------------------------------------
def _frame(r, split=False):
    r.update()
    if split:
        side = r.torch.cuda.Stream(device=r.device)
        r.execute(shading_stream=side)
    else:
        r.execute()
    r.torch.cuda.synchronize()
    return r.hdr().copy()


@pytest.mark.parametrize("clustered", [1, 0], ids=["clustered", "unclustered"])
def test_off_is_off_and_split(clustered):
    from basicrenderer_amd import capi, shadows as sh
    from basicrenderer_amd.renderer import VisibilityRenderer
    rec, spot, point = cases.lights()
    r = VisibilityRenderer(cases.scene(), enableClusteredLighting=clustered)
    try:
        plain = _frame(r)
        r.set_shadows([spot, point], resolution=128, point_resolution=64)
        r.render_shadow_maps()
        maps = r.shadow_maps()
        assert len(maps) == 7 and all(m.dtype == np.float32 for m in maps)
        assert all(((m > 0) & (m <= 1)).all() for m in maps) and any((m < 1).any() for m in maps)
        shadowed = _frame(r)
        changed = (shadowed != plain).mean()
        print(f"clustered={clustered}: {changed:.3f} of the pixels change with shadows bound")
        assert changed > 0.01                       # the two lights do cast shadows in this frame
        # a shadow only ever removes a light's (non-negative) contribution
        assert np.all(orc_rgb(shadowed) <= orc_rgb(plain) + 1e-6)
        assert np.array_equal(_frame(r, split=True), shadowed)      # brmi_execute_split gives the bytes of brmi_execute
        # a bound pass whose lights all carry -1: byte for byte the frame without
        sd = r._shadows
        off = sd["lights"].copy()
        for k in ("shadowViewInfoIndex", "shadowMapIndex"):
            off[k] = -1
        r.device_arrays["lights"].copy_(r.torch.from_numpy(off.view(np.uint8)).to(r.device))
        assert np.array_equal(_frame(r), plain)
        # a directional light with shadow fields set is unshadowed
        directional = np.flatnonzero(off["type"] == sh.LIGHT_DIRECTIONAL)
        assert len(directional) >= 1
        off["shadowViewInfoIndex"][directional[0]], off["shadowMapIndex"][directional[0]] = 0, 0
        r.device_arrays["lights"].copy_(r.torch.from_numpy(off.view(np.uint8)).to(r.device))
        assert np.array_equal(_frame(r), plain)
        # the three invalid bindings
        b = sd["buffers"]
        bad = sd["lights"].copy(); bad["shadowMapIndex"][spot] = 7
        r.device_arrays["lights"].copy_(r.torch.from_numpy(bad.view(np.uint8)).to(r.device)); r.torch.cuda.synchronize()
        assert r.lib.brmi_set_shadows(r._h, C.byref(b)) == -1 and b"shadow map" in r.lib.brmi_last_error(r._h)
        r.device_arrays["lights"].copy_(r.torch.from_numpy(sd["lights"].view(np.uint8)).to(r.device)); r.torch.cuda.synchronize()
        keep_ptr = b.spotCameraIndices
        wrong = r.torch.from_numpy(np.array([int(r.sb.cameraCount)], dtype=np.int32)).to(r.device)
        b.spotCameraIndices = wrong.data_ptr()
        assert r.lib.brmi_set_shadows(r._h, C.byref(b)) == -1 and b"spot view" in r.lib.brmi_last_error(r._h)
        b.spotCameraIndices = keep_ptr
        sd["views"][2]["desc"].format = capi.TEXTURE_FORMAT_RGBA8_UNORM
        table = r.torch.from_numpy(np.frombuffer(b"".join(bytes(x["desc"]) for x in sd["views"]), dtype=np.uint8).copy()).to(r.device)
        keep_maps, b.maps = b.maps, table.data_ptr()
        assert r.lib.brmi_set_shadows(r._h, C.byref(b)) == -1 and b"format" in r.lib.brmi_last_error(r._h)
        b.maps = keep_maps
        sd["views"][2]["desc"].format = capi.TEXTURE_FORMAT_R32_FLOAT
        # the refused calls changed nothing; unbinding reproduces the frame without shadows byte for byte
        assert np.array_equal(_frame(r), shadowed)
        r.set_shadows(None)
        assert np.array_equal(_frame(r), plain)
    finally:
        r.close()


def orc_rgb(hdr):
    return hdr.view(np.float16).reshape(hdr.shape + (4,))[..., :3].astype(np.float32)
