"""Environments for the image-based lighting of the shading pass (brmi_set_environment).

An Environment is what one entry of the reference's EnvironmentInfo table names: a prefiltered cubemap -- six RGBA8 mip chains in the order +X -X +Y -Y +Z -Z -- and
the nine RGB coefficients of irradianceSH with their scale, and optionally the cube the skybox stage shows (six RGBA16F faces).  `procedural()` makes one from a
closed-form radiance; its mips are 2x2 box filters of the linear values unless prefilter="ggx" asks for the build below.  `from_equirect()` / `from_cube()` make
one from an image the way the reference does, on the device (brmi_env_convert, brmi_env_project_sh, brmi_env_prefilter): equirectangular panorama -> RGBA16F cube
-> the SH integers and the GGX-prefiltered RGBA8 chain.  `read_hdr()` reads a Radiance .hdr panorama.
"""
import numpy as np

from . import capi

FACES = ("+X", "-X", "+Y", "-Y", "+Z", "-Z")


def face_directions(size):
    """(6, size, size, 3) float64: the direction through every texel centre, by the Direct3D cube layout the sampler inverts (row = v, column = u;
    sc = 2u - 1, tc = 2v - 1 are the face coordinates of DESIGN.md 2)."""
    c = (np.arange(size, dtype=np.float64) + 0.5) / size * 2.0 - 1.0
    sc, tc = np.meshgrid(c, c, indexing="xy")
    one = np.ones_like(sc)
    d = np.stack([np.stack([one, -tc, -sc], -1), np.stack([-one, -tc, sc], -1),
                  np.stack([sc, one, tc], -1), np.stack([sc, -one, -tc], -1),
                  np.stack([sc, -tc, one], -1), np.stack([-sc, -tc, -one], -1)])
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


class Polynomial:
    """A radiance L(w) = c0 + a . w + w^T Q w per colour channel (degree <= 2 in the unit direction): c0 (3,), a (3 axes, 3 channels), Q (3, 3, 3 channels),
    Q symmetric in its first two axes.  Order-2 spherical harmonics hold it exactly."""

    def __init__(self, c0, a, Q):
        self.c0, self.a, self.Q = (np.asarray(v, dtype=np.float64) for v in (c0, a, Q))

    def __call__(self, w):
        w = np.asarray(w, dtype=np.float64)
        return self.c0 + np.einsum("...i,ic->...c", w, self.a) + np.einsum("...i,...j,ijc->...c", w, w, self.Q)

    def irradiance_coefficients(self):
        """(9, 3): the coefficients k of irradianceSH's basis (1, y, z, x, yx, yz, 3z^2 - 1, zx, x^2 - y^2) with sum k_i b_i(n) = E(n), the irradiance
        of L on a surface of normal n.  A band-l harmonic comes through the clamped-cosine convolution times pi, 2 pi / 3, pi / 4 (l = 0, 1, 2); the
        quadratic form splits into its trace (band 0) and its traceless part (band 2)."""
        tr = np.einsum("iic->c", self.Q)
        Qt = self.Q - np.eye(3)[:, :, None] * tr / 3.0
        k = np.zeros((9, 3))
        k[0] = np.pi * (self.c0 + tr / 3.0)
        k[1], k[2], k[3] = (2.0 * np.pi / 3.0) * self.a[1], (2.0 * np.pi / 3.0) * self.a[2], (2.0 * np.pi / 3.0) * self.a[0]
        q = np.pi / 4.0
        k[4], k[5], k[7] = q * 2.0 * Qt[0, 1], q * 2.0 * Qt[1, 2], q * 2.0 * Qt[0, 2]
        k[6] = q * Qt[2, 2] / 2.0
        k[8] = q * (Qt[0, 0] - Qt[1, 1]) / 2.0
        return k


def sky_polynomial(sky=(0.35, 0.55, 0.95), horizon=(0.85, 0.8, 0.7), ground=(0.25, 0.2, 0.15), side=(0.9, 0.6, 0.3)):
    """A sky gradient, a ground tint and a side tilt, every value in [0, 1]: with t = (1 + y) / 2,
    L = 0.8 * (ground (1 - t)^2 + horizon 2 t (1 - t) + sky t^2) + 0.1 * side * (1 + x)."""
    sky, horizon, ground, side = (np.asarray(v, dtype=np.float64) for v in (sky, horizon, ground, side))
    # in powers of y: (1 - t)^2 = (1 - 2y + y^2) / 4, 2 t (1 - t) = (1 - y^2) / 2, t^2 = (1 + 2y + y^2) / 4
    c0 = 0.8 * (ground / 4 + horizon / 2 + sky / 4) + 0.1 * side
    a = np.zeros((3, 3)); a[1] = 0.8 * (sky - ground) / 2; a[0] = 0.1 * side
    Q = np.zeros((3, 3, 3)); Q[1, 1] = 0.8 * (ground / 4 - horizon / 2 + sky / 4)
    return Polynomial(c0, a, Q)


def box_mips(level0):
    """The chain below an (n, n, 4) uint8 level: 2x2 box filters of the linear values (code / 255), each level rounded to nearest from the unrounded one above."""
    out, lin = [np.ascontiguousarray(level0, dtype=np.uint8)], level0.astype(np.float64) / 255.0
    while lin.shape[0] > 1:
        lin = 0.25 * (lin[0::2, 0::2] + lin[1::2, 0::2] + lin[0::2, 1::2] + lin[1::2, 1::2])
        out.append(np.clip(np.rint(lin * 255.0), 0, 255).astype(np.uint8))
    return out


class Environment:
    """faces: six lists of (n >> l, n >> l, 4) uint8 levels (+X -X +Y -Y +Z -Z, square, one size and level count); sh: (9, 3) int32 coefficients;
    scale: sphericalHarmonicsScale (a coefficient is worth sh * scale / 100)."""

    def __init__(self, faces, sh, scale, radiance=None, cube16=None, device_cubes=None):
        """cube16: (6, n, n, 4) float16, the cube cubeMapDescriptorIndex names (the sky the skybox stage shows), or None: the skybox then shows level 0 of the
        prefiltered cube.  device_cubes: the tensors a device build left (from_equirect / from_cube), for callers that bind tables themselves."""
        self.cube16 = None if cube16 is None else np.ascontiguousarray(cube16, dtype=np.float16)
        self.device_cubes = device_cubes
        self.faces = [[np.ascontiguousarray(l, dtype=np.uint8) for l in f] for f in faces]
        self.sh, self.scale, self.radiance = np.ascontiguousarray(sh, dtype=np.int32).reshape(9, 3), float(np.float32(scale)), radiance
        n, levels = self.faces[0][0].shape[0], len(self.faces[0])
        if len(self.faces) != 6 or any(len(f) != levels or any(l.shape != (max(1, n >> i), max(1, n >> i), 4) for i, l in enumerate(f)) for f in self.faces):
            raise ValueError("an environment needs six square faces of one size and level count")
        self.size, self.levels = n, levels

    @staticmethod
    def quantise(coefficients, max_radiance=1.0):
        """(sh, scale): the integers round(c * 100 / scale) with the smallest power-of-two scale whose rounding -- nine coefficients, half a step each,
        9 * 0.5 * scale / 100 -- stays below 1e-4 of the largest radiance, and under which every coefficient fits an int32."""
        c = np.asarray(coefficients, dtype=np.float64)
        scale = 2.0 ** np.floor(np.log2(1.0e-4 * max(max_radiance, 1e-30) * capi.SH_FLOAT_SCALE / 4.5 * (1 - 1e-9)))
        if np.abs(c).max(initial=0.0) * capi.SH_FLOAT_SCALE / scale >= 2.0 ** 31:
            raise ValueError("the coefficients do not fit 32-bit integers at the scale the accuracy bound asks for")
        return np.rint(c * capi.SH_FLOAT_SCALE / scale).astype(np.int32), float(scale)

    @classmethod
    def procedural(cls, size=16, radiance=None, levels=None, prefilter="box", device="cuda:0"):
        """The radiance (default: sky_polynomial()) at the texel centres, box-filtered mips (all of them, or `levels`), exact order-2 coefficients.
        prefilter="ggx": the chain and the SH integers come from the device build run on that level 0 (RGBA8) instead, as from_cube makes them."""
        radiance = radiance or sky_polynomial()
        L = radiance(face_directions(size))
        if prefilter == "ggx":
            level0 = np.concatenate([np.clip(L, 0.0, 1.0), np.ones((6, size, size, 1))], -1)
            env = build_on_device(cube=np.clip(np.rint(level0 * 255.0), 0, 255).astype(np.uint8), levels=levels, device=device)
            env.radiance = radiance
            return env
        if prefilter != "box":
            raise ValueError("prefilter is 'box' or 'ggx'")
        faces = []
        for f in range(6):
            rgba = np.concatenate([np.clip(L[f], 0.0, 1.0), np.ones((size, size, 1))], -1)
            chain = box_mips(np.clip(np.rint(rgba * 255.0), 0, 255).astype(np.uint8))
            faces.append(chain[:levels] if levels else chain)
        sh, scale = cls.quantise(radiance.irradiance_coefficients(), float(max(L.max(), 1e-30)))
        return cls(faces, sh, scale, radiance)

    @classmethod
    def constant(cls, colour, size=4):
        colour = np.asarray(colour, dtype=np.float64)
        return cls.procedural(size, Polynomial(colour, np.zeros((3, 3)), np.zeros((3, 3, 3))))

    @classmethod
    def from_equirect(cls, image, size=None, levels=None, device="cuda:0"):
        """(H, W, 3) float panorama (row 0 = up, as a .hdr file stores it) -> an Environment built on the device the way the reference builds one: faces of
        `size` (default: H / 2 rounded down to a power of two, at least 1), `levels` prefiltered levels (default: the whole chain, at most 16)."""
        image = np.asarray(image)
        if image.ndim != 3 or image.shape[2] < 3:
            raise ValueError("from_equirect takes an (H, W, 3) array")
        if size is None:
            size = 1 << max(0, int(np.floor(np.log2(max(1, image.shape[0] // 2)))))
        return build_on_device(equirect=image[..., :3], size=int(size), levels=levels, device=device)

    @classmethod
    def from_cube(cls, faces, levels=None, device="cuda:0"):
        """(6, n, n, 3 or 4) float faces (+X -X +Y -Y +Z -Z, row = v) -> the same build without the conversion; uint8 faces are taken as an RGBA8 cube."""
        return build_on_device(cube=np.asarray(faces), levels=levels, device=device)

    def info_words(self, cubemap_index, sky_index=None):
        """The 32 words of this environment's brmi_environment_info with `cubemap_index` as its prefiltered cubemap and `sky_index` (default: the same) as the
        cube the skybox stage shows."""
        w = np.zeros(32, dtype=np.uint32)
        w[0], w[1] = cubemap_index if sky_index is None else sky_index, cubemap_index
        w[2:3] = np.array([self.scale], dtype=np.float32).view(np.uint32)
        w[3:30] = self.sh.reshape(-1).view(np.uint32)
        return w

    def texel_words(self):
        """(texels uint8 blob, per face (size, levels, mip offsets in texels, byte offset of the face's chain in the blob))."""
        blob, faces, at = [], [], 0
        for f in self.faces:
            offs, t = [], 0
            for l in f:
                offs.append(t); t += l.shape[0] * l.shape[1]; blob.append(l.reshape(-1))
            faces.append((self.size, len(f), offs, at)); at += t * 4
        return np.ascontiguousarray(np.concatenate(blob)), faces


def environment_tables(environments, base_address_of):
    """Host images of the two device tables of brmi_environment_buffers for a list of n Environments (environment e reads cubemap e as its prefiltered cube):
    (info words (n, 32) uint32, descriptor words (6m, 24) uint32, texel blob uint8).  base_address_of(blob) -> the device address the blob will live at.
    An environment with a sky cube (cube16) gets a cubemap of its own behind the first n -- six one-level RGBA16F faces, 8-byte aligned in the blob -- and names
    it in cubeMapDescriptorIndex; the others name their prefiltered cube there, as they always did."""
    blobs, per, at_byte = [], [], 0
    for e in environments:
        b, faces = e.texel_words()
        per.append((at_byte, faces)); blobs.append(b); at_byte += len(b)
    skies = [i for i, e in enumerate(environments) if e.cube16 is not None]
    sky_start = {}
    for i in skies:
        pad = (-at_byte) % 8
        if pad:
            blobs.append(np.zeros(pad, dtype=np.uint8)); at_byte += pad
        b = environments[i].cube16.view(np.uint8).reshape(-1)
        sky_start[i] = at_byte; blobs.append(b); at_byte += len(b)
    blob = np.ascontiguousarray(np.concatenate(blobs))
    base = int(base_address_of(blob))
    if skies and base % 8:
        raise ValueError("the texel blob must be 8-byte aligned on the device (RGBA16F texels)")
    n = len(environments)
    info = np.stack([e.info_words(i, n + skies.index(i) if i in sky_start else None) for i, e in enumerate(environments)])
    descs = np.zeros((6 * (n + len(skies)), 24), dtype=np.uint32)
    for i, (start, faces) in enumerate(per):
        for f, (size, levels, offs, at) in enumerate(faces):
            d = descs[6 * i + f]
            addr = base + start + at
            d[0], d[1] = addr & 0xFFFFFFFF, addr >> 32
            d[2:6] = (size, size, levels, 0)
            d[6:6 + levels] = offs
    for k, i in enumerate(skies):
        size = environments[i].cube16.shape[1]
        for f in range(6):
            d = descs[6 * (n + k) + f]
            addr = base + sky_start[i] + f * size * size * 8
            d[0], d[1] = addr & 0xFFFFFFFF, addr >> 32
            d[2:6] = (size, size, 1, capi.TEXTURE_FORMAT_RGBA16_FLOAT)
    return info, descs, blob


# ------------------------------------------------------------------------------------------------ the device build
def descriptor_words(address, width, height, levels, fmt, offsets=None):
    """The 24 words of one brmi_texture_desc; offsets default to a tightly packed chain of max(1, w >> l) x max(1, h >> l) levels (in texels)."""
    d = np.zeros(24, dtype=np.uint32)
    d[0], d[1] = address & 0xFFFFFFFF, address >> 32
    d[2:6] = (width, height, levels, fmt)
    if offsets is None:
        offsets, t = [], 0
        for l in range(levels):
            offsets.append(t); t += max(1, width >> l) * max(1, height >> l)
    d[6:6 + levels] = offsets
    return d


def chain_texels(size, levels):
    return sum(max(1, size >> l) ** 2 for l in range(levels))


def build_on_device(equirect=None, cube=None, size=None, levels=None, device="cuda:0"):
    """convert (when `equirect` is given) + project + prefilter on `device`, read back into an Environment that also keeps the device tensors.
    equirect: (H, W, 3) float; cube: (6, n, n, 3 | 4) float (-> RGBA16F) or uint8 (6, n, n, 4) (-> an RGBA8 source cube, no sky cube of its own)."""
    import ctypes as C
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("the environment build runs on the GPU (brmi_env_*): there is no CPU path")
    lib, dev = capi.brmi_lib(), torch.device(device)
    torch.cuda.set_device(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    def rgba16(a):
        a = np.asarray(a, dtype=np.float32)
        if a.shape[-1] == 3:
            a = np.concatenate([a, np.ones(a.shape[:-1] + (1,), dtype=np.float32)], -1)
        return np.ascontiguousarray(a.astype(np.float16))

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc})")
    rgba8_source = cube is not None and np.asarray(cube).dtype == np.uint8
    if equirect is not None:
        src = rgba16(equirect)
        t_src = up(src)
        t_src_desc = up(descriptor_words(t_src.data_ptr(), src.shape[1], src.shape[0], 1, capi.TEXTURE_FORMAT_RGBA16_FLOAT))
        t_cube = torch.zeros(6 * size * size * 8, dtype=torch.uint8, device=dev)
    else:
        src = np.ascontiguousarray(cube) if rgba8_source else rgba16(cube)
        size = src.shape[1]
        t_cube = up(src)
    texel = 4 if rgba8_source else 8
    fmt = capi.TEXTURE_FORMAT_RGBA8_UNORM if rgba8_source else capi.TEXTURE_FORMAT_RGBA16_FLOAT
    t_cube_desc = up(np.stack([descriptor_words(t_cube.data_ptr() + f * size * size * texel, size, size, 1, fmt) for f in range(6)]))
    if equirect is not None:
        check(lib.brmi_env_convert(t_src_desc.data_ptr(), t_cube_desc.data_ptr(), size, capi.TEXTURE_FORMAT_RGBA16_FLOAT, stream), "brmi_env_convert")
    levels = int(levels) if levels else min(capi.TEXTURE_MAX_MIPS, int(np.floor(np.log2(size))) + 1)
    info = np.zeros(32, dtype=np.uint32)
    t_info = up(info)
    check(lib.brmi_env_project_sh(t_cube_desc.data_ptr(), 1, t_info.data_ptr(), 1, 0, size, stream), "brmi_env_project_sh")
    per_face = chain_texels(size, levels)
    t_chain = torch.zeros(6 * per_face * 4, dtype=torch.uint8, device=dev)
    t_chain_desc = up(np.stack([descriptor_words(t_chain.data_ptr() + f * per_face * 4, size, size, levels, capi.TEXTURE_FORMAT_RGBA8_UNORM) for f in range(6)]))
    check(lib.brmi_env_prefilter(t_cube_desc.data_ptr(), t_chain_desc.data_ptr(), size, levels, capi.TEXTURE_FORMAT_RGBA8_UNORM, stream), "brmi_env_prefilter")
    torch.cuda.synchronize(dev)
    words = t_info.cpu().numpy().view(np.uint32)
    chain = t_chain.cpu().numpy().reshape(6, per_face, 4)
    faces = []
    for f in range(6):
        levels_f, t = [], 0
        for l in range(levels):
            s = max(1, size >> l)
            levels_f.append(chain[f, t:t + s * s].reshape(s, s, 4)); t += s * s
        faces.append(levels_f)
    cube16 = None if rgba8_source else t_cube.cpu().numpy().view(np.float16).reshape(6, size, size, 4)
    keep = dict(cube=t_cube, cube_descs=t_cube_desc, prefiltered=t_chain, prefiltered_descs=t_chain_desc, info=t_info)
    return Environment(faces, words[3:30].view(np.int32), float(words[2:3].view(np.float32)[0]), cube16=cube16, device_cubes=keep)


# ------------------------------------------------------------------------------------------------ Radiance .hdr
def read_hdr(source):
    """A Radiance picture (RGBE; flat or new-style run-length scanlines, the standard -Y H +X W orientation) from a path or bytes -> (H, W, 3) float32.
    A pixel is mantissa * 2^(exponent - 136) per channel, (0, 0, 0) where the exponent byte is 0."""
    data = source if isinstance(source, (bytes, bytearray)) else open(source, "rb").read()
    if not (data.startswith(b"#?RADIANCE") or data.startswith(b"#?RGBE")):
        raise ValueError("not a Radiance .hdr file")
    end = data.find(b"\n\n")
    if end < 0:
        raise ValueError("the .hdr header does not end")
    header = data[:end].split(b"\n")
    if not any(l.strip().replace(b" ", b"") == b"FORMAT=32-bit_rle_rgbe" for l in header):
        raise ValueError("only FORMAT=32-bit_rle_rgbe is read")
    eol = data.find(b"\n", end + 2)
    dims = data[end + 2:eol].split()
    if len(dims) != 4 or dims[0] != b"-Y" or dims[2] != b"+X":
        raise ValueError("only the -Y H +X W orientation is read")
    H, W = int(dims[1]), int(dims[3])
    buf = np.frombuffer(data, dtype=np.uint8, offset=eol + 1)
    out = np.zeros((H, W, 4), dtype=np.uint8)
    at = 0
    for y in range(H):
        if 8 <= W <= 0x7FFF and at + 4 <= len(buf) and buf[at] == 2 and buf[at + 1] == 2 and not buf[at + 2] & 0x80 and (int(buf[at + 2]) << 8 | int(buf[at + 3])) == W:
            at += 4
            for c in range(4):
                x = 0
                while x < W:
                    if at + 2 > len(buf):
                        raise ValueError("the .hdr file ends inside a scanline")
                    n = int(buf[at]); at += 1
                    if n > 128:
                        n -= 128
                        if n == 0 or x + n > W:
                            raise ValueError("a bad run in the .hdr scanline")
                        out[y, x:x + n, c] = buf[at]; at += 1
                    else:
                        if n == 0 or x + n > W:
                            raise ValueError("a bad literal count in the .hdr scanline")
                        if at + n > len(buf):
                            raise ValueError("the .hdr file ends inside a scanline")
                        out[y, x:x + n, c] = buf[at:at + n]; at += n
                    x += n
        else:
            if at + 4 * W > len(buf):
                raise ValueError("the .hdr file ends inside a scanline")
            out[y] = buf[at:at + 4 * W].reshape(W, 4); at += 4 * W
    e = out[..., 3].astype(np.int32)
    scale = np.where(e == 0, 0.0, np.ldexp(1.0, e - 136)).astype(np.float32)
    return (out[..., :3].astype(np.float32) * scale[..., None]).astype(np.float32)
