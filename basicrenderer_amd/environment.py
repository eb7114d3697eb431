"""Environments for the image-based lighting of the shading pass (brmi_set_environment).

An Environment is what one entry of the reference's EnvironmentInfo table names: a prefiltered cubemap -- six RGBA8 mip chains in the order +X -X +Y -Y +Z -Z -- and
the nine RGB coefficients of irradianceSH with their scale.  `procedural()` makes one from a closed-form radiance.  Its mips are 2x2 box filters of the linear
values: a stand-in for the reference's GGX prefilter pass, which is not part of this path (a rougher lookup reads a blurrier sky, not the BRDF-weighted one).
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

    def __init__(self, faces, sh, scale, radiance=None):
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
    def procedural(cls, size=16, radiance=None, levels=None):
        """The radiance (default: sky_polynomial()) at the texel centres, box-filtered mips (all of them, or `levels`), exact order-2 coefficients."""
        radiance = radiance or sky_polynomial()
        L = radiance(face_directions(size))
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

    def info_words(self, cubemap_index):
        """The 32 words of this environment's brmi_environment_info with `cubemap_index` as its prefiltered cubemap."""
        w = np.zeros(32, dtype=np.uint32)
        w[0], w[1] = cubemap_index, cubemap_index
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
    """Host images of the two device tables of brmi_environment_buffers for a list of Environments (environment e reads cubemap e):
    (info words (n, 32) uint32, descriptor words (6n, 24) uint32, texel blob uint8).  base_address_of(blob) -> the device address the blob will live at."""
    blobs, per = [], []
    for e in environments:
        b, faces = e.texel_words()
        per.append((sum(len(x) for x in blobs), faces)); blobs.append(b)
    blob = np.ascontiguousarray(np.concatenate(blobs))
    base = int(base_address_of(blob))
    info = np.stack([e.info_words(i) for i, e in enumerate(environments)])
    descs = np.zeros((6 * len(environments), 24), dtype=np.uint32)
    for i, (start, faces) in enumerate(per):
        for f, (size, levels, offs, at) in enumerate(faces):
            d = descs[6 * i + f]
            addr = base + start + at
            d[0], d[1] = addr & 0xFFFFFFFF, addr >> 32
            d[2:6] = (size, size, levels, 0)
            d[6:6 + levels] = offs
    return info, descs, blob
