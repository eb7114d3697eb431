"""A small .glb assembled with struct.pack, and a PNG encoder of the test's own (every filter, colour types 0 / 2 / 3 / 4 / 6)."""
import json
import struct
import zlib

import numpy as np


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def encode_png(px, ctype, filters, palette=None, trns=None):
    """px: (h, w, channels) uint8 in the colour type's own channels; filters: one filter type per row."""
    h, w, bpp = px.shape
    rows, prev = [], [0] * (w * bpp)
    for y in range(h):
        cur = [int(v) for v in px[y].reshape(-1)]
        f, out = filters[y % len(filters)], []
        for i, v in enumerate(cur):
            a = cur[i - bpp] if i >= bpp else 0
            b, c = prev[i], (prev[i - bpp] if i >= bpp else 0)
            pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[f]
            out.append((v - pred) & 255)
        rows.append(bytes([f]) + bytes(out)); prev = cur

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))
    data = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0))
    if palette is not None:
        data += chunk(b"PLTE", bytes(np.asarray(palette, np.uint8).reshape(-1)))
    if trns is not None:
        data += chunk(b"tRNS", bytes(np.asarray(trns, np.uint8)))
    raw = zlib.compress(b"".join(rows))
    return data + chunk(b"IDAT", raw[: len(raw) // 2]) + chunk(b"IDAT", raw[len(raw) // 2:]) + chunk(b"IEND", b"")


def mask_image():
    """8 x 8 RGBA: coloured, with a 4 x 4 hole of alpha 0 in the middle"""
    rng = np.random.default_rng(5)
    img = rng.integers(40, 250, (8, 8, 4), dtype=np.uint8); img[..., 3] = 255; img[2:6, 2:6, 3] = 0
    return img


def orm_image():
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (16, 4, 3), dtype=np.uint8)
    return img


def write_glb(path):
    """Two quads facing +z: the left one MASK with the 8 x 8 RGBA PNG (sampler: clamp / mirror, nearest mag, linear-mipmap-nearest min), the right one opaque
    with a metallic-roughness texture on TEXCOORD_1 (no sampler: the defaults), occlusion sharing it, a normal and an emissive texture on TEXCOORD_0."""
    quad = lambda x0: np.array([[x0, -1, 0], [x0 + 2, -1, 0], [x0 + 2, 1, 0], [x0, 1, 0]], np.float32)
    uv0 = np.array([[0, 1], [1, 1], [1, 0], [0, 0]], np.float32)
    uv1 = np.array([[0, 2], [2, 2], [2, 0], [0, 0]], np.float32)
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint16)
    parts, views = [], []

    def add(b):
        off = sum(len(p) for p in parts); parts.append(b + b"\0" * (-len(b) % 4)); views.append({"buffer": 0, "byteOffset": off, "byteLength": len(b)}); return len(views) - 1
    v_pos = [add(quad(-2.1).tobytes()), add(quad(0.1).tobytes())]
    v_uv0, v_uv1, v_idx = add(uv0.tobytes()), add(uv1.tobytes()), add(idx.tobytes())
    v_mask = add(encode_png(mask_image(), 6, [0, 1, 2, 3, 4]))
    v_orm = add(encode_png(orm_image(), 2, [4, 3, 1]))
    acc = [{"bufferView": v_pos[0], "componentType": 5126, "count": 4, "type": "VEC3", "min": [-2.1, -1, 0], "max": [-0.1, 1, 0]},
           {"bufferView": v_pos[1], "componentType": 5126, "count": 4, "type": "VEC3", "min": [0.1, -1, 0], "max": [2.1, 1, 0]},
           {"bufferView": v_uv0, "componentType": 5126, "count": 4, "type": "VEC2"}, {"bufferView": v_uv1, "componentType": 5126, "count": 4, "type": "VEC2"},
           {"bufferView": v_idx, "componentType": 5123, "count": 6, "type": "SCALAR"}]
    doc = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [{"mesh": 0}],
           "meshes": [{"primitives": [{"attributes": {"POSITION": 0, "TEXCOORD_0": 2}, "indices": 4, "material": 0},
                                      {"attributes": {"POSITION": 1, "TEXCOORD_0": 2, "TEXCOORD_1": 3}, "indices": 4, "material": 1}]}],
           "materials": [{"name": "masked", "alphaMode": "MASK", "alphaCutoff": 0.4, "doubleSided": True,
                          "pbrMetallicRoughness": {"baseColorFactor": [0.9, 0.8, 0.7, 1.0], "baseColorTexture": {"index": 0}, "metallicFactor": 0.25, "roughnessFactor": 0.75}},
                         {"name": "opaque", "emissiveFactor": [0.5, 0.25, 0.125], "emissiveTexture": {"index": 2},
                          "normalTexture": {"index": 1}, "occlusionTexture": {"index": 1, "texCoord": 1},
                          "pbrMetallicRoughness": {"metallicRoughnessTexture": {"index": 1, "texCoord": 1}}}],
           "textures": [{"source": 0, "sampler": 0}, {"source": 1}, {"source": 1, "sampler": 1}],
           "samplers": [{"wrapS": 33071, "wrapT": 33648, "magFilter": 9728, "minFilter": 9985}, {"minFilter": 9729}],
           "images": [{"bufferView": v_mask, "mimeType": "image/png", "name": "mask"}, {"bufferView": v_orm, "mimeType": "image/png", "name": "orm"}],
           "bufferViews": views, "accessors": acc, "buffers": [{"byteLength": sum(len(p) for p in parts)}]}
    js = json.dumps(doc).encode(); js += b" " * (-len(js) % 4)
    blob = b"".join(parts)
    with open(path, "wb") as f:
        f.write(struct.pack("<4sII", b"glTF", 2, 12 + 8 + len(js) + 8 + len(blob)) + struct.pack("<I4s", len(js), b"JSON") + js + struct.pack("<I4s", len(blob), b"BIN\0") + blob)
    return path
