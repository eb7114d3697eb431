"""PNG -> (h, w, 4) uint8 RGBA with zlib and numpy (harness only; examples/render_obj.py writes PNG by hand the same way).
8 bits per sample, not interlaced, colour types 0 (grey), 2 (RGB), 3 (palette, with tRNS), 4 (grey + alpha), 6 (RGBA); all five row filters."""
import struct
import zlib

import numpy as np

_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


class PngError(ValueError):
    pass


def decode_png(data):
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise PngError("not a PNG file")
    off, idat, header, palette, trns = 8, [], None, None, None
    while off + 8 <= len(data):
        n, kind = struct.unpack_from(">I4s", data, off)
        body = data[off + 8: off + 8 + n]
        if len(body) != n:
            raise PngError("truncated chunk")
        if kind == b"IHDR":
            if n != 13:
                raise PngError("IHDR is not 13 bytes")
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"PLTE":
            if n % 3:
                raise PngError("PLTE length is not a multiple of 3")
            palette = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif kind == b"tRNS":
            trns = np.frombuffer(body, np.uint8)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
        off += 12 + n
    if header is None:
        raise PngError("no IHDR")
    w, h, depth, ctype, _, _, interlace = header
    if depth != 8 or interlace != 0 or ctype not in _CHANNELS or w == 0 or h == 0:
        raise PngError(f"unsupported PNG: bit depth {depth}, colour type {ctype}, interlace {interlace}")
    bpp = _CHANNELS[ctype]
    stride = w * bpp
    try:
        raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    except zlib.error as e:
        raise PngError(f"image data: {e}")
    if raw.size < h * (stride + 1):
        raise PngError("image data too short")
    raw = raw[: h * (stride + 1)].reshape(h, stride + 1)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        f, line = int(raw[y, 0]), raw[y, 1:].astype(np.int32)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + prev) & 255
        elif f in (1, 3, 4):      # left-dependent: a running pass per pixel, vectorised over the bytes of a pixel
            cur = np.zeros(stride, np.int32)
            left, upleft = np.zeros(bpp, np.int32), np.zeros(bpp, np.int32)
            for x in range(0, stride, bpp):
                up = prev[x:x + bpp]
                if f == 1:
                    pred = left
                elif f == 3:
                    pred = (left + up) >> 1
                else:
                    p = left + up - upleft
                    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
                    pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
                left = (line[x:x + bpp] + pred) & 255
                cur[x:x + bpp] = left
                upleft = up
        else:
            raise PngError(f"row filter {f}")
        out[y] = cur
        prev = cur
    px = out.reshape(h, w, bpp)
    rgba = np.full((h, w, 4), 255, np.uint8)
    if ctype == 0:
        rgba[..., :3] = px
    elif ctype == 2:
        rgba[..., :3] = px
    elif ctype == 4:
        rgba[..., :3] = px[..., :1]; rgba[..., 3] = px[..., 1]
    elif ctype == 6:
        rgba[...] = px
    else:
        if palette is None or int(px.max()) >= len(palette):
            raise PngError("palette index out of range")
        rgba[..., :3] = palette[px[..., 0]]
        if trns is not None:
            a = np.full(len(palette), 255, np.uint8); a[: len(trns)] = trns[: len(palette)]
            rgba[..., 3] = a[px[..., 0]]
    return rgba
