"""numpy restatement of the temporal resolve (brmi_temporal_math.h) in float32, and the synthetic cases the host program and the kernel are held to.

Every operation is a separate float32 operation in the header's order; halves go through np.float16; min / max are np.fmin / np.fmax (fminf / fmaxf: the other
operand for a NaN).  No transcendental function is involved, so header and kernel must match this bit for bit.
"""
import numpy as np

F = np.float32
DEPTH_EMPTY = np.array([0x7F7FFFFF], dtype=np.uint32).view(np.float32)[0]
MIN_INVERSE, MAX_HALF = F(2.0 ** -16), F(65504.0)
SIZES = [(100, 72), (50, 36)]


def unpack(u64):
    """(H, W) uint64 -> (H, W, 3) float32 colour, (H, W) uint16 alpha bits."""
    h = np.ascontiguousarray(u64).view(np.uint16).reshape(u64.shape + (4,))
    return h[..., :3].view(np.float16).astype(F), h[..., 3].copy()


def pack(rgb16, alpha_bits):
    out = np.empty(rgb16.shape[:2] + (4,), dtype=np.uint16)
    out[..., :3] = np.ascontiguousarray(rgb16).view(np.uint16)
    out[..., 3] = alpha_bits
    return out.view(np.uint64)[..., 0]


def to_half(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=F).astype(np.float16)


def max3(c):
    return np.fmax(np.fmax(c[..., 0], c[..., 1]), c[..., 2])


def to_w(c):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = (F(1.0) + max3(c)).astype(F)
        return (c / d[..., None]).astype(F)


def halton(i, b):
    f, r, bf = F(1.0), F(0.0), F(b)
    while i > 0:
        f = F(f / bf)
        r = F(r + F(f * F(i % b)))
        i = int(np.floor(F(F(i) / bf)))
    return r


def jitter_offset(frame_index, phases=16):
    i = frame_index % phases
    return F(halton(i + 1, 2) - F(0.5)), F(halton(i + 1, 3) - F(0.5))


def resolve(hdr, depth, motion, history, blend=0.1):
    """hdr, history (or None): (H, W) uint64; depth (H, W) float32; motion (H, W) uint32 (two halves).  Returns (out (H, W) uint64, present (H, W) bool)."""
    H, W = hdr.shape
    blend = F(blend)
    cur, alpha = unpack(hdr)
    w16 = to_half(to_w(cur)).astype(F)                               # the neighbourhood is stored as halves
    wp = np.pad(w16, ((1, 1), (1, 1), (0, 0)), mode="edge")          # coordinates clamped to the frame
    dp = np.pad(np.asarray(depth, dtype=F), 1, mode="edge")
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    lo = hi = None
    best = bx = by = None
    for dy in range(3):
        for dx in range(3):
            w = wp[dy: dy + H, dx: dx + W]
            d = dp[dy: dy + H, dx: dx + W]
            nx, ny = np.clip(xs + dx - 1, 0, W - 1), np.clip(ys + dy - 1, 0, H - 1)
            if lo is None:
                lo, hi, best, bx, by = w.copy(), w.copy(), d.copy(), nx.copy(), ny.copy()
            else:
                lo, hi = np.fmin(lo, w), np.fmax(hi, w)
                with np.errstate(invalid="ignore"):
                    closer = d < best                                   # strictly: the first in row-major order keeps a tie
                best, bx, by = np.where(closer, d, best), np.where(closer, nx, bx), np.where(closer, ny, by)
    out = np.array(hdr, dtype=np.uint64, copy=True)
    present = np.zeros((H, W), dtype=bool)
    if history is None:
        return out, present
    mv = np.ascontiguousarray(motion[by, bx]).view(np.uint16).reshape(H, W, 2).view(np.float16).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        prev_x = ((xs.astype(F) + F(0.5)) - ((F(0.5) * mv[..., 0]).astype(F) * F(W)).astype(F)).astype(F)
        prev_y = ((ys.astype(F) + F(0.5)) + ((F(0.5) * mv[..., 1]).astype(F) * F(H)).astype(F)).astype(F)
        x, y = (prev_x - F(0.5)).astype(F), (prev_y - F(0.5)).astype(F)
        inside = (x >= F(0)) & (x <= F(W - 1)) & (y >= F(0)) & (y <= F(H - 1))
    xi, yi = np.where(inside, x, F(0)), np.where(inside, y, F(0))
    x0f, y0f = np.floor(xi).astype(F), np.floor(yi).astype(F)
    fx, fy = (xi - x0f).astype(F), (yi - y0f).astype(F)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    hist, _ = unpack(history)
    t00, t10, t01, t11 = hist[y0, x0], hist[y0, x1], hist[y1, x0], hist[y1, x1]
    with np.errstate(invalid="ignore", over="ignore"):
        r0 = (t00 + (fx[..., None] * (t10 - t00).astype(F)).astype(F)).astype(F)
        r1 = (t01 + (fx[..., None] * (t11 - t01).astype(F)).astype(F)).astype(F)
        h = (r0 + (fy[..., None] * (r1 - r0).astype(F)).astype(F)).astype(F)
    present = inside & np.isfinite(h).all(axis=-1)
    hs = np.where(present[..., None], h, F(0))
    hw = to_w(hs)
    hc = np.fmin(np.fmax(hw, lo), hi)
    cw = w16
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = (hc + (blend * (cw - hc).astype(F)).astype(F)).astype(F)
        m = max3(r)
        den = np.fmax((F(1.0) - m).astype(F), MIN_INVERSE)
        c = np.fmin((r / den[..., None]).astype(F), MAX_HALF)
    resolved = pack(to_half(c), alpha)
    out[present] = resolved[present]
    return out, present


# ---------------------------------------------------------------- synthetic cases ------------------------------------------------------------------------
def _motion_words(mvx, mvy):
    m = np.stack([to_half(mvx), to_half(mvy)], axis=-1)
    return np.ascontiguousarray(m).view(np.uint32)[..., 0]


def motion_of_pixels(dx, dy, W, H, shape=None):
    """The motion plane that moves the history sample by (dx, dy) pixels: prev = p + (dx, dy), i.e. mv = (-2 dx / W, 2 dy / H), rounded to halves."""
    shape = shape or (H, W)
    return _motion_words(np.full(shape, -2.0 * dx / W, dtype=F), np.full(shape, 2.0 * dy / H, dtype=F))


def _content(rng, W, H, bright=True):
    c = np.exp2(rng.uniform(-8, 4, size=(H, W, 3))).astype(F)
    if bright:
        k = rng.integers(0, W * H, size=max(4, W * H // 50))
        c.reshape(-1, 3)[k] *= np.exp2(rng.uniform(6, 11, size=(len(k), 1))).astype(F)      # up to 16 * 2048: well above 1000
    alpha = rng.integers(0, 0x7C00, size=(H, W)).astype(np.uint16)
    return pack(to_half(c), alpha)


CASES = ["zero_motion", "fractional", "left", "right", "up", "down", "no_history", "non_finite", "fireflies", "dilated", "ties", "empty_depth"]


def case(kind, W, H):
    """dict(hdr, depth, motion, history or None, blend) of one synthetic case."""
    rng = np.random.default_rng(sum(map(ord, kind)) * 1009 + W)
    hdr, history = _content(rng, W, H), _content(rng, W, H)
    depth = rng.uniform(0.5, 60.0, size=(H, W)).astype(F)
    motion = motion_of_pixels(0.0, 0.0, W, H)
    blend = 0.1
    if kind == "fractional":
        motion = motion_of_pixels(0.37, -0.61, W, H)
    elif kind in ("left", "right", "up", "down"):
        dx, dy = dict(left=(-1.5, 0.0), right=(1.5, 0.0), up=(0.0, -1.5), down=(0.0, 1.5))[kind]
        motion = motion_of_pixels(dx, dy, W, H)
    elif kind == "no_history":
        history = None
    elif kind == "non_finite":
        h = np.ascontiguousarray(history).view(np.uint16).reshape(H, W, 4)
        k = rng.integers(0, W * H, size=40)
        h.reshape(-1, 4)[k[:14], 0] = 0x7C00      # +inf
        h.reshape(-1, 4)[k[14:27], 1] = 0x7E00    # NaN
        h.reshape(-1, 4)[k[27:], 2] = 0xFC00      # -inf
        motion = motion_of_pixels(0.25, 0.5, W, H)
        blend = 0.25
    elif kind == "fireflies":
        hdr, history = _content(rng, W, H, bright=False), _content(rng, W, H, bright=False)
        hh = np.ascontiguousarray(history).view(np.uint16).reshape(H, W, 4)
        ch = np.ascontiguousarray(hdr).view(np.uint16).reshape(H, W, 4)
        for (x, y) in [(5, 5), (W - 1, 3), (17, H - 1), (W // 2, H // 2)]:
            hh[y, x, :3] = np.array([30000.0, 20000.0, 65504.0], dtype=np.float16).view(np.uint16)
            ch[(y + 7) % H, (x + 9) % W, :3] = np.array([65504.0, 4000.0, 900.0], dtype=np.float16).view(np.uint16)
        hdr, history = ch.view(np.uint64)[..., 0], hh.view(np.uint64)[..., 0]
    elif kind == "dilated":
        # a step edge: the near half (left) moves by 2.25 pixels, the far half does not
        near = np.arange(W)[None, :] < W // 2 + 3
        depth = np.where(near, F(2.0), F(40.0)).astype(F) * np.ones((H, 1), dtype=F)
        moving, still = motion_of_pixels(2.25, 0.0, W, H), motion_of_pixels(0.0, 0.0, W, H)
        motion = np.where(near, moving, still).astype(np.uint32)
    elif kind == "ties":
        depth = np.repeat(rng.integers(1, 4, size=(H, 1)).astype(F), W, axis=1)      # rows of equal depths, neighbouring rows often equal too
        motion = _motion_words(rng.uniform(-2.0, 2.0, size=(H, W)).astype(F) * F(2.0 / W), rng.uniform(-2.0, 2.0, size=(H, W)).astype(F) * F(2.0 / H))
    elif kind == "empty_depth":
        empty = rng.uniform(size=(H, W)) < 0.6
        depth = np.where(empty, DEPTH_EMPTY, depth).astype(F)
        motion = _motion_words(rng.uniform(-2.0, 2.0, size=(H, W)).astype(F) * F(2.0 / W), rng.uniform(-2.0, 2.0, size=(H, W)).astype(F) * F(2.0 / H))
    return dict(hdr=np.ascontiguousarray(hdr), depth=np.ascontiguousarray(depth), motion=np.ascontiguousarray(motion), history=history, blend=blend)
