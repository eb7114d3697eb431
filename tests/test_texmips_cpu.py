"""The mip-chain restatement (tests/texmips_ref.py) held to its own properties, without a GPU."""
import numpy as np
import pytest

import texmips_ref as T

f32 = np.float32


def fence(w, h, pitch=8):
    """One-texel opaque wires on a transparent sheet: the content whose coverage a plain chain thins out level by level."""
    rng = np.random.default_rng(11)
    img = rng.integers(32, 224, (h, w, 4), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    img[..., 3] = np.where((x % pitch == 3) | (y % pitch == 3), 255, 0)
    return img


def covered_share(level):
    return float((T.unorm_decode(level[..., 3]) >= f32(0.5)).mean())


def test_level_sizes_and_offsets():
    assert T.level_sizes(130, 70, 8) == [(130, 70), (65, 35), (32, 17), (16, 8), (8, 4), (4, 2), (2, 1), (1, 1)]
    assert T.level_sizes(1, 37, 6) == [(1, 37), (1, 18), (1, 9), (1, 4), (1, 2), (1, 1)]
    offs, total = T.mip_offsets(5, 3, 3)
    assert offs == [0, 15, 17] and total == 18
    assert [T.full_mip_count(*s) for s in ((1, 1), (2, 2), (5, 3), (64, 64), (65, 33), (4096, 1))] == [1, 2, 3, 7, 7, 13]
    for (w, h) in ((5, 3), (65, 33), (130, 70)):
        n = T.full_mip_count(w, h)
        for chain in (T.plain_chain(T.noise_image(w, h, 1), 0, n)[0], T.alpha_chain(T.noise_image(w, h, 1), 0, n)[0]):
            assert [c.shape for c in chain] == [(lh, lw, 4) for lw, lh in T.level_sizes(w, h, n)]
            assert T.pack(chain).shape[0] == T.mip_offsets(w, h, n)[1]


@pytest.mark.parametrize("srgb", [0, 1])
def test_a_constant_image_stays_constant(srgb):
    colour = np.array((200, 17, 99, 140), np.uint8)
    # levels 1..6 come from level 0 (decoded once, encoded once) whatever the size
    for (w, h) in ((64, 64), (37, 21), (1, 37)):
        img = np.broadcast_to(colour, (h, w, 4)).copy()
        for chain in (T.plain_chain(img, srgb, T.full_mip_count(w, h))[0],):
            assert all((lvl == colour).all() for lvl in chain)
    # beyond level 6 the plain chain re-reads stored codes: a linear chain stays constant on any size (the re-read clamps to the level); an sRGB chain
    # encodes the codes a second time there, as the shader text has it, and stays constant only at the fixed points of the encode
    img = np.broadcast_to(colour, (70, 130, 4)).copy()
    chain = T.plain_chain(img, srgb, 8)[0]
    assert all((lvl == colour).all() for lvl in chain[:7])
    if srgb:
        assert (chain[7][..., 3] == 140).all() and not (chain[7][..., :3] == colour[:3]).all()
        for code in (0, 255):
            img = np.full((70, 130, 4), code, np.uint8)
            assert all((lvl == code).all() for lvl in T.plain_chain(img, 1, 8)[0])
    else:
        assert (chain[7] == colour).all()
    # the alpha chain of an opaque constant image: the scale is 0.55 / 1 and alpha stays saturated... only where it was 255
    img = np.broadcast_to(np.array((200, 17, 99, 255), np.uint8), (21, 37, 4)).copy()
    levels, _, _, scales = T.alpha_chain(img, srgb, T.full_mip_count(37, 21))
    assert all((lvl[..., :3] == (200, 17, 99)).all() for lvl in levels)


def test_the_inputs_of_the_gpu_tests_are_mostly_decided():
    """Before any image is looked at: on every test input at most 1 % of a level's texels lie within the encode's bound of a rounding cut."""
    for (w, h, mips, seed) in T.PLAIN_CASES:
        T.assert_mostly_decided(T.plain_chain(T.noise_image(w, h, seed), 1, mips)[1])
    for name, img in T.alpha_inputs().items():
        T.assert_mostly_decided(T.alpha_chain(img, 1, T.full_mip_count(img.shape[1], img.shape[0]))[1])
    assert 0.0 < T.ENCODE_BOUND < 1e-3


def round_holes(w, h, pitch=16, radius=4.5):
    """An opaque sheet with hard-edged round holes"""
    rng = np.random.default_rng(7)
    img = rng.integers(32, 224, (h, w, 4), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    d = np.hypot((x % pitch) - (pitch - 1) / 2.0, (y % pitch) - (pitch - 1) / 2.0)
    img[..., 3] = np.where(d < radius, 0, 255)
    return img


def _steps(levels, stats, scales, n):
    """per level: (total, target, covered, step): `step` = texels in the bins from the lowest one the scale still lifts to >= 128 up to the selected bin"""
    out = []
    for l in range(1, n):
        s = stats[l * T.STATS_WORDS:(l + 1) * T.STATS_WORDS]
        hist, total = s[T.HIST_BASE:T.HIST_BASE + 256].astype(np.int64), int(s[T.DST_TOTAL])
        target = min(total, max(1, int(np.rint(f32(s[T.PREV_COVERED]) / f32(s[T.PREV_TOTAL]) * f32(total)))))
        lifted = T.unorm_store(np.clip(T.unorm_decode(np.arange(256, dtype=np.uint8)) * scales[l], f32(0), f32(1))) >= 128
        acc = np.cumsum(hist[::-1])[::-1]
        selected = max([b for b in range(1, 256) if acc[b] >= target], default=255)
        lowest = int(np.argmax(lifted)) if lifted.any() else 256
        out.append((total, target, int(round(covered_share(levels[l]) * total)), int(hist[lowest:selected + 1].sum())))
    return out


@pytest.mark.parametrize("mask", ["round_holes", "fence"])
def test_alpha_chain_keeps_the_covered_share_where_the_plain_chain_thins_it_out(mask):
    """The property the feature exists for, on a mask of round holes (and on one-texel wires, where the plain chain loses everything).
    What the shader guarantees per level: the resolve aims at the SOURCE LEVEL's covered count and selects the bin at which the histogram, summed from 255
    down, reaches it; 0.55 / selected lifts every bin from `lowest` (the smallest code that still stores >= 128) up.  So
        target <= covered <= target + (texels in bins [lowest, selected]) - 1:
    one step of the histogram's scan, asserted here for every level without exception.
    On the round holes every level's share is, beyond that, within ONE such step of LEVEL 0's share: asserted as the issue states it.  On the wires it is not
    (each level's target is the level above, not level 0, so the steps add up: level 2 is 0.516 from level 0 with a step of 0.5); there the sum of the steps so
    far is asserted, and the plain chain of the same wires leaves even that bound: its share falls to zero.  (On the round holes the plain chain stays inside:
    its share rises to 1 as the alpha chain's does.)"""
    img = round_holes(64, 64) if mask == "round_holes" else fence(64, 64)
    n = T.full_mip_count(64, 64)
    levels, _, stats, scales = T.alpha_chain(img, 0, n)
    plain = T.plain_chain(img, 0, n)[0]
    share0 = covered_share(levels[0])
    low = high = 0.0
    left = False
    for l, (total, target, covered, step) in enumerate(_steps(levels, stats, scales, n), start=1):
        a, p = covered_share(levels[l]), covered_share(plain[l])
        print(f"{mask} level {l}: {total} texels, target {target}, covered {covered}, step {step}, scale {scales[l]:.4f}, share {a:.4f} (level 0: {share0:.4f}), plain share {p:.4f}")
        assert target <= covered <= target + max(step, 1) - 1
        if mask == "round_holes":
            assert abs(a - share0) <= (max(step, 1) + 0.5) / total      # (+ 0.5: the rounding of the target)
        low += 0.5 / total
        high += (max(step, 1) - 0.5) / total
        assert share0 - low <= a <= share0 + high
        left = left or not (share0 - low <= p <= share0 + high)
    if mask == "fence":
        assert left, "the plain chain stayed inside the alpha chain's bound on this input"
        assert covered_share(plain[3]) == 0.0 and covered_share(levels[3]) > 0.0


def test_scale_resolves_to_one_and_reaches_its_clamps():
    s = np.zeros(T.STATS_WORDS, np.uint32)
    assert T.resolve_scale(s) == f32(1.0)                                     # empty destination (and empty source)
    s[T.PREV_TOTAL], s[T.DST_TOTAL], s[T.HIST_BASE] = 64, 16, 16
    assert T.resolve_scale(s) == f32(1.0)                                     # all-transparent source level: nothing covered
    s[T.PREV_COVERED] = 64; s[T.HIST_BASE] = 0; s[T.HIST_BASE + 3] = 16
    assert T.resolve_scale(s) == f32(16.0)                                    # 0.55 / (3 / 255) = 46.75, clamped
    s[T.HIST_BASE + 3] = 0; s[T.HIST_BASE + 255] = 16
    # selectedAlpha <= 1, so 0.55 / selectedAlpha >= 0.55: the clamp at 0.25 cannot be reached by any statistics; 0.55 is the least scale there is
    assert T.resolve_scale(s) == f32(0.55) / f32(1.0)
    # the same through whole chains
    inputs = T.alpha_inputs()
    assert (T.alpha_chain(inputs["transparent"], 0, 6)[3][1:] == f32(1.0)).all()
    # an image cannot reach either clamp (texmips_ref.alpha_inputs says why); these are the extremes it does reach
    assert T.alpha_chain(inputs["scale_high"], 0, 2)[3][1] == f32(0.55) / (f32(32.0) / f32(255.0))
    assert T.alpha_chain(inputs["scale_low"], 0, 2)[3][1] == f32(0.55)
    assert T.alpha_chain(inputs["opaque"], 0, 2)[3][1] == f32(0.55)


def test_half_to_even_cases_occur_in_the_histogram_inputs():
    """A 2 x 2 mean of 8-bit alphas times 255 can land on an exact half in fp32 (not every half of real arithmetic does: code / 255 rounds first); HLSL's
    round sends those to the even bin, where round-half-up would pick the bin above."""
    img = np.zeros((2, 2, 4), np.uint8)
    seen = 0
    down = 0
    for codes in ((1, 0, 0, 1), (1, 1, 1, 3), (2, 2, 2, 4), (255, 254, 254, 255), (9, 9, 9, 11), (17, 17, 16, 16)):
        img[..., 3] = np.array(codes, np.uint8).reshape(2, 2)
        a = (T.unorm_decode(img[..., 3]).sum(dtype=f32) * f32(0.25)) * f32(255.0)
        _, _, stats, _ = T.alpha_chain(img, 0, 2)
        hist = stats[T.STATS_WORDS + T.HIST_BASE:T.STATS_WORDS + T.HIST_BASE + 256]
        assert hist.sum() == 1 and hist[int(np.rint(a))] == 1, (codes, a, np.nonzero(hist))
        seen += int(a - np.floor(a) == 0.5)
        down += int(a - np.floor(a) == 0.5 and int(np.rint(a)) == int(np.floor(a)))
    assert seen >= 2 and down >= 1, "no constructed input landed on an exact half in fp32 that rounds down to even"
    holes = T.alpha_inputs()["holes"]
    a = T.unorm_decode(holes[..., 3])
    m = (((a[0::2, 0::2] + a[0::2, 1::2]) + a[1::2, 0::2]) + a[1::2, 1::2]) * f32(0.25) * f32(255.0)
    assert (m - np.floor(m) == 0.5).any(), "the round-holes input has no exact half among its level-1 alphas"
