"""Cases of the training-time augmentation (uenc/train_data.py, csrc/augment.hip), shared by tests/test_augment_cases_cpu.py (which
pins the host rules against PIL, torch and plain Python loops) and tests/test_augment_kernels_gpu.py (which holds both kernels against
the host path, bit for bit).  Every output is uint8 or int32: every comparison is equality.

The image kernel makes 64 x 16 output tiles (UENC_AUG_TILE_W x UENC_AUG_TILE_H), a thread stores four pixels as one 32-bit word when the
output width is a multiple of 4 and as bytes otherwise; the label kernel stores int4 under the same condition.  Which case takes which
branch is said per case below.  Source sizes are tens of pixels; scale factors run from 0.5 (5 taps per axis) to 2.0 (3 taps)."""
import functools
import itertools

import numpy as np

TILE_W, TILE_H = 64, 16

# id, source (h, w), resized (h, w), crop (x0, y0, cw, ch), flip, output (h, w) or None = the crop's own, frames, label dtype or None
GEOMETRY = [
    # x2 both axes, whole image: 2 x 4 tiles, ragged last tile column (122 = 64 + 58) and row (60 = 3 * 16 + 12), byte stores (122 % 4)
    ("up2_full_f4", (30, 61), (60, 122), (0, 0, 122, 60), False, None, 4, "uint8"),
    ("up2_full_flip", (30, 61), (60, 122), (0, 0, 122, 60), True, None, 1, "uint8"),
    # x0.5 (5 taps), a window smaller than one tile at odd offsets, away from every border
    ("down2_inner_odd", (24, 48), (12, 24), (3, 2, 17, 9), False, None, 1, "uint8"),
    # x0.5, the window in the bottom-right corner (taps clipped at both far borders), flipped, word stores (16 % 4 == 0)
    ("down2_corner_br_flip", (24, 48), (12, 24), (8, 4, 16, 8), True, None, 1, "uint8"),
    # ~x0.51 on odd sizes, the window in the top-left corner = the whole image, four frames, byte stores (27 % 4)
    ("down_odd_full_f4", (37, 53), (19, 27), (0, 0, 27, 19), False, None, 4, "uint8"),
    # ~x1.24 on odd sizes, an inner window two tiles high (20 > 16), word stores, flipped, a uint16 label file (int32 on the device)
    ("up_odd_two_rows_flip", (33, 47), (41, 58), (5, 7, 40, 20), True, None, 1, "uint16"),
    # the height unchanged (an identity pass), the width x0.625
    ("axis_unchanged", (16, 32), (16, 20), (0, 0, 20, 16), False, None, 1, "uint8"),
    # no resize at all (ResizeShortestEdge drew the source's own size), a window at the top and bottom border
    ("identity_window", (16, 32), (16, 32), (4, 0, 24, 16), False, None, 4, "uint8"),
    # x2, a window that straddles a tile edge on both axes (70 = 64 + 6, 23 = 16 + 7) at odd offsets, flipped, byte stores (70 % 4)
    ("up2_straddle_flip", (30, 61), (60, 122), (29, 9, 70, 23), True, None, 1, "uint8"),
    # the pad grows the output (SIZE_DIVISIBILITY = 32 > crop): padding inside a tile and a tile row that is padding only
    ("pad_grows_flip", (24, 48), (12, 24), (2, 1, 20, 10), True, (32, 32), 1, "uint8"),
    # the pad crops (SIZE_DIVISIBILITY = 32 < crop): F.pad with negative amounts; flipped first, so the window's right part survives
    ("pad_crops_flip", (30, 61), (60, 122), (10, 5, 100, 50), True, (32, 32), 1, "uint8"),
    # the pad grows the height and crops the width
    ("pad_mixed", (24, 48), (12, 24), (0, 0, 24, 12), False, (40, 20), 4, "uint8"),
    # x1.5, the window at the right and bottom border, no label file
    ("up15_border_nolabel", (24, 48), (36, 72), (2, 3, 70, 33), False, None, 1, None),
    # x0.5 on the widest source: the source rectangle of a tile is at its widest (61 columns for 31 outputs)
    ("down2_wide", (30, 61), (15, 31), (0, 0, 31, 15), True, None, 4, "uint8"),
]

GEOMETRY_IDS = [g[0] for g in GEOMETRY]


def _colour_cases():
    from uenc.train_data import ColourParams
    out = []
    # every on / off combination of the four stages in both orders, the hue at -18, 0 and 18 when it is on
    betas, alphas_c, alphas_s = (-32.0, 31.625, 17.3), (0.5, 1.5, 1.2345678), (1.5, 0.5, 0.777)
    k = 0
    for bright, contrast, sat, hue, order in itertools.product((False, True), (False, True), (False, True), (None, -18, 0, 18), (True, False)):
        out.append((f"b{int(bright)}c{int(contrast)}s{int(sat)}h{hue}o{int(order)}",
                    ColourParams(betas[k % 3] if bright else None, order, alphas_c[k % 3] if contrast else None,
                                 alphas_s[(k + 1) % 3] if sat else None, hue, True)))
        k += 1
    # beyond what the augmentation draws: tables that saturate everywhere, a zero scale, BGR frames
    out.append(("extreme_hi", ColourParams(255.0, True, 3.0, 4.0, 17, True)))
    out.append(("extreme_lo", ColourParams(-255.0, False, 0.0, 0.0, -17, True)))
    out.append(("bgr_all", ColourParams(-7.5, True, 1.3, 0.6, 9, False)))
    out.append(("bgr_after", ColourParams(12.25, False, 0.8, 1.4, -5, False)))
    return out


COLOUR = _colour_cases()
COLOUR_IDS = [c[0] for c in COLOUR]


def colour_pixels() -> np.ndarray:
    """(24, 96, 3) uint8: the 256 greys (s = 0), the primaries and secondaries, ties of the maximum (r == g, r == b, g == b, with the
    third channel below), near-greys with diff = 1, and random triples."""
    rng = np.random.RandomState(7)
    px = rng.randint(0, 256, (24 * 96, 3)).astype(np.uint8)
    g = np.arange(256, dtype=np.uint8)
    px[:256] = g[:, None]
    px[256:262] = [[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]]
    n = 262
    for hi in (255, 200, 128, 17, 1):
        for lo in (0, hi // 2, max(hi - 1, 0)):
            for tie in ((hi, hi, lo), (hi, lo, hi), (lo, hi, hi)):
                px[n] = tie
                n += 1
    return px.reshape(24, 96, 3)


def make_plan(case, colour=None):
    from uenc.train_data import AugPlan
    _, src, rs, crop, flip, out, _, _ = case
    return AugPlan(src, rs, crop, flip, out if out is not None else (crop[3], crop[2]), colour, 128, 255, 0)


@functools.lru_cache(maxsize=None)
def make_inputs(case_id: str):
    """-> (frames list of (h, w, 3) uint8, panoptic PNG (h, w, 3) uint8, label (h, w) or None), deterministic per case."""
    case = GEOMETRY[GEOMETRY_IDS.index(case_id)]
    (h, w), F, label_dtype = case[1], case[6], case[7]
    rng = np.random.RandomState(100 + GEOMETRY_IDS.index(case_id))
    frames = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(F)]
    # piecewise-constant ids with all three bytes in use, as a panoptic PNG has them
    blocks = rng.randint(0, 1 << 24, ((h + 4) // 5, (w + 6) // 7))
    ids = np.kron(blocks, np.ones((5, 7), dtype=np.int64))[:h, :w]
    pan = np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], axis=-1).astype(np.uint8)
    label = None
    if label_dtype is not None:
        label = rng.randint(0, 20, (h, w)).astype(label_dtype)
        label[rng.rand(h, w) < 0.1] = 255
        if label_dtype == "uint16":
            label[0, 0] = 40000
    for a in frames + [pan] + ([label] if label is not None else []):
        a.setflags(write=False)
    return frames, pan, label


def case_colour(i: int):
    """The colour parameters a geometry case runs with: the cases cycle through the colour list, every third runs without colour."""
    return None if i % 3 == 2 else COLOUR[(i * 11) % len(COLOUR)][1]


@functools.lru_cache(maxsize=None)
def host_reference(case_id: str):
    """The host path's result for a geometry case, computed once and shared."""
    from uenc.train_data import apply_plan_host
    i = GEOMETRY_IDS.index(case_id)
    frames, pan, label = make_inputs(case_id)
    out = apply_plan_host(make_plan(GEOMETRY[i], case_colour(i)), frames, pan, label)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out
