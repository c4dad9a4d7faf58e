"""Training-time input pipeline: dataset dicts -> the dicts OneFormer's training forward takes, and the training loader.

Counterpart of the reference's model/data/dataset_mappers/oneformer_unified_dataset_mapper.py (`OneFormerUnifiedDatasetMapper`),
oneformer_multi_pass_cityscapes_mapper.py (`OneFormerUnifiedMultiPassCityscapesMapper`) and custom_augs.py:11-137
(`CustomColorAugSSDAugment` / `CustomColorAugSSDTransform`), which `INPUT.DATASET_MAPPER_NAME` = "oneformer_unified" /
"oneformer_unified_multi_pass" name.  The Detectron2 / fvcore pieces they rest on are [not in reference] and are restated here in the
slice the two mappers use: ResizeShortestEdge ("choice" / "range"), RandomCrop ("absolute"), RandomCrop_CategoryAreaConstraint,
RandomFlip (horizontal), ResizeTransform (PIL BILINEAR for uint8 images, PIL NEAREST for the uint8 panoptic PNG, torch "nearest" for the
label map the mapper casts to double), CropTransform, HFlipTransform, TrainingSampler, build_detection_train_loader.

Split in two:

  the plan     every random draw and every size decision of one sample, made on the host before any pixel is touched (`TrainAugmentation.plan`
               -> `AugPlan`).  The generators (a numpy RandomState-like and a random.Random-like, default the two global modules as in the
               reference) are consumed exactly as the reference's loops consume them, whichever pixel path runs afterwards.
  the pixels   `apply_plan_host` (PIL + numpy, the reference's method: resize everything, crop, colour, flip, pad) or `apply_plans`
               (csrc/augment.hip: only the crop window is computed, on the device, bit-equal to the host path).

The 8-bit HSV conversions of the colour augmentation are OpenCV's (`cv2.COLOR_BGR2HSV` / `COLOR_HSV2BGR`); cv2 is not a dependency, they
are restated in `bgr2hsv` / `hsv2bgr` (parity with cv2 itself is not pinned).
"""
import copy
import functools
import itertools
import json
import logging
import math
import random as _py_random
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.utils.data as torchdata

from .data import (MetadataCatalog, ResizeShortestEdge, _MapDataset, check_image_size, get_detection_dataset_dicts, read_image,
                   read_sequence_image, rgb2id, trivial_batch_collator)

logger = logging.getLogger(__name__)

__all__ = ["AugPlan", "ColourParams", "TrainAugmentation", "OneFormerUnifiedDatasetMapper", "OneFormerUnifiedMultiPassCityscapesMapper",
           "OneFormerMultiPassCityscapesMapper", "TrainingSampler", "build_detection_train_loader", "build_train_mapper", "apply_plans",
           "apply_plan_host", "apply_plan_device", "apply_packed", "pack_plan", "pil_bilinear_coeffs", "resize_window", "pil_nearest_table",
           "torch_nearest_table", "ssd_colour", "colour_tables", "bgr2hsv", "hsv2bgr", "draw_ssd_colour"]

PRECISION_BITS = 22                      # PIL's 8-bit resample: 32 - 8 - 2


# ---------------------------------------------------------------------------------------------------------------------
# resize rules
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def pil_bilinear_coeffs(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """PIL's `precompute_coeffs` + `normalize_coeffs_8bpc` for the BILINEAR filter (support 1.0) along one axis [not in reference]:
    -> first (out,) int32 = the first source index of every output index, count (out,) int32 = its taps, coeff (out, ksize) int32 =
    the 22-bit fixed-point weights (0 beyond count).  A pass is clip(((1 << 21) + sum(pixel * coeff)) >> 22, 0, 255)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    first, count, coeff = np.zeros(out_size, np.int32), np.zeros(out_size, np.int32), np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        first[xx], count[xx] = xmin, xmax
        coeff[xx, :xmax] = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
    for a in (first, count, coeff):
        a.setflags(write=False)
    return first, count, coeff


def _pass(a: np.ndarray, first, count, coeff, axis: int) -> np.ndarray:
    """One separable pass over `axis` (0 or 1) of an (h, w, c) integer array for the given output records."""
    n_in = a.shape[axis]
    acc = np.full((len(first), a.shape[1], a.shape[2]) if axis == 0 else (a.shape[0], len(first), a.shape[2]), 1 << (PRECISION_BITS - 1), np.int64)
    for t in range(coeff.shape[1]):
        idx = np.minimum(first.astype(np.int64) + t, n_in - 1)              # a tap beyond `count` has coefficient 0
        k = np.where(t < count, coeff[:, t], 0).astype(np.int64)
        acc += (a[idx] * k[:, None, None]) if axis == 0 else (a[:, idx] * k[None, :, None])
    return np.clip(acc >> PRECISION_BITS, 0, 255)


def resize_window(img: np.ndarray, new_hw: Tuple[int, int], window: Optional[Tuple[int, int, int, int]] = None) -> np.ndarray:
    """`PIL.Image.fromarray(img).resize((new_w, new_h), BILINEAR)[y0:y0 + ch, x0:x0 + cw]` computed for the window (x0, y0, cw, ch)
    only: the horizontal pass into a uint8 intermediate over the source rows the window's rows touch, then the vertical pass.  Every
    output pixel depends on its own coefficient rows alone, so this equals resize-then-crop bit for bit."""
    assert img.dtype == np.uint8 and img.ndim == 3
    h, w = img.shape[:2]
    new_h, new_w = new_hw
    x0, y0, cw, ch = (0, 0, new_w, new_h) if window is None else window
    cf, cc, ck = (a[x0:x0 + cw] for a in pil_bilinear_coeffs(w, new_w))
    rf, rc, rk = (a[y0:y0 + ch] for a in pil_bilinear_coeffs(h, new_h))
    sy0, sy1 = int(rf.min()), int((rf + rc).max())
    mid = _pass(img[sy0:sy1].astype(np.int64), cf, cc, ck, 1)
    return _pass(mid, rf - sy0, rc, rk, 0).astype(np.uint8)


@functools.lru_cache(maxsize=64)
def pil_nearest_table(in_size: int, out_size: int) -> np.ndarray:
    """Source index of every output index of `PIL.Image.resize(NEAREST)` along one axis.  PIL walks the axis by repeated addition of
    the scale in floating point, which is not floor((i + 0.5) * scale) in general: the table is taken from PIL itself, by resizing an
    int32 index ramp."""
    from PIL import Image
    ramp = Image.fromarray(np.arange(in_size, dtype=np.int32).reshape(1, in_size))
    out = np.asarray(ramp.resize((out_size, 1), Image.NEAREST)).reshape(-1).astype(np.int32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=64)
def torch_nearest_table(in_size: int, out_size: int) -> np.ndarray:
    """Source index of every output index of `F.interpolate(mode="nearest")` along one axis: min(floor(i * scale), in - 1) with the scale
    and the product in float32 (ATen's nearest_neighbor_compute_source_index)."""
    scale = np.float32(in_size) / np.float32(out_size)
    out = np.minimum(np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64), in_size - 1).astype(np.int32)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the SSD colour augmentation (custom_augs.py:11-137)
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ColourParams:
    """The draws of CustomColorAugSSDAugment.__call__ (custom_augs.py:55-63); None = the stage is off."""
    beta_brightness: Optional[float] = None
    con_sat_hue_order: bool = True
    alpha_contrast: Optional[float] = None
    alpha_saturation: Optional[float] = None
    hue: Optional[int] = None
    is_rgb: bool = True


def draw_ssd_colour(py_rng, img_format: str = "RGB", brightness_delta=32, contrast_low=0.5, contrast_high=1.5, saturation_low=0.5,
                    saturation_high=1.5, hue_delta=18) -> ColourParams:
    """custom_augs.py:55-63, in its order of draws from Python's `random`."""
    assert img_format in ("BGR", "RGB")
    beta = py_rng.uniform(-brightness_delta, brightness_delta) if py_rng.randrange(2) else None
    order = True if py_rng.randrange(2) else False
    contrast = py_rng.uniform(contrast_low, contrast_high) if py_rng.randrange(2) else None
    saturation = py_rng.uniform(saturation_low, saturation_high) if py_rng.randrange(2) else None
    hue = py_rng.randint(-hue_delta, hue_delta)
    return ColourParams(beta, order, contrast, saturation, hue, img_format == "RGB")


def _convert(img: np.ndarray, alpha=1, beta=0) -> np.ndarray:
    """custom_augs.py:134-137."""
    img = img.astype(np.float32) * alpha + beta
    img = np.clip(img, 0, 255)
    return img.astype(np.uint8)


@functools.lru_cache(maxsize=1)
def _hsv_div_tables() -> Tuple[np.ndarray, np.ndarray]:
    """OpenCV's RGB2HSV_b tables: sdiv[i] = round((255 << 12) / i), hdiv[i] = round((180 << 12) / (6 i)), half to even, [0] = 0."""
    i = np.arange(1, 256, dtype=np.float64)
    sdiv, hdiv = np.zeros(256, np.int32), np.zeros(256, np.int32)
    sdiv[1:] = np.rint((255 << 12) / i)
    hdiv[1:] = np.rint((180 << 12) / (6.0 * i))
    return sdiv, hdiv


def bgr2hsv(bgr: np.ndarray) -> np.ndarray:
    """cv2.cvtColor(bgr, COLOR_BGR2HSV) on uint8 (..., 3), restated: integers only, H in [0, 180)."""
    sdiv, hdiv = _hsv_div_tables()
    b, g, r = (bgr[..., i].astype(np.int32) for i in range(3))
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    s = (diff * sdiv[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + (1 << 11)) >> 12
    h = np.where(h < 0, h + 180, h)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


_SECTORS = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])       # (b, g, r) of every sector


def hsv2bgr(hsv: np.ndarray) -> np.ndarray:
    """cv2.cvtColor(hsv, COLOR_HSV2BGR) on uint8 (..., 3), restated: float32, every operation rounded once (the device path repeats
    these operations one by one, without fused multiply-adds), the result rounded half to even and saturated."""
    f32 = np.float32
    h, s, v = (hsv[..., i].astype(f32) for i in range(3))
    s = s * (f32(1.0) / f32(255.0))
    v = v * (f32(1.0) / f32(255.0))
    h = h * (f32(6.0) / f32(180.0))
    h = np.where(h >= f32(6.0), h - f32(6.0), h)
    sector = np.floor(h).astype(np.int64)
    frac = h - sector.astype(f32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    frac = np.where(bad, f32(0.0), frac).astype(f32)
    one = f32(1.0)
    tab = np.stack([v, v * (one - s), v * (one - s * frac), v * (one - s * (one - frac))], axis=-1)
    out = np.take_along_axis(tab, _SECTORS[sector], axis=-1)
    out = np.where((hsv[..., 1] == 0)[..., None], v[..., None], out).astype(f32)
    return np.clip(np.rint(out * f32(255.0)), 0, 255).astype(np.uint8)


def ssd_colour(img: np.ndarray, p: Optional[ColourParams]) -> np.ndarray:
    """CustomColorAugSSDTransform.apply_image (custom_augs.py:105-132) on an (h, w, 3) uint8 image."""
    if p is None:
        return img
    if p.is_rgb:
        img = img[:, :, [2, 1, 0]]
    if p.beta_brightness is not None:
        img = _convert(img, beta=p.beta_brightness)
    if p.con_sat_hue_order and p.alpha_contrast is not None:
        img = _convert(img, alpha=p.alpha_contrast)
    if p.alpha_saturation is not None:
        img = bgr2hsv(img)
        img[:, :, 1] = _convert(img[:, :, 1], alpha=p.alpha_saturation)
        img = hsv2bgr(img)
    if p.hue is not None:
        img = bgr2hsv(img)
        img[:, :, 0] = (img[:, :, 0].astype(int) + p.hue) % 180
        img = hsv2bgr(img)
    if not p.con_sat_hue_order and p.alpha_contrast is not None:
        img = _convert(img, alpha=p.alpha_contrast)
    if p.is_rgb:
        img = img[:, :, [2, 1, 0]]
    return img


COLOUR_SAT, COLOUR_HUE, COLOUR_CONTRAST_FIRST, COLOUR_RGB = 1, 2, 4, 8       # UENC_AUG_COLOUR_*


def colour_tables(p: ColourParams) -> Tuple[np.ndarray, int, int]:
    """The device's view of the colour parameters -> (table (704,) int32, flags, hue).  Brightness, contrast and the saturation scaling
    are maps of one uint8 value: each becomes a 256-entry table made with the reference's own numpy expression (`_convert`), the
    identity when the stage is off; then OpenCV's two reciprocal tables."""
    ramp = np.arange(256, dtype=np.uint8)
    lut = np.stack([ramp if p.beta_brightness is None else _convert(ramp, beta=p.beta_brightness),
                    ramp if p.alpha_contrast is None else _convert(ramp, alpha=p.alpha_contrast),
                    ramp if p.alpha_saturation is None else _convert(ramp, alpha=p.alpha_saturation)])
    sdiv, hdiv = _hsv_div_tables()
    flags = ((COLOUR_SAT if p.alpha_saturation is not None else 0) | (COLOUR_HUE if p.hue is not None else 0) |
             (COLOUR_CONTRAST_FIRST if p.con_sat_hue_order else 0) | (COLOUR_RGB if p.is_rgb else 0))
    return np.concatenate([np.ascontiguousarray(lut).view(np.int32).reshape(-1), sdiv, hdiv]), flags, int(p.hue or 0)


# ---------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class AugPlan:
    """Everything the pixel paths need to know about one sample; no pixel has been touched when it exists."""
    src_hw: Tuple[int, int]
    resized_hw: Tuple[int, int]
    crop: Tuple[int, int, int, int]             # (x0, y0, cw, ch) in the resized image
    flip: bool
    out_hw: Tuple[int, int]                     # after the pad (which crops when the target is smaller)
    colour: Optional[ColourParams] = None
    pad_image: int = 128
    pad_label: int = 255
    pad_pan: int = 0


class TrainAugmentation:
    """The augmentation list of one mapper as a planner.  Order, as in the reference's lists: ResizeShortestEdge,
    RandomCrop_CategoryAreaConstraint, CustomColorAugSSDAugment, RandomFlip; then the mapper's pad."""

    def __init__(self, min_sizes, max_size: int, sample_style: str = "choice", *, crop_enabled: bool = False, crop_type: str = "absolute",
                 crop_size=(512, 1024), single_category_max_area: float = 1.0, ignored_category: Optional[int] = 255,
                 colour_ssd: bool = False, image_format: str = "RGB", flip: bool = False, size_divisibility: int = -1,
                 ignore_label: int = 255, crop_key: str = "INPUT.CROP.TYPE"):
        if isinstance(min_sizes, int):
            min_sizes = (min_sizes, min_sizes)
        assert sample_style in ("range", "choice"), sample_style
        if sample_style == "range":
            assert len(min_sizes) == 2, "short_edge_length must be two values using 'range' sample style."
        if crop_enabled and crop_type != "absolute":
            raise NotImplementedError(f"{crop_key} = {crop_type!r}: only \"absolute\" crops are implemented (the shipped configurations use no other)")
        self.min_sizes, self.max_size, self.sample_style = tuple(min_sizes), max_size, sample_style
        self.crop_enabled, self.crop_size = crop_enabled, tuple(int(c) for c in crop_size)
        self.single_category_max_area, self.ignored_category = single_category_max_area, ignored_category
        self.colour_ssd, self.image_format, self.flip = colour_ssd, image_format, flip
        self.size_divisibility, self.ignore_label = size_divisibility, ignore_label

    def __repr__(self):
        return (f"TrainAugmentation(resize={self.min_sizes}/{self.max_size}/{self.sample_style}, crop={self.crop_size if self.crop_enabled else None}"
                f"/{self.single_category_max_area}, colour_ssd={self.colour_ssd}, flip={self.flip}, size_divisibility={self.size_divisibility})")

    def _accept(self, label, rows, cols, x0, y0, cw, ch) -> bool:
        """RandomCrop_CategoryAreaConstraint's test on the window of the RESIZED label map, which is never materialised: the nearest
        resize is a row table and a column table, so the window is the source label map indexed through their slices."""
        win = label[rows[y0:y0 + ch]][:, cols[x0:x0 + cw]]
        cnt = np.bincount(win.reshape(-1))
        if self.ignored_category is not None and 0 <= self.ignored_category < len(cnt):
            cnt[self.ignored_category] = 0
        cnt = cnt[cnt > 0]
        return len(cnt) > 1 and np.max(cnt) < np.sum(cnt) * self.single_category_max_area

    def plan(self, h: int, w: int, label: Optional[np.ndarray] = None, np_rng=None, py_rng=None) -> AugPlan:
        np_rng = np.random if np_rng is None else np_rng
        py_rng = _py_random if py_rng is None else py_rng
        # ResizeShortestEdge.get_transform
        if self.sample_style == "range":
            size = int(np_rng.randint(self.min_sizes[0], self.min_sizes[1] + 1))
        else:
            size = int(np_rng.choice(self.min_sizes))
        new_h, new_w = (h, w) if size == 0 else ResizeShortestEdge.get_output_shape(h, w, size, self.max_size)
        # RandomCrop_CategoryAreaConstraint.get_transform
        x0, y0, cw, ch = 0, 0, new_w, new_h
        if self.crop_enabled:
            ch, cw = min(self.crop_size[0], new_h), min(self.crop_size[1], new_w)
            if self.single_category_max_area >= 1.0:
                y0 = int(np_rng.randint(new_h - ch + 1))
                x0 = int(np_rng.randint(new_w - cw + 1))
            else:
                if label is None:
                    raise ValueError("a crop with SINGLE_CATEGORY_MAX_AREA < 1.0 needs the label map (\"sem_seg_file_name\")")
                lab = _label_ints(label)
                rows, cols = torch_nearest_table(h, new_h), torch_nearest_table(w, new_w)
                for _ in range(10):
                    y0 = int(np_rng.randint(new_h - ch + 1))
                    x0 = int(np_rng.randint(new_w - cw + 1))
                    if self._accept(lab, rows, cols, x0, y0, cw, ch):
                        break
        colour = draw_ssd_colour(py_rng, self.image_format) if self.colour_ssd else None
        flip = bool(np_rng.uniform(0, 1.0) < 0.5) if self.flip else False
        out_hw = (self.size_divisibility, self.size_divisibility) if self.size_divisibility > 0 else (ch, cw)
        return AugPlan((h, w), (new_h, new_w), (x0, y0, cw, ch), flip, out_hw, colour, 128, self.ignore_label, 0)


def _label_ints(label: np.ndarray) -> np.ndarray:
    if label.ndim != 2 or label.dtype.kind not in "ui":
        raise ValueError(f"the label map must be an (h, w) integer image, got {label.dtype} {label.shape}")
    return label


def _pad2d(a: np.ndarray, out_hw, value) -> np.ndarray:
    """F.pad(a, [0, W - w, 0, H - h], value=value) on the last two axes: a negative amount crops."""
    H, W = out_hw
    h, w = a.shape[-2:]
    out = np.full(a.shape[:-2] + (H, W), value, dtype=a.dtype)
    out[..., :min(h, H), :min(w, W)] = a[..., :min(h, H), :min(w, W)]
    return out


def apply_plan_host(plan: AugPlan, frames: Sequence[np.ndarray], pan: Optional[np.ndarray] = None, label: Optional[np.ndarray] = None):
    """The reference's method with PIL and numpy: resize every full frame, crop, colour, flip, pad.
    -> (images (F, 3, H, W) uint8, pan id map (H, W) int32 or None, label map (H, W) int32 or None) as numpy arrays."""
    from PIL import Image
    (h, w), (new_h, new_w), (x0, y0, cw, ch) = plan.src_hw, plan.resized_hw, plan.crop
    out = []
    for img in frames:
        assert img.dtype == np.uint8 and img.shape == (h, w, 3), (img.dtype, img.shape)
        img = np.asarray(Image.fromarray(np.ascontiguousarray(img)).resize((new_w, new_h), Image.BILINEAR))
        img = ssd_colour(img[y0:y0 + ch, x0:x0 + cw], plan.colour)
        if plan.flip:
            img = img[:, ::-1]
        out.append(_pad2d(img.transpose(2, 0, 1), plan.out_hw, plan.pad_image))
    ids = lab = None
    if pan is not None:
        assert pan.dtype == np.uint8 and pan.shape == (h, w, 3), (pan.dtype, pan.shape)
        rows, cols = pil_nearest_table(h, new_h)[y0:y0 + ch], pil_nearest_table(w, new_w)[x0:x0 + cw]
        ids = rgb2id(pan[rows][:, cols])
        ids = _pad2d(ids[:, ::-1] if plan.flip else ids, plan.out_hw, plan.pad_pan)
    if label is not None:
        rows, cols = torch_nearest_table(h, new_h)[y0:y0 + ch], torch_nearest_table(w, new_w)[x0:x0 + cw]
        lab = _label_ints(label)[rows][:, cols].astype(np.int32)
        lab = _pad2d(lab[:, ::-1] if plan.flip else lab, plan.out_hw, plan.pad_label)
    return np.stack(out), ids, lab


# ---------------------------------------------------------------------------------------------------------------------
# the device path
# ---------------------------------------------------------------------------------------------------------------------
def _axis_records(in_size: int, out_size: int, lo: int, n: int) -> Tuple[np.ndarray, int]:
    first, count, coeff = pil_bilinear_coeffs(in_size, out_size)
    return np.concatenate([first[lo:lo + n], count[lo:lo + n], coeff[lo:lo + n].reshape(-1)]), coeff.shape[1]


def pack_plan(plan: AugPlan, frames: Sequence[np.ndarray], pan: Optional[np.ndarray], label: Optional[np.ndarray]):
    """One sample's upload: a single uint8 buffer holding the int32 tables first (coefficient records of the window's columns and rows,
    colour tables, the four nearest index tables), then the frames, the panoptic PNG and the label map, each at a 16-byte boundary.
    -> (buffer, offsets: name -> byte offset, meta)."""
    (h, w), (new_h, new_w), (x0, y0, cw, ch) = plan.src_hw, plan.resized_hw, plan.crop
    col, kx = _axis_records(w, new_w, x0, cw)
    row, ky = _axis_records(h, new_h, y0, ch)
    parts: List[Tuple[str, np.ndarray]] = [("col_tab", col), ("row_tab", row)]
    flags = hue = 0
    if plan.colour is not None:
        tab, flags, hue = colour_tables(plan.colour)
        parts.append(("colour_tab", tab))
    if pan is not None:
        parts += [("pan_col", pil_nearest_table(w, new_w)[x0:x0 + cw]), ("pan_row", pil_nearest_table(h, new_h)[y0:y0 + ch])]
    label_bytes = 0
    if label is not None:
        label = _label_ints(label)
        label = label if label.dtype == np.uint8 else label.astype(np.int32)
        label_bytes = label.dtype.itemsize
        parts += [("lab_col", torch_nearest_table(w, new_w)[x0:x0 + cw]), ("lab_row", torch_nearest_table(h, new_h)[y0:y0 + ch])]
    parts = [(k, np.ascontiguousarray(v, dtype=np.int32)) for k, v in parts]
    for i, img in enumerate(frames):
        assert img.dtype == np.uint8 and img.shape == (h, w, 3), (img.dtype, img.shape)
        parts.append((f"frame{i}", img))
    if pan is not None:
        assert pan.dtype == np.uint8 and pan.shape == (h, w, 3), (pan.dtype, pan.shape)
        parts.append(("pan", pan))
    if label is not None:
        parts.append(("label", label))
    offsets, total = {}, 0
    for k, v in parts:
        offsets[k] = total
        total += (v.nbytes + 15) // 16 * 16
    buf = torch.empty(total, dtype=torch.uint8)
    view = buf.numpy()
    for k, v in parts:
        view[offsets[k]:offsets[k] + v.nbytes] = np.ascontiguousarray(v).reshape(-1).view(np.uint8)
    meta = {"kx": kx, "ky": ky, "flags": flags, "hue": hue, "label_bytes": label_bytes, "F": len(frames),
            "frame_stride": (h * w * 3 + 15) // 16 * 16}
    return buf, offsets, meta


def apply_packed(plan: AugPlan, buf: torch.Tensor, off: dict, meta: dict, device):
    """One upload of a packed sample and at most two launches on the current stream, no synchronisation (the upload is an ordinary copy
    from pageable memory).  -> (images (F, 3, H, W) uint8, pan id map (H, W) int32 or None, label map (H, W) int32 or None) on `device`."""
    from . import kernels as K
    return K.augment_sample(buf.to(device, non_blocking=True), off, meta, plan)


def apply_plan_device(plan: AugPlan, frames: Sequence[np.ndarray], pan: Optional[np.ndarray], label: Optional[np.ndarray], device):
    """`pack_plan` + `apply_packed`: the device path on source arrays."""
    return apply_packed(plan, *pack_plan(plan, frames, pan, label), device)


def apply_plans(batch: List[dict], device="cuda") -> List[dict]:
    """Finish the dicts a mapper with augment="device" returned: every dict's "_augment" record (the plan + the packed upload buffer that
    holds the untouched source arrays) is replaced by the augmented tensors, on `device`: one upload and two launches per record.  Dicts
    without a record (sequence dicts, host-finished dicts) pass through."""
    out = []
    for d in batch:
        rec = d.pop("_augment", None) if isinstance(d, dict) else None
        if rec is not None:
            images, ids, lab = apply_packed(rec["plan"], rec["buf"], rec["off"], rec["meta"], device)
            _store(d, rec["keys"], images, ids, lab)
            _add_instances(d, rec.get("instances"))
        out.append(d)
    return out


def _store(d: dict, keys: Sequence[str], images, ids, lab):
    for i, k in enumerate(keys):
        d[k] = images[i]
    if ids is not None:
        d["pan_seg"] = ids
    if lab is not None:
        d["sem_seg_gt"] = lab


def _add_instances(d: dict, spec: Optional[dict]):
    """with_instances=True: the reference's "instances" / "text" / "sem_seg" from the finished id map, through the rules of
    uenc.modeling.targets (`_get_semantic_dict` / `_get_instance_dict` / `_get_panoptic_dict`).  On a device id map this synchronises once."""
    if spec is None:
        return
    from .d2 import Instances
    from .modeling.targets import build_targets
    targets, sem_seg, texts = build_targets([d["pan_seg"]], [d["segments_info"]], [d["task"]], thing_ids=d["thing_ids"],
                                            class_names=spec["class_names"], ignore_label=spec["ignore_label"], num_texts=spec["num_texts"])
    inst = Instances(tuple(d["orig_shape"]))
    inst.gt_classes = targets[0]["labels"]
    inst.gt_masks = targets[0]["masks"] != 0
    d["instances"], d["text"], d["sem_seg"] = inst, texts[0], sem_seg[0]


# ---------------------------------------------------------------------------------------------------------------------
# the mappers
# ---------------------------------------------------------------------------------------------------------------------
def _draw_task(np_rng, semantic_prob: float, instance_prob: float) -> str:
    prob_task = np_rng.uniform(0, 1.)
    if prob_task < semantic_prob:
        return "The task is semantic"
    if prob_task < instance_prob:
        return "The task is instance"
    return "The task is panoptic"


class _TrainMapper:
    """What the two mappers share: the generators, the pixel path and the keys of a finished segmentation dict."""

    def _init_common(self, is_train, meta, name, num_queries, image_format, ignore_label, size_divisibility, semantic_prob, instance_prob,
                     augment, with_instances, np_rng, py_rng):
        assert is_train, f"{type(self).__name__} should only be used for training!"
        if augment not in ("host", "device"):
            raise ValueError(f"augment must be \"host\" or \"device\", got {augment!r}")
        self.is_train, self.meta, self.name, self.num_queries = True, meta, name, num_queries
        self.img_format, self.ignore_label, self.size_divisibility = image_format, ignore_label, size_divisibility
        self.semantic_prob, self.instance_prob = semantic_prob, instance_prob
        self.augment, self.with_instances = augment, with_instances
        self.np_rng = np.random if np_rng is None else np_rng
        self.py_rng = _py_random if py_rng is None else py_rng
        self.things = list(meta.thing_dataset_id_to_contiguous_id.values()) if meta is not None and meta.get("thing_dataset_id_to_contiguous_id") else []
        self.class_names = list(meta.get("stuff_classes") or []) if meta is not None else []

    def _finish_segmentation(self, d: dict, aug: "TrainAugmentation", frames: Dict[str, np.ndarray], pan: np.ndarray, label, segments_info):
        if "annotations" in d:
            raise ValueError("Pemantic segmentation dataset should not have 'annotations'.")
        h, w = next(iter(frames.values())).shape[:2]
        plan = aug.plan(h, w, label, self.np_rng, self.py_rng)
        d["task"] = _draw_task(self.np_rng, self.semantic_prob, self.instance_prob)
        d["segments_info"] = segments_info
        d["orig_shape"] = tuple(plan.out_hw)
        d["thing_ids"] = self.things
        spec = None
        if self.with_instances:
            spec = {"class_names": self.class_names, "ignore_label": self.ignore_label, "num_texts": self.num_queries}
        if self.augment == "device":
            # packed here, in the worker: the buffer is ONE torch tensor, which a DataLoader passes through shared memory (numpy arrays
            # in a dict would be pickled), and the main process is left with the upload and the launches
            buf, off, meta = pack_plan(plan, list(frames.values()), pan, label)
            d["_augment"] = {"plan": plan, "buf": buf, "off": off, "meta": meta, "keys": list(frames), "instances": spec}
            return d
        images, ids, lab = apply_plan_host(plan, list(frames.values()), pan, label)
        _store(d, list(frames), torch.from_numpy(images), torch.from_numpy(ids), None if lab is None else torch.from_numpy(lab))
        _add_instances(d, spec)
        return d


def _meta_of(cfg):
    names = cfg.DATASETS.TRAIN
    meta = MetadataCatalog.get(names[0])
    return names[0], meta, meta.get("ignore_label", 255)


def _refuse_depth_jitter(cfg):
    if getattr(cfg.INPUT, "DEPTH_COLOR_JITTER", False):
        raise NotImplementedError("INPUT.DEPTH_COLOR_JITTER True: the sequence frames' colour jitter is torchvision's tensor ColorJitter, "
                                  "which is not restated here")


class OneFormerUnifiedDatasetMapper(_TrainMapper):
    """oneformer_unified_dataset_mapper.py: the current frame, its right, previous and next frames under ONE plan (resize, constrained
    crop, SSD colour; no flip), the panoptic PNG and the optional label file, the task drawn by TASK_PROB, the file's camera constants.

    `OneFormerUnifiedDatasetMapper(cfg, True)` or keyword arguments.  augment="host" finishes the dict here; augment="device" returns
    the plan and the untouched source arrays, packed into one upload buffer, under "_augment" (no GPU API is touched: safe in DataLoader
    workers) for `apply_plans`."""

    FRAMES = (("left_image", "file_name"), ("right_image", "right_file_name"), ("left_prev_image", "left_prev_image_file"),
              ("left_next_image", "left_nxt_image_file"))

    def __init__(self, cfg=None, is_train: bool = True, *, name=None, num_queries=None, meta=None, augmentations: Optional[TrainAugmentation] = None,
                 image_format="RGB", ignore_label=255, size_divisibility=-1, semantic_prob=0.33, instance_prob=0.66, augment="host",
                 with_instances=False, np_rng=None, py_rng=None):
        if cfg is not None:                                    # from_config (:93-136)
            name, meta, ignore_label = _meta_of(cfg)
            I = cfg.INPUT
            image_format, size_divisibility = I.FORMAT, I.SIZE_DIVISIBILITY
            augmentations = TrainAugmentation(
                I.SEG_MIN_SIZE_TRAIN, I.SEG_MAX_SIZE_TRAIN, I.SEG_MIN_SIZE_TRAIN_SAMPLING, crop_enabled=I.CROP.ENABLED, crop_type=I.CROP.TYPE,
                crop_size=I.CROP.SIZE, single_category_max_area=I.CROP.SINGLE_CATEGORY_MAX_AREA,
                ignored_category=cfg.MODEL.SEM_SEG_HEAD.IGNORE_VALUE, colour_ssd=I.COLOR_AUG_SSD, image_format=I.FORMAT, flip=False,
                size_divisibility=size_divisibility, ignore_label=ignore_label, crop_key="INPUT.CROP.TYPE")
            num_queries = cfg.MODEL.ONE_FORMER.NUM_OBJECT_QUERIES - cfg.MODEL.TEXT_ENCODER.N_CTX
            semantic_prob, instance_prob = I.TASK_PROB.SEMANTIC, I.TASK_PROB.INSTANCE
        self._init_common(is_train, meta, name, num_queries, image_format, ignore_label, size_divisibility, semantic_prob, instance_prob,
                          augment, with_instances, np_rng, py_rng)
        self.tfm_gens = augmentations
        logger.info("[%s] Augmentations used in training: %s", type(self).__name__, augmentations)

    def __call__(self, dataset_dict: dict) -> dict:
        d = copy.deepcopy(dataset_dict)
        frames = {}
        for key, src in self.FRAMES:
            frames[key] = read_image(d[src], format=self.img_format)
        for img in frames.values():
            check_image_size(d, img)
        label = read_image(d.pop("left_sem_seg_file_name")) if "left_sem_seg_file_name" in d else None
        if "left_pan_seg_file_name" not in d:
            raise ValueError("Cannot find 'pan_seg_file_name' for panoptic segmentation dataset {}.".format(d.get("left_file_name", d["file_name"])))
        pan = read_image(d.pop("left_pan_seg_file_name"), "RGB")
        d = self._finish_segmentation(d, self.tfm_gens, frames, pan, label, d["left_segments_info"])
        if d.get("cam_info_file") is not None:
            with open(d["cam_info_file"], "r") as f:
                d["baseline"] = json.load(f).get("extrinsic", {}).get("baseline", 0.0)
        K = np.array([[2262.52 / 2048 * 512, 0, 0.5 * 512, 0], [0, 2265.30 / 1024 * 256, 0.5 * 256, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
        d["K"] = torch.from_numpy(K).float()
        d["inv_K"] = torch.from_numpy(np.linalg.pinv(K)).float()
        stereo_T = np.eye(4, dtype=np.float32)
        stereo_T[0, 3] = -0.1                                   # the list has no flip: its last transform never is one (:456)
        d["stereo_T"] = torch.from_numpy(stereo_T).float()
        return d


class OneFormerUnifiedMultiPassCityscapesMapper(_TrainMapper):
    """oneformer_multi_pass_cityscapes_mapper.py: "segmentation" dicts get resize, constrained crop, SSD colour and flip; "sequence"
    dicts three 192 x 512 frames with a shared flip, their `orig_*` copies, the pad, and K / inv_K from the camera file.  Sequence dicts
    are always finished on the host."""

    def __init__(self, cfg=None, is_train: bool = True, *, name=None, num_queries=None, meta=None,
                 seg_augmentations: Optional[TrainAugmentation] = None, image_format="RGB", ignore_label=255, size_divisibility=-1,
                 semantic_prob=0.33, instance_prob=0.66, augment="host", with_instances=False, np_rng=None, py_rng=None):
        if cfg is not None:                                    # from_config (:100-165)
            _refuse_depth_jitter(cfg)
            name, meta, ignore_label = _meta_of(cfg)
            I = cfg.INPUT
            image_format, size_divisibility = I.FORMAT, I.SIZE_DIVISIBILITY
            seg_augmentations = TrainAugmentation(
                I.SEG_MIN_SIZE_TRAIN, I.SEG_MAX_SIZE_TRAIN, I.SEG_MIN_SIZE_TRAIN_SAMPLING, crop_enabled=I.SEG_CROP.ENABLED,
                crop_type=I.SEG_CROP.TYPE, crop_size=I.SEG_CROP.SIZE, single_category_max_area=I.SEG_CROP.SINGLE_CATEGORY_MAX_AREA,
                ignored_category=cfg.MODEL.SEM_SEG_HEAD.IGNORE_VALUE, colour_ssd=I.SEG_COLOR_AUG_SSD, image_format=I.FORMAT, flip=True,
                size_divisibility=size_divisibility, ignore_label=ignore_label, crop_key="INPUT.SEG_CROP.TYPE")
            num_queries = cfg.MODEL.ONE_FORMER.NUM_OBJECT_QUERIES - cfg.MODEL.TEXT_ENCODER.N_CTX
            semantic_prob, instance_prob = I.TASK_PROB.SEMANTIC, I.TASK_PROB.INSTANCE
        self._init_common(is_train, meta, name, num_queries, image_format, ignore_label, size_divisibility, semantic_prob, instance_prob,
                          augment, with_instances, np_rng, py_rng)
        self.seg_tfm_gens = seg_augmentations
        logger.info("[%s] Augmentations used in training for segmentations: %s", type(self).__name__, seg_augmentations)
        logger.info("[%s] Augmentations used in training for depth: RandomFlip", type(self).__name__)

    def __call__(self, dataset_dict: dict) -> dict:
        d = copy.deepcopy(dataset_dict)
        if d.get("type") == "segmentation":
            return self.process_segmentation_data(d)
        if d.get("type") == "sequence":
            return self.process_sequence_data(d)
        raise ValueError("Unknown dataset type: {}".format(d.get("type")))

    def process_segmentation_data(self, d: dict) -> dict:
        # the reference passes dataset='cs' to detectron2's read_image here, a keyword that reader does not have: the plain reader is meant
        image = read_image(d["file_name"], format=self.img_format)
        check_image_size(d, image)
        label = read_image(d.pop("sem_seg_file_name")) if "sem_seg_file_name" in d else None
        if "pan_seg_file_name" not in d:
            raise ValueError("Cannot find 'pan_seg_file_name' for panoptic segmentation dataset {}.".format(d["file_name"]))
        pan = read_image(d.pop("pan_seg_file_name"), "RGB")
        return self._finish_segmentation(d, self.seg_tfm_gens, {"left_image": image}, pan, label, d["segments_info"])

    def process_sequence_data(self, d: dict) -> dict:
        keys = (("left_image", "file_name"), ("left_prev_image", "left_prev_image_file"), ("left_next_image", "left_nxt_image_file"))
        frames = {k: read_sequence_image(d[src], format=self.img_format, dataset="cs") for k, src in keys}
        for img in frames.values():
            check_image_size(d, img)
        flip = bool(self.np_rng.uniform(0, 1.0) < 0.5)                       # depth_resize_augmentations = [RandomFlip()]
        for k, img in frames.items():
            img = img[:, ::-1] if flip else img
            t = torch.as_tensor(np.ascontiguousarray(img.transpose(2, 0, 1)))
            if self.size_divisibility > 0:
                t = torch.from_numpy(_pad2d(t.numpy(), (self.size_divisibility, self.size_divisibility), 128))
            d[k] = t
            d["orig_" + k] = t.clone()                                       # no colour jitter runs between the copy and the frame
        with open(d["cam_info_file"], "r") as f:
            data = json.load(f)
        fx = data["intrinsic"]["fx"] / 2048.0 * 512.0
        fy = data["intrinsic"]["fy"] / 768.0 * 192.0
        u0 = data["intrinsic"]["u0"] / 2048.0 * 512.0
        v0 = data["intrinsic"]["v0"] / 768.0 * 192.0
        if flip:
            u0 = 512. - u0
        K = np.array([[fx, 0, u0, 0], [0, fy, v0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
        d["K"] = torch.from_numpy(K).float()
        d["inv_K"] = torch.from_numpy(np.linalg.pinv(K)).float()
        return d


OneFormerMultiPassCityscapesMapper = OneFormerUnifiedMultiPassCityscapesMapper

MAPPERS = {"oneformer_unified": OneFormerUnifiedDatasetMapper, "oneformer_unified_multi_pass": OneFormerUnifiedMultiPassCityscapesMapper}


def build_train_mapper(cfg, **kw):
    """The mapper `INPUT.DATASET_MAPPER_NAME` names."""
    name = cfg.INPUT.DATASET_MAPPER_NAME
    if name not in MAPPERS:
        raise NotImplementedError(f"INPUT.DATASET_MAPPER_NAME = {name!r}: known training mappers are {sorted(MAPPERS)}")
    return MAPPERS[name](cfg, True, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the training loader
# ---------------------------------------------------------------------------------------------------------------------
class TrainingSampler(torchdata.Sampler):
    """detectron2.data.samplers.TrainingSampler: an infinite stream of indices, a fresh seeded permutation per pass (or 0 .. size - 1
    unshuffled), dealt round-robin over the ranks: rank r takes entries r, r + world, ... of the one stream every rank computes."""

    def __init__(self, size: int, shuffle: bool = True, seed: int = 0, rank: Optional[int] = None, world_size: Optional[int] = None):
        import torch.distributed as dist
        if size <= 0:
            raise ValueError(f"TrainingSampler(size=) expected a positive value. Got {size}.")
        on = dist.is_available() and dist.is_initialized()
        self._size, self._shuffle, self._seed = size, shuffle, int(seed)
        self._rank = (dist.get_rank() if on else 0) if rank is None else rank
        self._world_size = (dist.get_world_size() if on else 1) if world_size is None else world_size

    def __iter__(self):
        yield from itertools.islice(self._infinite_indices(), self._rank, None, self._world_size)

    def _infinite_indices(self):
        g = torch.Generator()
        g.manual_seed(self._seed)
        while True:
            if self._shuffle:
                yield from torch.randperm(self._size, generator=g).tolist()
            else:
                yield from range(self._size)


def _worker_init_reset_seed(worker_id):
    seed = (torch.initial_seed() + worker_id) % 2 ** 31
    np.random.seed(seed)
    _py_random.seed(seed)


class _TrainLoader:
    """Iterable over lists of finished dicts; with augment="device" the plans are applied as the batches leave the DataLoader (in the
    main process: the workers never initialise the GPU)."""

    def __init__(self, loader, device):
        self.loader, self.device = loader, device

    def __iter__(self):
        for batch in self.loader:
            yield apply_plans(batch, self.device) if self.device is not None else batch


def build_detection_train_loader(dataset, *, mapper=None, total_batch_size: Optional[int] = None, augment: Optional[str] = None, sampler=None,
                                 num_workers: int = 0, seed: int = 0, device="cuda", world_size: Optional[int] = None):
    """detectron2.data.build_detection_train_loader in the slice the trainers use: `dataset` is a cfg (dataset dicts of DATASETS.TRAIN,
    the mapper INPUT.DATASET_MAPPER_NAME names, SOLVER.IMS_PER_BATCH, DATALOADER.NUM_WORKERS, SEED) or a list of dataset dicts with
    `mapper` and `total_batch_size` given.  Infinite seeded rank-sharded TrainingSampler, no collation: yields lists of finished dicts.
    augment: "host" | "device", default the mapper's own setting."""
    if hasattr(dataset, "DATALOADER"):
        cfg = dataset
        dataset = get_detection_dataset_dicts(cfg.DATASETS.TRAIN)
        if mapper is None:
            mapper = build_train_mapper(cfg, augment=augment or "host")
        total_batch_size = cfg.SOLVER.IMS_PER_BATCH if total_batch_size is None else total_batch_size
        num_workers = cfg.DATALOADER.NUM_WORKERS
        seed = cfg.SEED if getattr(cfg, "SEED", -1) >= 0 else seed
    if mapper is None or total_batch_size is None:
        raise ValueError("build_detection_train_loader: a list of dataset dicts needs mapper= and total_batch_size=")
    if augment is not None:
        if augment not in ("host", "device"):
            raise ValueError(f"augment must be \"host\" or \"device\", got {augment!r}")
        mapper.augment = augment
    if sampler is None:
        sampler = TrainingSampler(len(dataset), seed=seed, world_size=world_size)
    world = sampler._world_size if isinstance(sampler, TrainingSampler) else (world_size or 1)
    if total_batch_size <= 0 or total_batch_size % world:
        raise ValueError(f"Total batch size ({total_batch_size}) must be divisible by the number of gpus ({world}).")
    loader = torchdata.DataLoader(_MapDataset(dataset, mapper), batch_size=total_batch_size // world, sampler=sampler, drop_last=True,
                                  num_workers=num_workers, collate_fn=trivial_batch_collator, worker_init_fn=_worker_init_reset_seed)
    return _TrainLoader(loader, device if getattr(mapper, "augment", "host") == "device" else None)
