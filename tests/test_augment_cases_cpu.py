"""The host rules of the training-time augmentation (uenc/train_data.py) against the libraries that define them: PIL (BILINEAR and
NEAREST resize), torch (nearest interpolation of the label map), the reference's numpy expression (value tables) and plain Python loops
(the crop constraint, the integer HSV conversion).  No GPU.  Every comparison is equality."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

import augment_cases as AC
from uenc import train_data as T


@pytest.mark.parametrize("case", AC.GEOMETRY, ids=AC.GEOMETRY_IDS)
def test_window_resize_equals_pil_resize_then_crop(case):
    frames, _, _ = AC.make_inputs(case[0])
    (nh, nw), (x0, y0, cw, ch) = case[2], case[3]
    for img in frames:
        ref = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))[y0:y0 + ch, x0:x0 + cw]
        assert np.array_equal(T.resize_window(img, (nh, nw), (x0, y0, cw, ch)), ref)


@pytest.mark.parametrize("case", AC.GEOMETRY, ids=AC.GEOMETRY_IDS)
def test_nearest_tables_equal_pil_and_torch(case):
    _, pan, label = AC.make_inputs(case[0])
    (h, w), (nh, nw) = case[1], case[2]
    ref = np.asarray(Image.fromarray(pan).resize((nw, nh), Image.NEAREST))
    assert np.array_equal(pan[T.pil_nearest_table(h, nh)][:, T.pil_nearest_table(w, nw)], ref)
    lab = np.arange(h * w, dtype=np.float64).reshape(h, w) if label is None else label.astype("double")
    t = torch.from_numpy(lab).view(h, w, 1, 1).permute(2, 3, 0, 1)          # detectron2's ResizeTransform on a non-uint8 array
    ref = torch.nn.functional.interpolate(t, (nh, nw), mode="nearest", align_corners=None)[0, 0].numpy()
    assert np.array_equal(lab[T.torch_nearest_table(h, nh)][:, T.torch_nearest_table(w, nw)], ref)


def test_pil_nearest_is_not_the_half_pixel_floor():
    """The reason the table is taken from PIL: 24 -> 51 differs from floor((i + 0.5) * scale)."""
    assert not np.array_equal(T.pil_nearest_table(24, 51), np.floor((np.arange(51) + 0.5) * 24 / 51).astype(np.int32))


def _literal_crop(aug, label, new_hw, np_rng):
    """RandomCrop_CategoryAreaConstraint.get_transform on a MATERIALISED resized label map, ten tries."""
    h, w = label.shape
    t = torch.from_numpy(label.astype("double")).view(h, w, 1, 1).permute(2, 3, 0, 1)
    sem_seg = torch.nn.functional.interpolate(t, new_hw, mode="nearest")[0, 0].numpy()
    nh, nw = sem_seg.shape
    crop = (min(aug.crop_size[0], nh), min(aug.crop_size[1], nw))
    for _ in range(10):
        y0 = np_rng.randint(nh - crop[0] + 1)
        x0 = np_rng.randint(nw - crop[1] + 1)
        tmp = sem_seg[y0:y0 + crop[0], x0:x0 + crop[1]]
        labels, cnt = np.unique(tmp, return_counts=True)
        cnt = cnt[labels != aug.ignored_category]
        if len(cnt) > 1 and np.max(cnt) < np.sum(cnt) * aug.single_category_max_area:
            break
    return (x0, y0, crop[1], crop[0])


@pytest.mark.parametrize("max_area", [0.3, 0.55, 0.75, 0.999])
@pytest.mark.parametrize("src,sizes", [((24, 48), (12, 24, 48)), ((37, 53), (19, 40, 74)), ((33, 47), (33,))])
def test_crop_constraint_plan_equals_the_ten_try_loop(src, sizes, max_area):
    h, w = src
    rng = np.random.RandomState(h * w)
    label = np.kron(rng.randint(0, 4, ((h + 7) // 8, (w + 7) // 8)), np.ones((8, 8), dtype=np.int64))[:h, :w].astype(np.uint8)
    label[rng.rand(h, w) < 0.15] = 255
    aug = T.TrainAugmentation(sizes, 4096, "choice", crop_enabled=True, crop_size=(16, 24), single_category_max_area=max_area, ignored_category=255)
    for seed in range(12):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        plan = aug.plan(h, w, label, a, random.Random(seed))
        size = int(b.choice(sizes))
        new_hw = T.ResizeShortestEdge.get_output_shape(h, w, size, 4096)
        assert plan.resized_hw == new_hw
        assert plan.crop == _literal_crop(aug, label, new_hw, b)
        sa, sb = a.get_state(), b.get_state()                                # the loop stopped drawing at the same try
        assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


def test_plain_crop_range_style_flip_and_draw_order():
    aug = T.TrainAugmentation((20, 40), 4096, "range", crop_enabled=True, crop_size=(512, 30), colour_ssd=True, flip=True, size_divisibility=64)
    a, b, pa, pb = np.random.RandomState(5), np.random.RandomState(5), random.Random(5), random.Random(5)
    plan = aug.plan(24, 48, None, a, pa)
    size = b.randint(20, 41)
    nh, nw = T.ResizeShortestEdge.get_output_shape(24, 48, size, 4096)
    ch, cw = min(512, nh), min(30, nw)
    y0 = b.randint(nh - ch + 1)
    x0 = b.randint(nw - cw + 1)
    colour = T.draw_ssd_colour(pb, "RGB")
    flip = b.uniform() < 0.5
    assert (plan.resized_hw, plan.crop, plan.flip, plan.colour, plan.out_hw) == ((nh, nw), (x0, y0, cw, ch), flip, colour, (64, 64))
    assert a.uniform() == b.uniform() and pa.random() == pb.random()


def test_ssd_colour_draws_follow_the_reference_order():
    r, q = random.Random(11), random.Random(11)
    for _ in range(50):
        p = T.draw_ssd_colour(r)
        beta = q.uniform(-32, 32) if q.randrange(2) else None
        order = True if q.randrange(2) else False
        con = q.uniform(0.5, 1.5) if q.randrange(2) else None
        sat = q.uniform(0.5, 1.5) if q.randrange(2) else None
        hue = q.randint(-18, 18)
        assert p == T.ColourParams(beta, order, con, sat, hue, True)


@pytest.mark.parametrize("name,p", AC.COLOUR, ids=AC.COLOUR_IDS)
def test_value_tables_equal_the_reference_convert(name, p):
    tab, flags, hue = T.colour_tables(p)
    lut = tab[:192].view(np.uint8).reshape(3, 256)
    ramp = np.arange(256, dtype=np.uint8)

    def convert(img, alpha=1, beta=0):                                        # custom_augs.py:134-137
        img = img.astype(np.float32) * alpha + beta
        img = np.clip(img, 0, 255)
        return img.astype(np.uint8)

    assert np.array_equal(lut[0], convert(ramp, beta=p.beta_brightness) if p.beta_brightness is not None else ramp)
    assert np.array_equal(lut[1], convert(ramp, alpha=p.alpha_contrast) if p.alpha_contrast is not None else ramp)
    assert np.array_equal(lut[2], convert(ramp, alpha=p.alpha_saturation) if p.alpha_saturation is not None else ramp)
    assert flags == (p.alpha_saturation is not None) * 1 + (p.hue is not None) * 2 + p.con_sat_hue_order * 4 + p.is_rgb * 8
    assert hue == (p.hue or 0) and tab.shape == (704,) and tab.dtype == np.int32


def test_hsv_of_the_primaries():
    rgb = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]]], dtype=np.uint8)
    assert T.bgr2hsv(rgb[:, :, ::-1]).tolist() == [[[0, 255, 255], [60, 255, 255], [120, 255, 255]]]
    assert np.array_equal(T.hsv2bgr(T.bgr2hsv(rgb[:, :, ::-1]))[:, :, ::-1], rgb)


def test_greys_are_fixed_points_of_saturation_and_hue():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    assert np.array_equal(T.bgr2hsv(grey)[..., :2], np.zeros((1, 256, 2), np.uint8))
    for p in (T.ColourParams(None, True, None, 1.5, None), T.ColourParams(None, True, None, None, 18), T.ColourParams(None, False, None, 0.5, -18)):
        assert np.array_equal(T.ssd_colour(grey, p), grey)


def _round_half_even(x):
    return int(np.rint(x))


def test_integer_hsv_equals_a_per_pixel_loop():
    px = AC.colour_pixels().reshape(-1, 3)
    got = T.bgr2hsv(px.reshape(1, -1, 3))[0]
    sdiv = [0] + [_round_half_even((255 << 12) / i) for i in range(1, 256)]
    hdiv = [0] + [_round_half_even((180 << 12) / (6 * i)) for i in range(1, 256)]
    for (b, g, r), out in zip(px.tolist(), got.tolist()):
        v, diff = max(b, g, r), max(b, g, r) - min(b, g, r)
        s = (diff * sdiv[v] + 2048) >> 12
        h = (g - b) if v == r else ((b - r + 2 * diff) if v == g else (r - g + 4 * diff))
        h = (h * hdiv[diff] + 2048) >> 12
        if h < 0:
            h += 180
        assert [h, s, v] == out, ((b, g, r), [h, s, v], out)


def test_float_hsv_stage_equals_a_per_pixel_float32_loop():
    """hsv2bgr, the expression the device repeats operation by operation, against scalar numpy float32 arithmetic."""
    f = np.float32
    hsv = T.bgr2hsv(AC.colour_pixels().reshape(1, -1, 3))[0]
    hsv[:180, 0] = np.arange(180)                                             # every hue
    got = T.hsv2bgr(hsv.reshape(1, -1, 3))[0]
    sectors = [[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]]
    for (h, s, v), out in zip(hsv.tolist(), got.tolist()):
        sf, vf = f(s) * (f(1) / f(255)), f(v) * (f(1) / f(255))
        if s == 0:
            bgr = [vf] * 3
        else:
            hf = f(h) * (f(6) / f(180))
            sec = int(np.floor(hf))
            fr = hf - f(sec)
            tab = [vf, vf * (f(1) - sf), vf * (f(1) - sf * fr), vf * (f(1) - sf * (f(1) - fr))]
            bgr = [tab[i] for i in sectors[sec]]
        assert [int(np.clip(np.rint(x * f(255)), 0, 255)) for x in bgr] == out


def test_host_path_pads_and_flips_like_the_reference():
    """apply_plan_host against the straight-line composition: PIL resize, crop, colour, np.flip, F.pad with possibly negative amounts."""
    for cid in ("pad_grows_flip", "pad_crops_flip", "pad_mixed"):
        i = AC.GEOMETRY_IDS.index(cid)
        case, colour = AC.GEOMETRY[i], AC.case_colour(i)
        frames, pan, label = AC.make_inputs(cid)
        images, ids, lab = AC.host_reference(cid)
        (h, w), (nh, nw), (x0, y0, cw, ch), flip, (H, W) = case[1], case[2], case[3], case[4], case[5]
        amounts = [0, W - cw, 0, H - ch]
        for k, img in enumerate(frames):
            img = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))[y0:y0 + ch, x0:x0 + cw]
            img = T.ssd_colour(img, colour)
            img = np.flip(img, axis=1) if flip else img
            t = torch.nn.functional.pad(torch.as_tensor(np.ascontiguousarray(img.transpose(2, 0, 1))), amounts, value=128)
            assert np.array_equal(images[k], t.numpy())
        seg = np.asarray(Image.fromarray(pan).resize((nw, nh), Image.NEAREST))[y0:y0 + ch, x0:x0 + cw]
        seg = np.flip(seg, axis=1) if flip else seg
        t = torch.nn.functional.pad(torch.as_tensor(T.rgb2id(seg).astype("long")), amounts, value=0)
        assert np.array_equal(ids, t.numpy()) and ids.dtype == np.int32
        t = torch.from_numpy(label.astype("double")).view(h, w, 1, 1).permute(2, 3, 0, 1)
        sem = torch.nn.functional.interpolate(t, (nh, nw), mode="nearest")[0, 0].numpy()[y0:y0 + ch, x0:x0 + cw]
        sem = np.flip(sem, axis=1) if flip else sem
        t = torch.nn.functional.pad(torch.as_tensor(sem.astype("long")), amounts, value=255)
        assert np.array_equal(lab, t.numpy())


def test_every_geometry_case_fits_the_kernel_tile_and_its_records_are_well_formed():
    from uenc import kernels as K
    assert (K.AUG_TILE_W, K.AUG_TILE_H) == (AC.TILE_W, AC.TILE_H)
    for i, case in enumerate(AC.GEOMETRY):
        frames, pan, label = AC.make_inputs(case[0])
        plan = AC.make_plan(case, AC.case_colour(i))
        buf, off, meta = T.pack_plan(plan, frames, pan, label)
        assert K.augment_tile_fits(*plan.src_hw, *plan.resized_hw, meta["kx"], meta["ky"]), case[0]
        assert all(v % 16 == 0 for v in off.values()) and buf.numel() % 16 == 0
        cw = plan.crop[2]
        col = buf.numpy()[off["col_tab"]:off["col_tab"] + 4 * cw * (2 + meta["kx"])].view(np.int32)
        first, count = col[:cw], col[cw:2 * cw]
        assert (first >= 0).all() and (count >= 1).all() and (count <= meta["kx"]).all() and (first + count <= plan.src_hw[1]).all()
