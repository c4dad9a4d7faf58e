"""csrc/augment.hip against the host path (uenc.train_data.apply_plan_host: PIL resize, crop, the numpy colour stages, flip, pad), bit for
bit, for every case of tests/augment_cases.py: the image planes, the id map and the label map.  The float32 HSV -> BGR stage is part of
the comparison: the device repeats the host's operations one by one."""
import numpy as np
import pytest
import torch

import augment_cases as AC
from uenc import train_data as T

pytestmark = pytest.mark.gpu


def _device(plan, frames, pan, label):
    images, ids, lab = T.apply_plan_device(plan, frames, pan, label, "cuda")
    torch.cuda.synchronize()
    return images.cpu().numpy(), None if ids is None else ids.cpu().numpy(), None if lab is None else lab.cpu().numpy()


@pytest.mark.parametrize("case", AC.GEOMETRY, ids=AC.GEOMETRY_IDS)
def test_kernels_equal_the_host_path(case):
    i = AC.GEOMETRY_IDS.index(case[0])
    frames, pan, label = AC.make_inputs(case[0])
    ref_images, ref_ids, ref_lab = AC.host_reference(case[0])
    images, ids, lab = _device(AC.make_plan(case, AC.case_colour(i)), frames, pan, label)
    assert images.dtype == np.uint8 and images.shape == ref_images.shape
    assert np.array_equal(images, ref_images), int((images != ref_images).sum())
    assert ids.dtype == np.int32 and np.array_equal(ids, ref_ids)
    if label is None:
        assert lab is None and ref_lab is None
    else:
        assert lab.dtype == np.int32 and np.array_equal(lab, ref_lab)


@pytest.mark.parametrize("name,p", AC.COLOUR, ids=AC.COLOUR_IDS)
def test_colour_stages_equal_the_host_path(name, p):
    """The colour stages alone (an identity resize of the pixel set), every stage combination, order and hue."""
    px = AC.colour_pixels()
    h, w = px.shape[:2]
    plan = T.AugPlan((h, w), (h, w), (0, 0, w, h), False, (h, w), p)
    images, _, _ = _device(plan, [px], None, None)
    ref = T.ssd_colour(px, p).transpose(2, 0, 1)
    bad = np.argwhere((images[0] != ref).any(0))
    assert len(bad) == 0, (len(bad), px[tuple(bad[0])].tolist(), images[0][:, bad[0][0], bad[0][1]].tolist(), ref[:, bad[0][0], bad[0][1]].tolist())


def test_geometry_with_every_colour_off_and_frames_apart():
    """No colour table at all (colour_tab NULL), and four frames whose stride is not their size (the 16-byte padding between them)."""
    case = AC.GEOMETRY[AC.GEOMETRY_IDS.index("down_odd_full_f4")]
    frames, pan, label = AC.make_inputs(case[0])
    plan = AC.make_plan(case, None)
    assert (case[1][0] * case[1][1] * 3) % 16 != 0
    ref = T.apply_plan_host(plan, frames, pan, label)
    got = _device(plan, frames, pan, label)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)


def test_a_plan_whose_tile_does_not_fit_is_an_error():
    from uenc.capi import UencError
    img = np.zeros((64, 640, 3), np.uint8)
    plan = T.AugPlan((64, 640), (16, 160), (0, 0, 160, 16), False, (16, 160), None)      # x0.25: 9 taps, 257 source pixels per tile
    with pytest.raises(UencError):
        T.apply_plan_device(plan, [img], None, None, "cuda")
