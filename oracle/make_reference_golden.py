"""tests/golden/oracle_vs_reference.npz from the reference's own modules (build container only; python -m oracle.make_reference_golden).

TEST INFRASTRUCTURE.  Runs the cases of tests/test_oracle_vs_reference.py and the live case of tests/test_postproc_cpu.py on the
reference's classes (oracle/ref_loader.py) and stores data only: the inputs, the parameter names and shapes of each module (from which
oracle/fill.py regenerates the same name-hashed values; the modules' only buffers, `relative_position_index`, are not read by the oracle
and are pinned by their own case) and the reference's outputs."""
import json
import os
import types
import warnings

import numpy as np
import torch

from . import fill, postproc_ref as P, ref_loader

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "oracle_vs_reference.npz")
BASIC_LAYERS = [(32, 1, 4, 9, 11), (64, 2, 7, 14, 14), (64, 2, 12, 5, 30), (96, 3, 3, 6, 9)]     # C, nH, ws, H, W
RPI_WINDOWS = (3, 7, 12)
POSTPROC_SEEDS = (5, 6)


def _layout(module, prefix, tag, meta):
    meta[tag] = {"param_shapes": {prefix + n: list(p.shape) for n, p in module.named_parameters()}}


def main():
    warnings.filterwarnings("ignore")
    ref = ref_loader.load()
    arrs, meta = {}, {}

    for C, nH, ws, H, W in BASIC_LAYERS:
        tag = f"basic_layer_{C}_{nH}_{ws}_{H}_{W}"
        layer = ref.swin.BasicLayer(dim=C, depth=2, num_heads=nH, window_size=ws, drop_path=0.0)
        layer.eval()
        fill.fill_module(layer, "backbone.layers.0.")
        x = torch.randn(2, H * W, C, generator=torch.Generator().manual_seed(H * W))
        with torch.no_grad():
            want = layer(x, H, W)[0]
        _layout(layer, "backbone.layers.0.", tag, meta)
        arrs[tag + "_x"], arrs[tag + "_out"] = x.numpy(), want.numpy()

    for ws in RPI_WINDOWS:
        arrs[f"rpi_{ws}"] = ref.swin.WindowAttention(32, (ws, ws), 1).relative_position_index.numpy().astype(np.int16)

    m = ref.swin.SwinTransformer(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=5)
    m.eval()
    fill.fill_module(m, "backbone.")
    x = torch.randn(1, 3, 70, 107, generator=torch.Generator().manual_seed(1))   # not a multiple of 4
    with torch.no_grad():
        want = m(x)
    _layout(m, "backbone.", "swin_odd", meta)
    arrs["swin_odd_x"] = x.numpy()
    meta["swin_odd"]["outputs"] = sorted(want)
    for k, v in want.items():
        arrs[f"swin_odd_{k}"] = v.numpy()

    g = torch.Generator().manual_seed(3)
    shapes = [(5, 7), (3, 4)]
    S = sum(h * w for h, w in shapes)
    value = torch.randn(2, S, 4, 8, generator=g)
    loc = torch.rand(2, 13, 4, 2, 3, 2, generator=g) * 1.4 - 0.2
    w = torch.rand(2, 13, 4, 2, 3, generator=g)
    arrs.update(msda_value=value.numpy(), msda_loc=loc.numpy(), msda_w=w.numpy(), msda_shapes=np.array(shapes, dtype=np.int64),
                msda_out=ref.msda_func.ms_deform_attn_core_pytorch(value, shapes, loc, w).numpy())

    O = ref_loader.load_meta_arch().OneFormer
    meta["postproc_info"] = {}
    for seed in POSTPROC_SEEDS:
        cls, masks = P.synthetic_predictions(14, 7, 12, 20, seed)
        mp = P.upsample_and_crop(masks, (48, 80), (44, 80), (44, 80))
        fake = types.SimpleNamespace(sem_seg_head=types.SimpleNamespace(num_classes=7), object_mask_threshold=0.4, overlap_threshold=0.7,
                                     metadata=types.SimpleNamespace(thing_dataset_id_to_contiguous_id={5: 5, 6: 6}))
        seg, info = O.panoptic_inference(fake, cls, mp)
        arrs.update({f"pp{seed}_cls": cls.numpy(), f"pp{seed}_masks": masks.numpy(),
                     f"pp{seed}_sem": O.semantic_inference(fake, cls, mp).numpy(), f"pp{seed}_pan": seg.numpy()})
        meta["postproc_info"][str(seed)] = info

    arrs["meta_json"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **arrs)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
