"""Eager training step vs its HIP-graph replay (uenc.graphs.GraphedTrainStep) on the bench workload: Swin-L OneFormer, 1024 x 2048,
batch 2, one GPU.  Prints one JSON line per mode (eval / train) with ms/step (mean, median, min, max) of both.

The loss is a capture-safe restatement of bench.synthetic_loss (the same mean squares, without its host-built coefficient tensor); the
eager steps use the same loss.  Eager train mode draws its randomness on the host, as the product does by default.

    python tools/graph_step_bench.py --steps 10 --warmup 3
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "uni-encoder-code_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def loss_fn(out):
    loss = out["pred_logits"].float().square().mean() + out["pred_masks"].float().square().mean()
    for a in out["aux_outputs"]:
        loss = loss + 0.1 * (a["pred_logits"].float().square().mean() + a["pred_masks"].float().square().mean())
    return loss


def _stats(ms):
    return {"mean": round(statistics.mean(ms), 3), "median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def _timed(fn, steps):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="eval,train")
    args = ap.parse_args()

    import bench
    from uenc import ops
    from uenc.d2 import build_model
    from uenc.graphs import GraphedTrainStep

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = build_model(bench.make_cfg(dev))
    g = torch.Generator().manual_seed(1000)
    images = torch.randint(0, 256, (bench.PER_GPU_BATCH, 3, bench.H_IMG, bench.W_IMG), generator=g).float().to(dev)
    batch = [{"left_image": images[i], "task": "The task is panoptic", "type": "segmentation"} for i in range(images.shape[0])]
    params = [p for p in model.parameters() if p.requires_grad]

    def eager_step():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()
        ops.begin_step(fresh_grads=True)
        out, _ = model.forward_features(batch)
        loss_fn(out).backward()
        ops.flush_wgrads()

    for mode in args.modes.split(","):
        model.train(mode == "train")
        for _ in range(args.warmup):
            eager_step()
        torch.cuda.synchronize()
        eager = _timed(eager_step, args.steps)
        gs = GraphedTrainStep(model, loss_fn, batch, warmup=args.warmup)
        for _ in range(args.warmup):
            gs.step(images)
        torch.cuda.synchronize()
        replay = _timed(lambda: gs.step(images), args.steps)
        print(json.dumps({"tool": "graph_step_bench", "mode": mode, "workload": "Swin-L OneFormer 1024x2048 bs=%d fwd+bwd" % images.shape[0],
                          "steps": args.steps, "eager_ms": _stats(eager), "replay_ms": _stats(replay),
                          "speedup_median": round(statistics.median(eager) / statistics.median(replay), 3)}), flush=True)
        del gs
        torch.cuda.synchronize()
    model.eval()


if __name__ == "__main__":
    main()
