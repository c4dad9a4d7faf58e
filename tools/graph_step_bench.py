"""Eager training step vs its HIP-graph replay (uenc.graphs.GraphedTrainStep) on the bench workload: Swin-L OneFormer, 1024 x 2048,
batch 2, one GPU.  Prints one JSON line per mode (eval / train) with ms/step (mean, median, min, max) of both.

The loss is a capture-safe restatement of bench.synthetic_loss (the same mean squares, without its host-built coefficient tensor); the
eager steps use the same loss.  Eager train mode draws its randomness on the host, as the product does by default.

    python tools/graph_step_bench.py --steps 10 --warmup 3

--optimizer adds the weight update to every leg (eval mode): the eager step followed by the reference's composition on torch
(nan_to_num per parameter, clip_grad_norm_, torch.optim.AdamW), the eager step followed by uenc.optim.FusedAdamW.step(), and the replay
of a graph that was captured with the optimizer inside.

    python tools/graph_step_bench.py --steps 10 --warmup 3 --optimizer
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


def optimizer_legs(args, model, eager_step, images, batch):
    """Eager step + torch's optimizer, eager step + FusedAdamW, replay with FusedAdamW captured.  The learning rate is tiny so that
    the weights stay where the timing of the forward / backward was measured."""
    from uenc.graphs import GraphedTrainStep
    from uenc.optim import FusedAdamW
    model.eval()
    lr, max_norm = 1e-7, 0.01
    eager_step()                                     # gradients exist; which parameters train is known
    live = [p for p in model.parameters() if p.requires_grad and p.grad is not None]
    topt = torch.optim.AdamW(live, lr=lr, weight_decay=0.05, foreach=True)

    def eager_torch():
        eager_step()
        for p in live:
            torch.nan_to_num(p.grad, nan=0.0, posinf=1e5, neginf=-1e5, out=p.grad)
        torch.nn.utils.clip_grad_norm_(live, max_norm)
        topt.step()
    fopt = FusedAdamW(live, lr=lr, weight_decay=0.05, max_grad_norm=max_norm)

    def eager_fused():
        eager_step()
        fopt.step()
    out = {}
    for name, fn in (("eager_plus_torch_adamw", eager_torch), ("eager_plus_fused_adamw", eager_fused)):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        out[name] = _stats(_timed(fn, args.steps))
    del topt
    gs = GraphedTrainStep(model, loss_fn, batch, warmup=args.warmup, optimizer=fopt)
    for _ in range(args.warmup):
        gs.step(images)
    torch.cuda.synchronize()
    out["replay_with_optimizer"] = _stats(_timed(lambda: gs.step(images), args.steps))
    print(json.dumps({"tool": "graph_step_bench", "mode": "eval+optimizer", "workload": "Swin-L OneFormer 1024x2048 bs=%d fwd+bwd+AdamW" % images.shape[0],
                      "steps": args.steps, "trained_tensors": len(live), "ms": out, "optimizer_steps_on_device": fopt.device_state()["step"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="eval,train")
    ap.add_argument("--optimizer", action="store_true", help="time the step with its weight update (eval mode only)")
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

    if args.optimizer:
        optimizer_legs(args, model, eager_step, images, batch)
        return

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
