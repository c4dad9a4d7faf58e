"""Micro-benchmark of the few-row NT GEMM shapes of the step, on the library that is loaded.  Per shape: N back-to-back launches timed by
device events after a warm-up, and the same N launches with a 300-row layernorm_fwd between them (the step runs these GEMMs inside
dependent chains, so the second figure minus the LayerNorm control is the one that matters).  Controls, two kernels the few-row work
does not change: layernorm_fwd on 300 x 256 and gemm_nt on 16384 x 768 x 768.  Prints one JSON line:

    python tools/gemm_fewrow_bench.py [--n 200] [--label TEXT]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uni-encoder-code_amd"))
import torch
from uenc import kernels as K

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=200)
ap.add_argument("--label", default="")
args = ap.parse_args()
bf, f32 = torch.bfloat16, torch.float32
# (M, N, K, A dtype, epilogue, out dtype): the operand / epilogue forms the step runs (profiles/r03_gemm_shapes.txt)
SHAPES = [
    (300, 256, 256, f32, 0, bf), (300, 256, 256, bf, 0, f32), (300, 256, 256, bf, 3, f32), (300, 256, 256, bf, 5, bf),
    (300, 512, 256, f32, 0, bf), (300, 256, 512, bf, 0, f32),
    (298, 256, 2048, bf, 0, f32), (300, 256, 2048, bf, 3, f32),
    (300, 2048, 256, f32, 2, bf), (300, 2048, 256, f32, 5, bf),
    (4096, 256, 256, bf, 0, f32), (4096, 256, 256, f32, 0, bf),
    (16384, 256, 256, bf, 0, f32),
]
ln_x = torch.randn(300, 256, device="cuda"); ln_g = torch.ones(256, device="cuda"); ln_b = torch.zeros(256, device="cuda")


def ln():
    K.layernorm_fwd(ln_x, ln_g, ln_b, out_dtype=bf)


def timed(fn, n, between=None):
    """us per iteration: the n launches are captured into one graph (a linear chain), so that the host's enqueue cost, which is above
    these kernels' durations, is not what is timed; the graph is replayed four times and the fastest replay counts."""
    def body(k):
        for _ in range(k):
            fn()
            if between is not None:
                between()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body(5)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body(n)
    best = 1e30
    for _ in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / n)
    return best


res = {"label": args.label, "n": args.n, "shapes": {}, "controls": {}}
res["controls"]["layernorm_300x256"] = round(timed(ln, args.n), 3)
ca = torch.randn(16384, 768, device="cuda").to(bf); cw = (torch.randn(768, 768, device="cuda") / 28).to(bf); co = torch.empty(16384, 768, device="cuda", dtype=bf)
res["controls"]["gemm_nt_16384x768x768"] = round(timed(lambda: K.gemm_nt(ca, cw, out=co), args.n), 3)
for M, N, Kd, adt, epi, odt in SHAPES:
    a = torch.randn(M, Kd, device="cuda").to(adt)
    w = (torch.randn(N, Kd, device="cuda") * Kd ** -0.5).to(bf)
    bias = torch.randn(N, device="cuda")
    aux = torch.randn(M, N, device="cuda").to(f32 if epi == 3 else bf) if epi >= 3 else None
    out = torch.empty(M, N, device="cuda", dtype=odt)
    fn = lambda: K.gemm_nt(a, w, bias=bias, epilogue=epi, aux=aux, out=out)
    key = f"{M}x{N}x{Kd}-{'f32' if adt == f32 else 'bf16'}-e{epi}-{'f32' if odt == f32 else 'bf16'}"
    res["shapes"][key] = {"back_to_back_us": round(timed(fn, args.n), 3), "with_layernorm_us": round(timed(fn, args.n, ln), 3)}
res["controls"]["layernorm_300x256_again"] = round(timed(ln, args.n), 3)
res["controls"]["gemm_nt_16384x768x768_again"] = round(timed(lambda: K.gemm_nt(ca, cw, out=co), args.n), 3)
print(json.dumps(res))
