"""Records a sha256 of every output of the few-row GEMM case table (tests/gemm_fewrow_cases.py) on the library that is loaded, with a
hash of the seeded CPU-generated inputs beside it.  Run on the GPU box:

    python tools/gemm_fewrow_identity.py OUT.json [--label TEXT]

Run on the parent commit's library (twice: the kernels have no atomics, the two files must agree) the result is
tests/golden/gemm_fewrow_parent.json; tests/test_gemm_fewrow_gpu.py asserts that the current library reproduces it."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uni-encoder-code_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import gemm_fewrow_cases as C
from uenc import kernels as K

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--label", default="")
args = ap.parse_args()
rec = {"label": args.label, "cases": {}}
for ci, vi, v in C.all_variants():
    inp = C.make_inputs(ci, vi)
    buf, win, aux_out = C.run_variant(K, ci, vi, inp)
    torch.cuda.synchronize()
    rec["cases"][C.variant_id(ci, vi)] = {"inputs": C.inputs_hash(inp), "outputs": C.outputs_hash(buf, win, aux_out)}
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{len(rec['cases'])} calls hashed -> {args.out}")
