"""Case table of the few-row NT GEMM kernel (csrc/gemm.hip: gemm_nt_fewrow_kernel), shared by tests/test_gemm_fewrow_gpu.py,
tests/test_gemm_fewrow_cases.py, tools/gemm_fewrow_identity.py and tools/gemm_fewrow_bench.py.

A case is an output shape with what it exercises; a variant is one call of kernels.gemm_nt on that shape.  Every case has the four
(A dtype, output dtype) combinations; epilogues, bias, alpha, the per-sample scale and the strided operands rotate over them so
that the table as a whole covers each (test_gemm_fewrow_cases.py checks the claims made here without a GPU).

Inputs are generated on the CPU from seeds (the scheme of `_r` in tests/test_kernels_gpu.py), so the committed hashes of
tests/golden/gemm_fewrow_parent.json are reproducible on any box; the hash of the inputs is stored beside the hash of the outputs, so
that a generator difference is reported as that and not as a kernel difference."""
import hashlib
from collections import namedtuple

EPI_NONE, EPI_GELU, EPI_RELU, EPI_RESIDUAL, EPI_MUL_DGELU, EPI_MUL_DRELU = 0, 1, 2, 3, 4, 5

# route: the kernel the shape ran on before the few-row kernel ("skinny": four k-ranges summed in order; "tile128": one chain).
# empty / partial: how many of the four k-ranges [w * per * 32, min(K, (w + 1) * per * 32)), per = ceil(ceil(K / 32) / 4), are empty /
# end inside a 32-wide k-step or before their nominal end.  tails: which edges the shape has ("m": M % 16, "n8": a column group of 4,
# "k32": K % 32).  in_step: the shape occurs in the benchmark's step.
Case = namedtuple("Case", "M N K route empty partial tails in_step what")
CASES = [
    Case(1, 4, 64, "skinny", 2, 0, ("m", "n8"), False, "smallest legal; ranges 2 and 3 empty"),
    Case(17, 36, 72, "skinny", 1, 1, ("m", "n8", "k32"), False, "K not a multiple of 32; full8 false in the last column group"),
    Case(65, 132, 136, "skinny", 1, 1, ("m", "n8", "k32"), False, "one past a 64 tile both ways; range 2 partial, range 3 empty"),
    Case(150, 20, 256, "skinny", 0, 0, ("m", "n8"), False, "N = 20"),
    Case(1000, 136, 72, "skinny", 1, 1, ("m", "k32"), False, "16 tiles of 128 x 128: on the skinny kernel before"),
    Case(300, 256, 256, "skinny", 0, 0, ("m",), True, "bench shape"),
    Case(298, 256, 2048, "skinny", 0, 0, ("m",), True, "long K, odd row count"),
    Case(300, 512, 256, "skinny", 0, 0, ("m",), True, "bench shape"),
    Case(300, 2048, 256, "tile128", 0, 0, ("m",), True, "bench shape; 48 tiles of 128 x 128"),
    Case(4096, 256, 256, "tile128", 0, 0, (), True, "bench shape; 64 tiles of 128 x 128"),
]

# One call.  scale: alpha is multiplied per sample of M / 2 rows; a_slice: A is a column slice of a wider matrix; out_slice: the
# output is a column slice of a wider buffer (the tests fill it with NaN first).  aux_out: EPI_GELU stores the pre-activation.
Variant = namedtuple("Variant", "a_f32 out_f32 epi bias alpha scale a_slice out_slice aux_out")
_BF16_EPIS = [EPI_NONE, EPI_GELU, EPI_RELU, EPI_MUL_DGELU, EPI_MUL_DRELU]
_F32_EPIS = [EPI_NONE, EPI_RESIDUAL, EPI_RELU]


def variants(ci):
    """The four calls of case `ci`: (A bf16 | fp32) x (out bf16 | fp32).  Everything else rotates with the case and combination index."""
    c = CASES[ci]
    out = []
    for j, (a_f32, out_f32) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        r = ci * 4 + j
        epi = (_F32_EPIS[(ci + j) % 3] if out_f32 else _BF16_EPIS[(ci + 2 * j) % 5])
        out.append(Variant(a_f32, out_f32, epi, bias=(r % 3 != 2), alpha=(0.5 if r % 4 == 1 else 1.0),
                           scale=(c.M == 300 and j in (0, 3)), a_slice=(r % 5 == 3), out_slice=(r % 2 == 0),
                           aux_out=(epi == EPI_GELU and r % 8 != 5)))
    return out


def all_variants():
    return [(ci, vi, v) for ci in range(len(CASES)) for vi, v in enumerate(variants(ci))]


def variant_id(ci, vi):
    c, v = CASES[ci], variants(ci)[vi]
    return f"{c.M}x{c.N}x{c.K}-{'f32' if v.a_f32 else 'bf16'}-{'f32' if v.out_f32 else 'bf16'}-e{v.epi}"


def k_ranges(K):
    """The four k-ranges of the skinny summation order, as (begin, end) with end <= begin for an empty one."""
    per = (((K + 31) // 32) + 3) // 4
    return [(w * per * 32, min(K, (w + 1) * per * 32)) for w in range(4)]


def parent_route(M, N, K):
    """The kernel of the parent commit for an unbatched, unsummed call with tile == 0 whose shape the LDS-DMA kernels do not take
    (every case here: fewer than 160 tiles of 256 x 256 and fewer than 96 of 128 x 256)."""
    tiles256 = ((M + 255) // 256) * ((N + 255) // 256)
    htiles = ((M + 127) // 128) * ((N + 255) // 256)
    assert tiles256 < 160 and htiles < 96
    tiles128 = ((M + 127) // 128) * ((N + 127) // 128)
    return "skinny" if tiles128 <= 32 and K >= 64 else "tile128"


def _randn(shape, seed, scale=1.0):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def make_inputs(ci, vi):
    """CPU tensors of one call, by seed: dict with a (M, K [+ 16 when sliced]), w, bias, aux, scale (None where unused)."""
    import torch
    c, v = CASES[ci], variants(ci)[vi]
    seed = 100 * ci + 10 * vi
    Kw = c.K + 16 if v.a_slice else c.K
    a = _randn((c.M, Kw), seed + 1).to(torch.float32 if v.a_f32 else torch.bfloat16)
    w = _randn((c.N, c.K), seed + 2, c.K ** -0.5).to(torch.bfloat16)
    bias = _randn((c.N,), seed + 3) if v.bias else None
    aux = None
    if v.epi == EPI_RESIDUAL:
        aux = _randn((c.M, c.N), seed + 4)
    elif v.epi in (EPI_MUL_DGELU, EPI_MUL_DRELU):
        aux = _randn((c.M, c.N), seed + 4).to(torch.bfloat16)
    scale = torch.tensor([1.25, 0.75]) if v.scale else None
    return {"a": a, "w": w, "bias": bias, "aux": aux, "scale": scale}


def inputs_hash(inp):
    h = hashlib.sha256()
    for k in ("a", "w", "bias", "aux", "scale"):
        t = inp[k]
        if t is not None:
            h.update(k.encode())
            h.update(t.contiguous().view(-1).view(__import__("torch").uint8).numpy().tobytes())
    return h.hexdigest()


PAD = 8     # columns of sentinel on each side of a sliced output


def run_variant(K, ci, vi, inp):
    """One call on the GPU.  Returns (padded output buffer, (column begin, column end) of the window, aux_out or None)."""
    import torch
    c, v = CASES[ci], variants(ci)[vi]
    dev = {k: (t.cuda() if t is not None else None) for k, t in inp.items()}
    a = dev["a"][:, 8:8 + c.K] if v.a_slice else dev["a"]
    odt = torch.float32 if v.out_f32 else torch.bfloat16
    lo, hi = (PAD, PAD + c.N) if v.out_slice else (0, c.N)
    buf = torch.full((c.M, c.N + (2 * PAD if v.out_slice else 0)), float("nan"), dtype=odt, device="cuda")
    aux_out = torch.full((c.M, c.N), float("nan"), dtype=torch.bfloat16, device="cuda") if v.aux_out else None
    kw = dict(bias=dev["bias"], epilogue=v.epi, aux=dev["aux"], aux_out=aux_out, out=buf[:, lo:hi], alpha=v.alpha)
    if v.scale:
        kw.update(sample_scale=dev["scale"], rows_per_sample=c.M // 2)
    K.gemm_nt(a, dev["w"], **kw)
    return buf, (lo, hi), aux_out


def outputs_hash(buf, win, aux_out):
    h = hashlib.sha256()
    import torch
    o = buf[:, win[0]:win[1]].contiguous().cpu()
    h.update(o.view(-1).view(torch.uint8).numpy().tobytes())
    if aux_out is not None:
        h.update(aux_out.contiguous().cpu().view(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def reference(ci, vi, inp):
    """(pre-activation, result) in float64 from the bf16-rounded operands."""
    import torch
    c, v = CASES[ci], variants(ci)[vi]
    a = inp["a"][:, 8:8 + c.K] if v.a_slice else inp["a"]
    pre = a.to(torch.bfloat16).double() @ inp["w"].double().t()
    if v.bias:
        pre = pre + inp["bias"].double()
    al = torch.full((c.M, 1), v.alpha, dtype=torch.float64)
    if v.scale:
        al = al * inp["scale"].double()[torch.arange(c.M) // (c.M // 2)].unsqueeze(1)
    pre = pre * al
    if v.epi == EPI_NONE:
        y = pre
    elif v.epi == EPI_GELU:
        y = torch.nn.functional.gelu(pre)
    elif v.epi == EPI_RELU:
        y = pre.clamp_min(0)
    elif v.epi == EPI_RESIDUAL:
        y = pre + inp["aux"].double()
    else:
        s = inp["aux"].double()
        if v.epi == EPI_MUL_DGELU:
            d = 0.5 * (1 + torch.erf(s * 0.5 ** 0.5)) + s * torch.exp(-0.5 * s * s) * (2 * torch.pi) ** -0.5
        else:
            d = (s > 0).double()
        y = pre * d
    return pre, y
