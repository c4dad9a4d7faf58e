"""Thin launch wrappers: torch tensors in, C-ABI calls out.  No autograd here (see `ops.py`).

Every wrapper validates what the kernel's grid assumes (device, dtype, inner stride 1) before
handing raw pointers to the library; the library re-checks alignment and sizes and refuses
(-1) rather than launching on a bad shape.
"""
import collections
import ctypes
import itertools
import operator
import os
from typing import Optional

import numpy as np
import torch

from . import capi
from .capi import BF16, F32, check, dt, lib, ptr, stream_ptr

EPI_NONE, EPI_GELU, EPI_RELU, EPI_RESIDUAL, EPI_MUL_DGELU, EPI_MUL_DRELU = (
    capi.EPI_NONE, capi.EPI_GELU, capi.EPI_RELU, capi.EPI_RESIDUAL, capi.EPI_MUL_DGELU, capi.EPI_MUL_DRELU)
_H = capi.CONSTANTS             # the integer UENC_* macros of include/uenc.h: the constants of this module that mirror one are read from it
NT_TILE_256X256, NT_TILE_256X192, NT_TILE_128X256 = (_H["UENC_NT_TILE_" + t] for t in ("256X256", "256X192", "128X256"))     # gemm_nt's `tile`


# fp32 "exact" arithmetic mode (csrc/exact.hip): every activation that is bf16 between kernels in the
# product becomes fp32 and every contraction runs on fp32 operands.  A verification mode: UENC_EXACT=1 or ops.set_exact(True).
EXACT = os.environ.get("UENC_EXACT", "0") == "1"


def adt():
    """dtype of activations handed from kernel to kernel: bf16, or fp32 in exact mode."""
    return torch.float32 if EXACT else torch.bfloat16


def _odt(dtype):
    return torch.float32 if (EXACT and dtype == torch.bfloat16) else dtype


def _mat(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise capi.UencError(f"{name} must live on the GPU")
    if t.dim() != 2 or t.stride(1) != 1:
        raise capi.UencError(f"{name} must be 2-D with unit inner stride, got {tuple(t.shape)} / {t.stride()}")
    return t


# While a training step is being captured into a HIP graph (uenc/graphs.py): [pinned uint8 host buffer, next free offset].  Descriptor
# tables are then staged in this buffer, which the captured step owns for the graph's lifetime, and copied by uenc_upload: every replay
# re-reads them from there.  (A temporary pinned tensor would be recycled by torch's host allocator once freed.)
CAPTURE_ARENA = None


def upload_table(arr, device, pinned: bool = True) -> torch.Tensor:
    """Device copy of a numpy descriptor table (raw bytes).  Eager: a pinned (or, pinned=False, pageable) temporary and torch's copy, as the
    launch sites always did; during a capture: staged in the capture's host arena."""
    raw = arr.view(np.uint8).reshape(-1)
    if CAPTURE_ARENA is None:
        if not pinned:
            return torch.from_numpy(raw.copy()).to(device)
        return torch.from_numpy(raw).pin_memory().to(device, non_blocking=True)
    host, off = CAPTURE_ARENA[0], CAPTURE_ARENA[1]
    n = int(raw.size)
    end = off + -(-n // 256) * 256
    if end > host.numel():
        raise RuntimeError(f"captured step: descriptor tables exceed the capture's {host.numel()} byte host arena")
    host[off:off + n].numpy()[:] = raw
    CAPTURE_ARENA[1] = end
    tab = torch.empty(n, dtype=torch.uint8, device=device)
    check(lib.uenc_upload(tab.data_ptr(), host.data_ptr() + off, n, stream_ptr()), "upload")
    return tab


def pack_table(dtype, recs, counts, begin: str):
    """Descriptor table of a grouped launch: every field of `dtype` read from the records' attribute of the same name, except `pad`
    (zero) and `begin`, the running sum of `counts` (the work items / workgroups of each record).  -> (numpy table, the count in all)"""
    names = [f for f, _ in dtype if f not in (begin, "pad")]
    tab = np.zeros(len(recs), dtype=dtype)
    tab[names] = list(map(operator.attrgetter(*names), recs))
    begins = [0, *itertools.accumulate(counts)]
    total = begins.pop()
    tab[begin] = begins
    return tab, total


class SeedSlot:
    """A dropout seed that lives on the device: word `slot` of the seed table `seeds` (uint32 as int32), written once per step by
    uenc_step_rng_advance.  Kernels given a SeedSlot read the seed themselves (the *_sp entry points), so a replayed graph draws the
    step's fresh mask."""
    __slots__ = ("seeds", "slot", "owner", "gen")

    def __init__(self, seeds: torch.Tensor, slot: int, owner=None):
        assert seeds.dtype == torch.int32 and seeds.is_cuda and 0 <= slot < seeds.numel()
        self.seeds, self.slot, self.owner = seeds, int(slot), owner
        self.gen = owner.generation if owner is not None else 0

    def check(self):
        """owner: the ops.DeviceRNG that wrote the table; refuses a use after it moved on to another step (begin_step between a forward
        and its backward)."""
        if self.owner is not None and self.owner.generation != self.gen:
            raise RuntimeError("device RNG: ops.begin_step() ran between this dropout's forward and its backward -- the seed table now "
                               "holds the next step's seeds")

    def value(self) -> int:
        """The seed as a python int (a device sync: tests only)."""
        return int(self.seeds[self.slot].item()) & 0xFFFFFFFF


def dropout_bf16(x16: torch.Tensor, seed, p: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Inverted dropout of a contiguous bf16 tensor with the index-hash keep mask (uenc_dropout_bf16); out=x16 for in place.
    seed: an int, or a SeedSlot (uenc_dropout_sp: the same mask, seed read on the device)."""
    assert x16.dtype == torch.bfloat16 and x16.is_contiguous() and x16.is_cuda and x16.numel() % 8 == 0
    if out is None:
        out = torch.empty_like(x16)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.numel() == x16.numel()
    if isinstance(seed, SeedSlot):
        return dropout_sp(x16, seed, p, out=out)
    check(lib.uenc_dropout_bf16(x16.data_ptr(), out.data_ptr(), x16.numel(), int(seed) & 0xFFFFFFFF, float(p), stream_ptr()), "dropout_bf16")
    return out


def dropout_keep_reference(shape, p: float, seed: int) -> torch.Tensor:
    """The keep-mask uenc_dropout_bf16 derives for a tensor of `shape` (row-major index), restated on the host.  Test helper."""
    from .attention import keep_mask_reference
    n = 1
    for d in shape:
        n *= int(d)
    return keep_mask_reference(1, 1, 1, n, p, int(seed) & 0xFFFFFFFF).view(tuple(shape))


def dropout_sp(x: torch.Tensor, seed: SeedSlot, p: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Inverted dropout of a contiguous fp32 / bf16 tensor (any size) with the seed read from the device table (uenc_dropout_sp):
    the keep-mask of `dropout_keep_reference(x.shape, p, seed)`.  out=x for in place."""
    assert x.is_cuda and x.is_contiguous() and x.dtype in (torch.float32, torch.bfloat16) and isinstance(seed, SeedSlot)
    seed.check()
    if out is None:
        out = torch.empty_like(x)
    assert out.dtype == x.dtype and out.is_contiguous() and out.numel() == x.numel()
    if x.numel():
        check(lib.uenc_dropout_sp(x.data_ptr(), out.data_ptr(), x.numel(), dt(x), seed.seeds.data_ptr(), seed.slot, float(p), stream_ptr()),
              "dropout_sp")
    return out


def scale_rows_bf16(g16: torch.Tensor, sample_scale: torch.Tensor, rows_per_sample: int) -> torch.Tensor:
    """bf16 copy of a (M, C) gradient with the rows of sample b multiplied by sample_scale[b] (device fp32)."""
    g16 = _mat(g16, "g16")
    assert g16.dtype == torch.bfloat16 and sample_scale.dtype == torch.float32 and sample_scale.is_cuda
    M, C = g16.shape
    out = torch.empty((M, C), dtype=torch.bfloat16, device=g16.device)
    check(lib.uenc_scale_rows_bf16(g16.data_ptr(), g16.stride(0), out.data_ptr(), C, M, C, sample_scale.data_ptr(), int(rows_per_sample),
                                   stream_ptr()), "scale_rows_bf16")
    return out


def step_rng_advance(state: torch.Tensor, keep_prob: torch.Tensor, n_branch: int, n_samples: int, scales: torch.Tensor, n_seed: int,
                     seeds: torch.Tensor, advance: bool = True):
    """uenc_step_rng_advance: state (2,) int64 {base seed, step} on the device; keep_prob (>= n_branch,) fp32; scales (>= n_branch * n_samples,)
    fp32; seeds (>= n_seed,) int32 (uint32 bits)."""
    assert state.dtype == torch.int64 and state.numel() == 2 and state.is_cuda
    assert keep_prob.dtype == torch.float32 and scales.dtype == torch.float32 and seeds.dtype == torch.int32
    assert keep_prob.numel() >= n_branch and scales.numel() >= n_branch * n_samples and seeds.numel() >= n_seed
    check(lib.uenc_step_rng_advance(state.data_ptr(), keep_prob.data_ptr(), int(n_branch), int(n_samples), scales.data_ptr(), int(n_seed),
                                    seeds.data_ptr(), int(bool(advance)), stream_ptr()), "step_rng_advance")


def _mix32_np(seed, idx):
    """uenc_mix32 of common.h on numpy uint64 arrays (seed: uint32 values, idx: uint64) -> uint32 values as uint64."""
    M = np.uint64(0xFFFFFFFF)
    idx = np.asarray(idx, dtype=np.uint64)
    x = (((idx & M) ^ (((idx >> np.uint64(32)) * np.uint64(0x9E3779B9)) & M)) + np.asarray(seed, dtype=np.uint64)) & M
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & M
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & M
    x ^= x >> np.uint64(16)
    return x


def step_rng_reference(base_seed: int, step: int, keep_prob, n_samples: int, n_seed: int):
    """The tables uenc_step_rng_advance writes for (base seed, step), restated on the host with numpy integer / fp32 arithmetic.
    -> (scales (len(keep_prob), n_samples) float32, seeds (n_seed,) uint32).  `step` is the counter value AFTER the advance."""
    base, step = np.uint64(int(base_seed) & (2 ** 64 - 1)), np.uint64(int(step) & (2 ** 64 - 1))
    h = _mix32_np(base >> np.uint64(32), step)
    key = _mix32_np((base & np.uint64(0xFFFFFFFF)) ^ h, step)
    seeds = _mix32_np(key, np.uint64(1 << 40) | np.arange(n_seed, dtype=np.uint64)).astype(np.uint32)
    kp = np.asarray(keep_prob, dtype=np.float32)
    nb = kp.size
    idx = np.arange(nb * n_samples, dtype=np.uint64)
    x = _mix32_np(key, np.uint64(1 << 41) | idx).reshape(nb, n_samples)
    dp = (np.float32(1.0) - kp).astype(np.float32)
    thresh = np.array([0 if d <= 0 else (0xFFFFFFFF if d >= 1 else int(float(d) * 4294967296.0)) for d in dp], dtype=np.uint64)
    keep = (kp[:, None] > 0) & (x >= thresh[:, None])
    inv = (np.float32(1.0) / np.where(kp > 0, kp, np.float32(1.0))).astype(np.float32)
    scales = np.where(keep, inv[:, None], np.float32(0.0)).astype(np.float32)
    return scales, seeds


def cast_bf16(src: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 -> bf16 copy (weights).  numel must be a multiple of 8, else falls to the padded path."""
    assert src.dtype == torch.float32 and src.is_contiguous() and src.is_cuda
    if EXACT:                                   # the "bf16 copy" of an fp32 tensor is the tensor itself
        return src if out is None else out.copy_(src)
    if out is None:
        out = torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    n = src.numel()
    if n % 8 == 0 and src.data_ptr() % 16 == 0:
        check(lib.uenc_cast_f32_bf16(src.data_ptr(), out.data_ptr(), n, stream_ptr()), "cast_f32_bf16")
    else:  # tiny odd-sized vectors (biases of odd length): treated as a 1 x n transpose
        check(lib.uenc_cast_transpose_f32_bf16(src.data_ptr(), out.data_ptr(), 1, n, stream_ptr()), "cast_f32_bf16")
    return out


def cast_transpose_bf16(src: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(R, C) fp32 -> (C, R) bf16."""
    assert src.dtype == torch.float32 and src.dim() == 2 and src.is_contiguous() and src.is_cuda
    R, C = src.shape
    if EXACT:                                   # data movement only
        return src.t().contiguous() if out is None else out.copy_(src.t())
    if out is None:
        out = torch.empty((C, R), dtype=torch.bfloat16, device=src.device)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (C, R) and out.is_contiguous()
    check(lib.uenc_cast_transpose_f32_bf16(src.data_ptr(), out.data_ptr(), R, C, stream_ptr()), "cast_transpose")
    return out


def gemm_nt(a: torch.Tensor, w: torch.Tensor, *, bias: Optional[torch.Tensor] = None, epilogue: int = EPI_NONE,
            aux: Optional[torch.Tensor] = None, aux_out: Optional[torch.Tensor] = None,
            out: Optional[torch.Tensor] = None, out_dtype=torch.bfloat16, alpha: float = 1.0,
            splitk: int = 1, accumulate: bool = False, sample_scale: Optional[torch.Tensor] = None, rows_per_sample: int = 0,
            tile: int = 0) -> torch.Tensor:
    """out[m, n] = epi(alpha * (sum_k a[m, k] * w[n, k] + bias[n])).  a fp32|bf16, w bf16, fp32 accumulate.
    sample_scale (device fp32, one entry per `rows_per_sample` rows): alpha is multiplied by the row's sample scale (DropPath).
    tile (tests, A/B tools): NT_TILE_256X256 / NT_TILE_256X192 / NT_TILE_128X256 names the large-tile kernel instead of the library's
    measured choice; a shape that kernel does not take raises UencError and launches nothing."""
    _mat(a, "a"); _mat(w, "w")
    M, K = a.shape
    N, K2 = w.shape
    if EXACT:
        if sample_scale is not None:
            raise capi.UencError("gemm_nt: the fp32 verification kernels take no per-sample scale")
        return _gemm_nt_exact(a, w, bias, epilogue, aux, aux_out, out, alpha, accumulate)
    if K != K2 or w.dtype != torch.bfloat16:
        raise capi.UencError(f"gemm_nt: a {tuple(a.shape)} vs w {tuple(w.shape)} / {w.dtype}")
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
        if splitk > 1 or accumulate:
            out.zero_()
    _mat(out, "out")
    assert out.shape == (M, N)
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == N and bias.is_contiguous()
    if aux is not None:
        _mat(aux, "aux"); assert aux.shape == (M, N)
        assert aux.dtype == (torch.float32 if epilogue == EPI_RESIDUAL else torch.bfloat16)
    if aux_out is not None:
        _mat(aux_out, "aux_out"); assert aux_out.shape == (M, N) and aux_out.dtype == torch.bfloat16
    if sample_scale is not None:
        assert sample_scale.dtype == torch.float32 and sample_scale.is_cuda and sample_scale.is_contiguous()
        assert rows_per_sample > 0 and sample_scale.numel() * rows_per_sample >= M and splitk == 1 and not accumulate and tile == 0
        check(lib.uenc_gemm_nt_scaled(a.data_ptr(), dt(a), a.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), dt(out),
                                      out.stride(0), M, N, K, ptr(bias), epilogue, ptr(aux), aux.stride(0) if aux is not None else 0,
                                      ptr(aux_out), aux_out.stride(0) if aux_out is not None else 0, float(alpha), sample_scale.data_ptr(),
                                      int(rows_per_sample), stream_ptr()), "gemm_nt_scaled")
        return out
    if tile != 0:
        check(lib.uenc_gemm_nt_tile(a.data_ptr(), dt(a), a.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), dt(out),
                                    out.stride(0), M, N, K, ptr(bias), epilogue, ptr(aux), aux.stride(0) if aux is not None else 0,
                                    ptr(aux_out), aux_out.stride(0) if aux_out is not None else 0, float(alpha), int(splitk),
                                    int(accumulate), int(tile), stream_ptr()), "gemm_nt_tile")
        return out
    check(lib.uenc_gemm_nt(a.data_ptr(), dt(a), a.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), dt(out),
                           out.stride(0), M, N, K, ptr(bias), epilogue, ptr(aux), aux.stride(0) if aux is not None else 0,
                           ptr(aux_out), aux_out.stride(0) if aux_out is not None else 0, float(alpha), int(splitk),
                           int(accumulate), stream_ptr()), "gemm_nt")
    return out


def _gemm_nt_exact(a, w, bias, epilogue, aux, aux_out, out, alpha, accumulate) -> torch.Tensor:
    """fp32 operands, fp32 result (uenc_gemm_nt_f32); same epilogues as the bf16 kernels, aux / aux_out fp32."""
    M, K = a.shape
    N, K2 = w.shape
    f32 = torch.float32
    if K != K2 or a.dtype != f32 or w.dtype != f32:
        raise capi.UencError(f"gemm_nt (exact): a {tuple(a.shape)} {a.dtype} vs w {tuple(w.shape)} {w.dtype}")
    if out is None:
        out = torch.zeros((M, N), dtype=f32, device=a.device) if accumulate else torch.empty((M, N), dtype=f32, device=a.device)
    _mat(out, "out")
    assert out.shape == (M, N) and out.dtype == f32
    for t, name in ((aux, "aux"), (aux_out, "aux_out")):
        if t is not None:
            _mat(t, name); assert t.shape == (M, N) and t.dtype == f32
    if bias is not None:
        assert bias.dtype == f32 and bias.numel() == N and bias.is_contiguous()
    check(lib.uenc_gemm_nt_f32(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), out.stride(0), M, N, K, ptr(bias),
                               epilogue, ptr(aux), aux.stride(0) if aux is not None else 0, ptr(aux_out),
                               aux_out.stride(0) if aux_out is not None else 0, float(alpha), int(accumulate), stream_ptr()), "gemm_nt_f32")
    return out


def gemm_nt_splitk(a: torch.Tensor, w: torch.Tensor, splitk: int, *, alpha: float = 1.0) -> torch.Tensor:
    """sum_k a[m, k] * w[n, k] in fp32 for a long contraction with few output tiles: `splitk` k-ranges computed by separate
    workgroups, each STORING its partial tile (no atomics), then summed.  a, w bf16 with unit inner stride."""
    _mat(a, "a"); _mat(w, "w")
    M, K = a.shape
    N, K2 = w.shape
    if EXACT:
        return _gemm_nt_exact(a, w, None, EPI_NONE, None, None, None, alpha, False)
    if K != K2 or w.dtype != torch.bfloat16:
        raise capi.UencError(f"gemm_nt_splitk: a {tuple(a.shape)} vs w {tuple(w.shape)} / {w.dtype}")
    s = lib.uenc_gemm_nt_splits(K, int(splitk))
    part = torch.empty((s, M, N), dtype=torch.float32, device=a.device)
    check(lib.uenc_gemm_nt_partials(a.data_ptr(), dt(a), a.stride(0), w.data_ptr(), w.stride(0), part.data_ptr(), N, M * N, M, N, K,
                                    float(alpha), s, stream_ptr()), "gemm_nt_partials")
    return part[0] if s == 1 else part.sum(0)


def gemm_nt_batched(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, alpha: float = 1.0, splitk: int = 1, accumulate: bool = False):
    """out[b] (+)= a[b] @ w[b]^T for b in range(B): a (B, M, K) fp32|bf16, w (B, N, K) bf16, out (B, M, N) fp32|bf16, inner strides 1.
    One launch; with splitk > 1 / accumulate, out must be fp32 (zeroed by the caller for splitk > 1)."""
    B, M, K = a.shape
    _, N, _ = w.shape
    if EXACT:
        for b in range(B):
            _gemm_nt_exact(a[b], w[b], None, EPI_NONE, None, None, out[b], alpha, accumulate or splitk > 1)
        return out
    assert a.is_cuda and w.dtype == torch.bfloat16 and w.shape == (B, N, K) and out.shape == (B, M, N)
    assert a.stride(2) == 1 and w.stride(2) == 1 and out.stride(2) == 1
    check(lib.uenc_gemm_nt_batched(a.data_ptr(), dt(a), a.stride(1), a.stride(0), w.data_ptr(), w.stride(1), w.stride(0), out.data_ptr(), dt(out),
                                   out.stride(1), out.stride(0), B, M, N, K, float(alpha), int(splitk), int(accumulate), stream_ptr()),
          "gemm_nt_batched")
    return out


def gemm_tn(dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor, db: Optional[torch.Tensor] = None, splitm: int = 0, alpha: float = 1.0,
            tile: int = 0):
    """dw[n, k] += alpha * sum_m dy[m, n] * x[m, k];  db[n] += alpha * sum_m dy[m, n].  dy bf16, x fp32|bf16, dw/db fp32 (accumulated).
    tile (tests): 256 or 128 names the output tile of the LDS-DMA kernel instead of the library's choice; operands it does not take
    (not both bf16, M % 64 != 0, M < 2048) raise UencError and launch nothing."""
    _mat(dy, "dy"); _mat(x, "x"); _mat(dw, "dw")
    M, N = dy.shape
    M2, K = x.shape
    if M != M2 or dw.dtype != torch.float32 or dw.shape != (N, K):
        raise capi.UencError(f"gemm_tn: dy {tuple(dy.shape)} x {tuple(x.shape)} dw {tuple(dw.shape)}")
    if db is not None:
        assert db.dtype == torch.float32 and db.numel() == N and db.is_contiguous()
    if EXACT:
        assert dy.dtype == torch.float32 and x.dtype == torch.float32 and alpha == 1.0
        check(lib.uenc_gemm_tn_f32(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dw.data_ptr(), dw.stride(0), ptr(db), M, N, K,
                                   stream_ptr()), "gemm_tn_f32")
        return
    if alpha != 1.0:
        assert tile == 0
        check(lib.uenc_gemm_tn_scaled(dy.data_ptr(), dt(dy), dy.stride(0), x.data_ptr(), dt(x), x.stride(0), dw.data_ptr(), dw.stride(0),
                                      ptr(db), M, N, K, int(splitm), float(alpha), stream_ptr()), "gemm_tn_scaled")
        return
    if tile != 0:
        check(lib.uenc_gemm_tn_tile(dy.data_ptr(), dt(dy), dy.stride(0), x.data_ptr(), dt(x), x.stride(0), dw.data_ptr(), dw.stride(0),
                                    ptr(db), M, N, K, int(splitm), int(tile), stream_ptr()), "gemm_tn_tile")
        return
    check(lib.uenc_gemm_tn(dy.data_ptr(), dt(dy), dy.stride(0), x.data_ptr(), dt(x), x.stride(0), dw.data_ptr(), dw.stride(0),
                           ptr(db), M, N, K, int(splitm), stream_ptr()), "gemm_tn")


def gemm_nt_ln(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], residual: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
               eps: float = 1e-5, want_y32: bool = True, want_y16: bool = True):
    """LayerNorm(a @ w^T + bias + residual) with the LayerNorm inside the GEMM's epilogue (one pass over the row instead of GEMM -> h ->
    LayerNorm kernel).  a (M, K) bf16, w (N, K) bf16, residual (M, N) fp32, N <= 256.
    -> (h fp32 pre-norm sum, y fp32 | None, y16 bf16 | None, stats (M, 2)) or None when the shape is not one the fused kernels take (the
    caller then runs gemm_nt + layernorm_fwd); never in the fp32 verification mode."""
    M, Kd = a.shape
    N = w.shape[0]
    if (EXACT or a.dtype != torch.bfloat16 or N > 256 or N % 8 or Kd % 64 or os.environ.get("UENC_GEMM_LN", "1") == "0"
            or not (a.stride(1) == 1 and w.stride(1) == 1 and residual.is_contiguous() and residual.dtype == torch.float32)):
        return None
    h = torch.empty((M, N), dtype=torch.float32, device=a.device)
    y32 = torch.empty((M, N), dtype=torch.float32, device=a.device) if want_y32 else None
    y16 = torch.empty((M, N), dtype=torch.bfloat16, device=a.device) if want_y16 else None
    stats = torch.empty((M, 2), dtype=torch.float32, device=a.device)
    rc = lib.uenc_gemm_nt_ln(a.data_ptr(), dt(a), a.stride(0), w.data_ptr(), w.stride(0), h.data_ptr(), N, M, N, Kd, ptr(bias), residual.data_ptr(), N,
                             gamma.data_ptr(), beta.data_ptr(), float(eps), ptr(y32), ptr(y16), stats.data_ptr(), stream_ptr())
    if rc == -1:
        return None
    check(rc, "gemm_nt_ln")
    return h, y32, y16, stats


def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, res: Optional[torch.Tensor] = None,
                  out_dtype=torch.bfloat16, want_h: bool = False, want_stats: bool = True, eps: float = 1e-5,
                  twin: Optional[list] = None):
    """y = LN(x + res).  Returns (y, h, stats): h = x + res in fp32 if want_h, stats = (M, 2) (mean, rstd).
    twin: a list that receives the bf16 copy of an fp32 y, written in the same pass."""
    C = x.shape[-1]
    assert x.is_cuda and x.is_contiguous() and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    M = x.numel() // C
    out_dtype = _odt(out_dtype)
    if EXACT and twin is not None:
        twin_exact, twin = twin, None           # the operand copy of an fp32 y is y itself
    else:
        twin_exact = None
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    h = torch.empty(x.shape, dtype=torch.float32, device=x.device) if want_h else None
    stats = torch.empty((M, 2), dtype=torch.float32, device=x.device) if want_stats else None
    if res is not None:
        assert res.shape == x.shape and res.is_contiguous()
    y16 = None
    if twin is not None and out_dtype == torch.float32:
        y16 = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
        twin.append(y16)
    check(lib.uenc_layernorm_fwd(x.data_ptr(), dt(x), ptr(res), dt(res) if res is not None else 0, ptr(h),
                                 gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), dt(y), ptr(stats), M, C, float(eps),
                                 ptr(y16), stream_ptr()), "layernorm_fwd")
    if twin_exact is not None and out_dtype == torch.float32:
        twin_exact.append(y)
    return y, h, stats


def layernorm_bwd(dy: torch.Tensor, h: torch.Tensor, stats: torch.Tensor, gamma: torch.Tensor, *,
                  dres: Optional[torch.Tensor] = None, dgamma: Optional[torch.Tensor] = None,
                  dbeta: Optional[torch.Tensor] = None, dx_dtype=torch.float32, twin: Optional[list] = None,
                  defer: Optional["SmallReductions"] = None) -> torch.Tensor:
    """dx = LN'(dy) [+ dres]; dgamma / dbeta are accumulated in place (fp32).  twin: a list that receives the bf16 copy of an
    fp32 dx, written in the same pass.  defer: a SmallReductions queue -- the dgamma / dbeta block partials are parked in a private
    buffer and summed by the queue's next flush (one launch for all parked passes) instead of by a launch of their own."""
    C = h.shape[-1]
    M = h.numel() // C
    assert dy.is_contiguous() and h.is_contiguous() and dy.shape == h.shape
    dx_dtype = _odt(dx_dtype)
    twin_exact = None
    if EXACT and twin is not None:
        twin_exact, twin = twin, None
    dx = torch.empty(h.shape, dtype=dx_dtype, device=h.device)
    if dres is not None:
        assert dres.dtype == torch.float32 and dres.is_contiguous() and dres.shape == h.shape
    dx16 = None
    if twin is not None and dx_dtype == torch.float32:
        dx16 = torch.empty(h.shape, dtype=torch.bfloat16, device=h.device)
        twin.append(dx16)
    part, deferred = _ln_part(M, C, dgamma, dbeta, h.device, defer)
    check(lib.uenc_layernorm_bwd(dy.data_ptr(), dt(dy), h.data_ptr(), dt(h), stats.data_ptr(), gamma.data_ptr(),
                                 ptr(dres), dx.data_ptr(), dt(dx), ptr(dgamma), ptr(dbeta), M, C, ptr(dx16), ptr(part), int(deferred), stream_ptr()),
          "layernorm_bwd")
    if twin_exact is not None and dx_dtype == torch.float32:
        twin_exact.append(dx)
    return dx


def postproc_semantic(mask_logits: torch.Tensor, class_prob: torch.Tensor, padded_size, out_size) -> torch.Tensor:
    """mask_logits (Q, h, w) fp32, class_prob (Q, C) fp32 -> (C, Ho, Wo) fp32 = sum_q p[q, c] * sigmoid(upsample(m_q)), upsampled
    to `padded_size` and cropped to `out_size` without materialising the (Q, H, W) masks."""
    Q, hl, wl = mask_logits.shape
    C = class_prob.shape[1]
    assert mask_logits.dtype == torch.float32 and mask_logits.is_contiguous() and class_prob.shape[0] == Q
    Cp = -(-C // 32) * 32
    P = torch.zeros((Q, Cp), dtype=torch.float32, device=mask_logits.device)
    P[:, :C] = class_prob
    sem = torch.empty((C, out_size[0], out_size[1]), dtype=torch.float32, device=mask_logits.device)
    check(lib.uenc_postproc_semantic(mask_logits.data_ptr(), P.data_ptr(), sem.data_ptr(), Q, C, Cp, hl, wl, padded_size[0], padded_size[1],
                                     out_size[0], out_size[1], stream_ptr()), "postproc_semantic")
    return sem


def postproc_panoptic_stats(mask_logits: torch.Tensor, score: torch.Tensor, padded_size, out_size):
    """-> ids (Ho, Wo) int32 (argmax over queries with score > 0 of score * sigmoid(upsampled mask)), counts (3, Q) int32:
    pixels won, pixels with sigmoid >= 0.5, pixels with both."""
    Q, hl, wl = mask_logits.shape
    assert mask_logits.dtype == torch.float32 and mask_logits.is_contiguous() and score.dtype == torch.float32 and score.numel() == Q
    ids = torch.empty(tuple(out_size), dtype=torch.int32, device=mask_logits.device)
    counts = torch.zeros((3, Q), dtype=torch.int32, device=mask_logits.device)
    check(lib.uenc_postproc_panoptic_stats(mask_logits.data_ptr(), score.contiguous().data_ptr(), ids.data_ptr(), counts.data_ptr(), Q, hl, wl,
                                           padded_size[0], padded_size[1], out_size[0], out_size[1], stream_ptr()), "postproc_panoptic_stats")
    return ids, counts


def postproc_panoptic_label(mask_logits: torch.Tensor, ids: torch.Tensor, segid: torch.Tensor, padded_size) -> torch.Tensor:
    Q, hl, wl = mask_logits.shape
    assert ids.dtype == torch.int32 and segid.dtype == torch.int32 and segid.numel() == Q and ids.is_contiguous()
    seg = torch.empty_like(ids)
    check(lib.uenc_postproc_panoptic_label(mask_logits.data_ptr(), ids.data_ptr(), segid.contiguous().data_ptr(), seg.data_ptr(), Q, hl, wl,
                                           padded_size[0], padded_size[1], ids.shape[0], ids.shape[1], stream_ptr()), "postproc_panoptic_label")
    return seg


def im2col3x3_s2(x16: torch.Tensor) -> torch.Tensor:
    """x (B, H, W, C) bf16 channels-last -> patch matrix (B * ceil(H/2) * ceil(W/2), 9C) bf16 of the 3x3 stride-2 pad-1 convolution."""
    B, H, W, C = x16.shape
    if EXACT and x16.dtype == torch.float32:     # pure data movement: the fp32 map gathered as a bf16 map with twice the channels
        return im2col3x3_s2(x16.contiguous().view(torch.bfloat16)).view(torch.float32)
    assert x16.dtype == torch.bfloat16 and x16.is_contiguous() and C % 8 == 0
    col = torch.empty((B * ((H + 1) // 2) * ((W + 1) // 2), 9 * C), dtype=torch.bfloat16, device=x16.device)
    check(lib.uenc_im2col3x3_s2(x16.data_ptr(), col.data_ptr(), B, H, W, C, stream_ptr()), "im2col3x3_s2")
    return col


def col2im3x3_s2(dcol: torch.Tensor, B: int, H: int, W: int, C: int) -> torch.Tensor:
    """adjoint of im2col3x3_s2: (rows, 9C) bf16 -> (B, H, W, C) fp32."""
    if EXACT and dcol.dtype == torch.float32:   # adjoint of the strided gather as nine shifted fp32 adds (verification mode only)
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        d = dcol.view(B, Ho, Wo, 9, C)
        dxp = dcol.new_zeros((B, 2 * Ho + 2, 2 * Wo + 2, C))
        for t in range(9):
            ky, kx = divmod(t, 3)
            dxp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] += d[:, :, :, t]
        return dxp[:, 1:1 + H, 1:1 + W].contiguous()
    assert dcol.dtype == torch.bfloat16 and dcol.is_contiguous() and dcol.shape[1] == 9 * C
    dx = torch.empty((B, H, W, C), dtype=torch.float32, device=dcol.device)
    check(lib.uenc_col2im3x3_s2(dcol.data_ptr(), dx.data_ptr(), B, H, W, C, stream_ptr()), "col2im3x3_s2")
    return dx


def na2d_fwd(qkv: torch.Tensor, rpb: Optional[torch.Tensor], nH: int, ks: int, dilation: int, scale: float, need_lse: bool = True):
    """Neighbourhood attention on qkv (B, H, W, 3C) bf16 (C = nH * 32) -> out (B, H, W, C) bf16, lse (B, nH, H, W) fp32.
    Exact mode: qkv and out fp32 (uenc_na2d_f32_fwd)."""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    if rpb is not None:
        assert rpb.dtype == torch.float32 and rpb.is_contiguous() and tuple(rpb.shape) == (nH, 2 * ks - 1, 2 * ks - 1)
    if EXACT:
        assert qkv.dtype == torch.float32 and qkv.is_contiguous() and C == nH * 32, "na2d: head_dim must be 32"
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=qkv.device)
        lse = torch.empty((B, nH, H, W), dtype=torch.float32, device=qkv.device) if need_lse else None
        check(lib.uenc_na2d_f32_fwd(qkv.data_ptr(), ptr(rpb), out.data_ptr(), ptr(lse), B, H, W, nH, ks, dilation, float(scale), stream_ptr()),
              "na2d_f32_fwd")
        return out, lse
    assert qkv.dtype == torch.bfloat16 and qkv.is_contiguous() and C == nH * 32, "na2d: head_dim must be 32"
    out = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((B, nH, H, W), dtype=torch.float32, device=qkv.device) if need_lse else None
    check(lib.uenc_na2d_fwd(qkv.data_ptr(), ptr(rpb), out.data_ptr(), ptr(lse), B, H, W, nH, ks, dilation, float(scale), stream_ptr()),
          "na2d_fwd")
    return out, lse


def na2d_bwd(qkv, rpb, out, dout, lse, nH: int, ks: int, dilation: int, scale: float, drpb: Optional[torch.Tensor]):
    """-> dqkv (B, H, W, 3C) bf16; drpb (nH, 2ks-1, 2ks-1) fp32 is accumulated in place when given.  Exact mode: qkv, out, dout
    and dqkv fp32 (uenc_na2d_f32_bwd)."""
    B, H, W, C3 = qkv.shape
    if EXACT:
        assert qkv.dtype == torch.float32 and qkv.is_contiguous() and out.dtype == torch.float32 and out.is_contiguous()
        assert dout.dtype == torch.float32 and dout.is_contiguous() and dout.shape == out.shape
        dqkv = torch.empty_like(qkv)
        check(lib.uenc_na2d_f32_bwd(qkv.data_ptr(), ptr(rpb), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), ptr(drpb),
                                    B, H, W, nH, ks, dilation, float(scale), stream_ptr()), "na2d_f32_bwd")
        return dqkv
    assert dout.dtype == torch.bfloat16 and dout.is_contiguous() and out.is_contiguous() and dout.shape == out.shape
    dqkv = torch.empty_like(qkv)
    ws = _scratch("na2d_delta", B * nH * H * W * 4, qkv.device)
    check(lib.uenc_na2d_bwd(qkv.data_ptr(), ptr(rpb), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), ptr(drpb),
                            ws.data_ptr(), B, H, W, nH, ks, dilation, float(scale), stream_ptr()), "na2d_bwd")
    return dqkv


def patch_merge_ln_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5):
    """x (B, H, W, C) fp32 -> (y (B, ceil(H/2) * ceil(W/2), 4C) bf16, stats): PatchMerging's gather + LayerNorm in one pass."""
    B, H, W, C = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and gamma.numel() == 4 * C
    L2 = ((H + 1) // 2) * ((W + 1) // 2)
    y = torch.empty((B, L2, 4 * C), dtype=torch.bfloat16, device=x.device)
    stats = torch.empty((B * L2, 2), dtype=torch.float32, device=x.device)
    check(lib.uenc_patch_merge_ln_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), stats.data_ptr(), B, H, W, C, float(eps),
                                      stream_ptr()), "patch_merge_ln_fwd")
    return y, stats


def patch_merge_ln_bwd(dy: torch.Tensor, x: torch.Tensor, stats: torch.Tensor, gamma: torch.Tensor, dgamma=None, dbeta=None,
                       defer: Optional["SmallReductions"] = None) -> torch.Tensor:
    B, H, W, C = x.shape
    assert dy.is_contiguous() and dy.shape[-1] == 4 * C
    dx = torch.empty_like(x)
    M = B * ((H + 1) // 2) * ((W + 1) // 2)
    part, deferred = _ln_part(M, 4 * C, dgamma, dbeta, x.device, defer)
    check(lib.uenc_patch_merge_ln_bwd(dy.data_ptr(), dt(dy), x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), dx.data_ptr(), ptr(dgamma),
                                      ptr(dbeta), ptr(part), B, H, W, C, int(deferred), stream_ptr()), "patch_merge_ln_bwd")
    return dx


class SmallReductions:
    """Parameter-gradient reductions that nothing in the backward pass waits for, parked and launched together.

    A LayerNorm backward leaves [blocks][2][C] partial sums of dgamma / dbeta, a window-attention backward dense dS partials of its
    relative-position table; summing them is ~2 us of work in a ~10 / ~19 us launch, ~70 + 24 times per step.  Only the optimiser (and the
    gradient all-reduce) reads the results, so the partials stay in private buffers and ONE grouped launch per kind sums them when the
    queue is flushed (ops.WgradQueue.flush: with the deferred weight-gradient groups, and at the end of every backward pass)."""
    _LN = [("part", "<u8"), ("dgamma", "<u8"), ("dbeta", "<u8"), ("nblk", "<i4"), ("C", "<i4"), ("begin", "<i4"), ("pad", "<i4")]
    _DT = [("wsd", "<u8"), ("dtab", "<u8"), ("G", "<i4"), ("nH", "<i4"), ("ws", "<i4"), ("ntiles", "<i4"), ("begin", "<i4"), ("pad", "<i4")]
    LnSum = collections.namedtuple("LnSum", "part dgamma dbeta nblk C")                  # the records' fields, by the structs' names
    TableSum = collections.namedtuple("TableSum", "wsd dtab G nH ws ntiles")

    CHUNK = 64 << 20          # floats' worth of bytes per arena chunk

    def __init__(self):
        self.ln, self.dt, self.keep = [], [], []
        self._chunks, self._cur, self._off = [], 0, 0        # bump-allocated arena for the parked partials, reused every step

    def alloc(self, nfloats: int, device) -> torch.Tensor:
        """A private fp32 buffer that stays untouched until the next flush.  Bump-allocated from chunks that persist across steps (the
        ~1 GB of partials a backward pass parks would otherwise go through the caching allocator ~140 times per step)."""
        nbytes = (nfloats * 4 + 255) // 256 * 256
        while True:
            if self._cur < len(self._chunks):
                c = self._chunks[self._cur]
                if c.device == device and self._off + nbytes <= c.numel():
                    out = c[self._off:self._off + nfloats * 4].view(torch.float32)
                    self._off += nbytes
                    return out
                self._cur += 1
                self._off = 0
                continue
            self._chunks.append(torch.empty(max(self.CHUNK, nbytes), dtype=torch.uint8, device=device))

    def __bool__(self):
        return bool(self.ln or self.dt)

    def add_ln(self, part, dgamma, dbeta, nblk: int, C: int):
        self.ln.append(self.LnSum(part.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), nblk, C))
        self.keep.append((part, dgamma, dbeta))

    def add_dtable(self, wsd, dtab, G: int, nH: int, ws: int, ntiles: int):
        self.dt.append(self.TableSum(wsd.data_ptr(), dtab.data_ptr(), G, nH, ws, ntiles))
        self.keep.append((wsd, dtab))

    def clear(self):
        self.ln, self.dt, self.keep = [], [], []
        self._cur, self._off = 0, 0           # stream order: whatever is parked next is written after the reductions launched above

    def release(self):
        """Give the arena back to the allocator (a model that goes on to inference only has no use for it).  Buffers parked and not
        yet flushed stay valid: `keep` holds views into their chunks.  The next alloc() starts a fresh chunk."""
        self._chunks, self._cur, self._off = [], 0, 0

    def flush(self):
        dev = self.keep[0][0].device if self.keep else None
        if self.ln:
            tab, blocks = pack_table(self._LN, self.ln, [-(-2 * r.C // 64) for r in self.ln], "begin")
            check(lib.uenc_ln_param_grouped(upload_table(tab, dev).data_ptr(), len(self.ln), blocks, stream_ptr()), "ln_param_grouped")
        if self.dt:
            tab, blocks = pack_table(self._DT, self.dt, [r.nH * r.ntiles for r in self.dt], "begin")
            check(lib.uenc_window_attn_dtable_grouped(upload_table(tab, dev).data_ptr(), len(self.dt), blocks, stream_ptr()),
                  "window_attn_dtable_grouped")
        self.clear()


def _ln_part(M: int, C: int, dgamma, dbeta, device, defer):
    """Scratch for a LayerNorm backward's dgamma / dbeta block partials: the shared buffer (the pass reduces them itself), or -- deferred --
    a private one registered with the queue.  -> (buffer | None, deferred?)"""
    if dgamma is None:
        return None, False
    nblk = int(lib.uenc_layernorm_bwd_blocks(M, C)) if defer is not None else 0
    if nblk > 0:
        part = defer.alloc(nblk * 2 * C, device)
        defer.add_ln(part, dgamma, dbeta, nblk, C)
        return part, True
    return _scratch("ln_bwd", 2048 * 2 * C * 4, device), False


def relpos_expand(table: torch.Tensor, ws: int):
    """relative_position_bias_table ((2ws-1)^2, nH) fp32 -> dense (nH, NP, NP) in query-major and key-major order."""
    assert table.dtype == torch.float32 and table.is_contiguous() and table.shape[0] == (2 * ws - 1) ** 2
    if EXACT:                                   # the fp32 window-attention kernels index the table themselves
        return table, table
    nH = table.shape[1]
    NP = lib.uenc_window_attn_np(ws)
    bq = torch.empty((nH, NP, NP), dtype=torch.float32, device=table.device)
    bk = torch.empty_like(bq)
    check(lib.uenc_relpos_expand(table.data_ptr(), bq.data_ptr(), bk.data_ptr(), nH, ws, stream_ptr()), "relpos_expand")
    return bq, bk


def window_attn_fwd(qkv: torch.Tensor, qkv_bias16: torch.Tensor, bias_q: torch.Tensor, ws: int, shift: int,
                    scale: float, want_lse: bool = False):
    """qkv (B, H, W, 3C) bf16 -> attention output (B, H, W, C) bf16 (before proj).  head_dim is 32.
    want_lse: also return the softmax row statistics (B, H, W, nH) fp32 (max + log2 sum, log2 units) for window_attn_bwd(lse=...)."""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    if EXACT:                                   # qkv / bias fp32, bias_q = the raw relative-position table ((2ws-1)^2, nH)
        assert qkv.dtype == torch.float32 and qkv.is_contiguous() and qkv_bias16.dtype == torch.float32 and qkv_bias16.numel() == C3
        assert bias_q.dtype == torch.float32 and tuple(bias_q.shape) == ((2 * ws - 1) ** 2, C // 32) and bias_q.is_contiguous()
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=qkv.device)
        check(lib.uenc_window_attn_f32_fwd(qkv.data_ptr(), qkv_bias16.data_ptr(), bias_q.data_ptr(), out.data_ptr(), B, H, W, C, C // 32, ws,
                                           shift, float(scale), stream_ptr()), "window_attn_f32_fwd")
        return (out, None) if want_lse else out
    assert qkv.dtype == torch.bfloat16 and qkv.is_contiguous() and qkv_bias16.dtype == torch.bfloat16
    assert qkv_bias16.numel() == C3 and C % 32 == 0 and bias_q.shape[0] == C // 32
    out = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((B, H, W, C // 32), dtype=torch.float32, device=qkv.device) if want_lse else None
    check(lib.uenc_window_attn_fwd(qkv.data_ptr(), qkv_bias16.data_ptr(), bias_q.data_ptr(), out.data_ptr(), lse.data_ptr() if want_lse else 0,
                                   B, H, W, C, C // 32, ws, shift, float(scale), stream_ptr()), "window_attn_fwd")
    return (out, lse) if want_lse else out


_SCRATCH = {}


def _scratch(tag: str, nbytes: int, device) -> torch.Tensor:
    """Kernel-internal scratch kept across calls: one buffer per (purpose, device), grown on demand.  Launches on one
    stream are ordered, so a buffer can be reused by the next call as soon as this one is enqueued."""
    key = (tag, str(device))
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        _SCRATCH[key] = buf
    return buf


def window_attn_bwd(qkv, qkv_bias16, bias_q, bias_k, o_saved, d_out, ws: int, shift: int, scale: float,
                    dtable: Optional[torch.Tensor] = None, dbias: Optional[torch.Tensor] = None, defer: Optional[SmallReductions] = None,
                    lse: Optional[torch.Tensor] = None):
    """-> dqkv (B,H,W,3C).  The two parameter gradients are ACCUMULATED by the kernels into `dtable` ((2ws-1)^2, nH) fp32 -- the
    relative-position table's .grad -- and `dbias` (3C) fp32 -- the share of qkv.bias.grad that flows through padding slots; when
    a buffer is not given (no training) the contribution goes to scratch."""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    nH = C // 32
    TT = (2 * ws - 1) ** 2
    if dtable is None:
        dtable = _scratch("wattn_dtab", TT * nH * 4, qkv.device).view(torch.float32)[:TT * nH].view(TT, nH)
    if dbias is None:
        dbias = _scratch("wattn_dpad", 3 * C * 4, qkv.device).view(torch.float32)[:3 * C]
    assert dtable.dtype == torch.float32 and dtable.is_contiguous() and tuple(dtable.shape) == (TT, nH)
    assert dbias.dtype == torch.float32 and dbias.is_contiguous() and dbias.numel() == 3 * C
    if EXACT:
        assert qkv.dtype == torch.float32 and d_out.dtype == torch.float32 and d_out.is_contiguous() and d_out.shape == (B, H, W, C)
        dqkv = torch.empty_like(qkv)
        check(lib.uenc_window_attn_f32_bwd(qkv.data_ptr(), qkv_bias16.data_ptr(), bias_q.data_ptr(), d_out.data_ptr(), dqkv.data_ptr(),
                                           dtable.data_ptr(), dbias.data_ptr(), B, H, W, C, nH, ws, shift, float(scale), stream_ptr()),
              "window_attn_f32_bwd")
        return dqkv
    assert d_out.dtype == torch.bfloat16 and d_out.is_contiguous() and d_out.shape == (B, H, W, C)
    assert o_saved.dtype == torch.bfloat16 and o_saved.is_contiguous()
    dqkv = torch.empty_like(qkv)
    nws = int(lib.uenc_window_attn_bwd_ws_floats(B, H, W, nH, ws))
    if defer is not None:                                                # the table gradient is reduced by the queue's grouped launch
        wsbuf = defer.alloc(nws, qkv.device)
        defer.add_dtable(wsbuf, dtable, int(lib.uenc_window_attn_bwd_groups(B, H, W, nH, ws)), nH, ws, int(lib.uenc_window_attn_np(ws)) // 16)
    else:
        wsbuf = _scratch("wattn_dS", nws * 4, qkv.device)                # dense dS partials (internal)
    if lse is not None:
        assert lse.dtype == torch.float32 and lse.is_contiguous() and tuple(lse.shape) == (B, H, W, nH)
    check(lib.uenc_window_attn_bwd(qkv.data_ptr(), qkv_bias16.data_ptr(), bias_q.data_ptr(), bias_k.data_ptr(),
                                   o_saved.data_ptr(), lse.data_ptr() if lse is not None else 0, d_out.data_ptr(), dqkv.data_ptr(), wsbuf.data_ptr(),
                                   dtable.data_ptr(), dbias.data_ptr(),
                                   B, H, W, C, nH, ws, shift, float(scale), int(defer is not None), stream_ptr()), "window_attn_bwd")
    return dqkv


def msdeform_tiled_eligible(value, shapes_host, Lq: int, L: int, P: int) -> bool:
    """Geometry of the deformable encoder (queries = the pixels of the L maps): the LDS-tiled forward applies."""
    if shapes_host is None or os.environ.get("UENC_MSDA_TILED", "1") == "0":
        return False
    B, S, M, D = value.shape
    return (D == 32 and value.dtype == torch.bfloat16 and L <= 4 and L * P <= 16 and Lq == S and B * M < 65536
            and sum(int(h) * int(w) for h, w in shapes_host) == S)


def msdeform_fused_tiled_eligible(value, offaw, shapes_host, Lq: int, L: int, P: int) -> bool:
    """The LDS-tiled FUSED forward applies: the encoder's geometry, P == 4 and 16-byte aligned projection rows.  The one place that decides
    it: msdeform_attn_fused_fwd launches by it and DeformEncoderLayerFn chooses its forward by it."""
    return P == 4 and offaw.stride(0) % 4 == 0 and offaw.data_ptr() % 16 == 0 and msdeform_tiled_eligible(value, shapes_host, Lq, L, P)


def _shapes_c(shapes_host, L: int):
    """[(H, W), ...] -> the int64[2 L] array the C entry points take as `shapes_host`."""
    flat = [int(v) for hw in shapes_host for v in hw]
    assert len(flat) == 2 * L
    return (ctypes.c_int64 * len(flat))(*flat)


def msdeform_attn_fwd(value, shapes, level_start, loc, attn, out_dtype=torch.float32, shapes_host=None):
    """value (B,S,M,D) fp32|bf16, shapes (L,2) int64, level_start (L) int64, loc (B,Lq,M,L,P,2), attn (B,Lq,M,L,P)
    -> (B, Lq, M*D).  Same tensor contract as the reference's ms_deform_attn_forward.  shapes_host: optional [(H, W), ...] host copy
    of `shapes`; with it the encoder's geometry (Lq == S) takes the LDS-tiled kernel (same result)."""
    B, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    for t in (value, shapes, level_start, loc, attn):
        if not (t.is_cuda and t.is_contiguous()):
            raise capi.UencError("msdeform_attn: tensors must be contiguous CUDA tensors")
    assert shapes.dtype == torch.int64 and level_start.dtype == torch.int64
    assert loc.dtype == torch.float32 and attn.dtype == torch.float32 and attn.shape == (B, Lq, M, L, P)
    out = torch.empty((B, Lq, M * D), dtype=_odt(out_dtype), device=value.device)
    if msdeform_tiled_eligible(value, shapes_host, Lq, L, P):
        check(lib.uenc_msdeform_attn_fwd_tiled(value.data_ptr(), dt(value), shapes.data_ptr(), level_start.data_ptr(), loc.data_ptr(),
                                               attn.data_ptr(), out.data_ptr(), dt(out), B, S, M, D, L, Lq, P, _shapes_c(shapes_host, L), stream_ptr()),
              "msdeform_attn_fwd_tiled")
        return out
    check(lib.uenc_msdeform_attn_fwd(value.data_ptr(), dt(value), shapes.data_ptr(), level_start.data_ptr(), loc.data_ptr(),
                                     attn.data_ptr(), out.data_ptr(), dt(out), B, S, M, D, L, Lq, P, stream_ptr()),
          "msdeform_attn_fwd")
    return out


def msdeform_attn_bwd(value, shapes, level_start, loc, attn, grad_out, shapes_host=None):
    """-> grad_value (fp32, B,S,M,D), grad_loc, grad_attn (the reference's ms_deform_attn_backward contract).

    shapes_host: optional [(H, W), ...] host copy of `shapes`; enables the binned (on-chip summed) grad_value path."""
    B, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    assert grad_out.is_contiguous() and grad_out.shape == (B, Lq, M * D)
    gv = torch.zeros((B, S, M, D), dtype=torch.float32, device=value.device)
    gl = torch.empty_like(loc)
    ga = torch.empty_like(attn)
    sh, ws, ws_bytes = None, None, 0
    if shapes_host is not None:
        sh, ws_bytes = _msda_host_plan(shapes_host, B, M, D, L, Lq, P)
        if ws_bytes > 0:
            ws = _scratch("msda_bins", ws_bytes, value.device)
    check(lib.uenc_msdeform_attn_bwd(value.data_ptr(), dt(value), shapes.data_ptr(), level_start.data_ptr(), loc.data_ptr(),
                                     attn.data_ptr(), grad_out.data_ptr(), dt(grad_out), gv.data_ptr(), gl.data_ptr(),
                                     ga.data_ptr(), B, S, M, D, L, Lq, P, sh, ws.data_ptr() if ws is not None else None,
                                     ws_bytes, stream_ptr()), "msdeform_attn_bwd")
    return gv, gl, ga


def _msda_host_plan(shapes_host, B, M, D, L, Lq, P):
    """-> (shapes_host for C, bytes of scratch the binned backward needs: bin counters + records; 0 = no binned plan for the shape)."""
    sh = _shapes_c(shapes_host, L)
    return sh, int(lib.uenc_msdeform_attn_bwd_workspace_bytes(sh, B, M, D, L, Lq, P))


def msdeform_fused_available(shapes_host, B, M, D, L, Lq, P) -> bool:
    """The fused forward / backward pair (locations and weights derived inside the kernels) needs D = 32, L * P <= 16 and the binned
    backward's plan; never in the fp32 verification mode (its reference path stays module by module)."""
    return (not EXACT) and D == 32 and L * P <= 16 and shapes_host is not None and _msda_host_plan(shapes_host, B, M, D, L, Lq, P)[1] > 0


def msdeform_attn_fused_fwd(value, shapes, level_start, offaw, ref, L: int, P: int, out_dtype=torch.bfloat16, shapes_host=None):
    """value (B, S, M, D), offaw (B * Lq, ld) fp32 = [M][L][P][2] offsets | [M][L * P] logits, ref (B | 1, Lq, L, 2) -> (B, Lq, M * D).
    shapes_host: optional host copy of `shapes`; with it the encoder's geometry (Lq == S, P == 4) takes the LDS-tiled kernel (same result)."""
    B, S, M, D = value.shape
    Lq = ref.shape[1]
    assert offaw.dtype == torch.float32 and offaw.stride(1) == 1 and offaw.shape[0] == B * Lq and ref.dtype == torch.float32 and ref.is_contiguous()
    out = torch.empty((B, Lq, M * D), dtype=_odt(out_dtype), device=value.device)
    if msdeform_fused_tiled_eligible(value, offaw, shapes_host, Lq, L, P):
        check(lib.uenc_msdeform_attn_fused_fwd_tiled(value.data_ptr(), dt(value), shapes.data_ptr(), level_start.data_ptr(), offaw.data_ptr(), offaw.stride(0),
                                                     ref.data_ptr(), int(ref.shape[0] != 1), out.data_ptr(), dt(out), B, S, M, D, L, Lq, P, _shapes_c(shapes_host, L),
                                                     stream_ptr()), "msdeform_attn_fused_fwd_tiled")
        return out
    check(lib.uenc_msdeform_attn_fused_fwd(value.data_ptr(), dt(value), shapes.data_ptr(), level_start.data_ptr(), offaw.data_ptr(), offaw.stride(0),
                                           ref.data_ptr(), int(ref.shape[0] != 1), out.data_ptr(), dt(out), B, S, M, D, L, Lq, P, stream_ptr()),
          "msdeform_attn_fused_fwd")
    return out


def msdeform_attn_fused_bwd(value, shapes, level_start, offaw, ref, L: int, P: int, grad_out, shapes_host):
    """-> grad_value (fp32, B, S, M, D), d(offaw) (B * Lq, 3 M L P) bf16."""
    B, S, M, D = value.shape
    Lq = ref.shape[1]
    assert grad_out.is_contiguous() and grad_out.shape == (B, Lq, M * D)
    sh, ws_bytes = _msda_host_plan(shapes_host, B, M, D, L, Lq, P)
    assert ws_bytes > 0
    ws = _scratch("msda_bins", ws_bytes, value.device)
    gv = torch.zeros((B, S, M, D), dtype=torch.float32, device=value.device)
    ncol = 3 * M * L * P
    doffaw = torch.empty((B * Lq, ncol), dtype=torch.bfloat16, device=value.device)
    check(lib.uenc_msdeform_attn_fused_bwd(value.data_ptr(), dt(value), shapes.data_ptr(), level_start.data_ptr(), offaw.data_ptr(), offaw.stride(0),
                                           ref.data_ptr(), int(ref.shape[0] != 1), grad_out.data_ptr(), dt(grad_out), gv.data_ptr(), doffaw.data_ptr(), doffaw.stride(0),
                                           B, S, M, D, L, Lq, P, sh, ws.data_ptr(), ws_bytes, stream_ptr()), "msdeform_attn_fused_bwd")
    return gv, doffaw


def attn_mask(logits: torch.Tensor, size) -> torch.Tensor:
    """(B, Q, Hi, Wi) fp32 mask logits -> (B, Q, Ho*Wo) bool, True = blocked; fully blocked rows are cleared."""
    B, Q, Hi, Wi = logits.shape
    Ho, Wo = int(size[0]), int(size[1])
    assert logits.dtype == torch.float32 and logits.is_cuda and logits.is_contiguous()
    out = torch.empty((B, Q, Ho * Wo), dtype=torch.bool, device=logits.device)
    check(lib.uenc_attn_mask(logits.data_ptr(), out.data_ptr(), B * Q, Hi, Wi, Ho, Wo, stream_ptr()), "attn_mask")
    return out


def upsample_bilinear(x: torch.Tensor, size) -> torch.Tensor:
    """(N, C, Hi, Wi) fp32 -> (N, C, Ho, Wo), bilinear, align_corners=False (forward only; Wo % 4 == 0)."""
    N, C, Hi, Wi = x.shape
    Ho, Wo = int(size[0]), int(size[1])
    assert x.dtype == torch.float32 and x.is_cuda and Wo % 4 == 0
    x = x.contiguous()
    out = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=x.device)
    check(lib.uenc_upsample_bilinear(x.data_ptr(), out.data_ptr(), N * C, Hi, Wi, Ho, Wo, stream_ptr()), "upsample_bilinear")
    return out


# --------------------------------------------------------------------------------------------
# FPN branch on token matrices
# --------------------------------------------------------------------------------------------
def groupnorm_tokens_fwd(x, gamma, beta, G: int, eps: float, *, relu=False, add_src=None, add_hw=None, out_dtype=torch.float32):
    """x (B, HW, C) fp32|bf16 -> (y (B, HW, C) out_dtype, stats (B, G, 2)).  add_src: fp32 (B, Hs, Ws, C) merged in by
    bilinear resize to add_hw = (H, W)."""
    B, HW, C = x.shape
    assert x.is_cuda and x.is_contiguous() and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    y = torch.empty((B, HW, C), dtype=_odt(out_dtype), device=x.device)
    stats = torch.empty((B, G, 2), dtype=torch.float32, device=x.device)
    scratch = _scratch("gn", int(lib.uenc_groupnorm_tokens_scratch_bytes(B, HW, C, G)), x.device)
    Hs = Ws = H = W = 0
    if add_src is not None:
        assert add_src.dtype == torch.float32 and add_src.is_contiguous() and add_src.shape[0] == B and add_src.shape[3] == C
        Hs, Ws = add_src.shape[1], add_src.shape[2]
        H, W = add_hw
    check(lib.uenc_groupnorm_tokens_fwd(x.data_ptr(), dt(x), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), dt(y), stats.data_ptr(),
                                        scratch.data_ptr(), ptr(add_src), Hs, Ws, H, W, B, HW, C, G, float(eps), int(relu),
                                        stream_ptr()), "groupnorm_tokens_fwd")
    return y, stats


def groupnorm_tokens_bwd(dy, x, gamma, beta, stats, G: int, *, relu=False, dgamma=None, dbeta=None, dx_dtype=torch.bfloat16):
    B, HW, C = x.shape
    assert dy.is_contiguous() and dy.shape == x.shape and x.is_contiguous()
    dx = torch.empty((B, HW, C), dtype=_odt(dx_dtype), device=x.device)
    scratch = _scratch("gn", int(lib.uenc_groupnorm_tokens_scratch_bytes(B, HW, C, G)), x.device)
    check(lib.uenc_groupnorm_tokens_bwd(dy.data_ptr(), dt(dy), x.data_ptr(), dt(x), gamma.data_ptr(), beta.data_ptr(), stats.data_ptr(),
                                        dx.data_ptr(), dt(dx), ptr(dgamma), ptr(dbeta), scratch.data_ptr(), B, HW, C, G, int(relu),
                                        stream_ptr()), "groupnorm_tokens_bwd")
    return dx


def upsample_bilinear_tokens_bwd(dy, Hs: int, Ws: int):
    """dy (B, H, W, C) fp32|bf16 -> (B, Hs, Ws, C) fp32: adjoint of the align_corners=False bilinear resize (Hs, Ws) -> (H, W)."""
    B, H, W, C = dy.shape
    assert dy.is_contiguous()
    out = torch.empty((B, Hs, Ws, C), dtype=torch.float32, device=dy.device)
    check(lib.uenc_upsample_bilinear_tokens_bwd(dy.data_ptr(), dt(dy), out.data_ptr(), B, H, W, Hs, Ws, C, stream_ptr()),
          "upsample_bilinear_tokens_bwd")
    return out


def merge_nearest_tokens_fwd(a, prev, hw, out_dtype=torch.float32):
    """a (B, H*W, C) + nearest-resized prev (B, Hs, Ws, C) -> (B, H*W, C) out_dtype; fp32|bf16 operands, the sum in fp32."""
    B, HW, C = a.shape
    H, W = hw
    assert a.is_cuda and a.is_contiguous() and prev.is_contiguous() and HW == H * W and prev.shape[0] == B and prev.shape[3] == C
    out = torch.empty((B, HW, C), dtype=_odt(out_dtype), device=a.device)
    check(lib.uenc_merge_nearest_tokens_fwd(a.data_ptr(), dt(a), prev.data_ptr(), dt(prev), out.data_ptr(), dt(out), B, H, W,
                                            prev.shape[1], prev.shape[2], C, stream_ptr()), "merge_nearest_tokens_fwd")
    return out


def merge_nearest_tokens_bwd(dy, Hs: int, Ws: int):
    """dy (B, H, W, C) fp32|bf16 -> (B, Hs, Ws, C) fp32: adjoint of the nearest resize (Hs, Ws) -> (H, W)."""
    B, H, W, C = dy.shape
    assert dy.is_contiguous()
    out = torch.empty((B, Hs, Ws, C), dtype=torch.float32, device=dy.device)
    check(lib.uenc_merge_nearest_tokens_bwd(dy.data_ptr(), dt(dy), out.data_ptr(), B, H, W, Hs, Ws, C, stream_ptr()),
          "merge_nearest_tokens_bwd")
    return out


def im2col3x3(x16):
    """(B, H, W, C) bf16 -> (B*H*W, 9*C) bf16 patch matrix, column order (ky, kx, c)."""
    B, H, W, C = x16.shape
    if EXACT and x16.dtype == torch.float32:
        # pure data movement: gather the fp32 map as a bf16 map with twice the channels (same bytes, same (ky, kx, c) column order)
        return im2col3x3(x16.contiguous().view(torch.bfloat16)).view(torch.float32)
    assert x16.dtype == torch.bfloat16 and x16.is_contiguous()
    col = torch.empty((B * H * W, 9 * C), dtype=torch.bfloat16, device=x16.device)
    check(lib.uenc_im2col3x3(x16.data_ptr(), col.data_ptr(), B, H, W, C, stream_ptr()), "im2col3x3")
    return col


def col2im3x3(dcol, B: int, H: int, W: int, C: int):
    if EXACT and dcol.dtype == torch.float32:   # adjoint of the gather as nine shifted fp32 adds (verification mode only)
        d = dcol.view(B, H, W, 9, C)
        dxp = dcol.new_zeros((B, H + 2, W + 2, C))
        for t in range(9):
            ky, kx = divmod(t, 3)
            dxp[:, ky:ky + H, kx:kx + W] += d[:, :, :, t]
        return dxp[:, 1:1 + H, 1:1 + W].contiguous()
    assert dcol.dtype == torch.bfloat16 and dcol.is_contiguous() and dcol.numel() == B * H * W * 9 * C
    dx = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=dcol.device)
    check(lib.uenc_col2im3x3(dcol.data_ptr(), dx.data_ptr(), B, H, W, C, stream_ptr()), "col2im3x3")
    return dx


# --------------------------------------------------------------------------------------------
# deformable encoder layer glue
# --------------------------------------------------------------------------------------------
def add_cast_bf16(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """bf16(a + b); b may be one period of a (e.g. (S, C) against (B, S, C))."""
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous()
    if EXACT:
        return (a.view(-1, b.numel()) + b.view(1, -1)).view(a.shape)
    out = torch.empty(a.shape, dtype=torch.bfloat16, device=a.device)
    check(lib.uenc_add_cast_bf16(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), b.numel(), stream_ptr()), "add_cast_bf16")
    return out


def msda_prep_fwd(offaw: torch.Tensor, ref: torch.Tensor, shapes: torch.Tensor, B: int, Lq: int, M: int, L: int, P: int):
    """offaw (B*Lq, >= 3*M*L*P) fp32 -> loc (B, Lq, M, L, P, 2), aw (B, Lq, M, L, P) (softmaxed)."""
    assert offaw.dtype == torch.float32 and offaw.stride(1) == 1 and ref.dtype == torch.float32 and ref.is_contiguous()
    loc = torch.empty((B, Lq, M, L, P, 2), dtype=torch.float32, device=offaw.device)
    aw = torch.empty((B, Lq, M, L, P), dtype=torch.float32, device=offaw.device)
    check(lib.uenc_msda_prep_fwd(offaw.data_ptr(), offaw.stride(0), ref.data_ptr(), int(ref.shape[0] != 1), shapes.data_ptr(),
                                 loc.data_ptr(), aw.data_ptr(), B * Lq, Lq, M, L, P, stream_ptr()), "msda_prep_fwd")
    return loc, aw


def msda_prep_bwd(dloc, daw, aw, shapes, ncols: int):
    """-> d(offaw) (B*Lq, ncols) bf16."""
    B, Lq, M, L, P, _ = dloc.shape
    assert dloc.is_contiguous() and daw.is_contiguous() and aw.is_contiguous() and ncols == 3 * M * L * P
    if EXACT:   # fp32 result: d(offset) = d(loc) / (W_l, H_l); d(logit) = aw * (d(aw) - sum_{l,p} aw * d(aw))   (elementwise glue)
        norm = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(torch.float32).view(1, 1, 1, L, 1, 2)
        doff = (dloc / norm).reshape(B * Lq, 2 * M * L * P)
        a, g = aw.view(B * Lq, M, L * P), daw.view(B * Lq, M, L * P)
        dlog = (a * (g - (a * g).sum(-1, keepdim=True))).reshape(B * Lq, M * L * P)
        return torch.cat([doff, dlog], 1).contiguous()
    out = torch.empty((B * Lq, ncols), dtype=torch.bfloat16, device=dloc.device)
    check(lib.uenc_msda_prep_bwd(dloc.data_ptr(), daw.data_ptr(), aw.data_ptr(), shapes.data_ptr(), out.data_ptr(), ncols, B * Lq, Lq,
                                 M, L, P, stream_ptr()), "msda_prep_bwd")
    return out


def segment_colsum(x16: torch.Tensor, seg_start: torch.Tensor, rows_per_image: int, images: int) -> torch.Tensor:
    """x16 (images * rows_per_image, cols) bf16 -> (nseg, cols) fp32 sums over the row segments of every image."""
    if EXACT:
        st = seg_start.tolist() + [rows_per_image]
        xv = x16.view(images, rows_per_image, -1)
        return torch.stack([xv[:, st[i]:st[i + 1]].sum((0, 1)) for i in range(len(st) - 1)])
    assert x16.dtype == torch.bfloat16 and x16.stride(1) == 1 and seg_start.dtype == torch.int64
    nseg, cols = seg_start.numel(), x16.shape[1]
    out = torch.empty((nseg, 128, cols), dtype=torch.float32, device=x16.device)          # 128 stored block partials per segment
    check(lib.uenc_segment_colsum(x16.data_ptr(), x16.stride(0), cols, seg_start.data_ptr(), nseg, rows_per_image, images, out.data_ptr(),
                                  stream_ptr()), "segment_colsum")
    return out.sum(1)


# ---- bipartite matching (csrc/matcher.hip) ------------------------------------------------------------------------------------------
LSAP_MAX = 256                  # LSAP_MAX_N of csrc/matcher.hip: most queries / targets of one problem


def _match_dtypes():
    mp = np.dtype([("logits", "<u8"), ("masks", "<u8"), ("points", "<u8"), ("gt", "<u8"), ("labels", "<u8"), ("T", "<i4"), ("pad", "<i4")])
    lp = np.dtype([("cost", "<u8"), ("row_ind", "<u8"), ("col_ind", "<u8"), ("T", "<i4"), ("ld", "<i4")])
    assert mp.itemsize == 48 and lp.itemsize == 32
    return mp, lp


def _dev(t, name: str, dtype, ndim: int):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise capi.UencError(f"{name} must live on the GPU")
    if t.dtype != dtype or t.dim() != ndim or not t.is_contiguous():
        raise capi.UencError(f"{name} must be contiguous {dtype} with {ndim} dimensions, got {t.dtype} {tuple(t.shape)} / {t.stride()}")
    return t


def match_cost(problems, w_class: float, w_mask: float, w_dice: float, nan_fill: float = 100.0) -> torch.Tensor:
    """problems = [(logits (Q, C1) f32, masks (Q, h, w) f32, points (P, 2) f32, gt (T, Hg, Wg) uint8, labels (T) int64), ...], all on one
    GPU, same Q / C1 / h / w / P / Hg / Wg, any T per problem -> cost (n_prob, Q, Tmax) fp32 with Tmax = max(1, max T); columns >= a
    problem's T are zero.  One call of uenc_match_cost; the descriptors travel in the kernel arguments."""
    mp, _ = _match_dtypes()
    n = len(problems)
    if n == 0:
        raise capi.UencError("match_cost: no problems")
    lg0, mk0, pt0 = problems[0][:3]
    _dev(lg0, "logits", torch.float32, 2); _dev(mk0, "masks", torch.float32, 3); _dev(pt0, "points", torch.float32, 2)
    Q, C1 = lg0.shape
    h, w = mk0.shape[1:]
    P = pt0.shape[0]
    Ts = [int(pr[3].shape[0]) for pr in problems]
    Tmax = max(1, max(Ts))
    Hg = Wg = 1
    for pr in problems:
        if pr[3].shape[0]:
            Hg, Wg = int(pr[3].shape[1]), int(pr[3].shape[2])
            break
    rows = np.zeros(n, dtype=mp)
    for i, (lg, mk, pt, gt, lab) in enumerate(problems):
        _dev(lg, "logits", torch.float32, 2); _dev(mk, "masks", torch.float32, 3); _dev(pt, "points", torch.float32, 2)
        if tuple(lg.shape) != (Q, C1) or tuple(mk.shape) != (Q, h, w) or tuple(pt.shape) != (P, 2):
            raise capi.UencError("match_cost: every problem of one call must have the same Q, C + 1, h, w and P")
        if Ts[i]:
            _dev(gt, "target masks", torch.uint8, 3); _dev(lab, "labels", torch.int64, 1)
            if tuple(gt.shape[1:]) != (Hg, Wg) or lab.shape[0] != Ts[i]:
                raise capi.UencError("match_cost: target masks must share one (padded) size and come with one label each")
        rows[i] = (lg.data_ptr(), mk.data_ptr(), pt.data_ptr(), gt.data_ptr() if Ts[i] else 0, lab.data_ptr() if Ts[i] else 0, Ts[i], 0)
    nws = lib.uenc_match_cost_workspace_floats(n, Q, Tmax, P)
    if nws < 0:
        raise capi.UencError(f"match_cost: Q = {Q} / T = {Tmax} beyond the limit of {LSAP_MAX}, or no points")
    cost = torch.empty((n, Q, Tmax), dtype=torch.float32, device=lg0.device)
    ws = torch.empty(nws, dtype=torch.float32, device=lg0.device)
    check(lib.uenc_match_cost(rows.ctypes.data, n, Q, C1, h, w, Hg, Wg, P, Tmax, w_class, w_mask, w_dice, nan_fill, ws.data_ptr(), nws,
                              cost.data_ptr(), stream_ptr()), "match_cost")
    return cost


def lsap_solve(cost: torch.Tensor, Ts):
    """cost (n_prob, Q, ld) fp32 on the GPU, problem p being cost[p, :, :Ts[p]] -> (row_ind, col_ind, offsets): two flat int64 device buffers
    holding min(Q, Ts[p]) pairs per problem from offsets[p] on (scipy's convention: row_ind ascending).  One call of uenc_lsap_solve, no
    synchronisation; the offsets are host integers because the shapes are."""
    _, lp = _match_dtypes()
    _dev(cost, "cost", torch.float32, 3)
    n, Q, ld = cost.shape
    Ts = [int(t) for t in Ts]
    if len(Ts) != n or n == 0:
        raise capi.UencError("lsap_solve: one T per problem")
    if Q < 1 or Q > LSAP_MAX or any(t < 0 or t > LSAP_MAX or t > ld for t in Ts):
        raise capi.UencError(f"lsap_solve: 1 <= Q <= {LSAP_MAX} and 0 <= T <= min({LSAP_MAX}, row stride) are required, got Q = {Q}, T = {Ts}")
    offs = [0]
    for t in Ts:
        offs.append(offs[-1] + min(Q, t))
    out = torch.empty((2, max(offs[-1], 1)), dtype=torch.int64, device=cost.device)
    rows = np.zeros(n, dtype=lp)
    base, rp, cp = cost.data_ptr(), out[0].data_ptr(), out[1].data_ptr()
    for i, t in enumerate(Ts):
        rows[i] = (base + 4 * i * Q * ld, rp + 8 * offs[i], cp + 8 * offs[i], t, ld)
    check(lib.uenc_lsap_solve(rows.ctypes.data, n, Q, stream_ptr()), "lsap_solve")
    return out[0], out[1], offs


# ---- set criterion (csrc/criterion.hip) ---------------------------------------------------------------------------------------------------
CRIT_MAX_HEADS, CRIT_MAX_IMAGES = 16, 32        # of csrc/criterion.hip: heads and images of one call


class CritCall:
    """The shapes and the 1024-byte descriptor (struct CritDesc) the four uenc_crit_* entry points of one criterion call share.
    masks: per head (bs, Q, h, w) f32 or None; logits: per head (bs, Q, C1) f32 or None; gts: per image (T, Hg, Wg) uint8; labels: per image
    (T) int64.  Row r = head * N + n of every buffer is pair n of that head, N = sum_b min(Q, T_b)."""

    def __init__(self, masks, logits, gts, labels):
        first = masks[0] if masks[0] is not None else logits[0]
        self.n_heads, self.bs, self.Q = len(masks), int(first.shape[0]), int(first.shape[1])
        if not (1 <= self.n_heads <= CRIT_MAX_HEADS and 1 <= self.bs <= CRIT_MAX_IMAGES and len(logits) == self.n_heads and len(gts) == len(labels) == self.bs):
            raise capi.UencError(f"criterion: at most {CRIT_MAX_HEADS} heads and {CRIT_MAX_IMAGES} images per call, one target entry per image")
        self.h = self.w = self.C1 = 0
        for mk, lg in zip(masks, logits):
            if mk is not None:
                _dev(mk, "pred_masks", torch.float32, 4)
                self.h, self.w = int(mk.shape[2]), int(mk.shape[3])
                if tuple(mk.shape) != (self.bs, self.Q, self.h, self.w) or tuple(mk.shape) != tuple(masks[0].shape):
                    raise capi.UencError("criterion: every head's pred_masks must have one shape")
            if lg is not None:
                _dev(lg, "pred_logits", torch.float32, 3)
                self.C1 = int(lg.shape[2])
                if tuple(lg.shape) != (self.bs, self.Q, self.C1) or tuple(lg.shape) != tuple(logits[0].shape):
                    raise capi.UencError("criterion: every head's pred_logits must have one shape")
        self.Ts = [int(g.shape[0]) for g in gts]
        self.Hg = self.Wg = 1
        desc = np.zeros(1, dtype=np.dtype([("head", [("masks", "<u8"), ("logits", "<u8")], CRIT_MAX_HEADS),
                                           ("img", [("gt", "<u8"), ("labels", "<u8"), ("T", "<i4"), ("pair0", "<i4")], CRIT_MAX_IMAGES)]))
        assert desc.itemsize == 1024
        for i, (mk, lg) in enumerate(zip(masks, logits)):
            desc["head"][0, i] = (ptr(mk), ptr(lg))
        pairs = 0
        for b, (gt, lab) in enumerate(zip(gts, labels)):
            T = self.Ts[b]
            if T:
                _dev(gt, "target masks", torch.uint8, 3); _dev(lab, "labels", torch.int64, 1)
                if pairs == 0:                          # the first image with targets sets the size
                    self.Hg, self.Wg = int(gt.shape[1]), int(gt.shape[2])
                if tuple(gt.shape[1:]) != (self.Hg, self.Wg) or lab.shape[0] != T:
                    raise capi.UencError("criterion: target masks must share one (padded) size and come with one label each")
            desc["img"][0, b] = (gt.data_ptr() if T else 0, lab.data_ptr() if T else 0, T, pairs)
            pairs += min(self.Q, T)
        self.N, self.desc, self.device = pairs, desc, first.device
        self._keep = (masks, logits, gts, labels)       # the descriptor holds raw pointers

    def _rows(self, t, name, dtype, tail):
        _dev(t, name, dtype, 1 + len(tail))
        if tuple(t.shape) != (self.n_heads * self.N,) + tuple(tail):
            raise capi.UencError(f"criterion: {name} must be {(self.n_heads * self.N,) + tuple(tail)}, got {tuple(t.shape)}")
        return t


def crit_point_logits(call: CritCall, row_ind, points):
    """points (heads * N, M, 2) -> (heads * N, M): every pair's predicted logit map at its M points (uenc_crit_point_logits)."""
    M = int(points.shape[1])
    call._rows(row_ind, "row_ind", torch.int64, ()); call._rows(points, "points", torch.float32, (M, 2))
    out = torch.empty((call.n_heads * call.N, M), dtype=torch.float32, device=call.device)
    check(lib.uenc_crit_point_logits(call.desc.ctypes.data, call.n_heads, call.bs, call.Q, call.h, call.w, call.N, M, row_ind.data_ptr(),
                                     points.data_ptr(), out.data_ptr(), stream_ptr()), "crit_point_logits")
    return out


def crit_mask_loss_fwd(call: CritCall, row_ind, col_ind, points, need_grad: bool = True):
    """points (heads * N, P, 2) -> loss (heads * N, 2) = ce_n, dice_n; sums (heads * N, 3) = sum s t, sum s, sum t; and, for the backward,
    unit (heads * N, P, 2) and keys (heads * N, 4 P) int32 (None, None without need_grad).  uenc_crit_mask_loss_fwd."""
    P, R = int(points.shape[1]), call.n_heads * call.N
    call._rows(row_ind, "row_ind", torch.int64, ()); call._rows(col_ind, "col_ind", torch.int64, ()); call._rows(points, "points", torch.float32, (P, 2))
    loss = torch.empty((R, 2), dtype=torch.float32, device=call.device)
    sums = torch.empty((R, 3), dtype=torch.float32, device=call.device)
    unit = torch.empty((R, P, 2), dtype=torch.float32, device=call.device) if need_grad else None
    keys = torch.empty((R, 4 * P), dtype=torch.int32, device=call.device) if need_grad else None
    check(lib.uenc_crit_mask_loss_fwd(call.desc.ctypes.data, call.n_heads, call.bs, call.Q, call.h, call.w, call.Hg, call.Wg, call.N, P,
                                      row_ind.data_ptr(), col_ind.data_ptr(), points.data_ptr(), loss.data_ptr(), sums.data_ptr(), ptr(unit),
                                      ptr(keys), stream_ptr()), "crit_mask_loss_fwd")
    return loss, sums, unit, keys


def crit_mask_loss_bwd(call: CritCall, row_ind, points, unit, sorted_keys, order, gce, gdice, inv_num_masks: float):
    """-> (heads, bs, Q, h, w): the gradient of every head's mask logits from the per-head upstream gradients gce / gdice (heads) of the summed
    ce_n / dice_n times inv_num_masks.  sorted_keys / order: the stable sort of the forward's keys along dim 1.  uenc_crit_mask_loss_bwd."""
    P = int(points.shape[1])
    call._rows(row_ind, "row_ind", torch.int64, ()); call._rows(points, "points", torch.float32, (P, 2)); call._rows(unit, "unit", torch.float32, (P, 2))
    call._rows(sorted_keys, "sorted_keys", torch.int32, (4 * P,)); call._rows(order, "order", torch.int64, (4 * P,))
    for g in (gce, gdice):
        _dev(g, "upstream gradient", torch.float32, 1)
        if g.shape[0] != call.n_heads:
            raise capi.UencError("criterion: one upstream gradient per head")
    gmasks = torch.zeros((call.n_heads, call.bs, call.Q, call.h, call.w), dtype=torch.float32, device=call.device)
    check(lib.uenc_crit_mask_loss_bwd(call.desc.ctypes.data, call.n_heads, call.bs, call.Q, call.h, call.w, call.N, P, row_ind.data_ptr(),
                                      points.data_ptr(), unit.data_ptr(), sorted_keys.data_ptr(), order.data_ptr(), gce.data_ptr(), gdice.data_ptr(),
                                      inv_num_masks, gmasks.data_ptr(), stream_ptr()), "crit_mask_loss_bwd")
    return gmasks


def crit_class_loss(call: CritCall, row_ind, col_ind, eos_coef: float):
    """-> loss (heads), grad (heads, bs * Q, C1): F.cross_entropy(logits, target classes built from the indices, weights (1, ..., 1, eos_coef))
    of every head and its gradient.  row_ind / col_ind may be None when there is no pair.  uenc_crit_class_loss."""
    if call.N:
        call._rows(row_ind, "row_ind", torch.int64, ()); call._rows(col_ind, "col_ind", torch.int64, ())
    R = call.bs * call.Q
    rows = torch.empty((call.n_heads, R, 2), dtype=torch.float32, device=call.device)
    loss = torch.empty(call.n_heads, dtype=torch.float32, device=call.device)
    grad = torch.empty((call.n_heads, R, call.C1), dtype=torch.float32, device=call.device)
    check(lib.uenc_crit_class_loss(call.desc.ctypes.data, call.n_heads, call.bs, call.Q, call.C1, call.N, ptr(row_ind) if call.N else 0,
                                   ptr(col_ind) if call.N else 0, eos_coef, rows.data_ptr(), loss.data_ptr(), grad.data_ptr(), stream_ptr()),
          "crit_class_loss")
    return loss, grad


# ---- training targets from a panoptic id map (csrc/targets.hip) --------------------------------------------------------------------------------
TARGETS_MAX_SEGMENTS = _H["UENC_TARGETS_MAX_SEGMENTS"]


def _targets_table(pan, table, B):
    """The batch (B, H, W) and its packed int32 table: seg_ids (B, 256), n_seg (B), sizes (B, 2) as one buffer of B * 259 entries (one
    upload) -> the three views."""
    _dev(pan, "pan", torch.int32, 3)
    _dev(table, "table", torch.int32, 1)
    S = TARGETS_MAX_SEGMENTS
    if pan.shape[0] != B or table.numel() != B * (S + 3) or pan.shape[1] * pan.shape[2] >= 2 ** 31 - 4096:
        raise capi.UencError(f"targets: pan (B, H, W) with H * W < 2^31 - 4096 and a table of B * {S + 3} entries are expected")
    return table[:B * S], table[B * S:B * S + B], table[B * S + B:]


def targets_area(pan: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """-> area (B, 256) int32: the pixels of every table row inside its image's own size.  pan (B, H, W) int32; table: seg_ids (B, 256),
    n_seg (B), sizes (B, 2) packed in that order.  uenc_targets_area."""
    B, H, W = pan.shape
    ids, n_seg, sizes = _targets_table(pan, table, B)
    area = torch.zeros((B, TARGETS_MAX_SEGMENTS), dtype=torch.int32, device=pan.device)
    check(lib.uenc_targets_area(pan.data_ptr(), sizes.data_ptr(), ids.data_ptr(), n_seg.data_ptr(), area.data_ptr(), B, H, W, stream_ptr()),
          "targets_area")
    return area


def targets_write(pan: torch.Tensor, table: torch.Tensor, plan: torch.Tensor, total_planes: int, ignore_label: int):
    """-> masks (total_planes, H, W) uint8, sem_seg (B, H, W) int64.  plan: slot (B, 256), cls (B, 256), plane0 (B), T (B) int32 packed in
    that order (one upload).  Neither output is zeroed first: the kernel writes every byte.  uenc_targets_write."""
    B, H, W = pan.shape
    ids, n_seg, sizes = _targets_table(pan, table, B)
    _dev(plan, "plan", torch.int32, 1)
    S = TARGETS_MAX_SEGMENTS
    if plan.numel() != B * (2 * S + 2) or total_planes < 0:
        raise capi.UencError(f"targets_write: a plan of B * {2 * S + 2} entries and total_planes >= 0 are expected")
    masks = torch.empty((total_planes, H, W), dtype=torch.uint8, device=pan.device)
    sem = torch.empty((B, H, W), dtype=torch.int64, device=pan.device)
    slot, cls, plane0, T = plan[:B * S], plan[B * S:2 * B * S], plan[2 * B * S:2 * B * S + B], plan[2 * B * S + B:]
    check(lib.uenc_targets_write(pan.data_ptr(), sizes.data_ptr(), ids.data_ptr(), n_seg.data_ptr(), slot.data_ptr(), cls.data_ptr(),
                                 plane0.data_ptr(), T.data_ptr(), int(ignore_label), masks.data_ptr() if total_planes else 0, sem.data_ptr(),
                                 B, H, W, total_planes, stream_ptr()), "targets_write")
    return masks, sem


# ---- evaluation statistics on the device (csrc/evalstats.hip) ------------------------------------------------------------------------------------
EVAL_MAX_CLASSES = _H["UENC_EVAL_MAX_CLASSES"]
EVAL_PQ_DIM = _H["UENC_EVAL_PQ_DIM"]            # TARGETS_MAX_SEGMENTS + 2: VOID, 256 table rows, "unknown"


def eval_confusion(pred: torch.Tensor, gt: torch.Tensor, sizes: torch.Tensor, conf: torch.Tensor, ignore_label: int, max_blocks: int = 0):
    """conf ((N + 1), (N + 1)) int64 += the confusion counts conf[pred, gt] of one padded batch.  pred: scores (B, C, H, W) fp32 (the class
    argmax is taken in the kernel) or a label map (B, H, W) int32; gt (B, H, W) int32; sizes (B, 2) int32 = each image's own (h, w).
    Nothing is copied back.  uenc_eval_confusion."""
    _dev(gt, "gt", torch.int32, 3); _dev(sizes, "sizes", torch.int32, 2); _dev(conf, "conf", torch.int64, 2)
    B, H, W = gt.shape
    if pred.dim() == 4:
        _dev(pred, "pred", torch.float32, 4)
        C = int(pred.shape[1])
        ok = C >= 1 and tuple(pred.shape) == (B, C, H, W)
    else:
        _dev(pred, "pred", torch.int32, 3)
        C, ok = 0, tuple(pred.shape) == (B, H, W)
    N = int(conf.shape[0]) - 1
    if not ok or tuple(sizes.shape) != (B, 2) or conf.shape[0] != conf.shape[1]:
        raise capi.UencError(f"eval_confusion: pred {tuple(pred.shape)}, gt {tuple(gt.shape)}, sizes {tuple(sizes.shape)}, conf {tuple(conf.shape)} do not fit")
    check(lib.uenc_eval_confusion(pred.data_ptr(), gt.data_ptr(), sizes.data_ptr(), conf.data_ptr(), B, C, H, W, N, int(ignore_label),
                                  int(max_blocks), stream_ptr()), "eval_confusion")
    return conf


def _eval_pq_table(table, B):
    """The packed int32 table of a panoptic-quality call (one upload): gt_ids, pred_ids, gt_cat, gt_crowd, pred_cat (B, 256 each), n_gt (B),
    n_pred (B), sizes (B, 2), in that order -> the eight views."""
    S = TARGETS_MAX_SEGMENTS
    _dev(table, "table", torch.int32, 1)
    if table.numel() != B * (5 * S + 4):
        raise capi.UencError(f"eval_pq: a table of B * {5 * S + 4} entries is expected")
    cut = [B * S] * 5 + [B, B, 2 * B]
    return torch.split(table, cut)


def eval_pq_intersect(pred: torch.Tensor, gt: torch.Tensor, table: torch.Tensor, max_blocks: int = 0) -> torch.Tensor:
    """-> inter (B, 258, 258) int32: pixels per (ground-truth row, predicted column); row / column 0 is id 0 (VOID), 1 + k the k-th id of
    the table, n + 1 an id the table does not list.  pred, gt (B, H, W) int32; table as `_eval_pq_table`.  uenc_eval_pq_intersect."""
    _dev(pred, "pred", torch.int32, 3); _dev(gt, "gt", torch.int32, 3)
    B, H, W = gt.shape
    if tuple(pred.shape) != (B, H, W):
        raise capi.UencError(f"eval_pq_intersect: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ")
    gt_ids, pred_ids, _, _, _, n_gt, n_pred, sizes = _eval_pq_table(table, B)
    inter = torch.zeros((B, EVAL_PQ_DIM, EVAL_PQ_DIM), dtype=torch.int32, device=gt.device)
    check(lib.uenc_eval_pq_intersect(pred.data_ptr(), gt.data_ptr(), sizes.data_ptr(), gt_ids.data_ptr(), n_gt.data_ptr(), pred_ids.data_ptr(),
                                     n_pred.data_ptr(), inter.data_ptr(), B, H, W, int(max_blocks), stream_ptr()), "eval_pq_intersect")
    return inter


def eval_pq_match(inter: torch.Tensor, table: torch.Tensor, num_categories: int) -> torch.Tensor:
    """-> one flat int32 buffer of B * (1024 + 2 K + 1) entries (one allocation; `eval_pq_unpack` gives its parts): rec (B, 256, 4) =
    matched predicted row or -1, inter, union, category per ground-truth row; fp (B, K); fn (B, K); unknown (B) = the pixels of predicted
    ids the table does not list.  uenc_eval_pq_match."""
    _dev(inter, "inter", torch.int32, 3)
    B, K = int(inter.shape[0]), int(num_categories)
    if tuple(inter.shape[1:]) != (EVAL_PQ_DIM, EVAL_PQ_DIM) or not 1 <= K <= EVAL_MAX_CLASSES:
        raise capi.UencError(f"eval_pq_match: inter (B, {EVAL_PQ_DIM}, {EVAL_PQ_DIM}) and 1 <= K <= {EVAL_MAX_CLASSES} are expected")
    _, _, gt_cat, gt_crowd, pred_cat, n_gt, n_pred, _ = _eval_pq_table(table, B)
    out = torch.empty(B * (4 * TARGETS_MAX_SEGMENTS + 2 * K + 1), dtype=torch.int32, device=inter.device)
    rec, fp, fn, unknown = eval_pq_unpack(out, B, K)
    check(lib.uenc_eval_pq_match(inter.data_ptr(), n_gt.data_ptr(), n_pred.data_ptr(), gt_cat.data_ptr(), gt_crowd.data_ptr(), pred_cat.data_ptr(),
                                 rec.data_ptr(), fp.data_ptr(), fn.data_ptr(), unknown.data_ptr(), B, K, stream_ptr()), "eval_pq_match")
    return out


def eval_pq_unpack(out, B: int, num_categories: int):
    """The buffer of `eval_pq_match` (a tensor or a numpy array) -> views rec (B, 256, 4), fp (B, K), fn (B, K), unknown (B)."""
    S, K = TARGETS_MAX_SEGMENTS, int(num_categories)
    a, b, c = B * 4 * S, B * (4 * S + K), B * (4 * S + 2 * K)
    return out[:a].reshape(B, S, 4), out[a:b].reshape(B, K), out[b:c].reshape(B, K), out[c:]


# ---- depth evaluation on the device (csrc/ext/depth_eval.hip; declared in include/uenc_ext.h) ---------------------------------------------------
_X = capi.EXT_CONSTANTS
DEPTH_EVAL_ROW = _X["UENC_DEPTH_EVAL_ROW"]      # doubles per image: the seven metrics, n, median gt, median pred, the three threshold counts
DEPTH_EVAL_LAUNCHES = {torch.float32: _X["UENC_DEPTH_EVAL_LAUNCHES_F32"], torch.float64: _X["UENC_DEPTH_EVAL_LAUNCHES_F64"]}   # kernels of one score
_DEPTH_GT = {torch.float32: F32, torch.float64: _X["UENC_EXT_F64"]}


def depth_eval_pred(disp: torch.Tensor, size, want_resized: bool = False):
    """disp (h, w) fp32, a scaled disparity -> pred (H, W) fp32 = 1 / bilinear resize to size = (H, W) (half-pixel centres, taps and
    lerps in fp64, one rounding); with want_resized also the resized disparity.  uenc_depth_eval_pred."""
    _dev(disp, "disp", torch.float32, 2)
    H, W = int(size[0]), int(size[1])
    pred = torch.empty((H, W), dtype=torch.float32, device=disp.device)
    resized = torch.empty_like(pred) if want_resized else None
    check(lib.uenc_depth_eval_pred(disp.data_ptr(), pred.data_ptr(), ptr(resized), int(disp.shape[0]), int(disp.shape[1]), H, W, stream_ptr()),
          "depth_eval_pred")
    return (pred, resized) if want_resized else pred


def depth_eval_ws(H: int, W: int, device) -> torch.Tensor:
    """The workspace `depth_eval_score` needs for (H, W) maps.  uenc_depth_eval_ws_bytes."""
    n = lib.uenc_depth_eval_ws_bytes(int(H), int(W))
    if n < 0:
        raise capi.UencError(f"depth_eval_ws: a map of {H} x {W} is refused")
    return torch.empty((n + 7) // 8, dtype=torch.int64, device=device)


def depth_eval_score(gt: torch.Tensor, pred: torch.Tensor, window, min_depth: float, max_depth: float, rows: torch.Tensor, row: int,
                     ws: Optional[torch.Tensor] = None):
    """rows[row] <- the score of one image: gt (H, W) fp32 or fp64, pred (H, W) fp32, window = (r0, r1, c0, c1), rows
    (capacity, DEPTH_EVAL_ROW) fp64.  Nothing is copied back.  uenc_depth_eval_score."""
    if gt.dtype not in _DEPTH_GT:
        raise capi.UencError(f"depth_eval_score: gt must be float32 or float64, got {gt.dtype}")
    _dev(gt, "gt", gt.dtype, 2); _dev(pred, "pred", torch.float32, 2); _dev(rows, "rows", torch.float64, 2)
    H, W = gt.shape
    if tuple(pred.shape) != (H, W) or rows.shape[1] != DEPTH_EVAL_ROW:
        raise capi.UencError(f"depth_eval_score: gt {tuple(gt.shape)}, pred {tuple(pred.shape)}, rows {tuple(rows.shape)} do not fit")
    if ws is None:
        ws = depth_eval_ws(H, W, gt.device)
    r0, r1, c0, c1 = (int(v) for v in window)
    check(lib.uenc_depth_eval_score(gt.data_ptr(), _DEPTH_GT[gt.dtype], pred.data_ptr(), H, W, r0, r1, c0, c1, float(min_depth), float(max_depth),
                                    ws.data_ptr(), ws.numel() * 8, rows.data_ptr(), int(row), int(rows.shape[0]), stream_ptr()),
          "depth_eval_score")
    return rows


# ---- MonodepthLoss: view synthesis + photometric loss (csrc/monodepth.hip) -----------------------------------------------------------------
# slots of the 67-pointer descriptor of uenc_view_synth_fwd / _bwd (struct VsDesc)
_VS = {"disp": 0, "cflow": 4, "mask": 12, "T": 20, "K": 21, "invK": 22, "src": 23, "color": 24, "sample": 25, "sample_ego": 26, "sample_cmp": 27,
       "depth": 28, "residual": 29, "gcolor": 37, "gres": 38, "gdisp": 46, "gcflow": 50, "gmask": 58, "gT": 66}
_VS_SLOTS = 67


def _vs_desc(mode, K, inv_K, src, T, disps, cflows, masks):
    """Checks the inputs of one view-synthesis call and fills the input slots -> (descriptor, S, NF, B, H, W)."""
    _dev(src, "src", torch.float32, 5)
    NF, B, _, H, W = src.shape
    S = len(disps)
    if not (1 <= S <= 4 and 1 <= NF <= 2) or src.shape[2] != 3 or mode not in (0, 1, 2):
        raise capi.UencError("view_synth: 1..4 scales, 1..2 source frames of 3 channels, mode 0 / 1 / 2")
    _dev(K, "K", torch.float32, 3); _dev(inv_K, "inv_K", torch.float32, 3); _dev(T, "cam_T_cam", torch.float32, 4)
    if tuple(K.shape) != (B, 4, 4) or tuple(inv_K.shape) != (B, 4, 4) or tuple(T.shape) != (NF, B, 4, 4):
        raise capi.UencError("view_synth: K / inv_K (B, 4, 4) and cam_T_cam (NF, B, 4, 4) are required")
    d = np.zeros(_VS_SLOTS, dtype=np.uint64)
    d[_VS["T"]], d[_VS["K"]], d[_VS["invK"]], d[_VS["src"]] = T.data_ptr(), K.data_ptr(), inv_K.data_ptr(), src.data_ptr()
    for s in range(S):
        if (H >> s) << s != H or (W >> s) << s != W:
            raise capi.UencError(f"view_synth: {H} x {W} is not divisible by 2^{s}")
        shape = (B, 1, H >> s, W >> s)
        if tuple(_dev(disps[s], "disp", torch.float32, 4).shape) != shape:
            raise capi.UencError(f"view_synth: disp of scale {s} must be {shape}")
        d[_VS["disp"] + s] = disps[s].data_ptr()
        for f in range(NF):
            if mode >= 1:
                if tuple(_dev(cflows[s * NF + f], "complete_flow", torch.float32, 4).shape) != (B, 3, H >> s, W >> s):
                    raise capi.UencError(f"view_synth: complete_flow of scale {s} must be {(B, 3, H >> s, W >> s)}")
                d[_VS["cflow"] + s * NF + f] = cflows[s * NF + f].data_ptr()
            if mode >= 2:
                if tuple(_dev(masks[s * NF + f], "motion_mask", torch.float32, 4).shape) != shape:
                    raise capi.UencError(f"view_synth: motion_mask of scale {s} must be {shape}")
                d[_VS["mask"] + s * NF + f] = masks[s * NF + f].data_ptr()
    return d, S, NF, B, H, W


def view_synth_fwd(mode: int, K, inv_K, src, T, disps, cflows=None, masks=None):
    """One uenc_view_synth_fwd launch for all scales, source frames and images -> {"color" (S, NF, B, 3, H, W), "sample" (S, NF, B, H, W, 2),
    "depth" (S, B, 1, H, W)} and for mode >= 1 {"sample_ego", "sample_complete", "residual": S * NF tensors (B, 3, H, W)}."""
    d, S, NF, B, H, W = _vs_desc(mode, K, inv_K, src, T, disps, cflows, masks)
    dev = src.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = {"color": new(S, NF, B, 3, H, W), "sample": new(S, NF, B, H, W, 2), "depth": new(S, B, 1, H, W)}
    d[_VS["color"]], d[_VS["sample"]], d[_VS["depth"]] = out["color"].data_ptr(), out["sample"].data_ptr(), out["depth"].data_ptr()
    if mode >= 1:
        out["sample_ego"], out["sample_complete"] = new(S, NF, B, H, W, 2), new(S, NF, B, H, W, 2)
        out["residual"] = [new(B, 3, H, W) for _ in range(S * NF)]
        d[_VS["sample_ego"]], d[_VS["sample_cmp"]] = out["sample_ego"].data_ptr(), out["sample_complete"].data_ptr()
        for i, r in enumerate(out["residual"]):
            d[_VS["residual"] + i] = r.data_ptr()
    check(lib.uenc_view_synth_fwd(d.ctypes.data, S, NF, B, H, W, mode, stream_ptr()), "view_synth_fwd")
    return out


def view_synth_bwd(mode: int, K, inv_K, src, T, disps, cflows, masks, gcolor, gres=None):
    """-> (d cam_T_cam (NF, B, 4, 4), [d disp], [d complete_flow] or None, [d motion_mask] or None) from d color and, for mode >= 1, the S * NF
    d residual tensors (None = zero).  Two launches, no atomics."""
    d, S, NF, B, H, W = _vs_desc(mode, K, inv_K, src, T, disps, cflows, masks)
    dev = src.device
    gcolor = _dev(gcolor.contiguous(), "grad color", torch.float32, 6)
    if tuple(gcolor.shape) != (S, NF, B, 3, H, W):
        raise capi.UencError("view_synth_bwd: grad color must be (S, NF, B, 3, H, W)")
    d[_VS["gcolor"]] = gcolor.data_ptr()
    keep = [gcolor]
    if mode >= 1 and gres is not None:
        for i, g in enumerate(gres):
            if g is not None:
                g = _dev(g.contiguous(), "grad residual", torch.float32, 4)
                if tuple(g.shape) != (B, 3, H, W):
                    raise capi.UencError("view_synth_bwd: grad residual must be (B, 3, H, W)")
                keep.append(g)
                d[_VS["gres"] + i] = g.data_ptr()
    gT = torch.empty((NF, B, 4, 4), dtype=torch.float32, device=dev)
    gdisp = [torch.empty_like(t) for t in disps]
    gcf = [torch.empty_like(t) for t in cflows] if mode >= 1 else None
    gmask = [torch.empty_like(t) for t in masks] if mode >= 2 else None
    d[_VS["gT"]] = gT.data_ptr()
    for s in range(S):
        d[_VS["gdisp"] + s] = gdisp[s].data_ptr()
    for i in range(S * NF):
        if mode >= 1:
            d[_VS["gcflow"] + i] = gcf[i].data_ptr()
        if mode >= 2:
            d[_VS["gmask"] + i] = gmask[i].data_ptr()
    nws = lib.uenc_view_synth_workspace_floats(S, NF, B, H, W)
    if nws < 0:
        raise capi.UencError("view_synth_bwd: shape beyond the kernel's limits")
    ws = torch.empty(nws, dtype=torch.float32, device=dev)
    check(lib.uenc_view_synth_bwd(d.ctypes.data, S, NF, B, H, W, mode, ws.data_ptr(), nws, stream_ptr()), "view_synth_bwd")
    return gT, gdisp, gcf, gmask


def _photo_shapes(color, target):
    _dev(color, "color", torch.float32, 6); _dev(target, "target", torch.float32, 4)
    S, NF, B, C, H, W = color.shape
    if C != 3 or tuple(target.shape) != (B, 3, H, W):
        raise capi.UencError("photo_loss: color (S, NF, B, 3, H, W) and target (B, 3, H, W) are required")
    return S, NF, B, H, W


def photo_loss_fwd(color, target, src=None, noise=None):
    """-> (p_photo (S,), argmin (S, B, H, W) uint8).  `noise` (S, B, NF, H, W) switches auto-masking on: the source frames `src`
    (NF, B, 3, H, W) plus noise * 1e-5 are candidates 0 .. NF - 1, the warped frames follow."""
    S, NF, B, H, W = _photo_shapes(color, target)
    automask = int(noise is not None)
    if automask:
        _dev(src, "src", torch.float32, 5); _dev(noise, "noise", torch.float32, 5)
        if tuple(src.shape) != (NF, B, 3, H, W) or tuple(noise.shape) != (S, B, NF, H, W):
            raise capi.UencError("photo_loss: src (NF, B, 3, H, W) and noise (S, B, NF, H, W) are required for auto-masking")
    nws = lib.uenc_photo_loss_workspace_floats(S, B, H, W)
    if nws < 0:
        raise capi.UencError("photo_loss: shape beyond the kernel's limits")
    ws = torch.empty(nws, dtype=torch.float32, device=color.device)
    arg = torch.empty((S, B, H, W), dtype=torch.uint8, device=color.device)
    p = torch.empty(S, dtype=torch.float32, device=color.device)
    check(lib.uenc_photo_loss_fwd(color.data_ptr(), target.data_ptr(), ptr(src) if automask else 0, ptr(noise), S, NF, B, H, W, automask,
                                  ws.data_ptr(), nws, arg.data_ptr(), p.data_ptr(), stream_ptr()), "photo_loss_fwd")
    return p, arg


def photo_loss_bwd(color, target, argmin, grad_p, automask: bool):
    """d(sum_s grad_p[s] p_photo[s]) / d color, shaped as color."""
    S, NF, B, H, W = _photo_shapes(color, target)
    _dev(argmin, "argmin", torch.uint8, 4); _dev(grad_p, "grad p_photo", torch.float32, 1)
    if tuple(argmin.shape) != (S, B, H, W) or grad_p.shape[0] != S:
        raise capi.UencError("photo_loss_bwd: argmin (S, B, H, W) and grad (S,) are required")
    g = torch.empty_like(color)
    check(lib.uenc_photo_loss_bwd(color.data_ptr(), target.data_ptr(), argmin.data_ptr(), grad_p.data_ptr(), S, NF, B, H, W, int(automask),
                                  g.data_ptr(), stream_ptr()), "photo_loss_bwd")
    return g


# ---- ConvNeXt block: 7x7 depthwise convolution + LayerNorm (csrc/dwconv.hip) ----
def _dw_check(x: torch.Tensor, name: str):
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
        raise capi.UencError(f"{name} must be a contiguous (B, H, W, C) fp32 GPU tensor, got {tuple(x.shape)} {x.dtype}")
    if x.shape[-1] % 8 != 0:
        raise ValueError(f"the depthwise-convolution kernels need a channel count that is a multiple of 8 (got {x.shape[-1]}); every "
                         "stock ConvNeXt width satisfies this")
    return x.shape


def dwconv7_ln_fwd(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-6):
    """x (B, H, W, C) fp32 channels-last, w (C, 1, 7, 7), b (C) -> (y = dwconv7x7(x) + b in fp32, h = LN_C(y) in the GEMM operand dtype
    (bf16; fp32 in exact mode), stats (B*H*W, 2) = (mean, rstd))."""
    B, H, W, C = _dw_check(x, "x")
    assert w.dtype == torch.float32 and w.is_contiguous() and w.numel() == 49 * C and (b is None or (b.dtype == torch.float32 and b.numel() == C))
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == C and beta.numel() == C
    y = torch.empty_like(x)
    h = torch.empty(x.shape, dtype=adt(), device=x.device)
    stats = torch.empty((B * H * W, 2), dtype=torch.float32, device=x.device)
    check(lib.uenc_dwconv7_ln_fwd(x.data_ptr(), w.data_ptr(), ptr(b), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), h.data_ptr(), dt(h),
                                  stats.data_ptr(), B, H, W, C, float(eps), stream_ptr()), "dwconv7_ln_fwd")
    return y, h, stats


def dwconv7_ln_bwd_data(dh: torch.Tensor, y: torch.Tensor, stats: torch.Tensor, gamma: torch.Tensor, w: torch.Tensor, *,
                        dout: Optional[torch.Tensor] = None, dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None,
                        defer: Optional["SmallReductions"] = None):
    """-> (dx, dy): dy = LN'(dh) per pixel (fp32, the weight-gradient kernel's operand), dx = dwconv7x7^T(dy) [+ dout].  dh in the operand
    dtype, dout the fp32 gradient of the block's skip path; the LayerNorm's dgamma / dbeta are accumulated in place (`defer`: as in
    layernorm_bwd)."""
    B, H, W, C = _dw_check(y, "y")
    assert dh.is_contiguous() and dh.numel() == y.numel() and dh.is_cuda and w.is_contiguous() and w.numel() == 49 * C
    if dout is not None:
        assert dout.dtype == torch.float32 and dout.is_contiguous() and dout.numel() == y.numel()
    dy, dx = torch.empty_like(y), torch.empty_like(y)
    part, deferred = _ln_part(B * H * W, C, dgamma, dbeta, y.device, defer)
    check(lib.uenc_dwconv7_ln_bwd_data(dh.data_ptr(), dt(dh), y.data_ptr(), stats.data_ptr(), gamma.data_ptr(), w.data_ptr(), ptr(dout),
                                       dy.data_ptr(), dx.data_ptr(), ptr(dgamma), ptr(dbeta), ptr(part), int(deferred), B, H, W, C,
                                       stream_ptr()), "dwconv7_ln_bwd_data")
    return dx, dy


def dwconv7_bwd_weight(dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor, db: Optional[torch.Tensor] = None):
    """dw (C, 1, 7, 7) += correlation of dy with x over all pixels, db (C) += sum of dy; two stages, fixed summation order."""
    B, H, W, C = _dw_check(x, "x")
    _dw_check(dy, "dy")
    assert dy.shape == x.shape and dw.dtype == torch.float32 and dw.is_contiguous() and dw.numel() == 49 * C
    assert db is None or (db.dtype == torch.float32 and db.is_contiguous() and db.numel() == C)
    nbytes = int(lib.uenc_dwconv7_bwd_weight_workspace_bytes(B, H, W, C))
    ws = _scratch("dwconv_wgrad", nbytes, x.device)
    check(lib.uenc_dwconv7_bwd_weight(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), ptr(db), ws.data_ptr(), ws.numel(), B, H, W, C, stream_ptr()),
          "dwconv7_bwd_weight")


def layer_scale_grads(dw2p: torch.Tensor, db2p: Optional[torch.Tensor], w2: torch.Tensor, b2: Optional[torch.Tensor], gamma: torch.Tensor,
                      gw2: Optional[torch.Tensor], gb2: Optional[torch.Tensor], ggamma: Optional[torch.Tensor]):
    """Gradients of W2, b2, gamma from those of the folded layer W2' = gamma (.) W2, b2' = gamma (.) b2 (accumulated in place)."""
    N, Kd = w2.shape
    for t in (dw2p, w2, gw2):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (N, Kd))
    for t in (db2p, b2, gamma, gb2, ggamma):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == N)
    check(lib.uenc_layer_scale_grads(dw2p.data_ptr(), ptr(db2p), w2.data_ptr(), ptr(b2), gamma.data_ptr(), ptr(gw2), ptr(gb2), ptr(ggamma),
                                     N, Kd, stream_ptr()), "layer_scale_grads")


# ---- ResNet backbone: stem patch gather, max pooling, BatchNorm + residual + ReLU (csrc/resnet.hip) ----
def _cl_check(x: torch.Tensor, name: str, ndim: int):
    if x.dim() != ndim or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_cuda or not x.is_contiguous():
        raise capi.UencError(f"{name} must be a contiguous {ndim}-D channels-last fp32 | bf16 GPU tensor, got {tuple(x.shape)} {x.dtype}")
    if x.shape[-1] % 8 != 0:
        raise ValueError(f"the ResNet kernels need a channel count that is a multiple of 8 (got {x.shape[-1]}); every stock ResNet width "
                         "satisfies this")
    return x.shape


def _cvec(t: Optional[torch.Tensor], C: int, name: str):
    assert t is None or (t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() == C), name
    return t


def stem7x7_s2_patches(x: torch.Tensor) -> torch.Tensor:
    """x (B, 3, H, W) fp32 NCHW -> (B * Ho * Wo, 152) patch matrix of the 7x7 stride-2 padding-3 convolution in the GEMM operand dtype,
    (ky, kx, c) column order, 147 columns zero-padded to 152; Ho = (H - 1) // 2 + 1."""
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
        raise capi.UencError(f"stem7x7_s2_patches: x must be a contiguous (B, 3, H, W) fp32 GPU tensor, got {tuple(x.shape)} {x.dtype}")
    B, _, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    col = torch.empty((B * Ho * Wo, 152), dtype=adt(), device=x.device)
    check(lib.uenc_stem7x7_s2_patches(x.data_ptr(), col.data_ptr(), dt(col), B, H, W, stream_ptr()), "stem7x7_s2_patches")
    return col


def maxpool3x3_s2_fwd(x: torch.Tensor):
    """F.max_pool2d(x, 3, 2, 1) on x (B, H, W, C) channels-last -> (y (B, Ho, Wo, C) in x's dtype, idx uint8: the selected tap)."""
    B, H, W, C = _cl_check(x, "x", 4)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, Ho, Wo, C), dtype=x.dtype, device=x.device)
    idx = torch.empty((B, Ho, Wo, C), dtype=torch.uint8, device=x.device)
    check(lib.uenc_maxpool3x3_s2_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr(), dt(x), B, H, W, C, stream_ptr()), "maxpool3x3_s2_fwd")
    return y, idx


def maxpool3x3_s2_bwd(dy: torch.Tensor, idx: torch.Tensor, H: int, W: int) -> torch.Tensor:
    B, Ho, Wo, C = _cl_check(dy, "dy", 4)
    assert idx.dtype == torch.uint8 and idx.is_contiguous() and idx.shape == dy.shape and (Ho, Wo) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    dx = torch.empty((B, H, W, C), dtype=dy.dtype, device=dy.device)
    check(lib.uenc_maxpool3x3_s2_bwd(dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), dt(dy), B, H, W, C, stream_ptr()), "maxpool3x3_s2_bwd")
    return dx


def _bn_ws(M: int, C: int, device) -> torch.Tensor:
    return _scratch("bn_slabs", 4 * int(lib.uenc_bn_workspace_floats(M, C)), device)


def bn_stats(x2: torch.Tensor, running_mean=None, running_var=None, num_batches_tracked=None, momentum: float = 0.1):
    """x2 (M, C) -> (mean, biased variance) per channel, fp32; the running statistics (unbiased variance) and the int64 batch counter are
    updated in place on the device.  One value per channel is refused as torch does."""
    M, C = _cl_check(x2, "x", 2)
    if M <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x2.shape)}")
    _cvec(running_mean, C, "running_mean"); _cvec(running_var, C, "running_var")
    assert num_batches_tracked is None or (num_batches_tracked.dtype == torch.int64 and num_batches_tracked.is_cuda)
    mean = torch.empty((C,), dtype=torch.float32, device=x2.device)
    var = torch.empty_like(mean)
    ws = _bn_ws(M, C, x2.device)
    check(lib.uenc_bn_stats(x2.data_ptr(), dt(x2), M, C, mean.data_ptr(), var.data_ptr(), ptr(running_mean), ptr(running_var),
                            ptr(num_batches_tracked), float(momentum), ws.data_ptr(), ws.numel() // 4, stream_ptr()), "bn_stats")
    return mean, var


def bn_act_fwd(x2: torch.Tensor, mean, var, gamma, beta, *, res=None, relu=False, eps: float = 1e-5, out_dtype=torch.float32):
    """act(x * s + t (+ res)) with s = gamma / sqrt(var + eps), t = beta - mean * s per channel: x2, res (M, C) -> (M, C) out_dtype."""
    M, C = _cl_check(x2, "x", 2)
    for t, n in ((mean, "mean"), (var, "var"), (gamma, "gamma"), (beta, "beta")):
        _cvec(t, C, n)
    if res is not None:
        assert _cl_check(res, "res", 2) == x2.shape
    y = torch.empty((M, C), dtype=out_dtype, device=x2.device)
    check(lib.uenc_bn_act_fwd(x2.data_ptr(), dt(x2), mean.data_ptr(), var.data_ptr(), ptr(gamma), ptr(beta), ptr(res),
                              dt(res) if res is not None else 0, y.data_ptr(), dt(y), M, C, float(eps), int(relu), stream_ptr()), "bn_act_fwd")
    return y


def bn_act_bwd(dy2: torch.Tensor, y2: Optional[torch.Tensor], x2: torch.Tensor, mean, var, gamma, *, relu: bool, train: bool, eps: float = 1e-5,
               dgamma=None, dbeta=None, want_dres: bool = False, dx_dtype=torch.float32, param_sums: bool = True):
    """Backward of bn_act_fwd -> (dx (M, C) dx_dtype, dres | None: the masked gradient in dy's dtype).  y2: the saved output (the ReLU mask),
    x2: the saved input.  dgamma / dbeta (fp32, accumulated in place) may be None; the reduction is skipped when neither the
    parameters (param_sums) nor the batch statistics (train) need it."""
    M, C = _cl_check(dy2, "dy", 2)
    assert x2.shape == dy2.shape and (not relu or (y2 is not None and y2.shape == dy2.shape and y2.is_contiguous()))
    _cl_check(x2, "x", 2)
    for t, n in ((mean, "mean"), (var, "var"), (gamma, "gamma"), (dgamma, "dgamma"), (dbeta, "dbeta")):
        _cvec(t, C, n)
    sums = None
    if train or (param_sums and (dgamma is not None or dbeta is not None)):
        sums = torch.empty((2, C), dtype=torch.float32, device=dy2.device)
        ws = _bn_ws(M, C, dy2.device)
        check(lib.uenc_bn_act_bwd_reduce(dy2.data_ptr(), dt(dy2), ptr(y2), dt(y2) if y2 is not None else 0, x2.data_ptr(), dt(x2),
                                         mean.data_ptr(), var.data_ptr(), M, C, float(eps), int(relu), sums.data_ptr(), ptr(dgamma), ptr(dbeta),
                                         ws.data_ptr(), ws.numel() // 4, stream_ptr()), "bn_act_bwd_reduce")
    dx = torch.empty((M, C), dtype=dx_dtype, device=dy2.device)
    dres = torch.empty_like(dy2) if want_dres else None
    check(lib.uenc_bn_act_bwd_apply(dy2.data_ptr(), dt(dy2), ptr(y2), dt(y2) if y2 is not None else 0, x2.data_ptr(), dt(x2), mean.data_ptr(),
                                    var.data_ptr(), ptr(gamma), ptr(sums), dx.data_ptr(), dt(dx), ptr(dres), dt(dres) if want_dres else 0,
                                    M, C, float(eps), int(relu), int(train), stream_ptr()), "bn_act_bwd_apply")
    return dx, dres


# ---- depth decoder in training: x2 align-corners upsample, softmax gate, soft-attention depth head (csrc/depth_head.hip) --------------
def _dh_check(t: Optional[torch.Tensor], name: str, shape=None):
    if t is None:
        return None
    if t.dtype not in (torch.float32, torch.bfloat16) or not t.is_cuda or not t.is_contiguous():
        raise capi.UencError(f"{name} must be a contiguous channels-last fp32 | bf16 GPU tensor, got {tuple(t.shape)} {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise capi.UencError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def upsample2x_ac_fwd(x: torch.Tensor, out_dtype=None) -> torch.Tensor:
    """x (B, H, W, C) -> (B, 2H, 2W, C): bilinear, align_corners=True, F.interpolate's source coordinates."""
    _dh_check(x, "x")
    B, H, W, C = x.shape
    y = torch.empty((B, 2 * H, 2 * W, C), dtype=x.dtype if out_dtype is None else out_dtype, device=x.device)
    check(lib.uenc_upsample2x_ac_fwd(x.data_ptr(), dt(x), y.data_ptr(), dt(y), B, H, W, C, stream_ptr()), "upsample2x_ac_fwd")
    return y


def upsample2x_ac_bwd(dy: torch.Tensor, out_dtype=None) -> torch.Tensor:
    """dy (B, 2H, 2W, C) -> dx (B, H, W, C): the adjoint of upsample2x_ac_fwd as a gather (no atomics)."""
    _dh_check(dy, "dy")
    B, Ho, Wo, C = dy.shape
    if Ho % 2 or Wo % 2:
        raise capi.UencError(f"upsample2x_ac_bwd: dy must have even height and width, got {tuple(dy.shape)}")
    dx = torch.empty((B, Ho // 2, Wo // 2, C), dtype=dy.dtype if out_dtype is None else out_dtype, device=dy.device)
    check(lib.uenc_upsample2x_ac_bwd(dy.data_ptr(), dt(dy), dx.data_ptr(), dt(dx), B, Ho // 2, Wo // 2, C, stream_ptr()), "upsample2x_ac_bwd")
    return dx


def softmax_gate_fwd(a: torch.Tensor, b: torch.Tensor, z: torch.Tensor, out_dtype=torch.float32):
    """a, b, z (..., C) -> (res = a + b, g = res * softmax over the last axis of z), both out_dtype."""
    _dh_check(a, "a"), _dh_check(b, "b", a.shape), _dh_check(z, "z", a.shape)
    C = a.shape[-1]
    res = torch.empty(a.shape, dtype=out_dtype, device=a.device)
    g = torch.empty_like(res)
    check(lib.uenc_softmax_gate_fwd(a.data_ptr(), dt(a), b.data_ptr(), dt(b), z.data_ptr(), dt(z), res.data_ptr(), g.data_ptr(), dt(res),
                                    a.numel() // max(C, 1), C, stream_ptr()), "softmax_gate_fwd")
    return res, g


def softmax_gate_bwd(dg: torch.Tensor, d_res_in: Optional[torch.Tensor], z: torch.Tensor, res: torch.Tensor, out_dtype=torch.float32):
    """-> (d_res = dg * att + d_res_in, d_z = att * (dg * res - sum_c(dg * res * att))) with att = softmax(z) recomputed."""
    _dh_check(dg, "dg"), _dh_check(d_res_in, "d_res_in", dg.shape), _dh_check(z, "z", dg.shape), _dh_check(res, "res", dg.shape)
    C = dg.shape[-1]
    d_res = torch.empty(dg.shape, dtype=out_dtype, device=dg.device)
    d_z = torch.empty_like(d_res)
    check(lib.uenc_softmax_gate_bwd(dg.data_ptr(), dt(dg), ptr(d_res_in), dt(d_res_in) if d_res_in is not None else 0, z.data_ptr(), dt(z),
                                    res.data_ptr(), dt(res), d_res.data_ptr(), d_z.data_ptr(), dt(d_res), dg.numel() // max(C, 1), C,
                                    stream_ptr()), "softmax_gate_bwd")
    return d_res, d_z


def _dh_grid(grid: torch.Tensor, D: int):
    if grid.dtype != torch.float32 or not grid.is_cuda or not grid.is_contiguous() or grid.numel() != D:
        raise capi.UencError(f"grid must be a contiguous fp32 GPU vector of {D} depth bins, got {tuple(grid.shape)} {grid.dtype}")


def soft_att_depth_fwd(z: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
    """z (..., D), grid (D) fp32 -> disp (...) fp32 = sum_k softmax(z)_k * grid_k."""
    _dh_check(z, "z")
    D = z.shape[-1]
    _dh_grid(grid, D)
    disp = torch.empty(z.shape[:-1], dtype=torch.float32, device=z.device)
    check(lib.uenc_soft_att_depth_fwd(z.data_ptr(), dt(z), grid.data_ptr(), disp.data_ptr(), z.numel() // max(D, 1), D, stream_ptr()),
          "soft_att_depth_fwd")
    return disp


def soft_att_depth_bwd(ddisp: torch.Tensor, z: torch.Tensor, grid: torch.Tensor, out_dtype=torch.float32) -> torch.Tensor:
    """ddisp (...) fp32, z (..., D) -> dz (..., D) out_dtype = p * (grid - disp) * ddisp, p and disp recomputed."""
    _dh_check(z, "z")
    D = z.shape[-1]
    _dh_grid(grid, D)
    if ddisp.dtype != torch.float32 or not ddisp.is_cuda or not ddisp.is_contiguous() or ddisp.numel() != z.numel() // max(D, 1):
        raise capi.UencError(f"ddisp must be a contiguous fp32 GPU tensor with one value per row of z, got {tuple(ddisp.shape)} {ddisp.dtype}")
    dz = torch.empty(z.shape, dtype=out_dtype, device=z.device)
    check(lib.uenc_soft_att_depth_bwd(ddisp.data_ptr(), z.data_ptr(), dt(z), grid.data_ptr(), dz.data_ptr(), dt(dz), z.numel() // max(D, 1), D,
                                      stream_ptr()), "soft_att_depth_bwd")
    return dz


# ---- training-time augmentation of one sample (csrc/augment.hip) ------------------------------------------------------------------------------
AUG_TILE_W, AUG_TILE_H, AUG_MAX_TAPS, AUG_COLOUR_TAB_INTS = (_H["UENC_AUG_" + n] for n in ("TILE_W", "TILE_H", "MAX_TAPS", "COLOUR_TAB_INTS"))


def augment_tile_fits(in_h: int, in_w: int, rs_h: int, rs_w: int, kx: int, ky: int) -> bool:
    """Whether one 64 x 16 output tile of the resize (in_h, in_w) -> (rs_h, rs_w) fits the image kernel's LDS.  No GPU is needed."""
    return bool(lib.uenc_augment_tile_fits(int(in_h), int(in_w), int(rs_h), int(rs_w), int(kx), int(ky)))


def _augment_geometry(plan):
    (h, w), (rs_h, rs_w), (x0, y0, cw, ch), (out_h, out_w) = plan.src_hw, plan.resized_hw, plan.crop, plan.out_hw
    return h, w, rs_h, rs_w, x0, y0, cw, ch, out_h, out_w


def augment_image(buf: torch.Tensor, off: dict, meta: dict, plan) -> torch.Tensor:
    """One launch on the current stream: the frames of one sample's upload `buf` (uint8, on the GPU; uenc.train_data.pack_plan wrote it:
    tables, frames, panoptic PNG, label map at the byte offsets `off`) -> images (F, 3, H, W) uint8 under the sample's AugPlan.  A plan
    whose tile does not fit the kernel's LDS is an error (UencError), there is no other path.  uenc_augment_image."""
    _dev(buf, "buf", torch.uint8, 1)
    h, w, rs_h, rs_w, x0, y0, cw, ch, out_h, out_w = _augment_geometry(plan)
    base, F = buf.data_ptr(), int(meta["F"])
    at = lambda name: base + off[name] if name in off else None
    images = torch.empty((F, 3, out_h, out_w), dtype=torch.uint8, device=buf.device)
    check(lib.uenc_augment_image(at("frame0"), int(meta["frame_stride"]), F, h, w, rs_h, rs_w, x0, y0, cw, ch, at("col_tab"), int(meta["kx"]),
                                 at("row_tab"), int(meta["ky"]), at("colour_tab"), int(meta["flags"]), int(meta["hue"]), int(plan.flip),
                                 out_h, out_w, int(plan.pad_image), images.data_ptr(), stream_ptr()), "augment_image")
    return images


def augment_labels(buf: torch.Tensor, off: dict, meta: dict, plan):
    """One launch: the panoptic PNG and the label map of the upload -> (id map (H, W) int32, label map (H, W) int32 or None), or
    (None, None) for an upload without a panoptic PNG.  uenc_augment_labels."""
    _dev(buf, "buf", torch.uint8, 1)
    if "pan" not in off:
        return None, None
    h, w, rs_h, rs_w, x0, y0, cw, ch, out_h, out_w = _augment_geometry(plan)
    base = buf.data_ptr()
    at = lambda name: base + off[name] if name in off else None
    ids = torch.empty((out_h, out_w), dtype=torch.int32, device=buf.device)
    lab = torch.empty((out_h, out_w), dtype=torch.int32, device=buf.device) if "label" in off else None
    check(lib.uenc_augment_labels(at("pan"), at("label"), int(meta["label_bytes"]), h, w, rs_h, rs_w, x0, y0, cw, ch, at("pan_col"),
                                  at("pan_row"), at("lab_col"), at("lab_row"), int(plan.flip), out_h, out_w, int(plan.pad_label),
                                  ids.data_ptr(), ptr(lab), stream_ptr()), "augment_labels")
    return ids, lab


def augment_sample(buf: torch.Tensor, off: dict, meta: dict, plan):
    """The two launches of one sample on the current stream, nothing copied back -> (images, id map or None, label map or None)."""
    images = augment_image(buf, off, meta, plan)
    ids, lab = augment_labels(buf, off, meta, plan)
    return images, ids, lab
