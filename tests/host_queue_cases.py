"""Shared by tests/test_host_queue_cpu.py and this module's own `--record` mode: one fixed scenario for the host bookkeeping of a
training step -- `ops.CACHE` (the bf16 operand copies and their batched refresh), `ops.WGRADS` (the deferred, grouped weight-gradient
GEMMs, the held notifications, the store flag) and `ops.SMALLQ` (the parked partial sums) -- played on CPU tensors with every launch
site replaced by a recorder.  `play()` returns the log of everything the three classes would have handed to the library, in order:

  ["table", fields, rows]     a descriptor table given to `K.upload_table`: the dtype's field names and one list of values per record;
                              every `<u8` (pointer) field reads "name+byte offset" of a tensor the scenario registered, or 0
  ["launch", entry, args]     a call of one of the library's grouped entry points with its scalar arguments (the table's pointer
                              normalised the same way)
  ["notify", name]            the gradient listener was told that parameter `name` is final
  ["post", name] / ["say", ...]   a held step ran / a figure the scenario reads back (queue counters, cache counters)

Nothing here knows how the classes keep their records: the scenario uses the public names only, so the same file plays against any
revision of `uenc/`.  `python tests/host_queue_cases.py --record OUT.json --pkg DIR --rev HASH` plays it against the package in DIR
(a checkout of revision HASH with the built library copied in) and writes the golden that tests/test_host_queue_cpu.py compares with.
Integers and floats are compared exactly: an fp32 `alpha` is logged as the double of the stored float, `flops` / `nbytes` as given.
"""
import gc
import json
import sys

import numpy as np
import torch

BF16, F32 = torch.bfloat16, torch.float32
# the six problems of tests/test_ops_gpu.py::test_wgrad_queue_grouped_launch (both tile classes, ragged N / K, several token splits)
BIG = [(4096, 512, 256), (2048, 96, 200), (131072, 192, 64), (16384, 768, 3072), (6400, 264, 1024), (2048, 1024, 1280)]
# (M, N, K, dy dtype, x dtype) for the register-staged class: first guesses 1, 3 and 10
SMALL = [(1000, 72, 136, F32, BF16), (5000, 256, 64, BF16, F32), (20000, 8, 24, BF16, BF16)]
CONV = (32832, 256, 576)            # floor rule: max(1, M // 16384) = 2 -> mlen 16448, nsplit 2 (a ceil would split 3-way)
LAUNCHES = ("uenc_gemm_tn_grouped", "uenc_gemm_tn_grouped_small", "uenc_prof_next_bytes", "uenc_ln_param_grouped",
            "uenc_window_attn_dtable_grouped", "uenc_cast_multi", "uenc_relpos_expand_grouped")


class _Recorder:
    def __init__(self):
        self.log, self.named, self.count = [], [], {}

    def reg(self, name, t):
        """Give tensor `t` a name; a detached alias keeps its storage (and so its address range) alive to the end of the scenario."""
        a = t.detach()
        self.named.append((a.data_ptr(), a.data_ptr() + max(1, a.numel() * a.element_size()), name, a))
        return t

    def auto(self, kind, t):
        self.count[kind] = self.count.get(kind, 0) + 1
        return self.reg(f"{kind}{self.count[kind]}", t)

    def name(self, p):
        p = int(p)
        if p == 0:
            return 0
        for lo, hi, name, _ in self.named:
            if lo <= p < hi:
                return f"{name}+{p - lo}"
        raise AssertionError(f"pointer {p:#x} belongs to no registered tensor")

    def scalar(self, v):
        if isinstance(v, float):
            return v
        v = int(v)
        return self.name(v) if any(lo <= v < hi for lo, hi, _, _ in self.named) else v

    def say(self, *what):
        self.log.append(["say", *what])


def play():
    """Run the scenario against the importable `uenc` and return its log (JSON-serialisable)."""
    from uenc import capi, kernels as K, ops
    R = _Recorder()
    q, cache = ops.WGRADS, ops.CACHE

    def upload_table(arr, device, pinned=True):
        names = list(arr.dtype.names)
        rows = []
        for rec in arr:
            rows.append([R.name(rec[f]) if arr.dtype[f].str == "<u8" else rec[f].item() for f in names])
        R.log.append(["table", names, rows])
        return R.auto("table", torch.empty(max(1, arr.nbytes), dtype=torch.uint8))

    def launch(entry):
        def fn(*args):
            R.log.append(["launch", entry, [R.scalar(a) for a in args]])
            return 0
        return fn

    def cast_bf16(src, out=None):
        assert src.dtype == F32 and src.is_contiguous()
        return R.auto("op", src.to(BF16)) if out is None else out.copy_(src)

    def cast_transpose_bf16(src, out=None):
        assert src.dtype == F32 and src.dim() == 2 and src.is_contiguous()
        return R.auto("op", src.t().contiguous().to(BF16))

    def relpos_expand(table, ws):
        NP = K.lib.uenc_window_attn_np(ws)
        return R.auto("bias", torch.zeros(table.shape[1], NP, NP)), None

    mods = [m for m in (capi, K, ops) if hasattr(m, "stream_ptr")]
    saved = ([(m, "stream_ptr", m.stream_ptr) for m in mods] + [(K.lib, e, getattr(K.lib, e)) for e in LAUNCHES]
             + [(K, n, getattr(K, n)) for n in ("upload_table", "cast_bf16", "cast_transpose_bf16", "relpos_expand")])
    listener, exact, chunks = ops._GRAD_LISTENER, K.EXACT, ops.SMALLQ._chunks
    try:
        ops.SMALLQ._chunks = []                 # the scenario's partial sums get an arena chunk of their own, at offset 0
        for m in mods:
            m.stream_ptr = lambda: 0
        for e in LAUNCHES:
            setattr(K.lib, e, launch(e))
        K.upload_table, K.cast_bf16, K.cast_transpose_bf16, K.relpos_expand = upload_table, cast_bf16, cast_transpose_bf16, relpos_expand
        K.EXACT = False
        ops.set_grad_listener(lambda p: R.log.append(["notify", R.name(p.data_ptr())]))
        cache.invalidate()
        q.reset()
        _queue(R, ops, q)
        _conv(R, ops)
        _ordering(R, ops, q)
        _cache(R, ops, cache)
    finally:
        for obj, name, val in saved:
            setattr(obj, name, val)
        K.EXACT = exact
        ops.set_grad_listener(listener)
        cache.invalidate()
        ops.SMALLQ._chunks = chunks
        q.reset()
    return R.log


def _param(R, name, *shape):
    return R.reg(name, torch.nn.Parameter(torch.zeros(*shape)))


def _queue(R, ops, q):
    """Both tile classes, the small class and the parked reductions gathered by hand, then ONE flush."""
    q.callback_armed = True                 # as inside a backward pass: add() queues instead of launching at once
    try:
        for i, (M, N, Kd) in enumerate(BIG):
            dy, x = R.reg(f"dy{i}", torch.empty(M, N, dtype=BF16)), R.reg(f"x{i}", torch.empty(M, Kd, dtype=BF16))
            gw, gb, p = R.reg(f"gw{i}", torch.empty(N, Kd)), R.reg(f"gb{i}", torch.empty(N)), _param(R, f"p{i}", 1)
            q.fresh = i % 2 == 0
            q.add(dy, x, gw, None if N == 96 else gb, notify=(p, None), first=q.touch(gw), alpha=0.3 + 0.25 * i)
            R.say("items", q.items[256], q.items[128])
        for i, (M, N, Kd, ty, tx) in enumerate(SMALL):
            dy, x = R.reg(f"sdy{i}", torch.empty(M, N, dtype=ty)), R.reg(f"sx{i}", torch.empty(M, Kd, dtype=tx))
            gw, gb, p = R.reg(f"sgw{i}", torch.empty(N, Kd)), R.reg(f"sgb{i}", torch.empty(N)), _param(R, f"sp{i}", 1)
            q.add_small(dy, x, gw, gb if i else None, notify=(p,), alpha=1.0 + i)
            R.say("small_items", q.small_items, len(q.small))
        sq, dev = ops.SMALLQ, torch.device("cpu")
        for i, (nblk, C) in enumerate([(4, 64), (2048, 40)]):
            part = sq.alloc(nblk * 2 * C, dev)
            if not i:
                R.reg("arena", sq._chunks[0])
            sq.add_ln(part, R.reg(f"dgamma{i}", torch.zeros(C)), R.reg(f"dbeta{i}", torch.zeros(C)), nblk, C)
        sq.add_dtable(sq.alloc(5000, dev), R.reg("dtab", torch.zeros(169, 3)), 2, 3, 7, 4)
        q.post.append(lambda: R.log.append(["post", "queue"]))
        R.say("busy", q.busy(), bool(sq), len(sq.keep))
    finally:
        q.callback_armed = False
        q.flush()
    R.say("after flush", q.items[256], q.items[128], q.small_items, len(q.small), len(q.notify), len(q.post), q.busy(), bool(ops.SMALLQ))


def _conv(R, ops):
    M, Co, Kd = CONV
    dy2, col = R.reg("cdy", torch.empty(M, Co, dtype=BF16)), R.reg("ccol", torch.empty(M, Kd, dtype=BF16))
    ops.Conv3x3Fn._wgrad_gemm(dy2, col, R.reg("cdw", torch.empty(Co, Kd)), None)


def _ordering(R, ops, q):
    """Notifications and dependent steps keep their place behind a queued GEMM; a second writer turns its store into an add."""
    pa, pb, pc = _param(R, "pa", 1), _param(R, "pb", 1), _param(R, "pc", 1)
    ops._tn_notify(pa, None)                                        # idle: fires at once
    dy, x = R.reg("ody", torch.empty(2048, 256, dtype=BF16)), R.reg("ox", torch.empty(2048, 256, dtype=BF16))
    gw, gb = R.reg("ogw", torch.empty(256, 256)), R.reg("ogb", torch.empty(256))
    q.callback_armed = True
    try:
        q.fresh = True
        first = q.touch(gw)
        q.add(dy, x, gw, gb, notify=(pb,), first=first)
        R.say("first", first, "stores", len(q.stores))
        R.say("touch again", q.touch(gw), "stores", len(q.stores))  # the queued store becomes an accumulation
        ops._tn_notify(pc)                                          # held
        ops._after_wgrads(lambda: R.log.append(["post", "after_wgrads"]), (pb,))   # held; pb is notified twice
        R.say("held", len(q.notify), len(q.post))
    finally:
        q.callback_armed = False
        q.flush()
    ops._after_wgrads(lambda: R.log.append(["post", "idle"]), (pa,))  # idle again: runs at once


def _cache(R, ops, cache):
    def state(what):
        R.say(what, "casts", cache.casts, "entries", len(cache._store))
    w, wodd = _param(R, "w", 64, 128), _param(R, "wodd", 30, 50)
    p1, p2, b1, b2 = _param(R, "p1", 32, 64), _param(R, "p2", 16, 64), _param(R, "b1", 32), _param(R, "b2", 16)
    gamma, b, table = _param(R, "gamma", 64), _param(R, "b", 64), _param(R, "table", 169, 3)
    cache.casts = 0
    made = [cache.mat(w), cache.mat_t(w, (8, 40)), cache.cat(p1, p2), cache.cat(p1, p2, True), cache.catvec(b1, b2),
            cache.scaled(w, gamma), cache.scaled(w, gamma, True), cache.scaled_vec(b, gamma), cache.vec16(b), cache.relpos(table, 7),
            cache.mat(wodd)]
    R.say("shapes", [list(t.shape) for t in made])
    assert cache.mat(w) is made[0] and cache.cat(p1, p2) is made[2] and cache.relpos(table, 7) is made[9]     # hits
    state("made")
    cache.refresh()                                     # planned entries refreshed by the two grouped launches, the others dropped
    state("refreshed")
    assert cache.mat(w) is made[0] and cache.cat(p1, p2, True) is made[3]
    state("hits")
    cache.refresh()                                     # the device tables are reused: launches only
    with torch.no_grad():
        w.add_(1.0)
    assert cache.mat(w) is not made[0]                  # the version moved without a refresh: re-made
    state("re-made")
    cache.refresh()
    state("refreshed again")
    p1.data = R.reg("p1new", torch.zeros(32, 64))       # the storage moved: both stacked operands are dropped
    cache.refresh()
    state("storage moved")
    del table, made
    gc.collect()
    cache.refresh()                                     # an owner died
    state("owner gone")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, help="the JSON file to write")
    ap.add_argument("--pkg", required=True, help="directory that holds the `uenc` package to play against")
    ap.add_argument("--rev", required=True, help="the revision that package was checked out from")
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    log = json.loads(json.dumps(play()))
    with open(a.record, "w") as f:
        json.dump({"recorded_from": a.rev, "generator": "python tests/host_queue_cases.py --record", "torch": torch.__version__,
                   "numpy": np.__version__, "log": log}, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(f"{len(log)} events -> {a.record}")
