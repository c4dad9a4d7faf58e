"""The host bookkeeping of a training step (ops.CACHE, ops.WGRADS, ops.SMALLQ) hands the library exactly what it did before its records
were named: tests/host_queue_cases.py plays one scenario on CPU tensors with the launch sites recorded, and the log -- every descriptor
table by field, every launch's scalars, every notification, in order -- equals the one recorded from the revision named in the golden."""
import json
import os

import host_queue_cases as HQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_bookkeeping_parent.json")


def test_bookkeeping_log_equals_the_recorded_one():
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert len(gold["recorded_from"]) == 40
    want = gold["log"]
    got = json.loads(json.dumps(HQ.play()))
    kinds = [e[0] for e in want]
    assert {"table", "launch", "notify", "post", "say"} == set(kinds) and kinds.count("table") >= 12       # the golden is the whole scenario
    assert [e[:2] for e in got if e[0] != "say"] == [e[:2] for e in want if e[0] != "say"]                  # order of all events, field names
    for i, (g, w) in enumerate(zip(got, want)):
        # the serialised form tells 1 from 1.0: integers stay integers, floats (alpha, flops, nbytes) equal to the last bit
        assert json.dumps(g) == json.dumps(w), (i, g, w)
    assert len(got) == len(want)
    # what the issue fixes about the scenario: both tile classes sorted longest token range first, the conv's floor rule
    tables = [e for e in got if e[0] == "table" and "store" in e[1]]
    for _, names, rows in tables[:2]:
        mlen = [r[names.index("mlen")] for r in rows]
        assert len(rows) == 3 and mlen == sorted(mlen, reverse=True)
    conv = dict(zip(tables[2][1], tables[2][2][0]))
    assert (conv["M"], conv["mlen"], conv["nsplit"]) == (32832, 16448, 2)


def test_retired_knobs_are_not_read(monkeypatch):
    from uenc import kernels as K, ops
    monkeypatch.setenv("UENC_WGRAD_FLUSH", "7")
    monkeypatch.setenv("UENC_DEFER_SMALL", "0")
    monkeypatch.setattr(K, "EXACT", False)
    assert ops.WgradQueue().FLUSH_ITEMS is ops.WgradQueue.FLUSH_ITEMS == {256: 4096, 128: 16384}
    assert ops.WGRADS.enabled and ops._defer() is ops.SMALLQ
    pkg = os.path.dirname(ops.__file__)
    for name in ("ops.py", "kernels.py", "dp.py"):           # nor at import time
        with open(os.path.join(pkg, name)) as f:
            src = f.read()
        assert "UENC_WGRAD_FLUSH" not in src and "UENC_DEFER_SMALL" not in src, name
