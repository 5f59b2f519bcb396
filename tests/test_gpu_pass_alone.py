"""Each candidate-pass variant, alone: on planted-gap data (tests/_planted.py) the pass and the
finish must produce the exact answer without any of the safety nets behind them.

The parity helpers elsewhere compare final results, which the exact fallback repairs whenever the
certificate, the finish's approx-vs-exact consistency guard or the int8 checksum rejects a query:
a pass that is subtly wrong (a ragged last tile, a dropped dimension group, a stale operand in one
prefetch variant, a bound too small) would only make the search slower.  Here every query's gap
s_k - s_{k+1} is at least 6 eps (tests/test_planted_precondition.py, on the CPU against the
reference arithmetic alone; 4 eps forces certification), so for every variant of
the matrix (_planted.MATRIX: the smallest shapes that still distinguish the variants)
  (a) indices and fp64 keys equal the oracle's, bit for bit,
  (b) no query fell back, overflowed, was flagged inconsistent or re-passed,
  (c) the intended pass ran,
and with (b), (a) is a statement about the pass and the finish only.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # tests/_planted.py, under any pytest import mode
import _planted as pl  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


def _index(vdb, c, V):
    ix = vdb.NativeIndex(c["D"], c["metric"], precision=c["precision"])
    for name, value in c["params"].items():
        ix.set_param(name, value)
    ix.add(V)
    return ix


def _assert_exact(ix, c):
    """(a): one host-memory search, indices / fp64 keys / scores bit-exact against the oracle."""
    V, Q, _ = pl.data(c["N"], c["D"], c["B"], c["k"], c["seed"])
    es, ei, ek, _ = pl.oracle(c["N"], c["D"], c["B"], c["k"], c["seed"], c["metric"])
    s, i, kk = ix.search(Q, c["k"], with_keys=True)
    np.testing.assert_array_equal(i, ei)
    np.testing.assert_array_equal(kk, ek)
    np.testing.assert_array_equal(s, es)


def _assert_unaided(ix):
    """(b): no safety net took part."""
    st = {n: ix.stat(n) for n in ("fallback_queries", "overflow_queries", "inconsistent_queries", "repass_queries")}
    assert all(v == 0 for v in st.values()), st


def _assert_pass(ix, c):
    """(c): the intended pass ran, once."""
    prec = pl.resolved(c["precision"], c["metric"], c["k"])
    ran = {p: ix.stat(f"searches_{p}") for p in ("fp32", "bf16x3", "bf16", "i8", "i8x3", "i8q")}
    assert ran == {p: int(p == prec) for p in ran}, (prec, ran)
    assert ix.stat("searches") == 1
    assert ix.stat("searches_wide") == c["wide"], ix.stat("searches_wide")
    assert ix.stat("searches_q4") == c["q4"], ix.stat("searches_q4")
    if c["precision"] == "auto":
        assert ix.stat("auto_hold") == 0 and ix.stat("auto_hold8") == 0


@pytest.mark.parametrize("c", pl.MATRIX, ids=[pl.case_id(c) for c in pl.MATRIX])
def test_pass_alone_is_exact(vdb, c):
    V, _, _ = pl.data(c["N"], c["D"], c["B"], c["k"], c["seed"])
    ix = _index(vdb, c, V)
    _assert_exact(ix, c)
    _assert_unaided(ix)
    _assert_pass(ix, c)
    ix.close()


@pytest.fixture
def debug_knobs(monkeypatch):
    """The test-only corruption knobs (debug_*) are refused unless VDB_DEBUG_KNOBS=1."""
    monkeypatch.setenv("VDB_DEBUG_KNOBS", "1")


SHORT_L2 = {p: next(c for c in pl.MATRIX if c["name"] == "short" and c["metric"] == "euclidean" and
                    c["precision"] == p and c["params"]["scan_qlds"] == -1) for p in ("i8", "bf16x3")}


@pytest.mark.parametrize("precision", ["i8", "bf16x3"])
def test_stats_see_a_stale_operand_the_results_hide(vdb, precision, debug_knobs):
    """Teeth: a stale L2 start value (debug_stale_rinit, the operand class of the round-3 failure)
    on a row outside every query's top k over-scores that row by |x|^2; the consistency guard
    sends the query it reaches to the exact path, so (a) still holds -- and (b) raises.

    The guard sees reranked rows only (approx >= a_k - 2 eps), and on normal data a stale bulk row
    scores 2 q.x, near 0, far below most queries' planted rows: the row taken is the bulk row whose
    2 q.x exceeds some query's k-th honest score 2 q.x_k - |x_k|^2 by most (checked here on the
    CPU to be above it), which puts it into that query's approximate top k."""
    c = SHORT_L2[precision]
    V, Q, pos = pl.data(c["N"], c["D"], c["B"], c["k"], c["seed"])
    _, _, ek, _ = pl.oracle(c["N"], c["D"], c["B"], c["k"], c["seed"], c["metric"])
    stale = 2.0 * V.astype(np.float64) @ Q.T.astype(np.float64)  # [N, B]: the score with -|x|^2 / 2 read as 0
    stale[pos.ravel()] = -np.inf  # not a top-k row of any query
    lift = stale - (ek[:, -1] + (Q.astype(np.float64) ** 2).sum(1))[None, :]  # keys are -|x - q|^2
    row = int(np.unravel_index(lift.argmax(), lift.shape)[0])
    assert lift.max() > 0.0
    ix = _index(vdb, c, V)
    _assert_exact(ix, c)
    _assert_unaided(ix)
    ix.set_param("debug_stale_rinit", row)
    _assert_exact(ix, c)
    with pytest.raises(AssertionError):
        _assert_unaided(ix)
    assert ix.stat("inconsistent_queries") >= 1
    ix.close()


def test_stats_see_an_under_scored_row_the_results_hide(vdb, debug_knobs):
    """Teeth: each query's top-1 row with its int8 planes overwritten (debug_sink_row8; the column
    sums stay): the pass's checksum flags the queries, the exact path answers, (a) holds and (b)
    raises."""
    c = SHORT_L2["i8"]
    V, _, _ = pl.data(c["N"], c["D"], c["B"], c["k"], c["seed"])
    _, ei, _, _ = pl.oracle(c["N"], c["D"], c["B"], c["k"], c["seed"], c["metric"])
    ix = _index(vdb, c, V)
    _assert_exact(ix, c)
    _assert_unaided(ix)
    for r in sorted(set(ei[:, 0].tolist())):
        ix.set_param("debug_sink_row8", int(r))
    _assert_exact(ix, c)
    with pytest.raises(AssertionError):
        _assert_unaided(ix)
    assert ix.stat("inconsistent_queries") == c["B"]
    ix.close()
