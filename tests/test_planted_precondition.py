"""The CPU precondition of tests/test_gpu_pass_alone.py: on the planted-gap data of every case of
the variant matrix (tests/_planted.py MATRIX), each query's gap s_k - s_{k+1} is at least
6 eps_upper, so a correct candidate pass and finish must certify it unaided (4 is the derived
requirement; 2 more for the rerank cut's 2.001 eps and the fp32 terms the models leave out).
Measured against the reference arithmetic alone -- the oracle's exact keys and numpy models of the
bounds -- never against the library.  Also the two capacity rules' data conditions: no
workgroup's row range holds KW = 64 of a query's planted rows (k = 100), no wide-pass segment
more than 16 of them.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # tests/_planted.py, under any pytest import mode
import _planted as pl  # noqa: E402


def _datasets():
    seen = {}
    for c in pl.MATRIX:
        key = (c["name"], c["N"], c["D"], c["B"], c["k"], c["seed"], c["metric"])
        seen.setdefault(key, set()).add(pl.resolved(c["precision"], c["metric"], c["k"]))
    return [(key, tuple(sorted(precs))) for key, precs in seen.items()]


DATASETS = _datasets()


@pytest.mark.parametrize("key,precisions", DATASETS,
                         ids=[f"{k[0]}-N{k[1]}-D{k[2]}-B{k[3]}-k{k[4]}-{k[6]}" for k, _ in DATASETS])
def test_gap_is_six_eps_on_every_case(key, precisions):
    name, N, D, B, k, seed, metric = key
    V, Q, pos = pl.data(N, D, B, k, seed)
    es, ei, ek, gap = pl.oracle(N, D, B, k, seed, metric)
    # the planted rows are each query's k nearest, under either metric
    np.testing.assert_array_equal(np.sort(ei, axis=1), np.sort(pos, axis=1))
    for prec in precisions:
        eps = pl.eps_upper(V, Q, metric, prec)
        ratio = float((gap / eps).min())
        print(f"{name} N {N} D {D} B {B} k {k} {metric} {prec}: min gap / eps = {ratio:.1f}")
        assert ratio >= 6.0, (prec, ratio)


def test_capacity_rules_cannot_fire_on_the_planted_rows():
    checked = set()
    for c in pl.MATRIX:
        key = (c["N"], c["D"], c["B"], c["k"], c["seed"])
        if key in checked:
            continue
        _, _, pos = pl.data(*key)
        if c["name"] == "k100":  # KW rule: a workgroup's contiguous row range (n_wg = 64)
            assert c["params"]["n_wg"] == 64
            worst = pl.max_planted_in_window(pos, c["N"] // 64 + 2048)
            print(f"k100: at most {worst} planted rows of a query in a workgroup's range (KW = 64)")
            assert worst < 64
            checked.add(key)
        elif c["name"] in ("wide", "wide100"):  # segment capacity 32 (n_wg = 256 segments)
            assert c["params"]["n_wg"] == 256 and c["params"]["pilot_rank"] == c["k"] + 1
            worst = pl.max_planted_in_segment(pos, 256)
            print(f"{c['name']}: at most {worst} planted rows of a query in a segment (32 slots)")
            assert worst <= 16
            checked.add(key)
