"""The float-to-fraction rule of the Jaccard range reads (service/optimized_vector_store.py
``jaccard_threshold``): for 64-bit codes the returned (num, den) passes exactly the similarities i / u,
u <= 64, that are at or above the float's exact value -- brute force over every fraction, for exact
fractions, their neighbours by ``nextafter``, 0 and 1 -- and it is the smallest such fraction.  A pair is
passed through; what is outside [0, 1], a NaN and a bad pair raise.  No GPU."""
import math
from fractions import Fraction

import pytest

N_BITS = 64
SIMS = sorted({Fraction(i, u) for u in range(1, N_BITS + 1) for i in range(u + 1)})


def _floats():
    out = {0.0, 1.0, 0.7, 0.1, 1e-9, 1 - 1e-9}
    for d in (2, 3, 5, 7, 10, 31, 63, 64):
        for n in range(d + 1):
            t = n / d
            out.update(x for x in (t, math.nextafter(t, 0.0), math.nextafter(t, 1.0)) if 0.0 <= x <= 1.0)
    return sorted(out)


def test_float_thresholds_pass_the_same_fractions():
    from service.optimized_vector_store import jaccard_threshold
    floats = _floats()
    assert len(floats) > 300
    for t in floats:
        num, den = jaccard_threshold(t, N_BITS)
        assert 1 <= den <= N_BITS and 0 <= num <= den
        want = [s for s in SIMS if s >= Fraction(t)]
        assert [s for s in SIMS if s.numerator * den >= num * s.denominator] == want, t
        assert Fraction(num, den) == want[0], t  # the smallest similarity at or above t


def test_pairs_and_refusals():
    from service.optimized_vector_store import jaccard_threshold
    assert jaccard_threshold((2, 4), N_BITS) == (2, 4) and jaccard_threshold((1 << 17, 1 << 18), 8) == (1 << 17, 1 << 18)
    assert jaccard_threshold(0.5, 8192) == (1, 2) and jaccard_threshold(1, 8) == (1, 1) and jaccard_threshold(0, 8) == (0, 1)
    for bad in (-0.1, 1.0000001, float("nan"), float("inf"), (3, 2), (0, 0), (-1, 2), (1, (1 << 18) + 1), (1, 2, 3), (0.5, 1)):
        with pytest.raises(ValueError):
            jaccard_threshold(bad, N_BITS)
