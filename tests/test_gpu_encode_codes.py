"""Binary codes derived on the device (include/vdb.h vdb_index_encode_codes / vdb_index_encode;
csrc/vdb_encode.hip).

Contract: bit j of vector x is 1 iff canonical_dot64(P[j], x) > t[j] (identity projection: (double)x[j] >
t[j]), packed least significant bit first, pad bits 0.  Every comparison is byte equality with that
oracle: vdb_index_encode in host and in device memory (the device output between guard bytes, at an
odd address), under knob encode_mfma 0 (fp32 MFMA + undecided pass) and 2 (every pair in fp64), and
vdb_index_encode_codes, with its projection and thresholds in host and in device memory and under both
knob values, through the column it attaches: a Hamming search over it must equal the search over
set_codes(oracle bytes).
"""
import ctypes

import numpy as np
import pytest

from oracle.ref_cpu import canonical_dot64

pytestmark = pytest.mark.gpu
BM, BN = 128, 128  # the GEMM's row chunk and bit block (csrc/vdb_encode_plan.h)
GUARD = 61
STATS = ("encode_calls", "encode_vectors", "encode_pairs", "encode_exact_pairs", "code_sets")


@pytest.fixture(scope="module")
def vdb():
    from service import _vdb
    assert _vdb.device_count() >= 1, "no GPU visible"
    return _vdb


def oracle(V, P, t):
    t = np.zeros(V.shape[1] if P is None else P.shape[0]) if t is None else t
    with np.errstate(all="ignore"):
        if P is None:
            bits = V.astype(np.float64) > t[None, :]
        else:
            bits = np.stack([canonical_dot64(P[j], V) > t[j] for j in range(P.shape[0])]).T
    return np.packbits(bits, axis=1, bitorder="little")


def _device(ix, V, P, t, n_bits):
    import torch
    n, nb = V.shape[0], (n_bits + 7) // 8
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dv, dp, dt = (torch.from_numpy(a.copy()).to("cuda") if a is not None else None for a in (V, P, t))
        buf = torch.full((n * nb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        ix.encode_device(dv.data_ptr(), n, dp.data_ptr() if dp is not None else 0, dt.data_ptr() if dt is not None else 0,
                         n_bits, buf.data_ptr() + GUARD, stream=st.cuda_stream)
    st.synchronize()
    b = buf.cpu().numpy()
    assert (b[:GUARD] == 0xA5).all() and (b[-GUARD:] == 0xA5).all(), "guard bytes written"
    return b[GUARD:-GUARD].reshape(n, nb)


def _attach(ix, P, t, n_bits, mem):
    if mem == "host":
        return ix.encode_codes(P, t)
    import torch
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):  # the uploads are queued on st: the call must order itself after them
        dp, dt = (torch.from_numpy(a.copy()).to("cuda") if a is not None else None for a in (P, t))
        ix.encode_codes_device(dp.data_ptr() if dp is not None else 0, dt.data_ptr() if dt is not None else 0, n_bits,
                               stream=st.cuda_stream)


def _check(vdb, V, P, t, column=True, metric="cosine"):
    """-> (pairs, fp64 pairs of one knob-0 host encode).  column: V can be stored (it is finite)."""
    n, dim = V.shape
    n_bits = dim if P is None else P.shape[0]
    want = oracle(V, P, t)
    ix = vdb.NativeIndex(dim, metric)
    exact = None
    if column:
        ix.add(V)
        Q, k = want[:: max(1, n // 4)], min(n, 8)
        ix.set_codes(want)
        ref = ix.search_hamming(Q, k)
    for knob in (0, 2):
        ix.set_param("encode_mfma", knob)
        e0 = ix.stat("encode_exact_pairs")
        np.testing.assert_array_equal(ix.encode(V, P, t), want, err_msg=f"host, knob {knob}")
        paid = ix.stat("encode_exact_pairs") - e0
        if knob == 0:
            exact = paid
        elif P is not None:
            assert paid == n * n_bits
        np.testing.assert_array_equal(_device(ix, V, P, t, n_bits), want, err_msg=f"device, knob {knob}")
        for mem in ("host", "device") if column else ():
            ix.set_codes(None)
            e0 = ix.stat("encode_exact_pairs")
            _attach(ix, P, t, n_bits, mem)
            assert (ix.stat("code_rows"), ix.stat("code_bytes")) == (n, want.shape[1])
            if knob == 2 and P is not None:
                assert ix.stat("encode_exact_pairs") - e0 == n * n_bits
            for g, w in zip(ix.search_hamming(Q, k), ref):
                np.testing.assert_array_equal(g, w, err_msg=f"column, {mem}, knob {knob}")
    ix.close()
    return n * n_bits, exact


# rows: 1, 33, 64, 65, one past the row chunk; dims: 1, 33 (ragged K), 64, 257 (second canonical pass), 768
# once; bits: 8, 20 (pad bits), 32, 40, 72, one past the bit block, 8 192 at a small dim
@pytest.mark.parametrize("rows,dim,bits,metric", [
    (1, 1, 8, "cosine"), (33, 33, 20, "cosine"), (33, 33, 20, "euclidean"), (64, 64, 32, "cosine"), (65, 257, 40, "cosine"),
    (BM + 1, 33, 72, "euclidean"), (65, 64, BN + 1, "cosine"), (33, 768, 72, "cosine"), (5, 8, 8192, "cosine")])
def test_standard_normal(vdb, rows, dim, bits, metric):
    rng = np.random.default_rng(rows * 1000 + bits)
    V = rng.standard_normal((rows, dim), dtype=np.float32)
    P = rng.standard_normal((bits, dim), dtype=np.float32)
    t = 0.1 * rng.standard_normal(bits) if bits % 16 else None
    pairs, exact = _check(vdb, V, P, t, metric=metric)
    if dim > 1:  # (one dim: a - t is its own margin's size whenever both are tiny; nothing to assert)
        assert exact < pairs, "the fp32 path decided nothing"


@pytest.mark.parametrize("dim", [8, 70])
def test_sign(vdb, dim):
    rng = np.random.default_rng(dim)
    V = rng.standard_normal((65, dim), dtype=np.float32)
    t = rng.standard_normal(dim)
    t[0], t[1] = V[3, 0], np.nan  # on the threshold: 0; a NaN threshold: 0
    assert _check(vdb, V, None, None)[1] == 0
    _check(vdb, V, None, t)
    V[1, 2], V[2, 3], V[4, 5] = np.nan, np.inf, -np.inf
    _check(vdb, V, None, t, column=False)


def test_integers_on_the_bound(vdb):
    """Integers up to +-250 at 33 dims: every fp32 partial sum is an integer below 2^24, so the GEMM is
    exact, while the margin's leading term crel |p| |x| (csrc/vdb_encode_plan.h) is above 1 for every
    chosen pair.  t_j is the sum of (row j, bit j) for even j and that sum - 1 for odd j: s == t gives 0,
    s == t + 1 gives 1, and both are inside the margin.  Each chosen pair is encoded alone, so exactly
    one pair per call must pay fp64; then the whole matrix goes through the usual check."""
    rng = np.random.default_rng(5)
    V = rng.integers(-250, 251, (40, 33)).astype(np.float32)
    P = rng.integers(-250, 251, (40, 33)).astype(np.float32)
    V64, P64 = V.astype(np.float64), P.astype(np.float64)
    assert 33 * 250 * 250 < 2 ** 24
    crel = 2.02 * (33 + 8) * 2.0 ** -24
    assert (crel * np.linalg.norm(V64, axis=1) * np.linalg.norm(P64, axis=1)).min() > 1.0
    t = (V64 * P64).sum(axis=1) - (np.arange(40) & 1)
    ix = vdb.NativeIndex(33, "cosine")
    for j in range(40):
        e0 = ix.stat("encode_exact_pairs")
        assert ix.encode(V[j:j + 1], P[j:j + 1], t[j:j + 1])[0, 0] == (j & 1), j
        assert ix.stat("encode_exact_pairs") - e0 == 1, j
    ix.close()
    _check(vdb, V, P, t)


@pytest.mark.parametrize("kind", ["tiny", "huge", "nonfinite"])
def test_scaled_and_non_finite(vdb, kind):
    rng = np.random.default_rng(9)
    V = rng.standard_normal((65, 70), dtype=np.float32)
    P = rng.standard_normal((40, 70), dtype=np.float32)
    t = None
    if kind == "nonfinite":
        V[0, 1], V[1, 69], V[2, 5], V[3] = np.nan, np.inf, -np.inf, 0.0
        P[7, 3] = np.inf
        t = np.zeros(40)
        t[1], t[2], t[3] = np.nan, np.inf, -np.inf
    else:
        V *= np.float32(2.0 ** (-70 if kind == "tiny" else 63))
    _check(vdb, V, P, t, column=kind != "nonfinite")


def test_column_lifetime_and_stats(vdb):
    rng = np.random.default_rng(2)
    V = rng.standard_normal((130, 64), dtype=np.float32)
    P = rng.standard_normal((72, 64), dtype=np.float32)
    ix = vdb.NativeIndex(64, "cosine")
    ix.add(V)
    before = [ix.stat(s) for s in STATS]
    ix.encode_codes(P)
    after = [ix.stat(s) for s in STATS]
    assert [a - b for a, b in zip(after, before)][:3] == [1, 130, 130 * 72] and after[4] == before[4] + 1
    assert ix.stat("code_rows") == 130 and ix.stat("code_bytes") == 9
    ix.add(V[:3])
    assert ix.stat("code_rows") == 0, "an add drops the column"
    ix.encode_codes()  # the identity: 64 bits
    assert ix.stat("code_rows") == 133 and ix.stat("code_bytes") == 8
    ix.close()


def test_validation_moves_no_stat(vdb):
    ix = vdb.NativeIndex(16, "cosine")
    V = np.ones((4, 16), np.float32)
    ix.add(V)
    P = np.ones((8, 16), np.float32)
    out = np.zeros((4, 1), np.uint8)
    before = [ix.stat(s) for s in STATS]
    lib, h, vp = ix._lib, ix._h, ctypes.c_void_p
    raw = [  # (call, args): bad mem, NULL vectors, NULL out_codes
        (lib.vdb_index_encode, (h, vp(V.ctypes.data), 4, vp(P.ctypes.data), None, 8, 7, vp(out.ctypes.data), None)),
        (lib.vdb_index_encode, (h, None, 4, vp(P.ctypes.data), None, 8, 0, vp(out.ctypes.data), None)),
        (lib.vdb_index_encode, (h, vp(V.ctypes.data), 4, vp(P.ctypes.data), None, 8, 0, None, None)),
        (lib.vdb_index_encode, (h, vp(V.ctypes.data), -1, vp(P.ctypes.data), None, 8, 0, vp(out.ctypes.data), None)),
        (lib.vdb_index_encode_codes, (h, vp(P.ctypes.data), None, 8, 7, None)),
    ]
    for fn, args in raw:
        assert fn(*args) == vdb.VDB_ERR_INVALID, args
    for bits in (0, 8193, 15):  # out of range twice; the identity needs n_bits == dim
        with pytest.raises(ValueError):
            ix.encode(V, None, None, bits)
        with pytest.raises(ValueError):
            ix.encode_codes(None, None, bits)
    for knob in (1, 3, -1):
        with pytest.raises(ValueError):
            ix.set_param("encode_mfma", knob)
    assert [ix.stat(s) for s in STATS] == before
    assert ix.encode(V[:0], P).shape == (0, 1)  # n == 0 is fine
    ix.close()
