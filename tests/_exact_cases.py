"""Fixtures for the exact path, the list merge and the top-k operator tested alone.

Every result the library returns is either certified by the finish or comes from the exact path
(vdb_exact.hip exact_scan_kernel -> vdb_merge_block.h merge_block -> finalize_kernel or the fused
tail).  tests/test_gpu_exact_alone.py drives that path, the merge kernel and the top-k operator
with the data built here, at the sizes where their loops and branches change; the comparisons are
bit for bit (oracle/ref_cpu.py), so this module holds no tolerance.
tests/test_exact_precondition.py checks, without a GPU, that each fixture is what its case claims:
that the lists are sorted and padded, that a "short" case really has fewer entries than k, that a
query meant to be flagged cannot certify, and that the oracle equals a direct computation on the
walls of ties built here.

`merge_survivors` restates merge_block's choice of branch (head threshold T, survivors, the
64 / 128 / 256 / 1024 steps), so the case tables can say which branch a case reaches and the CPU
test can assert it.
"""
import functools

import numpy as np

from oracle import ref_cpu

BOTH = ("cosine", "euclidean")
MERGE_BUF = 1024   # vdb_merge_block.h
MERGE_HEADS = 512
TOPK_CHUNK = 16384  # vdb_ops.hip
POISON_IDX = -7     # what every output buffer holds before a call (keys and scores: NaN)


def next_pow2(v):
    p = 1
    while p < v:
        p *= 2
    return p


def merge_kp(k_in, k_out):
    """vdb_merge_topk's KP."""
    return max(32, next_pow2(max(k_in, k_out)))


# =============================================================================
# A. merge lists
# =============================================================================
def pack_lists(G, k_in, per_query):
    """per_query: one (keys f64 [c], ids i64 [c], list [c]) per query -> ([G, B, k_in] keys,
    [G, B, k_in] ids): each list sorted (key desc, id asc) and padded (-inf, -1), as a search
    writes its results."""
    B = len(per_query)
    K = np.full((G, B, k_in), -np.inf)
    I = np.full((G, B, k_in), -1, np.int64)
    for b, (k, i, l) in enumerate(per_query):
        if k.size == 0:
            continue
        order = np.lexsort((i, -k, l))
        ls = l[order]
        pos = np.arange(ls.size) - np.searchsorted(ls, ls, side="left")
        assert pos.max() < k_in, "a list holds more than k_in entries"
        K[ls, b, pos] = k[order]
        I[ls, b, pos] = i[order]
    return K, I


def random_entries(rng, c, G, k_in, key_steps=64):
    """c entries with distinct ids (about half above 2^32: shard offsets are 64-bit) and finite
    keys <= 0 (so the L2 score sqrt(-key) exists) on a grid of 1 / key_steps, which repeats keys
    within and across lists; each entry in a random list with room."""
    assert c <= G * k_in, (c, G, k_in)
    ids = rng.permutation(4 * c + 16)[:c].astype(np.int64)
    high = rng.random(c) < 0.5
    ids[high] += (np.int64(1) << 33) * rng.integers(1, 100, size=int(high.sum()))
    keys = -np.round(np.abs(rng.standard_normal(c)) * key_steps) / key_steps
    lists = rng.permutation(np.repeat(np.arange(G), k_in))[:c]
    return keys, ids, lists


def random_lists(G, k_in, counts, seed):
    rng = np.random.default_rng(seed)
    return pack_lists(G, k_in, [random_entries(rng, int(c), G, k_in) for c in counts])


def merge_expected(K, I, k_out, metric):
    """(scores f32, ids i64, keys f64) [B, k_out] of vdb_merge_topk: ref_cpu.merge_topk, and the
    score finalize_kernel writes for each key (0 in an empty slot)."""
    ek, ei = ref_cpu.merge_topk(K, I, k_out)
    es = np.zeros(ek.shape, np.float32)
    v = ei >= 0
    es[v] = ref_cpu.keys_to_scores(ek[v], metric)
    return es, ei, ek


def merge_survivors(Kq, Iq, KP):
    """merge_block's branch for one query's lists [G, k_in]: (survivors c or None, branch), branch
    one of "e1" "e2" "e4" (register sorts of 64 / 128 / 256), "lds" (<= MERGE_BUF), "stream"."""
    G, k_in = Kq.shape
    if G > MERGE_HEADS:
        return None, "stream"
    u = Iq.astype(np.uint64)  # better() compares ids unsigned: the sentinel -1 is the largest
    tk, ti = -np.inf, np.uint64(0xFFFFFFFFFFFFFFFF)
    if G >= KP and KP <= MERGE_HEADS:
        o = np.lexsort((u[:, 0], -Kq[:, 0]))[KP - 1]
        tk, ti = Kq[o, 0], u[o, 0]
    c = 0
    for g in range(G):
        for e in range(k_in):
            if Iq[g, e] == -1 or tk > Kq[g, e] or (tk == Kq[g, e] and ti < u[g, e]):
                break
            c += 1
    branch = "e1" if c <= 64 else "e2" if c <= 128 else "e4" if c <= 256 else "lds" if c <= MERGE_BUF else "stream"
    return c, branch


def _mcase(name, G, k_in, k_out, counts, seed, **extra):
    return dict(name=name, G=G, k_in=k_in, k_out=k_out, counts=tuple(int(c) for c in counts), seed=seed, **extra)


def _few_valid():
    """A.1: c valid entries in all for query 0 (queries 1 and 2: c // 3 and c + 1 where they fit)
    over G lists of k_in = k_out entries (more where c needs the room).  With KP >= 128 > G the
    head threshold is (-inf, sentinel), so every valid entry survives and c is merge_block's c."""
    out = []
    for G in (1, 2, 33):
        for k_out in (100, 250, 500, 1024):
            for c in (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025):
                k_in = max(k_out, -(-c // G))
                if k_in > 1024:  # one list holds at most 1024 entries
                    continue
                cap = G * k_in
                out.append(_mcase("few", G, k_in, k_out, (c, c // 3, min(c + 1, cap)), 1000 * G + 7 * k_out + c,
                                  short=c < k_out))
    return out


FEW_VALID = _few_valid()


def _full_counts(G, k_in):
    """B = 3 with different valid counts: every list full, half the entries, five entries."""
    return (G * k_in, G * k_in // 2, min(5, G * k_in))


# A.2: the list count against the head threshold (T is real from G >= KP on) and MERGE_HEADS
LIST_COUNTS = [_mcase("heads", G, 32, 32, _full_counts(G, 32), 50 + G) for G in (1, 31, 32, 33, 511, 512, 513)] + [
    _mcase("heads", 64, 64, 64, _full_counts(64, 64), 61),
    _mcase("heads", 600, 10, 10, _full_counts(600, 10), 62),
]
# A.3: k against KP, and k_out != k_in
K_SIZES = [_mcase("k", 4, k, k, _full_counts(4, k), 300 + k)
           for k in (1, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] + [
    _mcase("k", 4, 100, 10, _full_counts(4, 100), 98),
    _mcase("k", 8, 10, 40, _full_counts(8, 10), 99),
]


def case_id(c):
    return f"{c['name']}-G{c['G']}-in{c['k_in']}-out{c['k_out']}-c{c['counts'][0]}"


def all_equal_lists(G=64, k_in=32, contiguous=False):
    """A.4: every key of every list equal (query 0; queries 1 and 2 random); the result is the k
    lowest ids.  Entries not worse than T survive, and T is the KP-th lowest list head here, so
    with the ids dealt at random only a few dozen do.  contiguous: list g holds the g-th run of
    k_in ids, as row shards do; then KP - 1 whole lists survive, which at G = k_in = 64 is 4033
    entries, over MERGE_BUF: the select path overflows into the stream path (at k_in = 32 it
    cannot: 31 lists of 32)."""
    rng = np.random.default_rng(77)
    per = []
    k, i, l = random_entries(rng, G * k_in, G, k_in)
    if contiguous:
        l = np.argsort(np.argsort(i)) // k_in
    per.append((np.full_like(k, -0.25), i, l))
    per.append(random_entries(rng, G * k_in // 2, G, k_in))
    per.append(random_entries(rng, 7, G, k_in))
    return pack_lists(G, k_in, per)


def heads_are_the_answer(G, k_in):
    """The case in which the head threshold is tight: the G list heads are the G best entries of
    all (every deeper entry is worse than every head), so with G = KP the threshold T is exactly
    the KP-th best entry and exactly KP entries survive -- a T one rank too high loses the last
    result.  Query 0: distinct head keys; query 1: every head the same key (T's id decides);
    query 2: random lists."""
    rng = np.random.default_rng(79 + G)
    per = []
    for b in range(2):
        k, i, l = random_entries(rng, G * k_in, G, k_in)
        k = k - 10.0
        heads = np.asarray([np.flatnonzero(l == g)[0] for g in range(G)])
        k[heads] = -0.5 if b else -rng.permutation(G) / (2.0 * G)
        per.append((k, i, l))
    per.append(random_entries(rng, G * k_in // 2, G, k_in))
    return pack_lists(G, k_in, per)


def tie_block_lists(G=4, k_in=32, block=30):
    """A.4: 10 entries, then `block` entries of one key spread over lists 0, 1 and 2, then worse
    entries; k_out = 25 cuts the block in its middle.  The same lists for the three queries but
    for the block's ids."""
    rng = np.random.default_rng(78)
    per = []
    for b in range(3):
        ids = rng.permutation(400)[:10 + block + 40].astype(np.int64) + (np.int64(b) << 34)
        keys = np.concatenate([-rng.random(10), np.full(block, -2.0), -3.0 - rng.random(40)])
        lists = np.concatenate([rng.integers(0, G, 10), np.arange(block) % 3, rng.integers(0, G, 40)])
        per.append((keys, ids, lists))
    return pack_lists(G, k_in, per)


# =============================================================================
# B. corpora for the exact scan
# =============================================================================
def rows(N, D, seed, dist="uniform"):
    rng = np.random.default_rng(seed)
    if dist == "uniform":
        return rng.random((N, D), dtype=np.float32)
    return rng.standard_normal((N, D)).astype(np.float32)


def row_split(N, cus, gated=False):
    """(n_wg, rows per workgroup) of vdb_api.cpp run_exact: about two workgroups per CU (the
    device-gated form: one), at least 256 rows each, the last range ragged."""
    target = max(1, cus) if gated else 2 * cus
    n_wg = min(target, max(1, N // 256))
    rpw = -(-N // n_wg)
    return -(-N // rpw), rpw


def mask_words(mask_bool, junk=False):
    """uint32 mask words (bit r & 31 of word r >> 5).  junk: the bits past N of the last word
    set, and two further all-ones words."""
    n = mask_bool.size
    bits = np.zeros(((n + 31) // 32) * 32, bool)
    bits[:n] = mask_bool
    if junk:
        bits[n:] = True
    w = np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)
    return np.concatenate([w, np.full(2, 0xFFFFFFFF, np.uint32)]) if junk else w


def big_n(kind, cus):
    """The two corpus sizes that give the merge its most lists.  "issue": 2 * 256 * CUs + 5 rows,
    which run_exact splits into 2 CUs - 1 ranges of 257 rows.  "full": the same range length and
    all 2 CUs lists, the last one 3 rows long."""
    if kind == "issue":
        return 2 * 256 * cus + 5
    return (2 * cus - 1) * 257 + 3


def _scase(name, N, D, B, k, metric, dist="uniform", force=1, mask=None, seed=None):
    return dict(name=name, N=N, D=D, B=B, k=k, metric=metric, dist=dist, force=force, mask=mask,
                seed=seed if seed is not None else 11 * (N if isinstance(N, int) else 1) + 3 * D + 5 * B + 7 * k)


def _scan_cases():
    out = []
    for m in BOTH:
        # D at the key loop's boundaries: 4 floats per lane, 256 dims per piece, 4 pieces per round
        for D in (1, 3, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4100):
            for dist in ("uniform", "normal"):
                out.append(_scase("D", 1500, D, 3, 10, m, dist))
        # N against the row split
        for j, N in enumerate((1, 2, 255, 256, 257, 511, 512, 513)):
            out.append(_scase("N", N, 24, 3, 10, m, ("uniform", "normal")[j % 2]))
        out.append(_scase("Nbig", "issue", 16, 3, 10, m))
        out.append(_scase("Nbig", "full", 16, 3, 10, m, "normal"))
        # k (KE = 32 ... 1024); up to 200 only force_exact reaches the exact path
        for j, k in enumerate((1, 32, 33, 200, 201, 256, 257, 512, 513, 1000, 1024)):
            out.append(_scase("k", 5000, 40, 2, k, m, ("uniform", "normal")[j % 2], force=int(k <= 200)))
        for B in (1, 65, 300):
            out.append(_scase("B", 1500, 24, B, 10, m, "normal"))
        # masks: a random half (4500 eligible rows: past the oracle's direct form), one whole
        # workgroup range cut out, mask words with bits past N
        out.append(_scase("mask", 9000, 24, 3, 10, m, mask="half"))
        out.append(_scase("mask", 1500, 24, 3, 10, m, "normal", mask="range"))
        out.append(_scase("mask", 1501, 24, 3, 300, m, mask="junk", force=0))
    return out


SCAN_CASES = _scan_cases()


def scan_id(c):
    return (f"{c['name']}-N{c['N']}-D{c['D']}-B{c['B']}-k{c['k']}-{c['metric']}-{c['dist']}" +
            (f"-{c['mask']}" if c["mask"] else ""))


def scan_data(c, cus):
    """(V, Q, mask bool or None, mask words or None) of a SCAN_CASES entry on a device of `cus` CUs."""
    N = big_n(c["N"], cus) if isinstance(c["N"], str) else c["N"]
    V = rows(N, c["D"], c["seed"], c["dist"])
    Q = rows(c["B"], c["D"], c["seed"] + 1, c["dist"])
    mask = words = None
    if c["mask"] == "half":
        mask = np.random.default_rng(c["seed"] + 2).random(N) < 0.5
    elif c["mask"] == "range":
        _, rpw = row_split(N, cus)
        mask = np.ones(N, bool)
        mask[rpw:2 * rpw] = False
    elif c["mask"] == "junk":
        mask = np.random.default_rng(c["seed"] + 2).random(N) < 0.7
    if mask is not None:
        words = mask_words(mask, junk=c["mask"] == "junk")
    return V, Q, mask, words


FEW_UNMASKED = ((50, 100), (100, 250), (200, 300), (300, 1024))
FEW_N, FEW_D = 9000, 24
FEW_ELIGIBLE = (0, 1, 63, 64, 65, 128, 129, 256, 257)
FEW_K = (100, 200, 300, 1024)


def few_mask(eligible, seed=5):
    """`eligible` rows of FEW_N, spread over the whole corpus."""
    mask = np.zeros(FEW_N, bool)
    mask[np.random.default_rng(seed + eligible).permutation(FEW_N)[:eligible]] = True
    return mask


def boundary_ties(N, D, cus, seed=21):
    """Identical rows rpw - 2 ... rpw + 2 (a block of equal keys straddling the first two
    workgroups' ranges); query 0 is that row.  Returns (V, Q, rpw)."""
    n_wg, rpw = row_split(N, cus)
    assert n_wg >= 2
    V = rows(N, D, seed, "normal")
    V[rpw - 2:rpw + 3] = V[rpw]
    Q = rows(3, D, seed + 1, "normal")
    Q[0] = V[rpw]
    return V, Q, rpw


def spread_copies(N=16384, D=8, copies=2100, seed=22):
    """`copies` copies of one row spread evenly over N rows; query 0 equals it, query 1 is a
    multiple of it.  Returns (V, Q, the copies' rows)."""
    V = rows(N, D, seed, "normal")
    pos = (np.arange(copies) * N) // copies
    V[pos] = V[pos[0]]
    Q = rows(3, D, seed + 1, "normal")
    Q[0] = V[pos[0]]
    Q[1] = 2.0 * V[pos[0]]
    return V, Q, pos


def scan_lists(keys, n_wg, rpw, KE, mask=None):
    """What exact_scan_kernel writes for one query with exact keys `keys`: each range's best KE
    (key desc, row asc), padded: ([n_wg, KE] keys, [n_wg, KE] rows)."""
    K = np.full((n_wg, KE), -np.inf)
    I = np.full((n_wg, KE), -1, np.int64)
    for g in range(n_wg):
        r = np.arange(g * rpw, min(len(keys), (g + 1) * rpw))
        if mask is not None:
            r = r[mask[r]]
        o = r[ref_cpu.exact_topk_from_keys(keys[r], KE)]
        K[g, :o.size], I[g, :o.size] = keys[o], o
    return K, I


def zero_rows(N=1500, D=24, seed=23):
    """Cosine with zero rows and a zero query: a zero vector's key is 0 against everything, so
    query 0 (all zero) ranks the rows in row order; query 1 is an ordinary one, for which the
    zero rows tie at key 0."""
    V = rows(N, D, seed, "normal")
    V[np.random.default_rng(seed + 2).permutation(N)[:200]] = 0.0
    Q = rows(3, D, seed + 1, "normal")
    Q[0] = 0.0
    return V, Q


def direct_search(Q, V, k, metric, mask=None):
    """exact_search without its prefilter: every row's canonical key, then the stable order."""
    B = Q.shape[0]
    out_s = np.zeros((B, k), np.float32)
    out_i = np.full((B, k), -1, np.int64)
    out_k = np.full((B, k), -np.inf)
    elig = np.arange(V.shape[0]) if mask is None else np.flatnonzero(mask)
    if elig.size == 0:
        return out_s, out_i, out_k
    Ve = V[elig]
    xn = ref_cpu.canonical_norm64(Ve) if metric == "cosine" else None
    for b in range(B):
        keys = ref_cpu.exact_keys(Q[b], Ve, metric, xn)
        sel = ref_cpu.exact_topk_from_keys(keys, k)
        out_i[b, :sel.size] = elig[sel]
        out_k[b, :sel.size] = keys[sel]
        out_s[b, :sel.size] = ref_cpu.keys_to_scores(keys[sel], metric)
    return out_s, out_i, out_k


def _plant(rng, q, cs):
    """Rows at cosines `cs` to q, of q's norm (so they are q's nearest under both metrics too)."""
    q = q.astype(np.float64)
    qn = np.sqrt((q ** 2).sum())
    qh = q / qn
    u = rng.standard_normal((len(cs), q.size))
    u -= (u @ qh)[:, None] * qh
    u /= np.sqrt((u ** 2).sum(1))[:, None]
    cs = np.asarray(cs)
    return ((cs[:, None] * qh + np.sqrt(1.0 - cs ** 2)[:, None] * u) * qn).astype(np.float32)


COPIES = 320  # more than the largest KP (256): a_KP = a_k, so no certificate can pass for any eps

# (ii) the flagged subset of a host-memory search
HOST_FLAGGED = (1, 5, 6)
HOST_D, HOST_B = 256, 9
HOST_K = (10, 150)
# the planted cosines of an unflagged query's 150 nearest rows: gaps of 0.32 below the 10th and of
# about 0.3 (to the best bulk row, near 0.27 at 256 dims) below the 150th; the int8 pass's eps on
# standard-normal rows is about 0.03 (L2: 0.03 |q|^2), and the certificate needs 4 eps
HOST_PLANT = np.concatenate([np.linspace(0.995, 0.97, 10), np.linspace(0.65, 0.60, 140)])


@functools.lru_cache(maxsize=1)
def host_flagged():
    """(V, Q, mask): 9 queries; 1, 5 and 6 each equal a row with COPIES copies spread over the
    corpus (flagged whatever the pass); each other query has its 150 nearest rows planted with a
    gap below the 10th and below the 150th that every pass certifies (the precondition test
    bounds eps).  The mask keeps the planted rows, 9 copies in 10 and half of the bulk."""
    rng = np.random.default_rng(31)
    bulk = rng.standard_normal((5000, HOST_D)).astype(np.float32)
    Q = rng.standard_normal((HOST_B, HOST_D)).astype(np.float32)
    parts, kind = [bulk], [np.zeros(5000, np.int8)]
    for b in range(HOST_B):
        if b in HOST_FLAGGED:
            parts.append(np.repeat(Q[b][None, :], COPIES, axis=0))
            kind.append(np.full(COPIES, 1, np.int8))
        else:
            parts.append(_plant(rng, Q[b], HOST_PLANT))
            kind.append(np.full(HOST_PLANT.size, 2, np.int8))
    V, kind = np.concatenate(parts), np.concatenate(kind)
    perm = rng.permutation(V.shape[0])
    V, kind = np.ascontiguousarray(V[perm]), kind[perm]
    u = rng.random(V.shape[0])
    mask = np.where(kind == 2, True, np.where(kind == 1, u < 0.9, u < 0.5))
    for a in (V, Q, mask):
        a.setflags(write=False)
    return V, Q, mask


# (iii) the device-gated fused tail
GATED_D = 16
GATED_PLANT = np.linspace(0.9995, 0.995, 10)


@functools.lru_cache(maxsize=4)
def gated(cus, B, n_flag, seed=41):
    """(V, Q, flagged): M distinct rows x COPIES copies, interleaved (row i = distinct row
    i mod M), N >= 256 cus + 64 so the gated scan runs one workgroup per CU; `n_flag` of the B
    queries each equal a distinct row; every other query has its 10 nearest rows planted (appended
    to the corpus) with a gap the bf16x3 pass certifies."""
    rng = np.random.default_rng(seed + 7 * B + n_flag)
    M = -(-(256 * cus + 64) // COPIES)
    assert M >= n_flag
    distinct = rng.standard_normal((M, GATED_D)).astype(np.float32)
    V = distinct[np.arange(M * COPIES) % M]
    Q = rng.standard_normal((B, GATED_D)).astype(np.float32)
    flagged = np.sort(rng.permutation(B)[:n_flag])
    Q[flagged] = distinct[rng.permutation(M)[:n_flag]]
    plain = [b for b in range(B) if b not in set(flagged.tolist())]
    V = np.concatenate([V] + [_plant(rng, Q[b], GATED_PLANT) for b in plain])
    for a in (V, Q, flagged):
        a.setflags(write=False)
    return np.ascontiguousarray(V), Q, flagged


def gated_mask(N, seed=43):
    """The planted tail and a random 9 in 10 of the other rows: about 288 of every distinct
    row's COPIES copies stay (the precondition test asserts more than 256)."""
    mask = np.random.default_rng(seed).random(N) < 0.9
    mask[(N // COPIES) * COPIES:] = True
    return mask


def single_wg(seed=51):
    """N = 300 (one workgroup whatever the device): 280 copies of one row among 20 others; the 5
    queries are positive multiples of that row, so each ties on all 280 copies.
    Returns (V, Q, the copies' rows)."""
    rng = np.random.default_rng(seed)
    V = rng.random((300, GATED_D), dtype=np.float32)
    other = np.sort(rng.permutation(300)[:20])
    pos = np.setdiff1d(np.arange(300), other)
    V[pos] = V[pos[0]]
    Q = np.stack([V[pos[0]] * np.float32(s) for s in (1.0, 0.9, 1.1, 1.05, 0.95)])
    return V, Q, pos


def tied_with_best(Q, V, metric, mask=None, width=COPIES + 8):
    """Per query: how many eligible rows have exactly the best eligible row's key (counted within
    the oracle's best `width` rows)."""
    _, _, ek = ref_cpu.exact_search(Q, V, width, metric, row_mask=mask)
    return (ek == ek[:, :1]).sum(axis=1)


# =============================================================================
# C. score rows for the top-k operator
# =============================================================================
TOPK_N = (1, 63, 16383, 16384, 16385, 3 * TOPK_CHUNK + 1, 512 * TOPK_CHUNK + 1)
TOPK_K = (1, 32, 33, 1000, 1024)


def topk_ks(n):
    ks = [k for k in TOPK_K if k <= n]
    if n < 1024 and n not in ks:
        ks.append(n)
    return ks


def topk_rows(rows_, n, seed):
    """Standard-normal scores, three in ten of them rounded to eighths (ties everywhere, also
    between a score's copies in different chunks)."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((rows_, n)).astype(np.float32)
    q = rng.random((rows_, n)) < 0.3
    s[q] = np.round(s[q] * 8) / 8
    return s


def topk_reference(s, k, largest):
    """[rows, k] indices: reference_topk_indices (a stable argsort) of each row with NaN taken as
    -inf, the input negated for the smallest."""
    out = np.empty((s.shape[0], k), np.int64)
    for b in range(s.shape[0]):
        x = s[b] if largest else -s[b]
        out[b] = ref_cpu.reference_topk_indices(np.where(np.isnan(x), -np.inf, x).astype(np.float32), k)
    return out


def topk_special(largest):
    """Rows of special values ([4, 2 * TOPK_CHUNK + 5]) and the k to take from each:
    0: equal values at 16383 and 16384 (a tie across a chunk boundary) as the two best;
    1: a run of 3000 equal best values, k = 1000;
    2: both infinities, -0.0 against 0.0 everywhere else;
    3: the winning infinity, zeros of both signs and one NaN (never a NaN beside the losing
       infinity: the kernel keys them equal and the contract does not say which wins)."""
    n = 2 * TOPK_CHUNK + 5
    rng = np.random.default_rng(91)
    sgn = np.float32(1.0 if largest else -1.0)
    s = rng.standard_normal((4, n)).astype(np.float32)
    s[0, [TOPK_CHUNK - 1, TOPK_CHUNK]] = sgn * np.float32(50.0)
    s[1, 15000:18000] = sgn * np.float32(40.0)
    z = rng.random(n) < 0.5
    s[2] = np.where(z, np.float32(0.0), np.float32(-0.0))
    s[2, [5, 20000]] = sgn * np.float32(np.inf)
    s[2, [7, 30000]] = -sgn * np.float32(np.inf)
    s[3] = np.where(z, np.float32(-0.0), np.float32(0.0))
    s[3, 9] = sgn * np.float32(np.inf)
    s[3, 17000] = np.float32(np.nan)
    return s, (2, 1000, 1024, 1024)


def topk_small_special(largest):
    """One row of 63 scores taken whole (k = n): the winning infinity, zeros of both signs, and
    one NaN, which must come last."""
    rng = np.random.default_rng(92)
    sgn = np.float32(1.0 if largest else -1.0)
    s = rng.standard_normal((1, 63)).astype(np.float32)
    s[0, [3, 30, 31, 50]] = np.float32(0.0), np.float32(-0.0), np.float32(0.0), np.float32(-0.0)
    s[0, 40] = sgn * np.float32(np.inf)
    s[0, 12] = np.float32(np.nan)
    return s, 63
