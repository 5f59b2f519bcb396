"""Cases that pin the graph path bit for bit (tests/test_gpu_graph_exact.py on the GPU,
tests/test_graph_precondition.py for the data conditions, on the CPU).

Data.  Rows are integer-valued fp32 in [-3, 3].  L2 queries are integer-valued, so 2 q.x - |x|^2
is an exact small integer however the kernel orders its FMAs.  Cosine queries are integer-valued
with |q|^2 a power of 4 (c entries of +-a with c a^2 in {4, 16, 64, 256}): sqrtf, the reciprocal
and q_hat = q / |q| are then exact (a power of two times integers) and so is every partial sum of
q_hat . x; the one rounding left, fl32(dot * inv|x|), is a single fp32 multiply that numpy
repeats.  Batches of more than one end with an all-zero query (cosine: every row ties at score
0, the order is pure row id).  Search graphs are built here in numpy (an L2 kNN graph, stable
order) and attached with NativeGraph.from_arrays, so the search pins do not depend on the build.

SEARCH is the matrix: the smallest shapes that still reach each branch of graph_search_kernel
(see the comment on each case).  restated(name) runs oracle.ref_cpu.graph_beam_search over a
case's batch once per process and keeps the result.
"""
import functools

import numpy as np

from oracle import ref_cpu

METRICS = ("cosine", "euclidean")
N_BASE = 3000


@functools.lru_cache(maxsize=None)
def rows(N, D, seed):
    V = np.random.default_rng(seed).integers(-3, 4, (N, D)).astype(np.float32)
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def rows64(N, D, seed):
    return rows(N, D, seed).astype(np.float64)


@functools.lru_cache(maxsize=None)
def scales(N, D, seed, metric):
    return ref_cpu._row_scales(rows(N, D, seed), metric)


def queries(metric, D, B, seed):
    """B queries; a batch of more than one ends with the all-zero query."""
    rng = np.random.default_rng(1000 + seed)
    Q = np.zeros((B, D), np.float32)
    shapes = [(c, a) for c, a in ((4, 1), (16, 1), (64, 1), (256, 1), (1, 2), (4, 2), (16, 2), (64, 2)) if c <= D]
    for b in range(B if B == 1 else B - 1):
        if metric == "cosine":
            c, a = shapes[int(rng.integers(len(shapes)))] if D < 448 else ((64, 2), (256, 1))[b % 2]
            pos = rng.choice(D, c, replace=False)
            Q[b, pos] = a * rng.choice([-1.0, 1.0], c)
        else:
            Q[b] = rng.integers(-3, 4, D)
    return Q


def knn_lists(V, R):
    """Each row's R nearest other rows by squared L2 (exact integers), ties to the lower row."""
    V = np.asarray(V, np.float64)
    N = V.shape[0]
    sq = (V * V).sum(1)
    Dm = sq[:, None] + sq[None, :] - 2.0 * (V @ V.T)
    np.fill_diagonal(Dm, np.inf)
    nbr = np.argsort(Dm, axis=1, kind="stable")[:, :R].astype(np.int32)
    if R > N - 1:
        nbr[:, N - 1:] = -1
    return nbr


@functools.lru_cache(maxsize=None)
def knn_graph(N, D, seed, R):
    return knn_lists(rows64(N, D, seed), R)


@functools.lru_cache(maxsize=None)
def dirty_graph(N, D, seed, R):
    """The kNN graph with a -1 in the middle of a list, a repeated id, or a self loop, by row."""
    nbr = knn_graph(N, D, seed, R).copy()
    r = np.arange(N)
    nbr[r % 3 == 0, 2] = -1
    nbr[r % 3 == 1, 3] = nbr[r % 3 == 1, 0]
    nbr[r % 3 == 2, 1] = r[r % 3 == 2]
    return nbr


@functools.lru_cache(maxsize=None)
def tiny_graph():
    """8 rows in two rings of 4: from an entry in the first ring the other is unreachable."""
    return np.asarray([[1, 3], [2, 0], [3, 1], [0, 2], [5, 7], [6, 4], [7, 5], [4, 6]], np.int32)


@functools.lru_cache(maxsize=None)
def hash_graph(N, seed, R):
    """Rows r, r + 16384 and r + 32768 share a visited-hash slot ((row * 2654435761) & 16383
    depends on row mod 16384 only, and is a bijection on ids below 16384), so only such rows
    ever probe: every list starts with the rows that collide with its own, then both ring
    neighbours, then random rows."""
    rng = np.random.default_rng(seed)
    nbr = rng.integers(0, N, (N, R)).astype(np.int32)
    r = np.arange(N)
    slot = 0
    for off in (16384, 32768, -16384, -32768):
        t = r + off
        ok = (t >= 0) & (t < N)
        col = nbr[:, slot]
        col[ok] = t[ok]
        slot += 1
    nbr[:, slot] = (r + 1) % N
    nbr[:, slot + 1] = (r - 1) % N
    return nbr


def spread_entries(N, E):
    return np.asarray([i * N // E for i in range(E)], np.int32)


def _case(name, D=64, R=16, ef=8, k=8, B=9, ent=64, teams=1, N=N_BASE, graph="knn", seed=7):
    return dict(name=name, D=D, R=R, ef=ef, k=k, B=B, ent=ent, teams=teams, N=N, graph=graph, seed=seed)


_SHAPES = [
    _case("base"),                                                 # entries (64) exceed ef; ties; overflow
    _case("d8-batch1", D=8, ef=63, k=1, B=1),                      # Dp = 64 from D = 8, a batch of 1
    _case("d40-r33-ent3-t2", D=40, R=33, ef=65, k=65, ent=3, teams=2),  # odd degree, beam wider than a wave
    _case("d448", D=448),                                          # nper = 14 > GS_PC: a second round of pieces
    _case("r1-ef1-ent1-t5", R=1, ef=1, k=1, ent=1, teams=5),       # degree 1, ef 1, teams clamped to 1
    _case("r64-ef256-k256", R=64, ef=256, k=256, B=1, ent=256),    # full-width lists, the widest beam
    _case("r64-ef256-k1", R=64, ef=256, k=1, B=2, ent=256),
    _case("ent256-t64", ef=63, k=63, B=2, ent=256, teams=64),      # 4 entries per team
    _case("ent256-t5", ent=256, teams=5),                          # 51 or 52 entries per team, past ef
    _case("ent3-t5", D=40, R=33, k=1, ent=3, teams=5),             # teams clamped to 3
    _case("ent64-t64-ef1", ef=1, k=1, teams=64),                   # one entry per team
    _case("ent1-t2", D=8, ef=63, k=63, ent=1, teams=2),            # teams clamped to 1
    _case("ent257", ef=63, k=63, ent=257),                         # sliced form: the last entry is never scored
    _case("ent1000-t3", ef=65, k=1, ent=1000, teams=3),            # sliced, E = 256 of 333
    _case("ent1000-t7", ent=1000, teams=7),                        # uneven slices: Ev = 143 or 142
    _case("ent1000-t256", B=2, ent=1000, teams=256),               # E = 4, Ev = 4 or 3
    _case("tiny", D=8, R=2, N=8, ent=1, graph="tiny"),             # the beam never fills: -1 / inf slots
    _case("dirty", ef=63, k=63, teams=2, graph="dirty"),           # -1 in the middle, a repeat, a self loop
    _case("hash", D=8, ef=63, k=63, N=33000, graph="hash"),        # ids past 16384: the visited hash probes
]

SEARCH = [dict(c, metric=m, name=f"{c['name']}-{m}") for c in _SHAPES for m in METRICS]
BY_NAME = {c["name"]: c for c in SEARCH}


def inputs(c):
    """(rows fp32, queries fp32 [B, D], neighbours int32 [N, R], entries int32)."""
    V = rows(c["N"], c["D"], c["seed"])
    Q = queries(c["metric"], c["D"], c["B"], c["seed"])
    if c["graph"] == "knn":
        nbr = knn_graph(c["N"], c["D"], c["seed"], c["R"])
    elif c["graph"] == "dirty":
        nbr = dirty_graph(c["N"], c["D"], c["seed"], c["R"])
    elif c["graph"] == "tiny":
        nbr = tiny_graph()
    else:
        nbr = hash_graph(c["N"], c["seed"], c["R"])
    return V, Q, nbr, spread_entries(c["N"], c["ent"])


def beam_batch(V, Q, nbr, ent, k, ef, metric, teams, sc=None, V64=None, flaw=None):
    """graph_beam_search over a batch: dict(labels [B, k], dist [B, k], iterations, visited (both
    summed over the batch, as vdb_graph_stat counts them), trace)."""
    V64 = V.astype(np.float64) if V64 is None else V64
    sc = ref_cpu._row_scales(V, metric) if sc is None else sc
    trace = {}
    labels = np.empty((Q.shape[0], k), np.int64)
    dist = np.empty((Q.shape[0], k), np.float32)
    iters = scored = 0
    for b in range(Q.shape[0]):
        labels[b], dist[b], it, sv = ref_cpu.graph_beam_search(V64, nbr, ent, Q[b], k, ef, metric, teams, scales=sc,
                                                               flaw=flaw, trace=trace)
        iters += it
        scored += sv
    return dict(labels=labels, dist=dist, iterations=iters, visited=scored, trace=trace)


@functools.lru_cache(maxsize=None)
def restated(name, flaw=None):
    c = BY_NAME[name]
    V, Q, nbr, ent = inputs(c)
    return beam_batch(V, Q, nbr, ent, c["k"], c["ef"], c["metric"], c["teams"],
                      sc=scales(c["N"], c["D"], c["seed"], c["metric"]), V64=rows64(c["N"], c["D"], c["seed"]), flaw=flaw)


def same_result(a, b):
    """Labels, distances (as fp32 bits) and both statistics."""
    return (np.array_equal(a["labels"], b["labels"]) and
            np.array_equal(a["dist"].view(np.uint32), b["dist"].view(np.uint32)) and
            a["iterations"] == b["iterations"] and a["visited"] == b["visited"])


def longest_run(visited, slots=ref_cpu.GS_VIS):
    """Longest (circular) run of occupied slots of the kernel's visited table after the rows of
    `visited` were inserted: linear probing's occupied set does not depend on insertion order."""
    ids = np.fromiter(visited, np.int64, len(visited))
    if ids.size == 0:
        return 0
    h = (ids * 2654435761) & (slots - 1)
    occ = np.zeros(slots, bool)
    uniq, first = np.unique(h, return_index=True)
    occ[uniq] = True
    rest = np.delete(h, first)
    for s in rest.tolist():  # colliding rows walk to the next free slot
        while occ[s]:
            s = (s + 1) & (slots - 1)
        occ[s] = True
    if occ.all():
        return slots
    start = int(np.flatnonzero(~occ)[0])
    o = np.roll(occ, -start).astype(np.int8)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], o, [0]])))
    return int((edges[1::2] - edges[0::2]).max()) if edges.size else 0


# ---- incremental insertion ------------------------------------------------------------------
# (name, D, degree, knn or None = attached with from_arrays, rows at the start, rows per add)
ADD = [
    ("r16-grow-then-fit", 32, 16, 16, 1500, (300, 1, 200)),  # grows the device array; then two adds that fit it
    ("r32-knn48", 32, 32, 48, 600, (150,)),
    ("attached", 32, 16, None, 600, (100,)),                 # knn falls back to the degree
    ("one-row-plus-3", 32, 16, 16, 1, (3,)),                 # N < knn + 1
]


def add_rows(D, n, seed=11):
    return rows(n, D, seed)
