"""Planted-gap data: corpora on which the CPU can say that every query MUST certify.

The suite's parity helpers compare final results, which the exact fallback repairs whenever a
guard (certificate, consistency check, int8 checksum) rejects a query: a candidate pass that is
subtly wrong then only shows as a slower search.  On the data built here a correct pass cannot be
rejected, so `fallback_queries == 0` can be asserted (tests/test_gpu_pass_alone.py).

The argument.  Query with exact sorted keys s_1 >= s_2 >= ..., gap
g = s_k - s_{k+1}, and the pass's per-row bound |a - (s - shift)| <= eps.  The certificate
(vdb_exact.hip finish_kernel) passes when a_k - eps > max(a_KP, T) + eps.  a_k >= s_k - shift - eps;
a_KP <= a_{k+1} <= s_{k+1} - shift + eps; the pilot bound T is the r-th best of 256 slot maxima
and at most k slots hold a top-k row, so for r > k it is the score of a row outside the top k:
T <= s_{k+1} - shift + eps.  Hence g > 4 eps forces certification.  `eps_upper` bounds the
finish's eps from above with the reference arithmetic alone (numpy; never the library), and
tests/test_planted_precondition.py asserts g >= 6 eps_upper on every case of `MATRIX` (the extra
2: the rerank cut's 2.001 eps and the fp32 terms the models leave out).

`i8_model` is the numpy model of the int8 kernels' arithmetic that tests/test_int8_bounds.py
checks against the exact keys; its eps is the int8 precisions' eps here.
"""
import functools

import numpy as np

from oracle import ref_cpu


def _scored_rows(V, metric):
    """(Y, nr): the rows a pass scores (cosine: normalised in fp32 as pack_rows does) and the fp64
    row norms."""
    nr = np.sqrt((V.astype(np.float64) ** 2).sum(1))
    if metric == "cosine":
        iv = (1.0 / np.maximum(nr, 1e-8)).astype(np.float32)
        return (V * iv[:, None]).astype(np.float32), nr
    return V.astype(np.float32), nr


def i8_model(V, Q, metric, prec, want_approx=True, setup=None, maxima=None):
    """(approx [N, B], eps [B], shift [B]) of the int8 pass (vdb_scan8_kernel.h, vdb_scan8.hip
    prep8, vdb_api.cpp fa.*), prec "i8", "i8x3" or "i8q".  want_approx=False skips the integer
    matmuls (approx is None): eps and shift only.

    setup: the rows [m, D] (m <= 65536) that mu, s_x and dir are derived from, where they are not
    the first min(N, 65536) rows of V (vdb_api.cpp vdb_index_add: an add that does not double the
    index keeps the earlier setup; vdb_index_update and vdb_index_remove never derive it again).
    maxima: the rows of V (index array or boolean mask) whose residuals, plane norms and norms
    enter the running maxima eps is built from; default all of them."""
    f32 = np.float32
    D = V.shape[1]
    Y, nr = _scored_rows(V, metric)
    if setup is None:
        m = min(len(V), 65536)  # setup_direction: the first kDirRows rows
        S = Y[:m]
    else:
        m = len(setup)
        assert 0 < m <= 65536, m
        S, _ = _scored_rows(np.asarray(setup, dtype=f32), metric)
    sel = slice(None) if maxima is None else maxima
    sums = S.astype(np.float64).sum(0)
    dirv = (sums / np.sqrt((sums ** 2).sum())).astype(f32)
    mu = (sums / m).astype(f32)
    Z = (Y - mu).astype(f32)
    zmax = np.abs(Z[:m]).max() if setup is None else np.abs((S - mu).astype(f32)).max()
    sx = f32(1.25 * zmax / 127) if zmax > 0 else f32(1.0)
    t = Z * (f32(1) / sx)
    xh = np.clip(np.rint(t), -127, 127)
    xl = np.clip(np.rint((t - xh) * f32(256)), -127, 127)
    r8 = Z.astype(np.float64) - np.float64(sx) * xh
    r16 = r8 - np.float64(sx) * xl / 256.0
    R8, R16 = np.sqrt((r8 ** 2).sum(1))[sel].max(), np.sqrt((r16 ** 2).sum(1))[sel].max()
    M8, M16 = np.abs(r8 @ dirv.astype(np.float64))[sel].max(), np.abs(r16 @ dirv.astype(np.float64))[sel].max()
    ZA = np.sqrt(((np.float64(sx) * xh) ** 2).sum(1))[sel].max()
    XL = np.sqrt(((np.float64(sx) * xl / 256.0) ** 2).sum(1))[sel].max()
    xmax = nr[sel].max()
    # queries (prep_queries + prep8)
    qn = np.sqrt((Q.astype(np.float64) ** 2).sum(1))
    q = (Q * (1.0 / np.maximum(qn, 1e-8)).astype(f32)[:, None]).astype(f32) if metric == "cosine" else Q.astype(f32)
    sq = f32(np.abs(q).max() / 127)
    if metric == "euclidean":
        sq = max(sq, f32(0.5 * xmax * xmax / (float(sx) * 1.0e9)))
    tq = q * (f32(1) / sq)
    qh = np.clip(np.rint(tq), -127, 127)
    ql = np.clip(np.rint((tq - qh) * f32(256)), -127, 127)
    uH = f32(sx * sq)
    uL = f32(uH * f32(1.0 / 256.0))
    approx = None
    if want_approx:
        H = xh.astype(np.int64) @ qh.T.astype(np.int64)
        if metric == "euclidean":  # H starts at rint(-|x|^2/2 / uH) per row (rinit32 in fp32)
            rinit = (f32(-0.5) * (nr ** 2).astype(f32)).astype(f32)
            H = H + np.rint((rinit * (f32(1) / uH)).astype(f32)).astype(np.int64)[:, None]
        if prec == "i8":
            half = (H.astype(f32) * uH).astype(np.float64)
        else:  # I8X3: L = xh.ql + xl.qh; I8Q (the 16-bit query on the 8-bit rows): xh.ql alone
            L = xh.astype(np.int64) @ ql.T.astype(np.int64)
            if prec == "i8x3":
                L = L + xl.astype(np.int64) @ qh.T.astype(np.int64)
            half = (H.astype(f32) * uH + L.astype(f32) * uL).astype(np.float64)
        approx = half if metric == "cosine" else 2.0 * half
    # eps (vdb_api.cpp fa.*, finish_kernel, prep8 qerr)
    x3 = prec == "i8x3"
    q16 = x3 or prec == "i8q"  # (prep8_kernel: the query residual is the 16-bit query's)
    R, M = (R16, M16) if x3 else (R8, M8)
    qd = q.astype(np.float64)
    c = qd @ dirv.astype(np.float64)
    w = np.sqrt(((qd - c[:, None] * dirv.astype(np.float64)) ** 2).sum(1))
    xres, dres = 1.01 * R, 1.01 * M  # fa.xres / fa.dres; finish_kernel's bq (min of the two bounds)
    bq = np.minimum(xres * (1.0 if metric == "cosine" else qn), (w * xres + np.abs(c) * dres) * (1 + 1e-6) + 1e-6 * xres)
    r8q = np.sqrt(((qd - np.float64(sq) * qh) ** 2).sum(1))
    r16q = np.sqrt(((qd - np.float64(sq) * (qh + ql / 256.0)) ** 2).sum(1))
    qlv = np.sqrt(((np.float64(sq) * ql / 256.0) ** 2).sum(1))
    e = (ZA + (XL if x3 else 0.0)) * (r16q if q16 else r8q) + (XL * qlv if x3 else 0.0)
    e = e + (float(uH) if metric == "euclidean" else 0.0)
    qerr = 1.01 * (e if metric == "cosine" else 2.0 * e)
    eps_rel = 1.01 * 8.0 * 2.0 ** -24
    if metric == "cosine":
        eps = eps_rel + bq + qerr
    else:  # (the finish adds 2.4e-7 max(|a_k|, |acut|) on top: left out here, a stricter check)
        eps = eps_rel * (2.0 * qn * xmax + xmax * xmax) + 2.0 * bq + qerr
    shift = (mu.astype(np.float64) @ qd.T) if metric == "cosine" else (2.0 * (mu.astype(np.float64) @ qd.T) - qn ** 2)
    return approx, eps, shift


def planted(N, D, B, k, seed):
    """(V [N, D], Q [B, D], pos [B, k]): standard-normal fp32 rows and queries; query b's k
    nearest rows, under both metrics, are planted at pos[b] (distinct positions spread over the
    corpus, disjoint between queries): (c_j q^ + sqrt(1 - c_j^2) u_j) |q| with u_j random unit
    vectors orthogonal to q and c = linspace(0.97, 0.90, k).  Needs B k <= N / 1.5."""
    assert B * k <= N / 1.5, (N, B, k)
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((N, D)).astype(np.float32)
    Q = rng.standard_normal((B, D)).astype(np.float32)
    pos = rng.permutation(N)[:B * k].reshape(B, k)
    c = np.linspace(0.97, 0.90, k)
    for b in range(B):
        q = Q[b].astype(np.float64)
        qn = np.sqrt((q ** 2).sum())
        qh = q / qn
        u = rng.standard_normal((k, D))
        u -= (u @ qh)[:, None] * qh
        u /= np.sqrt((u ** 2).sum(1))[:, None]
        V[pos[b]] = ((c[:, None] * qh + np.sqrt(1.0 - c ** 2)[:, None] * u) * qn).astype(np.float32)
    return V, Q, pos


def _bf16_rne(y):
    """fp32 -> bf16 (round to nearest even) -> fp32."""
    u = np.ascontiguousarray(y, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def eps_upper(V, Q, metric, precision):
    """An upper bound, per query, of the finish's eps for one candidate pass (DESIGN.md §3.2 as
    written there), from numpy arithmetic alone.  precision: fp32, bf16x3, bf16, i8, i8x3, i8q."""
    D = V.shape[1]
    Vd = V.astype(np.float64)
    nr = np.sqrt((Vd ** 2).sum(1))
    xmax = nr.max()
    qn = np.sqrt((Q.astype(np.float64) ** 2).sum(1))
    l2_scale = 2.0 * qn * xmax + xmax * xmax
    if precision in ("i8", "i8x3", "i8q"):
        # I8Q takes I8's eps: the corpus term is the same (vdb_api.cpp: fa.xres = i8st[0] and
        # fa.dres = i8st[1] for every precision but I8X3) and the query term smaller (prep8: za is
        # zmax_h for both, the query residual that of the 16-bit query, |r8 - ql| <= |r8| per
        # element) -- read in vdb_api.cpp / vdb_scan8.hip prep8_kernel
        _, eps, _ = i8_model(V, Q, metric, "i8x3" if precision == "i8x3" else "i8", want_approx=False)
        if metric == "euclidean":  # the L2 rounding term: |a| <= 2 |q| (|x| + |mu|) + |x|^2, |mu| <= xmax
            eps = eps + 2.4e-7 * (2.0 * l2_scale)
        return eps
    u = 2.0 ** -24
    if precision == "fp32":
        eps_rel = 1.01 * (D + 8) * u
    elif precision == "bf16x3":
        eps_rel = 1.01 * (3.0 * D * 2.0 ** -23 + 3.1 * 2.0 ** -16 + 8 * u)
    elif precision == "bf16":
        eps_rel = 1.01 * (2.0 * D * 2.0 ** -23 + 1.1 * 2.0 ** -16 + 8 * u)
    else:
        raise ValueError(precision)
    bq = np.zeros_like(qn)
    if precision == "bf16":
        # the corpus rounding in its Cauchy-Schwarz form 1.01 |q| R (the finish takes the smaller of
        # this and the directional bound): R the largest row residual |y - bf16(y)|, cosine on the
        # unit rows (both as the fp32-normalised row's residual and as the raw row's over its norm)
        res = np.sqrt(((V - _bf16_rne(V)).astype(np.float64) ** 2).sum(1))
        if metric == "cosine":
            Y = (V * (1.0 / np.maximum(nr, 1e-8)).astype(np.float32)[:, None]).astype(np.float32)
            resy = np.sqrt(((Y - _bf16_rne(Y)).astype(np.float64) ** 2).sum(1))
            bq = np.full_like(qn, 1.01 * max(resy.max(), (res / np.maximum(nr, 1e-8)).max()))
        else:
            bq = 1.01 * qn * res.max()
    if metric == "cosine":
        return eps_rel + bq
    return eps_rel * l2_scale + 2.0 * bq + 2.4e-7 * l2_scale  # |a| = |2 q.x - |x|^2| <= l2_scale


# ---- the variant matrix: the smallest shapes that still distinguish the pass variants -------------

SEVEN = ("fp32", "bf16x3", "bf16", "i8", "i8x3", "i8q", "auto")
BOTH = ("cosine", "euclidean")


def resolved(precision, metric, k):
    """The pass VDB_PREC_AUTO takes with nothing held (vdb_api.cpp search_locked): I8 up to
    k = 16; above, I8Q for L2 up to k = 100, else I8X3."""
    if precision != "auto":
        return precision
    if k <= 16:
        return "i8"
    return "i8q" if metric == "euclidean" and k <= 100 else "i8x3"


def _case(name, N, D, B, k, metric, precision, params=None, wide=0, q4=0, seed=None):
    return dict(name=name, N=N, D=D, B=B, k=k, metric=metric, precision=precision, params=dict(params or {}),
                wide=wide, q4=q4, seed=seed if seed is not None else N + 3 * D + 5 * B + 7 * k)


def _matrix():
    out = []
    for m in BOTH:
        for p in SEVEN:
            for ql in (-1, 0):  # query block in LDS / from L2; the 4-group step
                out.append(_case("short", 6000, 96, 16, 10, m, p, {"scan_qlds": ql}))
            out.append(_case("ragged", 6000, 200, 70, 10, m, p))  # Dp = 256, a ragged second query block
            out.append(_case("c2like", 4000, 768, 64, 10, m, p))  # long steps
            out.append(_case("c2like", 4000, 768, 64, 10, m, p, {"finish_split": 2}))
        for p in ("i8", "i8x3", "i8q"):
            for ql in (-1, 0):  # Dp = 192, 6 groups: the 2-deep prefetch variant
                out.append(_case("prefetch", 5000, 176, 8, 10, m, p, {"scan_qlds": ql}))
        for p in ("bf16x3", "i8"):
            for sync in (1, 2):  # lockstep / flag-gated step end
                out.append(_case("c2like", 4000, 768, 64, 10, m, p, {"scan_sync": sync}))
            out.append(_case("long", 3000, 1090, 24, 25, m, p))  # the 8-wave finish
        # k = 100.  n_wg = 64 (a knob that changes which rows a correct workgroup inserts, not the
        # kernel): each workgroup scans ceil(steps / 64) steps of contiguous rows, fewer than
        # N / 64 + 2048 rows, whatever the device's CU count; the CPU precondition checks that no
        # such window holds 64 (= KW at KP = 256, vdb_scan8_kernel.h S8_KP) of one query's planted
        # rows, so the KW rule cannot fire.
        for p in ("bf16x3", "i8x3", "i8q", "auto"):
            out.append(_case("k100", 24000, 128, 64, 100, m, p, {"n_wg": 64}))
        # ... and the split pass at KP = 256 (32-query blocks): margin 156 -> KP = next_pow2(256)
        out.append(_case("k100", 24000, 128, 64, 100, m, "bf16x3", {"n_wg": 64, "margin": 156}))
        # q4: bf16 takes KP = 128 at k = 10 by itself; bf16x3 with margin 118 (k + margin = 128)
        out.append(_case("q4", 48000, 128, 256, 10, m, "bf16", q4=1))
        out.append(_case("q4", 48000, 128, 256, 10, m, "bf16x3", {"margin": 118}, q4=1))
        # wide short rows.  pilot_rank = k + 1: still provably below the top k (the slot argument
        # above) and tight: only rows above the best row of the other 256 - k slots pass, about k
        # per query, so no 32-slot segment fills with bulk rows; n_wg = 256 fixes the segment of
        # row p at (p / 32) mod 256 (vdb_scan8w.hip: tile t -> workgroup t mod n_seg), where the CPU
        # precondition counts each query's planted rows (<= 16 per segment).  Both knobs change
        # which rows a correct kernel inserts, not the kernel.
        for p in ("i8", "i8x3", "i8q", "auto"):
            out.append(_case("wide", 20000, 128, 300, 10, m, p, {"scan_wide": 1, "pilot_rank": 11, "n_wg": 256}, wide=1))
        for p in ("i8x3", "i8q"):  # ragged D, a 512-query block
            out.append(_case("wide100", 48000, 100, 300, 100, m, p,
                             {"scan_wide": 1, "pilot_rank": 101, "n_wg": 256}, wide=1))
    # wide long rows (I8 cosine): scan8wl1 (one wave per query tile) and, small batches, the
    # split-tile forms of scan8wl.  pilot_rank = k + 1 here too: these corpora have fewer than 256
    # row tiles, so the default rank (KP = 256) finds fewer than KP pilot slots filled and sets NO
    # bound (vdb_scan.hip pilot_bound_kernel); every row then goes to the lists, which is past the
    # 4096 entries of the finish's small form (seen on the GPU: finish_small = 1 flagged all 129
    # queries as overflowed) and fills each 32-slot segment to the brim.  With rank k + 1 about k
    # rows per query pass.
    for N, D, B in ((8000, 1024, 129), (6000, 1536, 256)):
        for fs in (0, 1):
            out.append(_case("widelong", N, D, B, 10, "cosine", "i8",
                             {"scan_wide": 1, "finish_small": fs, "pilot_rank": 11}, wide=1))
    for B in (1, 5, 33):
        out.append(_case("widelong_small", 8000, 768, B, 10, "cosine", "i8", {"scan_wide": 1, "pilot_rank": 11}, wide=1))
    return out


MATRIX = _matrix()


def case_id(c):
    knobs = "-".join(f"{n}{v}" for n, v in c["params"].items())
    return f"{c['name']}-N{c['N']}-D{c['D']}-B{c['B']}-k{c['k']}-{c['metric']}-{c['precision']}" + (f"-{knobs}" if knobs else "")


@functools.lru_cache(maxsize=4)
def data(N, D, B, k, seed):
    V, Q, pos = planted(N, D, B, k, seed)
    for a in (V, Q, pos):
        a.setflags(write=False)
    return V, Q, pos


@functools.lru_cache(maxsize=8)
def oracle(N, D, B, k, seed, metric):
    """exact_search at k + 1 (once per data set and metric, shared and read-only):
    (scores [B, k], indices [B, k], keys [B, k], gap [B] = s_k - s_{k+1})."""
    V, Q, _ = data(N, D, B, k, seed)
    es, ei, ek = ref_cpu.exact_search(Q, V, k + 1, metric)
    out = (es[:, :k].copy(), ei[:, :k].copy(), ek[:, :k].copy(), ek[:, k - 1] - ek[:, k])
    for a in out:
        a.setflags(write=False)
    return out


def max_planted_in_window(pos, width):
    """The most of one query's planted rows inside any window of `width` consecutive rows."""
    worst = 0
    for p in np.sort(pos, axis=1):
        hi = np.searchsorted(p, p + width, side="left")  # rows in [p_i, p_i + width)
        worst = max(worst, int((hi - np.arange(p.size)).max()))
    return worst


def max_planted_in_segment(pos, n_seg):
    """The most of one query's planted rows in one segment of the wide pass (tile t = row / 32
    goes to workgroup t mod n_seg)."""
    seg = (pos // 32) % n_seg
    return max(int(np.bincount(s, minlength=n_seg).max()) for s in seg)
