"""fp64 numpy restatement of the IVF search (tvc_ivf_probe / tvc_ivf_scan, include/tvc.h) and the case generator the CPU and
GPU tests share.  Operands are taken as the kernels see them (``operands``): the bf16 values, or hi + lo of an fp32 row's bf16
planes.  tests/test_ivf_ref.py checks this file against plain numpy; tests/test_gpu_ivf.py measures the kernels against it."""
import functools

import numpy as np
import torch


def operands(X: torch.Tensor) -> np.ndarray:
    """fp64 values of rows as the kernels see them: the bf16 values, or hi + lo of the fp32 rows' bf16 planes."""
    if X.dtype == torch.bfloat16:
        return X.double().numpy()
    hi = X.bfloat16().float()
    lo = (X - hi).bfloat16().float()
    return hi.double().numpy() + lo.double().numpy()


def probe_scores(Q, C):
    """q.c - |c|^2 / 2, fp64 [M, nlist]."""
    Q, C = np.asarray(Q, np.float64), np.asarray(C, np.float64)
    return Q @ C.T - 0.5 * (C * C).sum(1)[None, :]


def probe(Q, C, nprobe):
    """-> (lists int64 [M, nprobe], score fp64 [M, nprobe]): the nprobe largest scores, ties to the lower list id, NaN scores
    never win; ranks without a list (nprobe > nlist, NaN scores) are -1 / -inf."""
    S = probe_scores(Q, C)
    M, nlist = S.shape
    S = np.where(np.isnan(S), -np.inf, S)
    order = np.argsort(-S, axis=1, kind="stable")          # stable: equal scores keep ascending ids
    lists = np.full((M, nprobe), -1, np.int64)
    score = np.full((M, nprobe), -np.inf)
    n = min(nprobe, nlist)
    lists[:, :n] = order[:, :n]
    score[:, :n] = np.take_along_axis(S, order[:, :n], 1)
    lists[score == -np.inf] = -1
    return lists, score


def scan(Q, X, probes, offsets, ids, k):
    """Exact top-k of every query over the rows of its probed lists.  X: the STORED rows (list order); ids: original index
    of every stored row or None (identity); probes: list ids, entries outside [0, nlist) are skipped.
    -> (idx int64 [M, k], sim fp64 [M, k], pos int64 [M, k]), (sim desc, idx asc), -1 / -inf / -1 padded; NaN and -inf
    similarities are never returned."""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    offsets = np.asarray(offsets, np.int64)
    nlist = len(offsets) - 1
    M = Q.shape[0]
    idx = np.full((M, k), -1, np.int64)
    sim = np.full((M, k), -np.inf)
    pos = np.full((M, k), -1, np.int64)
    for q in range(M):
        p = [np.arange(offsets[l], offsets[l + 1]) for l in probes[q] if 0 <= l < nlist]
        p = np.concatenate(p) if p else np.zeros(0, np.int64)
        if not len(p):
            continue
        s = X[p] @ Q[q]
        i = p if ids is None else np.asarray(ids, np.int64)[p]
        ok = np.isfinite(s) | (s == np.inf)
        p, s, i = p[ok], s[ok], i[ok]
        o = np.lexsort((i, -s))[:k]
        idx[q, :len(o)], sim[q, :len(o)], pos[q, :len(o)] = i[o], s[o], p[o]
    return idx, sim, pos


def search(Q, X, C, offsets, ids, nprobe, k):
    lists, _ = probe(Q, C, nprobe)
    return scan(Q, X, lists, offsets, ids, k)


def near_tie_share(sim, tau):
    """Share of (query, rank) entries whose similarity is closer than tau (scalar or per query) to the next rank's."""
    sim = np.asarray(sim)
    valid = np.isfinite(sim[:, :-1]) & np.isfinite(sim[:, 1:])
    with np.errstate(invalid="ignore"):
        gap = np.where(valid, sim[:, :-1] - sim[:, 1:], np.inf)
    t = np.broadcast_to(np.asarray(tau, np.float64).reshape(-1, 1) if np.ndim(tau) else tau, gap.shape)
    return float((gap < t).sum()) / max(1, int(np.isfinite(sim).sum()))


# ---- cases ------------------------------------------------------------------------------------------------------------
def make_rows(rng, n, D, kind, centres=None, labels=None):
    """unit: random unit rows; blobs: centre of the row's list + 0.3 noise."""
    if kind == "unit":
        X = rng.standard_normal((n, D))
        return X / np.linalg.norm(X, axis=1, keepdims=True)
    return centres[labels] + 0.3 * rng.standard_normal((n, D))


@functools.lru_cache(maxsize=None)
def probe_case(M, nlist, D, kind):
    """-> (Q fp32 tensor, C fp32 tensor): queries and centroids of a probe test."""
    # (the seed's + 1: with + 0 the fp64 reference's own share of near-tied adjacent scores at (130, 1024, 768, 32) unit is
    # 0.58 %, above the 0.5 % tests/test_ivf_ref.py requires of these inputs; the expectation at that shape is about 0.45 %)
    rng = np.random.default_rng(7 * M + 13 * nlist + D + len(kind) + 1)
    if kind == "unit":
        C = make_rows(rng, nlist, D, "unit")
        Q = make_rows(rng, M, D, "unit")
    else:
        C = rng.standard_normal((nlist, D))
        Q = make_rows(rng, M, D, "blobs", C, rng.integers(0, nlist, M))
    return torch.from_numpy(Q.astype(np.float32)), torch.from_numpy(C.astype(np.float32))


PROBE_SHAPES = [(1, 1, 128, 1), (3, 5, 128, 5), (65, 257, 128, 8), (48, 100, 512, 10), (130, 1024, 768, 32)]
KINDS = ["unit", "blobs"]
# (R, D, M, nlist, nprobe, k): the sizes the near-tie shares were measured at, plus two small ones for the 16- and 32-query
# forms of the scan kernel
SEARCH_CASES = [(3000, 128, 130, 40, 8, 20), (5000, 512, 65, 64, 64, 128), (20000, 768, 48, 100, 10, 20), (1000, 128, 70, 7, 3, 128),
                (600, 512, 9, 6, 2, 20), (900, 768, 24, 9, 3, 20)]
EDGE_LENGTHS = [0, 1, 15, 16, 17, 0, 300, 600, 513]     # the 16-row group edges, two lists longer than one 512-row chunk
EDGE_NLIST = 20
EDGE_NPROBE = 8
EDGE_DUPS = 4                                            # rows of list 6 stored again in list 7


@functools.lru_cache(maxsize=None)
def index_case(R, D, nlist, kind, bf16, shuffled=True, seed=0):
    """A hand-made index (no k-means): -> dict(X stored rows tensor, X64, C fp32 tensor, offsets int64 [nlist + 1],
    ids int64 [R] or None, labels).  Rows are dealt to lists at random; ids is a random permutation sorted inside each list."""
    rng = np.random.default_rng(seed + R + 31 * D + 7 * nlist + len(kind) + 2 * bf16)
    labels = np.sort(rng.integers(0, nlist, R))
    C = rng.standard_normal((nlist, D))
    if kind == "unit":
        C /= np.linalg.norm(C, axis=1, keepdims=True)
    X = make_rows(rng, R, D, kind, C, labels)
    return _finish(rng, X, C, labels, nlist, bf16, shuffled)


def _finish(rng, X, C, labels, nlist, bf16, shuffled):
    R = len(X)
    counts = np.bincount(labels, minlength=nlist)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ids = None
    if shuffled:
        ids = rng.permutation(R).astype(np.int64)
        for l in range(nlist):
            ids[offsets[l]:offsets[l + 1]].sort()
    Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))
    if bf16:
        Xt = Xt.bfloat16()
    return dict(X=Xt, X64=operands(Xt), C=torch.from_numpy(C.astype(np.float32)), offsets=offsets, ids=ids, labels=labels,
                max_list_rows=int(counts.max()))


@functools.lru_cache(maxsize=None)
def edge_case(D, bf16, shuffled):
    """The scan's edge index: EDGE_LENGTHS, then random lengths; EDGE_DUPS rows of list 6 are stored again in list 7 (planted
    ties).  -> the index dict plus Q (fp32 tensor [M, D]), probes (int64 [M, EDGE_NPROBE]), dup (list of (pos in 6, pos in 7))
    and the query rows ``dup_q`` aimed at each planted pair."""
    rng = np.random.default_rng(100 + D + 2 * bf16 + shuffled)
    lengths = EDGE_LENGTHS + [int(v) for v in rng.integers(1, 120, EDGE_NLIST - len(EDGE_LENGTHS))]
    labels = np.repeat(np.arange(EDGE_NLIST), lengths)
    X = make_rows(rng, len(labels), D, "unit")
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    dup = [(int(offsets[6] + 7 + 50 * j), int(offsets[7] + 530 + 11 * j)) for j in range(EDGE_DUPS)]
    for a, b in dup:
        X[b] = X[a]
    ix = _finish(rng, X, make_rows(rng, EDGE_NLIST, D, "unit"), labels, EDGE_NLIST, bf16, shuffled)
    others = [l for l in range(EDGE_NLIST) if l not in (6, 7, 8)]

    def row(first, n_other, n_skip=0):
        r = list(first) + [int(v) for v in rng.choice(others, n_other, replace=False)] + [-1] * n_skip
        r += [-1] * (EDGE_NPROBE - len(r))
        return [r[i] for i in rng.permutation(EDGE_NPROBE)]

    probes = [row([7, 6], 3) for _ in range(65)]                   # 65 queries name list 7 (and 6): two groups of 64
    probes += [row([8], 2, 2) for _ in range(33)]                  # 33 name list 8: two groups of 32
    probes += [[-1] * EDGE_NPROBE]                                 # nothing probed
    probes += [row([], 3, 4) for _ in range(6)]                    # -1 mixed with lists
    probes += [[1, -1, 2, 0, -1, 5, -1, -1]]                       # 16 rows in all: fewer than k = 20 / 128
    probes = np.array(probes, np.int64)
    Q = make_rows(rng, len(probes), D, "unit")
    dup_q = list(range(EDGE_DUPS))
    for j, (a, b) in enumerate(dup):                               # aimed at the planted pairs: they lead the result
        Q[j] = X[a] + 0.05 * Q[j]
    ix.update(Q=torch.from_numpy(Q.astype(np.float32)), probes=probes, dup=dup, dup_q=dup_q)
    return ix


@functools.lru_cache(maxsize=None)
def search_case(R, D, M, nlist, kind, bf16):
    """An index whose rows sit in the list the probe rule ranks first for them (fp64), and M queries."""
    rng = np.random.default_rng(5 * R + D + 3 * M + nlist + len(kind) + 2 * bf16)
    C = rng.standard_normal((nlist, D))
    if kind == "unit":
        C /= np.linalg.norm(C, axis=1, keepdims=True)
    X = make_rows(rng, R, D, kind, C, rng.integers(0, nlist, R))
    Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))
    if bf16:
        Xt = Xt.bfloat16()
    labels = probe_scores(operands(Xt), C.astype(np.float32)).argmax(1)
    order = np.argsort(labels, kind="stable")
    counts = np.bincount(labels, minlength=nlist)
    Xs = Xt[torch.from_numpy(order)]
    Q = make_rows(rng, M, D, kind, C, rng.integers(0, nlist, M))
    return dict(X=Xs, X64=operands(Xs), C=torch.from_numpy(C.astype(np.float32)), offsets=np.concatenate([[0], np.cumsum(counts)]),
                ids=order.astype(np.int64), max_list_rows=int(counts.max()), Q=torch.from_numpy(Q.astype(np.float32)))
