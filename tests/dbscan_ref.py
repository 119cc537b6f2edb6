"""fp64 numpy restatement of the DBSCAN the engine runs (``TVCEngine.dbscan``), written the plain way: the eps-graph, the
labels as a closed form of that graph, the cluster means, and the band inside which the GPU's fp32 distance test may fall on
either side.  tests/test_dbscan_ref.py pins it to sklearn's DBSCAN and scipy's connected components; tests/test_gpu_dbscan.py
measures the kernels against it."""
import numpy as np


def dist2(X64):
    """|x_i - x_j|^2 = |x_i|^2 + |x_j|^2 - 2 x_i.x_j in fp64, the diagonal exactly 0."""
    X = np.asarray(X64, np.float64)
    n2 = (X * X).sum(1)
    d2 = n2[:, None] + n2[None, :] - 2.0 * (X @ X.T)
    np.fill_diagonal(d2, 0.0)
    return d2


def adjacency(X64, eps):
    """A[i, j] = (|x_i - x_j|^2 <= eps^2), self included; a row with a non-finite entry has no neighbours, not even itself."""
    X = np.asarray(X64, np.float64)
    finite = np.isfinite(X).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        A = dist2(np.where(finite[:, None], X, 0.0)) <= float(eps) ** 2
    return A & finite[:, None] & finite[None, :]


def labels(A, min_samples):
    """-> (labels [R], core [R], n_clusters).  Core rows have degree >= min_samples; clusters are the connected components of
    the core-core graph numbered in ascending order of their lowest core index; a non-core row with a core neighbour takes the
    lowest id among them; the rest is -1."""
    A = np.asarray(A, bool)
    R = len(A)
    core = A.sum(1) >= min_samples
    comp = np.where(core, np.arange(R), R)
    Ac = A & core[None, :] & core[:, None]
    while True:                                   # plain minimum-label propagation to its fixed point
        new = np.minimum(comp, np.where(Ac, comp[None, :], R).min(1)) if R else comp
        new = np.where(core, new, R)
        if np.array_equal(new, comp):
            break
        comp = np.where(core, new[np.minimum(new, R - 1)], R)      # one pointer jump
    roots = np.flatnonzero(core & (comp == np.arange(R)))
    cid = np.full(R + 1, -1, np.int64)
    cid[roots] = np.arange(len(roots))
    out = np.full(R, -1, np.int64)
    out[core] = cid[comp[core]]
    big = np.iinfo(np.int64).max
    best = np.where(A & core[None, :], np.where(core, out, big)[None, :], big).min(1) if R else np.zeros(0, np.int64)
    border = ~core & (best < big)
    out[border] = best[border]
    return out, core, len(roots)


def centres(X64, lab, n_clusters):
    """The mean of all rows labelled c, core and border, c ascending; None without a cluster."""
    if n_clusters == 0:
        return None
    X = np.asarray(X64, np.float64)
    return np.stack([X[lab == c].mean(0) for c in range(n_clusters)])


def tau(X64):
    """tau_ij = 8e-6 |x_i| |x_j| + 2^-20 (|x_i|^2 + |x_j|^2): twice the 4e-6 |x| |c| score bound of tests/test_gpu_kmeans.py
    (the factor 2 of d^2), plus the fp32 rounding of two D-term norm sums for D <= 1 024."""
    n = np.linalg.norm(np.asarray(X64, np.float64), axis=1)
    return 8e-6 * n[:, None] * n[None, :] + 2.0 ** -20 * (n[:, None] ** 2 + n[None, :] ** 2)


def band(X64, eps):
    """-> (margin [R, R] = |d^2 - eps^2| / tau, undecided [R, R] bool).  A pair is decided when margin > 1; the diagonal always is."""
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = np.abs(dist2(X64) - float(eps) ** 2) / tau(X64)
    und = ~(margin > 1.0)
    np.fill_diagonal(und, False)
    return margin, und


def pack_bits(A):
    """bool [R, R] -> the bitmask uint32 [R, round_up(R, 64) / 32]: bit (j & 31) of word j // 32 of row i = A[i, j]."""
    A = np.asarray(A, bool)
    R = len(A)
    W = (R + 63) // 64 * 2
    P = np.zeros((R, W * 32), bool)
    P[:, :R] = A
    return np.packbits(P.reshape(R, W, 32), axis=2, bitorder="little").view(np.uint32).reshape(R, W)


def unpack_bits(words, R):
    """the inverse of pack_bits, padding included: uint32 [R, W] -> bool [R, 32 W]."""
    w = np.ascontiguousarray(words).view(np.uint8).reshape(len(words), -1)
    return np.unpackbits(w, axis=1, bitorder="little").astype(bool)


def gen(R, D, kind, seed):
    """fp32 [R, D]: 'blobs' (centres on the unit sphere, per-row spread 0.03 / 0.045 / 0.06), 'unit' (unit-norm rows around
    such centres) or 'chain' (a randomly permuted chain with 0.4 between neighbours)."""
    rng = np.random.default_rng(seed)
    if kind == "chain":
        X = np.zeros((R, D))
        X[rng.permutation(R), 0] = 0.4 * np.arange(R)
        X[:, 1:] = 0.01 * rng.standard_normal((R, D - 1))
        return X.astype(np.float32)
    K = max(2, R // (40 if kind == "blobs" else 30))
    C = rng.standard_normal((K, D))
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    if kind == "blobs":
        X = C[rng.integers(K, size=R)] + rng.standard_normal((R, D)) * rng.choice([0.03, 0.045, 0.06], size=(R, 1))
    elif kind == "unit":
        X = C[rng.integers(K, size=R)] + rng.standard_normal((R, D)) * (0.36 / np.sqrt(D))
        X /= np.linalg.norm(X, axis=1, keepdims=True)
    else:
        raise ValueError(kind)
    return X.astype(np.float32)
