"""fp64 restatement of the data validator's two all-pairs checks (src/evaluation/data_validator.py:353-543), pinned to
sklearn's cosine_similarity plus the reference's double loops and to a fixture made by the reference's own code
(tests/test_validator_ref.py).  The GPU tests compare the kernels with these functions."""
import numpy as np


def pairs(A, groups=None):
    """The pair list of a bool graph A [R, >= R] in the order of ``for i: for j in range(i + 1, R)`` -> int64 [P, 2]: the set
    entries with i < j < R; with ``groups`` a pair also needs both groups >= 0 and different.  Also the exclusive prefix
    sums of the rows' counts, int64 [R + 1]."""
    A = np.asarray(A, bool)
    R = len(A)
    U = np.triu(A[:, :R], 1)
    if groups is not None:
        g = np.asarray(groups, np.int64)
        U &= (g[:, None] >= 0) & (g[None, :] >= 0) & (g[:, None] != g[None, :])
    offsets = np.zeros(R + 1, np.int64)
    offsets[1:] = np.cumsum(U.sum(1))
    return np.argwhere(U).astype(np.int64).reshape(-1, 2), offsets     # argwhere is row-major: lexicographic in (i, j)


def cosine64(X, P=None):
    """fp64 cosine of the rows of X: the full matrix, or of the listed pairs [P, 2].  A zero row has cosine 0 with everything
    (sklearn's normalisation leaves it zero); NaN propagates."""
    X = np.asarray(X, np.float64)
    n = np.sqrt((X * X).sum(1))
    n = np.where(n == 0, 1.0, n)
    if P is None:
        U = X / n[:, None]
        return U @ U.T
    P = np.asarray(P, np.int64).reshape(-1, 2)
    return (X[P[:, 0]] * X[P[:, 1]]).sum(1) / (n[P[:, 0]] * n[P[:, 1]])


def near_duplicates(X, t):
    """-> (pairs int64 [P, 2], sims fp64 [P]): every i < j with cosine >= t, in the loops' order (:407-415)."""
    S = cosine64(X)
    P, _ = pairs(S >= t)
    return P, S[P[:, 0], P[:, 1]]


def leakage(X, split_info, t, n_images=None):
    """:495-535 -- the rows concatenated split by split in ``split_info``'s own order (an index listed in two splits appears
    twice), then every i < j of that list in two different splits with cosine >= t -> a list of the reference's dicts."""
    n_images = len(X) if n_images is None else n_images
    idx, split = [], []
    for name, indices in split_info.items():
        for i in indices:
            if i < n_images:
                idx.append(int(i)); split.append(name)
    if len(idx) < 2:
        return []
    S = cosine64(np.asarray(X, np.float64)[idx])
    order = {name: k for k, name in enumerate(split_info)}
    P, _ = pairs(S >= t, [order[s] for s in split])
    return [{"type": "image", "index1": idx[i], "index2": idx[j], "split1": split[i], "split2": split[j], "similarity": float(S[i, j])}
            for i, j in P.tolist()]


def score(total, valid, n_exact, n_near, n_leak):
    """:617-646."""
    s = 100.0
    if total > 0:
        s = min(s, valid / total * 100)
    s -= 5 * n_exact + 2 * n_near + 10 * n_leak
    return max(0.0, min(100.0, s))
