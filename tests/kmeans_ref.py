"""fp64 numpy reference of the k-means the engine runs (``TVCEngine.kmeans``): the same assign rule, update, stop rule and
empty-cluster rule, written the plain way.  tests/test_kmeans_ref.py pins it to sklearn's Lloyd; tests/test_gpu_kmeans.py
measures the kernels against it."""
import numpy as np


def scores(X, C):
    """x.c - |c|^2 / 2: its arg-max over the centres is the Euclidean nearest centre."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    return X @ C.T - 0.5 * (C * C).sum(1)[None, :]


def assign(X, C):
    """-> (labels [R] (first index on ties), score [R], dist2 [R] = |x - c_label|^2)."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    S = scores(X, C)
    labels = np.argmax(S, axis=1)
    d2 = ((X - C[labels]) ** 2).sum(1)
    return labels.astype(np.int64), S[np.arange(len(X)), labels], d2


def update(X, labels, C_in):
    """-> (centres [K, D], counts [K]): the mean of every cluster's rows; an empty cluster keeps its row of ``C_in``;
    labels outside [0, K) belong to no cluster."""
    X, C_in = np.asarray(X, np.float64), np.asarray(C_in, np.float64)
    K = len(C_in)
    C = C_in.copy()
    counts = np.zeros(K, np.int64)
    for j in range(K):
        m = labels == j
        counts[j] = int(m.sum())
        if counts[j]:
            C[j] = X[m].mean(0)
    return C, counts


def lists(labels, K):
    """-> (offsets [K + 1], order): the row indices grouped by cluster, ascending inside a cluster."""
    labels = np.asarray(labels)
    order = np.concatenate([np.flatnonzero(labels == j) for j in range(K)]) if K else np.zeros(0, np.int64)
    counts = np.array([(labels == j).sum() for j in range(K)], np.int64)
    return np.concatenate([[0], np.cumsum(counts)]), order


def lloyd(X, C0, max_iter=300, tol=1e-4):
    """-> (centres, labels, inertia, n_iter, emptied).  Stop when the labels did not change or the squared centre shift is
    <= tol * mean feature variance (sklearn's rule), then one final assign.  After an update the e empty clusters take the e
    rows with the largest dist2 (ties: lower row index) in ascending cluster id, the donors are not adjusted
    (``emptied`` counts the iterations in which that happened)."""
    X = np.asarray(X, np.float64)
    C = np.asarray(C0, np.float64).copy()
    tol_abs = tol * X.var(axis=0).mean()
    prev, n_iter, emptied = None, 0, 0
    for it in range(max_iter):
        labels, _, d2 = assign(X, C)
        Cn, counts = update(X, labels, C)
        empty = np.flatnonzero(counts == 0)
        if len(empty):
            emptied += 1
            far = np.argsort(-d2, kind="stable")[:len(empty)]
            Cn[empty] = X[far]
        n_iter = it + 1
        shift = ((Cn - C) ** 2).sum()
        C = Cn
        if prev is not None and np.array_equal(labels, prev):
            break
        if shift <= tol_abs:
            break
        prev = labels
    labels, _, d2 = assign(X, C)
    return C, labels, float(d2.sum()), n_iter, emptied


def blobs(R, K, D, seed):
    """-> (rows fp32 [R, D], C0 fp32 [K, D]): Gaussian blobs around max(K, 4) centres, C0 = K distinct rows."""
    rng = np.random.default_rng(seed)
    nb = max(K, 4)
    centres = rng.standard_normal((nb, D))
    X = (centres[rng.integers(0, nb, R)] + 0.3 * rng.standard_normal((R, D))).astype(np.float32)
    C0 = X[rng.choice(R, K, replace=False)]
    return X, C0
