"""CPU: tests/kmeans_ref.py (the fp64 reference the GPU k-means is measured against) agrees with the library the reference
bank itself calls, sklearn.cluster.KMeans (src/ref_bank.py:298), run as plain Lloyd from the same starting centres."""
import numpy as np
import pytest

import kmeans_ref

CASES = [(2000, 8, 64, 0), (1000, 100, 512, 1), (257, 3, 64, 4), (20, 20, 512, 3)]


@pytest.mark.parametrize("R,K,D,seed", CASES)
def test_lloyd_matches_sklearn(R, K, D, seed):
    from sklearn.cluster import KMeans
    X, C0 = kmeans_ref.blobs(R, K, D, seed)
    C, labels, inertia, n_iter, emptied = kmeans_ref.lloyd(X, C0, max_iter=300, tol=1e-4)
    # precondition: once a cluster empties, sklearn (which adjusts the donor clusters) and the helper differ by design
    assert emptied == 0
    km = KMeans(n_clusters=K, init=C0.astype(np.float64), n_init=1, algorithm="lloyd", tol=1e-4, max_iter=300).fit(X.astype(np.float64))
    assert np.array_equal(labels, km.labels_)
    assert n_iter == km.n_iter_
    assert np.abs(C - km.cluster_centers_).max() <= 1e-12
    assert abs(inertia - km.inertia_) <= 1e-12 * km.inertia_


def test_helper_pieces():
    X = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [5.0, 5.0]])
    C = np.array([[0.0, 0.0], [0.0, 0.0], [5.0, 5.0]])                 # centres 0 and 1 identical: the first wins
    labels, score, d2 = kmeans_ref.assign(X, C)
    assert labels.tolist() == [0, 0, 0, 2] and d2.tolist() == [0.0, 1.0, 1.0, 0.0]
    Cn, counts = kmeans_ref.update(X, labels, C)
    assert counts.tolist() == [3, 0, 1] and np.array_equal(Cn[1], C[1]) and np.allclose(Cn[0], [1 / 3, 1 / 3])
    offsets, order = kmeans_ref.lists(np.array([2, 0, -1, 2, 0]), 3)
    assert offsets.tolist() == [0, 2, 2, 4] and order.tolist() == [1, 4, 0, 3]
    # an emptied cluster takes the farthest row and the fit goes on
    X, C0 = kmeans_ref.blobs(300, 4, 64, 7)
    C0 = C0.copy(); C0[2] = 1e3
    C, labels, _, _, emptied = kmeans_ref.lloyd(X, C0)
    assert emptied >= 1 and np.bincount(labels, minlength=4).min() >= 1
