"""CPU: tests/dbscan_ref.py, the fp64 restatement the GPU tests measure against, pinned to sklearn's DBSCAN (labels and core
sets, border rows included) and its component part to scipy's connected components."""
import numpy as np
import pytest

import dbscan_ref

SHAPES = [(300, 64, "blobs", 5), (1000, 128, "blobs", 5), (2000, 512, "unit", 5), (1000, 64, "chain", 2), (1000, 64, "chain", 3),
          (4096, 768, "unit", 5), (257, 64, "unit", 3)]


def shared_border_case():
    """On the first axis: six rows at 1.1 and an arm at 0.85 (rows 0 .. 6), six rows at 0 and an arm at 0.25 (rows 8 .. 14), and two
    rows at 0.55 (7 and 15) that see both arms and nothing else.  At eps = 0.5, min_samples = 7 the groups and their arms are
    core, the arms are 0.6 apart, and the two middle rows are border rows of both clusters."""
    rng = np.random.default_rng(3)
    x = np.array([1.1] * 6 + [0.85, 0.55] + [0.0] * 6 + [0.25, 0.55])
    X = 1e-3 * rng.standard_normal((16, 64))
    X[:, 0] += x
    return X.astype(np.float32)


@pytest.mark.parametrize("R,D,kind,ms", SHAPES)
def test_restatement_equals_sklearn(R, D, kind, ms):
    cluster = pytest.importorskip("sklearn.cluster")
    X = dbscan_ref.gen(R, D, kind, 7).astype(np.float64)
    lab, core, C = dbscan_ref.labels(dbscan_ref.adjacency(X, 0.5), ms)
    want = cluster.DBSCAN(eps=0.5, min_samples=ms, algorithm="brute").fit(X)
    assert np.array_equal(np.flatnonzero(core), want.core_sample_indices_)
    assert np.array_equal(lab, want.labels_)
    assert C == want.labels_.max() + 1
    if kind == "chain":
        assert C == 1 and int((~core & (lab >= 0)).sum()) == (2 if ms == 3 else 0)      # the two ends are border rows


def test_border_rows_shared_between_two_clusters():
    cluster = pytest.importorskip("sklearn.cluster")
    X = shared_border_case().astype(np.float64)
    A = dbscan_ref.adjacency(X, 0.5)
    lab, core, C = dbscan_ref.labels(A, 7)
    assert C == 2 and not core[7] and not core[15] and core[np.r_[0:7, 8:15]].all()
    assert A[7, 6] and A[7, 14] and A[15, 6] and A[15, 14] and not A[6, 14]      # the border rows see both clusters' arms
    assert lab[:7].tolist() == [0] * 7 and lab[8:15].tolist() == [1] * 7         # the clusters did not merge
    assert lab[7] == 0 and lab[15] == 0                      # and the border rows take the lower id
    want = cluster.DBSCAN(eps=0.5, min_samples=7, algorithm="brute").fit(X)
    assert np.array_equal(lab, want.labels_) and np.array_equal(np.flatnonzero(core), want.core_sample_indices_)
    cen = dbscan_ref.centres(X, lab, C)
    assert np.allclose(cen[0], X[lab == 0].mean(0)) and cen.shape == (2, 64)
    assert dbscan_ref.centres(X, np.full(16, -1), 0) is None


@pytest.mark.parametrize("R,p", [(1, 0.0), (40, 0.02), (200, 0.004), (200, 0.02), (777, 0.006), (777, 0.02)])
def test_components_equal_scipy(R, p):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(R + int(1e4 * p))
    A = np.triu(rng.random((R, R)) < p, 1)
    A = A | A.T | np.eye(R, dtype=bool)
    lab, core, C = dbscan_ref.labels(A, 1)                   # min_samples 1: every row is core, clusters = components
    n, want = csgraph.connected_components(sparse.csr_matrix(A), directed=False)
    assert core.all() and C == n
    first = {}
    for i, c in enumerate(want):                             # scipy numbers components by first appearance too
        first.setdefault(c, len(first))
    assert np.array_equal(lab, np.array([first[c] for c in want]))


def test_bit_packing_round_trip_and_non_finite_rows():
    rng = np.random.default_rng(0)
    for R in (1, 31, 32, 33, 64, 65, 200):
        A = rng.random((R, R)) < 0.3
        P = dbscan_ref.pack_bits(A)
        assert P.dtype == np.uint32 and P.shape == (R, (R + 63) // 64 * 2)
        U = dbscan_ref.unpack_bits(P, R)
        assert np.array_equal(U[:, :R], A) and not U[:, R:].any()
    X = rng.standard_normal((10, 8)) * 0.05
    X[4, 3] = np.nan
    A = dbscan_ref.adjacency(X, 0.5)
    assert not A[4].any() and not A[:, 4].any() and A[np.arange(10) != 4][:, np.arange(10) != 4].all()
    margin, und = dbscan_ref.band(np.delete(X, 4, 0), 0.5)
    assert not und.any() and margin.shape == (9, 9)
