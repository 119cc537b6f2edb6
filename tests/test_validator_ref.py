"""CPU: the fp64 restatement of the data validator's all-pairs checks (tests/validator_ref.py) is the reference's rule --
pinned to sklearn's cosine_similarity walked by the reference's double loops (src/evaluation/data_validator.py:403-415,
:519-535, restated here) and to tests/golden/data_validator.npz, which the reference's own code wrote
(tests/make_validator_fixture.py)."""
from pathlib import Path

import numpy as np
import pytest

import validator_ref

GOLDEN = Path(__file__).resolve().parent / "golden" / "data_validator.npz"


def fixture():
    z = np.load(GOLDEN)
    names = [str(n) for n in z["split_names"]]
    cuts = np.cumsum(z["split_sizes"])[:-1]
    splits = {n: [int(i) for i in part] for n, part in zip(names, np.split(z["split_indices"], cuts))}
    return z, names, splits


def rows(R, D, seed):
    """random rows of random norm with a duplicate, a scaled copy, near copies and a zero row"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((R, D)) * (10.0 ** rng.uniform(-2, 2, R))[:, None]
    if R >= 8:
        X[1] = X[0]
        X[2] = -2.5 * X[0]
        X[3] = 4.0 * X[0]
        X[5] = X[4] + 0.2 * np.linalg.norm(X[4]) / np.sqrt(D) * rng.standard_normal(D)
        X[6] = X[4] + 0.5 * np.linalg.norm(X[4]) / np.sqrt(D) * rng.standard_normal(D)
        X[7] = 0.0
    return X


@pytest.mark.parametrize("R,D,t", [(2, 8, 0.5), (9, 16, 0.95), (40, 32, 0.9), (65, 48, 0.8), (130, 24, 0.3), (50, 16, -0.1)])
def test_near_duplicates_is_sklearn_plus_the_double_loop(R, D, t):
    from sklearn.metrics.pairwise import cosine_similarity
    X = rows(R, D, R)
    S = cosine_similarity(X)
    want = [(i, j, S[i, j]) for i in range(R) for j in range(i + 1, R) if S[i, j] >= t]
    P, sims = validator_ref.near_duplicates(X, t)
    # no pair of these inputs is within 1e-9 of t, so fp64 summation orders cannot disagree on a pair
    assert np.abs(validator_ref.cosine64(X)[np.triu_indices(R, 1)] - t).min() > 1e-9
    assert [(i, j) for i, j, _ in want] == [tuple(p) for p in P.tolist()]
    assert np.allclose([s for _, _, s in want], sims, rtol=0, atol=1e-12)
    if R >= 8:
        assert (0, 1) in {tuple(p) for p in P.tolist()} and (0, 3) in {tuple(p) for p in P.tolist()}
        assert (0, 2) not in {tuple(p) for p in P.tolist()} or t <= -1
        S64 = validator_ref.cosine64(X)
        assert np.all(S64[7] == 0) and np.all(S64[:, 7] == 0)             # a zero row: cosine 0 with everything, itself included


def test_pairs_order_groups_and_offsets():
    rng = np.random.default_rng(0)
    for R in (1, 2, 33, 70):
        A = rng.random((R, R + 7)) < 0.3                                 # not symmetric, with columns beyond R
        g = rng.integers(-1, 3, R)
        for groups in (None, g):
            want = [(i, j) for i in range(R) for j in range(i + 1, R)
                    if A[i, j] and (groups is None or (g[i] >= 0 and g[j] >= 0 and g[i] != g[j]))]
            P, off = validator_ref.pairs(A, groups)
            assert P.shape == (len(want), 2) and [tuple(p) for p in P.tolist()] == want
            assert off[0] == 0 and off[-1] == len(want)
            assert all(np.all(P[off[i]:off[i + 1], 0] == i) for i in range(R))


def test_leakage_is_sklearn_plus_the_double_loop():
    from sklearn.metrics.pairwise import cosine_similarity
    X = rows(60, 24, 5)
    X[40] = X[4]; X[41] = X[5]; X[55] = 2.0 * X[0]
    split_info = {"val": [30, 31, 40, 41, 3], "train": list(range(0, 30)), "test": list(range(42, 60)) + [3, 99]}
    t = 0.8
    feats, idx, split = [], [], []
    for name, indices in split_info.items():                            # :502-514
        for i in indices:
            if i < len(X):
                feats.append(X[i]); idx.append(i); split.append(name)
    S = cosine_similarity(np.array(feats))
    want = [dict(type="image", index1=idx[i], index2=idx[j], split1=split[i], split2=split[j], similarity=S[i, j])
            for i in range(len(idx)) for j in range(i + 1, len(idx)) if split[i] != split[j] and S[i, j] >= t]
    got = validator_ref.leakage(X, split_info, t)
    assert len(want) >= 5 and len(got) == len(want)
    for a, b in zip(got, want):
        assert {k: a[k] for k in a if k != "similarity"} == {k: b[k] for k in b if k != "similarity"}
        assert abs(a["similarity"] - b["similarity"]) < 1e-12
    assert any(d["index1"] == 3 and d["index2"] == 3 for d in got)      # an index in two splits pairs with itself


def test_restatement_reproduces_the_reference_fixture():
    z, names, splits = fixture()
    X = z["features"]
    assert X.dtype == np.float32 and X.shape[1] % 64 != 0
    S64 = validator_ref.cosine64(X)
    for t in (float(z["near_t"]), float(z["leak_t"])):
        assert np.abs(S64[np.triu_indices(len(X), 1)] - t).min() > 1e-4    # the maker's condition on the inputs
    P, sims = validator_ref.near_duplicates(X, float(z["near_t"]))
    assert np.array_equal(P, z["near_pairs"])
    assert np.abs(sims - z["near_sims"]).max() <= float(z["e_ref"])
    got = validator_ref.leakage(X, splits, float(z["leak_t"]))
    assert [(d["index1"], d["index2"]) for d in got] == [tuple(p) for p in z["leak_idx"].tolist()]
    assert [(names.index(d["split1"]), names.index(d["split2"])) for d in got] == [tuple(p) for p in z["leak_split"].tolist()]
    assert np.abs(np.array([d["similarity"] for d in got]) - z["leak_sims"]).max() <= float(z["e_ref"])
    assert float(z["e_ref"]) < 1e-6                                     # the reference's fp32 similarities: a few ulps from fp64
    shared = set(splits["train"]) & set(splits["test"])
    assert shared and any(d["index1"] == d["index2"] for d in got)     # the shared index leaks into itself
    assert any(i >= len(X) for i in splits["test"])                     # and an index beyond the dataset is skipped
