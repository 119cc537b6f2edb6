"""CPU: the numpy restatement of the retrieval evaluation (tests/retrieval_ref.py) against the REFERENCE's own outputs
(tests/golden/retrieval_eval.npz, written by tests/make_retrieval_fixture.py with src/utils/metrics.py).  Both forms of the
restatement -- positions from labels, and the dense loops -- must give the reference's numbers; 1e-12 is the room of a
differently ordered fp64 sum of at most 200 terms of size <= 1."""
from pathlib import Path

import numpy as np
import pytest

import retrieval_ref as R

G = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def fx():
    z = np.load(G / "retrieval_eval.npz")
    d = {k: z[k] for k in z.files}
    d["ks"] = [int(k) for k in d["k_values"]]
    d["want"] = np.concatenate([d["recall_at_k"], d["precision_at_k"], d["ndcg_at_k"], [d["map_score"], d["mrr"]]])
    return d


def test_fixture_shape_and_cases(fx):
    assert fx["queries"].shape == (40, 96) and fx["gallery"].shape == (200, 96) and fx["cosine"].shape == (40, 200)
    assert fx["ks"] == [1, 5, 10, 20, 50]
    rel = R.relevance(fx["qlabel"], fx["glabel"])
    assert (fx["qlabel"] < 0).any() and (fx["glabel"] < 0).any()
    assert (~np.isin(fx["qlabel"][fx["qlabel"] >= 0], fx["glabel"])).any()          # a label absent from the gallery
    assert (rel.sum(1) == 0).sum() >= 4
    assert float(fx["min_gap"]) > 1e-5
    assert rel[:, fx["glabel"] < 0].sum() == 0 and rel[fx["qlabel"] < 0].sum() == 0


def test_dense_restatement_equals_the_reference(fx):
    got = R.flatten(R.dense(fx["cosine"], R.relevance(fx["qlabel"], fx["glabel"]), fx["ks"]), fx["ks"])
    assert np.abs(got - fx["want"]).max() <= 1e-12


def test_positions_restatement_equals_the_reference(fx):
    got = R.flatten(R.from_labels(fx["cosine"], fx["qlabel"], fx["glabel"], fx["ks"]), fx["ks"])
    assert np.abs(got - fx["want"]).max() <= 1e-12


def test_positions_in_fp64_are_the_reference_matrix_positions(fx):
    """The gap of the fixture means the fp32 rounding of the reference's matrix moved no relevant row."""
    q, g = fx["queries"].astype(np.float64), fx["gallery"].astype(np.float64)
    S64 = (q / np.linalg.norm(q, axis=1, keepdims=True)) @ (g / np.linalg.norm(g, axis=1, keepdims=True)).T
    a, b = R.positions(S64, fx["qlabel"], fx["glabel"]), R.positions(fx["cosine"], fx["qlabel"], fx["glabel"])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_positions_ties_nan_and_empty():
    S = np.array([[1.0, 2.0, 2.0, np.nan, 0.5],
                  [0.0, 0.0, 0.0, 0.0, 0.0]])
    off, rows, pos = R.positions(S, [7, 7], [7, -1, 7, 7, 9])
    # query 0 ranks 1, 2, 0, 4, 3 (the NaN last); its relevant rows 0, 2, 3 sit at 2, 1, 4.  Query 1: all tied, row order.
    assert off.tolist() == [0, 3, 6]
    assert rows.tolist() == [2, 0, 3, 0, 2, 3] and pos.tolist() == [1, 2, 4, 0, 2, 3]
    off, rows, pos = R.positions(S, [-1, 8], [7, -1, 7, 7, 9])
    assert off.tolist() == [0, 0, 0] and len(rows) == 0 and len(pos) == 0
    ap, rr, hits, dcg, idcg = R.per_query(off, pos, [1, 3])
    assert not ap.any() and not rr.any() and not hits.any() and not dcg.any() and not idcg.any()
    m = R.means(off, ap, rr, hits, dcg, idcg, [1, 3], skip_empty=True)
    assert m["map_score"] == 0.0 and m["recall_at_k"][3] == 0.0


def test_two_forms_agree_with_k_beyond_n_and_empty_queries():
    rng = np.random.default_rng(5)
    S = rng.standard_normal((9, 13))
    ql, gl = rng.integers(-1, 4, 9), rng.integers(-1, 3, 13)
    ks = [1, 4, 13, 50]
    a = R.flatten(R.from_labels(S, ql, gl, ks), ks)
    b = R.flatten(R.dense(S, R.relevance(ql, gl), ks), ks)
    assert np.abs(a - b).max() <= 1e-12
    keep = R.relevance(ql, gl).sum(1) > 0
    assert 0 < keep.sum() < 9
    c = R.flatten(R.from_labels(S, ql, gl, ks, skip_empty=True), ks)
    d = R.flatten(R.from_labels(S[keep], ql[keep], gl, ks), ks)
    assert np.abs(c - d).max() <= 1e-12
