"""CPU: the host half of the retrieval evaluation -- the product's dense ``RetrievalEvaluator.compute_retrieval_metrics`` against
the REFERENCE's outputs (tests/golden/retrieval_eval.npz) and the restatement (tests/retrieval_ref.py), the means of
``RetrievalEvaluator.from_ranks`` over handmade per-query terms, and the declarations of the three entry points.  1e-12: the
room of a differently ordered fp64 sum of at most 200 terms of size <= 1."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import retrieval_ref as R

G = Path(__file__).resolve().parent / "golden"
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def fx():
    z = np.load(G / "retrieval_eval.npz")
    d = {k: z[k] for k in z.files}
    d["ks"] = [int(k) for k in d["k_values"]]
    d["want"] = np.concatenate([d["recall_at_k"], d["precision_at_k"], d["ndcg_at_k"], [d["map_score"], d["mrr"]]])
    return d


def test_dense_metrics_equal_the_reference(pkg, fx):
    m = pkg.RetrievalEvaluator.compute_retrieval_metrics(fx["cosine"], R.relevance(fx["qlabel"], fx["glabel"]), fx["ks"])
    assert isinstance(m, pkg.RetrievalMetrics)
    assert np.abs(R.flatten(m, fx["ks"]) - fx["want"]).max() <= 1e-12
    assert set(m.to_dict()) == {"recall_at_k", "precision_at_k", "map_score", "ndcg_at_k", "mrr"}
    assert list(m.recall_at_k) == fx["ks"]


def test_dense_metrics_default_k_values(pkg, fx):
    m = pkg.RetrievalEvaluator.compute_retrieval_metrics(fx["cosine"], R.relevance(fx["qlabel"], fx["glabel"]))
    assert list(m.recall_at_k) == [1, 5, 10, 20, 50]
    assert np.abs(R.flatten(m, fx["ks"]) - fx["want"]).max() <= 1e-12


def test_dense_metrics_empty_queries_k_beyond_n_and_ties(pkg):
    rng = np.random.default_rng(5)
    S = rng.integers(-2, 3, (9, 13)).astype(np.float32)             # ties everywhere: the stable order decides
    ql, gl = rng.integers(-1, 4, 9), rng.integers(-1, 3, 13)
    rel = R.relevance(ql, gl)
    assert 0 < (rel.sum(1) == 0).sum() < 9
    ks = [1, 4, 13, 50]
    m = pkg.RetrievalEvaluator.compute_retrieval_metrics(S, rel, ks)
    assert np.abs(R.flatten(m, ks) - R.flatten(R.dense(S, rel, ks), ks)).max() <= 1e-12
    assert np.abs(R.flatten(m, ks) - R.flatten(R.from_labels(S, ql, gl, ks), ks)).max() <= 1e-12
    none = pkg.RetrievalEvaluator.compute_retrieval_metrics(S, np.zeros_like(rel), ks)
    assert not R.flatten(none, ks).any()


def test_from_ranks_means_and_skip_empty(pkg):
    """Handmade positions -> per-query terms (the restatement) -> the product's means, both conventions."""
    ks = (1, 3, 10)
    off = np.array([0, 3, 3, 4, 9], np.int64)
    pos = np.array([0, 2, 7, 5, 1, 2, 3, 11, 40], np.int64)
    ap, rr, hits, dcg, idcg = R.per_query(off, pos, ks)
    ranks = pkg.RetrievalRanks(k_values=ks, tgt_off=torch.from_numpy(off), tgt_row=torch.zeros(9, dtype=torch.int32),
                               tgt_sim=torch.zeros(9), pos=torch.from_numpy(pos).int(), hist=torch.zeros(9, dtype=torch.int32),
                               ap=torch.from_numpy(ap), rr=torch.from_numpy(rr), hits=torch.from_numpy(hits).int(),
                               dcg=torch.from_numpy(dcg), idcg=torch.from_numpy(idcg))
    assert ranks.n_targets.tolist() == [3, 0, 1, 5]
    for skip in (False, True):
        got = R.flatten(pkg.RetrievalEvaluator.from_ranks(ranks, skip_empty_queries=skip), ks)
        want = R.flatten(R.means(off, ap, rr, hits, dcg, idcg, ks, skip_empty=skip), ks)
        assert np.abs(got - want).max() <= 1e-12
    a = pkg.RetrievalEvaluator.from_ranks(ranks).map_score
    b = pkg.RetrievalEvaluator.from_ranks(ranks, skip_empty_queries=True).map_score
    assert abs(a * 4 - b * 3) <= 1e-12 and a > 0


def test_metrics_calculator_has_the_reference_signature(pkg):
    import inspect
    sig = inspect.signature(pkg.MetricsCalculator.calculate_retrieval_metrics)
    assert list(sig.parameters) == ["self", "query_embeddings", "gallery_embeddings", "query_labels", "gallery_labels", "k_values"]
    assert list(sig.parameters["k_values"].default) == [1, 5, 10]
    sig = inspect.signature(pkg.RetrievalEvaluator.evaluate_retrieval)
    assert list(sig.parameters) == ["query_embeddings", "gallery_embeddings", "query_labels", "gallery_labels", "k_values",
                                    "engine", "normalize", "skip_empty_queries"]
    assert hasattr(pkg.MultiModalRetriever, "evaluate_retrieval") and hasattr(pkg.TVCEngine, "retrieval_ranks")


def test_rank_entry_points_are_declared_and_bound(pkg):
    header = (ROOT / "include" / "tvc.h").read_text()
    for name in ("tvc_rank_targets", "tvc_rank_count", "tvc_rank_metrics"):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in pkg._lib.SIGNATURES
    assert int(re.search(r"#define TVC_RANK_MAX_K (\d+)", header).group(1)) == pkg.TVCEngine.RANK_MAX_K == 8
    assert int(re.search(r"#define TVC_ABI_VERSION (\d+)", header).group(1)) == pkg._lib.TVC_ABI_VERSION == 4
