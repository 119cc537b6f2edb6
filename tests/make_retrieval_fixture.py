"""Writes tests/golden/retrieval_eval.npz with the REFERENCE's own code (not collected by pytest; the only retrieval file that
reads the reference):

    python tests/make_retrieval_fixture.py <checkout of Zhang-Xin-Duke/multimodal-detection-consistency>

``src/utils/metrics.py`` is loaded by path; its ``SimilarityCalculator.batch_cosine_similarity`` gives the cosine matrix and its
``RetrievalEvaluator.compute_retrieval_metrics`` the metrics for k = 1, 5, 10, 20, 50.

Inputs: 40 x 96 queries and 200 x 96 gallery rows (96 is not a multiple of 64: the evaluator pads) of random norm (the cosine
must not see it), labels in 25 groups; label 24 is on no gallery row, some query labels are 24 or negative (queries without a
relevant row), some gallery labels are negative (distractors).  No relevant row lies within 1e-5 of another score of its query
in fp64 (asserted; SEED was chosen so that it holds), so neither the reference's fp32 rounding nor the kernels' decides a
position.  The file holds arrays only."""
import importlib.util
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import retrieval_ref  # noqa: E402

Q, N, D, GROUPS = 40, 200, 96, 25
K_VALUES = [1, 5, 10, 20, 50]
SEED = 31                   # of the seeds 0 .. 39 the one with the largest gap (1.4e-5); `--seeds` prints them all


def inputs(seed=SEED):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((Q, D)) * (10.0 ** rng.uniform(-1, 1, Q))[:, None]
    g = rng.standard_normal((N, D)) * (10.0 ** rng.uniform(-1, 1, N))[:, None]
    glabel = rng.integers(0, GROUPS - 1, N)                     # 0 .. 23: label 24 is absent from the gallery
    glabel[rng.choice(N, 12, replace=False)] = -1               # distractors
    qlabel = rng.integers(0, GROUPS, Q)
    qlabel[[3, 17]] = GROUPS - 1                                # a label no gallery row carries
    qlabel[[5, 29]] = -1                                        # a negative query label
    return q.astype(np.float32), g.astype(np.float32), qlabel.astype(np.int64), glabel.astype(np.int64)


def min_gap(q, g, qlabel, glabel) -> float:
    """the smallest fp64 distance of a relevant row's cosine to another cosine of its query"""
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    S = (q64 / np.linalg.norm(q64, axis=1, keepdims=True)) @ (g64 / np.linalg.norm(g64, axis=1, keepdims=True)).T
    rel = retrieval_ref.relevance(qlabel, glabel)
    gap = np.inf
    for i, j in zip(*np.nonzero(rel)):
        d = np.abs(S[i] - S[i, j])
        d[j] = np.inf
        gap = min(gap, d.min())
    return float(gap)


def main():
    spec = importlib.util.spec_from_file_location("ref_metrics", Path(sys.argv[1]) / "src" / "utils" / "metrics.py")
    ref = importlib.util.module_from_spec(spec)
    sys.modules["ref_metrics"] = ref
    spec.loader.exec_module(ref)
    q, g, qlabel, glabel = inputs()
    gap = min_gap(q, g, qlabel, glabel)
    assert gap > 1e-5, f"a relevant row lies within {gap:.3e} of another score of its query: choose another SEED"
    rel = retrieval_ref.relevance(qlabel, glabel)
    assert (rel.sum(1) == 0).sum() >= 4 and rel.sum() > 100
    S = ref.SimilarityCalculator.batch_cosine_similarity(q, g)
    m = ref.RetrievalEvaluator.compute_retrieval_metrics(S, rel, K_VALUES)
    out = HERE / "golden" / "retrieval_eval.npz"
    np.savez_compressed(out, queries=q, gallery=g, qlabel=qlabel, glabel=glabel, cosine=np.asarray(S), k_values=np.array(K_VALUES, np.int64),
                        recall_at_k=np.array([m.recall_at_k[k] for k in K_VALUES], np.float64),
                        precision_at_k=np.array([m.precision_at_k[k] for k in K_VALUES], np.float64),
                        ndcg_at_k=np.array([m.ndcg_at_k[k] for k in K_VALUES], np.float64),
                        map_score=np.float64(m.map_score), mrr=np.float64(m.mrr), min_gap=np.float64(gap))
    print(f"{out}: {int(rel.sum())} relevant pairs, {int((rel.sum(1) == 0).sum())} queries without one, min gap {gap:.3e}, "
          f"mAP {m.map_score:.6f}, MRR {m.mrr:.6f}")


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--seeds":          # the search that chose SEED
        for s in range(40):
            print(s, f"{min_gap(*inputs(s)):.3e}")
    else:
        main()
