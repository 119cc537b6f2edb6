"""Writes tests/golden/simmetrics.npz with the REFERENCE's own code (not collected by pytest; the only similarity-metric file
that reads the reference):

    python tests/make_simmetrics_fixture.py <checkout of Zhang-Xin-Duke/multimodal-detection-consistency>

``src/utils/metrics.py`` is loaded by path; its ``SimilarityCalculator.compute_all_similarities`` gives the five metrics of a
pair of 6 x 512 matrices (which it flattens) and of 24 pairs of rows of 512.  ``src/retrieval.py`` cannot be imported without
faiss and its sibling modules, so the ``ConsistencyCalculator`` class node alone is taken out of its syntax tree and executed;
its four methods run on 16 pairs of length-64 id and similarity lists.

Inputs are fp32-representable and handed to the reference as fp64, so that it computes in fp64 on the values the kernels see
(on fp32 arrays its ``pearsonr`` works in fp32).  Rows: correlated Gaussians, a quarter of each row rounded to a grid of 1/4
(planted ties), -0.0 beside 0.0 in row 0, row 5 of x constant, row 7 of x all zero.  Id lists share ids between the two lists
and repeat ids inside a list.  The file holds arrays only."""
import ast
import importlib.util
import sys
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np

HERE = Path(__file__).resolve().parent
NAMES = ("cosine_similarity", "euclidean_distance", "manhattan_distance", "pearson_correlation", "spearman_correlation")
KS = (1, 5, 10, 64, 100)


def inputs():
    rng = np.random.default_rng(20240917)

    def pair(shape):
        g = rng.standard_normal(shape)
        h = 0.7 * g + 0.7 * rng.standard_normal(shape)
        for m in (g, h):
            tied = rng.random(shape) < 0.25
            m[tied] = np.round(m[tied] * 4) / 4
        return g.astype(np.float32), h.astype(np.float32)

    E1, E2 = pair((6, 512))
    X, Y = pair((24, 512))
    X[0, :6] = [0.0, -0.0, 0.0, -0.0, 0.25, 0.25]
    Y[0, :6] = [-0.0, 0.0, 1.0, 1.0, -0.0, 0.0]
    X[5] = 0.25
    X[7] = 0.0
    idx1 = np.stack([rng.permutation(200)[:64] for _ in range(16)]).astype(np.int64)
    idx2 = idx1.copy()
    for r in range(16):
        moved = rng.random(64) < 0.4
        idx2[r, moved] = rng.integers(0, 300, int(moved.sum()))           # new ids, some equal to ids elsewhere in the lists
        idx2[r] = idx2[r, rng.permutation(64)] if r % 2 else idx2[r]
        idx1[r, 10] = idx1[r, 3]                                          # repeats inside a list
        idx2[r, 20] = idx2[r, 21]
    s1 = np.sort(rng.random((16, 64)), axis=1)[:, ::-1].astype(np.float32)
    s2 = (s1 + 0.1 * rng.standard_normal((16, 64))).astype(np.float32)
    return E1, E2, X, Y, idx1, idx2, np.ascontiguousarray(s1), s2


def consistency_calculator(checkout: Path):
    tree = ast.parse((checkout / "src" / "retrieval.py").read_text())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ConsistencyCalculator")
    ns = {"np": np, "Dict": Dict, "List": List, "Optional": Optional, "Tuple": Tuple, "Union": Union, "Any": Any}
    exec(compile(ast.Module(body=[node], type_ignores=[]), "ConsistencyCalculator", "exec"), ns)
    return ns["ConsistencyCalculator"]()


def main():
    checkout = Path(sys.argv[1])
    spec = importlib.util.spec_from_file_location("ref_metrics", checkout / "src" / "utils" / "metrics.py")
    ref = importlib.util.module_from_spec(spec)
    sys.modules["ref_metrics"] = ref
    spec.loader.exec_module(ref)
    E1, E2, X, Y, idx1, idx2, s1, s2 = inputs()
    f64 = lambda a: a.astype(np.float64)
    calc = ref.SimilarityCalculator
    flat = calc.compute_all_similarities(f64(E1), f64(E2)).to_dict()
    rows = [calc.compute_all_similarities(f64(x), f64(y)).to_dict() for x, y in zip(X, Y)]
    cc = consistency_calculator(checkout)
    dist = [cc.compute_similarity_distribution(f64(s)) for s in s1]
    out = HERE / "golden" / "simmetrics.npz"
    np.savez_compressed(
        out, E1=E1, E2=E2, X=X, Y=Y, idx1=idx1, idx2=idx2, s1=s1, s2=s2, ks=np.array(KS, np.int64),
        flat=np.array([flat[n] for n in NAMES], np.float64), rows=np.array([[r[n] for n in NAMES] for r in rows], np.float64),
        dist=np.array([[d[k] for k in ("mean", "std", "min", "max", "median")] for d in dist], np.float64),
        score=np.array([cc.compute_consistency_score(f64(a), f64(b)) for a, b in zip(s1, s2)], np.float64),
        topk=np.array([[cc.compute_top_k_consistency(a, b, k) for k in KS] for a, b in zip(idx1, idx2)], np.float64),
        rank=np.array([cc.compute_rank_correlation(a, b) for a, b in zip(idx1, idx2)], np.float64))
    print(f"{out}: flat {flat}; constant row {rows[5]}; zero row {rows[7]}; top-10 consistency {[r for r in np.load(out)['topk'][:4, 2]]}")


if __name__ == "__main__":
    main()
