"""Writes tests/golden/detection_eval.npz with the REFERENCE's own code (not collected by pytest; the only detection file that
reads the reference):

    python tests/make_detection_fixture.py <checkout of Zhang-Xin-Duke/multimodal-detection-consistency>

``src/utils/metrics.py`` is loaded by path; its ``DetectionEvaluator.compute_detection_metrics`` gives the detection fields and
its ``bootstrap_metric(roc_auc_score, labels, scores, n_bootstrap=200)``, after ``np.random.seed(SEED)``, the bootstrap dict.

Inputs: 400 scores, fp32-representable (the kernels take fp32; the reference sees the same values as fp64), positives shifted
up by one standard deviation, a quarter of them rounded to a grid of 1/4 (planted ties, across the classes), and -0.0 beside
0.0.  A test regenerates the 200 index rows from SEED with the legacy ``np.random`` stream (``np.random.choice(400, size=400,
replace=True)`` 200 times).  The file holds arrays only."""
import importlib.util
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
N, N_BOOTSTRAP, SEED = 400, 200, 20240611


def inputs():
    rng = np.random.default_rng(7)
    labels = (rng.random(N) < 0.4).astype(np.int64)
    s = rng.standard_normal(N) + labels
    tied = rng.random(N) < 0.25
    s[tied] = np.round(s[tied] * 4) / 4
    s[:4] = [0.0, -0.0, 0.0, -0.0]
    labels[:4] = [1, 0, 0, 1]
    return s.astype(np.float32), labels


def main():
    spec = importlib.util.spec_from_file_location("ref_metrics", Path(sys.argv[1]) / "src" / "utils" / "metrics.py")
    ref = importlib.util.module_from_spec(spec)
    sys.modules["ref_metrics"] = ref
    spec.loader.exec_module(ref)
    from sklearn.metrics import roc_auc_score
    scores, labels = inputs()
    s64 = scores.astype(np.float64)
    m = ref.DetectionEvaluator.compute_detection_metrics(s64, labels)
    np.random.seed(SEED)
    b = ref.bootstrap_metric(roc_auc_score, labels, s64, n_bootstrap=N_BOOTSTRAP)
    out = HERE / "golden" / "detection_eval.npz"
    np.savez_compressed(out, scores=scores, labels=labels, auc=np.float64(m.auc), accuracy=np.float64(m.accuracy),
                        precision=np.float64(m.precision), recall=np.float64(m.recall), f1_score=np.float64(m.f1_score),
                        fpr_at_95_tpr=np.float64(m.fpr_at_95_tpr), threshold=np.float64(m.threshold),
                        confusion_matrix=np.asarray(m.confusion_matrix, dtype=np.int64),
                        bootstrap=np.array([b["mean"], b["lower"], b["upper"], b["std"]], np.float64),
                        bootstrap_seed=np.int64(SEED), n_bootstrap=np.int64(N_BOOTSTRAP))
    print(f"{out}: {int(labels.sum())} positives of {N}, {N - len(np.unique(scores))} tied scores, AUROC {m.auc:.6f}, "
          f"threshold {m.threshold:.6f}, bootstrap mean {b['mean']:.6f} [{b['lower']:.6f}, {b['upper']:.6f}]")


if __name__ == "__main__":
    main()
