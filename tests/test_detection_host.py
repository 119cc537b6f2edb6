"""CPU: the host half of the detection evaluation -- the declarations of the three entry points and the constants the engine
mirrors, ``bootstrap_metric`` with a callable against the reference's loop, the signatures of the new surface, and the host code
of tvc_roc.cpp (checks, refusals, chunking, the workspace; the plan of host_plan.hpp) under AddressSanitizer / UBSan with leak
detection as a stand-alone program (tests/host_san_roc/driver.cpp on tests/host_san's HIP stand-in, built and run by
tests/host_san_build.py)."""
import inspect
import re
from pathlib import Path

import numpy as np

import host_san_build

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "multimodal-detection-consistency_amd" / "csrc"


def _define(text, name):
    return re.search(rf"#define {name} (.+)", text).group(1).split("//")[0].split("/*")[0].strip()


def test_roc_entry_points_are_declared_and_bound(pkg):
    header = (ROOT / "include" / "tvc.h").read_text()
    for name in ("tvc_roc_weights", "tvc_roc_sweep", "tvc_roc_curve"):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in pkg._lib.SIGNATURES
    plan = (CSRC / "host_plan.hpp").read_text()
    E = pkg.TVCEngine
    assert int(_define(header, "TVC_ROC_LDS_ROWS")) == int(_define(plan, "ROC_LDS_ROWS")) == E.ROC_LDS_ROWS
    assert int(_define(header, "TVC_ROC_MAX_THR")) == int(_define(plan, "ROC_MAX_THR")) == E.ROC_MAX_THR == 8
    assert int(_define(header, "TVC_ROC_MAX_N")) == eval(_define(plan, "ROC_MAX_N")) == E.ROC_MAX_N >= 1 << 20
    assert E.ROC_LDS_ROWS * 4 + 16 * 1024 <= 160 * 1024                 # uint32 counts + the scan's scratch in a CU's LDS
    assert [int(_define(header, f"TVC_ROC_SRC_{n}")) for n in ("WEIGHTS", "INDICES", "PHILOX")] == \
           [pkg._lib.TVC_ROC_SRC_WEIGHTS, pkg._lib.TVC_ROC_SRC_INDICES, pkg._lib.TVC_ROC_SRC_PHILOX] == [0, 1, 2]
    assert int(re.search(r"#define TVC_ABI_VERSION (\d+)", header).group(1)) == pkg._lib.TVC_ABI_VERSION == 4
    # the ctypes mirrors follow the header's field order
    rows = re.search(r"typedef struct tvc_roc_rows \{(.*?)\} tvc_roc_rows;", header, re.S).group(1)
    rows = re.sub(r"/\*.*?\*/", "", rows, flags=re.S)
    assert re.findall(r"(\w+);", rows) == ["scores_dev", "labels_dev", "order_dev", "N", "source", "src_dev", "B", "first", "seed"]
    assert [n for n, _ in pkg._lib.RocRows._fields_] == ["scores", "labels", "order", "N", "source", "src", "B", "first", "seed"]
    out = re.search(r"typedef struct tvc_roc_out \{(.*?)\} tvc_roc_out;", header, re.S).group(1)
    assert re.findall(r"\*\s*(\w+)", out) == list(pkg._lib.ROC_OUT_FIELDS) == [n for n, _ in pkg._lib.RocOut._fields_]


def test_new_surface_signatures(pkg):
    sig = inspect.signature(pkg.TVCEngine.roc_sweep)
    assert list(sig.parameters)[:3] == ["self", "scores", "labels"]
    for name, default in (("n_resamples", 0), ("weights", None), ("indices", None), ("seed", 0), ("target_tpr", 0.95), ("thresholds", ())):
        p = sig.parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == default, name
    assert hasattr(pkg.TVCEngine, "roc_weights") and hasattr(pkg.TVCEngine, "roc_curve") and hasattr(pkg, "RocSweep")
    sig = inspect.signature(pkg.DetectionEvaluator.evaluate_scores)
    assert list(sig.parameters) == ["scores", "labels", "pos_label", "engine"] and sig.parameters["pos_label"].default == 1
    sig = inspect.signature(pkg.bootstrap_metric)
    assert list(sig.parameters) == ["metric", "scores", "labels", "n_bootstrap", "confidence", "seed", "indices", "engine"]
    assert sig.parameters["n_bootstrap"].default == 1000 and sig.parameters["confidence"].default == 0.95
    assert hasattr(pkg.DetectionEvaluator, "compute_roc_curve") and hasattr(pkg.DetectionEvaluator, "compute_pr_curve")
    assert hasattr(pkg, "bootstrap_detection_metrics")
    sig = inspect.signature(pkg.AdversarialDetector.compute_optimal_threshold)
    assert list(sig.parameters) == ["self", "validation_data", "methods"] and sig.parameters["methods"].default is None
    det = pkg.AdversarialDetector(pkg.DetectorConfig(clip_model="ViT-T/16-test"))
    det.update_threshold(0.25)
    assert det.config.detection_threshold == 0.25
    assert det.compute_optimal_threshold([]) == 0.25                    # a failure falls back to the configured threshold
    assert isinstance(inspect.getattr_static(pkg.AdversarialDetector, "optimal_threshold_from_scores"), staticmethod)


def _reference_loop(metric, args, n_bootstrap, confidence=0.95):
    """src/utils/metrics.py:816-874, restated"""
    n = len(args[0])
    values = []
    for _ in range(n_bootstrap):
        idx = np.random.choice(n, size=n, replace=True)
        try:
            v = metric(*[a[idx] for a in args])
            if isinstance(v, (int, float)) and not np.isnan(v):
                values.append(v)
        except Exception:
            continue
    if not values:
        return {"mean": 0.0, "lower": 0.0, "upper": 0.0}
    alpha = 1 - confidence
    return {"mean": np.mean(values), "lower": np.percentile(values, (alpha / 2) * 100),
            "upper": np.percentile(values, (1 - alpha / 2) * 100), "std": np.std(values)}


def test_bootstrap_metric_with_a_callable_is_the_reference_loop(pkg):
    from sklearn.metrics import roc_auc_score
    rng = np.random.default_rng(3)
    labels = rng.integers(0, 2, 60)
    scores = rng.standard_normal(60) + labels
    for metric, args in ((roc_auc_score, (labels, scores)), (lambda s, y: float(np.mean((s > 0) == y)), (scores, labels))):
        np.random.seed(11)
        want = _reference_loop(metric, args, 50, 0.9)
        np.random.seed(11)
        got = pkg.bootstrap_metric(metric, args[0], args[1], n_bootstrap=50, confidence=0.9)
        assert got == want and set(got) == {"mean", "lower", "upper", "std"}
    # one-class resamples raise inside roc_auc_score and are dropped; explicit index rows replace the stream
    tiny_y, tiny_s = np.array([0, 1]), np.array([0.1, 0.9])
    np.random.seed(5)
    want = _reference_loop(roc_auc_score, (tiny_y, tiny_s), 40)
    np.random.seed(5)
    idx = np.stack([np.random.choice(2, size=2, replace=True) for _ in range(40)])
    assert pkg.bootstrap_metric(roc_auc_score, tiny_y, tiny_s, indices=idx) == want and want["mean"] == 1.0
    assert pkg.bootstrap_metric(lambda s, y: float("nan"), scores, labels, n_bootstrap=5) == {"mean": 0.0, "lower": 0.0, "upper": 0.0}
    assert pkg.bootstrap_metric(roc_auc_score, np.zeros(0), np.zeros(0)) == {"mean": 0.0, "lower": 0.0, "upper": 0.0}
    import pytest
    with pytest.raises(ValueError):
        pkg.bootstrap_metric("auroc", scores, labels)


def test_roc_host_code_under_address_and_ub_sanitizers(tmp_path_factory):
    host_san_build.run_driver("host_san_roc", "HOST_SAN_ROC_OK", tmp_path_factory)
