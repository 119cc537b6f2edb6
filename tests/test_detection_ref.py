"""CPU: the numpy restatement of the detection evaluation (tests/detection_ref.py) against sklearn and against the REFERENCE's
outputs (tests/golden/detection_eval.npz, written by tests/make_detection_fixture.py).  Curve and PR arrays, the Youden point and
the FPR at the target are compared for equality; AUROC and AP to 1e-12, the project's bound for reference fixtures (the
restatement's values are one rounding of an exact integer quotient; sklearn's trapezoid and its AP sum round every term)."""
from pathlib import Path

import numpy as np
import pytest
from sklearn.metrics import average_precision_score, precision_recall_curve, roc_auc_score, roc_curve

import detection_ref as R

G = Path(__file__).resolve().parent / "golden"
SIZES = (2, 3, 5, 63, 64, 65, 257, 1000, 4099)
KINDS = ("gaussian", "integer_ties", "one_group", "collinear", "worse_than_chance")


def _weights(rng, N, kind):
    if kind == "ones":
        return np.ones(N, np.int64)
    return np.bincount(rng.integers(0, N, N), minlength=N)


def _expand(scores, labels, w):
    """the weighted row as a plain sample: every original sample repeated w times"""
    idx = np.repeat(np.arange(len(w)), w)
    return scores[idx].astype(np.float64), labels[idx]


@pytest.mark.parametrize("wkind", ["ones", "resample"])
@pytest.mark.parametrize("N", SIZES)
def test_roc_restatement_equals_sklearn(N, wkind):
    rng = np.random.default_rng(1000 * N + len(wkind))
    for kind, (scores, labels) in R.score_kinds(rng, N).items():
        for rep in range(3):
            w = _weights(rng, N, wkind)
            s, y = _expand(scores, labels, w)
            if y.min() == y.max():
                continue
            ss, sl, order = R.prepare(scores, labels)
            r = R.sweep(ss, sl, w[order], target=0.95)
            fpr, tpr, thr = roc_curve(y, s)
            mine = R.roc_arrays(ss, r["TP"], r["FP"], r["pos"], r["kept"], r["n_pos"], r["n_neg"])
            for a, b in zip(mine, (fpr, tpr, thr)):
                assert a.shape == b.shape and np.array_equal(a, b), (kind, N, wkind)
            j = int(np.argmax(tpr - fpr))
            assert r["youden_j"] == (tpr - fpr)[j]
            assert R.sweep(ss, sl, w[order])["youden_pos"] == r["youden_pos"]
            want_thr = thr[j]
            got_thr = np.inf if r["youden_pos"] < 0 else np.float64(ss[r["youden_pos"]])
            assert got_thr == want_thr
            pred = s >= want_thr
            assert r["youden_tp"] == int((pred & (y == 1)).sum()) and r["youden_fp"] == int((pred & (y == 0)).sum())
            i95 = int(np.argmin(np.abs(tpr - 0.95)))
            assert np.float64(r["target_fp"]) / np.float64(r["n_neg"]) == fpr[i95]
            assert abs(r["auc"] - roc_auc_score(y, s)) <= 1e-12


@pytest.mark.parametrize("N", (2, 3, 17, 64, 65, 300, 1000))
def test_pr_restatement_equals_sklearn(N):
    rng = np.random.default_rng(77 + N)
    for kind, (scores, labels) in R.score_kinds(rng, N).items():
        for wkind in ("ones", "resample"):
            w = _weights(rng, N, wkind)
            s, y = _expand(scores, labels, w)
            if y.min() == y.max():
                continue
            ss, sl, order = R.prepare(scores, labels)
            TP, FP, pos, kept, P, Nn = R.points(ss, sl, w[order])
            for a, b in zip(R.pr_arrays(ss, TP, FP, pos, P), precision_recall_curve(y, s)):
                assert a.shape == b.shape and np.array_equal(a, b), (kind, N, wkind)
            exact = R.ap_fraction(TP, FP, P)
            assert abs(float(exact) - average_precision_score(y, s)) <= 1e-12
            assert abs(R.ap_scaled(TP, FP, P) - exact) <= len(TP) * 2.0 ** -200


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        assert tuple(int(x[0]) for x in R.philox4x32_10(counter, key)) == want
    d = R.philox_draws(1001, 3, (5 << 32) | 9)
    assert d.shape == (1001,) and d.min() >= 0 and d.max() < 1001 and len(np.unique(d)) > 500
    w = R.philox_weights(1001, 2, (5 << 32) | 9, first=3)
    assert w.sum(1).tolist() == [1001, 1001] and np.array_equal(w[0], np.bincount(d, minlength=1001))
    assert not np.array_equal(R.philox_weights(1001, 1, 10)[0], R.philox_weights(1001, 1, 11)[0])


@pytest.fixture(scope="module")
def fx():
    z = np.load(G / "detection_eval.npz")
    return {k: z[k] for k in z.files}


def test_fixture_reference_fields(fx):
    ss, sl, order = R.prepare(fx["scores"], fx["labels"])
    r = R.sweep(ss, sl, np.ones(len(ss), np.int64))
    P, Nn, tp, fp = r["n_pos"], r["n_neg"], r["youden_tp"], r["youden_fp"]
    acc, prec, rec, f1 = R.confusion_metrics(tp, fp, P, Nn)
    assert abs(r["auc"] - fx["auc"]) <= 1e-12
    for got, name in ((acc, "accuracy"), (prec, "precision"), (rec, "recall"), (f1, "f1_score")):
        assert abs(float(got) - fx[name]) <= 1e-12, name
    assert abs(r["target_fp"] / Nn - fx["fpr_at_95_tpr"]) <= 1e-12
    assert np.float64(ss[r["youden_pos"]]) == fx["threshold"]
    assert np.array_equal(np.array([[Nn - fp, fp], [P - tp, tp]]), fx["confusion_matrix"])


def test_fixture_bootstrap_dict_from_regenerated_rows(fx):
    N, B = len(fx["scores"]), int(fx["n_bootstrap"])
    np.random.seed(int(fx["bootstrap_seed"]))
    idx = np.stack([np.random.choice(N, size=N, replace=True) for _ in range(B)])
    ss, sl, order = R.prepare(fx["scores"], fx["labels"])
    vals = []
    for row in idx:
        r = R.sweep(ss, sl, np.bincount(row, minlength=N)[order])
        if r["valid"]:
            vals.append(r["auc"])
    d = R.bootstrap_dict(vals)
    got = np.array([d["mean"], d["lower"], d["upper"], d["std"]])
    assert np.abs(got - fx["bootstrap"]).max() <= 1e-12
