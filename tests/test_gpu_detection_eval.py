"""GPU: the detection evaluation (roc.hip behind tvc_roc_weights / tvc_roc_sweep / tvc_roc_curve, TVCEngine.roc_*, the detection
half of metrics.py, AdversarialDetector.compute_optimal_threshold) against the numpy restatement (tests/detection_ref.py, itself
pinned to sklearn and to the reference's fixture by tests/test_detection_ref.py).

Every integer output is compared for equality, J and auc bit for bit (each is one or two correctly rounded fp64 quotients of
integers and one subtraction).  ap is compared with the exact rational value: each of the at most `points` terms takes three
roundings and the terms sum to at most 1, so |ap - exact| <= (points + 4) * 2^-52; from 300 points on the exact value is
``ap_scaled`` (within points * 2^-200 of the Fraction, which that bound absorbs)."""
from pathlib import Path

import numpy as np
import pytest
import torch

import detection_ref as R

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"
INT_FIELDS = ("n_pos", "n_neg", "valid", "n_points", "n_kept", "auc2", "youden_pos", "youden_tp", "youden_fp", "target_pos",
              "target_tp", "target_fp")
KINDS = ("gaussian", "integer_ties", "one_group", "collinear", "worse_than_chance")


def _sizes(pkg):
    L = pkg.TVCEngine.ROC_LDS_ROWS
    return (2, 3, 63, 64, 65, 255, 256, 257, 1000, 4099, L, L + 1)


def _thresholds(ss):
    """equal to a score, between two scores, above all, below all"""
    mid = ss[len(ss) // 2]
    return (float(mid), float(np.nextafter(mid, np.float32(np.inf))), float(ss[0]) + 1.0, float(ss[-1]) - 1.0)


def _host(sw):
    return {n: getattr(sw, n).cpu().numpy() for n in INT_FIELDS + ("auc", "ap", "youden_j", "thr_tp", "thr_fp")}


def _check_rows(sw, ss, sl, W, target, thresholds):
    """rows of a RocSweep against the restatement: W int [rows, N] multiplicities over the SORTED positions, row 0 the ones"""
    got = _host(sw)
    assert got["valid"].shape == (len(W),)
    invalid = 0
    for b, w in enumerate(W):
        r = R.sweep(ss, sl, w, target, thresholds)
        for n in INT_FIELDS:
            assert int(got[n][b]) == r[n], (n, b)
        assert got["thr_tp"][b].tolist() == r["thr_tp"] and got["thr_fp"][b].tolist() == r["thr_fp"], b
        assert got["youden_j"][b] == r["youden_j"] and got["auc"][b] == r["auc"], b
        if not r["valid"]:
            invalid += 1
            assert got["ap"][b] == 0.0
            continue
        m = r["n_points"]
        exact = (R.ap_fraction if m < 300 else R.ap_scaled)(r["TP"], r["FP"], r["n_pos"])
        assert abs(float(got["ap"][b]) - exact) <= (m + 4) * 2.0 ** -52, b
    return invalid


@pytest.fixture(scope="module")
def cases(pkg):
    """the score kinds of every size, made once"""
    out = {}
    for N in _sizes(pkg):
        rng = np.random.default_rng(N)
        out[N] = R.score_kinds(rng, N)
    return out


@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("ni", range(12))
def test_weights_readback(pkg, gpu_engine, cases, ni, B):
    N = _sizes(pkg)[ni]
    scores, labels = cases[N]["integer_ties"]
    rng = np.random.default_rng(7 * N + B)
    ss, sl, order = R.prepare(scores, labels)
    pss, psl, porder = gpu_engine.roc_prepare(scores, labels)
    assert np.array_equal(porder.cpu().numpy(), order) and np.array_equal(pss.cpu().numpy(), ss) and np.array_equal(psl.cpu().numpy(), sl)
    idx = rng.integers(0, N, (B, N))
    got = gpu_engine.roc_weights(scores, labels, indices=idx).cpu().numpy()
    assert np.array_equal(got, np.stack([np.bincount(r, minlength=N) for r in idx])[:, order])
    seed, first = (N << 33) | 12345, 3
    got = gpu_engine.roc_weights(scores, labels, n_resamples=B, seed=seed, first=first).cpu().numpy()
    assert np.array_equal(got, R.philox_weights(N, B, seed, first)[:, order])
    w = rng.integers(0, 4, (B, N))
    assert np.array_equal(gpu_engine.roc_weights(scores, labels, weights=w).cpu().numpy(), w[:, order])
    assert np.array_equal(gpu_engine.roc_weights(scores, labels).cpu().numpy(), np.ones((1, N), np.int32))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ni", range(12))
def test_sweep_integers_and_fp64_outputs(pkg, gpu_engine, cases, ni, kind):
    N = _sizes(pkg)[ni]
    scores, labels = cases[N][kind]
    ss, sl, order = R.prepare(scores, labels)
    thr = _thresholds(ss)
    ones = np.ones((1, N), np.int64)
    rng = np.random.default_rng(N + len(kind))
    invalid = 0
    for B in (1, 3, 17):
        w = rng.integers(0, 3, (B, N))
        w[:, rng.integers(0, N)] += 1                                    # never an empty row
        sw = gpu_engine.roc_sweep(scores, labels, weights=w, target_tpr=0.95, thresholds=thr)
        invalid += _check_rows(sw, ss, sl, np.r_[ones, w[:, order]], 0.95, thr)
        idx = rng.integers(0, N, (B, N))
        sw = gpu_engine.roc_sweep(scores, labels, indices=idx, target_tpr=0.0, thresholds=thr[:1])
        W = np.stack([np.bincount(r, minlength=N) for r in idx])
        invalid += _check_rows(sw, ss, sl, np.r_[ones, W[:, order]], 0.0, thr[:1])
        seed = (B << 40) | N
        sw = gpu_engine.roc_sweep(scores, labels, n_resamples=B, seed=seed, target_tpr=1.0)
        invalid += _check_rows(sw, ss, sl, np.r_[ones, R.philox_weights(N, B, seed)[:, order]], 1.0, ())
    if N == 2:
        assert invalid > 0                                               # one-class resamples: valid == 0 and zeros


def test_planted_cases(gpu_engine):
    N = 300
    rng = np.random.default_rng(42)
    labels = rng.integers(0, 2, N)
    scores = np.round(rng.standard_normal(N) * 3).astype(np.float32)     # ~20 tie groups
    scores[:6] = [0.0, -0.0, 0.0, -0.0, 0.0, -0.0]
    labels[:6] = [1, 0, 1, 0, 0, 1]
    ss, sl, order = R.prepare(scores, labels)
    assert len(np.unique(ss)) == len(np.unique(scores + np.float32(0.0)))    # -0.0 and 0.0: one group
    levels = np.unique(scores + np.float32(0.0))
    w = np.ones((5, N), np.int64)
    w[0, np.isin(scores, levels[-3:])] = 0                               # zero-weight groups at the front of the order
    w[1, np.isin(scores, levels[len(levels) // 2 - 1:len(levels) // 2 + 2])] = 0     # in the middle
    w[2, np.isin(scores, levels[:3])] = 0                                # at the end
    w[3] = 0
    w[3, 17] = N                                                         # every draw hit one sample: one class
    w[4, ::2] = 0
    thr = _thresholds(ss) + (0.0, -0.0)
    for target in (0.0, 0.95, 1.0):
        sw = gpu_engine.roc_sweep(scores, labels, weights=w, target_tpr=target, thresholds=thr)
        assert _check_rows(sw, ss, sl, np.r_[np.ones((1, N), np.int64), w[:, order]], target, thr) == 1
        assert int(sw.valid[4]) == 0 and int(sw.n_pos[4]) == 0 and float(sw.auc[4]) == 0.0
    idx = np.full((2, N), 17)
    idx[1, :] = np.arange(N)
    sw = gpu_engine.roc_sweep(scores, labels, indices=idx)
    assert sw.valid.tolist() == [1, 0, 1] and int(sw.auc2[2]) == int(sw.auc2[0])
    # J <= 0 everywhere: every positive below every negative -> the origin wins, threshold +inf
    y = np.r_[np.ones(40, np.int64), np.zeros(60, np.int64)]
    s = np.r_[np.arange(40), 100 + np.arange(60)].astype(np.float32)
    sw = gpu_engine.roc_sweep(s, y)
    assert int(sw.youden_pos[0]) == -1 and float(sw.youden_j[0]) == 0.0 and int(sw.youden_tp[0]) == 0 and int(sw.youden_fp[0]) == 0
    assert sw.threshold_at(int(sw.youden_pos[0])) == float("inf") and int(sw.auc2[0]) == 0
    ss2, sl2, o2 = R.prepare(s, y)
    _check_rows(sw, ss2, sl2, np.ones((1, 100), np.int64), 0.95, ())


def test_two_runs_are_bit_identical(pkg, gpu_engine, cases):
    for N in (4099, pkg.TVCEngine.ROC_LDS_ROWS + 1):
        scores, labels = cases[N]["gaussian"]
        a = gpu_engine.roc_sweep(scores, labels, n_resamples=17, seed=99, thresholds=(0.5,))
        b = gpu_engine.roc_sweep(scores, labels, n_resamples=17, seed=99, thresholds=(0.5,))
        for n in pkg._lib.ROC_OUT_FIELDS:
            assert torch.equal(getattr(a, n), getattr(b, n)), n
        c = gpu_engine.roc_sweep(scores, labels, n_resamples=17, seed=100, thresholds=(0.5,))
        assert not torch.equal(a.auc2[1:], c.auc2[1:]) and torch.equal(a.auc2[:1], c.auc2[:1])


def test_chunked_rows_equal_unchunked_rows(pkg, gpu_engine):
    """N = ROC_MAX_N = 2^24 in the global form: 16 rows fill the 1 GiB workspace budget, so 17 resamples run as two chunks; rows
    of both chunks equal the same resamples run alone (one row per call, numbered by `first`)."""
    N, B = pkg.TVCEngine.ROC_MAX_N, 17
    g = torch.Generator(device="cuda").manual_seed(5)
    labels = (torch.rand(N, generator=g, device="cuda") < 0.3).to(torch.int64)
    scores = torch.randn(N, generator=g, device="cuda") + labels
    all_rows = gpu_engine.roc_sweep(scores, labels, n_resamples=B, seed=2024, thresholds=(0.25,))
    assert all_rows.valid.tolist() == [1] * (B + 1)
    for b in (0, 15, 16):
        one = gpu_engine.roc_sweep(scores, labels, n_resamples=1, seed=2024, first=b, thresholds=(0.25,))
        for n in pkg._lib.ROC_OUT_FIELDS:
            assert torch.equal(getattr(one, n)[1], getattr(all_rows, n)[1 + b]), (n, b)
    assert len(set(all_rows.auc2[1:].tolist())) == B
    # the full sample against torch: P, N and the doubled AUROC numerator by ranks (no ties to speak of; exact in int64)
    P = int(labels.sum())
    assert int(all_rows.n_pos[0]) == P and int(all_rows.n_neg[0]) == N - P and int(all_rows.n_pos[5]) + int(all_rows.n_neg[5]) == N


@pytest.fixture(scope="module")
def fx():
    z = np.load(G / "detection_eval.npz")
    return {k: z[k] for k in z.files}


def test_curves_equal_sklearn(pkg, gpu_engine, cases, fx):
    from sklearn.metrics import precision_recall_curve, roc_curve
    samples = [(fx["scores"], fx["labels"])] + [cases[N][k] for N in (257, 1000) for k in KINDS]
    for scores, labels in samples:
        s64 = scores.astype(np.float64)
        for got, want in zip(pkg.DetectionEvaluator.compute_roc_curve(scores, labels, engine=gpu_engine), roc_curve(labels, s64)):
            assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want)
        for got, want in zip(pkg.DetectionEvaluator.compute_pr_curve(scores, labels, engine=gpu_engine), precision_recall_curve(labels, s64)):
            assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want)
    # pos_label and a weighted row through the engine
    scores, labels = cases[257]["integer_ties"]
    got = pkg.DetectionEvaluator.compute_roc_curve(scores, 1 - labels, pos_label=0, engine=gpu_engine)
    assert all(np.array_equal(a, b) for a, b in zip(got, roc_curve(labels, scores.astype(np.float64))))
    w = np.random.default_rng(1).integers(0, 3, 257)
    tp, fp, pos, kept, ss_dev, P, Nn = gpu_engine.roc_curve(scores, labels, weights=w)
    ss, sl, order = R.prepare(scores, labels)
    TP, FP, rpos, rkept, rP, rN = R.points(ss, sl, w[order])
    assert (P, Nn) == (rP, rN) and np.array_equal(tp.cpu().numpy(), TP) and np.array_equal(fp.cpu().numpy(), FP)
    assert np.array_equal(pos.cpu().numpy(), rpos) and np.array_equal(kept.cpu().numpy().astype(bool), rkept)


def test_evaluate_scores_reproduces_the_reference(pkg, gpu_engine, fx):
    m = pkg.DetectionEvaluator.evaluate_scores(fx["scores"], fx["labels"], engine=gpu_engine)
    assert isinstance(m, pkg.DetectionMetrics)
    for name in ("auc", "accuracy", "precision", "recall", "f1_score", "fpr_at_95_tpr"):
        assert abs(getattr(m, name) - float(fx[name])) <= 1e-12, name
    assert m.threshold == float(fx["threshold"]) and np.array_equal(m.confusion_matrix, fx["confusion_matrix"])
    host = pkg.DetectionEvaluator.compute_detection_metrics(fx["scores"], fx["labels"])
    assert abs(host.auc - m.auc) <= 1e-12 and host.threshold == m.threshold
    worse = pkg.DetectionEvaluator.evaluate_scores(np.r_[np.arange(40), 100 + np.arange(60)], np.r_[np.ones(40), np.zeros(60)], engine=gpu_engine)
    assert worse.threshold == float("inf") and worse.recall == 0.0 and worse.precision == 0.0 and worse.f1_score == 0.0
    assert np.array_equal(worse.confusion_matrix, [[60, 0], [40, 0]]) and worse.accuracy == 0.6 and worse.auc == 0.0


def test_bootstrap_metric(pkg, gpu_engine, fx):
    scores, labels = fx["scores"], fx["labels"]
    N, B = len(scores), int(fx["n_bootstrap"])
    np.random.seed(int(fx["bootstrap_seed"]))
    idx = np.stack([np.random.choice(N, size=N, replace=True) for _ in range(B)])
    d = pkg.bootstrap_metric("auc", scores, labels, indices=idx, engine=gpu_engine)
    assert np.abs(np.array([d["mean"], d["lower"], d["upper"], d["std"]]) - fx["bootstrap"]).max() <= 1e-12
    # Philox resamples: the restatement's dicts
    ss, sl, order = R.prepare(scores, labels)
    full = R.sweep(ss, sl, np.ones(N, np.int64))
    thr = (float(ss[full["youden_pos"]]),)
    rows = [R.sweep(ss, sl, w, 0.95, thr) for w in R.philox_weights(N, 64, 31)[:, order]]
    assert all(r["valid"] for r in rows)
    acc, prec, rec, f1 = R.confusion_metrics([r["thr_tp"][0] for r in rows], [r["thr_fp"][0] for r in rows],
                                             [r["n_pos"] for r in rows], [r["n_neg"] for r in rows])
    want = {"auc": [r["auc"] for r in rows], "accuracy": acc, "precision": prec, "recall": rec, "f1": f1,
            "fpr_at_95_tpr": [np.float64(r["target_fp"]) / np.float64(r["n_neg"]) for r in rows]}
    got = pkg.bootstrap_detection_metrics(scores, labels, n_bootstrap=64, confidence=0.9, seed=31, engine=gpu_engine)
    assert set(got) == {"auc", "ap", "accuracy", "precision", "recall", "f1", "fpr_at_95_tpr"}
    for name, vals in want.items():
        assert got[name] == R.bootstrap_dict(vals, 0.9), name
        assert pkg.bootstrap_metric(name, scores, labels, n_bootstrap=64, confidence=0.9, seed=31, engine=gpu_engine) == got[name]
    ap = R.bootstrap_dict([float(R.ap_fraction(r["TP"], r["FP"], r["n_pos"])) for r in rows], 0.9)
    assert all(abs(got["ap"][k] - ap[k]) <= 1e-12 for k in ap)
    other = pkg.bootstrap_metric("auc", scores, labels, n_bootstrap=64, confidence=0.9, seed=32, engine=gpu_engine)
    assert other != got["auc"] and abs(other["mean"] - got["auc"]["mean"]) < 0.05
    # one-class resamples are dropped: two samples, 40 resamples
    tiny = pkg.bootstrap_metric("auc", [0.1, 0.9], [0, 1], n_bootstrap=40, seed=1, engine=gpu_engine)
    tw = R.philox_weights(2, 40, 1)
    assert 0 < (tw.min(1) > 0).sum() < 40 and tiny == R.bootstrap_dict([1.0] * int((tw.min(1) > 0).sum()))


def test_refusals_launch_nothing(pkg, gpu_engine):
    import ctypes as C
    E = pkg.TVCEngine
    ws = gpu_engine.workspace_bytes()
    good_s, good_y = np.array([0.1, 0.4, 0.35, 0.8], np.float32), np.array([0, 0, 1, 1])
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            gpu_engine.roc_sweep(np.array([0.1, bad, 0.35, 0.8], np.float32), good_y)
    for y in (np.zeros(4, np.int64), np.ones(4, np.int64)):
        with pytest.raises(ValueError, match="one class"):
            gpu_engine.roc_sweep(good_s, y)
        with pytest.raises(ValueError, match="one class"):
            pkg.DetectionEvaluator.compute_roc_curve(good_s, y, engine=gpu_engine)
    with pytest.raises(ValueError, match="thresholds"):
        gpu_engine.roc_sweep(good_s, good_y, thresholds=tuple(range(E.ROC_MAX_THR + 1)))
    with pytest.raises(ValueError, match="target_tpr"):
        gpu_engine.roc_sweep(good_s, good_y, target_tpr=1.5)
    with pytest.raises(ValueError, match="scores"):
        gpu_engine.roc_sweep(torch.zeros(E.ROC_MAX_N + 1), torch.zeros(E.ROC_MAX_N + 1, dtype=torch.int8))
    with pytest.raises(ValueError):
        gpu_engine.roc_sweep(good_s, good_y[:3])
    # the C-ABI's own refusals, with its error code
    ss, sl, order = gpu_engine.roc_prepare(good_s, good_y)
    out = {n: torch.zeros(8, dtype=torch.int64, device="cuda") for n in pkg._lib.ROC_OUT_FIELDS}
    o = pkg._lib.RocOut(*[out[n].data_ptr() for n in pkg._lib.ROC_OUT_FIELDS])
    thr = (C.c_float * 9)(*range(9))

    def call(N=4, B=1, source=0, n_thr=0, target=0.95):
        rows = pkg._lib.RocRows(ss.data_ptr(), sl.data_ptr(), order.data_ptr(), N, source, 0, B, 0, 0)
        return gpu_engine.lib.tvc_roc_sweep(gpu_engine.handle, C.byref(rows), target, thr, n_thr, C.byref(o), None)

    assert call() == pkg._lib.TVC_OK
    for kw in (dict(N=0), dict(N=E.ROC_MAX_N + 1), dict(B=0), dict(n_thr=9), dict(target=1.5), dict(target=-0.1), dict(source=1), dict(source=5)):
        assert call(**kw) == pkg._lib.TVC_E_INVALID, kw
    assert gpu_engine.workspace_bytes() == ws
    torch.cuda.synchronize()


def test_detector_threshold(pkg, fx):
    from sklearn.metrics import roc_curve
    clip = pkg.CLIPModel(pkg.CLIPConfig(model_name="ViT-T/16-test", device="cuda"))
    try:
        eng = clip.engine
        fpr, tpr, thr = roc_curve(fx["labels"], fx["scores"].astype(np.float64))
        got = pkg.AdversarialDetector.optimal_threshold_from_scores(fx["scores"], fx["labels"], engine=eng)
        assert got == thr[int(np.argmax(tpr - fpr))] == float(fx["threshold"])
        det = pkg.AdversarialDetector(pkg.DetectorConfig(clip_model="ViT-T/16-test", num_text_variants=3), clip_model=clip)
        texts = ["a cat on a sofa", "two dogs playing in the park", "a red car", "an old man reading a newspaper",
                 "a bowl of fruit on a wooden table", "city skyline at night", "a plate of food", "a child with a kite"]
        images = pkg.synth.make_images(len(texts), 64, seed=3).cuda()
        flags = [True, False, False, True, True, False, True, False]
        scores = np.array([r["aggregated_score"] for r in det.batch_detect(images, texts)])
        want = pkg.AdversarialDetector.optimal_threshold_from_scores(scores, flags, engine=eng)
        f2, t2, th2 = roc_curve(np.array(flags, int), scores.astype(np.float32).astype(np.float64))
        assert want == th2[int(np.argmax(t2 - f2))]
        got = det.compute_optimal_threshold(list(zip(images, texts, flags)))
        assert got == want and got != det.config.detection_threshold
        det.update_threshold(got)
        assert det.config.detection_threshold == got
        assert det.compute_optimal_threshold([(images[0], texts[0], True)]) == got      # one class: the configured threshold
    finally:
        clip.engine.close()
