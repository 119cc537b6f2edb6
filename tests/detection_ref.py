"""The numpy restatement of the detection evaluation (include/tvc.h, "detection evaluation"): the integer ROC sweep of sorted
fp32 scores under integer multiplicities, sklearn's curve rule, the PR arrays, Philox4x32-10 and the bootstrap dict.  Not a test
module; tests/test_detection_ref.py pins it to sklearn and to the reference's fixture, the GPU tests compare the kernels with it.

Everything that decides a result is an integer or one correctly rounded fp64 quotient of integers; AP is also given as an exact
``fractions.Fraction`` (``ap_fraction``) and, for long rows, as a Fraction within ``points * 2**-200`` of it (``ap_scaled``)."""
from fractions import Fraction

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of uint32, key: 2 -> the 4 output words as uint32 arrays."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def philox_draws(N, b, seed):
    """The N draws of resample number b: draw t = word t & 3 of the block with counter (t >> 2, b, 0, 0), key (seed lo, seed hi),
    mapped to (x * N) >> 32."""
    blocks = np.arange((N + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((blocks, b, 0, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    x = np.stack(words, 1).reshape(-1)[:N].astype(np.uint64)
    return ((x * np.uint64(N)) >> np.uint64(32)).astype(np.int64)


def philox_weights(N, B, seed, first=0):
    """int64 [B, N]: the multiplicities over the original indices of resamples first .. first + B - 1."""
    return np.stack([np.bincount(philox_draws(N, first + b, seed), minlength=N) for b in range(B)])


def prepare(scores, labels, pos_label=1):
    """-> (scores fp32 sorted descending and stably, labels 0 / 1 int64 in sorted order, order)."""
    s = np.asarray(scores, dtype=np.float32).reshape(-1) + np.float32(0.0)
    order = np.argsort(-s, kind="stable")
    return s[order], (np.asarray(labels).reshape(-1)[order] == pos_label).astype(np.int64), order


def points(ss, sl, w):
    """The points of a row: w int [N] multiplicities over the SORTED positions -> (TP, FP, pos int64 [m], kept bool [m], P, N)."""
    w = np.asarray(w, dtype=np.int64)
    ctp, cfp = np.cumsum(w * sl), np.cumsum(w * (1 - sl))
    ends = np.nonzero(np.r_[ss[1:] != ss[:-1], True])[0]
    cw = (ctp + cfp)[ends]
    pos = ends[cw > np.r_[0, cw[:-1]]]
    TP, FP = ctp[pos], cfp[pos]
    kept = np.ones(len(pos), bool)
    if len(pos) > 2:
        kept[1:-1] = (np.diff(FP, 2) != 0) | (np.diff(TP, 2) != 0)
    return TP, FP, pos, kept, int(ctp[-1]), int(cfp[-1])


def ap_fraction(TP, FP, P):
    """The exact average precision of a row's points."""
    prev, total = 0, Fraction(0)
    for tp, fp in zip(TP.tolist(), FP.tolist()):
        total += Fraction(tp - prev, P) * Fraction(tp, tp + fp)
        prev = tp
    return total


def ap_scaled(TP, FP, P, bits=200):
    """Within len(TP) * 2**-bits of ``ap_fraction`` (every term floored at 2**-bits / P), in plain integer arithmetic."""
    prev, total = 0, 0
    for tp, fp in zip(TP.tolist(), FP.tolist()):
        total += (((tp - prev) * tp) << bits) // (tp + fp)
        prev = tp
    return Fraction(total, P << bits)


ZERO_ROW = dict(n_pos=0, n_neg=0, valid=0, n_points=0, n_kept=0, auc2=0, auc=0.0, youden_j=0.0, youden_pos=0, youden_tp=0,
                youden_fp=0, target_pos=0, target_tp=0, target_fp=0)


def sweep(ss, sl, w, target=0.95, thresholds=()):
    """One row -> the dict of ``tvc_roc_sweep``'s outputs (without ap: see ``ap_fraction``), plus TP / FP / pos / kept."""
    TP, FP, pos, kept, P, Nn = points(ss, sl, w)
    n_thr = len(thresholds)
    if P == 0 or Nn == 0:
        return dict(ZERO_ROW, thr_tp=[0] * n_thr, thr_fp=[0] * n_thr, TP=TP[:0], FP=FP[:0], pos=pos[:0], kept=kept[:0])
    auc2 = int(np.sum(np.diff(np.r_[0, FP]) * (TP + np.r_[0, TP[:-1]])))
    kTP, kFP, kpos = np.r_[0, TP[kept]], np.r_[0, FP[kept]], np.r_[-1, pos[kept]]
    tpr, fpr = kTP.astype(np.float64) / np.float64(P), kFP.astype(np.float64) / np.float64(Nn)
    jd = tpr - fpr
    j = int(np.argmax(jd))
    t = int(np.argmin(np.abs(tpr - np.float64(target))))
    wl = np.asarray(w, dtype=np.int64)
    ctp, cfp = np.r_[0, np.cumsum(wl * sl)], np.r_[0, np.cumsum(wl * (1 - sl))]
    cnt = [int(np.count_nonzero(ss >= np.float32(th))) for th in thresholds]
    return dict(n_pos=P, n_neg=Nn, valid=1, n_points=len(pos), n_kept=int(kept.sum()), auc2=auc2,
                auc=float(np.float64(auc2) / (np.float64(2.0) * np.float64(P) * np.float64(Nn))),
                youden_j=float(jd[j]), youden_pos=int(kpos[j]), youden_tp=int(kTP[j]), youden_fp=int(kFP[j]),
                target_pos=int(kpos[t]), target_tp=int(kTP[t]), target_fp=int(kFP[t]),
                thr_tp=[int(ctp[c]) for c in cnt], thr_fp=[int(cfp[c]) for c in cnt], TP=TP, FP=FP, pos=pos, kept=kept)


def roc_arrays(ss, TP, FP, pos, kept, P, Nn):
    """sklearn's roc_curve arrays (fpr, tpr, thresholds) from a row's points."""
    fpr = np.r_[0.0, FP[kept].astype(np.float64) / np.float64(Nn)]
    tpr = np.r_[0.0, TP[kept].astype(np.float64) / np.float64(P)]
    return fpr, tpr, np.r_[np.inf, ss[pos[kept]].astype(np.float64)]


def pr_arrays(ss, TP, FP, pos, P):
    """sklearn's precision_recall_curve arrays (precision, recall, thresholds) from a row's points."""
    prec = TP.astype(np.float64) / (TP + FP).astype(np.float64)
    rec = TP.astype(np.float64) / np.float64(P)
    return np.r_[prec[::-1], 1.0], np.r_[rec[::-1], 0.0], ss[pos][::-1].astype(np.float64)


def confusion_metrics(tp, fp, P, Nn):
    """accuracy, precision, recall, f1 of the prediction with these counts (zero_division = 0), fp64 arrays."""
    tp, fp, P, Nn = (np.asarray(x, dtype=np.float64) for x in (tp, fp, P, Nn))
    acc = (tp + (Nn - fp)) / (P + Nn)
    prec = np.where(tp + fp > 0, tp / np.where(tp + fp > 0, tp + fp, 1.0), 0.0)
    rec = tp / P
    f1 = 2.0 * tp / (2.0 * tp + fp + (P - tp))
    return acc, prec, rec, f1


def bootstrap_dict(values, confidence=0.95):
    """The reference's summary of the kept bootstrap values (src/utils/metrics.py:857-874)."""
    values = list(values)
    if not values:
        return {"mean": 0.0, "lower": 0.0, "upper": 0.0}
    alpha = 1 - confidence
    return {"mean": np.mean(values), "lower": np.percentile(values, (alpha / 2) * 100),
            "upper": np.percentile(values, (1 - alpha / 2) * 100), "std": np.std(values)}


def score_kinds(rng, N):
    """The case classes of the tests: name -> (scores fp32 [N], labels [N] with both classes)."""
    lab = rng.integers(0, 2, N)
    lab[0], lab[-1] = 1, 0
    g = rng.standard_normal(N) + lab
    out = {
        "gaussian": (g, lab),
        "integer_ties": (rng.integers(0, max(2, N // 8), N) + lab, lab),
        "one_group": (np.full(N, 0.25), lab),
        "collinear": (np.repeat(np.arange((N + 3) // 4), 4)[:N], np.tile([1, 0, 1, 0], (N + 3) // 4)[:N]),
        "worse_than_chance": (-g, lab),
    }
    return {k: (np.asarray(s, dtype=np.float32), np.asarray(l, dtype=np.int64)) for k, (s, l) in out.items()}
