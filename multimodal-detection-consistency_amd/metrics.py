"""``SimilarityCalculator`` (``src/utils/metrics.py:109-164``) over the HIP cosine
kernel, and its distances and correlations with ``SimilarityMetrics`` (``:89-106,166-276``)
over the HIP row-pair kernels; the detection metrics (``:286-376,816-874``): ``compute_detection_metrics``
stays sklearn on the host exactly as in the reference, while ``evaluate_scores``, the
ROC / PR curves and the bootstrap run over the HIP ROC-sweep kernels;
and the retrieval metrics (``:70-86,379-573,951-972``): the dense form on the host, the
label form over the HIP rank-count kernels."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, Optional, Sequence, Union

import numpy as np
import torch

from .engine import TVCEngine, _ptr, _stream

_default_engine: Optional[TVCEngine] = None


def _engine(engine: Optional[TVCEngine]) -> TVCEngine:
    global _default_engine
    if engine is not None:
        return engine
    if _default_engine is None:
        _default_engine = TVCEngine()          # consistency-only handle; raises without a GPU
    return _default_engine


@dataclass
class SimilarityMetrics:
    """src/utils/metrics.py:89-106."""
    cosine_similarity: float = 0.0
    euclidean_distance: float = 0.0
    manhattan_distance: float = 0.0
    pearson_correlation: float = 0.0
    spearman_correlation: float = 0.0

    def to_dict(self) -> Dict[str, Any]:
        return {"cosine_similarity": self.cosine_similarity, "euclidean_distance": self.euclidean_distance,
                "manhattan_distance": self.manhattan_distance, "pearson_correlation": self.pearson_correlation,
                "spearman_correlation": self.spearman_correlation}


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _nan_to_zero(v: np.ndarray) -> np.ndarray:
    return np.where(np.isnan(v), 0.0, v)


class SimilarityCalculator:
    """src/utils/metrics.py:109-276.  The scalar functions take two arrays of any shape with equally many elements, flatten
    them as the reference does, and return Python floats; each is one call of ``TVCEngine.similarity_flat`` (the row kernel up
    to 4 096 elements, the long form up to 2^20; longer inputs raise ``ValueError``).  ``rowwise_similarities`` is the batched
    form: the five metrics of B pairs of rows from one launch.  Inputs are rounded to fp32 before the kernels, as everywhere in
    this package: fp64 inputs that fp32 cannot hold are rounded first, which can create ties that the fp64 values did not
    have (Spearman sees them as ties).  Sums are fp64; formulas, specials and error bounds are in include/tvc.h.  Where the
    reference turns an undefined correlation into 0.0 (a constant input, a NaN or inf element, a single element) so do these."""

    @staticmethod
    def _pair(x, y, engine: Optional[TVCEngine]) -> np.ndarray:
        """fp64 [5] of one flattened pair: the kernel's row, NaN where it is undefined"""
        return _engine(engine).similarity_flat(_host(x), _host(y)).values[0].cpu().numpy()

    @staticmethod
    def euclidean_distance(x, y, engine: Optional[TVCEngine] = None) -> float:
        """src/utils/metrics.py:166-187."""
        return float(SimilarityCalculator._pair(x, y, engine)[1])

    @staticmethod
    def manhattan_distance(x, y, engine: Optional[TVCEngine] = None) -> float:
        """src/utils/metrics.py:189-210."""
        return float(SimilarityCalculator._pair(x, y, engine)[2])

    @staticmethod
    def pearson_correlation(x, y, engine: Optional[TVCEngine] = None) -> float:
        """src/utils/metrics.py:212-233: 0.0 where the correlation is undefined (NaN) and for a single element."""
        return float(_nan_to_zero(SimilarityCalculator._pair(x, y, engine))[3])

    @staticmethod
    def spearman_correlation(x, y, engine: Optional[TVCEngine] = None) -> float:
        """src/utils/metrics.py:235-256: 0.0 where the correlation is undefined (NaN) and for a single element."""
        return float(_nan_to_zero(SimilarityCalculator._pair(x, y, engine))[4])

    @classmethod
    def compute_all_similarities(cls, x, y, engine: Optional[TVCEngine] = None) -> SimilarityMetrics:
        """src/utils/metrics.py:258-276 from ONE kernel row: two matrices are flattened into one pair, as the reference's five
        functions flatten them.  The cosine is 0.0 for a zero vector (the reference's norm check), NaN if an element is."""
        v = cls._pair(x, y, engine)
        return SimilarityMetrics(cosine_similarity=float(v[0]), euclidean_distance=float(v[1]), manhattan_distance=float(v[2]),
                                 pearson_correlation=float(_nan_to_zero(v)[3]), spearman_correlation=float(_nan_to_zero(v)[4]))

    @staticmethod
    def rowwise_similarities(x, y, engine: Optional[TVCEngine] = None) -> Dict[str, np.ndarray]:
        """x, y [B, D], D <= 4 096 -> the reference's five names, each an fp64 array [B]: the metrics of the pairs (x[b], y[b])
        from one launch (``TVCEngine.similarity_rows``).  Undefined correlations are 0.0, as in the scalar functions."""
        v = _engine(engine).similarity_rows(_host(x), _host(y)).values.cpu().numpy()
        v[:, 3:5] = _nan_to_zero(v[:, 3:5])
        return {name: v[:, j].copy() for j, name in enumerate(SimilarityMetrics().to_dict())}

    @staticmethod
    def batch_cosine_similarity(x: Union[np.ndarray, torch.Tensor], y: Union[np.ndarray, torch.Tensor],
                                engine: Optional[TVCEngine] = None) -> np.ndarray:
        """[N, D] x [M, D] -> [N, M] cosines (src/utils/metrics.py:144-164); D is
        zero-padded to a multiple of 64 (cosines are unchanged)."""
        eng = _engine(engine)
        xt = torch.as_tensor(x, dtype=torch.float32)
        yt = torch.as_tensor(y, dtype=torch.float32)
        N, D = xt.shape
        M = yt.shape[0]
        Dp = (D + 63) // 64 * 64
        if Dp != D:
            xt = torch.nn.functional.pad(xt, (0, Dp - D))
            yt = torch.nn.functional.pad(yt, (0, Dp - D))
        xd, yd = xt.to(eng.device).contiguous(), yt.to(eng.device).contiguous()
        out = torch.empty((N, M), dtype=torch.float32, device=eng.device)
        with eng._lock, torch.cuda.device(eng.device):
            eng._check(eng.lib.tvc_cosine_matrix(eng.handle, _ptr(xd), N, _ptr(yd), M, Dp, _ptr(out), _stream()))
        return out.cpu().numpy()

    @staticmethod
    def cosine_similarity(x, y, engine: Optional[TVCEngine] = None) -> float:
        """src/utils/metrics.py:116-141: scalar cosine, 0.0 for a zero vector."""
        xa = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32).reshape(1, -1)
        ya = np.asarray(y.detach().cpu() if isinstance(y, torch.Tensor) else y, dtype=np.float32).reshape(1, -1)
        if not xa.any() or not ya.any():
            return 0.0
        return float(SimilarityCalculator.batch_cosine_similarity(xa, ya, engine)[0, 0])


@dataclass
class DetectionMetrics:
    auc: float
    accuracy: float
    precision: float
    recall: float
    f1_score: float
    fpr_at_95_tpr: float
    threshold: float
    confusion_matrix: np.ndarray

    def to_dict(self) -> Dict[str, Any]:
        """src/utils/metrics.py:55-66."""
        return {"auc": self.auc, "accuracy": self.accuracy, "precision": self.precision, "recall": self.recall,
                "f1_score": self.f1_score, "fpr_at_95_tpr": self.fpr_at_95_tpr, "threshold": self.threshold,
                "confusion_matrix": self.confusion_matrix.tolist()}


class DetectionEvaluator:
    @staticmethod
    def compute_detection_metrics(scores: np.ndarray, labels: np.ndarray, pos_label: int = 1) -> DetectionMetrics:
        """src/utils/metrics.py:286-329: roc_auc_score + Youden-J threshold."""
        from sklearn.metrics import (accuracy_score, confusion_matrix, f1_score, precision_score, recall_score,
                                     roc_auc_score, roc_curve)
        scores = np.asarray(scores, dtype=np.float64)
        labels = np.asarray(labels).astype(int)
        fpr, tpr, thr = roc_curve(labels, scores, pos_label=pos_label)
        auc = roc_auc_score(labels, scores)
        j = int(np.argmax(tpr - fpr))
        pred = (scores >= thr[j]).astype(int)
        i95 = int(np.argmin(np.abs(tpr - 0.95)))       # src/utils/metrics.py:343-344: nearest TPR
        return DetectionMetrics(
            auc=float(auc), accuracy=float(accuracy_score(labels, pred)),
            precision=float(precision_score(labels, pred, pos_label=pos_label, zero_division=0)),
            recall=float(recall_score(labels, pred, pos_label=pos_label, zero_division=0)),
            f1_score=float(f1_score(labels, pred, pos_label=pos_label, zero_division=0)),
            fpr_at_95_tpr=float(fpr[i95]), threshold=float(thr[j]),
            confusion_matrix=confusion_matrix(labels, pred))

    @staticmethod
    def from_counts(auc: float, tp: int, fp: int, n_pos: int, n_neg: int, target_fp: int, threshold: float) -> DetectionMetrics:
        """The reference's fields from the integers of a sweep row: the prediction ``score >= threshold`` has ``tp`` true and
        ``fp`` false positives among ``n_pos`` positives and ``n_neg`` negatives (zero_division = 0)."""
        acc, prec, rec, f1 = _confusion_metrics(tp, fp, n_pos, n_neg)
        return DetectionMetrics(auc=float(auc), accuracy=float(acc), precision=float(prec), recall=float(rec), f1_score=float(f1),
                                fpr_at_95_tpr=float(np.float64(target_fp) / np.float64(n_neg)), threshold=float(threshold),
                                confusion_matrix=np.array([[n_neg - fp, fp], [n_pos - tp, tp]], dtype=np.int64))

    @staticmethod
    def evaluate_scores(scores, labels, pos_label: int = 1, engine: Optional[TVCEngine] = None) -> DetectionMetrics:
        """``compute_detection_metrics`` on the GPU (``TVCEngine.roc_sweep``): scores taken as fp32, every field from the
        sweep's integers.  The Youden threshold is +inf when no threshold beats predicting nothing; it then predicts nothing."""
        sw = _engine(engine).roc_sweep(scores, labels, pos_label=pos_label)
        r = {n: getattr(sw, n)[0].item() for n in ("auc", "youden_pos", "youden_tp", "youden_fp", "n_pos", "n_neg", "target_fp")}
        return DetectionEvaluator.from_counts(r["auc"], r["youden_tp"], r["youden_fp"], r["n_pos"], r["n_neg"], r["target_fp"],
                                              sw.threshold_at(r["youden_pos"]))

    @staticmethod
    def compute_roc_curve(scores, labels, pos_label: int = 1, engine: Optional[TVCEngine] = None):
        """src/utils/metrics.py:348-360 -> (fpr, tpr, thresholds) fp64, sklearn's ``roc_curve`` (drop_intermediate) from the
        points of ``TVCEngine.roc_curve``: the origin with threshold +inf, then the kept points."""
        tp, fp, pos, kept, ss, P, Nn = _engine(engine).roc_curve(scores, labels, pos_label=pos_label)
        k = kept.bool()
        tpk, fpk = tp[k].cpu().numpy().astype(np.float64), fp[k].cpu().numpy().astype(np.float64)
        thr = ss[pos[k].long()].cpu().numpy().astype(np.float64)
        return np.r_[0.0, fpk / np.float64(Nn)], np.r_[0.0, tpk / np.float64(P)], np.r_[np.inf, thr]

    @staticmethod
    def compute_pr_curve(scores, labels, pos_label: int = 1, engine: Optional[TVCEngine] = None):
        """src/utils/metrics.py:363-376 -> (precision, recall, thresholds) fp64, sklearn's ``precision_recall_curve``: every
        point of ``TVCEngine.roc_curve`` in ascending threshold order, then (1, 0)."""
        tp, fp, pos, kept, ss, P, Nn = _engine(engine).roc_curve(scores, labels, pos_label=pos_label)
        tpa, fpa = tp.cpu().numpy().astype(np.float64), fp.cpu().numpy().astype(np.float64)
        thr = ss[pos.long()].cpu().numpy().astype(np.float64)
        return np.r_[(tpa / (tpa + fpa))[::-1], 1.0], np.r_[(tpa / np.float64(P))[::-1], 0.0], thr[::-1].copy()


def _confusion_metrics(tp, fp, n_pos, n_neg):
    """accuracy, precision, recall, f1 (zero_division = 0) of counts, scalars or arrays, in fp64"""
    tp, fp, P, Nn = (np.asarray(x, dtype=np.float64) for x in (tp, fp, n_pos, n_neg))
    some = tp + fp > 0
    return ((tp + (Nn - fp)) / (P + Nn), np.where(some, tp / np.where(some, tp + fp, 1.0), 0.0), tp / P,
            2.0 * tp / (2.0 * tp + fp + (P - tp)))


BOOTSTRAP_METRICS = ("auc", "ap", "accuracy", "precision", "recall", "f1", "fpr_at_95_tpr")


def _summary(values, confidence: float) -> Dict[str, float]:
    """src/utils/metrics.py:857-874"""
    if len(values) == 0:
        return {"mean": 0.0, "lower": 0.0, "upper": 0.0}
    alpha = 1 - confidence
    return {"mean": np.mean(values), "lower": np.percentile(values, (alpha / 2) * 100),
            "upper": np.percentile(values, (1 - alpha / 2) * 100), "std": np.std(values)}


def bootstrap_detection_metrics(scores, labels, n_bootstrap: int = 1000, confidence: float = 0.95, seed: int = 0, indices=None,
                                pos_label: int = 1, engine: Optional[TVCEngine] = None) -> Dict[str, Dict[str, float]]:
    """The bootstrap of every metric of ``BOOTSTRAP_METRICS`` from ONE sweep of ``n_bootstrap`` resamples: name -> the
    reference's dict (mean, lower, upper, std).  The resamples are Philox draws on the device (``seed``) or the caller's
    ``indices`` int [B, N] (any host RNG: ``np.random.choice(n, size=n, replace=True)`` per row reproduces the reference's).
    accuracy / precision / recall / f1 are taken at the FULL sample's Youden threshold; resamples with one class are dropped,
    as the reference drops the metric's exception; the percentiles are ``np.percentile`` over the kept values."""
    eng = _engine(engine)
    full = eng.roc_sweep(scores, labels, pos_label=pos_label)
    thr = full.threshold_at(int(full.youden_pos[0]))
    sw = eng.roc_sweep(scores, labels, n_resamples=0 if indices is not None else int(n_bootstrap), indices=indices, seed=seed,
                       thresholds=(thr,), pos_label=pos_label)
    r = {n: getattr(sw, n)[1:].cpu().numpy() for n in ("valid", "auc", "ap", "n_pos", "n_neg", "target_fp", "thr_tp", "thr_fp")}
    ok = r["valid"] == 1
    P, Nn = r["n_pos"][ok], r["n_neg"][ok]
    acc, prec, rec, f1 = _confusion_metrics(r["thr_tp"][ok, 0], r["thr_fp"][ok, 0], P, Nn)
    values = {"auc": r["auc"][ok], "ap": r["ap"][ok], "accuracy": acc, "precision": prec, "recall": rec, "f1": f1,
              "fpr_at_95_tpr": r["target_fp"][ok].astype(np.float64) / Nn.astype(np.float64)}
    return {name: _summary(values[name], confidence) for name in BOOTSTRAP_METRICS}


def bootstrap_metric(metric, scores, labels, n_bootstrap: int = 1000, confidence: float = 0.95, seed: int = 0, indices=None,
                     engine: Optional[TVCEngine] = None) -> Dict[str, float]:
    """src/utils/metrics.py:816-874.  ``metric`` is one of ``BOOTSTRAP_METRICS`` (the GPU sweep: ``bootstrap_detection_metrics``)
    or a callable, which keeps the reference's host loop: ``metric(scores[idx], labels[idx])`` over ``np.random.choice`` draws
    of the legacy global stream (or the rows of ``indices``), values that are not a number and calls that raise dropped."""
    if callable(metric):
        args = [np.asarray(scores), np.asarray(labels)]
        n = len(args[0])
        if n == 0:
            return {"mean": 0.0, "lower": 0.0, "upper": 0.0}
        values = []
        for b in range(n_bootstrap if indices is None else len(indices)):
            idx = np.random.choice(n, size=n, replace=True) if indices is None else np.asarray(indices[b])
            try:
                v = metric(*[a[idx] for a in args])
            except Exception:
                continue
            if isinstance(v, (int, float)) and not np.isnan(v):
                values.append(v)
        return _summary(values, confidence)
    if metric not in BOOTSTRAP_METRICS:
        raise ValueError(f"metric must be a callable or one of {BOOTSTRAP_METRICS} (got {metric!r})")
    return bootstrap_detection_metrics(scores, labels, n_bootstrap, confidence, seed, indices, engine=engine)[metric]


@dataclass
class RetrievalMetrics:
    """src/utils/metrics.py:70-86."""
    recall_at_k: Dict[int, float]
    precision_at_k: Dict[int, float]
    map_score: float
    ndcg_at_k: Dict[int, float]
    mrr: float

    def to_dict(self) -> Dict[str, Any]:
        return {"recall_at_k": self.recall_at_k, "precision_at_k": self.precision_at_k, "map_score": self.map_score,
                "ndcg_at_k": self.ndcg_at_k, "mrr": self.mrr}


def _mean(x: np.ndarray) -> float:
    return float(x.sum() / x.size) if x.size else 0.0


class RetrievalEvaluator:
    """src/utils/metrics.py:379-573.  ``compute_retrieval_metrics`` keeps the reference's dense interface on the host;
    ``evaluate_retrieval`` (the function ``MetricsCalculator.calculate_retrieval_metrics`` forwards to, which the reference
    never defines) takes embeddings and labels and ranks on the GPU without a [Q, N] matrix (``TVCEngine.retrieval_ranks``)."""

    @staticmethod
    def compute_retrieval_metrics(similarities: np.ndarray, relevance: np.ndarray,
                                  k_values: Sequence[int] = (1, 5, 10, 20, 50)) -> RetrievalMetrics:
        """similarities [Q, N], relevance [Q, N] of 0 / 1 -> the reference's metrics, vectorised numpy.  The reference's
        semantics: a query without a relevant column counts as 0 in every mean, a k beyond N takes all N columns and still
        divides Precision@K by k.  Ties are ranked (similarity descending, column ascending) -- the reference's plain
        ``argsort`` leaves them unspecified."""
        S = np.asarray(similarities)
        rel = np.asarray(relevance)
        Q, N = S.shape
        order = np.argsort(-S, axis=1, kind="stable")
        srel = np.take_along_axis(rel, order, axis=1).astype(np.float64)
        isrel = srel == 1
        nrel = isrel.sum(1)
        some = nrel > 0
        prec = np.cumsum(isrel, 1) / np.arange(1, N + 1, dtype=np.float64)
        ap = np.where(some, (prec * isrel).sum(1) / np.maximum(nrel, 1), 0.0)
        rr = np.where(some, 1.0 / (np.argmax(isrel, 1) + 1.0), 0.0) if N else np.zeros(Q)
        total = rel.sum(1).astype(np.float64)
        disc = 1.0 / np.log2(np.arange(2, N + 2, dtype=np.float64))
        ideal = -np.sort(-srel, axis=1)
        recall, precision, ndcg = {}, {}, {}
        for k in k_values:
            got = srel[:, :k].sum(1)
            recall[k] = _mean(np.where(total > 0, got / np.where(total > 0, total, 1.0), 0.0))
            precision[k] = _mean(got / k) if k else 0.0
            dcg = (srel[:, :k] * disc[:k]).sum(1)
            idcg = (ideal[:, :k] * disc[:k]).sum(1)
            ndcg[k] = _mean(np.where(idcg > 0, dcg / np.where(idcg > 0, idcg, 1.0), 0.0)) if k else 0.0
        return RetrievalMetrics(recall_at_k=recall, precision_at_k=precision, map_score=_mean(ap), ndcg_at_k=ndcg, mrr=_mean(rr))

    @staticmethod
    def from_ranks(ranks, skip_empty_queries: bool = False) -> RetrievalMetrics:
        """The means over the queries of a ``RetrievalRanks``, in fp64.  A query without a relevant row counts as 0 in every
        mean (src/utils/metrics.py:469-470,511-512,558), or is left out with ``skip_empty_queries`` (the convention of
        experiments/utils/metrics.py:195; all means are then 0.0 when no query has a relevant row)."""
        P = ranks.n_targets.cpu().numpy().astype(np.float64)
        ap, rr = ranks.ap.cpu().numpy(), ranks.rr.cpu().numpy()
        hits, dcg, idcg = ranks.hits.cpu().numpy().astype(np.float64), ranks.dcg.cpu().numpy(), ranks.idcg.cpu().numpy()
        keep = P > 0 if skip_empty_queries else np.ones(P.shape, bool)
        safe_p = np.where(P > 0, P, 1.0)
        recall, precision, ndcg = {}, {}, {}
        for t, k in enumerate(ranks.k_values):
            recall[k] = _mean(np.where(P > 0, hits[:, t] / safe_p, 0.0)[keep])
            precision[k] = _mean((hits[:, t] / k)[keep])
            ndcg[k] = _mean(np.where(idcg[:, t] > 0, dcg[:, t] / np.where(idcg[:, t] > 0, idcg[:, t], 1.0), 0.0)[keep])
        return RetrievalMetrics(recall_at_k=recall, precision_at_k=precision, map_score=_mean(ap[keep]), ndcg_at_k=ndcg,
                                mrr=_mean(rr[keep]))

    @staticmethod
    def rank_embeddings(query_embeddings, gallery_embeddings, query_labels, gallery_labels, k_values: Sequence[int] = (1, 5, 10),
                        engine: Optional[TVCEngine] = None, normalize: bool = True):
        """-> ``RetrievalRanks`` of the queries over the gallery: rows L2-normalised in fp32 (``normalize``), D zero-padded to a
        multiple of 64 as ``batch_cosine_similarity`` does, the gallery registered as an fp32 bank in a slot of its own and
        released afterwards."""
        eng = _engine(engine)
        q = torch.as_tensor(query_embeddings, dtype=torch.float32).to(eng.device)
        g = torch.as_tensor(gallery_embeddings, dtype=torch.float32).to(eng.device)
        if q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
            raise ValueError(f"need [Q, D] queries and [N, D] gallery rows (got {tuple(q.shape)}, {tuple(g.shape)})")
        if normalize:
            q, g = torch.nn.functional.normalize(q, p=2, dim=1), torch.nn.functional.normalize(g, p=2, dim=1)
        D = q.shape[1]
        Dp = (D + 63) // 64 * 64
        if Dp != D:
            q, g = torch.nn.functional.pad(q, (0, Dp - D)), torch.nn.functional.pad(g, (0, Dp - D))
        name = f"retrieval-eval:{id(q):x}"
        eng.set_bank(g.contiguous(), name=name)
        try:
            return eng.retrieval_ranks(q.contiguous(), query_labels, gallery_labels, bank=name, k_values=tuple(k_values))
        finally:
            eng.release_bank(name)

    @staticmethod
    def evaluate_retrieval(query_embeddings, gallery_embeddings, query_labels, gallery_labels,
                           k_values: Sequence[int] = (1, 5, 10), engine: Optional[TVCEngine] = None, normalize: bool = True,
                           skip_empty_queries: bool = False) -> RetrievalMetrics:
        """Recall@K / Precision@K / mAP / NDCG@K / MRR of label-defined retrieval: gallery row j is relevant to query i iff
        ``query_labels[i] == gallery_labels[j] >= 0``.  Equals ``compute_retrieval_metrics`` on the cosine matrix and the
        label-equality matrix, computed on the GPU from rank counts (``rank_embeddings``, ``from_ranks``)."""
        ranks = RetrievalEvaluator.rank_embeddings(query_embeddings, gallery_embeddings, query_labels, gallery_labels, k_values,
                                                   engine, normalize)
        return RetrievalEvaluator.from_ranks(ranks, skip_empty_queries)


class MetricsCalculator:
    """src/utils/metrics.py:877-972: the reference's front door to the three evaluators, each on its GPU path."""

    def __init__(self, engine: Optional[TVCEngine] = None):
        self.engine = engine
        self.similarity_calculator = SimilarityCalculator()
        self.detection_evaluator = DetectionEvaluator()
        self.retrieval_evaluator = RetrievalEvaluator()

    def calculate_retrieval_metrics(self, query_embeddings, gallery_embeddings, query_labels, gallery_labels,
                                    k_values: Sequence[int] = (1, 5, 10)) -> RetrievalMetrics:
        return self.retrieval_evaluator.evaluate_retrieval(query_embeddings, gallery_embeddings, query_labels, gallery_labels,
                                                           k_values, engine=self.engine)


    def calculate_detection_metrics(self, predictions, labels) -> DetectionMetrics:
        """src/utils/metrics.py:921-933 (``DetectionEvaluator.evaluate_scores``: the ROC sweep on the GPU)."""
        return self.detection_evaluator.evaluate_scores(predictions, labels, engine=self.engine)

    def calculate_similarity_metrics(self, embeddings1, embeddings2) -> Dict[str, float]:
        """src/utils/metrics.py:935-949: ``compute_all_similarities`` of the two matrices, flattened into one pair, as a dict."""
        return self.similarity_calculator.compute_all_similarities(embeddings1, embeddings2, engine=self.engine).to_dict()

    def calculate_all_metrics(self, predictions, labels, embeddings1=None, embeddings2=None) -> Dict[str, Any]:
        """src/utils/metrics.py:888-919 -> {'detection': the detection fields as a dict} and, when both matrices are given,
        {'similarity': the five similarity metrics}."""
        results: Dict[str, Any] = {"detection": self.calculate_detection_metrics(predictions, labels).to_dict()}
        if embeddings1 is not None and embeddings2 is not None:
            results["similarity"] = self.calculate_similarity_metrics(embeddings1, embeddings2)
        return results
