"""``SimilarityCalculator`` (``src/utils/metrics.py:109-164``) over the HIP cosine
kernel, ``DetectionEvaluator.compute_detection_metrics`` (``:286-329``), which
stays sklearn on the host exactly as in the reference, and the
retrieval metrics (``:70-86,379-573,951-972``): the dense form on the host, the
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


class SimilarityCalculator:
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
    """The retrieval half of src/utils/metrics.py:951-972 (its detection half is ``DetectionEvaluator``)."""

    def __init__(self, engine: Optional[TVCEngine] = None):
        self.engine = engine
        self.similarity_calculator = SimilarityCalculator()
        self.detection_evaluator = DetectionEvaluator()
        self.retrieval_evaluator = RetrievalEvaluator()

    def calculate_retrieval_metrics(self, query_embeddings, gallery_embeddings, query_labels, gallery_labels,
                                    k_values: Sequence[int] = (1, 5, 10)) -> RetrievalMetrics:
        return self.retrieval_evaluator.evaluate_retrieval(query_embeddings, gallery_embeddings, query_labels, gallery_labels,
                                                           k_values, engine=self.engine)
