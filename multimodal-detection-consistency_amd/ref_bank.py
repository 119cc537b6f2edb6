"""``ReferenceBank`` (``src/ref_bank.py:86``) with the similarity scan on the GPU.

The reference rebuilds an fp64 matrix from a Python list on EVERY query
(``src/ref_bank.py:475``) and scans it with numpy.  Here the vectors are kept as
a device matrix of L2-normalised rows (re-registered lazily after additions) and
``query_similar`` is one ``tvc_bank_search`` call (fp32 bank -> split-bf16
planes, fp32-grade cosines).  In scope: ``add_reference`` (admission check
included), ``query_similar``, ``_compute_similarities``, size / FIFO-LRU-random
eviction bookkeeping, similarity eviction (``_remove_most_similar``,
``src/ref_bank.py:401-427``: the reference's double loop over all pairs on every
admission at capacity is one ``TVCEngine.closest_pair`` call, ``tvc_closest_pair``,
over the bank's own slot of unit rows; ``similarity_victim`` is the access-count
rule), and the KMeans clustering (``perform_clustering``,
``query_by_cluster``, ``get_cluster_centers``, the ``auto_clustering`` hook and the
cluster bookkeeping on eviction, ``src/ref_bank.py:226-339,429-450``): the raw
vectors are registered under a second, temporary bank slot and clustered by
``TVCEngine.kmeans`` (``tvc_kmeans_assign`` / ``tvc_kmeans_update``) with the
reference's ``n_init=10``, seed 42.  The restarts draw their starting centres from
numpy's generator, not sklearn's, so the clusters are a k-means optimum of the same
data but not sklearn's own labelling.  DBSCAN (``src/ref_bank.py:302-315``) runs over
the same temporary slot through ``TVCEngine.dbscan`` (``tvc_radius_graph``, the
``tvc_dbscan_*`` component calls and ``tvc_kmeans_update`` for the centres) once
``ReferenceBankConfig.dbscan_eps`` is set -- the reference's value is 0.5, which on
raw CLIP vectors of norm ~10 makes every row noise; with the default ``None`` the
method is refused as before (an error is logged and ``perform_clustering`` returns
False).  Its labels are sklearn's own: DBSCAN is a pure function of the eps-graph.
Out of scope: JSON persistence.
"""
from __future__ import annotations

import logging
import time
from collections import deque
from dataclasses import dataclass, field
from threading import Lock
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from .engine import TVCEngine

logger = logging.getLogger(__name__)


@dataclass
class ReferenceBankConfig:
    """src/ref_bank.py:24-44."""
    max_size: int = 10000
    similarity_threshold: float = 0.9
    clustering_method: str = "none"
    num_clusters: int = 100
    update_strategy: str = "fifo"
    persistence_enabled: bool = False
    save_path: str = "./cache/ref_bank"
    auto_clustering: bool = False
    clustering_interval: int = 1000
    feature_dim: int = 512
    dbscan_eps: Optional[float] = None      # None: "dbscan" is refused; the reference hard-codes 0.5 (:304)
    dbscan_min_samples: int = 5             # :304

    def __post_init__(self):
        if self.clustering_method not in ("kmeans", "dbscan", "none"):
            raise ValueError(f"unsupported clustering method: {self.clustering_method}")
        if self.update_strategy not in ("fifo", "lru", "random", "similarity"):
            raise ValueError(f"unsupported update strategy: {self.update_strategy}")
        if self.dbscan_eps is not None and not (0.0 < float(self.dbscan_eps) < float("inf")):
            raise ValueError(f"dbscan_eps must be positive and finite, or None (got {self.dbscan_eps})")
        if int(self.dbscan_min_samples) < 1:
            raise ValueError(f"dbscan_min_samples must be >= 1 (got {self.dbscan_min_samples})")


@dataclass
class ReferenceItem:
    """src/ref_bank.py:47-83."""
    vector: np.ndarray
    metadata: Dict[str, Any]
    timestamp: float
    access_count: int = 0
    cluster_id: Optional[int] = None
    similarity_scores: Dict[str, float] = field(default_factory=dict)


def similarity_victim(access_counts, pair, pair_sim) -> Optional[int]:
    """The row ``_remove_most_similar`` (src/ref_bank.py:401-427) removes, or None: a pure function of the references'
    access counts and of the closest pair ``(i, j)``, ``i < j``, with its cosine ``pair_sim`` -- the first maximal pair of the
    reference's loops.  The victim is ``i`` if ``access_counts[i] <= access_counts[j]``, else ``j``.  The reference's quirks
    stay: with fewer than 2 references nothing is removed, and when no pair's similarity exceeds -1 (``max_similarity``
    starts at -1 and the compare is strict; also: no pair at all, ``pair`` None or (-1, -1)) index 0 goes."""
    if len(access_counts) < 2:
        return None
    if pair is None or pair[0] < 0 or pair[1] < 0 or not (pair_sim > -1.0):
        return 0
    i, j = int(pair[0]), int(pair[1])
    return i if access_counts[i] <= access_counts[j] else j


class ReferenceBank:
    def __init__(self, config: Optional[ReferenceBankConfig] = None, engine: Optional[TVCEngine] = None,
                 rng: Optional[np.random.Generator] = None):
        self.config = config or ReferenceBankConfig()
        self.engine = engine or TVCEngine()
        self.references: List[ReferenceItem] = []
        self.clusters: Dict[int, List[int]] = {}            # cluster id -> reference indices (src/ref_bank.py:98)
        self.cluster_centers: Optional[np.ndarray] = None
        self.cluster_init: Optional[np.ndarray] = None      # the starting centres of the restart the last clustering kept
        self.access_order: deque = deque()
        self._lock = Lock()
        self._dirty = True
        self._rng = rng or np.random.default_rng()
        self.bank_name = f"ref_bank:{id(self):x}"       # own bank slot on the (possibly shared) engine
        self.stats = {"total_added": 0, "total_removed": 0, "total_queries": 0, "clustering_count": 0,
                      "last_clustering_time": None}

    def __len__(self) -> int:
        return len(self.references)

    def __del__(self):          # give the bank slot back to the (possibly shared) engine
        try:
            self.engine.release_bank(self.bank_name)
        except Exception:
            pass

    # -- device copy ----------------------------------------------------------
    def _padded_dim(self) -> int:
        return (self.config.feature_dim + 63) // 64 * 64

    def _sync_device(self) -> None:
        if not self._dirty:
            return
        D, Dp = self.config.feature_dim, self._padded_dim()
        V = np.zeros((len(self.references), Dp), dtype=np.float64)
        for i, r in enumerate(self.references):
            V[i, :D] = r.vector
        n = np.linalg.norm(V, axis=1, keepdims=True)
        V = V / np.where(n == 0, 1.0, n)          # cosine = dot of unit rows; the +1e-8 of :482 is < 1e-9 here
        self.engine.set_bank(torch.from_numpy(V.astype(np.float32)).to(self.engine.device), name=self.bank_name)
        self._dirty = False

    def _query_rows(self, q: np.ndarray) -> torch.Tensor:
        D, Dp = self.config.feature_dim, self._padded_dim()
        q = np.asarray(q, dtype=np.float64).reshape(-1, D)
        n = np.linalg.norm(q, axis=1, keepdims=True)
        out = np.zeros((q.shape[0], Dp), dtype=np.float32)
        out[:, :D] = q / np.where(n == 0, 1.0, n)
        return torch.from_numpy(out).to(self.engine.device)

    # -- API ------------------------------------------------------------------
    def _compute_similarities(self, query_vector: np.ndarray) -> np.ndarray:
        """src/ref_bank.py:462-484 for ALL references (debug / parity use): the
        cosine matrix kernel instead of the top-k search."""
        if not self.references:
            return np.array([])
        from .metrics import SimilarityCalculator
        V = np.stack([r.vector for r in self.references]).astype(np.float32)
        return SimilarityCalculator.batch_cosine_similarity(np.asarray(query_vector, np.float32).reshape(1, -1), V,
                                                            engine=self.engine)[0].astype(np.float64)

    def _is_too_similar(self, vector: np.ndarray) -> bool:
        """src/ref_bank.py:340-362: the reference samples <= 100 refs with the global
        numpy RNG (non-deterministic admission); here the check is against ALL
        references (max similarity from the search), which is the sampled check's
        limit and is deterministic."""
        if not self.references:
            return False
        self._sync_device()
        _, sim, _ = self.engine.bank_search_robust(self._query_rows(vector), 1, want_moments=False, bank=self.bank_name)
        return bool(sim[0, 0].item() > self.config.similarity_threshold)

    def add_reference(self, vector: np.ndarray, metadata: Dict[str, Any]) -> bool:
        """src/ref_bank.py:123-170."""
        with self._lock:
            if self._is_too_similar(vector):
                return False
            if len(self.references) >= self.config.max_size:
                self._remove_reference()
            self.references.append(ReferenceItem(np.array(vector, dtype=np.float64), dict(metadata), time.time()))
            self.stats["total_added"] += 1
            self._dirty = True
            if self.config.auto_clustering and len(self.references) % self.config.clustering_interval == 0:   # :156-159
                self._perform_clustering()
            return True

    def add_references(self, vectors: np.ndarray, metadatas: Optional[List[Dict[str, Any]]] = None) -> None:
        """Bulk load without the admission check (e.g. a stored ``references.json``)."""
        with self._lock:
            for i, v in enumerate(vectors):
                self.references.append(ReferenceItem(np.array(v, dtype=np.float64),
                                                     dict(metadatas[i]) if metadatas else {}, time.time()))
            self.stats["total_added"] += len(vectors)
            self._dirty = True

    def _remove_most_similar(self) -> None:
        """src/ref_bank.py:401-427 (lock held): the most similar pair of stored vectors loses the member that was accessed
        less.  The reference's double loop over i < j becomes ``engine.closest_pair`` over the bank's own slot, whose unit
        fp32 rows make the scores the cosines of the raw vectors; ``similarity_victim`` picks the row."""
        pair, pair_sim = None, float("-inf")
        if len(self.references) >= 2:
            self._sync_device()
            p, s, _, _ = self.engine.closest_pair(self.bank_name)
            pair, pair_sim = tuple(int(v) for v in p.tolist()), float(s.item())
        idx = similarity_victim([r.access_count for r in self.references], pair, pair_sim)
        if idx is None:
            return
        self.references.pop(idx)
        self._update_clusters_after_removal(idx)
        self._dirty = True

    def _remove_reference(self) -> None:
        """src/ref_bank.py:364-400 (fifo / lru / random / similarity)."""
        if not self.references:
            return
        s = self.config.update_strategy
        if s == "similarity":
            self._remove_most_similar()
            self.stats["total_removed"] += 1      # :399 counts the call, also when fewer than 2 references kept their row
            return
        idx = 0
        if s == "lru" and self.access_order:
            idx = self.access_order.popleft()
            idx = idx if idx < len(self.references) else 0
        elif s == "random":
            idx = int(self._rng.integers(len(self.references)))
        self.references.pop(idx)
        self._update_clusters_after_removal(idx)
        self.stats["total_removed"] += 1
        self._dirty = True

    def _update_clusters_after_removal(self, removed_idx: int) -> None:
        """src/ref_bank.py:429-460: indices above the removed one shift down, the removed one leaves its cluster, a
        cluster left without members leaves the dict; the same for the LRU order."""
        new_clusters = {}
        for cluster_id, indices in self.clusters.items():
            kept = [i if i < removed_idx else i - 1 for i in indices if i != removed_idx]
            if kept:
                new_clusters[cluster_id] = kept
        self.clusters = new_clusters
        self.access_order = deque(i if i < removed_idx else i - 1 for i in self.access_order if i != removed_idx)

    # -- clustering -------------------------------------------------------------
    def query_by_cluster(self, cluster_id: int, top_k: int = 10) -> List[ReferenceItem]:
        """src/ref_bank.py:226-247: the first ``top_k`` members of a cluster in index order; [] for an unknown id."""
        with self._lock:
            if cluster_id not in self.clusters:
                return []
            return [self.references[i] for i in self.clusters[cluster_id][:top_k]]

    def get_cluster_centers(self) -> Optional[np.ndarray]:
        """src/ref_bank.py:249-257: a copy."""
        with self._lock:
            return self.cluster_centers.copy() if self.cluster_centers is not None else None

    def perform_clustering(self, force: bool = False) -> bool:
        """src/ref_bank.py:259-274: True when the references were clustered; failures are logged, never raised."""
        try:
            with self._lock:
                return self._perform_clustering(force)
        except Exception as e:
            logger.error(f"clustering failed: {e}")
            return False

    def _perform_clustering(self, force: bool = False) -> bool:
        """src/ref_bank.py:276-339 (lock held).  KMeans(n_clusters, random_state=42, n_init=10) over the RAW vectors
        (:294, not the unit rows of the cosine search) becomes ``engine.kmeans`` over a temporary bank slot that holds
        them zero-padded to the 64 multiple; its starting centres stay in ``self.cluster_init`` (fp64 [n_clusters, D])."""
        if len(self.references) < 2:
            return False
        method = self.config.clustering_method
        if method == "none":                 # without force :289-290; with force the method falls through to :317-318
            return False
        try:
            if method != "kmeans" and not (method == "dbscan" and self.config.dbscan_eps is not None):
                raise NotImplementedError(f"clustering method {method!r} is not built on the GPU path")
            D, Dp = self.config.feature_dim, self._padded_dim()
            V = np.zeros((len(self.references), Dp), dtype=np.float32)
            for i, r in enumerate(self.references):
                V[i, :D] = r.vector
            name = self.bank_name + ":raw"
            if method == "dbscan":
                return self._cluster_dbscan(V, name)
            n_clusters = min(self.config.num_clusters, len(self.references))
            try:
                self.engine.set_bank(torch.from_numpy(V).to(self.engine.device), name=name)
                centres, labels, _, _, order, offsets = self.engine.kmeans(n_clusters, bank=name, n_init=10, seed=42, n_features=D)
                init = self.engine.kmeans_last_init
            finally:
                self.engine.release_bank(name)
            self.cluster_centers = centres[:, :D].double().cpu().numpy()
            self.cluster_init = init[:, :D].double().cpu().numpy()
            labels, order, offsets = labels.cpu().numpy(), order.cpu().numpy(), offsets.cpu().numpy()
            self.clusters.clear()
            for j in range(n_clusters):       # the member lists come grouped and ascending from the counting sort
                if offsets[j + 1] > offsets[j]:
                    self.clusters[j] = order[offsets[j]:offsets[j + 1]].tolist()
            for i, r in enumerate(self.references):
                r.cluster_id = int(labels[i]) if labels[i] >= 0 else None
            self.stats["clustering_count"] += 1
            self.stats["last_clustering_time"] = time.time()
            logger.info(f"clustering done: {len(self.clusters)} clusters")
            return True
        except Exception as e:               # the reference's failure contract (:337-339)
            logger.error(f"clustering failed: {e}")
            return False

    def _cluster_dbscan(self, V: np.ndarray, name: str) -> bool:
        """src/ref_bank.py:302-315 (lock held): DBSCAN(eps, min_samples) over the raw vectors, the mean of every non-noise
        cluster as its centre; no cluster at all is a success with ``clusters == {}`` and no centres, as in the reference."""
        D = self.config.feature_dim
        try:
            self.engine.set_bank(torch.from_numpy(V).to(self.engine.device), name=name)
            labels, _, centres, order, offsets = self.engine.dbscan(float(self.config.dbscan_eps), int(self.config.dbscan_min_samples),
                                                                    bank=name)
        finally:
            self.engine.release_bank(name)
        self.cluster_centers = centres[:, :D].double().cpu().numpy() if centres is not None else None
        self.cluster_init = None
        labels, order, offsets = labels.cpu().numpy(), order.cpu().numpy(), offsets.cpu().numpy()
        self.clusters.clear()
        for j in range(len(offsets) - 1):         # the member lists come grouped and ascending from the counting sort
            self.clusters[j] = order[offsets[j]:offsets[j + 1]].tolist()
        for i, r in enumerate(self.references):
            r.cluster_id = int(labels[i]) if labels[i] >= 0 else None
        self.stats["clustering_count"] += 1
        self.stats["last_clustering_time"] = time.time()
        logger.info(f"clustering done: {len(self.clusters)} clusters")
        return True

    def query_similar(self, query_vector: np.ndarray, top_k: int = 10,
                      similarity_threshold: Optional[float] = None) -> List[Tuple[ReferenceItem, float]]:
        """src/ref_bank.py:172-224: sims >= threshold, sorted descending, top_k."""
        with self._lock:
            if not self.references:
                return []
            thr = similarity_threshold or self.config.similarity_threshold       # :191 (0.0 falls through)
            self._sync_device()
            # the reference accepts any top_k (src/ref_bank.py:172,203); more than the bank holds cannot come
            # back, and beyond the kernel's TVC_MAX_TOPK the engine raises -- never a silent truncation
            k = max(1, min(top_k, len(self.references)))
            idx, sim, _ = self.engine.bank_search_robust(self._query_rows(query_vector), k, thr, want_moments=False,
                                                         bank=self.bank_name)
            idx, sim = idx[0].cpu().numpy(), sim[0].cpu().numpy().astype(np.float64)
            out = []
            for i, s in zip(idx, sim):
                if i < 0 or s < thr:
                    continue
                item = self.references[int(i)]
                item.access_count += 1
                if int(i) in self.access_order:
                    self.access_order.remove(int(i))
                self.access_order.append(int(i))
                out.append((item, float(s)))
            self.stats["total_queries"] += 1
            return out

    def get_statistics(self) -> Dict[str, Any]:
        return {**self.stats, "size": len(self.references), "max_size": self.config.max_size}


def create_reference_bank(config: Optional[ReferenceBankConfig] = None, **kw) -> ReferenceBank:
    """src/ref_bank.py:727."""
    return ReferenceBank(config, **kw)
