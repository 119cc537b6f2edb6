"""The numpy restatement of the retrieval evaluation (not collected by pytest): positions from a stable argsort, the metrics from
the positions, and the reference's dense form (src/utils/metrics.py:379-573) loop for loop.

Relevance: (i, j) is relevant iff qlabel[i] == glabel[j] >= 0.  Order: score descending, ties to the lower row index --
``np.argsort(-S, kind="stable")``; a NaN score sorts behind everything."""
import numpy as np


def relevance(qlabel, glabel) -> np.ndarray:
    """int64 [Q, N] of 0 / 1."""
    q, g = np.asarray(qlabel).reshape(-1, 1), np.asarray(glabel).reshape(1, -1)
    return ((q == g) & (g >= 0)).astype(np.int64)


def positions(S, qlabel, glabel):
    """-> (tgt_off int64 [Q + 1], tgt_row int64 [T], pos int64 [T]): every query's relevant rows best first, with their 0-based
    positions in the query's ranking of all rows."""
    S = np.asarray(S)
    rel = relevance(qlabel, glabel)
    off, rows, pos = [0], [], []
    for i in range(S.shape[0]):
        order = np.argsort(-S[i], kind="stable")
        at = np.flatnonzero(rel[i][order])
        rows.append(order[at])
        pos.append(at)
        off.append(off[-1] + len(at))
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)    # noqa: E731
    return np.array(off, np.int64), cat(rows), cat(pos)


def per_query(tgt_off, pos, k_values):
    """The per-query terms from the positions, in fp64: ap [Q], rr [Q], hits int64 [Q, K], dcg [Q, K], idcg [Q, K]; zeros for a
    query without a relevant row."""
    Q, K = len(tgt_off) - 1, len(k_values)
    ap, rr = np.zeros(Q), np.zeros(Q)
    hits, dcg, idcg = np.zeros((Q, K), np.int64), np.zeros((Q, K)), np.zeros((Q, K))
    for i in range(Q):
        p = np.asarray(pos[tgt_off[i]:tgt_off[i + 1]], dtype=np.float64)
        P = len(p)
        if P == 0:
            continue
        ap[i] = np.mean(np.arange(1, P + 1) / (p + 1))
        rr[i] = 1.0 / (p[0] + 1)
        for t, k in enumerate(k_values):
            top = p[p < k]
            hits[i, t] = len(top)
            dcg[i, t] = np.sum(1.0 / np.log2(top + 2))
            idcg[i, t] = np.sum(1.0 / np.log2(np.arange(min(k, P)) + 2.0))
    return ap, rr, hits, dcg, idcg


def means(tgt_off, ap, rr, hits, dcg, idcg, k_values, skip_empty=False):
    """-> dict(recall_at_k, precision_at_k, map_score, ndcg_at_k, mrr): a query without a relevant row counts as 0, or is left
    out with skip_empty (all means 0.0 when nothing is left)."""
    P = np.diff(tgt_off).astype(np.float64)
    keep = P > 0 if skip_empty else np.ones(len(P), bool)
    mean = lambda x: float(np.mean(x[keep])) if keep.any() else 0.0    # noqa: E731
    out = {"recall_at_k": {}, "precision_at_k": {}, "ndcg_at_k": {}, "map_score": mean(ap), "mrr": mean(rr)}
    for t, k in enumerate(k_values):
        out["recall_at_k"][k] = mean(np.where(P > 0, hits[:, t] / np.maximum(P, 1), 0.0))
        out["precision_at_k"][k] = mean(hits[:, t] / k)
        out["ndcg_at_k"][k] = mean(np.where(idcg[:, t] > 0, dcg[:, t] / np.where(idcg[:, t] > 0, idcg[:, t], 1.0), 0.0))
    return out


def from_labels(S, qlabel, glabel, k_values, skip_empty=False):
    off, _, pos = positions(S, qlabel, glabel)
    return means(off, *per_query(off, pos, k_values), k_values, skip_empty)


def dense(S, rel, k_values):
    """The reference's dense form, its loops restated (a stable argsort where it leaves ties open)."""
    S, rel = np.asarray(S), np.asarray(rel)
    order = np.argsort(-S, axis=1, kind="stable")
    out = {"recall_at_k": {k: [] for k in k_values}, "precision_at_k": {k: [] for k in k_values},
           "ndcg_at_k": {k: [] for k in k_values}}
    aps, rrs = [], []

    def dcg_of(r):
        return sum(float(x) / np.log2(i + 2) for i, x in enumerate(r))
    for i in range(S.shape[0]):
        sr = rel[i][order[i]]
        hit = np.flatnonzero(sr == 1)
        aps.append(float(np.mean(np.arange(1, len(hit) + 1) / (hit + 1))) if sr.sum() != 0 and len(hit) else 0.0)
        rrs.append(1.0 / (hit[0] + 1) if len(hit) else 0.0)
        total = rel[i].sum()
        for k in k_values:
            out["recall_at_k"][k].append(sr[:k].sum() / total if total != 0 else 0.0)
            out["precision_at_k"][k].append(sr[:k].sum() / k if k else 0.0)
            idcg = dcg_of(np.sort(sr)[::-1][:k])
            out["ndcg_at_k"][k].append(dcg_of(sr[:k]) / idcg if k and idcg > 0 else 0.0)
    res = {name: {k: float(np.mean(v)) for k, v in d.items()} for name, d in out.items()}
    res["map_score"], res["mrr"] = float(np.mean(aps)), float(np.mean(rrs))
    return res


def flatten(m, k_values):
    """A metrics dict (or an object with those attributes) as one fp64 vector: recall, precision, ndcg per k, then mAP, MRR."""
    get = (lambda n: m[n]) if isinstance(m, dict) else (lambda n: getattr(m, n))
    return np.array([get(n)[k] for n in ("recall_at_k", "precision_at_k", "ndcg_at_k") for k in k_values]
                    + [get("map_score"), get("mrr")], dtype=np.float64)
