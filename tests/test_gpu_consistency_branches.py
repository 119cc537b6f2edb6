"""Every decision branch of ``consistency_kernel`` (csrc/consistency.hip) against the CPU oracle.

The kernel's output depends on decisions (threshold filters, greedy de-duplication, the top-k cut, the
``> 0`` filter of the four modal scores), so the inputs here are crafted, not random: vectors are built
from a seeded fp64 orthonormal basis, every cosine that feeds a decision has a closed form, and the
generator asserts in fp64 that each such quantity is either at least ``MARGIN`` from its threshold or an
exact case that fp32 and fp64 decide identically (``_assert_margins``).

Three parts:

1. ``_oracle_record``: the record of one query, joined from ``oracle/tvc_oracle.py``.
2. the scenarios, run on the GPU through ``gpu_engine.consistency`` (plus the path through the bank and
   the host-side refusals of ``tvc_consistency``).
3. ``_record_np(..., mutate=...)``: a numpy restatement with named single-point mutations; the CPU tests
   prove that the unmutated restatement equals the oracle and that every mutation is caught by at least
   one scenario, i.e. that the scenario set can tell a wrong kernel.
"""
import ctypes as C
import functools
import re
from dataclasses import dataclass, field
from pathlib import Path
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional

import numpy as np
import pytest

from oracle import tvc_oracle

TOL = 1e-4            # BASELINE.json: consistency scores within 1e-4 (the bar of test_consistency_vs_oracle)
MARGIN = 1e-3         # distance of every decision quantity from its threshold: ~1000x the fp32 dot error at D <= 1024
MUTANT_GAP = 1e-3     # a mutation counts as caught when a record moves by more than 10x TOL
MAXREF = 16           # TVC_REC_MAXREF
COS_EPS = 1e-8
_NAMES = tvc_oracle.ConsistencyCheckerOracle._NAMES
SRC_WEIGHT_PAIRS = ((0.4, 0.2), (0.0, 0.2), (0.4, 0.0), (0.0, 0.0))    # the oracle's SRC_WEIGHTS are fixed

_CFG_DEFAULTS = dict(reference_count=5, similarity_threshold=0.3, retrieval_top_k=10, dup_threshold=0.95,
                     w_text_variants=0.4, w_consistency=0.2, w_exp=(0.25, 0.25, 0.25, 0.25))


def _cfg(**kw):
    d = dict(_CFG_DEFAULTS)
    d.update(kw)
    return SimpleNamespace(**d)


# ----------------------------------------------------------------------------------------------------
# part 1: the reference record, fp64, from oracle/tvc_oracle.py
# ----------------------------------------------------------------------------------------------------
def _src_methods(cfg):
    wt, wc = cfg.w_text_variants, cfg.w_consistency
    assert (wt, wc) in SRC_WEIGHT_PAIRS, "the oracle's src weights are fixed at 0.4 / 0.2 (or off)"
    return tuple(m for m, w in (("text_variants", wt), ("consistency", wc)) if w > 0)


def _pack(head, sv, kept_idx, kept_cos):
    idx = np.full(MAXREF, -1, np.int64)
    cos = np.zeros(MAXREF)
    idx[:len(kept_idx)] = kept_idx
    cos[:len(kept_cos)] = kept_cos
    return {"head": np.asarray(head, np.float64), "sv": np.asarray(sv, np.float64), "kept_idx": idx,
            "count": len(kept_idx), "kept_cos": cos}


def _oracle_record(img, txt, ref_idx, ref_sim, ref_feat, cfg):
    """Fields [0..10], the N variant similarities, kept indices (-1 padded), count and kept cosines of one query."""
    img = np.asarray(img, np.float64)
    txt = np.asarray(txt, np.float64)
    N1 = txt.shape[0]
    cand_idx, cand_feat = [], []
    if ref_idx is not None and ref_idx.shape[-1] > 0:
        # retrieve_references on an already sorted result list: first reference_count, sim >= threshold
        take = min(cfg.reference_count, ref_idx.shape[-1], ref_feat.shape[-2])
        for n in range(N1):
            for j in range(take):
                if ref_idx[n, j] >= 0 and np.float32(ref_sim[n, j]) >= np.float32(cfg.similarity_threshold):
                    cand_idx.append(int(ref_idx[n, j]))
                    cand_feat.append(np.asarray(ref_feat[n, j], np.float64))
    # the body of generate_retrieval_references: dedupe, then cut
    keep = tvc_oracle.deduplicate_references(cand_feat, cfg.dup_threshold)[:cfg.retrieval_top_k] if cand_feat else []
    kept_idx = [cand_idx[p] for p in keep]
    kept_feat = np.stack([cand_feat[p] for p in keep]) if keep else None
    s = tvc_oracle.compute_consistency_scores_exp(img, txt, kept_feat)
    overall = tvc_oracle.ConsistencyCheckerOracle(adaptive_threshold=False,
                                                  weights=dict(zip(_NAMES, cfg.w_exp))).overall(s)
    src = tvc_oracle.detect_adversarial_src(img, txt, methods=_src_methods(cfg))
    s0 = s["original_similarity"]
    sv = [tvc_oracle.cosine(img, t) for t in txt[1:]]
    head = [s0, s["text_variant_consistency"], s["text_variant_std"], tvc_oracle.text_variant_score(s0, sv)[0],
            tvc_oracle.consistency_score(s0)[0], src["aggregated_score"], s["retrieval_consistency"],
            s["retrieval_std"], float(len(keep)), s["cross_modal_variance"], overall]
    kept_cos = [tvc_oracle.cosine(img, f) for f in kept_feat] if keep else []
    return _pack(head, sv, kept_idx, kept_cos)


# ----------------------------------------------------------------------------------------------------
# part 3 (restatement): plain numpy, with named single-point mutations
# ----------------------------------------------------------------------------------------------------
MUTATIONS = ("dup_ge", "thr_gt", "dedupe_first_only", "cut_before_dedupe", "filter_before_take", "ignore_holes",
             "sign_ge", "var_ddof1", "vote_unfiltered", "n0_drops_tv", "mean_over_N1")


def _cos(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return float(np.dot(a, b) / (max(float(np.linalg.norm(a)), COS_EPS) * max(float(np.linalg.norm(b)), COS_EPS)))


def _record_np(img, txt, ref_idx, ref_sim, ref_feat, cfg, mutate=None):
    assert mutate is None or mutate in MUTATIONS
    img = np.asarray(img, np.float64)
    txt = np.asarray(txt, np.float64)
    N = txt.shape[0] - 1
    ddof = 1 if mutate == "var_ddof1" else 0

    def std(x):
        return float(np.std(x, ddof=ddof)) if len(x) > ddof else 0.0

    cands = []                                      # (bank id, feature row)
    if ref_idx is not None and ref_idx.shape[-1] > 0:
        ks, kf = ref_idx.shape[-1], ref_feat.shape[-2]
        thr = np.float32(cfg.similarity_threshold)
        for n in range(N + 1):
            def ok(j):
                hole = ref_idx[n, j] < 0 and mutate != "ignore_holes"
                sim = np.float32(ref_sim[n, j])
                return not hole and (sim > thr if mutate == "thr_gt" else sim >= thr)
            if mutate == "filter_before_take":      # filter the whole row, then take reference_count
                js = [j for j in range(min(ks, kf)) if ok(j)][:max(cfg.reference_count, 0)]
            else:
                js = [j for j in range(min(cfg.reference_count, ks, kf)) if ok(j)]
            cands += [(int(ref_idx[n, j]), np.asarray(ref_feat[n, j], np.float64)) for j in js]
    if mutate == "cut_before_dedupe":
        cands = cands[:cfg.retrieval_top_k]
    kept = []
    for cid, f in cands:
        against = kept[:1] if mutate == "dedupe_first_only" else kept
        if mutate == "dup_ge":
            dup = any(_cos(f, g) >= cfg.dup_threshold for _, g in against)
        else:
            dup = any(_cos(f, g) > cfg.dup_threshold for _, g in against)
        if not dup:
            kept.append((cid, f))
    kept = kept[:cfg.retrieval_top_k]

    s0 = _cos(img, txt[0])
    sv = [_cos(img, t) for t in txt[1:]]
    mv = ([s0] + sv) if mutate == "mean_over_N1" else sv
    mean, sd = (float(np.mean(mv)), std(sv)) if N > 0 else (s0, 0.0)
    # src polarity
    tv = 1.0 - ((1.0 - abs(s0 - mean)) * 0.7 + (1.0 - sd) * 0.3) if N > 0 else 0.0
    cs = 1.0 - s0
    terms = []
    if cfg.w_text_variants > 0 and not (mutate == "n0_drops_tv" and N == 0):
        terms.append((tv, cfg.w_text_variants))
    if cfg.w_consistency > 0:
        terms.append((cs, cfg.w_consistency))
    ws = tw = 0.0
    for x, w in terms:
        ws += x * w
        tw += w
    agg = ws / tw if tw > 0 else 0.0
    # exp polarity
    rc = [_cos(img, f) for _, f in kept]
    rmean, rsd = (float(np.mean(rc)), std(rc)) if rc else (0.0, 0.0)
    four = [s0, mean, rmean, 0.0]
    present = [(x >= 0 if mutate == "sign_ge" else x > 0) for x in four]
    valid = [x for x, p in zip(four, present) if p]
    xvar = float(np.var(valid, ddof=ddof)) if len(valid) >= 2 else 0.0
    ws = tw = 0.0
    for x, p, w in zip(four, present, cfg.w_exp):
        if p:
            ws += x * w
        if p or mutate == "vote_unfiltered":
            tw += w
    overall = ws / tw if tw != 0 else 0.0
    head = [s0, mean, sd, tv, cs, agg, rmean, rsd, float(len(kept)), xvar, overall]
    return _pack(head, sv, [cid for cid, _ in kept], rc)


def _record_gap(a, b):
    """Largest deviation of the continuous fields; inf when the kept indices or the count differ."""
    if a["count"] != b["count"] or not np.array_equal(a["kept_idx"], b["kept_idx"]):
        return float("inf")
    return max(float(np.abs(a[k] - b[k]).max()) if a[k].size else 0.0 for k in ("head", "sv", "kept_cos"))


# ----------------------------------------------------------------------------------------------------
# part 2: scenario generator
# ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _basis(D, seed):
    """Columns: a seeded fp64 orthonormal basis of R^D (QR of a Gaussian)."""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((D, D)))
    return q


class _Query:
    """One query: image [D], text [N+1, D], ref_idx / ref_sim [N+1, ks], ref_feat [N+1, kf, D].

    ``e0`` is the image direction.  ``at(base, c)`` returns a unit vector at cosine ``c`` to the unit vector
    ``base`` by mixing in a basis direction nobody has used yet, so cosines multiply along chains:
    ``cos(at(at(e0, a), b), e0) = a * b``, and two vectors made from different fresh directions off ``e0``
    at cosines a, b have cosine ``a * b`` with each other."""

    def __init__(self, D, N, ks, kf, seed, img_norm=3.0):
        self.D, self.N, self.ks, self.kf = D, N, ks, kf
        self.E = _basis(D, seed)
        self.used = 1
        self.e0 = self.E[:, 0].copy()
        self.img = img_norm * self.e0
        self.txt = np.zeros((N + 1, D))
        self.idx = np.full((N + 1, ks), -1, np.int32)
        self.sim = np.zeros((N + 1, ks), np.float32)
        self.feat = np.zeros((N + 1, kf, D))
        self.want_kept = None

    def fresh(self):
        assert self.used < self.D, "out of unused basis directions"
        self.used += 1
        return self.E[:, self.used - 1]

    def at(self, base, c):
        return c * base + np.sqrt(1.0 - c * c) * self.fresh()

    def texts(self, cosines, zero=()):
        assert len(cosines) == self.N + 1
        for n, c in enumerate(cosines):
            self.txt[n] = 0.0 if n in zero else (0.7 + 0.15 * n) * self.at(self.e0, c)
        return self

    def ref(self, n, j, rid, sim, vec=None, scale=None):
        self.idx[n, j] = rid
        self.sim[n, j] = np.float32(sim)
        if j < self.kf and vec is not None:
            self.feat[n, j] = (0.5 + 0.25 * ((n + j) % 5) if scale is None else scale) * vec
        return vec

    def fill_unique(self, c_img=0.6, sims=None, first_id=100):
        """Every slot a distinct row at cosine ``c_img`` to the image (pairwise cosine c_img^2), sorted sims."""
        rid = first_id
        for n in range(self.N + 1):
            for j in range(self.ks):
                s = (0.9 - 0.02 * j) if sims is None else sims[j]
                self.ref(n, j, rid, s, self.at(self.e0, c_img) if j < self.kf else None)
                rid += 1
        return self

    def arrays(self):
        f32 = lambda x: np.ascontiguousarray(x, np.float32)
        if self.ks == 0:
            return f32(self.img), f32(self.txt), None, None, None
        return f32(self.img), f32(self.txt), self.idx.copy(), self.sim.copy(), f32(self.feat)


@dataclass
class _Scenario:
    name: str
    cfg: SimpleNamespace
    N: int
    D: int
    ks: int
    kf: int
    queries: List[_Query] = field(default_factory=list)

    def query(self, seed=None, **kw):
        q = _Query(self.D, self.N, self.ks, self.kf, seed=1000 + len(self.queries) if seed is None else seed, **kw)
        self.queries.append(q)
        return q

    def batch(self):
        """fp32 arrays of the whole batch, as the kernel receives them."""
        parts = [q.arrays() for q in self.queries]
        img = np.stack([p[0] for p in parts])
        txt = np.stack([p[1] for p in parts])
        if self.ks == 0:
            return img, txt, None, None, None
        return img, txt, np.stack([p[2] for p in parts]), np.stack([p[3] for p in parts]), np.stack([p[4] for p in parts])


def _disjoint(a, b):
    return not np.any((a != 0) & (b != 0))


def _away(x, thr, what):
    assert abs(x - thr) >= MARGIN, f"{what}: {x!r} is within {MARGIN} of {thr!r}"


def _assert_margins(img, txt, ref_idx, ref_sim, ref_feat, cfg, where):
    """fp64 check on the fp32 inputs: every decision quantity is >= MARGIN from its threshold, or exact:
    a ref_sim bit-equal to float32(threshold) or one ulp below it, or a dot product that is exactly 0 because
    the two vectors have disjoint support (a zero vector included)."""
    img64, txt64 = img.astype(np.float64), txt.astype(np.float64)
    thr32 = np.float32(cfg.similarity_threshold)
    below32 = np.nextafter(thr32, np.float32(-np.inf), dtype=np.float32)
    cand = []
    if ref_idx is not None:
        take = min(cfg.reference_count, ref_idx.shape[-1], ref_feat.shape[-2])
        for n in range(ref_idx.shape[0]):
            for j in range(ref_idx.shape[1]):
                if ref_idx[n, j] < 0:
                    continue
                s = np.float32(ref_sim[n, j])
                if s != thr32 and s != below32:
                    _away(float(s), float(thr32), f"{where}: ref_sim[{n},{j}] against similarity_threshold")
                if j < take and s >= thr32:
                    cand.append(ref_feat[n, j].astype(np.float64))
    kept = []
    for c, f in enumerate(cand):                       # every cosine the dedupe can look at, not only up to the first hit
        dup = False
        for u, g in enumerate(kept):
            x = _cos(f, g)
            if not _disjoint(f, g):
                _away(x, cfg.dup_threshold, f"{where}: cos(candidate {c}, kept {u}) against dup_threshold")
            else:
                assert x == 0.0
            dup = dup or x > cfg.dup_threshold
        if not dup:
            kept.append(f)
    kept = kept[:cfg.retrieval_top_k]

    def score(members, what):
        """mean of cosines with the image: away from 0, or exactly 0 because every member is a disjoint-support zero"""
        vals = [_cos(img64, m) for m in members]
        if all(_disjoint(img64, m) for m in members):
            assert all(v == 0.0 for v in vals)
            return 0.0
        x = float(np.mean(vals))
        _away(x, 0.0, f"{where}: {what} against the > 0 filter")
        return x

    s0 = score([txt64[0]], "original_similarity")
    mean = score(list(txt64[1:]), "variant mean") if txt.shape[0] > 1 else s0
    rmean = score(kept, "retrieval mean") if kept else 0.0
    # tw != 0 and wsum > 0: decided identically by the fp32 weights the kernel receives and the oracle's doubles
    for w in (cfg.w_exp, [np.float32(x) for x in cfg.w_exp]):
        tw = sum(float(x) for x, s in zip(w, (s0, mean, rmean, 0.0)) if s > 0)
        assert tw == 0.0 or abs(tw) >= MARGIN, f"{where}: total weight {tw!r}"
    assert (cfg.w_text_variants, cfg.w_consistency) in SRC_WEIGHT_PAIRS


_BUILDERS: Dict[str, Callable[[], _Scenario]] = {}


def _scenario(name, N=3, D=64, ks=5, kf=5, **cfg):
    """Register ``fn(scenario)`` as the builder of scenario ``name``; building asserts the margin rule."""
    def deco(fn):
        def build():
            s = _Scenario(name, _cfg(**cfg), N, D, ks, kf)
            fn(s)
            assert s.queries
            for b, q in enumerate(s.queries):
                _assert_margins(*q.arrays(), s.cfg, f"{name}[{b}]")
            return s
        assert name not in _BUILDERS
        _BUILDERS[name] = build
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def _built(name) -> _Scenario:
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def _oracle_records(name):
    s = _built(name)
    return [_oracle_record(*q.arrays(), s.cfg) for q in s.queries]


POS = (0.62, 0.55, 0.5, 0.45)        # default text cosines for N = 3: everything comfortably positive


def _f32_below(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf), dtype=np.float32)


# ---- similarity threshold ----
def _thr_edge(s):
    thr = np.float32(s.cfg.similarity_threshold)
    q = s.query().texts(POS[:2])
    for n, first in ((0, 10), (1, 20)):
        sims = [0.9, thr, _f32_below(thr), 0.1, 0.05] if n == 0 else [thr, _f32_below(thr), 0.2, 0.1, 0.05]
        for j, sim in enumerate(sims):
            q.ref(n, j, first + j, sim, q.at(q.e0, 0.6))
    q.want_kept = [10, 11, 20]      # bit-equal kept, one ulp below dropped


_scenario("thr0.3_bit_equal_kept_ulp_below_dropped", N=1, D=64)(_thr_edge)
_scenario("thr0.5_bit_equal_kept_ulp_below_dropped", N=1, D=100, similarity_threshold=0.5)(_thr_edge)


@_scenario("thr_row_all_below", N=2, D=512)
def _(s):
    q = s.query().texts(POS[:3])
    q.fill_unique(sims=[0.25, 0.2, 0.15, 0.1, 0.05])
    q.ref(1, 0, 7, 0.8, q.at(q.e0, 0.6))
    q.ref(1, 1, 8, 0.31, q.at(q.e0, 0.6))
    q.want_kept = [7, 8]


@_scenario("thr_unsorted_row_first_count_then_filter", N=1, D=1024, ks=6, kf=6, reference_count=3)
def _(s):
    """ref_sim rows that are not non-increasing are outside what the reference can produce; include/tvc.h pins
    what the kernel does with them: the first reference_count entries, in order, then the filters."""
    q = s.query().texts(POS[:2])
    for n in range(2):
        for j, sim in enumerate([0.2, 0.6, 0.1, 0.7, 0.8, 0.9]):
            q.ref(n, j, 10 * (n + 1) + j, sim, q.at(q.e0, 0.6))
    q.want_kept = [11, 21]


# ---- holes ----
@_scenario("holes_start_middle_end", N=1, D=100)
def _(s):
    q = s.query().texts(POS[:2])
    q.fill_unique()
    for n, j in ((0, 0), (1, 1), (1, 4)):
        q.ref(n, j, -1, 0.9)
        q.feat[n, j] = 0.0                       # what tvc_bank_gather writes for idx < 0
    q.want_kept = [101, 102, 103, 104, 105, 107, 108]


@_scenario("holes_whole_query", N=2, D=64)
def _(s):
    q = s.query().texts(POS[:3])
    for n in range(3):
        for j in range(5):
            q.ref(n, j, -1, 0.9)
    q.want_kept = []


# ---- counts ----
def _counts(rc, ks, kf, N=1, D=64):
    @_scenario(f"count_rc{rc}_ks{ks}_kf{kf}", N=N, D=D, ks=ks, kf=kf, reference_count=rc)
    def _(s):
        q = s.query().texts(POS[:N + 1])
        q.fill_unique(sims=[0.9 - 0.02 * j for j in range(ks)])
        take = min(rc, ks, kf)
        q.want_kept = [100 + n * ks + j for n in range(N + 1) for j in range(take)][:10]


for _rc, _ks, _kf, _D in ((1, 1, 1, 64), (1, 3, 1, 100), (1, 3, 3, 512), (5, 3, 3, 1024), (5, 3, 5, 64), (5, 5, 2, 100),
                          (5, 20, 5, 512), (5, 7, 6, 1024), (8, 8, 8, 64), (8, 10, 9, 100), (8, 5, 5, 512), (0, 5, 5, 64)):
    _counts(_rc, _ks, _kf, D=_D)


# ---- dedupe ----
@_scenario("dup_0.952_dropped_0.948_kept", N=1, D=512)
def _(s):
    q = s.query().texts(POS[:2])
    f0 = q.ref(0, 0, 10, 0.9, q.at(q.e0, 0.6), scale=1.0)
    q.ref(0, 1, 11, 0.8, q.at(f0, 0.952), scale=2.5)
    q.ref(0, 2, 12, 0.7, q.at(f0, 0.948), scale=0.3)
    q.ref(1, 0, 13, 0.9, q.at(q.e0, 0.6))
    q.want_kept = [10, 12, 13]


@_scenario("dup_of_third_kept_not_first", N=1, D=1024)
def _(s):
    q = s.query().texts(POS[:2])
    fs = [q.ref(0, j, 10 + j, 0.9 - 0.1 * j, q.at(q.e0, 0.5), scale=1.0) for j in range(3)]
    q.ref(0, 3, 13, 0.5, q.at(fs[2], 0.98))
    q.ref(0, 4, 14, 0.4, q.at(q.e0, 0.5))
    q.ref(1, 0, 15, 0.9, q.at(fs[1], 0.99))
    q.want_kept = [10, 11, 12, 14]


@_scenario("dup_near_a_rejected_row_is_kept", N=1, D=64)
def _(s):
    """Greedy, no transitive closure: f2 is 0.97 from the rejected f1 and 0.9409 from the kept f0."""
    q = s.query().texts(POS[:2])
    f0 = q.ref(0, 0, 10, 0.9, q.at(q.e0, 0.6), scale=1.0)
    f1 = q.ref(0, 1, 11, 0.8, q.at(f0, 0.97), scale=1.0)
    q.ref(0, 2, 12, 0.7, q.at(f1, 0.97))
    q.want_kept = [10, 12]


@_scenario("dup_same_id_from_two_text_rows", N=2, D=100)
def _(s):
    q = s.query().texts(POS[:3])
    f = {rid: q.at(q.e0, 0.55) for rid in (5, 6, 7, 8)}
    for n, ids in enumerate(((5, 6), (6, 7), (5, 8))):
        for j, rid in enumerate(ids):
            q.ref(n, j, rid, 0.9 - 0.1 * j, f[rid], scale=1.0)
    q.want_kept = [5, 6, 7, 8]


@_scenario("dup_two_ids_identical_features", N=1, D=512)
def _(s):
    q = s.query().texts(POS[:2])
    f = q.at(q.e0, 0.6)
    q.ref(0, 0, 5, 0.9, f, scale=1.0)
    q.ref(0, 1, 9, 0.8, f, scale=1.0)
    q.ref(1, 0, 3, 0.9, f, scale=4.0)            # the same direction at another norm
    q.ref(1, 1, 4, 0.8, q.at(q.e0, 0.6))
    q.want_kept = [5, 4]


@_scenario("dup_zero_norm_rows_are_never_duplicates", N=1, D=1024)
def _(s):
    q = s.query().texts(POS[:2])
    q.ref(0, 0, 10, 0.9, q.at(q.e0, 0.6))
    q.ref(0, 1, 8, 0.8, np.zeros(s.D))
    q.ref(0, 2, 9, 0.7, np.zeros(s.D))           # cos(0, 0) clamps to 0 too
    q.ref(0, 3, 11, 0.6, q.at(q.e0, 0.6))
    q.want_kept = [10, 8, 9, 11]


@_scenario("dupthr_0.5", N=1, D=64, dup_threshold=0.5)
def _(s):
    q = s.query().texts(POS[:2])
    f0 = q.ref(0, 0, 10, 0.9, q.at(q.e0, 0.6))   # rows off e0 at 0.6: pairwise 0.36
    q.ref(0, 1, 11, 0.8, q.at(q.e0, 0.6))
    q.ref(0, 2, 12, 0.7, q.at(f0, 0.6))
    q.ref(0, 3, 13, 0.6, q.at(f0, 0.4))
    q.ref(1, 0, 14, 0.9, q.at(q.e0, 0.9))        # 0.54 against both rows off e0
    q.want_kept = [10, 11, 13]


@_scenario("dupthr_0.999", N=1, D=100, dup_threshold=0.999)
def _(s):
    q = s.query().texts(POS[:2])
    f0 = q.ref(0, 0, 10, 0.9, q.at(q.e0, 0.6), scale=1.0)
    q.ref(0, 1, 11, 0.8, q.at(f0, 0.997))
    q.ref(0, 2, 12, 0.7, f0, scale=1.0)
    q.ref(0, 3, 13, 0.6, q.at(f0, 0.96))
    q.want_kept = [10, 11, 13]


@_scenario("dupthr_-1_everything_after_the_first", N=2, D=512, dup_threshold=-1.0)
def _(s):
    q = s.query().texts(POS[:3]).fill_unique()
    q.ref(0, 1, 101, 0.88, q.at(q.e0, -0.6))     # cos -0.36 with the first: still > -1
    q.want_kept = [100]


def _blocks(D, nblk, seed):
    """nblk unit vectors with pairwise disjoint support (consecutive coordinate blocks)."""
    w = D // nblk
    out = np.zeros((nblk, D))
    rng = np.random.default_rng(seed)
    for i in range(nblk):
        v = rng.standard_normal(w)
        out[i, i * w:(i + 1) * w] = v / np.linalg.norm(v)
    return out


@_scenario("dupthr_0_exactly_orthogonal_rows_are_kept", N=1, D=100, dup_threshold=0.0)
def _(s):
    """cos exactly 0 by disjoint support against dup_threshold 0: `>` keeps the row, `>=` would drop it."""
    q = s.query()
    u = _blocks(s.D, 5, 77)
    e = (u[0] + u[1] + u[2] + u[3]) / 2.0        # cos 0.5 with each of u0..u3
    q.img = 3.0 * e
    q.txt[0] = 0.7 * (0.6 * e + 0.8 * u[4])
    q.txt[1] = 1.3 * (0.5 * e + np.sqrt(0.75) * u[4])
    q.ref(0, 0, 10, 0.9, u[0])
    q.ref(0, 1, 11, 0.8, u[1])
    q.ref(0, 2, 12, 0.7, u[2])
    q.ref(0, 3, 13, 0.6, 0.3 * u[0] + np.sqrt(0.91) * u[3])       # 0.3 with row 10: duplicate
    q.ref(0, 4, 14, 0.5, -0.3 * u[1] + np.sqrt(0.91) * u[3])      # -0.3 with row 11, 0 with 10 and 12: kept
    q.want_kept = [10, 11, 12, 14]


# ---- top_k ----
def _topk(k):
    @_scenario(f"topk_{k}" + ("_with_more_remaining" if k == 16 else ""), N=3, D=(64, 100, 512, 1024)[k % 4],
               retrieval_top_k=k)
    def _(s):
        q = s.query().texts(POS).fill_unique()
        q.want_kept = list(range(100, 100 + min(k, 20)))


for _k in (0, 1, 10, 16):
    _topk(_k)


@_scenario("topk_dedupe_then_cut_not_cut_then_dedupe", N=2, D=100)
def _(s):
    """15 candidates; candidates 3 and 6 duplicate earlier ones, so candidates 10 and 11 are the 9th and 10th
    unique rows: present after dedupe-then-cut, absent after cut-then-dedupe.  Candidate 12 is cut."""
    q = s.query().texts(POS[:3]).fill_unique()
    q.ref(0, 3, 103, 0.84, q.at(q.feat[0, 1] / np.linalg.norm(q.feat[0, 1]), 0.99))
    q.ref(1, 1, 106, 0.88, q.at(q.feat[0, 0] / np.linalg.norm(q.feat[0, 0]), 0.97))
    q.want_kept = [100, 101, 102, 104, 105, 107, 108, 109, 110, 111]


# ---- caps ----
@_scenario("cap_320_candidates_all_unique", N=39, D=512, ks=8, kf=8, reference_count=8, retrieval_top_k=16)
def _(s):
    q = s.query().texts([0.6 - 0.005 * n for n in range(40)]).fill_unique()
    q.want_kept = list(range(100, 116))


@_scenario("cap_320_candidates_nine_unique_last_one_new", N=39, D=1024, ks=8, kf=8, reference_count=8)
def _(s):
    """320 candidates over 9 directions; the 9th direction arrives as candidate 319, so the dedupe loop
    must run its full length."""
    q = s.query().texts([0.6 - 0.005 * n for n in range(40)])
    dirs = [q.at(q.e0, 0.5 + 0.03 * i) for i in range(9)]
    c = 0
    for n in range(40):
        for j in range(8):
            d = 8 if c == 319 else c % 8
            q.ref(n, j, 100 + c, 0.9 - 0.02 * j, dirs[d], scale=0.5 + (c % 7))
            c += 1
    q.want_kept = list(range(100, 108)) + [419]


@_scenario("N0_with_references", N=0, D=64)
def _(s):
    q = s.query().texts([0.62]).fill_unique()
    q.want_kept = [100, 101, 102, 103, 104]


@_scenario("N1_with_references", N=1, D=100)
def _(s):
    q = s.query().texts([0.62, 0.4]).fill_unique()
    q.want_kept = list(range(100, 110))


@_scenario("D1", N=3, D=1, ks=2, kf=2)
def _(s):
    q = s.query()
    q.img = np.array([3.0])
    q.txt[:, 0] = [0.5, 2.0, -1.5, 4.0]          # s0 = 1, variants 1, -1, 1
    q.ref(0, 0, 4, 0.9, np.array([2.0]), scale=1.0)
    q.ref(0, 1, 9, 0.8, np.array([0.5]), scale=1.0)
    q.ref(1, 0, 4, 0.9, np.array([2.0]), scale=1.0)
    q.ref(2, 0, 6, 0.9, np.array([7.0]), scale=1.0)
    q.want_kept = [4]


# ---- sign filters ----
def _signs(name, texts, c_ref, D=64, **cfg):
    @_scenario(name, N=3, D=D, **cfg)
    def _(s):
        q = s.query().texts(texts)
        if c_ref is not None:
            q.fill_unique(c_img=c_ref)


_signs("sign_s0_negative_variant_mean_positive", (-0.4, 0.55, 0.5, 0.45), 0.6, D=64)
_signs("sign_s0_positive_variant_mean_negative", (0.5, -0.55, -0.5, 0.2), 0.6, D=100)
_signs("sign_only_retrieval_positive_nv1", (-0.3, -0.55, -0.5, 0.2), 0.6, D=512)
_signs("sign_none_positive_nv0", (-0.3, -0.55, -0.5, 0.2), -0.5, D=1024)
_signs("sign_retrieval_mean_negative", POS, -0.5, D=64)
_signs("wexp_nonuniform", POS, 0.7, D=100, w_exp=(0.1, 0.2, 0.3, 0.4))
_signs("wexp_zero_weight_on_a_present_score", POS, 0.7, D=512, w_exp=(0.0, 0.5, 0.25, 0.25))
_signs("wexp_sums_to_zero_over_present_scores", POS, -0.5, D=1024, w_exp=(0.5, -0.5, 0.25, 0.25))
_signs("wexp_all_weight_on_an_absent_score", POS, -0.5, D=64, w_exp=(0.0, 0.0, 1.0, 0.0))
_signs("src_s0_minus_mean_greater_than_1", (0.8, -0.5, -0.6, -0.4), 0.6, D=100)


@_scenario("sign_s0_exactly_zero_by_disjoint_support", N=2, D=100)
def _(s):
    q = s.query()
    u = _blocks(s.D, 5, 78)
    e = (u[0] + u[1]) / np.sqrt(2.0)
    q.img = 3.0 * e
    q.txt[0] = 0.7 * u[2]                                         # disjoint from the image: s0 == 0 in any precision
    q.txt[1] = 1.1 * (0.5 * e + np.sqrt(0.75) * u[3])
    q.txt[2] = 0.4 * (0.3 * e + np.sqrt(0.91) * u[3])
    for j in range(3):
        q.ref(0, j, 10 + j, 0.9 - 0.1 * j, 0.6 * e + 0.8 * _blocks(s.D, 5, 80 + j)[4])
    # rows 10..12 share block 4 with random directions: pairwise 0.36 + 0.64 * cos(random 20-vectors)


# ---- src polarity ----
def _src(wt, wc, N, D):
    @_scenario(f"src_w[{wt},{wc}]_N{N}", N=N, D=D, ks=0, kf=0, w_text_variants=wt, w_consistency=wc)
    def _(s):
        s.query().texts((0.62, 0.2, 0.5, -0.3)[:N + 1])


for _i, (_wt, _wc) in enumerate(SRC_WEIGHT_PAIRS):
    _src(_wt, _wc, 3, (64, 100, 512, 1024)[_i])
    _src(_wt, _wc, 0, (100, 512, 1024, 64)[_i])


# ---- degenerate vectors ----
@_scenario("zero_image_row", N=3, D=512)
def _(s):
    q = s.query().texts(POS).fill_unique()
    q.img = np.zeros(s.D)
    q.want_kept = list(range(100, 110))


@_scenario("zero_text_rows", N=3, D=1024)
def _(s):
    s.query().texts(POS, zero=(2,)).fill_unique()                 # a zero variant row
    s.query().texts(POS, zero=(0,)).fill_unique()                 # a zero original row: s0 == 0 exactly
    s.query().texts(POS, zero=(0, 1, 2, 3)).fill_unique(c_img=-0.5)


# ---- grid ----
GRID_B = 4099


def _grid_kinds():
    """Fillers of one (N = 3, D = 100, ks = 6, kf = 5, default config) query each; the grid case cycles through them."""
    def plain(q, t):
        q.texts((0.62 - t, 0.55, 0.5 - t, 0.45)).fill_unique(c_img=0.6 - t)

    def dup(q, t):
        q.texts((0.5 + t, 0.55, 0.5, 0.45 - t)).fill_unique()
        q.ref(0, 2, 102, 0.86, q.at(q.feat[0, 0] / np.linalg.norm(q.feat[0, 0]), 0.97))
        q.ref(2, 1, 100, 0.88, q.feat[0, 0], scale=1.0)

    def holes(q, t):
        q.texts((0.62, 0.55 - t, 0.5, 0.45)).fill_unique()
        for n, j in ((0, 0), (1, 2), (3, 4)):
            q.ref(n, j, -1, 0.9)
            q.feat[n, j] = 0.0

    def below(q, t):
        q.texts((0.3 + t, 0.55, 0.5, 0.45)).fill_unique(sims=[0.9, 0.5, 0.25, 0.2, 0.1, 0.05], c_img=0.7 - t)

    def s0_neg(q, t):
        q.texts((-0.4 - t, 0.55, 0.5, 0.45)).fill_unique()

    def mean_neg(q, t):
        q.texts((0.5, -0.55 - t, -0.5, 0.2)).fill_unique()

    def r_neg(q, t):
        q.texts(POS).fill_unique(c_img=-0.5 - t)

    def zero_img(q, t):
        q.texts(POS).fill_unique()
        q.img = np.zeros(q.D)

    def no_refs(q, t):
        q.texts((0.62, 0.2 + t, 0.5, -0.3))
        q.sim[:] = 0.9                                            # ids stay -1

    return (plain, dup, holes, below, s0_neg, mean_neg, r_neg, zero_img, no_refs)


def _grid(s, B):
    kinds = _grid_kinds()
    for b in range(B):
        q = s.query(seed=2000 + b % 31)
        kinds[b % len(kinds)](q, 0.2 * (b // len(kinds)) / max(1, B // len(kinds)))


@_scenario("grid_B1", N=3, D=100, ks=6, kf=5)
def _(s):
    _grid(s, 1)


@_scenario(f"grid_B{GRID_B}_a_different_case_per_query", N=3, D=100, ks=6, kf=5)
def _(s):
    _grid(s, GRID_B)


SCENARIOS = tuple(_BUILDERS)
REQUIRED_D = {1, 64, 100, 512, 1024}


# ----------------------------------------------------------------------------------------------------
# CPU tests: the generator keeps its margins, the restatement is the oracle, every mutant is caught
# ----------------------------------------------------------------------------------------------------
def test_config_defaults_are_the_package_defaults(pkg):
    c = pkg.ConsistencyConfig()
    for k, v in _CFG_DEFAULTS.items():
        assert getattr(c, k) == v, k


@pytest.mark.parametrize("name", SCENARIOS)
def test_scenario_margins_and_expected_branch(name):
    """Building asserts the margin rule (``_assert_margins``); the oracle must also take the branch the id names."""
    s = _built(name)
    assert all(q.N == s.N and q.D == s.D for q in s.queries)
    for q, rec in zip(s.queries, _oracle_records(name)):
        if q.want_kept is not None:
            assert rec["kept_idx"][:rec["count"]].tolist() == q.want_kept


def test_scenario_set_covers_the_issue_list():
    assert {_built(n).D for n in SCENARIOS} == REQUIRED_D
    recs = {n: _oracle_records(n)[0] for n in SCENARIOS if not n.startswith("grid_B4")}
    head = lambda n: recs[n]["head"]
    assert recs["holes_whole_query"]["count"] == 0 and head("holes_whole_query")[6] == head("holes_whole_query")[7] == 0
    assert recs["count_rc0_ks5_kf5"]["count"] == 0 and recs["topk_0"]["count"] == 0
    assert recs["topk_16_with_more_remaining"]["count"] == 16 and recs["cap_320_candidates_all_unique"]["count"] == 16
    h = head("sign_only_retrieval_positive_nv1")       # nv = 1: variance 0, vote = that one score
    assert h[0] < 0 and h[1] < 0 and h[6] > 0 and h[9] == 0 and h[10] == pytest.approx(h[6], abs=1e-15)
    h = head("sign_none_positive_nv0")
    assert max(h[0], h[1], h[6]) < 0 and h[9] == 0 and h[10] == 0
    assert head("sign_s0_exactly_zero_by_disjoint_support")[0] == 0
    assert head("sign_retrieval_mean_negative")[6] < 0 < head("sign_retrieval_mean_negative")[0]
    assert head("wexp_sums_to_zero_over_present_scores")[10] == 0 and head("wexp_all_weight_on_an_absent_score")[10] == 0
    h = head("src_s0_minus_mean_greater_than_1")
    assert abs(h[0] - h[1]) > 1
    assert head("src_w[0.0,0.0]_N3")[5] == 0 and head("src_w[0.0,0.0]_N0")[5] == 0
    h = head("src_w[0.4,0.2]_N0")                       # the 0.0 text-variant score still enters the mean
    assert h[5] == pytest.approx(0.2 * h[4] / 0.6, abs=1e-15)
    assert not np.any(head("zero_image_row")[[0, 1, 2, 6, 7, 9, 10]])
    assert len(_built(f"grid_B{GRID_B}_a_different_case_per_query").queries) == GRID_B


def test_unsorted_ref_sim_contract_is_documented():
    """The kernel does not sort: include/tvc.h says what a caller must pass and what happens otherwise;
    `thr_unsorted_row_first_count_then_filter` pins the behaviour."""
    text = re.sub(r"[\s*]+", " ", (Path(__file__).resolve().parents[1] / "include" / "tvc.h").read_text())
    assert "each ref_sim row must be non-increasing over its entries with ref_idx >= 0" in text
    assert "looks at the first min(reference_count, ks, kf) entries of each row, in order" in text


def test_reference_restatement_equals_oracle():
    for name in SCENARIOS:
        s = _built(name)
        for b, (q, want) in enumerate(zip(s.queries, _oracle_records(name))):
            gap = _record_gap(_record_np(*q.arrays(), s.cfg), want)
            assert gap < 1e-12, f"{name}[{b}]: restatement differs from the oracle by {gap}"


def _catchers(mutation):
    out = []
    for name in SCENARIOS:
        s = _built(name)
        want = _oracle_records(name)
        nq = min(len(s.queries), len(_grid_kinds()))      # the big grid repeats its kinds: one round is enough here
        if any(_record_gap(_record_np(*s.queries[b].arrays(), s.cfg, mutate=mutation), want[b]) > MUTANT_GAP
               for b in range(nq)):
            out.append(name)
    return out


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_every_mutant_is_caught(mutation):
    caught = _catchers(mutation)
    print(f"[mutant] {mutation}: caught by {len(caught)} scenarios, first {caught[:3]}")
    assert caught, f"no scenario tells `{mutation}` from the oracle: the scenario list is incomplete"


# ----------------------------------------------------------------------------------------------------
# GPU tests
# ----------------------------------------------------------------------------------------------------
def _gpu_records(rec, N):
    """Split a [B, rec_stride(N)] fp32 record array into the same fields as ``_pack``."""
    out = []
    for r in rec:
        kept = r[12 + N:12 + N + MAXREF].copy().view(np.int32).astype(np.int64)
        out.append({"head": r[:11].astype(np.float64), "sv": r[12:12 + N].astype(np.float64), "kept_idx": kept,
                    "count": int(r[8]), "kept_cos": r[12 + N + MAXREF:12 + N + 2 * MAXREF].astype(np.float64)})
    return out


def _assert_record(got, want, where):
    assert got["head"][8] == want["count"], f"{where}: kept {got['head'][8]} references, oracle {want['count']}"
    assert got["kept_idx"].tolist() == want["kept_idx"].tolist(), f"{where}: kept indices"
    dev = _record_gap(got, want)
    assert np.isfinite(got["head"]).all() and dev < TOL, f"{where}: |gpu - oracle| = {dev}"
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENARIOS)
def test_consistency_branches_vs_oracle(gpu_engine, pkg, name):
    import torch
    s = _built(name)
    img, txt, idx, sim, feat = s.batch()
    cfg = pkg.ConsistencyConfig(**vars(s.cfg))
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    if idx is None:
        rec = gpu_engine.consistency(dev(img), dev(txt), cfg)
    else:
        B, N1 = idx.shape[:2]
        rec = gpu_engine.consistency(dev(img), dev(txt), cfg, dev(idx.reshape(B * N1, s.ks)),
                                     dev(sim.reshape(B * N1, s.ks)), dev(feat.reshape(B * N1, s.kf, s.D)))
    rec = rec.cpu().numpy()
    assert rec.shape == (len(s.queries), pkg._lib.rec_stride(s.N))
    assert not rec[:, 11].any()
    worst = 0.0
    for b, (got, want) in enumerate(zip(_gpu_records(rec, s.N), _oracle_records(name))):
        worst = max(worst, _assert_record(got, want, f"{name}[{b}]"))
    print(f"[measured] consistency branches {name}: B {len(s.queries)} max |gpu - oracle| {worst:.2e}")


def _bank_cases():
    """(id, bank rows fp64 [R, 128], text cosine plan): banks smaller than search_k, and exact duplicate rows."""
    E = _basis(128, 4242)
    r0, r1, r2 = E[:, 1], 0.5 * E[:, 1] + np.sqrt(0.75) * E[:, 2], E[:, 3]
    return (("R1", np.stack([r0])), ("R3", np.stack([r0, r1, r2])),
            ("R6_duplicate_rows", np.stack([r0, r0, r1, r1, r2, r0])))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bf16", "fp32"])
@pytest.mark.parametrize("case", [c[0] for c in _bank_cases()])
def test_branches_through_the_bank(gpu_engine, pkg, case, fmt):
    """detect_embeddings on banks with fewer rows than search_k (the search pads with -1, tvc_bank_gather writes
    zero rows) and with exact duplicate rows, against tvc_oracle.detect_batch.  Text rows sit at cosines
    0.8 / 0.5 / 0.1 / ~0 to the bank rows, so every similarity is >= 0.04 from the 0.3 threshold."""
    import torch
    bank64 = dict(_bank_cases())[case]
    E = _basis(128, 4242)
    B, N, D = 3, 2, 128
    img = np.zeros((B, D)); txt = np.zeros((B, N + 1, D))
    for b in range(B):
        img[b] = (2.0 + b) * (0.6 * E[:, 1] + 0.5 * E[:, 3] + np.sqrt(1 - 0.61) * E[:, 10 + b])
        for n, (c1, c3) in enumerate(((0.8, 0.1), (0.5, 0.5), (0.1, 0.8))):
            txt[b, n] = c1 * E[:, 1] + c3 * E[:, 3] + np.sqrt(1 - c1 * c1 - c3 * c3) * E[:, 20 + 3 * b + n]
    bank = torch.from_numpy(bank64).float()
    bank = bank.to(torch.bfloat16) if fmt == "bf16" else bank
    img32, txt32 = torch.from_numpy(img).float(), torch.from_numpy(txt).float()
    ref = tvc_oracle.detect_batch(img32.numpy(), txt32.numpy(), bank.float().numpy(),
                                  checker=tvc_oracle.ConsistencyCheckerOracle(adaptive_threshold=False))
    S = txt32.double().reshape(-1, D) @ bank.double().t()
    assert (S - 0.3).abs().min().item() >= 0.04                    # margin of the threshold decision
    P = bank.double() @ bank.double().t()
    assert ((P - 0.95).abs() >= 0.04).all()                         # margin of the dedupe decision
    cfg = pkg.ConsistencyConfig()
    assert bank.shape[0] < cfg.search_k or "duplicate" in case
    gpu_engine.set_bank(bank.cuda())
    rec = gpu_engine.detect_embeddings(img32.cuda(), txt32.cuda(), cfg).cpu().numpy()
    gpu_engine.bank_status()
    # tie order among bit-identical bank rows is not the reference's to define (numpy's argsort and faiss differ);
    # tvc.h promises ascending index, so the GPU keeps the first copy and the oracle's index maps onto it
    first = [min(j for j in range(len(bank64)) if np.array_equal(bank64[j], bank64[i])) for i in range(len(bank64))]
    worst = 0.0
    for b, got in enumerate(_gpu_records(rec, N)):
        want = [first[i] for i in ref["retrieval_indices"][b] if i >= 0]
        assert got["count"] == len(want) and got["kept_idx"][:len(want)].tolist() == want, f"{case}[{b}]"
        assert (got["kept_idx"][len(want):] == -1).all()
        for col, key in ((0, "original_similarity"), (1, "variant_mean"), (2, "variant_std"), (5, "score_src"),
                         (6, "retrieval_consistency"), (7, "retrieval_std"), (9, "cross_modal_variance"),
                         (10, "overall_exp")):
            worst = max(worst, abs(got["head"][col] - ref[key][b]))
        worst = max(worst, np.abs(got["sv"] - ref["variant_similarities"][b]).max())
    assert (ref["retrieval_indices"] >= 0).any()
    print(f"[measured] consistency through the bank {case} {fmt}: max |gpu - oracle| {worst:.2e}")
    assert worst < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["N+1>40", "(N+1)*reference_count>320", "retrieval_top_k=17", "retrieval_top_k<0",
                                  "ks>0_NULL_ref_feat", "ks>0_kf=0"])
def test_consistency_refusals(gpu_engine, pkg, what):
    """Host-side argument checks: TVC_E_INVALID, tvc_last_error set, the record buffer untouched, no launch."""
    import torch
    N, D, ks, kf, kw = 3, 64, 5, 5, {}
    null_feat = False
    if what == "N+1>40":
        N = 40
    elif what == "(N+1)*reference_count>320":
        N, kw = 39, dict(reference_count=9)
    elif what == "retrieval_top_k=17":
        kw = dict(retrieval_top_k=17)
    elif what == "retrieval_top_k<0":
        kw = dict(retrieval_top_k=-1)
    elif what == "ks>0_NULL_ref_feat":
        null_feat = True
    else:
        kf = 0
    B, N1 = 2, N + 1
    img = torch.ones((B, D), device="cuda:0")
    txt = torch.ones((B, N1, D), device="cuda:0")
    idx = torch.zeros((B * N1, ks), dtype=torch.int32, device="cuda:0")
    sim = torch.ones((B * N1, ks), device="cuda:0")
    feat = torch.ones((B * N1, max(kf, 1), D), device="cuda:0")
    rec = torch.full((B, pkg._lib.rec_stride(N)), -12345.0, device="cuda:0")
    p = pkg.ConsistencyConfig(**kw).to_c()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = gpu_engine.lib.tvc_consistency(gpu_engine.handle, ptr(img), ptr(txt), B, N, D, ptr(idx), ptr(sim),
                                        C.c_void_p(0) if null_feat else ptr(feat), ks, kf, C.byref(p), ptr(rec),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == pkg._lib.TVC_E_INVALID
    assert b"tvc_consistency" in gpu_engine.lib.tvc_last_error(gpu_engine.handle)
    torch.cuda.synchronize()
    assert (rec == -12345.0).all()
