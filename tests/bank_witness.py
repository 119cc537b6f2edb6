"""Witnesses of the exact top-k bank search (csrc/bank.hip): inputs whose right answer is known exactly, a plain model of
the search in the kernel's own three passes, and a table of one-line defects.  No GPU, no fixtures: the CPU suite
(tests/test_bank_witness.py) proves that every defect turns a probe red, the GPU suite (tests/test_gpu_bank_witness.py) makes
the kernels reproduce the model bit for bit through the same ``check_*`` functions.

Exactness.  Every maker builds banks and queries whose bf16 planes multiply and add without rounding: all entries are
multiples of a power of two (the ``unit`` of a plane), ``sum |b||q| < 2^24`` units for every (row, query) -- so every
partial sum of every accumulation, in any order, is an integer number of units below 2^24 and fp32 holds it -- and
``max |b||q| <= 2^16`` units inside one accumulation, so the exactness never rests on how the matrix pipe rounds its running
sum (csrc/skinny.hpp: it does not round to nearest; a sum that needs no rounding does not care).  ``assert_exact`` checks
both, and ``model`` checks that every similarity it returns is an fp32 number.  No tolerance is needed anywhere.

tau is the one quantity the model cannot reproduce bit for bit (hipcc contracts ``kth_finish``'s arithmetic into fused
multiply-adds as it sees fit), and it is not an output.  The model evaluates it in fp32 as written and demands that no
similarity of the probe lies within ``guard`` of it, or that such rows cannot matter -- listed or not, they reach no cap
and stay below k certain survivors (``decided``): the outputs are then the same under any contraction.
``guard`` is four ulp of the larger term of tau (its slack, 1e-6 (1 + |v|), is 8 ulp or more up to |v| = 2^20), plus -- for data that is NOT exact (``acc_err``, the one user is the
degenerate bank of tests/test_gpu_path.py::test_bank_search_overflow_is_reported) -- the fp32 accumulation bound
``D * 2^-24 * sum |b||q|`` on both sides of the comparison.

What cannot be isolated: the ``bl * ql`` term of the margin is ~2^-18 of the similarities, below the ``4e-6 (1 + bh qh)``
term beside it, so no probe can need it; and the position of the row that decides ``bank_bounds[0]`` (max |bank hi|) cannot
decide a result inside the exactness limits above (a tau row needs nearly the winner's norm to beat its one-product
value), so the row-position probes (d) decide on ``bank_bounds[1]`` only.  Neither is pretended to be tested.
"""
from dataclasses import dataclass, field

import numpy as np
import torch

CAP, POOL, KEFF, TILE = 128, 6144, 16, 256
f32 = np.float32
NINF = -np.inf

# form -> (one-product filter + re-scoring, sample partition, moments).  "filter" = bank_filter_ring_kernel and
# bank_search_kernel<true> (same products, same lists), "skinny" = skinny stream + skinny sample, "skinny_ds" = skinny stream
# + dense sample, "dense" = tvc_bank_search_dense (no lists at all)
FORMS = {"moments": (False, "dense", True), "products": (False, "dense", False), "filter": (True, "dense", False),
         "skinny": (True, "skinny", False), "skinny_ds": (True, "dense", False), "dense": (False, None, True)}


def form_of(R, M, D, bf16_bank, want_moments, allow_filter=True, skinny=True, skinny_sample=True):
    """launch_bank_search's choice (csrc/bank.hip), restated."""
    if want_moments:
        return "moments"
    if not allow_filter or D > 2048:
        return "products"
    if skinny and 1 <= M <= 64 and D in (128, 512, 768):
        return "skinny" if (skinny_sample and bf16_bank) else "skinny_ds"
    return "filter"


def plan(R, M, k):
    """bank_plan of csrc/host_plan.hpp (pinned against the header by tests/test_bank_witness.py) and pass 1's cut."""
    nbt = (R + TILE - 1) // TILE
    nqt = (M + TILE - 1) // TILE
    s = max(1, min((1280 + nqt - 1) // nqt, nbt))
    tpc = (nbt + s - 1) // s
    s = (nbt + tpc - 1) // tpc
    keff = max(k, KEFF)
    ns = max(keff * R // (8 * s), keff * R // (256 if M <= 2048 else 2048), 4096)
    ns_cap = max(65536, min(262144, (8 << 30) // (max(M, 1) * 4)))
    ns = min(ns, ns_cap)
    ns = max(1, min((ns + 255) // 256 * 256, R))
    s_min = min((keff * R + 24 * ns - 1) // (24 * ns), nbt)
    if s < s_min:
        tpc2 = (nbt + s_min - 1) // s_min
        s = (nbt + tpc2 - 1) // tpc2
    return {"n_sample": ns, "stride": max(R // ns, 1), "S": s, "nqt": nqt, "nbt": nbt, "tpc": (nbt + s - 1) // s}


def planes(x):
    """[n, D] bf16 or fp32 tensor -> (hi, lo) fp64 arrays: the bf16 planes launch_split_planes makes (lo None: bf16 input)."""
    if x.dtype == torch.bfloat16:
        return x.double().numpy(), None
    x = x.float()
    hi = x.bfloat16().float()
    return hi.double().numpy(), (x - hi).bfloat16().double().numpy()


def _unit(a):
    """largest power of two that divides every non-zero entry"""
    a = np.abs(a[a != 0])
    if a.size == 0:
        return np.inf
    m, e = np.frexp(a)
    mi = np.round(m * 2.0 ** 53).astype(np.int64)
    return float(2.0 ** (e - 53 + np.round(np.log2((mi & -mi).astype(np.float64)))).min())


def assert_exact(bank, q):
    """The maker's two conditions (module docstring) over every accumulation of the search: the MFMA sums of any subset of
    the plane products and the select pass's fp32 re-scoring of (hi + lo) rows against the fp32 query."""
    bh, bl = planes(bank)
    qh, ql = planes(q)
    assert np.array_equal(qh + ql, q.double().numpy()), "a query row is not the sum of its two planes"
    ub = min(_unit(bh), _unit(bl) if bl is not None else np.inf)
    uq = min(_unit(qh), _unit(ql))
    if not np.isfinite(ub * uq):
        return
    unit = ub * uq
    ba = np.abs(bh) + (np.abs(bl) if bl is not None else 0.0)
    qa = np.abs(qh) + np.abs(ql)
    worst = 0.0
    for j0 in range(0, qa.shape[0], 128):
        worst = max(worst, float((ba @ qa[j0:j0 + 128].T).max()))
    assert worst / unit < 2.0 ** 24, f"sum |b||q| = {worst / unit:.3g} units"
    bp, qp = [np.abs(bh)] + ([np.abs(bl)] if bl is not None else []), [np.abs(qh), np.abs(ql)]
    top = max(float((b.max(0) * p.max(0)).max()) for b in bp for p in qp)          # the plane products of the matrix pipe
    assert top / unit <= 2.0 ** 16, f"dynamic range 2^{np.log2(top / unit):.1f} inside one accumulation"


# ---------------------------------------------------------------------------------------------------------------
# the defects: name -> what a slipped index would do (each is one branch of `model` / `merge_model`)
# ---------------------------------------------------------------------------------------------------------------
BANK_DEFECTS = {
    # pass 0
    "sample_ignores_stride": "the sample reads rows 0 .. n_sample-1",
    "sample_clamped_row_in_two_groups": "skinny sample: the first row of the next group is counted in this one too",
    "rank_off_by_one": "tau from the (keff-1)-th group maximum",
    "slack_dropped": "tau = the k-th value itself: a tie at the k-th value is lost",
    "margin_lacks_bl_qh": "margin without |bank lo| |query hi|",
    "margin_lacks_bh_ql": "margin without |bank hi| |query lo|",
    "bounds_skip_last_row": "bank_bounds without row R-1",
    "bounds_hi_plane_only": "bank_bounds[1] = 0",
    # pass 1
    "ragged_last_row_dropped": "row R-1 of a ragged tile is masked",
    "rows_past_R_listed": "the ragged tile's rows past R are listed with their 0.0",
    "first_tile_of_chunk_only": "only the first 256 rows of a chunk are filtered",
    "chunk_first_row_dropped": "the first row of every chunk is skipped",
    "padded_lane_appends": "a padded query lane appends to (chunk + 1, q - M)",
    "cap_minus_one": "slot < BANK_CAP - 1",
    "cap_plus_one": "c > BANK_CAP + 1",
    "overflow_not_flagged": "a list past the cap sets no flag",
    "skinny_forgets_idx_offset": "the skinny stream lists row, not row + idx_offset",
    "k_block_dropped": "the filter product lacks the last 64 columns",
    # moments
    "moments_count_masked_rows": "the zeros of a ragged tile's rows past R are counted",
    "moments_wm_half_dropped": "the rows of the second wave row (tile rows 128 .. 255) are missing",
    "moments_last_chunk_missing": "the combine over chunks stops one short",
    "moments_max_from_survivors": "the maximum is taken over the stored candidates",
    # pass 2
    "rescore_ignores_lo": "the re-scoring reads the bank's hi plane only",
    "ties_by_list_slot": "equal similarities come out in list order",
    "pool_truncated_silently": "a pool past 6144 sets no flag",
    "wrong_slot_struck": "the slot after the winner's is struck: an index appears twice",
    "no_padding_beyond_candidates": "ranks beyond the candidates are 0 / 0.0, not -1 / -inf",
    "rescore_forgets_idx_offset": "the re-scoring reads row idx, not idx - idx_offset",
    # merge
    "merge_ties_by_shard": "equal similarities across shards come out in shard order",
    "merge_padding_first": "a padded entry of a shard's list sorts before a valid one",
    "merge_last_shard_moments_dropped": "the moments of the last shard are missing",
}


@dataclass
class Result:
    idx: np.ndarray            # [M, k] int32
    sim: np.ndarray            # [M, k] float32
    mom: np.ndarray = None     # [M, 4] float32 (forms with moments)
    overflow: int = 0          # 0 / non-zero, as tvc_bank_status reports it
    tau: np.ndarray = None     # [M] float32
    list_max: int = 0          # longest (chunk, query) list before the cap
    pool_max: int = 0          # largest pool before the cap
    decided: bool = True       # no similarity within `guard` of a tau that could change an output
    exact: bool = True         # every returned similarity is an fp32 number
    mom_exact: bool = True     # ... and every moment, with all partial sums


def _tau(gm_sorted, keff, margin, defect):
    """kth_finish in fp32 as written: (tau, guard)"""
    m = f32(gm_sorted[keff - 2 if defect == "rank_off_by_one" else keff - 1])
    if not m > NINF:
        return f32(NINF), 0.0
    if defect == "slack_dropped":
        v = f32(m - margin)
    else:
        v = f32(f32(f32(m - f32(1e-6)) - f32(f32(1e-6) * abs(m))) - margin)
    if not np.isfinite(v):
        return f32(NINF), 0.0
    return v, 2.0 ** -21 * max(abs(float(m)), float(margin))          # 4 ulp of the larger term


def model(bank, q, k, count_thr=0.3, form="filter", idx_offset=0, defect=None, qsel=None, acc_err=0.0):
    """The search of csrc/bank.hip in int64 / fp64, pass by pass, no tiles and no lanes.  ``qsel``: evaluate these queries only
    (the plan is the whole batch's; the other rows of the result stay -1 / -inf / 0)."""
    assert defect is None or defect in BANK_DEFECTS, defect
    filt, part, want_mom = FORMS[form]
    R, D = bank.shape
    M = q.shape[0]
    bh, bl = planes(bank)
    qh, ql = planes(q)
    P = plan(R, M, k)
    n, stride, S, rpc = P["n_sample"], P["stride"], P["S"], P["tpc"] * TILE
    keff = max(k, KEFF)
    pad = (-R) % TILE
    out = Result(np.full((M, k), -1, np.int32), np.full((M, k), NINF, f32), np.zeros((M, 4), f32) if want_mom else None)
    out.tau = np.full(M, NINF, f32)

    # ---- bank_bounds (filter forms): max row norms of the two planes, x 1.0001
    bnd = np.zeros(2, f32)
    if filt:
        rows = slice(0, R - 1) if defect == "bounds_skip_last_row" else slice(0, R)
        bnd[0] = f32(np.sqrt(f32((bh[rows] ** 2).sum(1).max(initial=0.0)))) * f32(1.0001)
        if bl is not None and defect != "bounds_hi_plane_only":
            bnd[1] = f32(np.sqrt(f32((bl[rows] ** 2).sum(1).max(initial=0.0)))) * f32(1.0001)

    # ---- pass 0: the sample's rows and their groups
    srows = np.arange(n, dtype=np.int64) * (1 if defect == "sample_ignores_stride" else stride)
    e = np.arange(n)
    if part == "skinny":
        per = (n + 255) // 256
        grp = e // per
        if defect == "sample_clamped_row_in_two_groups":
            twice = e[(e % per == 0) & (e > 0)]
            e, grp = np.concatenate([e, twice]), np.concatenate([grp, twice // per - 1])
    else:
        grp = (e >> 2) & 255 if n % 4 == 0 else e & 255
    order = np.argsort(grp, kind="stable")
    e_sorted, g_sorted = e[order], grp[order]
    starts = np.flatnonzero(np.r_[True, g_sorted[1:] != g_sorted[:-1]])

    bh_f = bh
    if defect == "k_block_dropped":
        bh_f = bh.copy()
        bh_f[:, D - 64:] = 0.0
    queries = list(range(M)) if qsel is None else list(qsel)
    for j0 in range(0, len(queries), 64):
        js = queries[j0:j0 + 64]
        Shh = qh[js] @ bh.T                                         # [queries, R]: a query's similarities are contiguous
        V = Shh + ql[js] @ bh.T if ql[js].any() else Shh           # the all-products value: hi.hi + hi.lo (+ lo.hi)
        X = V
        if bl is not None:
            Slh = qh[js] @ bl.T
            V = V + Slh
            X = V + ql[js] @ bl.T if defect != "rescore_ignores_lo" else V - Slh
        F = (Shh if bh_f is bh else qh[js] @ bh_f.T) if filt else V
        if not filt:
            X = V
        for c, j in enumerate(js):
            Vj, Fj, Xj = V[c], F[c], X[c]
            if form == "dense":
                _dense_row(out, j, Vj, k, count_thr, idx_offset)
                continue
            # ---- pass 0: group maxima -> tau
            gm = np.full(256, NINF)
            gm[g_sorted[starts]] = np.maximum.reduceat(Vj[srows][e_sorted], starts)
            margin = f32(0)
            if filt:
                nh, nl = f32(np.sqrt(f32((qh[j] ** 2).sum()))), f32(np.sqrt(f32((ql[j] ** 2).sum())))
                t1 = f32(0) if defect == "margin_lacks_bh_ql" else f32(bnd[0] * nl)
                t2 = f32(0) if defect == "margin_lacks_bl_qh" else f32(bnd[1] * nh)
                margin = f32(f32(f32(f32(t1 + t2) + f32(bnd[1] * nl)) * f32(1.001)) +
                             f32(f32(4e-6) * f32(f32(1) + f32(bnd[0] * nh))))
            tau, guard = _tau(np.sort(gm)[::-1], keff, margin, defect)
            out.tau[j] = tau
            guard += 2.0 * acc_err
            # ---- pass 1: the filter and the lists
            if defect == "rows_past_R_listed" and pad:
                Fj, Xj = np.r_[Fj, np.zeros(pad)], np.r_[Xj, np.zeros(pad)]
            near = np.flatnonzero(np.abs(Fj - float(tau)) <= guard) if np.isfinite(tau) else np.zeros(0, np.int64)
            if near.size and not _harmless(near, Fj, Xj, float(tau) - guard, rpc, S, k):
                out.decided = False
            rows = np.flatnonzero(Fj > float(tau))
            if defect == "ragged_last_row_dropped" and pad:
                rows = rows[rows != R - 1]
            if defect == "first_tile_of_chunk_only":
                rows = rows[rows % rpc < TILE]
            if defect == "chunk_first_row_dropped":
                rows = rows[rows % rpc != 0]
            chunk, val = rows // rpc, Fj[rows]
            if defect == "padded_lane_appends":
                mpad = (-M) % (16 if form.startswith("skinny") else TILE)
                if j < mpad and 0.0 > float(tau):                  # lane M + j: a zero query under query j's tau
                    extra = np.arange(0, (S - 1) * rpc)
                    rows, chunk, val = np.r_[rows, extra], np.r_[chunk, extra // rpc + 1], np.r_[val, np.zeros(extra.size)]
                    o = np.argsort(chunk, kind="stable")
                    rows, chunk, val = rows[o], chunk[o], val[o]
            cnt = np.bincount(chunk, minlength=S) if rows.size else np.zeros(S, np.int64)
            out.list_max = max(out.list_max, int(cnt.max(initial=0)))
            if (cnt > (CAP + 1 if defect == "cap_plus_one" else CAP)).any() and defect != "overflow_not_flagged":
                out.overflow |= 1
            first = np.searchsorted(chunk, chunk) if rows.size else rows
            keep = (np.arange(rows.size) - first) < (CAP - 1 if defect == "cap_minus_one" else CAP)
            rows, val = rows[keep], val[keep]
            # ---- moments (all-products form with moments)
            if want_mom:
                Vm = Vj
                if defect == "moments_count_masked_rows":
                    Vm = np.r_[Vj, np.zeros(pad)]
                elif defect == "moments_wm_half_dropped":
                    Vm = Vj[np.arange(R) % TILE < 128]
                elif defect == "moments_last_chunk_missing":
                    Vm = Vj[:(S - 1) * rpc]
                mx = val.max(initial=NINF) if defect == "moments_max_from_survivors" else Vm.max(initial=NINF)
                mom = np.array([Vm.sum(), (Vm * Vm).sum(), mx, (Vm >= float(f32(count_thr))).sum()])
                out.mom[j] = mom
                out.mom_exact &= _moments_exact(mom, out.mom[j], Vm)
            # ---- pass 2: pool, re-scoring, k rounds
            out.pool_max = max(out.pool_max, rows.size)
            if rows.size > POOL:
                if defect != "pool_truncated_silently":
                    out.overflow |= 2
                rows, val = rows[:POOL], val[:POOL]
            stored = rows + (0 if defect == "skinny_forgets_idx_offset" and form.startswith("skinny") else idx_offset)
            if filt:
                at = stored - (0 if defect == "rescore_forgets_idx_offset" else idx_offset)
                val = Xj[at % Xj.size]
            if defect == "wrong_slot_struck":
                alive, top = np.ones(rows.size, bool), []
                for _ in range(min(k, rows.size)):
                    cand = np.flatnonzero(alive)
                    if cand.size == 0:
                        break
                    w = cand[np.lexsort((stored[cand], -val[cand]))[0]]
                    top.append(w)
                    alive[(w + 1) % rows.size] = False
                top = np.array(top, np.int64)
            else:
                tie = -rows if defect == "ties_by_list_slot" else stored
                top = np.lexsort((tie, -val))[:k]
            if defect == "no_padding_beyond_candidates":
                out.idx[j], out.sim[j] = 0, 0.0
            out.idx[j, :top.size] = stored[top]
            out.sim[j, :top.size] = val[top]
            out.exact &= bool((out.sim[j, :top.size] == val[top]).all())
    return out


def _harmless(near, Fj, Xj, tau_lo, rpc, S, k):
    """Rows whose filter value is within the guard of tau may or may not be listed.  That changes no output if, with all of
    them listed, no list and no pool reaches its cap and each of them is below k certain survivors in the final order."""
    rows = np.flatnonzero(Fj > tau_lo)
    sure = np.setdiff1d(rows, near)
    if rows.size > POOL or np.bincount(rows // rpc, minlength=S).max() > CAP or sure.size < k:
        return False
    return bool(Xj[near].max() < np.sort(Xj[sure])[-k])


def _moments_exact(mom, mom32, v):
    """the four moments are fp32 numbers and so is every partial sum: sum |v| and sum v^2 below 2^24 units"""
    u = 1.0 if (v == np.round(v)).all() else _unit(v)
    return bool((mom == mom32).all()) and (not np.isfinite(u) or (np.abs(v).sum() < 2.0 ** 24 * u and (v * v).sum() < 2.0 ** 24 * u * u))


def _dense_row(out, j, Vj, k, count_thr, idx_offset):
    """row_topk_kernel: k rounds over the whole row in (v desc, idx asc), and the row's moments"""
    top = np.lexsort((np.arange(Vj.size), -Vj))[:k]
    top = top[Vj[top] > NINF]
    out.idx[j, :top.size] = top + idx_offset
    out.sim[j, :top.size] = Vj[top]
    mom = np.array([Vj.sum(), (Vj * Vj).sum(), Vj.max(initial=NINF), (Vj >= float(f32(count_thr))).sum()])
    out.mom[j] = mom
    out.mom_exact &= _moments_exact(mom, out.mom[j], Vj)
    out.exact &= bool((out.sim[j, :top.size] == Vj[top]).all())


def brute(bank, q, k, idx_offset=0, filt=True):
    """(idx, sim) by a stable sort of the similarity matrix, nothing of the search's structure."""
    bh, bl = planes(bank)
    qh, ql = planes(q)
    Sm = bh @ qh.T + bh @ ql.T
    if bl is not None:
        Sm = Sm + bl @ qh.T + (bl @ ql.T if filt else 0.0)
    order = np.argsort(-Sm.T, axis=1, kind="stable")[:, :k]
    idx = np.full((q.shape[0], k), -1, np.int32)
    sim = np.full((q.shape[0], k), NINF, f32)
    idx[:, :order.shape[1]] = order + idx_offset
    sim[:, :order.shape[1]] = np.take_along_axis(Sm.T, order, 1)
    return idx, sim


# ---------------------------------------------------------------------------------------------------------------
# merge of W shards' lists (topk_merge_kernel)
# ---------------------------------------------------------------------------------------------------------------
def merge_model(idx_parts, sim_parts, feat_parts, mom_parts, defect=None):
    """idx / sim [W, M, k], feat [W, M, kf, D], mom [W, M, 4] (numpy) -> (idx, sim, feat, mom)"""
    W, M, k = idx_parts.shape
    kf, D = feat_parts.shape[2:]
    idx, sim = np.zeros((M, k), np.int32), np.zeros((M, k), f32)
    feat, mom = np.zeros((M, kf, D), f32), np.zeros((M, 4), f32)
    for m in range(M):
        ids = idx_parts[:, m].reshape(-1).astype(np.int64)
        v = np.where(ids >= 0, sim_parts[:, m].reshape(-1).astype(np.float64), NINF)
        pos = np.arange(W * k)
        padded = ids < 0
        if defect == "merge_padding_first":
            padded = ~padded
        keys = (pos, ids, -v, padded) if defect != "merge_ties_by_shard" else (ids, pos, -v, padded)
        order = np.lexsort(keys)[:k]
        idx[m], sim[m] = ids[order], v[order]
        for r in range(kf):
            s = order[r]
            if ids[s] >= 0:
                feat[m, r] = feat_parts[s // k, m, min(s % k, kf - 1)]
        mp = mom_parts[:W - 1 if defect == "merge_last_shard_moments_dropped" else W, m].astype(np.float64)
        mom[m] = [mp[:, 0].sum(), mp[:, 1].sum(), mp[:, 2].max(initial=NINF), mp[:, 3].sum()]
    return idx, sim, feat, mom


def merge_probe():
    """(h): W * k = 256 (W = 2, k = 128), kf = 3 < k, M = 3.  Query 0: the two shards interleave, with similarities that tie
    across shards (the lower index wins wherever it sits); query 1: shard 0 holds 5 valid entries and 123 paddings, in the
    middle of which the merge must not stop; query 2: nothing valid at all.  Moments are small integers."""
    W, M, k, kf, D = 2, 3, 128, 3, 8
    idx = np.full((W, M, k), -1, np.int32)
    sim = np.full((W, M, k), NINF, f32)
    r = np.arange(k)
    idx[0, 0], idx[1, 0] = 1000 + 2 * r + (r % 2) * 3, 1000 + 2 * r + 1          # shard 0 holds some of the larger ids
    sim[0, 0] = sim[1, 0] = (500 - r // 2).astype(f32)                            # pairs of ties in and across the shards
    idx[0, 1, :5], sim[0, 1, :5] = [7, 9, 11, 13, 15], [9, 8, 7, 6, 5]
    sim[0, 1, 5:] = 99.0                                                          # a padded entry's similarity is never read
    idx[1, 1], sim[1, 1] = 2000 + r, (8 - r // 4).astype(f32)
    g = np.random.default_rng(5)
    feat = g.integers(-8, 8, (W, M, kf, D)).astype(f32)
    mom = g.integers(-50, 50, (W, M, 4)).astype(f32)
    return idx, sim, feat, mom


def check_merge(merge, defect_free=merge_model):
    """merge(idx_parts, sim_parts, feat_parts, mom_parts) -> (idx, sim, feat, mom), all numpy: list of what differs"""
    parts = merge_probe()
    want, got, fails = defect_free(*parts), merge(*parts), []
    for name, a, b in zip(("idx", "sim", "feat", "mom"), got, want):
        if not np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32)):
            fails.append(f"merge: {name} differs")
    return fails


# ---------------------------------------------------------------------------------------------------------------
# probes
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class Probe:
    name: str
    bank: torch.Tensor
    q: torch.Tensor
    k: int
    count_thr: float = 0.3
    idx_offset: int = 0
    mom_exact: bool = False            # the moments are exact too (compared bit for bit)
    overflow: bool = False             # the probe aims at a cap: the flag is the expected result
    planted: list = field(default_factory=list)      # (query, row) pairs the maker planted as winners
    acc_err: float = 0.0

    @property
    def shape(self):
        return self.bank.shape[0], self.q.shape[0], self.bank.shape[1], self.k

    def forms(self, moments_too=True):
        """the (form, search arguments) this probe is run in: the default form of its shape, all products without moments
        and (``moments_too``) all products with moments"""
        R, M, D, _ = self.shape
        bf = self.bank.dtype == torch.bfloat16
        runs = [(form_of(R, M, D, bf, False), dict(want_moments=False, allow_filter=True)),
                ("products", dict(want_moments=False, allow_filter=False))]
        if moments_too:
            runs.append(("moments", dict(want_moments=True, allow_filter=True)))
        return runs


_MODEL_CACHE = {}


def reference(p, form, qsel=None):
    """the defect-free model of a probe in a form, computed once"""
    key = (p.name, form, None if qsel is None else tuple(qsel))
    if key not in _MODEL_CACHE:
        _MODEL_CACHE[key] = model(p.bank, p.q, p.k, p.count_thr, form, p.idx_offset, None, qsel, p.acc_err)
    return _MODEL_CACHE[key]


def validate(p, form, qsel=None):
    """A probe is valid by the model alone: exact values, every list decided, and no cap reached unless it aims at one."""
    if p.acc_err == 0.0:
        assert_exact(p.bank, p.q)
    r = reference(p, form, qsel)
    assert r.exact, (p.name, form, "a value is not an fp32 number")
    assert r.decided, (p.name, form, "a similarity lies within the guard of tau")
    assert r.mom_exact or not (p.mom_exact and FORMS[form][2]), (p.name, form, "a moment is not exact")
    assert bool(r.overflow) == p.overflow, (p.name, form, r.list_max, r.pool_max)
    if not p.overflow:
        assert r.list_max <= CAP and r.pool_max <= POOL
    return r


def check_search(search, p, form, kwargs, switches=None, qsel=None):
    """search(bank, q, k, count_thr, idx_offset, want_moments, allow_filter) -> (idx, sim, mom | None, overflow) in numpy.
    Bit equality with the model: the flag always, idx and sim unless the model itself overflows (which 128 of 129 survive is
    the atomics' business), the moments where the probe makes them exact (they do not pass through the lists).  Returns the
    list of what differs."""
    if switches and form != "moments":
        R, M, D, _ = p.shape
        form = form if form == "products" else form_of(R, M, D, p.bank.dtype == torch.bfloat16, False, True, **switches)
    want = reference(p, form, qsel)
    idx, sim, mom, overflow = search(p.bank, p.q, p.k, p.count_thr, p.idx_offset, **kwargs,
                                     **({} if qsel is None else {"qsel": qsel}))
    sel = slice(None) if qsel is None else list(qsel)
    tag, fails = f"{p.name} [{form}]", []
    if bool(overflow) != bool(want.overflow):
        fails.append(f"{tag}: overflow flag {overflow}, model {want.overflow}")
    if not want.overflow:
        if not np.array_equal(idx[sel], want.idx[sel]):
            bad = np.flatnonzero((idx[sel] != want.idx[sel]).any(1))
            fails.append(f"{tag}: idx differs at {bad.size} queries, first {bad[0]}: {idx[sel][bad[0]][:8]} != {want.idx[sel][bad[0]][:8]}")
        if not np.array_equal(sim[sel].view(np.int32), want.sim[sel].view(np.int32)):
            fails.append(f"{tag}: sim bits differ")
    if kwargs.get("want_moments"):
        cols = [0, 1, 2, 3] if p.mom_exact else [2]          # the maximum is exact wherever the similarities are
        if mom is None or not np.array_equal(mom[sel][:, cols].view(np.int32), want.mom[sel][:, cols].view(np.int32)):
            fails.append(f"{tag}: moments differ (columns {cols})")
    return fails


def defective(defect, switches=None):
    """the model with a defect, in ``check_search``'s calling convention: the CPU suite's stand-in for a broken kernel"""
    def search(bank, q, k, count_thr, idx_offset, want_moments, allow_filter, qsel=None):
        R, D = bank.shape
        form = form_of(R, q.shape[0], D, bank.dtype == torch.bfloat16, want_moments, allow_filter, **(switches or {}))
        r = model(bank, q, k, count_thr, form, idx_offset, defect, qsel)
        return r.idx, r.sim, r.mom, r.overflow
    return search


# ---- code_bank: every similarity a known integer ------------------------------------------------------------------
H_TOP = 127 + 256 * 127      # a planted winner's similarity; the code's own rows stay below 126 + 256 * 126


def _code_query(j, D):
    """query j of the code: weight +-1 on column c1 and +-256 on c2, the ordered pair different for every j < D (D - 1)"""
    c1 = (37 * j) % D                                   # 37 is coprime to every D here: the pairs spread over all columns
    c2 = (c1 + 1 + (j // D) % (D - 1)) % D
    return c1, c2, (1 if (j >> 1) & 1 else -1), (1 if j % 3 else -1)


def code_bank(R, M, D, k, seed=0, fp32=False, plant=True, idx_offset=0, name=None):
    """Bank entries are integers in [-126, 126] (exact in bf16), query j has two non-zero weights, +-1 and +-256, on an
    ordered column pair of its own: sim(j, r) = +-a(r) +- 256 b(r), a 16-bit pseudo-random integer with another ranking for
    every query, the pairs spread over all D columns.  ``fp32``: the bank is fp32 with a non-zero lo plane -- hi an integer
    with 8 <= |hi| <= 15 (half an ulp of hi is 2^-5), lo = +-2^-6, the weights +-1 and +-16 -- so both planes are exact and
    a re-scoring that ignores lo returns other values.

    ``plant``: winners (the largest possible similarity, so ties among them are ordered by index) on top of the code, for
    the position read-back.  Per 64-query wave column (wn) of a query tile the tile-row positions 0 .. 255 are dealt to
    its queries in turn -- four per query, 64 apart, so both wave rows (wm) -- in tiles that are the first of a chunk,
    the last full tile of a chunk (the ring's last) or the ragged tile; the spare ranks take the rows a slipped bound
    would lose: row R-1, the first and last row of a chunk, rows past the sample's reach, the last full tile's last row."""
    g = np.random.default_rng(seed)
    w2, top = (16, 16) if fp32 else (256, 127)          # (16 + 2^-6 still rounds to 16 in bf16)
    if fp32:
        bank = g.integers(8, 16, (R, D)) * g.choice([-1, 1], (R, D))
        lo = g.choice([-1.0, 1.0], (R, D)) * 2.0 ** -6
    else:
        bank = g.integers(-126, 127, (R, D))
    q = np.zeros((M, D))
    for j in range(M):
        c1, c2, s1, s2 = _code_query(j, D)
        q[j, c1], q[j, c2] = s1, s2 * w2
    planted = []
    if plant:
        P = plan(R, M, k)
        S, tpc, n_full, rpc = P["S"], P["tpc"], R // TILE, P["tpc"] * TILE
        used, room = set(), [k] * M

        def put(j, row):
            if row in used or not 0 <= row < R or room[j] == 0:
                return False
            c1, c2, s1, s2 = _code_query(j, D)
            bank[row, c1], bank[row, c2] = s1 * top, s2 * top
            used.add(row)
            room[j] -= 1
            planted.append((j, row))
            return True

        extras = [R - 1, rpc - 1, min(rpc, R - 2), (S - 1) * rpc, n_full * TILE - 1, P["n_sample"] * P["stride"] + 1,
                  R - 1 - (R - 1) % 16, R - 1 - (R - 1) % 16 - 1, 7, min(15 * P["stride"] + 1, R - 3)]
        spare = [k - 4] * M
        for i, row in enumerate(extras):
            j = (2 * i) % M
            if spare[j] > 0 and put(j, row):
                spare[j] -= 1
        for qt in range(P["nqt"]):
            for wn in range(4):
                cls = list(range(qt * TILE + wn * 64, min(qt * TILE + wn * 64 + 64, M)))
                for i in range(TILE if cls else 0):
                    p, j = i // 4 + 64 * (i % 4), cls[(i // 4) % len(cls)]        # a query's four positions: 64 apart
                    for t in range(S):
                        ch = (7 * p + 3 * wn + 5 * qt + t) % S
                        kind = (p + t) % 3
                        tile = ch * tpc if kind == 0 else min(ch * tpc + tpc - 1, max(n_full - 1, 0)) if kind == 1 else R // TILE
                        if put(j, tile * TILE + p):
                            break
    bt = torch.from_numpy(bank.astype(np.float64))
    if fp32:
        bt = (bt + torch.from_numpy(lo)).float()
    else:
        bt = bt.to(torch.bfloat16)
    nm = name or f"code{'32' if fp32 else ''}({R},{M},{D},{k}{',+' + str(idx_offset) if idx_offset else ''})"
    return Probe(nm, bt, torch.from_numpy(q).float(), k, idx_offset=idx_offset, planted=planted)


def coverage(p, form):
    """What the planted winners that the model confirms (they are in their query's top-k) reach: the sets of
    (tile-row position, wn), (query position in its tile, wm), (row mod 16, query mod 64) and the named rows."""
    r = reference(p, form)
    R, M, _, k = p.shape
    P = plan(R, M, k)
    rpc = P["tpc"] * TILE
    ok = [(j, row) for j, row in p.planted if (row + p.idx_offset) in r.idx[j]]
    return {"confirmed": len(ok), "planted": len(p.planted),
            "row_x_wn": {(row % TILE, (j % TILE) // 64) for j, row in ok},
            "query_x_wm": {(j % TILE, (row % TILE) // 128) for j, row in ok},
            "row16_x_q64": {(row % 16, j % 64) for j, row in ok},
            "ragged_tile": sum(row >= R // TILE * TILE for _, row in ok), "last_row": any(row == R - 1 for _, row in ok),
            "chunk_first": sum(row % rpc == 0 for _, row in ok), "chunk_last": sum(row % rpc == rpc - 1 for _, row in ok),
            "second_tile_of_chunk": sum(row % rpc >= TILE for _, row in ok),
            "unsampled": sum(row % P["stride"] != 0 or row >= P["n_sample"] * P["stride"] for _, row in ok),
            "past_sample": sum(row >= P["n_sample"] * P["stride"] for _, row in ok)}


# ---- moment_bank ---------------------------------------------------------------------------------------------------
def moment_bank(R, M, D, k=5, count_thr=2.5, seed=0):
    """Small-range integer similarities with a thin upper tail: entries in [-2, 2] (one row in 50: [-30, 30]), weights +-1
    and +-3, so sum, sum of squares (< 2^24), max and count are exact in fp32 in any order.  3.0 is an attained value."""
    g = np.random.default_rng(seed)
    bank = g.integers(-2, 3, (R, D))
    tail = g.random(R) < 0.02
    bank[tail] = g.integers(-30, 31, (int(tail.sum()), D))
    q = np.zeros((M, D))
    for j in range(M):
        c1, c2, s1, s2 = _code_query(j, D)
        q[j, c1], q[j, c2] = s1, 3 * s2
    return Probe(f"moment({R},{M},{D},thr={count_thr})", torch.from_numpy(bank.astype(np.float64)).to(torch.bfloat16),
                 torch.from_numpy(q).float(), k, count_thr=count_thr, mom_exact=True)


# ---- the tight probes --------------------------------------------------------------------------------------------
def _pair_queries(M, D, w2=256):
    q = np.zeros((M, D))
    for j in range(M):
        q[j, 2 * j], q[j, 2 * j + 1] = 1, w2
    return q


def _groups(n, e):
    return ((e >> 2) & 255 if n % 4 == 0 else e & 255), e // ((n + 255) // 256)


def _distinct(n, count, first=0, every=1):
    """``count`` elements >= ``first`` of an n-element sample, each in another group of BOTH partitions (dense: (e >> 2) & 255
    or e & 255, skinny: e // ceil(n / 256)) -- the first element of its skinny group wherever the dense partition allows,
    in every ``every``-th skinny group (2: the group before a winner's holds none, so a row counted there too is one more)"""
    per = (n + 255) // 256
    dense = (lambda e: (e >> 2) & 255) if n % 4 == 0 else (lambda e: e & 255)
    seen, out = set(), []
    for G in range((first + per - 1) // per, 256, every):
        for e in range(G * per, min((G + 1) * per, n)):
            if dense(e) not in seen:
                seen.add(dense(e))
                out.append(e)
                break
        if len(out) == count:
            return out
    raise AssertionError("the sample has too few groups")


def tight_tau(k, D, M=3, fp32=False, count_thr=0.3):
    """(a): R = 4096 is sampled whole, keff = k >= 16, the top-k of every query sit in k distinct groups of both partitions,
    so tau is the k-th value less kth_finish's slack -- and the (k+1)-th value ties with the k-th (the row beside it, in the
    same groups).  A rank off by one, a dropped slack or a row counted in two groups loses rank k."""
    assert k >= KEFF and M <= D // 2
    g = np.random.default_rng(k)
    bank = g.integers(-126, 127, (4096, D))
    win = _distinct(4096, k, every=2)
    last = win[k - 1]
    tie = last + 1 if _groups(4096, last + 1) == _groups(4096, last) else last - 1          # the tie row: in the k-th's groups
    assert _groups(4096, tie) == _groups(4096, last) and tie not in win
    for j in range(M):
        bank[win, 2 * j], bank[win, 2 * j + 1] = 127, 127
        bank[[last, tie], 2 * j] = 126
        bank[tie, 2 * j + 1] = 127
    bt = torch.from_numpy(bank.astype(np.float64))
    return Probe(f"tight_tau(k={k},D={D},{'f32' if fp32 else 'bf16'})", bt.float() if fp32 else bt.to(torch.bfloat16),
                 torch.from_numpy(_pair_queries(M, D)).float(), k, count_thr=count_thr)


def stride_probe(D, M=2, k=20):
    """R = 70 001 is sampled with stride 12.  Each query's 20 winners sit on sampled rows past row n_sample, in 20 groups, so
    tau is their value less the slack; 200 rows three below them wait in ONE chunk.  A sample that reads rows 0 .. n_sample-1
    finds none of the winners, lowers tau and overflows that chunk's list."""
    R = 70001
    P = plan(R, M, k)
    g = np.random.default_rng(12)
    bank = g.integers(-126, 127, (R, D))
    win = P["stride"] * np.array(_distinct(P["n_sample"], k, first=2048))
    for j in range(M):
        bank[win, 2 * j], bank[win, 2 * j + 1] = 127, 127
        rows = 200 * P["tpc"] * TILE + 1 + np.arange(200)
        bank[rows, 2 * j], bank[rows, 2 * j + 1] = 124, 127          # 3 below: the filter forms' margin is ~1 on this data
    assert P["stride"] * 2048 >= P["n_sample"] and P["stride"] > 1
    return Probe(f"stride(D={D})", torch.from_numpy(bank.astype(np.float64)).to(torch.bfloat16),
                 torch.from_numpy(_pair_queries(M, D)).float(), k)


def margin_probe(term, D, R=4099, pos=None):
    """(b) ``term`` = "bl_qh": an fp32 bank; the winner is 16 + 3/64 on the 16 columns the query weighs 1 (hi 16, lo 3/4 of
    half an ulp), so its one-product value 256 understates its similarity 256.75 by nearly |lo| |q hi| = 0.75; the 16 rows
    that set tau (256.5: fifteen 16s and a 16.5, exact in bf16, in 16 groups) lie between.  With the margin's bl * qh term
    the filter threshold is 255.75, without it 256.50 and the winner is never listed.
    (c) ``term`` = "bh_ql": the mirror -- a bf16 bank and a query of 1 + 3/1024 (lo 3/4 of half an ulp) on 16 columns.
    (d) ``pos``: the winner's row; it alone decides bank_bounds[1] in (b), so R-1 and a row past 16 384 (the second trip of
    bank_bounds_kernel's grid-stride loop) probe that kernel's row range.  In (c) every near-winner has nearly the largest
    norm, so the row that decides bank_bounds[0] cannot decide the result (module docstring)."""
    g = np.random.default_rng(R)
    k, M = 5, 2
    P = plan(R, M, k)
    pos = R - 1 if pos is None else pos
    h = g.integers(-32, 25, (R, D)) * 0.5                       # filler: one-product values <= 16 * 12
    h[:, 16:] = 0.0
    lo = np.zeros((R, D))
    tau_rows = [P["stride"] * e for e in _distinct(P["n_sample"], KEFF)]
    assert pos not in tau_rows
    q = np.zeros((M, D))
    if term == "bl_qh":
        h[tau_rows, :16] = 16.0
        h[tau_rows, 3] = 16.5
        h[pos, :16], lo[pos, :16] = 16.0, 3.0 / 64
        q[0, :16] = 1.0
        bank = torch.from_numpy(h + lo).float()
    else:
        h[tau_rows, :16] = 16.0
        h[tau_rows, 3] = 15.75
        h[pos, :16] = 16.0
        q[0, :16] = 1.0 + 3.0 / 1024
        bank = torch.from_numpy(h).to(torch.bfloat16)
    q[1, :16] = -q[0, :16]                                      # and a query that sees the same rows upside down
    return Probe(f"margin_{term}(R={R},D={D},row={pos})", bank, torch.from_numpy(q).float(), k)


def negative_probe(R, M, D, fp32=False):
    """(e): every bank entry is positive, every query weight negative: all similarities are below zero, so the 0.0 of a ragged
    tile's rows past R, or of a padded query lane, would beat every real row; count_thr = -1 counts such zeros."""
    g = np.random.default_rng(R + M)
    bank = g.integers(1, 127, (R, D))
    q = np.zeros((M, D))
    for j in range(M):
        c1, c2, _, _ = _code_query(j, D)
        q[j, c1], q[j, c2] = -1, -256
    bt = torch.from_numpy(bank.astype(np.float64))
    return Probe(f"negative({R},{M},{D},{'f32' if fp32 else 'bf16'})", bt.float() if fp32 else bt.to(torch.bfloat16),
                 torch.from_numpy(q).float(), 5, count_thr=-1.0)


def cap_probe(n, D, R=4097):
    """(f): one query, k = 128, ``n`` rows of the second-largest value in chunk 0 (one chunk = one tile at this R) and 112 more
    in the later chunks, placed so that 128 groups of the whole sample hold one: tau is their value less the slack and
    chunk 0's list holds exactly ``n`` survivors.  n = 128: no overflow, and the 128 lowest indices -- chunk 0's list, whole
    -- are the answer.  n = 129: the flag.  The one row of the largest value is chunk 0's last survivor, so a maximum taken
    from the stored candidates misses it when the list is cut."""
    g = np.random.default_rng(n)
    bank = g.integers(-126, 127, (R, D))
    grp_rows = _distinct(4096, 128)
    rows0 = [r for r in grp_rows if r < TILE]
    rows0 += [r for r in range(TILE) if r not in grp_rows][:n - len(rows0)]
    for r in grp_rows + rows0:
        bank[r, 0], bank[r, 1] = 126, 127
    bank[max(rows0), 0] = 127
    return Probe(f"cap({n},D={D})", torch.from_numpy(bank.astype(np.float64)).to(torch.bfloat16),
                 torch.from_numpy(_pair_queries(1, D)).float(), 128, overflow=n > CAP)


def pool_probe(n, D):
    """(g): one query over R = 70 001 (274 chunks of 256 rows), k = 20: ``n`` rows of the top value, at most 128 per chunk, 24
    of them on sampled rows in 24 groups.  All tie, all survive: the pool holds exactly ``n``.  6144 fits, 6145 flags."""
    R, k = 70001, 20
    P = plan(R, 1, k)
    g = np.random.default_rng(n)
    bank = g.integers(-126, 127, (R, D))
    rows = {P["stride"] * e for e in _distinct(P["n_sample"], 24)}
    c = 40
    while len(rows) < n:
        have = sum(1 for r in rows if r // TILE == c)
        for r in range(c * TILE, (c + 1) * TILE):
            if have >= 120 or len(rows) >= n:
                break
            if r not in rows:
                rows.add(r)
                have += 1
        c += 1
    rows = sorted(rows)
    bank[rows, 0], bank[rows, 1] = 127, 127
    assert P["tpc"] == 1
    return Probe(f"pool({n},D={D})", torch.from_numpy(bank.astype(np.float64)).to(torch.bfloat16),
                 torch.from_numpy(_pair_queries(1, D)).float(), k, overflow=n > POOL)


def small_bank(D, M=3):
    """R = 100 < k = 128: tau is -inf (fewer than keff non-empty groups), every row is listed, ranks 100 .. 127 are -1 / -inf."""
    p = code_bank(100, M, D, 128, seed=3, plant=False, name=f"small(100,{M},{D},128)")
    return p


# ---------------------------------------------------------------------------------------------------------------
# the catalogue: every probe the CPU and the GPU suite run, by name.  Makers are deterministic, so two processes that build
# the same name hold the same bits.
# ---------------------------------------------------------------------------------------------------------------
OFFSET = 1_000_003
SKINNY_M = (1, 16, 17, 33, 49, 64)          # every NQT of the skinny filter (1 .. 4) and of the skinny sample (1, 2, 3, 2 x 2)

POSITION = {
    "code(255,70,64,7)": lambda: code_bank(255, 70, 64, 7),                        # one-tile filter
    "code(4097,257,64,5)": lambda: code_bank(4097, 257, 64, 5),                    # 17 chunks, ragged tile, ragged query tile
    "code(4097,257,64,32)": lambda: code_bank(4097, 257, 64, 32),
    **{f"code(4097,{M},128,7)": (lambda M=M: code_bank(4097, M, 128, 7)) for M in SKINNY_M},
    "code(4097,33,512,7)": lambda: code_bank(4097, 33, 512, 7),                    # the KB variants
    "code(4097,33,768,7)": lambda: code_bank(4097, 33, 768, 7),
    "code(70001,64,128,20)": lambda: code_bank(70001, 64, 128, 20),                # stride 12, winners in unsampled rows
    "code(90001,770,64,5)": lambda: code_bank(90001, 770, 64, 5),                  # two tiles per chunk, blocked item order
    "code(4097,257,64,5,+1000003)": lambda: code_bank(4097, 257, 64, 5, idx_offset=OFFSET),
    "code(4097,257,64,32,+1000003)": lambda: code_bank(4097, 257, 64, 32, idx_offset=OFFSET),
    **{f"code(4097,{M},128,7,+1000003)": (lambda M=M: code_bank(4097, M, 128, 7, idx_offset=OFFSET)) for M in SKINNY_M},
    "code32(4097,257,64,5)": lambda: code_bank(4097, 257, 64, 5, fp32=True),       # fp32 banks: a non-zero lo plane
    "code32(4097,33,128,7)": lambda: code_bank(4097, 33, 128, 7, fp32=True),
    "code32(255,70,64,7)": lambda: code_bank(255, 70, 64, 7, fp32=True),
}
MOMENTS = {f"moment({R},{M},{D},thr={t})": (lambda R=R, M=M, D=D, t=t: moment_bank(R, M, D, count_thr=t))
           for R, M, D in ((4097, 257, 64), (90001, 770, 64), (4097, 33, 128)) for t in (2.5, 3.0, -1.0)
           if R < 90000 or t == 3.0}
TIGHT = {
    # (a) through the dense sample (D = 64; an fp32 bank at D = 128) and through the skinny sample (bf16, D = 128)
    **{f"tight_tau(k={k},D={D},{'f32' if f else 'bf16'})": (lambda k=k, D=D, f=f: tight_tau(k, D, fp32=f))
       for k in (16, 17, 128) for D, f in ((64, False), (128, False), (128, True))},
    "stride(D=64)": lambda: stride_probe(64),
    "stride(D=128)": lambda: stride_probe(128),
    # (b), (c) and their repeats (d) with the deciding row at R-1 and past row 16 384
    **{f"margin_{t}(R={R},D={D},row={pos})": (lambda t=t, D=D, R=R, pos=pos: margin_probe(t, D, R, pos))
       for t in ("bl_qh", "bh_ql") for D in (64, 128) for R, pos in ((4099, 4098), (20001, 20000), (20001, 16421))},
    # (e)
    "negative(1000,5,128,bf16)": lambda: negative_probe(1000, 5, 128),
    "negative(1000,70,64,bf16)": lambda: negative_probe(1000, 70, 64),
    "negative(255,70,64,bf16)": lambda: negative_probe(255, 70, 64),
    "negative(1000,5,128,f32)": lambda: negative_probe(1000, 5, 128, fp32=True),
    # (f)
    **{f"cap({n},D={D})": (lambda n=n, D=D: cap_probe(n, D)) for n in (128, 129) for D in (64, 128)},
    "small(100,3,64,128)": lambda: small_bank(64),
    "small(100,3,128,128)": lambda: small_bank(128),
}
POOLS = {f"pool({n},D={D})": (lambda n=n, D=D: pool_probe(n, D)) for n in (6144, 6145) for D in (64, 128)}      # (g)
CATALOG = {**POSITION, **MOMENTS, **TIGHT, **POOLS}
_PROBES = {}


def probe(name):
    if name not in _PROBES:
        _PROBES[name] = CATALOG[name]()
        assert _PROBES[name].name == name, (_PROBES[name].name, name)
    return _PROBES[name]


def cpu_sized(name):
    R, M = (int(x) for x in name[name.index("(") + 1:].split(",")[:2]) if name.startswith(("code", "moment")) else (0, 0)
    return R * M <= 4097 * 257
