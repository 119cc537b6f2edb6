// C-ABI of the retrieval-evaluation kernels (rank.hip): tvc_rank_targets / tvc_rank_count / tvc_rank_metrics over the selected
// bank slot.  Its own translation unit: nothing here is called from another unit.
#include "handle.hpp"

static_assert(TVC_RANK_MAX_K == RANK_MAX_K, "include/tvc.h and host_plan.hpp disagree on the number of k values");

// the slot the call addresses and the plan of M queries over it, or the refusal
static int rank_slot(tvc_handle* h, const char* fn, int32_t M, int64_t T, BankSlot** out, RankPlan* plan) {
    int rc;
    if ((rc = filled_slot(h, fn, out))) return rc;
    *plan = rank_plan(M, (*out)->R, (*out)->D, bank_products((*out)->planes));
    if (!plan->ok) return fail(h, TVC_E_INVALID, std::string(fn) + ": need M >= 1");
    if (T < 0) return fail(h, TVC_E_INVALID, std::string(fn) + ": need T >= 0");
    return TVC_OK;
}

// the query planes and the padded per-query vectors of one tile pass
static int rank_tile_setup(tvc_handle* h, const BankSlot& bk, const RankPlan& plan, const float* rows_dev, int32_t M, bool count,
                           RankTileLaunch* L, hipStream_t st) {
    int rc;
    if ((rc = ensure_planes(h, WS_RK_QPLANES, M, 1, bk.D))) return rc;
    if ((rc = ensure(h, WS_RK_QLAB, (size_t)plan.mpad * 4))) return rc;
    if (count && (rc = ensure(h, WS_RK_TLOW, (size_t)plan.mpad * 4))) return rc;
    if ((rc = split_planes(h, WS_RK_QPLANES, rows_dev, M, bk.D, st, &L->qplanes))) return rc;
    L->bank = bank_rows(bk);
    L->M = M;
    L->qlab = (int32_t*)h->ws[WS_RK_QLAB].p;
    L->tlow = count ? (float*)h->ws[WS_RK_TLOW].p : nullptr;
    return TVC_OK;
}

int tvc_rank_targets(tvc_handle* h, const float* rows_dev, int32_t M, const int32_t* qlabel_dev, const int32_t* glabel_dev,
                     const int32_t* gpos_dev, const int64_t* tgt_off_dev, int64_t T, float* tgt_sim_dev, int32_t* tgt_row_dev,
                     void* stream) {
    if (!h) return TVC_E_INVALID;
    BankSlot* bk;
    RankPlan plan;
    int rc;
    if ((rc = rank_slot(h, "tvc_rank_targets", M, T, &bk, &plan))) return rc;
    if (!rows_dev || !qlabel_dev || !glabel_dev || !gpos_dev || !tgt_off_dev)
        return fail(h, TVC_E_INVALID, "tvc_rank_targets: rows, qlabel, glabel, gpos and tgt_off must not be NULL");
    if (T == 0) return TVC_OK;
    if (!tgt_sim_dev || !tgt_row_dev) return fail(h, TVC_E_INVALID, "tvc_rank_targets: tgt_sim and tgt_row must not be NULL when T > 0");
    hipStream_t st = (hipStream_t)stream;
    RankTileLaunch L;
    if ((rc = rank_tile_setup(h, *bk, plan, rows_dev, M, false, &L, st))) return rc;
    L.qlabel = qlabel_dev; L.glabel = glabel_dev; L.gpos = gpos_dev; L.tgt_off = tgt_off_dev;
    L.tgt_sim = tgt_sim_dev; L.tgt_row = tgt_row_dev;
    ProfScope ps(h, st, TVC_PROF_BANK, plan.flops);
    HIP_TRY(launch_rank_targets(L, st));
    return TVC_OK;
}

int tvc_rank_count(tvc_handle* h, const float* rows_dev, int32_t M, const int32_t* qlabel_dev, const int32_t* glabel_dev,
                   const int64_t* tgt_off_dev, const float* tgt_sim_dev, const int32_t* tgt_row_dev, int64_t T, int32_t* hist_dev,
                   void* stream) {
    if (!h) return TVC_E_INVALID;
    BankSlot* bk;
    RankPlan plan;
    int rc;
    if ((rc = rank_slot(h, "tvc_rank_count", M, T, &bk, &plan))) return rc;
    if (!rows_dev || !qlabel_dev || !glabel_dev || !tgt_off_dev)
        return fail(h, TVC_E_INVALID, "tvc_rank_count: rows, qlabel, glabel and tgt_off must not be NULL");
    if (T == 0) return TVC_OK;
    if (!tgt_sim_dev || !tgt_row_dev || !hist_dev)
        return fail(h, TVC_E_INVALID, "tvc_rank_count: tgt_sim, tgt_row and hist must not be NULL when T > 0");
    hipStream_t st = (hipStream_t)stream;
    RankTileLaunch L;
    if ((rc = rank_tile_setup(h, *bk, plan, rows_dev, M, true, &L, st))) return rc;
    L.qlabel = qlabel_dev; L.glabel = glabel_dev; L.tgt_off = tgt_off_dev;
    L.tgt_sim = const_cast<float*>(tgt_sim_dev); L.tgt_row = const_cast<int32_t*>(tgt_row_dev); L.hist = hist_dev;
    ProfScope ps(h, st, TVC_PROF_BANK, plan.flops);
    HIP_TRY(launch_rank_count(L, st));
    return TVC_OK;
}

int tvc_rank_metrics(tvc_handle* h, int32_t M, const int64_t* tgt_off_dev, const int32_t* hist_dev, int64_t T,
                     const int32_t* k_values, int32_t n_k, int32_t* pos_dev, double* ap_dev, double* rr_dev, int32_t* hits_dev,
                     double* dcg_dev, double* idcg_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    BankSlot* bk;
    RankPlan plan;
    int rc;
    if ((rc = rank_slot(h, "tvc_rank_metrics", M, T, &bk, &plan))) return rc;
    if (!rank_k_values_ok(k_values, n_k))
        return fail(h, TVC_E_INVALID, "tvc_rank_metrics: need at most TVC_RANK_MAX_K values of k, each >= 1");
    if (!tgt_off_dev || !ap_dev || !rr_dev || (n_k > 0 && (!hits_dev || !dcg_dev || !idcg_dev)))
        return fail(h, TVC_E_INVALID, "tvc_rank_metrics: tgt_off, ap, rr and (with k values) hits, dcg and idcg must not be NULL");
    if (T > 0 && (!hist_dev || !pos_dev)) return fail(h, TVC_E_INVALID, "tvc_rank_metrics: hist and pos must not be NULL when T > 0");
    RankMetricsLaunch L;
    L.M = M; L.n_k = n_k;
    for (int t = 0; t < n_k; ++t) L.k[t] = k_values[t];
    L.tgt_off = tgt_off_dev; L.hist = hist_dev; L.pos = pos_dev; L.ap = ap_dev; L.rr = rr_dev;
    L.hits = hits_dev; L.dcg = dcg_dev; L.idcg = idcg_dev;
    HIP_TRY(launch_rank_metrics(L, (hipStream_t)stream));
    return TVC_OK;
}
