// C-ABI of the detection-evaluation kernels (roc.hip): tvc_roc_weights / tvc_roc_sweep / tvc_roc_curve.  Its own translation
// unit: nothing here is called from another unit.  The calls read no bank and no tower; they need only a handle for the
// workspace of the global storage form.
#include "handle.hpp"

static_assert(TVC_ROC_MAX_THR == ROC_MAX_THR, "include/tvc.h and host_plan.hpp disagree on the number of thresholds");
static_assert(TVC_ROC_LDS_ROWS == ROC_LDS_ROWS, "include/tvc.h and host_plan.hpp disagree on the LDS form's sample count");
static_assert(TVC_ROC_MAX_N == ROC_MAX_N, "include/tvc.h and host_plan.hpp disagree on the sample cap");
static_assert(TVC_ROC_SRC_WEIGHTS == ROC_SRC_WEIGHTS && TVC_ROC_SRC_INDICES == ROC_SRC_INDICES && TVC_ROC_SRC_PHILOX == ROC_SRC_PHILOX,
              "include/tvc.h and kernels.hpp disagree on the sources");

// the checks every call shares and the plan of its rows, or the refusal; fills what the three launches have in common
static int roc_rows(tvc_handle* h, const char* fn, const tvc_roc_rows* r, int n_thr, double target, RocPlan* plan, RocLaunch* L) {
    const std::string f(fn);
    if (!r) return fail(h, TVC_E_INVALID, f + ": rows must not be NULL");
    *plan = roc_plan(r->N, r->B, n_thr, target);
    if (!plan->ok)
        return fail(h, TVC_E_INVALID, f + ": need 1 <= N <= TVC_ROC_MAX_N, B >= 1, at most TVC_ROC_MAX_THR thresholds and a target in [0, 1]");
    if (r->source != TVC_ROC_SRC_WEIGHTS && r->source != TVC_ROC_SRC_INDICES && r->source != TVC_ROC_SRC_PHILOX)
        return fail(h, TVC_E_INVALID, f + ": unknown source");
    if (r->first < 0 || r->first > 0xffffffffLL || r->first + r->B > 0x100000000LL) return fail(h, TVC_E_INVALID, f + ": need 0 <= first and first + B <= 2^32");
    if (!r->scores_dev || !r->labels_dev || !r->order_dev) return fail(h, TVC_E_INVALID, f + ": scores, labels and order must not be NULL");
    if (r->source == TVC_ROC_SRC_INDICES && !r->src_dev) return fail(h, TVC_E_INVALID, f + ": the INDICES source needs src");
    L->source = r->source; L->N = r->N; L->first = r->first; L->seed = r->seed;
    L->scores = r->scores_dev; L->labels = r->labels_dev; L->order = r->order_dev; L->src = r->src_dev;
    L->target = target; L->n_thr = n_thr;
    return TVC_OK;
}

// the rows of the call in the plan's chunks; the workspace is sized before the first launch
static int roc_run(tvc_handle* h, const tvc_roc_rows* r, const RocPlan& plan, RocLaunch& L, hipStream_t st) {
    int rc;
    if (!plan.lds && (rc = ensure(h, WS_ROC_COUNTS, (size_t)plan.ws_bytes))) return rc;
    L.ws = plan.lds ? nullptr : (uint32_t*)h->ws[WS_ROC_COUNTS].p;
    L.lds_bytes = plan.lds_bytes;
    for (int64_t c = 0; c < plan.n_chunks; ++c) {
        L.row0 = c * plan.chunk_rows;
        L.B = r->B - L.row0 < plan.chunk_rows ? r->B - L.row0 : plan.chunk_rows;
        HIP_TRY(launch_roc(L, st));
    }
    return TVC_OK;
}

int tvc_roc_weights(tvc_handle* h, const tvc_roc_rows* rows, int32_t* w_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    RocPlan plan;
    RocLaunch L;
    int rc;
    if ((rc = roc_rows(h, "tvc_roc_weights", rows, 0, 0.0, &plan, &L))) return rc;
    if (!w_dev) return fail(h, TVC_E_INVALID, "tvc_roc_weights: w must not be NULL");
    L.mode = ROC_MODE_WEIGHTS;
    L.w_out = w_dev;
    return roc_run(h, rows, plan, L, (hipStream_t)stream);
}

int tvc_roc_sweep(tvc_handle* h, const tvc_roc_rows* rows, double target_tpr, const float* thresholds, int32_t n_thr,
                  const tvc_roc_out* out, void* stream) {
    if (!h) return TVC_E_INVALID;
    RocPlan plan;
    RocLaunch L;
    int rc;
    if ((rc = roc_rows(h, "tvc_roc_sweep", rows, n_thr, target_tpr, &plan, &L))) return rc;
    if (n_thr > 0 && !thresholds) return fail(h, TVC_E_INVALID, "tvc_roc_sweep: thresholds must not be NULL when n_thr > 0");
    if (!out || !out->n_pos || !out->n_neg || !out->valid || !out->n_points || !out->n_kept || !out->auc2 || !out->auc || !out->ap ||
        !out->youden_j || !out->youden_pos || !out->youden_tp || !out->youden_fp || !out->target_pos || !out->target_tp ||
        !out->target_fp || (n_thr > 0 && (!out->thr_tp || !out->thr_fp)))
        return fail(h, TVC_E_INVALID, "tvc_roc_sweep: every output array must not be NULL (thr_tp and thr_fp when n_thr > 0)");
    L.mode = ROC_MODE_SWEEP;
    for (int t = 0; t < n_thr; ++t) L.thr[t] = thresholds[t];
    L.n_pos = out->n_pos; L.n_neg = out->n_neg; L.valid = out->valid; L.n_points = out->n_points; L.n_kept = out->n_kept;
    L.auc2 = out->auc2; L.auc = out->auc; L.ap = out->ap; L.youden_j = out->youden_j;
    L.youden_pos = out->youden_pos; L.youden_tp = out->youden_tp; L.youden_fp = out->youden_fp;
    L.target_pos = out->target_pos; L.target_tp = out->target_tp; L.target_fp = out->target_fp;
    L.thr_tp = out->thr_tp; L.thr_fp = out->thr_fp;
    return roc_run(h, rows, plan, L, (hipStream_t)stream);
}

int tvc_roc_curve(tvc_handle* h, const tvc_roc_rows* rows, int32_t* pt_tp_dev, int32_t* pt_fp_dev, int32_t* pt_pos_dev,
                  int32_t* pt_kept_dev, int32_t* count_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    RocPlan plan;
    RocLaunch L;
    int rc;
    if ((rc = roc_rows(h, "tvc_roc_curve", rows, 0, 0.0, &plan, &L))) return rc;
    if (rows->B != 1) return fail(h, TVC_E_INVALID, "tvc_roc_curve: need B == 1");
    if (!pt_tp_dev || !pt_fp_dev || !pt_pos_dev || !pt_kept_dev || !count_dev)
        return fail(h, TVC_E_INVALID, "tvc_roc_curve: pt_tp, pt_fp, pt_pos, pt_kept and count must not be NULL");
    L.mode = ROC_MODE_CURVE;
    L.pt_tp = pt_tp_dev; L.pt_fp = pt_fp_dev; L.pt_pos = pt_pos_dev; L.pt_kept = pt_kept_dev; L.pt_count = count_dev;
    return roc_run(h, rows, plan, L, (hipStream_t)stream);
}
