// C-ABI of the similarity-metric kernels (sim.hip): tvc_sim_rows, tvc_sim_flat_workspace / tvc_sim_flat_rank / tvc_sim_flat and
// tvc_topk_overlap.  Its own translation unit: nothing here is called from another unit.  The calls read no bank and no tower
// and keep nothing in the handle: the long form's workspace is the caller's.
#include "handle.hpp"

static_assert(TVC_SIM_MAX_D == SIM_MAX_D && TVC_SIM_MAX_N == SIM_MAX_N, "include/tvc.h and host_plan.hpp disagree on the size caps");
static_assert(TVC_SIM_COLS == SIM_COLS && TVC_SIM_INTS == SIM_INTS, "include/tvc.h and host_plan.hpp disagree on the output widths");
static_assert(TVC_SIM_KEY_F32 == SIM_KEY_F32 && TVC_SIM_KEY_I32 == SIM_KEY_I32, "include/tvc.h and kernels.hpp disagree on the key types");
static_assert(TVC_TOPK_OVERLAP_MAX_K == TOPK_OVERLAP_MAX_K, "include/tvc.h and host_plan.hpp disagree on the overlap's k");

int tvc_sim_rows(tvc_handle* h, const void* x_dev, const void* y_dev, int64_t B, int32_t D, int64_t ldx, int64_t ldy, int32_t key_type,
                 double* out_dev, int64_t* ints_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (B < 0 || B > 0x7fffffffLL) return fail(h, TVC_E_INVALID, "tvc_sim_rows: need 0 <= B < 2^31");
    if (D < 1 || D > TVC_SIM_MAX_D) return fail(h, TVC_E_INVALID, "tvc_sim_rows: need 1 <= D <= TVC_SIM_MAX_D");
    if (ldx < D || ldy < D) return fail(h, TVC_E_INVALID, "tvc_sim_rows: a row pitch is below D");
    if (key_type != TVC_SIM_KEY_F32 && key_type != TVC_SIM_KEY_I32) return fail(h, TVC_E_INVALID, "tvc_sim_rows: unknown key type");
    if (B == 0) return TVC_OK;
    if (!x_dev || !y_dev || !out_dev || !ints_dev) return fail(h, TVC_E_INVALID, "tvc_sim_rows: x, y, out and ints must not be NULL when B > 0");
    SimRowsLaunch L;
    L.x = x_dev; L.y = y_dev; L.ldx = ldx; L.ldy = ldy; L.B = B; L.D = D; L.key = key_type; L.out = out_dev; L.ints = ints_dev;
    HIP_TRY(launch_sim_rows(L, (hipStream_t)stream));
    return TVC_OK;
}

uint64_t tvc_sim_flat_workspace(int64_t n) {
    const SimFlatPlan plan = sim_flat_plan(n);
    return plan.ok ? (uint64_t)plan.ws_bytes : 0;
}

int tvc_sim_flat_rank(tvc_handle* h, const float* v_dev, const float* sorted_dev, int64_t n, int32_t* crank_dev, int64_t* nan_count_dev,
                      void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!sim_flat_plan(n).ok) return fail(h, TVC_E_INVALID, "tvc_sim_flat_rank: need 1 <= n <= TVC_SIM_MAX_N");
    if (!v_dev || !sorted_dev || !crank_dev) return fail(h, TVC_E_INVALID, "tvc_sim_flat_rank: v, sorted and crank must not be NULL");
    HIP_TRY(launch_sim_flat_rank(v_dev, sorted_dev, n, crank_dev, nan_count_dev, (hipStream_t)stream));
    return TVC_OK;
}

int tvc_sim_flat(tvc_handle* h, const float* x_dev, const float* y_dev, const int32_t* cx_dev, const int32_t* cy_dev, int64_t n,
                 double* out_dev, int64_t* ints_dev, void* ws_dev, uint64_t ws_bytes, void* stream) {
    if (!h) return TVC_E_INVALID;
    const SimFlatPlan plan = sim_flat_plan(n);
    if (!plan.ok) return fail(h, TVC_E_INVALID, "tvc_sim_flat: need 1 <= n <= TVC_SIM_MAX_N");
    if (!x_dev || !y_dev || !cx_dev || !cy_dev || !out_dev || !ints_dev)
        return fail(h, TVC_E_INVALID, "tvc_sim_flat: x, y, cx, cy, out and ints must not be NULL");
    if (!ws_dev || ws_bytes < (uint64_t)plan.ws_bytes || ((uintptr_t)ws_dev & 7))
        return fail(h, TVC_E_INVALID, "tvc_sim_flat: the workspace must be 8-byte aligned and hold tvc_sim_flat_workspace(n) bytes");
    SimFlatLaunch L;
    L.x = x_dev; L.y = y_dev; L.cx = cx_dev; L.cy = cy_dev; L.n = n; L.out = out_dev; L.ints = ints_dev; L.ws = ws_dev;
    HIP_TRY(launch_sim_flat(L, (hipStream_t)stream));
    return TVC_OK;
}

int tvc_topk_overlap(tvc_handle* h, const int32_t* a_dev, const int32_t* b_dev, int64_t M, int32_t La, int32_t Lb, int32_t k,
                     int32_t* count_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (M < 0 || M > 0x7fffffffLL) return fail(h, TVC_E_INVALID, "tvc_topk_overlap: need 0 <= M < 2^31");
    if (La < 0 || Lb < 0) return fail(h, TVC_E_INVALID, "tvc_topk_overlap: need La >= 0 and Lb >= 0");
    if (k < 1 || k > TVC_TOPK_OVERLAP_MAX_K) return fail(h, TVC_E_INVALID, "tvc_topk_overlap: need 1 <= k <= TVC_TOPK_OVERLAP_MAX_K");
    if (M == 0) return TVC_OK;
    if (!a_dev || !b_dev || !count_dev) return fail(h, TVC_E_INVALID, "tvc_topk_overlap: a, b and count must not be NULL when M > 0");
    HIP_TRY(launch_topk_overlap(a_dev, b_dev, M, La, Lb, k, count_dev, (hipStream_t)stream));
    return TVC_OK;
}
