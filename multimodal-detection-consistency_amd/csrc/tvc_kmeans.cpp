// C-ABI of the k-means kernels (kmeans.hip): tvc_kmeans_assign / tvc_kmeans_update over the selected bank slot.  Its own
// translation unit: nothing here is called from tvc_abi.cpp.
#include "handle.hpp"

// the slot the call addresses, or the refusal
static int kmeans_slot(tvc_handle* h, const char* fn, int32_t K, BankSlot** out) {
    int rc;
    if ((rc = filled_slot(h, fn, out))) return rc;
    if (K < 1 || K > (*out)->R || K > KMEANS_MAX_K) return fail(h, TVC_E_INVALID, std::string(fn) + ": need 1 <= K <= min(R, 65536)");
    return TVC_OK;
}

int tvc_kmeans_assign(tvc_handle* h, const float* centroids_dev, int32_t K, int32_t* labels_dev, float* score_dev,
                      float* dist2_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    BankSlot* bk;
    int rc;
    if ((rc = kmeans_slot(h, "tvc_kmeans_assign", K, &bk))) return rc;
    if (!centroids_dev || !labels_dev) return fail(h, TVC_E_INVALID, "tvc_kmeans_assign: centroids and labels must not be NULL");
    hipStream_t st = (hipStream_t)stream;
    const int D = bk->D;
    const size_t Kpad = ((size_t)K + HOST_PLAN_GEMM_BM - 1) / HOST_PLAN_GEMM_BM * HOST_PLAN_GEMM_BM;
    if ((rc = ensure_planes(h, WS_KM_CPLANES, K, 1, D))) return rc;
    if ((rc = ensure(h, WS_KM_HALFNORM, Kpad * 4))) return rc;
    KmeansAssignLaunch L;
    if ((rc = split_planes(h, WS_KM_CPLANES, centroids_dev, K, D, st, &L.cplanes))) return rc;
    L.bank = bank_rows(*bk);
    L.centroids = centroids_dev; L.K = K;
    L.halfnorm = (float*)h->ws[WS_KM_HALFNORM].p;
    L.labels = labels_dev; L.score = score_dev; L.dist2 = dist2_dev;
    ProfScope ps(h, st, TVC_PROF_BANK, slot_pass_flops(bk->R, K, D, bank_products(bk->planes)));
    HIP_TRY(launch_kmeans_assign(L, st));
    return TVC_OK;
}

int tvc_kmeans_update(tvc_handle* h, const int32_t* labels_dev, const float* centroids_in_dev, int32_t K,
                      float* centroids_out_dev, int32_t* counts_dev, int32_t* offsets_dev, int32_t* order_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    BankSlot* bk;
    int rc;
    if ((rc = kmeans_slot(h, "tvc_kmeans_update", K, &bk))) return rc;
    if (!labels_dev || !centroids_in_dev || !centroids_out_dev || !counts_dev)
        return fail(h, TVC_E_INVALID, "tvc_kmeans_update: labels, centroids_in, centroids_out and counts must not be NULL");
    hipStream_t st = (hipStream_t)stream;
    KmeansUpdateLaunch L;
    kmeans_update_plan(bk->R, K, &L.nblocks, &L.rows_per_block);
    if ((rc = ensure(h, WS_KM_BLKCNT, (size_t)L.nblocks * K * 4))) return rc;
    if (!offsets_dev) {
        if ((rc = ensure(h, WS_KM_OFFSETS, ((size_t)K + 1) * 4))) return rc;
        offsets_dev = (int32_t*)h->ws[WS_KM_OFFSETS].p;
    }
    if (!order_dev) {
        if ((rc = ensure(h, WS_KM_ORDER, (size_t)bk->R * 4))) return rc;
        order_dev = (int32_t*)h->ws[WS_KM_ORDER].p;
    }
    L.bank = bank_rows(*bk);
    L.labels = labels_dev; L.centroids_in = centroids_in_dev; L.K = K;
    L.blk_cnt = (int32_t*)h->ws[WS_KM_BLKCNT].p;
    L.centroids_out = centroids_out_dev; L.counts = counts_dev; L.offsets = offsets_dev; L.order = order_dev;
    HIP_TRY(launch_kmeans_update(L, st));
    return TVC_OK;
}
