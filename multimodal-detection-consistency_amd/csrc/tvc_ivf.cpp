// C-ABI of the IVF search (ivf.hip): tvc_ivf_probe (needs no bank) and tvc_ivf_scan over the selected bank slot.  Its own
// translation unit: nothing here is called from tvc_abi.cpp.  Every refusal comes before the first allocation and launch.
#include "handle.hpp"

int tvc_ivf_probe(tvc_handle* h, const float* rows_dev, int32_t M, int32_t D, const float* centroids_dev, int32_t nlist,
                  int32_t nprobe, int32_t* lists_dev, float* score_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (nprobe < 1 || nprobe > TVC_MAX_TOPK) return fail(h, TVC_E_INVALID, "tvc_ivf_probe: need 1 <= nprobe <= 128");
    if (nlist < 1 || nlist > IVF_MAX_NLIST) return fail(h, TVC_E_INVALID, "tvc_ivf_probe: need 1 <= nlist <= 65536");
    if (D <= 0 || D % 64 != 0 || M < 0) return fail(h, TVC_E_INVALID, "tvc_ivf_probe: need M >= 0 and D % 64 == 0");
    if (!centroids_dev || (M > 0 && (!rows_dev || !lists_dev)))
        return fail(h, TVC_E_INVALID, "tvc_ivf_probe: rows, centroids and lists must not be NULL");
    if (M == 0) return TVC_OK;
    hipStream_t st = (hipStream_t)stream;
    IvfProbeLaunch L;
    int64_t chunk = IVF_PROBE_SIMS_FLOATS / nlist;
    if (chunk > M) chunk = M;
    L.chunk = (int)chunk;
    int rc;
    if ((rc = ensure_planes(h, WS_IVF_CPLANES, nlist, 1, D))) return rc;
    if ((rc = ensure_planes(h, WS_IVF_PQPLANES, M, 1, D))) return rc;
    if ((rc = ensure(h, WS_IVF_HALFNORM, (size_t)nlist * 4))) return rc;
    if ((rc = ensure(h, WS_IVF_SIMS, (size_t)chunk * nlist * 4))) return rc;
    if ((rc = split_planes(h, WS_IVF_CPLANES, centroids_dev, nlist, D, st, &L.cplanes))) return rc;
    if ((rc = split_planes(h, WS_IVF_PQPLANES, rows_dev, M, D, st, &L.qplanes))) return rc;
    L.centroids = centroids_dev; L.halfnorm = (float*)h->ws[WS_IVF_HALFNORM].p;
    L.M = M; L.D = D; L.nlist = nlist; L.nprobe = nprobe;
    L.sims = (float*)h->ws[WS_IVF_SIMS].p; L.lists = lists_dev; L.score = score_dev;
    ProfScope ps(h, st, TVC_PROF_BANK, 2.0 * (double)M * nlist * D * 3);
    HIP_TRY(launch_ivf_probe(L, st));
    return TVC_OK;
}

int tvc_ivf_scan(tvc_handle* h, const float* rows_dev, int32_t M, int32_t k, const int32_t* probes_dev, int32_t nprobe,
                 const int32_t* list_offsets_dev, int32_t nlist, int32_t max_list_rows, const int32_t* row_ids_dev,
                 int64_t idx_offset, int32_t* topk_idx_dev, float* topk_sim_dev, int32_t* topk_pos_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    BankSlot* slot;
    int rc;
    if ((rc = filled_slot(h, "tvc_ivf_scan", &slot))) return rc;
    const BankSlot& bk = *slot;
    if (k < 1 || k > TVC_MAX_TOPK || nprobe < 1 || nprobe > TVC_MAX_TOPK)
        return fail(h, TVC_E_INVALID, "tvc_ivf_scan: need 1 <= k <= 128 and 1 <= nprobe <= 128");
    if (nlist < 1 || nlist > IVF_MAX_NLIST || max_list_rows < 1 || M < 0)
        return fail(h, TVC_E_INVALID, "tvc_ivf_scan: need 1 <= nlist <= 65536, max_list_rows >= 1 and M >= 0");
    if (!list_offsets_dev || (M > 0 && (!rows_dev || !probes_dev || !topk_idx_dev || !topk_sim_dev)))
        return fail(h, TVC_E_INVALID, "tvc_ivf_scan: rows, probes, list_offsets, topk_idx and topk_sim must not be NULL");
    if (!ivf_scan_covers(bk.D)) return fail(h, TVC_E_INVALID, "tvc_ivf_scan: the slot's D must be 128, 512 or 768");
    if (M == 0) return TVC_OK;
    const int D = bk.D;
    IvfScanLaunch L;
    L.plan = ivf_scan_plan(M, nprobe, nlist, max_list_rows, D, bk.planes);
    if (!L.plan.ok)
        return fail(h, TVC_E_INVALID, "tvc_ivf_scan: nprobe x round_up(max_list_rows, 16) floats exceed the 256 MiB score workspace");
    hipStream_t st = (hipStream_t)stream;
    if ((rc = ensure_planes(h, WS_IVF_QPLANES, M, 1, D))) return rc;
    if ((rc = ensure(h, WS_IVF_BLKCNT, (size_t)L.plan.sort_blocks * nlist * 4))) return rc;
    if ((rc = ensure(h, WS_IVF_PCOUNTS, (size_t)nlist * 4))) return rc;
    if ((rc = ensure(h, WS_IVF_POFFSETS, ((size_t)nlist + 1) * 4))) return rc;
    if ((rc = ensure(h, WS_IVF_PORDER, (size_t)L.plan.chunk * nprobe * 4))) return rc;
    if ((rc = ensure(h, WS_IVF_SCORES, (size_t)L.plan.score_bytes))) return rc;
    if ((rc = ensure(h, WS_OVERFLOW, 16))) return rc;
    if ((rc = split_planes(h, WS_IVF_QPLANES, rows_dev, M, D, st, &L.qplanes))) return rc;
    L.bank = bank_rows(bk);
    L.M = M; L.k = k; L.nprobe = nprobe; L.nlist = nlist; L.max_list_rows = max_list_rows;
    L.probes = probes_dev; L.list_offsets = list_offsets_dev; L.row_ids = row_ids_dev; L.idx_offset = idx_offset;
    L.blk_cnt = (int32_t*)h->ws[WS_IVF_BLKCNT].p; L.pair_counts = (int32_t*)h->ws[WS_IVF_PCOUNTS].p;
    L.pair_offsets = (int32_t*)h->ws[WS_IVF_POFFSETS].p; L.pair_order = (int32_t*)h->ws[WS_IVF_PORDER].p;
    L.scores = (float*)h->ws[WS_IVF_SCORES].p; L.overflow = (int32_t*)h->ws[WS_OVERFLOW].p;
    L.topk_idx = topk_idx_dev; L.topk_sim = topk_sim_dev; L.topk_pos = topk_pos_dev;
    // work as the bank search counts it: the rows of nprobe lists of R / nlist rows per query, 2 or 3 plane products
    ProfScope ps(h, st, TVC_PROF_BANK, 2.0 * (double)M * nprobe * ((double)bk.R / nlist) * D * bank_products(bk.planes));
    HIP_TRY(launch_ivf_scan(L, st));
    return TVC_OK;
}
