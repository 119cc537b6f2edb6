// C-ABI of the pair-list and pair-cosine kernels (pairs.hip): tvc_graph_pair_count / tvc_graph_pair_fill on any bitmask graph,
// tvc_pair_cosine over the selected bank slot.  Its own translation unit: nothing here is called from another unit, and it owns
// no workspace (the counts are scanned in place in the caller's offsets).
#include "handle.hpp"

static_assert(TVC_RADIUS_MAX_ROWS == RADIUS_MAX_ROWS, "include/tvc.h and host_plan.hpp disagree on the radius graph's row limit");

// the checks the two graph calls share; `fn` names the entry point in the message
static int pair_graph_args(tvc_handle* h, const char* fn, const uint32_t* adj_dev, int32_t R, const int64_t* offsets_dev) {
    if (R < 1 || R > TVC_RADIUS_MAX_ROWS) return fail(h, TVC_E_INVALID, std::string(fn) + ": need 1 <= R <= TVC_RADIUS_MAX_ROWS");
    if (!adj_dev || !offsets_dev) return fail(h, TVC_E_INVALID, std::string(fn) + ": adj and offsets must not be NULL");
    return TVC_OK;
}

int tvc_graph_pair_count(tvc_handle* h, const uint32_t* adj_dev, int32_t R, const int32_t* group_dev, int64_t* offsets_dev,
                         void* stream) {
    if (!h) return TVC_E_INVALID;
    int rc;
    if ((rc = pair_graph_args(h, "tvc_graph_pair_count", adj_dev, R, offsets_dev))) return rc;
    HIP_TRY(launch_graph_pair_count(adj_dev, R, group_dev, offsets_dev, (hipStream_t)stream));
    return TVC_OK;
}

int tvc_graph_pair_fill(tvc_handle* h, const uint32_t* adj_dev, int32_t R, const int32_t* group_dev, const int64_t* offsets_dev,
                        int32_t* pairs_dev, int64_t P, void* stream) {
    if (!h) return TVC_E_INVALID;
    int rc;
    if ((rc = pair_graph_args(h, "tvc_graph_pair_fill", adj_dev, R, offsets_dev))) return rc;
    if (P < 0) return fail(h, TVC_E_INVALID, "tvc_graph_pair_fill: need P >= 0");
    if (P == 0) return TVC_OK;
    if (!pairs_dev) return fail(h, TVC_E_INVALID, "tvc_graph_pair_fill: pairs must not be NULL when P > 0");
    HIP_TRY(launch_graph_pair_fill(adj_dev, R, group_dev, offsets_dev, pairs_dev, P, (hipStream_t)stream));
    return TVC_OK;
}

int tvc_pair_cosine(tvc_handle* h, const int32_t* pairs_dev, int64_t P, float* sim_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    BankSlot* slot;
    if (int rc = filled_slot(h, "tvc_pair_cosine", &slot)) return rc;
    const BankSlot& bk = *slot;
    if (P < 0) return fail(h, TVC_E_INVALID, "tvc_pair_cosine: need P >= 0");
    if (P == 0) return TVC_OK;
    if (!pairs_dev || !sim_dev) return fail(h, TVC_E_INVALID, "tvc_pair_cosine: pairs and sim must not be NULL when P > 0");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(h, st, TVC_PROF_BANK, 6.0 * (double)P * bk.D);       // three FMAs per element of a pair
    HIP_TRY(launch_pair_cosine(bank_rows(bk), pairs_dev, P, sim_dev, st));
    return TVC_OK;
}
