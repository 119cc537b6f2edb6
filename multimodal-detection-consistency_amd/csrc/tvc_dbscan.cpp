// C-ABI of the radius-graph and DBSCAN kernels (dbscan.hip): tvc_radius_graph over the selected bank slot, tvc_dbscan_sweep /
// tvc_dbscan_finish on any bitmask graph.  Its own translation unit: nothing here is called from tvc_abi.cpp.
#include "handle.hpp"

#include <cmath>

static_assert(TVC_RADIUS_MAX_ROWS == RADIUS_MAX_ROWS, "include/tvc.h and host_plan.hpp disagree on the radius graph's row limit");

int tvc_radius_graph(tvc_handle* h, float eps, uint32_t* adj_dev, int32_t* degree_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    BankSlot* slot;
    int rc;
    if ((rc = filled_slot(h, "tvc_radius_graph", &slot))) return rc;
    const BankSlot& bk = *slot;
    if (!std::isfinite(eps) || !(eps > 0.f)) return fail(h, TVC_E_INVALID, "tvc_radius_graph: eps must be finite and positive");
    if (bk.R > TVC_RADIUS_MAX_ROWS) return fail(h, TVC_E_INVALID, "tvc_radius_graph: the slot holds more than TVC_RADIUS_MAX_ROWS rows");
    if (!adj_dev || !degree_dev) return fail(h, TVC_E_INVALID, "tvc_radius_graph: adj and degree must not be NULL");
    if ((uintptr_t)adj_dev % 8 != 0) return fail(h, TVC_E_INVALID, "tvc_radius_graph: adj must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    RadiusGraphLaunch L;
    L.plan = radius_plan(bk.R);
    if ((rc = ensure(h, WS_DB_HALF, (size_t)L.plan.hpad * 4))) return rc;
    L.bank = bank_rows(bk);
    L.eps = eps;
    L.half = (float*)h->ws[WS_DB_HALF].p;
    L.adj = adj_dev; L.degree = degree_dev;
    const int products = bk.planes == 2 ? 4 : 1;
    ProfScope ps(h, st, TVC_PROF_BANK, 2.0 * L.plan.tile_pairs * HOST_PLAN_GEMM_BM * HOST_PLAN_GEMM_BN * bk.D * products);
    HIP_TRY(launch_radius_graph(L, st));
    return TVC_OK;
}

// the checks the two component calls share; `fn` names the entry point in the message
static int dbscan_args(tvc_handle* h, const char* fn, int32_t R, int32_t min_samples) {
    if (R < 1 || R > TVC_RADIUS_MAX_ROWS) return fail(h, TVC_E_INVALID, std::string(fn) + ": need 1 <= R <= TVC_RADIUS_MAX_ROWS");
    if (min_samples < 1) return fail(h, TVC_E_INVALID, std::string(fn) + ": need min_samples >= 1");
    return TVC_OK;
}

int tvc_dbscan_sweep(tvc_handle* h, const uint32_t* adj_dev, const int32_t* degree_dev, int32_t R, int32_t min_samples,
                     int32_t* comp_dev, int32_t* changed_dev, int32_t init, void* stream) {
    if (!h) return TVC_E_INVALID;
    int rc;
    if ((rc = dbscan_args(h, "tvc_dbscan_sweep", R, min_samples))) return rc;
    if (!adj_dev || !degree_dev || !comp_dev || !changed_dev)
        return fail(h, TVC_E_INVALID, "tvc_dbscan_sweep: adj, degree, comp and changed must not be NULL");
    HIP_TRY(launch_dbscan_sweep(adj_dev, degree_dev, R, min_samples, comp_dev, changed_dev, init != 0, (hipStream_t)stream));
    return TVC_OK;
}

int tvc_dbscan_finish(tvc_handle* h, const uint32_t* adj_dev, const int32_t* degree_dev, int32_t R, int32_t min_samples,
                      const int32_t* comp_dev, int32_t* labels_dev, uint8_t* core_dev, int32_t* n_clusters_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    int rc;
    if ((rc = dbscan_args(h, "tvc_dbscan_finish", R, min_samples))) return rc;
    if (!adj_dev || !degree_dev || !comp_dev || !labels_dev || !core_dev || !n_clusters_dev)
        return fail(h, TVC_E_INVALID, "tvc_dbscan_finish: adj, degree, comp, labels, core and n_clusters must not be NULL");
    HIP_TRY(launch_dbscan_finish(adj_dev, degree_dev, R, min_samples, comp_dev, labels_dev, core_dev, n_clusters_dev, (hipStream_t)stream));
    return TVC_OK;
}
