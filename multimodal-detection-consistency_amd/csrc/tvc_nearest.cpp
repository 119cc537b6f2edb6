// C-ABI of the closest-pair kernels (nearest.hip): tvc_closest_pair over the selected bank slot.  Its own translation unit:
// nothing here is called from tvc_abi.cpp.
#include "handle.hpp"

int tvc_closest_pair(tvc_handle* h, int32_t* partner_dev, float* sim_dev, int32_t* pair_dev, float* pair_sim_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    const BankSlot& bk = h->banks[h->cur_bank];
    if (bk.D == 0 || !bk.bank) return fail(h, TVC_E_INVALID, "tvc_closest_pair: the selected slot holds no bank");
    if (bk.R < 1) return fail(h, TVC_E_INVALID, "tvc_closest_pair: the selected slot holds no rows");
    if (!partner_dev || !sim_dev || !pair_dev || !pair_sim_dev)
        return fail(h, TVC_E_INVALID, "tvc_closest_pair: partner, sim, pair and pair_sim must not be NULL");
    if (bk.D % 64 != 0) return fail(h, TVC_E_INVALID, "tvc_closest_pair: D must be a multiple of 64");
    ClosestPairLaunch L;
    L.plan = nearest_plan(bk.R);
    if (!L.plan.ok) return fail(h, TVC_E_INVALID, "tvc_closest_pair: the slot holds more than 2^31 - 257 rows");
    int rc;
    if ((rc = ensure(h, WS_NN_RINV, (size_t)L.plan.rpad * 4))) return rc;
    hipStream_t st = (hipStream_t)stream;
    L.bank = bank_rows(bk);
    L.rinv = (float*)h->ws[WS_NN_RINV].p;
    L.partner = partner_dev; L.sim = sim_dev; L.pair = pair_dev; L.pair_sim = pair_sim_dev;
    const int products = bk.planes == 2 ? 4 : 1;
    ProfScope ps(h, st, TVC_PROF_BANK, 2.0 * L.plan.tile_pairs * HOST_PLAN_GEMM_BM * HOST_PLAN_GEMM_BN * bk.D * products);
    HIP_TRY(launch_closest_pair(L, st));
    return TVC_OK;
}
