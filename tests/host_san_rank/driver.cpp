// Host-only sanitizer driver of the retrieval-evaluation entry points (tests/test_retrieval_host_san.py), built by
// tests/host_san_build.py under ASan / UBSan against tests/host_san's HIP stand-in (kernels are no-ops, "device" blocks are exactly sized
// host blocks).  Walks every refusal of tvc_rank_targets / tvc_rank_count / tvc_rank_metrics (no bank, R = 0, M < 1, T < 0, NULL
// buffers, too many or non-positive k values) and checks that none allocates, then valid calls on an fp32 and on a bf16 slot,
// T = 0, workspace growth from a small to a larger M, the plan of host_plan.hpp, and a leak-free tvc_destroy.
#include "driver_common.hpp"
#include "host_plan.hpp"

#include <vector>

int main() {
    // ---- the plan: whole query tiles, refusals
    CHECK(!rank_plan(0, 10, 64, 2).ok && !rank_plan(-5, 10, 64, 2).ok && !rank_plan(0x7fffffffLL, 10, 64, 2).ok);
    CHECK(rank_plan(1, 10, 64, 2).n_qtiles == 1 && rank_plan(1, 10, 64, 2).mpad == 256);
    CHECK(rank_plan(256, 10, 64, 2).mpad == 256 && rank_plan(257, 10, 64, 3).mpad == 512 && rank_plan(5000, 10, 64, 2).n_qtiles == 20);
    CHECK(rank_plan(2, 3, 64, 3).flops == 2.0 * 3 * 2 * 64 * 3);
    const int32_t k_ok[8] = {1, 5, 10, 20, 50, 100, 1000, 1 << 30}, k_zero[2] = {1, 0}, k_neg[1] = {-3}, k_nine[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
    CHECK(rank_k_values_ok(k_ok, 8) && rank_k_values_ok(nullptr, 0) && !rank_k_values_ok(nullptr, 1));
    CHECK(!rank_k_values_ok(k_zero, 2) && !rank_k_values_ok(k_neg, 1) && !rank_k_values_ok(k_nine, 9) && !rank_k_values_ok(k_ok, -1));

    tvc_handle* h = nullptr;
    CHECK(tvc_create(nullptr, nullptr, nullptr, &h) == TVC_OK && h);       // a handle without towers: the bank calls need none
    std::vector<void*> keep;
    auto buf = [&](size_t elems, size_t es) { void* p = dev(elems * es); keep.push_back(p); return p; };
    const int R = 1000, D = 128, Mmax = 700;
    const int64_t T = 900;
    float* rows32 = (float*)buf((size_t)R * D, 4);
    uint16_t* rows16 = (uint16_t*)buf((size_t)R * D, 2);
    float* q = (float*)buf((size_t)Mmax * D, 4);
    int32_t* qlabel = (int32_t*)buf(Mmax, 4); int32_t* glabel = (int32_t*)buf(R, 4); int32_t* gpos = (int32_t*)buf(R, 4);
    int64_t* off = (int64_t*)buf(Mmax + 1, 8);
    float* sim = (float*)buf(T, 4); int32_t* row = (int32_t*)buf(T, 4); int32_t* hist = (int32_t*)buf(T, 4); int32_t* pos = (int32_t*)buf(T, 4);
    double* ap = (double*)buf(Mmax, 8); double* rr = (double*)buf(Mmax, 8);
    int32_t* hits = (int32_t*)buf((size_t)Mmax * 8, 4); double* dcg = (double*)buf((size_t)Mmax * 8, 8); double* idcg = (double*)buf((size_t)Mmax * 8, 8);

    auto targets = [&](tvc_handle* hh, int M, int64_t t) { return tvc_rank_targets(hh, q, M, qlabel, glabel, gpos, off, t, sim, row, nullptr); };
    auto count = [&](tvc_handle* hh, int M, int64_t t) { return tvc_rank_count(hh, q, M, qlabel, glabel, off, sim, row, t, hist, nullptr); };
    auto metrics = [&](tvc_handle* hh, int M, int64_t t, const int32_t* k, int n_k) {
        return tvc_rank_metrics(hh, M, off, hist, t, k, n_k, pos, ap, rr, hits, dcg, idcg, nullptr);
    };
    CHECK(targets(nullptr, 4, T) == TVC_E_INVALID && count(nullptr, 4, T) == TVC_E_INVALID && metrics(nullptr, 4, T, k_ok, 3) == TVC_E_INVALID);
    // ---- no bank in the slot, then a bank of no rows: TVC_E_STATE, with a message
    CHECK(targets(h, 4, T) == TVC_E_STATE && strlen(tvc_last_error(h)) > 0);
    CHECK(count(h, 4, T) == TVC_E_STATE && metrics(h, 4, T, k_ok, 3) == TVC_E_STATE);
    OK(tvc_bank_set(h, rows32, 0, D, TVC_DTYPE_F32, nullptr));
    CHECK(targets(h, 4, T) == TVC_E_STATE && count(h, 4, T) == TVC_E_STATE && metrics(h, 4, T, k_ok, 3) == TVC_E_STATE);
    OK(tvc_bank_set(h, nullptr, 0, D, TVC_DTYPE_BF16, nullptr));
    const uint64_t ws0 = tvc_workspace_bytes(h);                             // a refusal allocates nothing

    for (int dtype = 0; dtype < 2; ++dtype) {
        OK(tvc_bank_select(h, dtype));
        OK(tvc_bank_set(h, dtype == 0 ? (const void*)rows32 : (const void*)rows16, R, D, dtype == 0 ? TVC_DTYPE_F32 : TVC_DTYPE_BF16, nullptr));
        // M and T out of range
        CHECK(targets(h, 0, T) == TVC_E_INVALID && targets(h, -2, T) == TVC_E_INVALID && targets(h, 4, -1) == TVC_E_INVALID);
        CHECK(count(h, 0, T) == TVC_E_INVALID && count(h, 4, -1) == TVC_E_INVALID);
        CHECK(metrics(h, 0, T, k_ok, 3) == TVC_E_INVALID && metrics(h, 4, -1, k_ok, 3) == TVC_E_INVALID && strlen(tvc_last_error(h)) > 0);
        // k values
        CHECK(metrics(h, 4, T, k_nine, 9) == TVC_E_INVALID && metrics(h, 4, T, k_zero, 2) == TVC_E_INVALID);
        CHECK(metrics(h, 4, T, k_neg, 1) == TVC_E_INVALID && metrics(h, 4, T, nullptr, 2) == TVC_E_INVALID);
        // NULL required buffers
        CHECK(tvc_rank_targets(h, nullptr, 4, qlabel, glabel, gpos, off, T, sim, row, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_targets(h, q, 4, nullptr, glabel, gpos, off, T, sim, row, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_targets(h, q, 4, qlabel, nullptr, gpos, off, T, sim, row, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_targets(h, q, 4, qlabel, glabel, nullptr, off, T, sim, row, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_targets(h, q, 4, qlabel, glabel, gpos, nullptr, T, sim, row, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_targets(h, q, 4, qlabel, glabel, gpos, off, T, nullptr, row, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_targets(h, q, 4, qlabel, glabel, gpos, off, T, sim, nullptr, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_count(h, nullptr, 4, qlabel, glabel, off, sim, row, T, hist, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_count(h, q, 4, qlabel, glabel, nullptr, sim, row, T, hist, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_count(h, q, 4, qlabel, glabel, off, nullptr, row, T, hist, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_count(h, q, 4, qlabel, glabel, off, sim, nullptr, T, hist, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_count(h, q, 4, qlabel, glabel, off, sim, row, T, nullptr, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_metrics(h, 4, nullptr, hist, T, k_ok, 3, pos, ap, rr, hits, dcg, idcg, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_metrics(h, 4, off, nullptr, T, k_ok, 3, pos, ap, rr, hits, dcg, idcg, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_metrics(h, 4, off, hist, T, k_ok, 3, nullptr, ap, rr, hits, dcg, idcg, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_metrics(h, 4, off, hist, T, k_ok, 3, pos, nullptr, rr, hits, dcg, idcg, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_metrics(h, 4, off, hist, T, k_ok, 3, pos, ap, nullptr, hits, dcg, idcg, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_metrics(h, 4, off, hist, T, k_ok, 3, pos, ap, rr, nullptr, dcg, idcg, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_metrics(h, 4, off, hist, T, k_ok, 3, pos, ap, rr, hits, nullptr, idcg, nullptr) == TVC_E_INVALID);
        CHECK(tvc_rank_metrics(h, 4, off, hist, T, k_ok, 3, pos, ap, rr, hits, dcg, nullptr, nullptr) == TVC_E_INVALID);
        if (dtype == 0) CHECK(tvc_workspace_bytes(h) == ws0);
        // ---- T == 0 is legal: the tile calls need no lists and allocate nothing, the metrics call no hist and no pos
        CHECK(tvc_rank_targets(h, q, 4, qlabel, glabel, gpos, off, 0, nullptr, nullptr, nullptr) == TVC_OK);
        CHECK(tvc_rank_count(h, q, 4, qlabel, glabel, off, nullptr, nullptr, 0, nullptr, nullptr) == TVC_OK);
        if (dtype == 0) CHECK(tvc_workspace_bytes(h) == ws0);
        CHECK(tvc_rank_metrics(h, 4, off, nullptr, 0, k_ok, 8, nullptr, ap, rr, hits, dcg, idcg, nullptr) == TVC_OK);
        CHECK(tvc_rank_metrics(h, 4, off, nullptr, 0, nullptr, 0, nullptr, ap, rr, nullptr, nullptr, nullptr, nullptr) == TVC_OK);
        // ---- valid calls; then a larger M grows the workspaces
        OK(targets(h, 4, T)); OK(count(h, 4, T)); OK(metrics(h, 4, T, k_ok, 8));
        const uint64_t small = tvc_workspace_bytes(h);
        OK(targets(h, Mmax, T)); OK(count(h, Mmax, T)); OK(metrics(h, Mmax, T, k_ok, 3));
        if (dtype == 0) CHECK(tvc_workspace_bytes(h) > small);
        OK(targets(h, 1, T)); OK(count(h, 256, T)); OK(count(h, 257, T));    // back to small M, the tile edges: the blocks stay
    }
    // the fp32 slot still answers after the bf16 slot was used; a released slot refuses again
    OK(tvc_bank_select(h, 0));
    OK(count(h, 8, T));
    OK(tvc_bank_set(h, nullptr, 0, 64, TVC_DTYPE_BF16, nullptr));
    CHECK(count(h, 8, T) == TVC_E_STATE && metrics(h, 8, T, k_ok, 3) == TVC_E_STATE);
    // the profiling bracket counts each tile pass as bank work; the metrics call is not bracketed
    OK(tvc_bank_select(h, 1));
    double ms[TVC_PROF_NCAT], work[TVC_PROF_NCAT], big[3]; int64_t launches[TVC_PROF_NCAT];
    OK(tvc_profile_begin(h)); OK(targets(h, 8, T)); OK(count(h, 8, T)); OK(metrics(h, 8, T, k_ok, 3)); OK(tvc_profile_end(h, ms, work, launches, big));
    CHECK(launches[TVC_PROF_BANK] == 2);
    tvc_destroy(h);
    for (void* p : keep) (void)hipFree(p);
    CHECK(hip_stub_blocks().empty());                               // every handle-owned device block was released
    printf("HOST_SAN_RANK_OK\n");
    return 0;
}
