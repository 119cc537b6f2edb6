// Host-only sanitizer driver of the IVF entry points (tests/test_ivf_host.py), built by tests/host_san_build.py
// under ASan / UBSan against tests/host_san's HIP stand-in (kernels are no-ops, "device" blocks are exactly sized
// host blocks).  Walks every refusal of tvc_ivf_probe / tvc_ivf_scan and checks that a refusal allocates nothing, valid calls
// on an fp32 and on a bf16 slot with the optional outputs present and absent, workspace growth, a released slot and a
// leak-free tvc_destroy.
#include "driver_common.hpp"

#include <vector>

int main() {
    tvc_handle* h = nullptr;
    CHECK(tvc_create(nullptr, nullptr, nullptr, &h) == TVC_OK && h);
    std::vector<void*> keep;
    auto buf = [&](size_t elems, size_t es) { void* p = dev(elems * es); keep.push_back(p); return p; };
    const int R = 2000, D = 128, M = 70, K = 128, NL = 300, NP = 16;
    float* rows32 = (float*)buf((size_t)R * D, 4);
    uint16_t* rows16 = (uint16_t*)buf((size_t)R * D, 2);
    float* q = (float*)buf((size_t)M * D, 4);
    float* cent = (float*)buf((size_t)NL * D, 4);
    int32_t* lists = (int32_t*)buf((size_t)M * 128, 4); float* score = (float*)buf((size_t)M * 128, 4);
    int32_t* offs = (int32_t*)buf(NL + 1, 4); int32_t* ids = (int32_t*)buf(R, 4);
    int32_t* idx = (int32_t*)buf((size_t)M * K, 4); float* sim = (float*)buf((size_t)M * K, 4); int32_t* pos = (int32_t*)buf((size_t)M * K, 4);

    // ---- probe: needs no bank; every refusal, none allocates
    const uint64_t ws0 = tvc_workspace_bytes(h);
    CHECK(tvc_ivf_probe(nullptr, q, M, D, cent, NL, NP, lists, score, nullptr) == TVC_E_INVALID);
    CHECK(tvc_ivf_probe(h, q, M, D, cent, NL, 0, lists, score, nullptr) == TVC_E_INVALID && strlen(tvc_last_error(h)) > 0);
    CHECK(tvc_ivf_probe(h, q, M, D, cent, NL, 129, lists, score, nullptr) == TVC_E_INVALID);
    CHECK(tvc_ivf_probe(h, q, M, D, cent, 0, NP, lists, score, nullptr) == TVC_E_INVALID);
    CHECK(tvc_ivf_probe(h, q, M, D, cent, 65537, NP, lists, score, nullptr) == TVC_E_INVALID);
    CHECK(tvc_ivf_probe(h, q, M, 100, cent, NL, NP, lists, score, nullptr) == TVC_E_INVALID);
    CHECK(tvc_ivf_probe(h, q, M, 0, cent, NL, NP, lists, score, nullptr) == TVC_E_INVALID);
    CHECK(tvc_ivf_probe(h, q, -1, D, cent, NL, NP, lists, score, nullptr) == TVC_E_INVALID);
    CHECK(tvc_ivf_probe(h, nullptr, M, D, cent, NL, NP, lists, score, nullptr) == TVC_E_INVALID);
    CHECK(tvc_ivf_probe(h, q, M, D, nullptr, NL, NP, lists, score, nullptr) == TVC_E_INVALID);
    CHECK(tvc_ivf_probe(h, q, M, D, cent, NL, NP, nullptr, score, nullptr) == TVC_E_INVALID);
    CHECK(tvc_workspace_bytes(h) == ws0);
    OK(tvc_ivf_probe(h, q, 0, D, cent, NL, NP, lists, score, nullptr));            // no rows: nothing to do
    CHECK(tvc_workspace_bytes(h) == ws0);
    OK(tvc_ivf_probe(h, q, 3, D, cent, 5, 5, lists, score, nullptr));
    OK(tvc_ivf_probe(h, q, 3, D, cent, 5, 128, lists, nullptr, nullptr));           // nprobe > nlist, no scores
    const uint64_t small = tvc_workspace_bytes(h);
    OK(tvc_ivf_probe(h, q, M, D, cent, NL, NP, lists, score, nullptr));
    CHECK(tvc_workspace_bytes(h) > small);
    OK(tvc_ivf_probe(h, q, 1, D, cent, 1, 1, lists, score, nullptr));

    // ---- scan: no bank in the slot, then a bank of no rows: TVC_E_STATE
    const uint64_t ws1 = tvc_workspace_bytes(h);
    CHECK(tvc_ivf_scan(nullptr, q, M, K, lists, NP, offs, NL, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID);
    CHECK(tvc_ivf_scan(h, q, M, K, lists, NP, offs, NL, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_STATE && strlen(tvc_last_error(h)) > 0);
    OK(tvc_bank_set(h, rows32, 0, D, TVC_DTYPE_F32, nullptr));
    CHECK(tvc_ivf_scan(h, q, M, K, lists, NP, offs, NL, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_STATE);
    // a slot whose width the row stream does not cover
    OK(tvc_bank_select(h, 2));
    OK(tvc_bank_set(h, rows16, R, 64, TVC_DTYPE_BF16, nullptr));
    CHECK(tvc_ivf_scan(h, q, M, K, lists, NP, offs, NL, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID);
    OK(tvc_bank_set(h, rows16, R / 2, 256, TVC_DTYPE_BF16, nullptr));
    CHECK(tvc_ivf_scan(h, q, M, K, lists, NP, offs, NL, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID);
    CHECK(tvc_workspace_bytes(h) == ws1);

    for (int dtype = 0; dtype < 2; ++dtype) {
        OK(tvc_bank_select(h, dtype));
        OK(tvc_bank_set(h, dtype == 0 ? (const void*)rows32 : (const void*)rows16, R, D, dtype == 0 ? TVC_DTYPE_F32 : TVC_DTYPE_BF16, nullptr));
        const uint64_t ws2 = tvc_workspace_bytes(h);
        // k, nprobe, nlist, max_list_rows, M out of range
        CHECK(tvc_ivf_scan(h, q, M, 0, lists, NP, offs, NL, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID);
        CHECK(tvc_ivf_scan(h, q, M, 129, lists, NP, offs, NL, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID);
        CHECK(tvc_ivf_scan(h, q, M, K, lists, 0, offs, NL, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID);
        CHECK(tvc_ivf_scan(h, q, M, K, lists, 129, offs, NL, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID);
        CHECK(tvc_ivf_scan(h, q, M, K, lists, NP, offs, 0, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID);
        CHECK(tvc_ivf_scan(h, q, M, K, lists, NP, offs, 65537, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID);
        CHECK(tvc_ivf_scan(h, q, M, K, lists, NP, offs, NL, 0, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID);
        CHECK(tvc_ivf_scan(h, q, M, K, lists, NP, offs, NL, -7, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID);
        CHECK(tvc_ivf_scan(h, q, -1, K, lists, NP, offs, NL, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID);
        // one query's scores would not fit the 256 MiB workspace: refused, never truncated
        CHECK(tvc_ivf_scan(h, q, M, K, lists, 128, offs, NL, 0x7fffffff, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID &&
              strlen(tvc_last_error(h)) > 0);
        // NULL required buffers
        CHECK(tvc_ivf_scan(h, nullptr, M, K, lists, NP, offs, NL, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID);
        CHECK(tvc_ivf_scan(h, q, M, K, nullptr, NP, offs, NL, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID);
        CHECK(tvc_ivf_scan(h, q, M, K, lists, NP, nullptr, NL, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_INVALID);
        CHECK(tvc_ivf_scan(h, q, M, K, lists, NP, offs, NL, 40, ids, 0, nullptr, sim, pos, nullptr) == TVC_E_INVALID);
        CHECK(tvc_ivf_scan(h, q, M, K, lists, NP, offs, NL, 40, ids, 0, idx, nullptr, pos, nullptr) == TVC_E_INVALID);
        CHECK(tvc_workspace_bytes(h) == ws2);
        OK(tvc_ivf_scan(h, q, 0, K, lists, NP, offs, NL, 40, ids, 0, idx, sim, pos, nullptr));
        CHECK(tvc_workspace_bytes(h) == ws2);
        // ---- valid calls: optional row_ids / pos present and absent; a longer list and more probes grow the workspaces
        OK(tvc_ivf_scan(h, q, 3, 1, lists, 1, offs, NL, 1, ids, 0, idx, sim, pos, nullptr));
        OK(tvc_ivf_scan(h, q, 3, 1, lists, 1, offs, NL, 1, nullptr, 5, idx, sim, nullptr, nullptr));
        const uint64_t before = tvc_workspace_bytes(h);
        OK(tvc_ivf_scan(h, q, M, K, lists, NP, offs, NL, 700, ids, 1000, idx, sim, pos, nullptr));
        if (dtype == 0) CHECK(tvc_workspace_bytes(h) > before);
        OK(tvc_ivf_scan(h, q, M, 20, lists, 128, offs, NL, R, nullptr, 0, idx, sim, pos, nullptr));
        // many queries against long lists: the queries are chunked under the 256 MiB budget
        OK(tvc_ivf_scan(h, q, M, 20, lists, 128, offs, NL, 200000, nullptr, 0, idx, sim, pos, nullptr));
    }
    // the fp32 slot still answers after the bf16 slot was used; a released slot refuses again
    OK(tvc_bank_select(h, 0));
    OK(tvc_ivf_scan(h, q, M, K, lists, NP, offs, NL, 40, ids, 0, idx, sim, pos, nullptr));
    OK(tvc_bank_set(h, nullptr, 0, 64, TVC_DTYPE_BF16, nullptr));
    CHECK(tvc_ivf_scan(h, q, M, K, lists, NP, offs, NL, 40, ids, 0, idx, sim, pos, nullptr) == TVC_E_STATE);
    // the profiling bracket counts probe and scan as bank work
    OK(tvc_bank_select(h, 1));
    double ms[TVC_PROF_NCAT], work[TVC_PROF_NCAT], big[3]; int64_t launches[TVC_PROF_NCAT];
    OK(tvc_profile_begin(h));
    OK(tvc_ivf_probe(h, q, M, D, cent, NL, NP, lists, score, nullptr));
    OK(tvc_ivf_scan(h, q, M, K, lists, NP, offs, NL, 40, ids, 0, idx, sim, pos, nullptr));
    OK(tvc_profile_end(h, ms, work, launches, big));
    CHECK(launches[TVC_PROF_BANK] == 2);
    tvc_destroy(h);
    for (void* p : keep) (void)hipFree(p);
    CHECK(hip_stub_blocks().empty());                               // every handle-owned device block was released
    printf("HOST_SAN_IVF_OK\n");
    return 0;
}
