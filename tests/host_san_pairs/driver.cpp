// Host-only sanitizer driver of the pair-list / pair-cosine entry points (tests/test_validator_host.py), built by
// tests/host_san_build.py under ASan / UBSan against tests/host_san's HIP stand-in (kernels are no-ops that write
// their name to the stand-in's trace, "device" blocks are exactly sized host blocks).  Walks the launch plan of host_plan.hpp,
// every refusal of tvc_graph_pair_count / tvc_graph_pair_fill (no handle, R out of range, P < 0, NULL buffers) and of
// tvc_pair_cosine (no handle, an empty slot, P < 0, NULL buffers), checks through the trace that a refusal and P == 0 launch
// nothing and that an accepted call launches exactly its own kernel, that no call owns a workspace, the profiling bracket,
// and a leak-free tvc_destroy.
#include "driver_common.hpp"
#include "host_plan.hpp"

#include <string>
#include <vector>

// a refusal through fail() that launches nothing: the shared REFUSED between two counts of the trace's launch lines
#define QUIET_REFUSED(call, code, fn) do { const long before__ = launches("launch_"); REFUSED(call, code, fn); CHECK(launches("launch_") == before__); } while (0)

// lines of the stand-in's trace that start with `prefix`
static long launches(const char* prefix) {
    FILE* t = hip_trace();
    if (!t) abort();
    fflush(t);
    FILE* f = fopen(getenv("HIP_STUB_TRACE"), "r");
    if (!f) abort();
    long n = 0;
    char line[4096];
    while (fgets(line, sizeof line, f)) n += strncmp(line, prefix, strlen(prefix)) == 0;
    fclose(f);
    return n;
}

int main() {
    CHECK(getenv("HIP_STUB_TRACE") != nullptr);
    // the plan the product and this build share
    const int64_t Rs[] = {1, 2, 3, 4, 5, 63, 64, 65, 1000, 1023, 1024, 1025, 65535, 65536, 65537, 131071, 131072};
    for (int64_t R : Rs) {
        const PairsPlan p = pairs_plan(R);
        CHECK(p.ok && p.words == radius_plan(R).words && p.words * 32 >= R);
        CHECK(p.row_grid >= 1 && p.row_grid <= PAIRS_MAX_GRID && (p.row_grid == PAIRS_MAX_GRID || (int64_t)p.row_grid * 4 >= R));
        CHECK(p.scan_per >= 1 && (int64_t)p.scan_per * PAIRS_SCAN_THREADS >= R && (int64_t)(p.scan_per - 1) * PAIRS_SCAN_THREADS < R);
        CHECK(p.scan_per <= 128);
    }
    CHECK(!pairs_plan(0).ok && !pairs_plan(-3).ok && !pairs_plan(131073).ok);
    CHECK(256 % PAIR_COS_LANES == 0 && PAIR_COS_LANES <= 64);
    CHECK(pair_cosine_grid(0) == 0 && pair_cosine_grid(-1) == 0 && pair_cosine_grid(1) == 1 && pair_cosine_grid(16) == 1);
    CHECK(pair_cosine_grid(17) == 2 && pair_cosine_grid((int64_t)1 << 40) == 65536);

    tvc_handle* h = nullptr;
    CHECK(tvc_create(nullptr, nullptr, nullptr, &h) == TVC_OK && h);       // a handle without towers: the calls need none
    std::vector<void*> keep;
    auto buf = [&](size_t elems, size_t es) { void* p = dev(elems * es); keep.push_back(p); return p; };
    const int R = 1000, D = 128;
    const int W = pairs_plan(R).words;
    const int64_t P = 777;
    float* rows32 = (float*)buf((size_t)R * D, 4);
    uint16_t* rows16 = (uint16_t*)buf((size_t)R * D, 2);
    uint32_t* adj = (uint32_t*)buf((size_t)R * W, 4);
    int32_t* group = (int32_t*)buf(R, 4);
    int64_t* offsets = (int64_t*)buf(R + 1, 8);
    int32_t* pairs = (int32_t*)buf(P * 2, 4);
    float* sim = (float*)buf(P, 4);
    const char* PC = "tvc_graph_pair_count";
    const char* PF = "tvc_graph_pair_fill";
    const char* CO = "tvc_pair_cosine";
    const uint64_t ws0 = tvc_workspace_bytes(h);

    // ---- tvc_graph_pair_count / tvc_graph_pair_fill: they read no bank slot
    CHECK(tvc_graph_pair_count(nullptr, adj, R, group, offsets, nullptr) == TVC_E_INVALID);
    CHECK(tvc_graph_pair_fill(nullptr, adj, R, group, offsets, pairs, P, nullptr) == TVC_E_INVALID);
    QUIET_REFUSED(tvc_graph_pair_count(h, adj, 0, group, offsets, nullptr), TVC_E_INVALID, PC);
    QUIET_REFUSED(tvc_graph_pair_count(h, adj, -1, group, offsets, nullptr), TVC_E_INVALID, PC);
    QUIET_REFUSED(tvc_graph_pair_count(h, adj, TVC_RADIUS_MAX_ROWS + 1, group, offsets, nullptr), TVC_E_INVALID, PC);
    QUIET_REFUSED(tvc_graph_pair_count(h, nullptr, R, group, offsets, nullptr), TVC_E_INVALID, PC);
    QUIET_REFUSED(tvc_graph_pair_count(h, adj, R, group, nullptr, nullptr), TVC_E_INVALID, PC);
    QUIET_REFUSED(tvc_graph_pair_fill(h, adj, 0, group, offsets, pairs, P, nullptr), TVC_E_INVALID, PF);
    QUIET_REFUSED(tvc_graph_pair_fill(h, adj, TVC_RADIUS_MAX_ROWS + 1, group, offsets, pairs, P, nullptr), TVC_E_INVALID, PF);
    QUIET_REFUSED(tvc_graph_pair_fill(h, adj, R, group, offsets, pairs, -1, nullptr), TVC_E_INVALID, PF);
    QUIET_REFUSED(tvc_graph_pair_fill(h, nullptr, R, group, offsets, pairs, P, nullptr), TVC_E_INVALID, PF);
    QUIET_REFUSED(tvc_graph_pair_fill(h, adj, R, group, nullptr, pairs, P, nullptr), TVC_E_INVALID, PF);
    QUIET_REFUSED(tvc_graph_pair_fill(h, adj, R, group, offsets, nullptr, P, nullptr), TVC_E_INVALID, PF);
    long n0 = launches("launch_");
    OK(tvc_graph_pair_fill(h, adj, R, group, offsets, pairs, 0, nullptr));            // P == 0 is legal and launches nothing
    OK(tvc_graph_pair_fill(h, adj, R, nullptr, offsets, nullptr, 0, nullptr));
    CHECK(launches("launch_") == n0);
    OK(tvc_graph_pair_count(h, adj, R, group, offsets, nullptr));
    OK(tvc_graph_pair_count(h, adj, R, nullptr, offsets, nullptr));                   // the group vector is optional
    OK(tvc_graph_pair_count(h, adj, 1, nullptr, offsets, nullptr));
    OK(tvc_graph_pair_count(h, adj, TVC_RADIUS_MAX_ROWS, nullptr, offsets, nullptr)); // nothing is read here: only the checks run
    CHECK(launches("launch_graph_pair_count") == 4 && launches("launch_") == n0 + 4);
    OK(tvc_graph_pair_fill(h, adj, R, group, offsets, pairs, P, nullptr));
    OK(tvc_graph_pair_fill(h, adj, R, nullptr, offsets, pairs, 1, nullptr));
    CHECK(launches("launch_graph_pair_fill") == 2 && launches("launch_") == n0 + 6);
    CHECK(tvc_workspace_bytes(h) == ws0);                                             // neither graph call owns a workspace

    // ---- tvc_pair_cosine: no handle, no bank, a bank of no rows
    CHECK(tvc_pair_cosine(nullptr, pairs, P, sim, nullptr) == TVC_E_INVALID);
    QUIET_REFUSED(tvc_pair_cosine(h, pairs, P, sim, nullptr), TVC_E_STATE, CO);
    QUIET_REFUSED(tvc_pair_cosine(h, pairs, 0, sim, nullptr), TVC_E_STATE, CO);             // an empty slot refuses before P is looked at
    OK(tvc_bank_set(h, rows32, 0, D, TVC_DTYPE_F32, nullptr));
    QUIET_REFUSED(tvc_pair_cosine(h, pairs, P, sim, nullptr), TVC_E_STATE, CO);
    for (int dtype = 0; dtype < 2; ++dtype) {
        OK(tvc_bank_select(h, dtype));
        OK(tvc_bank_set(h, dtype == 0 ? (const void*)rows32 : (const void*)rows16, R, D, dtype == 0 ? TVC_DTYPE_F32 : TVC_DTYPE_BF16, nullptr));
        const uint64_t ws1 = tvc_workspace_bytes(h);
        QUIET_REFUSED(tvc_pair_cosine(h, pairs, -1, sim, nullptr), TVC_E_INVALID, CO);
        QUIET_REFUSED(tvc_pair_cosine(h, nullptr, P, sim, nullptr), TVC_E_INVALID, CO);
        QUIET_REFUSED(tvc_pair_cosine(h, pairs, P, nullptr, nullptr), TVC_E_INVALID, CO);
        n0 = launches("launch_pair_cosine");
        OK(tvc_pair_cosine(h, pairs, 0, sim, nullptr));
        OK(tvc_pair_cosine(h, nullptr, 0, nullptr, nullptr));
        CHECK(launches("launch_pair_cosine") == n0);
        OK(tvc_pair_cosine(h, pairs, P, sim, nullptr));
        OK(tvc_pair_cosine(h, pairs, 1, sim, nullptr));
        CHECK(launches("launch_pair_cosine") == n0 + 2);
        CHECK(tvc_workspace_bytes(h) == ws1);                                         // the cosine owns no workspace either
    }
    // a released slot refuses again
    OK(tvc_bank_set(h, nullptr, 0, 64, TVC_DTYPE_BF16, nullptr));
    QUIET_REFUSED(tvc_pair_cosine(h, pairs, P, sim, nullptr), TVC_E_STATE, CO);

    // the profiling bracket counts the cosine as bank work: three FMAs per element of a pair
    OK(tvc_bank_select(h, 0));
    double ms[TVC_PROF_NCAT], work[TVC_PROF_NCAT], big[3]; int64_t nl[TVC_PROF_NCAT];
    OK(tvc_profile_begin(h)); OK(tvc_pair_cosine(h, pairs, P, sim, nullptr)); OK(tvc_profile_end(h, ms, work, nl, big));
    CHECK(nl[TVC_PROF_BANK] == 1 && work[TVC_PROF_BANK] == 6.0 * P * D);
    tvc_destroy(h);
    for (void* p : keep) (void)hipFree(p);
    CHECK(hip_stub_blocks().empty());                               // every handle-owned device block was released
    printf("HOST_SAN_PAIRS_OK\n");
    return 0;
}
