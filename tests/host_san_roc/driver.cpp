// Host-only sanitizer driver of the detection-evaluation entry points (tests/test_detection_host.py), built by
// tests/host_san_build.py under ASan / UBSan against tests/host_san's HIP stand-in (kernels are no-ops, "device" blocks are exactly sized
// host blocks).  Checks the plan of host_plan.hpp (storage form, chunking, refusals), walks every refusal of tvc_roc_weights /
// tvc_roc_sweep / tvc_roc_curve and checks that none allocates, then valid calls in the LDS form (no workspace) and in the global
// form (a workspace that grows with N and never passes the budget), and a leak-free tvc_destroy.
#include "driver_common.hpp"
#include "host_plan.hpp"

#include <cmath>
#include <vector>

int main() {
    // ---- the plan: refusals
    CHECK(!roc_plan(0, 1, 0, 0.95).ok && !roc_plan(-3, 1, 0, 0.95).ok && !roc_plan(10, 0, 0, 0.95).ok && !roc_plan(10, -1, 0, 0.95).ok);
    CHECK(!roc_plan((int64_t)ROC_MAX_N + 1, 1, 0, 0.95).ok && roc_plan(ROC_MAX_N, 1, 0, 0.95).ok);
    CHECK(!roc_plan(10, 1, ROC_MAX_THR + 1, 0.95).ok && !roc_plan(10, 1, -1, 0.95).ok && roc_plan(10, 1, ROC_MAX_THR, 0.95).ok);
    CHECK(!roc_plan(10, 1, 0, -0.01).ok && !roc_plan(10, 1, 0, 1.01).ok && !roc_plan(10, 1, 0, NAN).ok);
    CHECK(roc_plan(10, 1, 0, 0.0).ok && roc_plan(10, 1, 0, 1.0).ok);
    // ---- the plan: the storage form and the chunks
    const RocPlan a = roc_plan(1, 5, 0, 0.95), b = roc_plan(ROC_LDS_ROWS, 1000, 8, 0.5), c = roc_plan(ROC_LDS_ROWS + 1, 17, 0, 0.95);
    CHECK(a.lds && a.lds_bytes == 16 && a.n_chunks == 1 && a.chunk_rows == 5 && a.ws_bytes == 0);
    CHECK(b.lds && b.lds_bytes == (size_t)ROC_LDS_ROWS * 4 && b.n_chunks == 1 && b.chunk_rows == 1000 && b.ws_bytes == 0);
    CHECK(b.lds_bytes + 16 * 1024 <= 160 * 1024);                          // the counts and the sweep's scratch share a CU's LDS
    CHECK(!c.lds && c.lds_bytes == 0 && c.n_chunks == 1 && c.chunk_rows == 17 && c.ws_bytes == (int64_t)17 * roc_ws_stride(ROC_LDS_ROWS + 1) * 4);
    CHECK(roc_ws_stride(1) == 32 && roc_ws_stride(32) == 32 && roc_ws_stride(33) == 64 && roc_ws_stride(ROC_LDS_ROWS + 1) == ROC_LDS_ROWS + 32);
    const RocPlan d = roc_plan(1 << 24, 17, 0, 0.95), e = roc_plan(ROC_MAX_N, 1000, 0, 0.95), f = roc_plan(100000, 5000, 0, 0.95);
    CHECK(!d.lds && d.chunk_rows == 16 && d.n_chunks == 2 && d.ws_bytes == ROC_WS_BUDGET);
    CHECK(e.chunk_rows == 16 && e.n_chunks == 63 && e.ws_bytes == ROC_WS_BUDGET);
    CHECK(f.chunk_rows == 2684 && f.n_chunks == 2 && f.ws_bytes <= ROC_WS_BUDGET && (f.chunk_rows + 1) * 100000 * 4 > ROC_WS_BUDGET);

    tvc_handle* h = nullptr;
    CHECK(tvc_create(nullptr, nullptr, nullptr, &h) == TVC_OK && h);       // a handle without towers: these calls need none
    std::vector<void*> keep;
    auto buf = [&](size_t elems, size_t es) { void* p = dev(elems * es); keep.push_back(p); return p; };
    const int Nbig = ROC_LDS_ROWS + 1000, B = 5;
    float* scores = (float*)buf(Nbig, 4);
    uint8_t* labels = (uint8_t*)buf(Nbig, 1);
    int32_t* order = (int32_t*)buf(Nbig, 4);
    int32_t* src = (int32_t*)buf((size_t)B * Nbig, 4);
    int32_t* w = (int32_t*)buf((size_t)B * Nbig, 4);
    int32_t* pts[4];
    for (auto& p : pts) p = (int32_t*)buf(Nbig, 4);
    int32_t* count = (int32_t*)buf(2, 4);
    void* o[17];
    for (int i = 0; i < 17; ++i) o[i] = buf((size_t)B * 8, 8);
    const tvc_roc_out out{(int32_t*)o[0], (int32_t*)o[1], (int32_t*)o[2], (int32_t*)o[3], (int32_t*)o[4], (int64_t*)o[5],
                          (double*)o[6], (double*)o[7], (double*)o[8], (int32_t*)o[9], (int32_t*)o[10], (int32_t*)o[11],
                          (int32_t*)o[12], (int32_t*)o[13], (int32_t*)o[14], (int32_t*)o[15], (int32_t*)o[16]};
    const float thr[9] = {0.f, 1.f, 2.f, 3.f, 4.f, 5.f, 6.f, 7.f, 8.f};
    auto rows = [&](int N, int source, const int32_t* s, int64_t nb, int64_t first = 0) {
        return tvc_roc_rows{scores, labels, order, N, source, s, nb, first, 42u};
    };
    const uint64_t ws0 = tvc_workspace_bytes(h);
    tvc_roc_rows r = rows(1000, TVC_ROC_SRC_PHILOX, nullptr, B);

    // ---- refusals: none allocates, each leaves a message
    CHECK(tvc_roc_weights(nullptr, &r, w, nullptr) == TVC_E_INVALID && tvc_roc_sweep(nullptr, &r, 0.95, thr, 2, &out, nullptr) == TVC_E_INVALID);
    CHECK(tvc_roc_curve(nullptr, &r, pts[0], pts[1], pts[2], pts[3], count, nullptr) == TVC_E_INVALID);
    CHECK(tvc_roc_weights(h, nullptr, w, nullptr) == TVC_E_INVALID && strlen(tvc_last_error(h)) > 0);
    CHECK(tvc_roc_weights(h, &r, nullptr, nullptr) == TVC_E_INVALID);
    auto refused = [&](tvc_roc_rows bad) {
        return tvc_roc_weights(h, &bad, w, nullptr) == TVC_E_INVALID && tvc_roc_sweep(h, &bad, 0.95, thr, 2, &out, nullptr) == TVC_E_INVALID &&
               tvc_roc_curve(h, &bad, pts[0], pts[1], pts[2], pts[3], count, nullptr) == TVC_E_INVALID && strlen(tvc_last_error(h)) > 0;
    };
    CHECK(refused(rows(0, TVC_ROC_SRC_PHILOX, nullptr, 1)) && refused(rows(-1, TVC_ROC_SRC_PHILOX, nullptr, 1)));
    CHECK(refused(rows(1000, TVC_ROC_SRC_PHILOX, nullptr, 0)) && refused(rows(1000, 3, nullptr, 1)) && refused(rows(1000, -1, nullptr, 1)));
    CHECK(refused(rows(1000, TVC_ROC_SRC_INDICES, nullptr, 1)) && refused(rows(1000, TVC_ROC_SRC_PHILOX, nullptr, 1, -1)));
    CHECK(refused(rows(1000, TVC_ROC_SRC_PHILOX, nullptr, 2, 0xffffffffLL)));
    {
        tvc_roc_rows bad = r;
        bad.scores_dev = nullptr; CHECK(refused(bad));
        bad = r; bad.labels_dev = nullptr; CHECK(refused(bad));
        bad = r; bad.order_dev = nullptr; CHECK(refused(bad));
        bad = r; bad.N = TVC_ROC_MAX_N; bad.N += 1; CHECK(refused(bad));
    }
    CHECK(tvc_roc_sweep(h, &r, 0.95, thr, 9, &out, nullptr) == TVC_E_INVALID && tvc_roc_sweep(h, &r, 0.95, thr, -1, &out, nullptr) == TVC_E_INVALID);
    CHECK(tvc_roc_sweep(h, &r, 0.95, nullptr, 2, &out, nullptr) == TVC_E_INVALID && tvc_roc_sweep(h, &r, 0.95, thr, 2, nullptr, nullptr) == TVC_E_INVALID);
    CHECK(tvc_roc_sweep(h, &r, 1.5, thr, 2, &out, nullptr) == TVC_E_INVALID && tvc_roc_sweep(h, &r, -0.5, thr, 2, &out, nullptr) == TVC_E_INVALID);
    CHECK(tvc_roc_sweep(h, &r, NAN, thr, 2, &out, nullptr) == TVC_E_INVALID);
    for (int i = 0; i < 17; ++i) {                                          // every output array is required (thr_* with thresholds)
        void* q[17];
        memcpy(q, o, sizeof q);
        q[i] = nullptr;
        const tvc_roc_out bad{(int32_t*)q[0], (int32_t*)q[1], (int32_t*)q[2], (int32_t*)q[3], (int32_t*)q[4], (int64_t*)q[5],
                              (double*)q[6], (double*)q[7], (double*)q[8], (int32_t*)q[9], (int32_t*)q[10], (int32_t*)q[11],
                              (int32_t*)q[12], (int32_t*)q[13], (int32_t*)q[14], (int32_t*)q[15], (int32_t*)q[16]};
        CHECK(tvc_roc_sweep(h, &r, 0.95, thr, 2, &bad, nullptr) == TVC_E_INVALID);
        if (i >= 15) CHECK(tvc_roc_sweep(h, &r, 0.95, nullptr, 0, &bad, nullptr) == TVC_OK);
    }
    CHECK(tvc_roc_curve(h, &r, pts[0], pts[1], pts[2], pts[3], count, nullptr) == TVC_E_INVALID);       // B = 5
    r.B = 1;
    CHECK(tvc_roc_curve(h, &r, nullptr, pts[1], pts[2], pts[3], count, nullptr) == TVC_E_INVALID);
    CHECK(tvc_roc_curve(h, &r, pts[0], nullptr, pts[2], pts[3], count, nullptr) == TVC_E_INVALID);
    CHECK(tvc_roc_curve(h, &r, pts[0], pts[1], nullptr, pts[3], count, nullptr) == TVC_E_INVALID);
    CHECK(tvc_roc_curve(h, &r, pts[0], pts[1], pts[2], nullptr, count, nullptr) == TVC_E_INVALID);
    CHECK(tvc_roc_curve(h, &r, pts[0], pts[1], pts[2], pts[3], nullptr, nullptr) == TVC_E_INVALID);
    CHECK(tvc_workspace_bytes(h) == ws0);

    // ---- valid calls in the LDS form: every source, no workspace
    for (int N : {1, 2, 1000, ROC_LDS_ROWS}) {
        for (int source = 0; source < 3; ++source) {
            tvc_roc_rows v = rows(N, source, source == TVC_ROC_SRC_PHILOX ? nullptr : src, B, 7);
            OK(tvc_roc_weights(h, &v, w, nullptr));
            OK(tvc_roc_sweep(h, &v, 0.95, thr, 8, &out, nullptr));
            OK(tvc_roc_sweep(h, &v, 0.0, nullptr, 0, &out, nullptr));
            v.B = 1;
            OK(tvc_roc_curve(h, &v, pts[0], pts[1], pts[2], pts[3], count, nullptr));
        }
        tvc_roc_rows ones = rows(N, TVC_ROC_SRC_WEIGHTS, nullptr, 1);
        OK(tvc_roc_sweep(h, &ones, 1.0, thr, 1, &out, nullptr));
    }
    CHECK(tvc_workspace_bytes(h) == ws0);
    // ---- the global form: the workspace holds the chunk's rows and grows with N
    tvc_roc_rows g1 = rows(ROC_LDS_ROWS + 1, TVC_ROC_SRC_INDICES, src, 2);
    OK(tvc_roc_sweep(h, &g1, 0.95, thr, 3, &out, nullptr));
    const uint64_t ws1 = tvc_workspace_bytes(h);
    CHECK(ws1 >= ws0 + (uint64_t)2 * (ROC_LDS_ROWS + 1) * 4);
    tvc_roc_rows g2 = rows(Nbig, TVC_ROC_SRC_PHILOX, nullptr, B);
    OK(tvc_roc_weights(h, &g2, w, nullptr));
    CHECK(tvc_workspace_bytes(h) >= ws0 + (uint64_t)B * Nbig * 4 && tvc_workspace_bytes(h) > ws1);
    g2.B = 1;
    OK(tvc_roc_curve(h, &g2, pts[0], pts[1], pts[2], pts[3], count, nullptr));
    OK(tvc_roc_sweep(h, &g1, 0.95, thr, 3, &out, nullptr));                 // back to the smaller call: the block stays
    tvc_destroy(h);
    for (void* p : keep) (void)hipFree(p);
    CHECK(hip_stub_blocks().empty());                               // every handle-owned device block was released
    printf("HOST_SAN_ROC_OK\n");
    return 0;
}
