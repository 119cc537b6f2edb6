// Host-only sanitizer driver of the FSTA / SMA attack entry points (tests/test_attack_host.py), built by
// tests/host_san_build.py under ASan / UBSan against tests/host_san's HIP stand-in (kernels are no-ops, "device" blocks are exactly
// sized host blocks).  Walks every refusal of tvc_attack_feature_grad / tvc_attack_step (no handle, negative sizes, unknown
// metric / norm, NULL buffers, an output aliasing an input, a bad eps or clamp range), the zero-size no-ops (which take NULL
// buffers), valid calls of both metrics and both norms, and a leak-free tvc_destroy: neither call may allocate.
#include "driver_common.hpp"

#include <cmath>
#include <vector>

int main() {
    tvc_handle* h = nullptr;
    CHECK(tvc_create(nullptr, nullptr, nullptr, &h) == TVC_OK && h);       // a handle without towers: the calls need none
    std::vector<void*> keep;
    auto buf = [&](size_t elems) { float* p = (float*)dev(elems * 4); keep.push_back(p); return p; };
    const int B = 5, D = 100;
    const int64_t n = 3 * 7 * 7;
    float *f = buf(B * D), *t = buf(B * D), *g = buf(B * D), *grad = buf(B * D), *rows = buf(B * 4);
    float *adv = buf(B * n), *clean = buf(B * n), *gp = buf(B * n), *mom = buf(B * n);
    const uint64_t ws0 = tvc_workspace_bytes(h);
    const int COS = TVC_ATTACK_METRIC_COSINE, EUC = TVC_ATTACK_METRIC_EUCLIDEAN, INF = TVC_ATTACK_NORM_INF, L2 = TVC_ATTACK_NORM_L2;
    const char* FG = "tvc_attack_feature_grad";
    const char* ST = "tvc_attack_step";

    // ---- tvc_attack_feature_grad
    CHECK(tvc_attack_feature_grad(nullptr, f, t, g, B, D, -1.f, 1.f, COS, 0.1f, 0.05f, grad, rows, nullptr) == TVC_E_INVALID);
    REFUSED(tvc_attack_feature_grad(h, f, t, g, -1, D, -1.f, 1.f, COS, 0.1f, 0.05f, grad, rows, nullptr), TVC_E_INVALID, FG);
    REFUSED(tvc_attack_feature_grad(h, f, t, g, B, -1, -1.f, 1.f, COS, 0.1f, 0.05f, grad, rows, nullptr), TVC_E_INVALID, FG);
    REFUSED(tvc_attack_feature_grad(h, f, t, g, B, D, -1.f, 1.f, 2, 0.1f, 0.05f, grad, rows, nullptr), TVC_E_INVALID, FG);
    REFUSED(tvc_attack_feature_grad(h, f, t, g, B, D, -1.f, 1.f, -1, 0.1f, 0.05f, grad, rows, nullptr), TVC_E_INVALID, FG);
    REFUSED(tvc_attack_feature_grad(h, f, t, g, 0, D, -1.f, 1.f, 7, 0.1f, 0.05f, grad, rows, nullptr), TVC_E_INVALID, FG);      // also at size 0
    REFUSED(tvc_attack_feature_grad(h, nullptr, t, g, B, D, -1.f, 1.f, COS, 0.1f, 0.05f, grad, rows, nullptr), TVC_E_INVALID, FG);
    REFUSED(tvc_attack_feature_grad(h, f, nullptr, g, B, D, -1.f, 1.f, COS, 0.1f, 0.05f, grad, rows, nullptr), TVC_E_INVALID, FG);
    REFUSED(tvc_attack_feature_grad(h, f, t, nullptr, B, D, -1.f, 1.f, COS, 0.1f, 0.05f, grad, rows, nullptr), TVC_E_INVALID, FG);
    REFUSED(tvc_attack_feature_grad(h, f, t, g, B, D, -1.f, 1.f, COS, 0.1f, 0.05f, nullptr, rows, nullptr), TVC_E_INVALID, FG);
    REFUSED(tvc_attack_feature_grad(h, f, t, g, B, D, -1.f, 1.f, COS, 0.1f, 0.05f, grad, nullptr, nullptr), TVC_E_INVALID, FG);
    REFUSED(tvc_attack_feature_grad(h, f, t, g, B, D, -1.f, 1.f, COS, 0.1f, 0.05f, f, rows, nullptr), TVC_E_INVALID, FG);       // grad aliases f
    REFUSED(tvc_attack_feature_grad(h, f, t, g, B, D, -1.f, 1.f, COS, 0.1f, 0.05f, t, rows, nullptr), TVC_E_INVALID, FG);
    REFUSED(tvc_attack_feature_grad(h, f, t, g, B, D, -1.f, 1.f, EUC, 0.1f, 0.05f, g, rows, nullptr), TVC_E_INVALID, FG);
    OK(tvc_attack_feature_grad(h, nullptr, nullptr, nullptr, 0, D, -1.f, 1.f, COS, 0.1f, 0.05f, nullptr, nullptr, nullptr));   // B = 0
    OK(tvc_attack_feature_grad(h, nullptr, nullptr, nullptr, B, 0, -1.f, 1.f, EUC, 0.1f, 0.05f, nullptr, nullptr, nullptr));   // D = 0
    OK(tvc_attack_feature_grad(h, f, t, g, B, D, -1.f, 1.f, COS, 0.1f, 0.05f, grad, rows, nullptr));
    OK(tvc_attack_feature_grad(h, f, t, g, B, D, -1.f, 1.f, EUC, 0.f, 0.f, grad, rows, nullptr));
    OK(tvc_attack_feature_grad(h, f, t, g, 1, D, -5.f, 5.f, COS, 0.f, 0.1f, grad, rows, nullptr));              // B = 1
    OK(tvc_attack_feature_grad(h, f, f, f, B, D, 0.f, 0.f, COS, 0.f, 0.f, grad, rows, nullptr));                // inputs may alias each other

    // ---- tvc_attack_step
    const float eps = 0.031f, lr = 0.01f, mu = 0.9f;
    CHECK(tvc_attack_step(nullptr, adv, clean, gp, mom, B, n, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, INF, nullptr) == TVC_E_INVALID);
    REFUSED(tvc_attack_step(h, adv, clean, gp, mom, -1, n, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, INF, nullptr), TVC_E_INVALID, ST);
    REFUSED(tvc_attack_step(h, adv, clean, gp, mom, B, -1, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, INF, nullptr), TVC_E_INVALID, ST);
    REFUSED(tvc_attack_step(h, adv, clean, gp, mom, B, n, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, 2, nullptr), TVC_E_INVALID, ST);
    REFUSED(tvc_attack_step(h, adv, clean, gp, mom, B, n, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, -1, nullptr), TVC_E_INVALID, ST);
    REFUSED(tvc_attack_step(h, adv, clean, gp, mom, B, n, -eps, lr, mu, 1.f, 0.f, 0.f, 1.f, INF, nullptr), TVC_E_INVALID, ST);
    REFUSED(tvc_attack_step(h, adv, clean, gp, mom, B, n, NAN, lr, mu, 1.f, 0.f, 0.f, 1.f, L2, nullptr), TVC_E_INVALID, ST);
    REFUSED(tvc_attack_step(h, adv, clean, gp, mom, B, n, eps, lr, mu, 1.f, 0.f, 1.f, 0.f, INF, nullptr), TVC_E_INVALID, ST);   // clip_min > clip_max
    REFUSED(tvc_attack_step(h, adv, clean, gp, mom, B, n, eps, lr, mu, 1.f, 0.f, NAN, 1.f, INF, nullptr), TVC_E_INVALID, ST);
    REFUSED(tvc_attack_step(h, adv, clean, gp, mom, 0, n, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, 9, nullptr), TVC_E_INVALID, ST);     // also at size 0
    REFUSED(tvc_attack_step(h, nullptr, clean, gp, mom, B, n, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, INF, nullptr), TVC_E_INVALID, ST);
    REFUSED(tvc_attack_step(h, adv, nullptr, gp, mom, B, n, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, INF, nullptr), TVC_E_INVALID, ST);
    REFUSED(tvc_attack_step(h, adv, clean, nullptr, mom, B, n, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, L2, nullptr), TVC_E_INVALID, ST);
    REFUSED(tvc_attack_step(h, adv, clean, gp, nullptr, B, n, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, INF, nullptr), TVC_E_INVALID, ST);   // mom is required
    REFUSED(tvc_attack_step(h, adv, clean, gp, nullptr, B, n, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, L2, nullptr), TVC_E_INVALID, ST);
    OK(tvc_attack_step(h, nullptr, nullptr, nullptr, nullptr, 0, n, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, INF, nullptr));  // B = 0
    OK(tvc_attack_step(h, nullptr, nullptr, nullptr, nullptr, B, 0, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, L2, nullptr));   // n = 0
    OK(tvc_attack_step(h, adv, clean, gp, mom, B, n, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, INF, nullptr));
    OK(tvc_attack_step(h, adv, clean, gp, mom, B, n, eps, lr, mu, 0.f, 1e-5f, 0.f, 1.f, L2, nullptr));
    OK(tvc_attack_step(h, adv, clean, gp, mom, B, n, 0.f, lr, mu, -1.f, 0.f, 0.5f, 0.5f, INF, nullptr));         // eps = 0, lo == hi, clip <= 0
    OK(tvc_attack_step(h, adv, clean, gp, mom, 1, (int64_t)B * n, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, L2, nullptr));

    CHECK(tvc_workspace_bytes(h) == ws0);                           // neither call owns a workspace
    // a successful call does not clear the last refusal's message; a refusal replaces it
    REFUSED(tvc_attack_step(h, adv, clean, gp, mom, B, n, eps, lr, mu, 1.f, 0.f, 0.f, 1.f, 5, nullptr), TVC_E_INVALID, ST);
    REFUSED(tvc_attack_feature_grad(h, f, t, g, B, D, -1.f, 1.f, 5, 0.f, 0.f, grad, rows, nullptr), TVC_E_INVALID, FG);
    tvc_destroy(h);
    for (void* p : keep) (void)hipFree(p);
    CHECK(hip_stub_blocks().empty());                               // every handle-owned device block was released
    printf("HOST_SAN_ATTACK_OK\n");
    return 0;
}
