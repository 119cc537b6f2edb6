// Stand-alone check of grad_split_keep_plan (csrc/host_plan.hpp) under g++ -fsanitize=undefined
// (tests/test_grad_split_host.py): prints one line per (B, geometry) -- B T width mlp layers D ok rows x qkv d1 u xl emb
// per_layer_bytes total_bytes -- which the test compares with its own arithmetic, then walks sizes that do not fit size_t or are
// not positive: each must come back refused (ok = 0), with no signed or unsigned overflow on the way.
#include "host_plan.hpp"

#include <cstdio>

int main() {
    struct G { int T, width, mlp, layers, D; };
    const G geos[] = {{17, 256, 512, 2, 128}, {50, 768, 3072, 12, 512}, {257, 1024, 4096, 24, 768}};
    for (const G& g : geos)
        for (int64_t B : {1, 32, 512}) {
            const GradSplitKeepPlan p = grad_split_keep_plan(B, g.T, g.width, g.mlp, g.layers, g.D);
            printf("%lld %d %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", (long long)B, g.T, g.width, g.mlp, g.layers, g.D, (int)p.ok,
                   p.rows, p.x_off, p.qkv_off, p.d1_off, p.u_off, p.xl_off, p.emb_off, p.per_layer_bytes, p.total_bytes);
        }
    int refused = 0, cases = 0;
    auto no = [&](int64_t B, int64_t T, int64_t w, int64_t mlp, int64_t L, int64_t D) {
        ++cases;
        refused += grad_split_keep_plan(B, T, w, mlp, L, D).ok ? 0 : 1;
    };
    const int64_t big = INT64_MAX;
    no(big, 257, 1024, 4096, 24, 768);
    no((int64_t)1 << 62, 4, 1024, 4096, 24, 768);       // B * T wraps
    no((int64_t)1 << 50, 257, 1024, 4096, 24, 768);     // rows * per_row wraps
    no((int64_t)1 << 40, 257, 1024, 4096, 1 << 20, 768);// ... * layers wraps
    no((int64_t)1 << 41, 257, 1024, 4096, 1, 768);      // 2^62.2 floats: only the final * 4 wraps
    no(32, 257, big, 4096, 24, 768);
    no(32, 257, 1024, big, 24, 768);
    no(32, 257, 1024, 4096, 24, big);
    no(0, 257, 1024, 4096, 24, 768);
    no(-1, 257, 1024, 4096, 24, 768);
    no(32, 0, 1024, 4096, 24, 768);
    no(32, 257, 0, 4096, 24, 768);
    no(32, 257, 1024, -5, 24, 768);
    no(32, 257, 1024, 4096, 0, 768);
    no(32, 257, 1024, 4096, 24, 0);
    printf("refused %d of %d\n", refused, cases);
    return refused == cases ? 0 : 1;
}
