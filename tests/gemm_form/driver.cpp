// Host-only driver of the 16-bit GEMM dispatch (tests/test_gemm_form.py): reads one launch per line on stdin --
//   I J K planes lda ldb epilogue splitk_small splitk_fixed has_ws ws_bytes a_rows_padded b_rows_padded
//   TVC_GEMM_VARIANT TVC_GEMM_RING_MIN_TILES TVC_GEMM_RING_FORM TVC_GEMM_SPLITK_TAIL TVC_GEMM_SPLITK_SMALL TVC_GEMM_RING_SPLIT
// -- and prints the form csrc/host_plan.hpp's gemm_form gives it (the one launch_gemm_bf16 takes) and its K split.
// and, for a caller-fixed split, whether its slices run in the ring kernel (1) or in the partial and finish kernels (0).
// With the arguments `bank_plan R M k` it prints bank_plan's cut of that search instead; with `fixed_split I K planes
// rows_per_sample` the K split the latent-diffusion model fixes for that GEMM (csrc/host_plan.hpp's sd_fixed_split).
#include "host_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static const char* form_name(GemmForm f) {
    switch (f) {
        case GEMM_FORM_ONE_TILE: return "ONE_TILE";
        case GEMM_FORM_RING1: return "RING1";
        case GEMM_FORM_RING4: return "RING4";
        case GEMM_FORM_SPLITK_SMALL: return "SPLITK_SMALL";
        case GEMM_FORM_SPLITK_TAIL: return "SPLITK_TAIL";
        case GEMM_FORM_SPLITK_FIXED: return "SPLITK_FIXED";
        case GEMM_FORM_MID_SPLIT: return "MID_SPLIT";
    }
    return "?";
}

// `driver bank_plan R M k`: csrc/host_plan.hpp's bank_plan for that search and what pass 1 (bank.hip) makes of it
static int print_bank_plan(long long R, int M, int k) {
    int n_sample, stride, S, cap;
    bank_plan(R, M, k, &n_sample, &stride, &S, &cap);
    const int nQt = (M + HOST_PLAN_GEMM_BN - 1) / HOST_PLAN_GEMM_BN;
    const int nbt = (int)((R + HOST_PLAN_GEMM_BM - 1) / HOST_PLAN_GEMM_BM);
    printf("n_sample=%d stride=%d S=%d nQt=%d bank_tiles=%d tiles_per_chunk=%d blocked=%d\n", n_sample, stride, S, nQt, nbt,
           (nbt + S - 1) / S, (int)(nQt % 4 == 0 && S % 8 == 0));
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "bank_plan")) return print_bank_plan(atoll(argv[2]), atoi(argv[3]), atoi(argv[4]));
    if (argc == 6 && !strcmp(argv[1], "fixed_split")) {
        printf("%d\n", sd_fixed_split(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoll(argv[5])));
        return 0;
    }
    long long v[19];
    for (;;) {
        for (int i = 0; i < 19; ++i)
            if (scanf("%lld", &v[i]) != 1) return i == 0 ? 0 : 1;
        GemmFormArgs a;
        a.I = (int)v[0]; a.J = (int)v[1]; a.K = (int)v[2]; a.planes = (int)v[3]; a.lda = v[4]; a.ldb = v[5];
        a.epilogue = (int)v[6]; a.splitk_small = v[7] != 0; a.splitk_fixed = (int)v[8]; a.has_ws = v[9] != 0;
        a.ws_bytes = (size_t)v[10]; a.a_rows_padded = v[11] != 0; a.b_rows_padded = v[12] != 0;
        GemmFormEnv e;
        e.variant = (int)v[13]; e.ring_min_tiles = (int)v[14]; e.ring_form = (int)v[15]; e.splitk_tail = v[16] != 0;
        e.splitk_small = v[17] != 0; e.ring_split = v[18] != 0;
        const GemmPlan p = gemm_form(a, e);
        printf("%s %d %d\n", form_name(p.form), p.S, (int)p.ring_split);
    }
}
