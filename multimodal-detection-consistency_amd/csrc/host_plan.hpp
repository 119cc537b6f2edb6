// Host-side planning arithmetic shared by the launchers (bank.hip, sd_ops.hip) and the C-ABI translation units: pure
// functions of sizes, no HIP.  Kept in a header so that the host-only sanitizer build of the C-ABI (tests/host_san:
// -fsanitize=address,undefined with the kernels stubbed out) runs the SAME arithmetic as the product.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define BANK_CAP 128
#define BANK_KEFF 16       // tau = max(k, 16)-th largest group maximum: a looser but far less noisy bound
#define HOST_PLAN_GEMM_BM 256
#define HOST_PLAN_GEMM_BN 256

inline void bank_plan(int64_t R, int M, int k, int* n_sample, int* sample_stride, int* S, int* cap) {
    const int64_t nbt = (R + HOST_PLAN_GEMM_BM - 1) / HOST_PLAN_GEMM_BM;
    const int nqt = (M + HOST_PLAN_GEMM_BN - 1) / HOST_PLAN_GEMM_BN;
    int64_t s = (1280 + nqt - 1) / nqt;
    if (s > nbt) s = nbt;
    if (s < 1) s = 1;
    const int64_t tpc = (nbt + s - 1) / s;
    s = (nbt + tpc - 1) / tpc;
    // expected survivors per query ~ keff * R / n_sample (relative spread ~ keff^-1/2):
    // aim at 8 per chunk list (cap 128) and at most ~2048 per query (select pool 6144)
    const int keff = k > BANK_KEFF ? k : BANK_KEFF;
    int64_t ns = (int64_t)keff * R / (8 * s);
    // the select pass re-scores every survivor of a query in ONE workgroup (~2 us per 16 rows): ~2 000 survivors cost 0.3-0.5 ms
    // there whatever M is -- more than streaming a 1 M-row bank -- while the sample's GEMM and the tau selection over it grow
    // with M: aim at ~256 survivors per query up to M = 2 048 (round 4; measured at R = 1 M, k = 10, M = 128 / 256 / 1 024 / 2 048:
    // 1.21 / 1.12 / 2.73 / 4.15 -> 0.57 / 0.62 / 1.73 / 3.26 ms; at M = 4 608 the two costs cancel: 6.9 -> 7.3 ms at k = 5)
    const int64_t ns2 = (int64_t)keff * R / (M <= 2048 ? 256 : 2048);
    if (ns < ns2) ns = ns2;
    if (ns < 4096) ns = 4096;
    // cap: the pre-pass similarities [M, ns] fp32 stay under 8 GiB (ns = 262144 at M = 5120 keeps a
    // 10 M-row bank at ~600 survivors per query; the old 65536 cap left ~2800 +- 25 % and overflowed
    // the 128-entry lists / 6144-entry pool for some of 5120 queries)
    int64_t ns_cap = ((int64_t)8 << 30) / ((int64_t)(M > 0 ? M : 1) * 4);
    if (ns_cap > 262144) ns_cap = 262144;
    if (ns_cap < 65536) ns_cap = 65536;
    if (ns > ns_cap) ns = ns_cap;
    ns = (ns + 255) / 256 * 256;
    if (ns > R) ns = R;
    if (ns < 1) ns = 1;
    // when the cap bites, keep the per-(chunk, query) lists short (<= ~24 expected, cap 128) by
    // cutting the bank into more chunks instead
    {
        int64_t s_min = ((int64_t)keff * R + 24 * ns - 1) / (24 * ns);
        if (s_min > nbt) s_min = nbt;
        if (s < s_min) {
            const int64_t tpc2 = (nbt + s_min - 1) / s_min;
            s = (nbt + tpc2 - 1) / tpc2;
        }
    }
    *n_sample = (int)ns;
    *sample_stride = (int)(R / ns > 0 ? R / ns : 1);
    *S = (int)s;
    *cap = BANK_CAP;
}

// k-means update (kmeans.hip): the counting sort cuts the R rows into nblocks runs of rows_per_block rows (a multiple of the
// 256-row chunk of the stable scatter); the [nblocks, K] counter matrix stays under 16 MiB and nblocks under 1 024 (the
// column scan walks the blocks one after the other)
#define KMEANS_MAX_K 65536
inline void kmeans_update_plan(int64_t R, int K, int* nblocks, int* rows_per_block) {
    int64_t nb = ((int64_t)4 << 20) / (K > 0 ? K : 1);
    if (nb > 1024) nb = 1024;
    const int64_t chunks = (R + 255) / 256;
    if (nb > chunks) nb = chunks;
    if (nb < 1) nb = 1;
    const int64_t rpb = ((R + nb - 1) / nb + 255) / 256 * 256;
    *rows_per_block = (int)(rpb > 0 ? rpb : 256);
    *nblocks = (int)((R + *rows_per_block - 1) / *rows_per_block > 0 ? (R + *rows_per_block - 1) / *rows_per_block : 1);
}

// GroupNorm statistics slabs: small slabs = many workgroups (the pass is latency-bound on few), at most 1024 slabs per image
inline int gn_slab_tokens(int HW) { int s = 64; while ((HW + s - 1) / s > 1024) s *= 2; return s; }
// ws: >= n * nslab * groups * 2 + n * groups * 2 floats
inline size_t sd_groupnorm_ws_floats(int n, int HW, int groups) {
    const int slab = gn_slab_tokens(HW);
    const int nslab = (HW + slab - 1) / slab;
    return (size_t)n * nslab * groups * 2 + (size_t)n * groups * 2;
}

// ---- the form of a 16-bit GEMM launch (tvc_gemm_bf16 / tvc_gemm_f16 and every internal caller of launch_gemm_bf16):
// launch_gemm_bf16 (gemm.hip) dispatches on exactly this plan, so a test can name the kernel a shape reaches without a GPU
enum GemmForm {
    GEMM_FORM_ONE_TILE = 0,     // gemm_bf16_kernel: one 256 x 256 tile per workgroup
    GEMM_FORM_RING1,            // gemm_ring_kernel: persistent ring, clamped rows (any shape)
    GEMM_FORM_RING4,            // gemm_ring4_kernel: persistent ring over whole-line K-tiles (whole row tiles, 128-byte pitches)
    GEMM_FORM_SPLITK_SMALL,     // few tiles, deep K: K split over the idle CUs (partial + finish kernels)
    GEMM_FORM_SPLITK_TAIL,      // ring launch of whole rounds + split-K partial / finish kernels for the left-over tile columns
    GEMM_FORM_SPLITK_FIXED,     // the caller fixed the K split (GemmLaunch::splitk_fixed >= 2)
    GEMM_FORM_MID_SPLIT,        // `splitk_small` launches of 64..128 tiles of a deep K: the split-K kernels of SPLITK_SMALL
};

// the env switches gemm.hip reads once per process, as values (the defaults = unset)
struct GemmFormEnv {
    int variant = -1;           // TVC_GEMM_VARIANT: 0 = one tile per workgroup everywhere, >= 1 = the ring from 8 tiles on
    int ring_min_tiles = 8;     // TVC_GEMM_RING_MIN_TILES
    int ring_form = 4;          // TVC_GEMM_RING_FORM: 1 forces ring form 1
    bool splitk_tail = false;   // TVC_GEMM_SPLITK_TAIL
    bool splitk_small = false;  // TVC_GEMM_SPLITK_SMALL
    bool ring_split = true;     // TVC_GEMM_RING_SPLIT
};

// the sizes and flags of a launch that the dispatch reads (a GemmLaunch without its pointers)
struct GemmFormArgs {
    int I = 0, J = 0, K = 0, planes = 1;
    int64_t lda = 0, ldb = 0;
    int epilogue = 0;           // TVC_EPI_*: 3 = the fp32 residual add, which ring form 4 does not carry
    bool splitk_small = false;
    int splitk_fixed = 0;
    bool has_ws = false;        // a split-K workspace was passed
    size_t ws_bytes = 0;
    bool a_rows_padded = false, b_rows_padded = false;
};

struct GemmPlan {
    GemmForm form = GEMM_FORM_ONE_TILE;
    int S = 0;                  // the K split of the split forms
    int jt_full = 0;            // SPLITK_TAIL: tile columns of the ring launch; the rest are split over K
    int left = 0;               // SPLITK_TAIL: tiles of the left-over columns
    bool ring_split = false;    // SPLITK_FIXED: the slices run in the ring kernel (else the one-tile partial loop)
};

inline GemmPlan gemm_form(const GemmFormArgs& a, const GemmFormEnv& env) {
    const int BM = HOST_PLAN_GEMM_BM, BN = HOST_PLAN_GEMM_BN;
    const size_t tile_bytes = (size_t)BM * BN * 4;      // one fp32 partial tile of the split-K workspace
    const int nIt = (a.I + BM - 1) / BM, nJt = (a.J + BN - 1) / BN;
    const int ntiles = nIt * nJt;
    const bool deep = (int64_t)a.K * a.planes >= 256;   // >= 8 ring stages per tile
    const int ring_min = (a.splitk_small && env.ring_min_tiles < 64) ? 64 : env.ring_min_tiles;
    const int nk64 = (int)((int64_t)a.K * a.planes / 64);
    const bool auto_split = a.splitk_fixed == 0;
    const int forced = env.variant;
    GemmPlan p;
    if (a.splitk_fixed >= 2) {
        p.form = GEMM_FORM_SPLITK_FIXED;
        p.S = a.splitk_fixed > nk64 ? nk64 : a.splitk_fixed;
        p.ring_split = env.ring_split && nk64 % p.S == 0 && nk64 / p.S >= 4 && (a.I % BM == 0 || a.a_rows_padded) &&
                       (a.J % BN == 0 || a.b_rows_padded) && a.lda % 64 == 0 && a.ldb % 64 == 0;
        return p;
    }
    const bool mid_split = auto_split && a.splitk_small && a.has_ws && forced < 0 && ntiles >= ring_min && ntiles <= 128 &&
                           nk64 >= 32 && (size_t)ntiles * (256 / ntiles) * tile_bytes <= a.ws_bytes;
    const bool ring = deep && !mid_split && (forced >= 0 ? (forced >= 1 && ntiles >= 8) : (ntiles >= ring_min));
    if (ring) {
        const int full_tiles = ntiles / 256 * 256;
        const int jt_full = full_tiles / nIt;
        const int left = ntiles - jt_full * nIt;
        int S = left > 0 ? 256 / left : 0;
        if (S > nk64 / 4) S = nk64 / 4;
        if (S > 16) S = 16;
        const bool whole_rounds = (jt_full * nIt) % 256 == 0;
        if (auto_split && forced < 0 && a.has_ws && jt_full >= 1 && left >= 1 && S >= 2 &&
            ((env.splitk_tail && whole_rounds && left <= 64) || (a.splitk_small && left <= 128)) &&
            (size_t)left * S * tile_bytes <= a.ws_bytes) {
            p.form = GEMM_FORM_SPLITK_TAIL; p.S = S; p.jt_full = jt_full; p.left = left;
            return p;
        }
        const bool form4 = env.ring_form == 4 && a.epilogue != 3 && (a.I % BM == 0 || a.a_rows_padded) &&
                           (a.J % BN == 0 || a.b_rows_padded) && a.lda % 64 == 0 && a.ldb % 64 == 0;
        p.form = form4 ? GEMM_FORM_RING4 : GEMM_FORM_RING1;
        return p;
    }
    int S = ntiles > 0 ? 256 / ntiles : 0;
    if (S > nk64 / 2) S = nk64 / 2;
    if (S > 16) S = 16;
    if (auto_split && (env.splitk_small || a.splitk_small) && forced < 0 && a.has_ws && S >= 2 &&
        (size_t)ntiles * S * tile_bytes <= a.ws_bytes) {
        p.form = mid_split ? GEMM_FORM_MID_SPLIT : GEMM_FORM_SPLITK_SMALL;
        p.S = S;
    }
    return p;
}
