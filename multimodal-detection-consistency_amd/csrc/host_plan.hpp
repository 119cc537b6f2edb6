// Host-side planning arithmetic shared by the launchers (bank.hip, sd_ops.hip) and the C-ABI translation units: pure
// functions of sizes, no HIP.  Kept in a header so that the host-only sanitizer build of the C-ABI (tests/host_san:
// -fsanitize=address,undefined with the kernels stubbed out) runs the SAME arithmetic as the product.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>

#define BANK_CAP 128
#define BANK_KEFF 16       // tau = max(k, 16)-th largest group maximum: a looser but far less noisy bound
#define HOST_PLAN_GEMM_BM 256
#define HOST_PLAN_GEMM_BN 256

// Workgroups of a wave-per-row grid-stride kernel over `rows` rows (rows.hpp: for_wave_rows): one wave to a row, the four rows
// of launch.hpp's ROWS_PER_BLOCK to a 256-thread workgroup, at most WAVE_STRIDE_MAX_GRID workgroups; the waves loop beyond it.
#define WAVE_STRIDE_MAX_GRID 16384
inline int wave_stride_grid(int64_t rows) {
    const int64_t g = (rows + 3) / 4;
    return (int)(g < WAVE_STRIDE_MAX_GRID ? g : WAVE_STRIDE_MAX_GRID);
}

// the work of one GEMM pass of X rows over R stored rows of D columns with `products` plane products
inline double slot_pass_flops(int64_t R, int64_t X, int D, int products) { return 2.0 * (double)R * (double)X * D * products; }

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

// Retrieval evaluation (rank.hip): the tile kernels read the query labels and the last-target scores as whole 16-byte pieces, so
// both vectors are padded to whole query tiles; the metrics kernel takes at most RANK_MAX_K values of k (include/tvc.h's
// TVC_RANK_MAX_K).  ok = false: M < 1, or more than RANK_MAX_K values, or a k < 1.
#define RANK_MAX_K 8
struct RankPlan {
    bool ok = false;
    int n_qtiles = 0;                   // 256-query tiles
    int64_t mpad = 0;                   // entries of the padded per-query vectors
    double flops = 0;                   // of one tile pass over R rows of D columns with `products` plane products
};
inline RankPlan rank_plan(int64_t M, int64_t R, int D, int products) {
    RankPlan p;
    if (M < 1 || M > 0x7fffffffLL - HOST_PLAN_GEMM_BM) return p;
    p.n_qtiles = (int)((M + HOST_PLAN_GEMM_BM - 1) / HOST_PLAN_GEMM_BM);
    p.mpad = (int64_t)p.n_qtiles * HOST_PLAN_GEMM_BM;
    p.flops = slot_pass_flops(R, M, D, products);
    p.ok = true;
    return p;
}
inline bool rank_k_values_ok(const int32_t* k, int n_k) {
    if (n_k < 0 || n_k > RANK_MAX_K || (n_k > 0 && !k)) return false;
    for (int t = 0; t < n_k; ++t)
        if (k[t] < 1) return false;
    return true;
}

// Detection evaluation (roc.hip): one workgroup of ROC_THREADS threads per row (a weighting of the N samples by integer
// multiplicities).  The row's multiplicities are uint32 counts over the N original indices; up to ROC_LDS_ROWS samples they live
// in LDS -- 144 KiB of the CU's 160 KiB, the other 16 KiB hold the sweep's scratch (ROC_THREADS points of 12 bytes, the waves'
// partials, the final reduction) -- and above it in a row of a global workspace, roc_ws_stride(N) uint32 per row of the call (whole
// 128-byte lines: two rows, whose workgroups may run on two XCDs, never share a cache line).  The rows of a
// call are cut into chunks so that the workspace of a chunk stays under ROC_WS_BUDGET; a row's results do not depend on the
// chunk it runs in.  ROC_MAX_N is include/tvc.h's TVC_ROC_MAX_N, ROC_MAX_THR its TVC_ROC_MAX_THR.
// ok = false: N < 1, B < 1, N over the cap, more than ROC_MAX_THR thresholds or a negative count, a target outside [0, 1] (or NaN).
#define ROC_THREADS 1024
#define ROC_LDS_ROWS 36864
#define ROC_MAX_N (1 << 24)
#define ROC_MAX_THR 8
#define ROC_WS_BUDGET ((int64_t)1 << 30)        // 268 rows of a million samples: such a chunk still covers every CU; 16 rows at the cap
constexpr int64_t roc_ws_stride(int64_t N) { return (N + 31) / 32 * 32; }      // constexpr: the kernel calls it too
struct RocPlan {
    bool ok = false;
    bool lds = false;                   // the storage form: LDS, or a global workspace row
    size_t lds_bytes = 0;               // dynamic LDS of the LDS form: N uint32 rounded up to 16 bytes
    int64_t chunk_rows = 0;             // rows per launch
    int64_t n_chunks = 0;
    int64_t ws_bytes = 0;               // global workspace of one chunk (0 in the LDS form)
};
inline RocPlan roc_plan(int64_t N, int64_t B, int n_thr, double target) {
    RocPlan p;
    if (N < 1 || B < 1 || N > ROC_MAX_N || n_thr < 0 || n_thr > ROC_MAX_THR || !(target >= 0.0 && target <= 1.0)) return p;
    p.lds = N <= ROC_LDS_ROWS;
    if (p.lds) {
        p.lds_bytes = (size_t)((N * 4 + 15) / 16 * 16);
        p.chunk_rows = B;
        p.n_chunks = 1;
    } else {
        int64_t rows = ROC_WS_BUDGET / (roc_ws_stride(N) * 4);      // >= 16: at the cap
        if (rows > B) rows = B;
        p.chunk_rows = rows;
        p.n_chunks = (B + rows - 1) / rows;
        p.ws_bytes = rows * roc_ws_stride(N) * 4;
    }
    p.ok = true;
    return p;
}

// Similarity metrics (sim.hip).  Row form: one workgroup per pair of rows of D <= SIM_MAX_D elements, sim_row_threads(D)
// threads (one wave up to 256 elements, four above: the summation order is a function of D alone), the sort keys of one row
// in LDS (at most SIM_MAX_D uint32 = 16 KiB).  Long form: one pair of n <= SIM_MAX_N elements; workgroup b of the two partial
// kernels owns the elements [b * SIM_FLAT_CHUNK, (b + 1) * SIM_FLAT_CHUNK), so the grid is a function of n alone, and one
// workgroup finishes each pass over the caller's workspace of 8-byte words:
//   [0, SIM_WS_HEAD)                              the totals of pass 1 (what pass 2 reads its means from)
//   [SIM_WS_HEAD + b * SIM_WS_P1, ...)            pass 1's partials of workgroup b: 7 fp64 sums, 4 extremes, 3 int64 rank sums, NaNs
//   [SIM_WS_HEAD + grid * SIM_WS_P1 + b * SIM_WS_P2, ...)   pass 2's partials: the 3 centred fp64 sums
// SIM_MAX_N = 2^20 keeps n (n - 1)^2, the bound of a sum of squared centred doubled ranks, inside int64.
// ok = false: n outside [1, SIM_MAX_N].
#define SIM_MAX_D 4096
#define SIM_MAX_N (1 << 20)
#define SIM_COLS 8
#define SIM_INTS 4
#define SIM_FLAT_CHUNK 4096
#define SIM_FLAT_THREADS 256
#define SIM_WS_HEAD 16
#define SIM_WS_P1 16
#define SIM_WS_P2 4
#define TOPK_OVERLAP_MAX_K 1024
inline int sim_row_threads(int D) { return D <= 256 ? 64 : 256; }
struct SimFlatPlan {
    bool ok = false;
    int grid = 0;                       // workgroups of the two partial kernels
    int pow2 = 0;                       // the smallest power of two >= n: the first step of the rank searches
    int64_t ws_bytes = 0;
};
inline SimFlatPlan sim_flat_plan(int64_t n) {
    SimFlatPlan p;
    if (n < 1 || n > SIM_MAX_N) return p;
    p.grid = (int)((n + SIM_FLAT_CHUNK - 1) / SIM_FLAT_CHUNK);
    p.pow2 = 1;
    while (p.pow2 < n) p.pow2 <<= 1;
    p.ws_bytes = 8 * ((int64_t)SIM_WS_HEAD + (int64_t)p.grid * (SIM_WS_P1 + SIM_WS_P2));
    p.ok = true;
    return p;
}

// Radius graph / DBSCAN (dbscan.hip): the graph of R rows is a bitmask uint32 [R, words], words = round_up(R, 64) / 32 (an even
// count: a wave of the tile kernel stores one 64-bit word per row).  The tile kernel's grid is tiles x tiles 256 x 256 tiles of
// which the upper triangle computes; the half-norm vector is padded to whole tiles (hpad floats, NaN beyond R).  The
// symmetrise pass owns one pair of 32 x 32 bit blocks per half wave: blocks32 row blocks on the grid's y, 8 column blocks per
// 256-thread workgroup on its x.  RADIUS_MAX_ROWS is include/tvc.h's TVC_RADIUS_MAX_ROWS: 2 GiB of bits.
#define RADIUS_MAX_ROWS 131072
struct RadiusPlan {
    bool ok = false;
    int64_t words = 0;                  // uint32 per row of adj
    int tiles = 0;                      // 256-row tiles per side
    int64_t hpad = 0;                   // floats of the padded half-norm vector
    int blocks32 = 0;                   // 32-row blocks per side (= words)
    int sym_grid_x = 0;                 // ceil(blocks32 / 8)
    int64_t adj_bytes = 0;
    double tile_pairs = 0;              // computed tiles: tiles * (tiles + 1) / 2
};
inline RadiusPlan radius_plan(int64_t R) {
    RadiusPlan p;
    if (R < 1 || R > RADIUS_MAX_ROWS) return p;
    p.words = (R + 63) / 64 * 2;
    p.tiles = (int)((R + HOST_PLAN_GEMM_BM - 1) / HOST_PLAN_GEMM_BM);
    p.hpad = (int64_t)p.tiles * HOST_PLAN_GEMM_BM;
    p.blocks32 = (int)p.words;
    p.sym_grid_x = (p.blocks32 + 7) / 8;
    p.adj_bytes = R * p.words * 4;
    p.tile_pairs = 0.5 * p.tiles * (p.tiles + 1.0);
    p.ok = true;
    return p;
}

// Closest pair of a bank slot (nearest.hip): the workgroup of row tile ti walks the partner tiles ti .. tiles - 1, so the pass
// multiplies the radius graph's upper triangle; the 1 / |x| vector is padded to whole tiles (rpad floats, NaN beyond R).
// NEAREST_MAX_ROWS: row ids and rpad stay in int32.  ok = false: R outside [1, NEAREST_MAX_ROWS].
#define NEAREST_MAX_ROWS (0x7fffffffLL - HOST_PLAN_GEMM_BM)
struct NearestPlan {
    bool ok = false;
    int tiles = 0;                      // 256-row tiles = workgroups of the tile kernel
    int64_t rpad = 0;                   // floats of the padded 1 / |x| vector
    double tile_pairs = 0;              // computed tiles: tiles * (tiles + 1) / 2
};
inline NearestPlan nearest_plan(int64_t R) {
    NearestPlan p;
    if (R < 1 || R > NEAREST_MAX_ROWS) return p;
    p.tiles = (int)((R + HOST_PLAN_GEMM_BM - 1) / HOST_PLAN_GEMM_BM);
    p.rpad = (int64_t)p.tiles * HOST_PLAN_GEMM_BM;
    p.tile_pairs = 0.5 * p.tiles * (p.tiles + 1.0);
    p.ok = true;
    return p;
}

// Pair lists of a bitmask graph and the cosine of listed pairs (pairs.hip).  The count and the fill are wave-per-row grid-stride
// kernels (wave_stride_grid: at most PAIRS_MAX_GRID workgroups); the scan of the counts is one workgroup of PAIRS_SCAN_THREADS
// threads that own scan_per consecutive rows each.  The cosine gives PAIR_COS_LANES lanes to a pair, so a workgroup takes
// 256 / PAIR_COS_LANES pairs per trip of its grid-stride loop.
#define PAIRS_MAX_GRID WAVE_STRIDE_MAX_GRID
#define PAIRS_SCAN_THREADS 1024
#define PAIR_COS_LANES 16
struct PairsPlan {
    bool ok = false;
    int words = 0;                      // uint32 per row of adj: radius_plan(R).words
    int row_grid = 0;                   // workgroups of the count and of the fill
    int scan_per = 0;                   // rows per thread of the scan: ceil(R / PAIRS_SCAN_THREADS)
};
inline PairsPlan pairs_plan(int64_t R) {
    PairsPlan p;
    if (R < 1 || R > RADIUS_MAX_ROWS) return p;
    p.words = (int)((R + 63) / 64 * 2);
    p.row_grid = wave_stride_grid(R);
    p.scan_per = (int)((R + PAIRS_SCAN_THREADS - 1) / PAIRS_SCAN_THREADS);
    p.ok = true;
    return p;
}
// workgroups of the cosine over P pairs (0 for P <= 0: nothing to launch)
inline int pair_cosine_grid(int64_t P) {
    if (P <= 0) return 0;
    const int64_t per = 256 / PAIR_COS_LANES;
    const int64_t g = (P + per - 1) / per;
    return (int)(g < 65536 ? g : 65536);
}

// IVF scan (ivf.hip): the scan writes every (query, probe) pair's similarities with the rows of its list into a score buffer
// [pairs, pitch] fp32, pitch = round_up(max_list_rows, 16); the queries are cut into chunks so that the buffer of a chunk
// stays under IVF_SCORE_BUDGET (256 MiB: 4 608 queries x 10 probes x lists of up to 1 450 rows go in one chunk).  A single
// query whose nprobe x pitch floats exceed the budget is refused (ok = false): the scan never truncates.
#define IVF_SCORE_BUDGET ((int64_t)256 << 20)
#define IVF_CHUNK_ROWS 512              // a work item = (list, chunk of <= 512 rows): the split rule for skewed lists
#define IVF_LDS_BYTES (160 * 1024)
#define IVF_MAX_NLIST 65536
#define IVF_MAX_GRID_CHUNKS 1024        // row chunks of a list on the grid's y; a longer list's items loop
#define IVF_SELECT_LDS_FLOATS 32768     // the select pass keeps a query's segments in LDS when nprobe * pitch fits this
#define IVF_PROBE_SIMS_FLOATS ((int64_t)16 << 20)   // the probe's [chunk, nlist] score workspace: 64 MiB
inline bool ivf_scan_covers(int D) { return D == 128 || D == 512 || D == 768; }      // the D of the skinny stream
struct IvfScanPlan {
    bool ok = false;
    int64_t pitch = 0;                  // floats per (query, probe) pair
    int chunk = 0, n_chunks = 0;        // queries per chunk, chunks
    int group = 0;                      // pairs per LDS image: both query planes of `group` queries fit IVF_LDS_BYTES
    int nqt = 0;                        // 16-query tiles per image the kernel is instantiated with: 1, 2 or 4, <= group / 16
    int grid_lists = 0, grid_chunks = 0;// the scan's grid
    int sort_blocks = 0, sort_rows_per_block = 0;    // the counting sort of a full chunk's pairs (kmeans_update_plan)
    size_t scan_lds = 0, select_lds = 0;// dynamic LDS bytes of the two kernels
    int64_t score_bytes = 0;            // of one chunk
};
inline IvfScanPlan ivf_scan_plan(int M, int nprobe, int nlist, int64_t max_list_rows, int D, int bank_planes) {
    IvfScanPlan p;
    if (M < 1 || nprobe < 1 || nprobe > 128 || nlist < 1 || nlist > IVF_MAX_NLIST || max_list_rows < 1 ||
        max_list_rows > 0x7fffffffLL || !ivf_scan_covers(D) || bank_planes < 1 || bank_planes > 2)
        return p;
    p.pitch = (max_list_rows + 15) / 16 * 16;
    const int64_t per_query = (int64_t)nprobe * p.pitch * 4;
    if (per_query > IVF_SCORE_BUDGET) return p;
    int64_t mc = IVF_SCORE_BUDGET / per_query;
    if (mc > M) mc = M;
    p.chunk = (int)mc;
    p.n_chunks = (int)(((int64_t)M + mc - 1) / mc);
    p.score_bytes = mc * per_query;
    const int qpitch = 4 * D + 16;      // both planes of a query row + the 16 bytes that keep the fragment reads conflict-free
    p.group = 64;
    while (p.group > 16 && p.group * qpitch > IVF_LDS_BYTES) p.group /= 2;
    // a list is read by at most one pair per query of the chunk
    const int need = (int)((mc + 15) / 16);
    p.nqt = need >= 3 ? 4 : need;
    if (p.nqt > p.group / 16) p.nqt = p.group / 16;
    p.scan_lds = (size_t)p.nqt * 16 * qpitch;
    p.grid_lists = nlist;
    int64_t gc = (max_list_rows + IVF_CHUNK_ROWS - 1) / IVF_CHUNK_ROWS;
    if (gc > IVF_MAX_GRID_CHUNKS) gc = IVF_MAX_GRID_CHUNKS;
    p.grid_chunks = (int)gc;
    kmeans_update_plan(mc * nprobe, nlist, &p.sort_blocks, &p.sort_rows_per_block);
    p.select_lds = (int64_t)nprobe * p.pitch <= IVF_SELECT_LDS_FLOATS ? (size_t)nprobe * p.pitch * 4 : 0;
    p.ok = true;
    return p;
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

// ---- K split of a latent-diffusion GEMM (tvc_sd.cpp: Run::fixed_split -> GemmLaunch::splitk_fixed; here so that
// tests/gemm_form/driver.cpp evaluates the same arithmetic on the host), chosen
// from the PER-SAMPLE shape only (never from the launch size): every sample's arithmetic is then the same whatever batch it is generated in, so an image is bit-for-bit independent of its batch mates and of the
// chunking of tvc_sd_generate (the reference's seed policy, src/sd_ref.py:389-412, promises reproducible references).
// Nominal batch: 24 samples (12 images x classifier-free guidance, the batch bench.py generates) -- K is split only
// where even that batch leaves most CUs without a tile (the 8 x 8 level, the time / text projections).  A split that
// filled the chip for a single image (S = 4 .. 16 at the 16 x 16 level) cost the 12-image batch 20 % of its GEMM time
// (r04_bench1: 602 against 497 ms) -- throughput of the batched generator is what configs[4] measures; one image alone
// runs its low-resolution levels on fewer workgroups than CUs.
#ifndef TVC_SD_NOMINAL
#define TVC_SD_NOMINAL 24
#endif
inline int sd_fixed_split(int I, int K, int planes, int64_t rows_per_sample, int nominal_samples = TVC_SD_NOMINAL) {
    const int64_t tiles0 = (int64_t)((I + 255) / 256) * ((nominal_samples * rows_per_sample + 255) / 256);
    const int nk64 = (int)((int64_t)K * planes / 64);
    int64_t S = tiles0 > 0 ? 256 / tiles0 : 1;
    if (S > nk64 / 4) S = nk64 / 4;
    if (S > 16) S = 16;
    // the split kernels run the one-tile loop at about half the ring kernel's rate: a two-way split of a shallow K
    // (the 16 x 16 level's linear layers: 120 tiles x 20 K-tiles) loses to 120 ring workgroups (measured 418 against
    // ~550 TFLOP/s); it pays from three ways on, or on a deep K (>= 32 K-tiles per slice)
    if (S == 2 && nk64 / 2 < 32) S = 1;
    // slices of equal depth (S divides the K-tile count) run in the ring kernel (gemm.hip, gemm_ring4_split_kernel)
    while (S > 2 && nk64 % S != 0) --S;
    if (S == 2 && (nk64 % 2 != 0 || nk64 / 2 < 32)) S = 1;
    return S >= 2 ? (int)S : 1;
}

// GEMM operand rows: readable to the next multiple of 256 plus one tile (gemm.hip's ring forms stage whole tiles and prefetch one)
inline int64_t tile_rows(int64_t r) { return (r + 255) / 256 * 256 + 256; }

// ---- what the split-bf16 input gradient keeps between its forward and its backward (tvc_grad_split.cpp), in ONE block of
// fp32: per layer the layer's input rows, QKV rows, out-projection output and FC1 pre-activation -- 4 * rows * (5 * width + mlp)
// bytes a layer, 7.3 GB at ViT-L/14 and 32 images --, then the ln_post input [B, width] and the un-normalised embedding
// [B, embed_dim].  Offsets in floats.  ok = false: an extent is not positive or a size does not fit size_t.
struct GradSplitKeepPlan {
    bool ok = false;
    size_t rows = 0;
    size_t x_off = 0, qkv_off = 0, d1_off = 0, u_off = 0, xl_off = 0, emb_off = 0;
    size_t per_layer_bytes = 0, total_bytes = 0;
};
inline GradSplitKeepPlan grad_split_keep_plan(int64_t B, int64_t T, int64_t width, int64_t mlp, int64_t layers, int64_t embed_dim) {
    GradSplitKeepPlan p;
    if (B < 1 || T < 1 || width < 1 || mlp < 1 || layers < 1 || embed_dim < 1) return p;
    size_t rows, per_row, per_layer, all_layers, head, total, bytes;
    if (__builtin_mul_overflow((size_t)B, (size_t)T, &rows)) return p;
    if (__builtin_mul_overflow((size_t)5, (size_t)width, &per_row) || __builtin_add_overflow(per_row, (size_t)mlp, &per_row)) return p;
    if (__builtin_mul_overflow(rows, per_row, &per_layer) || __builtin_mul_overflow(per_layer, (size_t)layers, &all_layers)) return p;
    if (__builtin_add_overflow((size_t)width, (size_t)embed_dim, &head) || __builtin_mul_overflow(head, (size_t)B, &head)) return p;
    if (__builtin_add_overflow(all_layers, head, &total) || __builtin_mul_overflow(total, (size_t)4, &bytes)) return p;
    const size_t lr = (size_t)layers * rows;       // <= all_layers: no overflow below
    p.rows = rows;
    p.x_off = 0;
    p.qkv_off = lr * (size_t)width;
    p.d1_off = p.qkv_off + lr * 3 * (size_t)width;
    p.u_off = p.d1_off + lr * (size_t)width;
    p.xl_off = all_layers;
    p.emb_off = all_layers + (size_t)B * (size_t)width;
    p.per_layer_bytes = per_layer * 4;
    p.total_bytes = bytes;
    p.ok = true;
    return p;
}

// ---- the latent-diffusion sampler's scheduler (tvc_sd.cpp): PNDMScheduler with skip_prk_steps (PLMS), scalar fp32.
// The scaled-linear schedule: betas = linspace(sqrt(b0), sqrt(b1), T)^2, out[i] = alphas_cumprod[i] = prod_{j <= i} (1 - beta_j)
inline void sd_alphas_cumprod(float beta_start, float beta_end, int T, float* out) {
    const float s0 = sqrtf(beta_start), s1 = sqrtf(beta_end);
    const float step = (s1 - s0) / (float)(T - 1);
    float prod = 1.0f;
    for (int i = 0; i < T; ++i) {
        const float r = i < T / 2 ? s0 + step * (float)i : s1 - step * (float)(T - 1 - i);
        prod *= 1.0f - r * r;
        out[i] = prod;
    }
}
// One UNet evaluation of the sampling loop and the update that follows it:
//   latents = cs * sample - ce * sum_k w[k] * e(age[k]),  sample = latents, or `cur` (the latents saved one evaluation earlier)
// e(a >= 0) = the a-th newest noise estimate of the 4-entry history ring, counted AFTER this evaluation's own estimate was
// appended (`append`); e(-1) = this evaluation's estimate where it is not appended (the 2nd evaluation: the ring keeps the 1st)
struct SdPlmsStep {
    int t = 0;                       // timestep the UNet is evaluated at
    bool append = true;
    int cur = 0;                     // 1: the latents are saved to `cur` before the update; 2: `cur` is the update's sample
    int n = 0;                       // terms of the sum
    int age[4] = {0, 0, 0, 0};
    float w[4] = {0.f, 0.f, 0.f, 0.f}, cs = 0.f, ce = 0.f;
};
// steps + 1 evaluations (PNDMScheduler.set_timesteps visits the second-to-last timestep twice), 2 <= steps <= T;
// prediction_type 1 = v-prediction; table = sd_alphas_cumprod's [T]
inline std::vector<SdPlmsStep> sd_plms_plan(const float* table, int T, int steps, int steps_offset, int prediction_type) {
    static const float AB[4][4] = {{1.f}, {1.5f, -0.5f}, {23.f / 12.f, -16.f / 12.f, 5.f / 12.f},
                                   {55.f / 24.f, -59.f / 24.f, 37.f / 24.f, -9.f / 24.f}};      // Adams-Bashforth, newest first
    const int ratio = T / steps;
    auto acp = [&](int t) { return t >= 0 ? table[t < T ? t : T - 1] : table[0]; };
    std::vector<SdPlmsStep> plan(steps + 1);
    int n_ets = 0;
    for (int i = 0; i <= steps; ++i) {
        SdPlmsStep& p = plan[i];
        p.t = (i < 2 ? steps - 1 - i : steps - i) * ratio + steps_offset;      // descending, the second one twice
        int prev_t = p.t - ratio, tt = p.t;
        if (i != 1) {
            if (n_ets < 4) ++n_ets;
            p.n = n_ets;
            for (int k = 0; k < n_ets; ++k) { p.age[k] = k; p.w[k] = AB[n_ets - 1][k]; }
            p.cur = i == 0 ? 1 : 0;
        } else {                     // the corrector of the first step: the mean of both estimates, from the saved sample
            p.append = false; p.cur = 2;
            prev_t = p.t; tt = p.t + ratio;
            p.n = 2; p.age[0] = -1; p.w[0] = 0.5f; p.age[1] = 0; p.w[1] = 0.5f;
        }
        const float a_t = acp(tt), a_prev = acp(prev_t);
        const float b_t = 1.f - a_t, b_prev = 1.f - a_prev;
        p.cs = sqrtf(a_prev / a_t);
        const float denom = a_t * sqrtf(b_prev) + sqrtf(a_t * b_t * a_prev);
        p.ce = (a_prev - a_t) / denom;
        if (prediction_type == 1) {
            // v-prediction (PNDMScheduler._get_prev_sample): the combined model output E stands for
            // sqrt(a_t) E + sqrt(b_t) sample -- folded into the two coefficients of prev = cs * sample - ce * E
            p.cs -= p.ce * sqrtf(b_t);
            p.ce *= sqrtf(a_t);
        }
    }
    return plan;
}
