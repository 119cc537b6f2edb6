// Host-side launch interface of the TVC HIP kernels (internal; the public
// boundary is include/tvc.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "host_plan.hpp"

// The stored rows of a bank slot: R rows of `planes` D-wide bf16 planes side by side at row pitch ld (elements); planes 1 = a
// bf16 bank, 2 = the (hi | lo) split of an fp32 bank.  What every launch over a bank slot reads (handle.hpp: bank_rows).
struct BankRows {
    const uint16_t* p = nullptr;
    int64_t ld = 0;
    int64_t R = 0;
    int D = 0;
    int planes = 1;
};
// what every GEMM-tile pass over a slot needs of it (slot_operands, gemm_core.hpp): 1 .. max_rows rows of whole 64-column K-tiles
inline bool slot_tile_ok(const BankRows& b, int64_t max_rows) {
    return b.R >= 1 && b.R <= max_rows && b.D >= 64 && b.D % 64 == 0 && b.planes >= 1 && b.planes <= 2;
}

enum { TVC_EPI_F32 = 0, TVC_EPI_BF16 = 1, TVC_EPI_GELU_BF16 = 2, TVC_EPI_RESID_F32 = 3 };

struct GemmLaunch {
    const uint16_t* A = nullptr;   // [I, lda] bf16  (weights / bank rows)
    const uint16_t* B = nullptr;   // [J, ldb] bf16  (tokens / query rows)
    int64_t lda = 0, ldb = 0;
    int I = 0, J = 0, K = 0;       // K per plane, multiple of 64
    int planes = 1;
    int a_plane_off[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};     // up to GEMM_MAX_PLANES
    int b_plane_off[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool splitk_small = false;     // launches of fewer tiles than CUs may split K over the idle CUs (needs splitk_ws; the fp32 sums are
                                   // then taken in a different order than in the one-pass kernels)
    int splitk_fixed = 0;          // 0: the launch decides (above).  1: never split.  S >= 2: split K exactly S ways for EVERY tile
                                   // (needs splitk_ws of tiles * S * 256 KiB) -- callers that promise results independent of the
                                   // launch size (the latent-diffusion model: an image must not depend on its batch mates) pick S
                                   // from the per-sample shape, never from J
    bool a_rows_padded = false;    // A has readable rows up to the next multiple of 256 beyond I (form 4 with a ragged last row tile)
    const float* bias = nullptr;   // [I]
    void* out = nullptr;           // [J, ldo]
    int64_t ldo = 0;
    int epilogue = TVC_EPI_F32;
    bool b_rows_padded = false;    // B has readable (garbage) rows up to the next multiple of 256 beyond J
    // optional scratch for the split-K tail (see launch_gemm_bf16); nullptr disables it
    float* splitk_ws = nullptr;
    size_t splitk_ws_bytes = 0;
    bool f16 = false;              // A, B are IEEE fp16 (v_mfma_f32_16x16x32_f16) and the 16-bit epilogues store fp16 (tower mode 3)
};
hipError_t launch_gemm_bf16(const GemmLaunch& L, hipStream_t stream);
// the plain one-plane product out[J, ldo] = epilogue(B[J, ldb] * A[I, lda]^T + bias); callers set the odd flags afterwards
inline GemmLaunch gemm_launch(const uint16_t* A, int64_t lda, int I, const uint16_t* B, int64_t ldb, int J, int K,
                              const float* bias, void* out, int64_t ldo, int epilogue) {
    GemmLaunch g;
    g.A = A; g.lda = lda; g.I = I; g.B = B; g.ldb = ldb; g.J = J; g.K = K;
    g.bias = bias; g.out = out; g.ldo = ldo; g.epilogue = epilogue;
    return g;
}
// the bank's (hi | lo) plane products, fp32 out: rows of A and B hold D-wide planes side by side, B always (hi | lo).
// bank_planes 1: hi * hi + hi * lo; 2: + lo * hi from A's second plane (the lo * lo term is below fp32)
inline GemmLaunch gemm_launch_planes(const uint16_t* A, int64_t lda, int I, int bank_planes, const uint16_t* B, int J, int D,
                                     float* out, int64_t ldo) {
    GemmLaunch g = gemm_launch(A, lda, I, B, 2 * (int64_t)D, J, D, nullptr, out, ldo, TVC_EPI_F32);
    g.planes = bank_planes == 2 ? 3 : 2;
    g.b_plane_off[1] = D;
    g.a_plane_off[2] = D;
    return g;
}
// what gemm_form() reads of a launch
inline GemmFormArgs form_args(const GemmLaunch& L) {
    GemmFormArgs a;
    a.I = L.I; a.J = L.J; a.K = L.K; a.planes = L.planes; a.lda = L.lda; a.ldb = L.ldb; a.epilogue = L.epilogue;
    a.splitk_small = L.splitk_small; a.splitk_fixed = L.splitk_fixed; a.has_ws = L.splitk_ws != nullptr;
    a.ws_bytes = L.splitk_ws_bytes; a.a_rows_padded = L.a_rows_padded; a.b_rows_padded = L.b_rows_padded;
    return a;
}

// ---- elementwise.hip
// y = LN(x [+ delta [+ delta2]]); with a delta and write_x the sum is written back to x (residual stream)
// delta_compact: the delta rows are [rows, d] in OUTPUT row order (a pooled last layer) instead of x's row layout
hipError_t launch_layernorm(float* x, int64_t x_row_stride, const int32_t* row_idx, const uint16_t* delta,
                            int write_x, const float* g, const float* b, uint16_t* y, int rows, int d,
                            hipStream_t stream, const uint16_t* delta2 = nullptr, int delta_compact = 0,
                            float* xsum_out = nullptr,      // xsum_out: fp32 [rows, d] receives x (+ deltas), compact
                            float* y32 = nullptr,           // y32: fp32 copy of the output rows (y may then be nullptr)
                            int f16 = 0);                   // f16: y and the deltas are IEEE fp16 instead of bf16
hipError_t launch_im2col(const float* pix, uint16_t* out, int B, int image, int patch, int Kp,
                         hipStream_t stream, int f16 = 0);  // f16: fp16 columns instead of bf16
hipError_t launch_assemble_lnpre(const float* patch_out, const float* cls, const float* pos,
                                 const float* g, const float* b, float* x, int B, int T, int d,
                                 hipStream_t stream);
// starts == nullptr: dense [n_text, ctx] rows; else packed rows (text n owns rows
// [starts[n], starts[n+1]), i.e. its tokens up to and including EOT)
// pfx (optional, with starts): prefix sharing - text n owns only the rows of positions >= pfx[n]; see
// text_lens_scan_kernel
hipError_t launch_text_embed(const int32_t* tok, const float* tok_emb, const float* pos, float* x,
                             int32_t* eot_row, const int32_t* starts, int n_text, int ctx, int d, int vocab,
                             hipStream_t stream, const int32_t* pfx = nullptr);
// starts[0..n_text] = exclusive scan of the own row counts (argmax position + 1 [- shared prefix]);
// starts[n_text + 1] = max length; pfx (optional, int32 [2 * n_text], groups of G texts): [n] = shared
// prefix length, [n_text + n] = packed row of the base text's position 0
hipError_t launch_text_lens_scan(const int32_t* tok, int32_t* starts, int32_t* pfx, int n_text, int ctx, int G,
                                 hipStream_t stream, int32_t* lens_ws);
hipError_t launch_l2norm_rows(float* x, int rows, int d, hipStream_t stream);
// exact (erf) GELU in place: the activation of towers with TVC_ACT_GELU, after a store-only FC1
hipError_t launch_gelu_erf_16(uint16_t* x, int64_t n, int f16, hipStream_t stream);      // bf16, or IEEE fp16 with f16
hipError_t launch_gelu_erf_f32(float* x, int64_t n, hipStream_t stream);
hipError_t launch_split_planes(const float* x, uint16_t* out, int64_t rows, int d, int planes,
                               hipStream_t stream);
hipError_t launch_gather_rows(const BankRows& bank, const int32_t* idx, int64_t idx_offset, int n, float* out, hipStream_t stream);

// ---- attention.hip
// pfx (optional, causal packed rows only): sequence s = pfx[s] rows starting at packed row
// pfx[n_seq + s] (shared prefix, keys only) followed by its own rows [starts[s], starts[s+1]) (keys + queries)
// pool_mode 1 / 2: only the pooled token's output per sequence (first token / EOT token), compact [n_seq, width]
hipError_t launch_attention(const uint16_t* qkv, uint16_t* out, const int32_t* starts, int n_seq,
                            int seq_len, int heads, int causal, hipStream_t stream, const int32_t* pfx = nullptr,
                            int pool_mode = 0, const int32_t* pool_row = nullptr,
                            int f16 = 0);       // f16: qkv and out are IEEE fp16, the products on the f16 MFMA

// ---- bank.hip
struct BankSearchLaunch {
    BankRows bank;
    const uint16_t* qplanes = nullptr;// [M, 2*D] bf16 (hi | lo) query planes
    const float* rows = nullptr;      // [M, D] the fp32 query rows (exact re-scoring of the fast form)
    const float* bank_bounds = nullptr;// [2] device: max |hi plane row|, max |lo plane row|
    bool allow_filter = true;         // one-product filter + re-scoring when no moments are requested
    bool q_rows_padded = false;       // qplanes is readable up to the next multiple of 256 rows (the ring-form filter pass)
    int M = 0;
    int k = 0;
    float count_thr = 0.f;
    int64_t idx_offset = 0;
    // workspace (sized by bank_workspace_bytes)
    float* s0 = nullptr;              // [M, n_sample] pre-pass similarities
    float* gmax = nullptr;            // [M, 256] group maxima of the sample (small-M form: bank_sample_skinny_kernel)
    float* tau = nullptr;             // [M]
    void* cand = nullptr;             // [S, M, CAP] {float, int}
    int32_t* cand_cnt = nullptr;      // [S, M]
    float* mom_part = nullptr;        // [S, M, 4]
    int32_t* overflow = nullptr;      // [1]
    int n_sample = 0, sample_stride = 1, S = 0, cap = 0;
    // outputs
    int32_t* topk_idx = nullptr;
    float* topk_sim = nullptr;
    float* moments = nullptr;
};
hipError_t launch_bank_search(const BankSearchLaunch& L, hipStream_t stream);
hipError_t launch_bank_bounds(const BankRows& bank, float* bounds, hipStream_t stream);
// brute force: sims_ws fp32 [block_rows, R]
hipError_t launch_bank_search_dense(const BankSearchLaunch& L, float* sims_ws, int block_rows, hipStream_t stream);
hipError_t launch_topk_merge(const int32_t* idx_parts, const float* sim_parts, const float* feat_parts,
                             const float* mom_parts, int W, int M, int k, int kf, int D,
                             int32_t* idx_out, float* sim_out, float* feat_out, float* mom_out,
                             hipStream_t stream);

// ---- kmeans.hip: k-means over a bank slot (assign: nearest centre per bank row; update: deterministic cluster means)
struct KmeansAssignLaunch {
    BankRows bank;
    const float* centroids = nullptr; // [K, D] fp32
    const uint16_t* cplanes = nullptr;// [K, 2 * D] bf16 (hi | lo) planes of the centres
    int K = 0;
    float* halfnorm = nullptr;        // workspace [round_up(K, 256)]: |c|^2 / 2, NaN in the padding
    int32_t* labels = nullptr;        // [R]: arg-max of x.c - |c|^2 / 2, lowest centre on ties, -1 when every score is NaN
    float* score = nullptr;           // [R] or nullptr: the winning score
    float* dist2 = nullptr;           // [R] or nullptr: max(0, |x|^2 - 2 score); 0 for label -1
};
hipError_t launch_kmeans_assign(const KmeansAssignLaunch& L, hipStream_t stream);
struct KmeansUpdateLaunch {
    BankRows bank;
    const int32_t* labels = nullptr;  // [R]; labels outside [0, K) belong to no cluster
    const float* centroids_in = nullptr;   // [K, D]: the row an empty cluster keeps
    int K = 0;
    int nblocks = 0, rows_per_block = 0;   // kmeans_update_plan
    int32_t* blk_cnt = nullptr;       // workspace [nblocks, K]
    float* centroids_out = nullptr;   // [K, D]
    int32_t* counts = nullptr;        // [K]
    int32_t* offsets = nullptr;       // [K + 1]
    int32_t* order = nullptr;         // [R]: row indices grouped by cluster, ascending inside a cluster
};
hipError_t launch_kmeans_update(const KmeansUpdateLaunch& L, hipStream_t stream);
// halfnorm[k] = |c_k|^2 / 2, k < K; NaN for K <= k < Kpad
hipError_t launch_kmeans_halfnorm(const float* centroids, int D, int K, int Kpad, float* halfnorm, hipStream_t stream);
// the update's stable counting sort on its own: the indices 0 .. R - 1 grouped by label
struct LabelSortLaunch {
    const int32_t* labels = nullptr;  // [R]; labels outside [0, K) are in no group
    int64_t R = 0;
    int K = 0;
    int nblocks = 0, rows_per_block = 0;   // kmeans_update_plan
    int32_t* blk_cnt = nullptr;       // workspace [nblocks, K]
    int32_t* counts = nullptr;        // [K]
    int32_t* offsets = nullptr;       // [K + 1]
    int32_t* order = nullptr;         // [R]: entries [0, offsets[K]) are written
};
hipError_t launch_label_sort(const LabelSortLaunch& L, hipStream_t stream);
// out[r] = |x_r|^2 of every stored row of the slot (hi + lo of an fp32 bank), fp32 [R]
hipError_t launch_kmeans_rownorm(const BankRows& bank, float* out, hipStream_t stream);

// ---- rank.hip: retrieval evaluation over a bank slot (the rank of every relevant row of every query; metrics from the ranks)
struct RankTileLaunch {
    BankRows bank;
    const uint16_t* qplanes = nullptr;// [M, 2 * D] bf16 (hi | lo) query planes
    int M = 0;
    const int32_t* qlabel = nullptr;  // [M]
    const int32_t* glabel = nullptr;  // [R]
    const int32_t* gpos = nullptr;    // [R]: the row's place inside its label group, ascending row order (targets)
    const int64_t* tgt_off = nullptr; // [M + 1]: exclusive scan of the queries' target counts
    float* tgt_sim = nullptr;         // [T]: targets writes it; count reads it, every query's list in rank order
    int32_t* tgt_row = nullptr;       // [T]: as tgt_sim
    int32_t* hist = nullptr;          // [T] (count): += the irrelevant rows whose first target behind them is this one
    int32_t* qlab = nullptr;          // workspace [rank_plan().mpad]
    float* tlow = nullptr;            // workspace [rank_plan().mpad] (count)
};
hipError_t launch_rank_targets(const RankTileLaunch& L, hipStream_t stream);
hipError_t launch_rank_count(const RankTileLaunch& L, hipStream_t stream);
struct RankMetricsLaunch {
    int M = 0, n_k = 0;
    int k[RANK_MAX_K] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t* tgt_off = nullptr; // [M + 1]
    const int32_t* hist = nullptr;    // [T]
    int32_t* pos = nullptr;           // [T]
    double* ap = nullptr;             // [M]
    double* rr = nullptr;             // [M]
    int32_t* hits = nullptr;          // [M, n_k]
    double* dcg = nullptr;            // [M, n_k]
    double* idcg = nullptr;           // [M, n_k]
};
hipError_t launch_rank_metrics(const RankMetricsLaunch& L, hipStream_t stream);

// ---- roc.hip: detection evaluation (ROC sweep of N sorted scores under B integer weightings: AUROC, AP, Youden, FPR at a TPR)
enum RocSource { ROC_SRC_WEIGHTS = 0, ROC_SRC_INDICES = 1, ROC_SRC_PHILOX = 2 };
enum RocMode { ROC_MODE_WEIGHTS = 0, ROC_MODE_SWEEP = 1, ROC_MODE_CURVE = 2 };
struct RocLaunch {
    int mode = ROC_MODE_SWEEP;
    int source = ROC_SRC_WEIGHTS;
    int N = 0;
    int64_t B = 0;                    // rows of this launch
    int64_t row0 = 0;                 // the first row's place in the caller's arrays (src and every output)
    int64_t first = 0;                // PHILOX: the resample number of the caller's row 0
    uint64_t seed = 0;
    const float* scores = nullptr;    // [N] sorted descending
    const uint8_t* labels = nullptr;  // [N] in sorted order, 0 / 1
    const int32_t* order = nullptr;   // [N]: the original index of every sorted position
    const int32_t* src = nullptr;     // WEIGHTS: [B, N] multiplicities or nullptr (all ones); INDICES: [B, N] draws
    uint32_t* ws = nullptr;           // the global form's counts [B, roc_ws_stride(N)]; nullptr = the LDS form
    size_t lds_bytes = 0;             // the LDS form's dynamic LDS (roc_plan)
    double target = 0.95;
    int n_thr = 0;
    float thr[ROC_MAX_THR] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int32_t* w_out = nullptr;         // ROC_MODE_WEIGHTS: [B, N] multiplicities over the sorted positions
    // ROC_MODE_SWEEP, per row
    int32_t *n_pos = nullptr, *n_neg = nullptr, *valid = nullptr, *n_points = nullptr, *n_kept = nullptr;
    int64_t* auc2 = nullptr;
    double *auc = nullptr, *ap = nullptr, *youden_j = nullptr;
    int32_t *youden_pos = nullptr, *youden_tp = nullptr, *youden_fp = nullptr;
    int32_t *target_pos = nullptr, *target_tp = nullptr, *target_fp = nullptr;
    int32_t *thr_tp = nullptr, *thr_fp = nullptr;       // [B, n_thr]
    // ROC_MODE_CURVE (B = 1): the points and their count
    int32_t *pt_tp = nullptr, *pt_fp = nullptr, *pt_pos = nullptr, *pt_kept = nullptr;      // [N]
    int32_t* pt_count = nullptr;      // [2]: points, kept points
};
hipError_t launch_roc(const RocLaunch& L, hipStream_t stream);

// ---- sim.hip: similarity metrics of pairs of rows (cosine, Euclidean, Manhattan, Pearson, Spearman) and top-k overlap counts
// out fp64 [*, SIM_COLS]: the five metrics in that order, then zeros; ints int64 [*, SIM_INTS]: the sums of cx cy, cx cx and
// cy cy over the centred doubled ranks (zeros when the pair holds a NaN), then the number of NaN elements of the pair
enum SimKey { SIM_KEY_F32 = 0, SIM_KEY_I32 = 1 };
struct SimRowsLaunch {
    const void* x = nullptr;          // [B, ldx] fp32 or int32 (key)
    const void* y = nullptr;          // [B, ldy]
    int64_t ldx = 0, ldy = 0;         // row pitches in elements, >= D
    int64_t B = 0;                    // pairs = workgroups; 0 launches nothing
    int D = 0;                        // 1 .. SIM_MAX_D
    int key = SIM_KEY_F32;
    double* out = nullptr;            // [B, SIM_COLS]
    int64_t* ints = nullptr;          // [B, SIM_INTS]
};
hipError_t launch_sim_rows(const SimRowsLaunch& L, hipStream_t stream);
// crank int32 [n]: lo + hi - n of every element of v in sorted_v (v ascending, NaN last); nan_count int64 [1] or nullptr
hipError_t launch_sim_flat_rank(const float* v, const float* sorted_v, int64_t n, int32_t* crank, int64_t* nan_count, hipStream_t stream);
struct SimFlatLaunch {
    const float* x = nullptr;         // [n]
    const float* y = nullptr;
    const int32_t* cx = nullptr;      // [n]: launch_sim_flat_rank's centred doubled ranks
    const int32_t* cy = nullptr;
    int64_t n = 0;                    // 1 .. SIM_MAX_N
    double* out = nullptr;            // [SIM_COLS]
    int64_t* ints = nullptr;          // [SIM_INTS]
    void* ws = nullptr;               // sim_flat_plan(n).ws_bytes, 8-byte aligned
};
hipError_t launch_sim_flat(const SimFlatLaunch& L, hipStream_t stream);
// count int32 [M]: |set(a[i, :k]) & set(b[i, :k])|; a int32 [M, La], b int32 [M, Lb], 1 <= k <= TOPK_OVERLAP_MAX_K
hipError_t launch_topk_overlap(const int32_t* a, const int32_t* b, int64_t M, int La, int Lb, int k, int32_t* count, hipStream_t stream);

// ---- dbscan.hip: the eps-graph of a bank slot as a bitmask, and DBSCAN's labels from such a graph (exact integer work)
struct RadiusGraphLaunch {
    BankRows bank;
    float eps = 0.f;
    RadiusPlan plan;                  // radius_plan(bank.R)
    float* half = nullptr;            // workspace [plan.hpad]: |x|^2 / 2 - eps^2 / 4; NaN for a non-finite norm and in the padding
    uint32_t* adj = nullptr;          // [R, plan.words]: bit j of row i = (|x_i - x_j|^2 <= eps^2), symmetric, padding bits zero
    int32_t* degree = nullptr;        // [R]: popcount of the row, self included
};
hipError_t launch_radius_graph(const RadiusGraphLaunch& L, hipStream_t stream);
// one sweep of minimum-label propagation over the core-core edges of adj [R, round_up(R, 64) / 32], then a pointer jump;
// init: comp[i] = i for core rows (degree >= min_samples), R otherwise, first.  A sweep that lowered a label ORs 1 into *changed.
hipError_t launch_dbscan_sweep(const uint32_t* adj, const int32_t* degree, int R, int min_samples, int32_t* comp, int32_t* changed,
                               int init, hipStream_t stream);
// comp at its fixed point -> labels [R] (clusters numbered by their lowest core row; border rows the lowest id among their core
// neighbours; -1 noise), core [R] (0 / 1) and *n_clusters
hipError_t launch_dbscan_finish(const uint32_t* adj, const int32_t* degree, int R, int min_samples, const int32_t* comp,
                                int32_t* labels, uint8_t* core, int32_t* n_clusters, hipStream_t stream);

// ---- nearest.hip: every row's most similar LATER row of a bank slot, and the closest pair of the slot
struct ClosestPairLaunch {
    BankRows bank;
    NearestPlan plan;                 // nearest_plan(bank.R)
    float* rinv = nullptr;            // workspace [plan.rpad]: 1 / |x|; 0 for a zero row, NaN for a non-finite norm and in the padding
    int32_t* partner = nullptr;       // [R]: arg-max over j > i of cos(x_i, x_j), (value desc, j asc); -1 where no later row is admissible
    float* sim = nullptr;             // [R]: that cosine; -inf where partner is -1
    int32_t* pair = nullptr;          // [2]: the first maximal (i, partner[i]) in lexicographic order; (-1, -1) when no row has a partner
    float* pair_sim = nullptr;        // [1]: its cosine; -inf for (-1, -1)
};
hipError_t launch_closest_pair(const ClosestPairLaunch& L, hipStream_t stream);

// ---- pairs.hip: the upper triangle of a bitmask graph as a pair list, and the fp32-grade cosine of listed pairs of a bank slot
// offsets int64 [R + 1]: the exclusive scan of the rows' counts of set bits j, i < j < R (with group: both groups >= 0 and
// different); adj [R, round_up(R, 64) / 32] is any bitmask
hipError_t launch_graph_pair_count(const uint32_t* adj, int R, const int32_t* group, int64_t* offsets, hipStream_t stream);
// pairs int32 [P, 2]: row i's pairs (i, j) in ascending j from slot offsets[i]; a slot outside [0, P) is not written
hipError_t launch_graph_pair_fill(const uint32_t* adj, int R, const int32_t* group, const int64_t* offsets, int32_t* pairs, int64_t P,
                                  hipStream_t stream);
// sim[p] = x.y / sqrt(|x|^2 |y|^2) of the stored rows pairs[p] of the slot in fp32 FMAs of a fixed order; 0 for a zero row, NaN
// for an index outside [0, R)
hipError_t launch_pair_cosine(const BankRows& bank, const int32_t* pairs, int64_t P, float* sim, hipStream_t stream);

// ---- ivf.hip: inverted-file search (probe: the nprobe best lists of a query; scan: exact top-k over the probed lists)
struct IvfProbeLaunch {
    const uint16_t* cplanes = nullptr;// [nlist, 2 * D] bf16 (hi | lo) planes of the centroids
    const uint16_t* qplanes = nullptr;// [M, 2 * D] bf16 (hi | lo) planes of the queries
    const float* centroids = nullptr; // [nlist, D] fp32
    float* halfnorm = nullptr;        // workspace [nlist]: |c|^2 / 2
    int M = 0, D = 0, nlist = 0, nprobe = 0;
    int chunk = 0;                    // queries per GEMM (the rows of sims)
    float* sims = nullptr;            // workspace [chunk, nlist]
    int32_t* lists = nullptr;         // [M, nprobe]: list ids, best first; -1 from the first rank that has no list
    float* score = nullptr;           // [M, nprobe] or nullptr: q.c - |c|^2 / 2; -inf where lists is -1
};
hipError_t launch_ivf_probe(const IvfProbeLaunch& L, hipStream_t stream);
struct IvfScanLaunch {
    BankRows bank;                    // the rows in list order
    const uint16_t* qplanes = nullptr;// [M, 2 * D] query planes
    int M = 0, k = 0, nprobe = 0, nlist = 0, max_list_rows = 0;
    const int32_t* probes = nullptr;  // [M, nprobe]
    const int32_t* list_offsets = nullptr;   // [nlist + 1]
    const int32_t* row_ids = nullptr; // [R] or nullptr (identity)
    int64_t idx_offset = 0;
    IvfScanPlan plan;                 // ivf_scan_plan
    // workspace
    int32_t* blk_cnt = nullptr;       // [plan.sort_blocks, nlist]
    int32_t* pair_counts = nullptr;   // [nlist]
    int32_t* pair_offsets = nullptr;  // [nlist + 1]
    int32_t* pair_order = nullptr;    // [plan.chunk * nprobe]
    float* scores = nullptr;          // [plan.chunk * nprobe, plan.pitch]
    int32_t* overflow = nullptr;      // [1]: bit 2 = a probed list was longer than max_list_rows
    // outputs
    int32_t* topk_idx = nullptr;
    float* topk_sim = nullptr;
    int32_t* topk_pos = nullptr;      // or nullptr
};
hipError_t launch_ivf_scan(const IvfScanLaunch& L, hipStream_t stream);

// ---- consistency.hip
struct ConsistencyParams {
    int reference_count;
    float similarity_threshold;
    int retrieval_top_k;
    float dup_threshold;
    float w_text_variants, w_consistency;
    float w_exp[4];
};
hipError_t launch_consistency(const float* img, const float* txt, int B, int N, int D,
                              const int32_t* ref_idx, const float* ref_sim, const float* ref_feat,
                              int ks, int kf, const ConsistencyParams& p, float* rec, int rec_stride,
                              hipStream_t stream);

// ---- backward.hip / attention_bwd.hip: input gradient (dX only) of the vision tower
hipError_t launch_layernorm_bwd(const float* x, int64_t x_row_stride, const uint16_t* delta, const void* dy, int dy_fp32,
                                const float* gamma, const float* dres, float* dx, uint16_t* dx16, int rows, int d,
                                int64_t out_row_stride, hipStream_t stream);
hipError_t launch_lnpre_bwd(const float* patch_out, const float* pos, const float* gamma, const float* dy,
                            uint16_t* dpatch, int B, int T, int d, hipStream_t stream);
hipError_t launch_gelu_bwd(uint16_t* dm, const uint16_t* u, int64_t n, hipStream_t stream);
hipError_t launch_gelu_fwd(const uint16_t* u, uint16_t* out, int64_t n, hipStream_t stream);
hipError_t launch_l2norm_bwd(const float* x, const float* dy, uint16_t* dx16, int rows, int d, int normalize, hipStream_t stream);
hipError_t launch_col2im(const float* dcols, float* dpix, int B, int S, int patch, int Kp, hipStream_t stream);
hipError_t launch_transpose_bf16(const uint16_t* in, uint16_t* out, int R, int C, hipStream_t stream);
hipError_t launch_pgd_step(float* adv, const float* clean, const float* grad, float* mom, int B, int64_t n, float eps,
                           float alpha, float mu, float lo, float hi, int targeted, hipStream_t stream);
hipError_t launch_l2_step(float* adv, const float* clean, const float* grad, int B, int64_t n, float eps, float step, float lo,
                          float hi, int descent, hipStream_t stream);
hipError_t launch_attention_bwd(const uint16_t* qkv, const uint16_t* dao, uint16_t* dqkv, float* stats_ws, int n_seq, int T,
                                int heads, hipStream_t stream);

// ---- the same path at fp32 grade (TVC_OPT_GRAD_PRECISION = 2; backward.hip, attention_split_bwd.hip, split.hip): fp32 in, fp32 out
// LayerNorm backward with an fp32 delta and fp32 dy (row addressing as launch_layernorm_bwd)
hipError_t launch_layernorm_bwd_f32(const float* x, int64_t x_row_stride, const float* delta, const float* dy, const float* gamma,
                                    const float* dres, float* dx, int rows, int d, int64_t out_row_stride, hipStream_t stream);
hipError_t launch_lnpre_bwd_f32(const float* patch_out, const float* pos, const float* gamma, const float* dy, float* dpatch, int B,
                                int T, int d, hipStream_t stream);
hipError_t launch_gelu_bwd_f32(float* dm, const float* u, int64_t n, hipStream_t stream);      // in place on dm; n % 4 == 0
hipError_t launch_l2norm_bwd_f32(const float* x, const float* dy, float* dx, int rows, int d, int normalize, hipStream_t stream);
// qkv fp32 [n_seq * T, 3 * width] (kept), dao fp32 [n_seq * T, width] -> dqkv fp32 [n_seq * T, 3 * width]; every product on
// hi | lo planes; stats_ws fp32 [n_seq * T, heads, 4] scratch; T <= 288
hipError_t launch_attention_split_bwd(const float* qkv, const float* dao, float* dqkv, float* stats_ws, int n_seq, int T, int heads,
                                      hipStream_t stream);
// fp32 W [I, ld] (K columns) -> planes of W^T [*, 2 * Ip]: rows k < K, columns i < I of each plane (the caller zeroes the padding)
hipError_t launch_rows_split_t(const float* w, int64_t ld, uint16_t* out, int I, int K, int Ip, hipStream_t stream);

// ---- attack.hip: the FSTA / SMA loops' embedding gradient and step (formulas in include/tvc.h)
// f, t, g, grad fp32 [B, D]; loss_rows fp32 [B, 4]; euclid 0: cosine terms, 1: Euclidean distances
hipError_t launch_attack_feature_grad(const float* f, const float* t, const float* g, int B, int D, float a_tgt, float a_txt,
                                      int euclid, float w_out, float w_div, float* grad, float* loss_rows, hipStream_t stream);
// in place on adv and mom, B images of n elements; l2 0: sign step and L-inf ball, 1: momentum step and L2 ball
hipError_t launch_attack_step(float* adv, const float* clean, const float* grad, float* mom, int B, int64_t n, float eps, float lr,
                              float mu, float clip, float p, float lo, float hi, int l2, hipStream_t stream);

// ---- precise.hip: fp32-grade towers (exact-f32 MFMA GEMM, fp32 attention)
// out[j, i] (op)= sum_k X[j, k] W[i, k] + bias[i]; epi 0 store, 1 QuickGELU, 2 out += ; K, ldw, ldx multiples of 4
hipError_t launch_gemm_f32(const float* W, int64_t ldw, const float* X, int64_t ldx, const float* bias, float* out,
                           int64_t ldo, int I, int J, int K, int epi, hipStream_t stream);
hipError_t launch_attention_f32(const float* qkv, float* out, int n_seq, int T, int heads, int causal, hipStream_t stream);
hipError_t launch_im2col_f32(const float* pix, float* out, int B, int image, int patch, hipStream_t stream);
hipError_t launch_gather_f32_rows(const float* x, int64_t ld, const int32_t* idx, int64_t idx_mul, float* out, int n,
                                  int d, hipStream_t stream);

// ---- split.hip: split-bf16 towers (hi | lo bf16 planes [rows, 2K], three MFMA products per element)
// LayerNorm of x (+ fp32 deltas d1, d2; written back to x when write_x) -> planes [rows, 2d] and / or fp32 rows y32
hipError_t launch_ln_split(float* x, int64_t x_row_stride, const int32_t* row_idx, const float* d1, const float* d2, int write_x,
                           const float* g, const float* b, uint16_t* planes, float* y32, int rows, int d, hipStream_t stream);
// fp32 [rows, ld_in] (K columns) -> planes [rows, 2 * Kp] zero padded; gelu 1: QuickGELU first, 2: erf GELU first
hipError_t launch_rows_split(const float* x, int64_t ld_in, uint16_t* out, int64_t rows, int K, int Kp, int gelu, hipStream_t stream);
// qkv fp32 [rows, 3 * width] -> attention output planes [rows, 2 * width]; ragged / prefix-sharing as launch_attention
hipError_t launch_attention_split(const float* qkv, uint16_t* out, const int32_t* starts, int n_seq, int seq_len, int heads,
                                  int causal, hipStream_t stream, const int32_t* pfx = nullptr);

// ---- sd_ops.hip / sd_attention.hip: latent-diffusion reference generator (16-bit token-major activations)
// f16 (TVC_OPT_SD_PRECISION = 1): every 16-bit tensor a launcher reads or writes is IEEE fp16 instead of bf16.  The launchers
// without the flag (im2col3x3, relayout, concat; launch_transpose_bf16) only move 16-bit words: one instantiation serves both.
hipError_t sd_im2col3x3(const uint16_t* in, uint16_t* out, int n, int Hi, int Wi, int C, int stride, int up, hipStream_t st);
hipError_t sd_im2col_in(const float* in, uint16_t* out, int n, int Cin, int H, int W, int Kp, float scale, hipStream_t st, int f16 = 0);
hipError_t sd_groupnorm(const uint16_t* x, const float* tadd, int64_t ld_t, const float* gamma, const float* beta, uint16_t* y,
                        int n, int H, int W, int C, int groups, float eps, int silu, int in_pad, int out_pad, float* ws,
                        hipStream_t st, int f16 = 0);
hipError_t sd_relayout(const uint16_t* in, uint16_t* out, int n, int H, int W, int C, int in_pad, int out_pad, int up, hipStream_t st);
hipError_t sd_add_padded(const uint16_t* a, const uint16_t* b_padded, uint16_t* out, int n, int H, int W, int C, hipStream_t st,
                         int f16 = 0);
// add: y = LN(r16(x + add)), the 16-bit sum also to sum_out
hipError_t sd_layernorm_bf16(const uint16_t* x, const float* g, const float* b, uint16_t* y, int64_t rows, int C, float eps, hipStream_t st,
                             const uint16_t* add = nullptr, uint16_t* sum_out = nullptr, int f16 = 0);
hipError_t sd_geglu(const uint16_t* in, uint16_t* out, int64_t rows, int Ch, hipStream_t st, int f16 = 0);
hipError_t sd_add_bf16(const uint16_t* a, const uint16_t* b, uint16_t* out, int64_t n, hipStream_t st, int f16 = 0);
hipError_t sd_concat(const uint16_t* a, int Ca, const uint16_t* b, int Cb, uint16_t* out, int64_t tokens, hipStream_t st);
hipError_t sd_cast_silu(const float* in, uint16_t* out, int64_t n, int silu, hipStream_t st, int f16 = 0);
hipError_t sd_tokens_to_nchw(const float* in, int64_t ld, float* out, int n, int C, int H, int W, float mul, float add, int clamp01,
                             int in_pad, hipStream_t st);
hipError_t sd_pointwise_small(const float* in, const float* w, const float* bias, float* out, int n, int C, int HW, float in_scale, hipStream_t st);
hipError_t sd_cfg(const float* e, float* out, int64_t n, float g, hipStream_t st);
hipError_t sd_lincomb(float* out, const float* sample, float cs, float ce, const float* e0, float c0, const float* e1, float c1,
                      const float* e2, float c2, const float* e3, float c3, int64_t n, hipStream_t st);
hipError_t sd_softmax_rows(const float* s, uint16_t* p, int64_t rows, int T, float scale, hipStream_t st, int f16 = 0);
hipError_t sd_nchw_to_tokens(const float* in, uint16_t* out, int n, int C, int HW, hipStream_t st, int f16 = 0);
hipError_t sd_tokens_bf16_to_nchw(const uint16_t* in, float* out, int n, int C, int HW, hipStream_t st, int f16 = 0);
hipError_t sd_timestep_embed(uint16_t* out, int n, int dim, float t, hipStream_t st, int f16 = 0);
// Q [n * Tq, ldq], K / V [n * Tk, ldk / ldv], O [n * Tq, ldo] bf16 (fp16 with f16); head h = columns [h * dh, (h + 1) * dh); dh % 8 == 0, <= 160
hipError_t sd_flash_attention(const uint16_t* Q, int64_t ldq, const uint16_t* K, int64_t ldk, const uint16_t* V, int64_t ldv,
                              uint16_t* O, int64_t ldo, int n, int heads, int Tq, int Tk, int dh, hipStream_t st, int f16 = 0);
hipError_t sd_resize_norm(const float* in, float* out, int n, int H, int W, int Hr, int Wr, int oy, int ox, int S, int cubic,
                          const float* mean, const float* sd, hipStream_t st);
