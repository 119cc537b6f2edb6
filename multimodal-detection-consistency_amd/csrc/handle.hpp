// Internal: the handle behind include/tvc.h, its workspace slots and the launch helpers shared by the translation
// units that implement the C-ABI (tvc_abi.cpp: the CLIP tower encode drivers of every precision mode and the bf16 /
// fp16 towers, bank, consistency; tvc_precise.cpp: the fp32-grade towers' stem, layer loop and head; tvc_split.cpp: the
// split-bf16 towers' stem, layer loop, head and weight planes; tvc_sd.cpp: latent-diffusion reference generator,
// tvc_sd_op.cpp: its entry points that read no model state; tvc_kmeans.cpp: k-means over a bank slot;
// tvc_ivf.cpp: IVF probe and list scan; tvc_grad_split.cpp: the split-bf16 input gradient; tvc_dbscan.cpp: radius graph and
// DBSCAN labels; tvc_pairs.cpp: pair lists of a bitmask graph and the cosine of listed pairs; tvc_rank.cpp: retrieval evaluation;
// tvc_roc.cpp: detection evaluation; tvc_nearest.cpp: closest pair of a bank slot; tvc_sim.cpp: similarity metrics of row pairs).
// The entry points that pass over a bank slot share filled_slot (the TVC_E_STATE refusal of an empty slot) and ensure_planes /
// split_planes (a workspace slot of (hi | lo) query planes); their work estimate is host_plan.hpp's slot_pass_flops.
#pragma once
#include "../../include/tvc.h"
#include "kernels.hpp"

#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

inline thread_local std::string g_create_error;

enum Slot {
    // tower workspaces exist twice (vision, text: + WS_TOWER_N) so that the two towers can run
    // concurrently on two streams
    WS_X = 0, WS_H, WS_QKV, WS_MLP, WS_CLS, WS_DELTA, WS_DELTA2, WS_SPLITK, WS_POOL, WS_TOWER_N,
    WS_TX = WS_TOWER_N, WS_TH, WS_TQKV, WS_TMLP, WS_TCLS, WS_TDELTA, WS_TDELTA2, WS_TSPLITK, WS_TPOOL,
    WS_PATCH, WS_EOT, WS_STARTS, WS_PFX, WS_LENS,
    WS_COSX, WS_COSY, WS_COSXP, WS_COSYP,
    WS_QPLANES, WS_S0, WS_TAU, WS_CAND, WS_CAND_CNT, WS_MOM_PART, WS_OVERFLOW,
    // input-gradient path (vision tower): saved layer inputs, gradient stream, scratch
    WS_GSAVE, WS_GOUT, WS_GXL, WS_GDX, WS_G16, WS_GMLP2, WS_GDQKV, WS_GSTATS, WS_GSMALL, WS_GPATCH,
    // fp32-grade towers (TVC_OPT_TOWER_PRECISION = 1): vision set, then the text set (+ WS_P_N)
    WS_PX, WS_PH, WS_PQKV, WS_PMLP, WS_PCLS, WS_P_N_END,
    WS_PTX = WS_P_N_END, WS_PTH, WS_PTQKV, WS_PTMLP, WS_PTCLS,
    // split-bf16 towers (TVC_OPT_TOWER_PRECISION = 2, tvc_split.cpp): vision set, then the text set (+ WS_S_N)
    WS_SX, WS_SH, WS_SQKV, WS_SU, WS_SM, WS_SDELTA1, WS_SDELTA2, WS_SCLS, WS_S_END,
    WS_STX = WS_S_END, WS_STH, WS_STQKV, WS_STU, WS_STM, WS_STDELTA1, WS_STDELTA2, WS_STCLS,
    // latent-diffusion reference generator (tvc_sd.cpp)
    WS_SD0, WS_SD1, WS_SD2, WS_SD3, WS_SD4, WS_SD5, WS_SD6, WS_SD7,
    // k-means over a bank slot (tvc_kmeans.cpp): centre planes, half norms, counting-sort counters, offsets / order when the
    // caller does not ask for them
    WS_KM_CPLANES, WS_KM_HALFNORM, WS_KM_BLKCNT, WS_KM_OFFSETS, WS_KM_ORDER,
    // IVF search (tvc_ivf.cpp): the probe's centroid / query planes, half norms and score rows; the scan's query planes, the
    // counting sort of its (query, probe) pairs and the score buffer
    WS_IVF_CPLANES, WS_IVF_PQPLANES, WS_IVF_HALFNORM, WS_IVF_SIMS,
    WS_IVF_QPLANES, WS_IVF_BLKCNT, WS_IVF_PCOUNTS, WS_IVF_POFFSETS, WS_IVF_PORDER, WS_IVF_SCORES,
    // split-bf16 input gradient (TVC_OPT_GRAD_PRECISION = 2, tvc_grad_split.cpp): what the forward keeps, the gradient's planes
    // (d-wide; mlp- / 3d-wide), fp32 scratch (mlp- / 3d- / Kp-wide; d-wide) and the head's small rows
    WS_GS_KEEP, WS_GS_GP, WS_GS_MP, WS_GS_WIDE, WS_GS_ROW, WS_GS_SMALL,
    // radius graph over a bank slot (tvc_dbscan.cpp): the padded half-norm vector of the distance test
    WS_DB_HALF,
    // retrieval evaluation (tvc_rank.cpp): the query planes, the query labels and the last-target scores padded to whole tiles
    WS_RK_QPLANES, WS_RK_QLAB, WS_RK_TLOW,
    // detection evaluation (tvc_roc.cpp): the multiplicity rows of the global storage form, uint32 [chunk rows, N]
    WS_ROC_COUNTS,
    // closest pair of a bank slot (tvc_nearest.cpp): the padded 1 / |x| vector
    WS_NN_RINV,
    WS_COUNT
};

struct Buf {
    void* p = nullptr;
    size_t n = 0;
};

struct BankSlot {
    const uint16_t* bank = nullptr;
    void* owned = nullptr;            // (hi | lo) planes of an fp32 bank
    int64_t R = 0;
    int D = 0;
    int planes = 1;
    float* bounds = nullptr;          // device [2]: max row norms of the bank planes
};

inline BankRows bank_rows(const BankSlot& bk) { return BankRows{bk.bank, (int64_t)bk.planes * bk.D, bk.R, bk.D, bk.planes}; }
// plane products of a full-precision pass over a slot: b.qhi + b.qlo, or bhi.qhi + bhi.qlo + blo.qhi
inline int bank_products(int planes) { return planes == 2 ? 3 : 2; }

constexpr int WS_P_N = WS_P_N_END - WS_PX;    // offset from a vision fp32-grade slot to its text twin
constexpr int WS_S_N = WS_S_END - WS_SX;      // offset from a vision split slot to its text twin

// hi | lo bf16 planes [round_up(out, 256), 2 * in] of one layer's GEMM weights (split-bf16 mode), handle-owned
struct SplitLayer { uint16_t *wqkv = nullptr, *wo = nullptr, *w1 = nullptr, *w2 = nullptr; };
// what split_layers keeps for the split-bf16 input gradient, fp32, layer l at l * rows * (the width): the layer's input rows
// [rows, d], its QKV rows [rows, 3d], its out-projection output [rows, d] and the FC1 pre-activation [rows, mlp]
struct SplitKeep { float *x = nullptr, *qkv = nullptr, *d1 = nullptr, *u = nullptr; };

struct ProfRec {
    hipEvent_t a, b;
    int cat;
    double work;
    double big_bytes = 0;     // GEMM launches of >= 64 output tiles (the persistent ring kernels): compulsory HBM bytes
    int gI = 0, gJ = 0, gK = 0, gP = 0, gS = 0;     // GEMM launches: shape, planes, fixed K split (TVC_PROF_DUMP)
};

// One registered weight set of a tower: the caller's struct with its layer array copied (the caller's array may go away
// after the call; the tensors themselves are referenced, not copied)
template <class W, class L>
struct TowerWeights {
    W w{};
    std::vector<L> layers;
    bool set = false;
    void assign(const W& src, int n_layers) {
        w = src;
        layers.assign(src.layers, src.layers + n_layers);
        w.layers = layers.data();
        set = true;
    }
};

struct tvc_handle {
    tvc_model_desc desc{};
    // bf16 weights (tvc_create): precision 0 and the input-gradient path; `set` = the handle has that tower
    TowerWeights<tvc_vision_weights, tvc_layer_weights> vision;
    TowerWeights<tvc_text_weights, tvc_layer_weights> text;
    // banks: TVC_MAX_BANKS independent slots (retriever index, reference bank, defense references ...
    // registered by different owners on one engine); tvc_bank_select picks the one the bank calls address
    BankSlot banks[TVC_MAX_BANKS];
    int cur_bank = 0;
    bool bank_filter = true;          // TVC_OPT_BANK_FILTER
    Buf ws[WS_COUNT];
    std::string err;
    int max_chunk_images = 512;
    int max_chunk_texts = 4608;
    bool pack_text = true;     // TVC_OPT_TEXT_PACKING
    int text_group = 0;        // TVC_OPT_TEXT_GROUP: texts come in groups of this many sharing prefixes (0: off)
    bool pooled_last = true;   // TVC_OPT_POOLED_LAST_LAYER
    // input-gradient state: transposed GEMM weights (built on first use), what the last tvc_encode_image_grad saw
    std::vector<void*> wT;     // per layer: wqkvT, woT, w1T, w2T; then projT, patchT
    int grad_B = 0;
    int grad_normalize = 0;
    const float* grad_pix = nullptr;
    int grad_precision = 0;    // TVC_OPT_GRAD_PRECISION: 0 = bf16, 2 = split-bf16 (tvc_grad_split.cpp)
    int grad_mode = 0;         // the mode the last tvc_encode_image_grad ran in: its backward runs in no other
    bool prof = false;
    std::vector<ProfRec> prof_recs;
    // fp32 copies of every weight (tvc_set_weights_f32): precision 1, and the source of precision 2's planes
    TowerWeights<tvc_vision_weights_f32, tvc_layer_weights_f32> vision32;
    TowerWeights<tvc_text_weights_f32, tvc_layer_weights_f32> text32;
    int tower_precision = 0;   // TVC_OPT_TOWER_PRECISION
    // fp16 towers (precision 3): the caller's IEEE fp16 weight set (tvc_set_weights_f16)
    TowerWeights<tvc_vision_weights, tvc_layer_weights> vision16;
    TowerWeights<tvc_text_weights, tvc_layer_weights> text16;
    // split-bf16 mode (precision 2): planes of every GEMM weight, built from the fp32 copies when the option is set
    std::vector<SplitLayer> vsplit, tsplit;
    uint16_t* vsplit_patch = nullptr;
    std::vector<void*> split_owned;
    bool split_ready = false;
    // split-bf16 input gradient: planes [round_up(in, 256), 2 * out] of the transposed vision GEMM weights, built on first use
    // from the fp32 copies; owned through split_owned (they live and die with the planes above)
    std::vector<SplitLayer> vsplit_t;
    uint16_t *vsplit_proj_t = nullptr, *vsplit_patch_t = nullptr;
    struct SdState* sd = nullptr;   // latent-diffusion model (tvc_sd.cpp), owned
    int sd_precision = 0;           // TVC_OPT_SD_PRECISION: 0 = bf16, 1 = IEEE fp16; fixed while a model is loaded (its tensors are one format)
    size_t sd_arena_bytes = (size_t)48 << 30;   // TVC_OPT_SD_ARENA_BYTES: activation arena of one UNet evaluation
    // TVC_OPT_SD_STREAMS: the two classifier-free-guidance halves of a UNet evaluation on two HIP streams (tvc_sd.cpp)
    int sd_streams = 2;
    hipStream_t sd_aux = nullptr;
    hipEvent_t sd_fork = nullptr, sd_join = nullptr;
};
void tvc_sd_free(tvc_handle* h);    // tvc_sd.cpp
void tvc_split_free(tvc_handle* h); // tvc_split.cpp
int tvc_split_prepare(tvc_handle* h);

// What precisions 1 (tvc_precise.cpp) and 2 (tvc_split.cpp) supply to the tower encode drivers of tvc_abi.cpp, which
// own everything else (checks, chunking, text packing, embeddings, L2 normalisation); `text` picks the tower.
//   *_ensure: the workspace of passes of up to n_seq sequences; X = the fp32 residual stream the embeddings go to
//   *_stem:   im2col + patch GEMM of n images -> patch_out fp32 [n * P, d]
//   *_layers: n_seq sequences of seq_len dense rows, or (starts) total_rows packed rows
//   *_head:   final LayerNorm of `rows` rows of X (x_stride, row_idx as launch_layernorm), then the projection to out
//             [rows, embed_dim]; hidden: the LayerNorm's fp32 rows to out instead
int precise_ensure(tvc_handle* h, bool text, int n_seq, float** X);
int precise_stem(tvc_handle* h, const float* pix, int n, const float** patch_out, hipStream_t st);
int precise_layers(tvc_handle* h, bool text, int n_seq, int seq_len, hipStream_t st);
int precise_head(tvc_handle* h, bool text, int64_t x_stride, const int32_t* row_idx, int rows, float* out, bool hidden,
                 hipStream_t st);
int split_ensure(tvc_handle* h, bool text, int n_seq, float** X);
int split_stem(tvc_handle* h, const float* pix, int n, const float** patch_out, hipStream_t st);
int split_layers(tvc_handle* h, bool text, int n_seq, int seq_len, const int32_t* starts, int total_rows,
                 const int32_t* pfx, hipStream_t st);
int split_head(tvc_handle* h, bool text, int64_t x_stride, const int32_t* row_idx, int rows, float* out, bool hidden,
               hipStream_t st);
// split_layers with the state of every layer kept for the backward (dense rows; see SplitKeep).  *d1_last / *d2_last: the last
// layer's two pending deltas, which the caller's final LayerNorm folds in.
int split_layers_keep(tvc_handle* h, int n_seq, int seq_len, const SplitKeep& keep, const float** d1_last, const float** d2_last,
                      hipStream_t st);
// out fp32 [J, ldo] = (W_hi + W_lo)[I, K] x (B_hi + B_lo)[J, K]^T + bias on planes [*, 2K], without the lo x lo term; both
// operands are readable to whole row tiles
int split_gemm3(tvc_handle* h, const uint16_t* Ws, int I, int K, const uint16_t* Bs, int64_t J, const float* bias, float* out,
                int64_t ldo, hipStream_t st);

// The two drivers of the split-bf16 input gradient (TVC_OPT_GRAD_PRECISION = 2; tvc_grad_split.cpp): tvc_encode_image_grad /
// _backward (tvc_abi.cpp) check the arguments both modes share and call these.
int grad_split_forward(tvc_handle* h, const float* pix, int B, float* out, int normalize, hipStream_t st);
int grad_split_backward(tvc_handle* h, const float* grad_out, float* grad_pix, hipStream_t st);

inline int fail(tvc_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t st__ = (expr);                                                            \
        if (st__ != hipSuccess)                                                              \
            return fail(h, TVC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(st__));  \
    } while (0)

inline int ensure(tvc_handle* h, Slot s, size_t bytes) {
    Buf& b = h->ws[s];
    if (b.n >= bytes && b.p) return TVC_OK;
    if (b.p) {
        // hipFree synchronises the device, so kernels still using the old block are done
        if (hipFree(b.p) != hipSuccess) return fail(h, TVC_E_HIP, "hipFree(workspace) failed");
        b.p = nullptr; b.n = 0;
    }
    // grow with a little slack so alternating sizes do not thrash
    const size_t want = bytes + bytes / 16 + 256;
    if (hipMalloc(&b.p, want) != hipSuccess) {
        b.p = nullptr;
        char m[128];
        snprintf(m, sizeof m, "workspace allocation of %zu bytes failed", want);
        return fail(h, TVC_E_NOMEM, m);
    }
    b.n = want;
    return TVC_OK;
}

// The slot the bank calls address, for an entry point that reads its stored rows; no bank (never set, or released) and an empty
// bank are its TVC_E_STATE refusal.  `fn` names the entry point in the message.
inline int filled_slot(tvc_handle* h, const char* fn, BankSlot** out) {
    BankSlot& bk = h->banks[h->cur_bank];
    if (bk.D == 0 || !bk.bank || bk.R == 0) return fail(h, TVC_E_STATE, std::string(fn) + ": the selected slot holds no bank rows");
    *out = &bk;
    return TVC_OK;
}

// The (hi | lo) bf16 planes of fp32 rows, kept in a workspace slot.  Two steps, because an entry point sizes all its slots
// before its first launch (a refusal for lack of memory comes before any work, and `ensure` may free and so synchronise):
//   ensure_planes  room for `rows` rows of D columns, the count rounded up to a multiple of row_pad (256 where the reader
//                  stages whole row tiles: the bank searches; else 1)
//   split_planes   splits x [rows, D] into the slot; *out = the slot's planes [rows, 2 * D]
inline int ensure_planes(tvc_handle* h, Slot s, int64_t rows, int row_pad, int D) {
    return ensure(h, s, (size_t)((rows + row_pad - 1) / row_pad * row_pad) * 2 * D * 2);
}
inline int split_planes(tvc_handle* h, Slot s, const float* x, int64_t rows, int D, hipStream_t st, const uint16_t** out) {
    *out = (const uint16_t*)h->ws[s].p;
    HIP_TRY(launch_split_planes(x, (uint16_t*)h->ws[s].p, rows, D, 2, st));
    return TVC_OK;
}

// RAII bracket: two events around whatever is launched inside the scope
struct ProfScope {
    tvc_handle* h; hipStream_t st; ProfRec r; bool on;
    ProfScope(tvc_handle* h_, hipStream_t st_, int cat, double work) : h(h_), st(st_), on(h_->prof) {
        if (!on) return;
        r.cat = cat; r.work = work;
        if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(r.a, st);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(r.b, st);
        h->prof_recs.push_back(r);
    }
};

inline double gemm_flops(const GemmLaunch& g) { return 2.0 * g.I * (double)g.J * g.K * g.planes; }

// Compulsory HBM bytes of a GEMM launch: every distinct operand plane read once, the output written once (read once
// more by the residual epilogue).  Planes that address the same rows shifted by whole rows (the nine taps of a 3 x 3
// convolution on the token operand) count once.
inline double gemm_compulsory_bytes(const GemmLaunch& g) {
    auto distinct = [&](const int* off, int64_t ld) {
        int n = 0;
        for (int p = 0; p < g.planes; ++p) {
            bool seen = false;
            for (int q = 0; q < p; ++q) seen = seen || (off[p] % ld == off[q] % ld);
            n += seen ? 0 : 1;
        }
        return n;
    };
    const double a = 2.0 * g.I * (double)g.K * distinct(g.a_plane_off, g.lda > 0 ? g.lda : g.K);
    const double b = 2.0 * g.J * (double)g.K * distinct(g.b_plane_off, g.ldb > 0 ? g.ldb : g.K);
    const double o = (double)g.I * g.J * (g.epilogue == TVC_EPI_F32 ? 4.0 : g.epilogue == TVC_EPI_RESID_F32 ? 8.0 : 2.0);
    return a + b + o;
}

inline hipError_t timed_gemm(tvc_handle* h, const GemmLaunch& g, hipStream_t st, int splitk_slot = -1) {
    ProfScope ps(h, st, TVC_PROF_GEMM, gemm_flops(g));
    if (ps.on && (int64_t)((g.I + 255) / 256) * ((g.J + 255) / 256) >= 64) ps.r.big_bytes = gemm_compulsory_bytes(g);
    if (ps.on) { ps.r.gI = g.I; ps.r.gJ = g.J; ps.r.gK = g.K; ps.r.gP = g.planes; ps.r.gS = g.splitk_fixed; }
    if (splitk_slot >= 0 && h->ws[splitk_slot].p) {
        GemmLaunch g2 = g;
        g2.splitk_ws = (float*)h->ws[splitk_slot].p;
        g2.splitk_ws_bytes = h->ws[splitk_slot].n;
        return launch_gemm_bf16(g2, st);
    }
    return launch_gemm_bf16(g, st);
}

// exact-f32 GEMM (precise.hip): out[j, i] (op)= sum_k X[j, k] W[i, k] + bias[i], epi as launch_gemm_f32
inline int timed_gemm_f32(tvc_handle* h, const float* W, int I, int K, const float* X, int64_t J, const float* bias, float* out,
                          int64_t ldo, int epi, hipStream_t st) {
    ProfScope ps(h, st, TVC_PROF_GEMM, 2.0 * I * (double)J * K);
    HIP_TRY(launch_gemm_f32(W, K, X, K, bias, out, ldo, I, (int)J, K, epi, st));
    return TVC_OK;
}
