// C-ABI of the TVC hot path (include/tvc.h): handle, workspace and the launch
// sequences of the CLIP towers, the bank search and the consistency kernel.
// No torch types, no exceptions across the boundary, no device synchronisation
// except where tvc.h says so.
#include "handle.hpp"

#include <cstdlib>

namespace {

bool tower_ok(const tvc_tower_arch& a) {
    return a.width > 0 && a.layers > 0 && a.heads > 0 && a.width == a.heads * 64 && a.width % 64 == 0 &&
           a.width <= 1024 && a.mlp > 0 && a.mlp % 64 == 0 && (a.act == TVC_ACT_QUICK_GELU || a.act == TVC_ACT_GELU);
}

// One transformer tower over `rows` packed token rows (n_seq sequences of seq_len).
// Sequences: n_seq x seq_len dense rows, or (starts != nullptr) packed rows with
// `total_rows` rows in all and seq_len = the maximum length.
// pool_mode (TVC_OPT_POOLED_LAST_LAYER): 1 / 2 = the caller only reads the pooled token of every sequence (first
// token / EOT token at packed row pool_row[s]).  The LAST layer then computes attention, out-proj, ln_2 and the
// MLP for those n_seq rows only (its K and V still need every token): outputs identical, 10/12 of the layer's
// GEMM work and all but one query of its attention dropped.  Its deltas are left COMPACT ([n_seq, d], WS_POOL)
// for the caller's final LayerNorm; `pooled_out` reports that.
struct PoolBufs { uint16_t *Hc, *D1c, *H2c, *MLPc, *D2c; };
PoolBufs pool_bufs(tvc_handle* h, const tvc_tower_arch& a, int n_seq, int wso) {
    uint16_t* p = (uint16_t*)h->ws[WS_POOL + wso].p;
    const size_t nd = ((size_t)n_seq + 256) * a.width;            // rows padded to a GEMM tile
    PoolBufs b;
    b.Hc = p; b.D1c = p + nd; b.H2c = p + 2 * nd; b.D2c = p + 3 * nd; b.MLPc = p + 4 * nd;
    return b;
}
size_t pool_bytes(const tvc_tower_arch& a, int n_seq) {
    return (((size_t)n_seq + 256) * a.width * 4 + ((size_t)n_seq + 256) * a.mlp) * 2;
}

// Input-gradient mode: what the backward of a layer reads is KEPT per layer instead of recomputed (288 GB of HBM:
// 20 * width bytes per token row and layer -- 3.9 GB at ViT-L/14, 32 images): the layer's fp32 input rows, its QKV
// rows, its out-projection output (ln_2's second operand) and the FC1 pre-activation.
struct GradSave {
    float* x;          // [layers][rows, d]      fp32
    uint16_t* qkv;     // [layers][rows, 3d]     bf16
    uint16_t* d1;      // [layers][rows, d]      bf16
    uint16_t* u;       // [layers][rows, mlp]    bf16
};

int run_layers(tvc_handle* h, const tvc_tower_arch& a, const tvc_layer_weights* lw, int n_seq, int seq_len,
               int causal, const int32_t* starts, int total_rows, int wso, hipStream_t st,
               const int32_t* pfx = nullptr, int pool_mode = 0, const int32_t* pool_row = nullptr,
               int64_t pool_x_stride = 0, const GradSave* gs = nullptr, bool f16 = false) {
    // f16 (TVC_OPT_TOWER_PRECISION = 3): lw holds IEEE fp16 GEMM weights; every 16-bit activation below is fp16, the
    // products run on the f16 MFMA.  Same launches, shapes and workspaces as the bf16 loop.
    const int d = a.width;
    const int rows = starts ? total_rows : n_seq * seq_len;
    float* X = (float*)h->ws[WS_X + wso].p;
    uint16_t* H = (uint16_t*)h->ws[WS_H + wso].p;
    uint16_t* QKV = (uint16_t*)h->ws[WS_QKV + wso].p;
    uint16_t* MLP = (uint16_t*)h->ws[WS_MLP + wso].p;
    uint16_t* D1 = (uint16_t*)h->ws[WS_DELTA + wso].p;     // attention out-proj output
    uint16_t* D2 = (uint16_t*)h->ws[WS_DELTA2 + wso].p;    // MLP fc2 output
    // The residual projections (attention out-proj, MLP fc2) are store-only GEMMs writing bf16
    // deltas; LayerNorm passes fold them into the fp32 residual stream X while they normalise (a
    // streaming kernel at the HBM roofline instead of a read-modify-write epilogue inside an
    // MFMA-bound kernel).  X is rewritten ONCE per layer: ln_2 normalises X + D1 without storing
    // it, the next ln_1 reads X + D1 + D2 (same fp32 sums, same order) and stores that.  The last
    // layer's two deltas are left pending for the caller's final LayerNorm (ln_post / ln_final).
    bool pending = false;
    for (int l = 0; l < a.layers; ++l) {
        const tvc_layer_weights& w = lw[l];
        {
            // D1 still points at the PREVIOUS layer's out-projection output here
            ProfScope ps(h, st, TVC_PROF_ROWOPS, (double)rows * d * (pending ? 14.0 : 6.0));
            // gradient mode keeps the residual stream as layer l sees it (X + the pending deltas): ln_1 writes it to the
            // kept buffer while it normalises (`xsum_out`) -- no separate device-to-device copy of X per layer
            HIP_TRY(launch_layernorm(X, d, nullptr, pending ? D1 : nullptr, 1, w.ln1_g, w.ln1_b, H, rows, d, st,
                                     pending ? D2 : nullptr, 0, gs ? gs->x + (size_t)l * rows * d : nullptr, nullptr, f16));
        }
        if (gs) {
            QKV = gs->qkv + (size_t)l * rows * 3 * d;
            D1 = gs->d1 + (size_t)l * rows * d;
        }
        GemmLaunch g = gemm_launch(w.wqkv, d, 3 * d, H, d, rows, d, w.bqkv, QKV, 3 * d, TVC_EPI_BF16);
        g.b_rows_padded = true; g.f16 = f16;
        g.splitk_small = gs != nullptr;            // gradient mode only (see tvc_encode_image_backward)
        HIP_TRY(timed_gemm(h, g, st, WS_SPLITK + wso));
        if (pool_mode && l == a.layers - 1) {
            const PoolBufs pb = pool_bufs(h, a, n_seq, wso);
            {
                const double avg_len = starts ? (double)rows / n_seq : (double)seq_len;
                ProfScope ps(h, st, TVC_PROF_ATTENTION, 4.0 * n_seq * a.heads * avg_len * 64);
                HIP_TRY(launch_attention(QKV, pb.Hc, starts, n_seq, seq_len, a.heads, causal, st, pfx, pool_mode, pool_row, f16));
            }
            g = gemm_launch(w.wo, d, d, pb.Hc, d, n_seq, d, w.bo, pb.D1c, d, TVC_EPI_BF16);
            g.b_rows_padded = true; g.f16 = f16;
            HIP_TRY(timed_gemm(h, g, st, WS_SPLITK + wso));
            HIP_TRY(launch_layernorm(X, pool_row ? d : pool_x_stride, pool_row, pb.D1c, 0, w.ln2_g, w.ln2_b, pb.H2c, n_seq, d,
                                     st, nullptr, 1, nullptr, nullptr, f16));
            g = gemm_launch(w.w1, d, a.mlp, pb.H2c, d, n_seq, d, w.b1, pb.MLPc, a.mlp,
                            a.act == TVC_ACT_GELU ? TVC_EPI_BF16 : TVC_EPI_GELU_BF16);
            g.b_rows_padded = true; g.f16 = f16;
            HIP_TRY(timed_gemm(h, g, st, WS_SPLITK + wso));
            if (a.act == TVC_ACT_GELU)
                HIP_TRY(launch_gelu_erf_16(pb.MLPc, (int64_t)n_seq * a.mlp, f16, st));
            g = gemm_launch(w.w2, a.mlp, d, pb.MLPc, a.mlp, n_seq, a.mlp, w.b2, pb.D2c, d, TVC_EPI_BF16);
            g.b_rows_padded = true; g.f16 = f16;
            HIP_TRY(timed_gemm(h, g, st, WS_SPLITK + wso));
            return TVC_OK;
        }
        {
            const double avg_len = starts ? (double)rows / n_seq : (double)seq_len;
            const double fl = 4.0 * n_seq * a.heads * avg_len * avg_len * 64 * (causal ? 0.5 : 1.0);
            ProfScope ps(h, st, TVC_PROF_ATTENTION, fl);
            HIP_TRY(launch_attention(QKV, H, starts, n_seq, seq_len, a.heads, causal, st, pfx, 0, nullptr, f16));
        }
        g = gemm_launch(w.wo, d, d, H, d, rows, d, w.bo, D1, d, TVC_EPI_BF16);
        g.b_rows_padded = true; g.f16 = f16; g.splitk_small = gs != nullptr;
        HIP_TRY(timed_gemm(h, g, st, WS_SPLITK + wso));
        {
            ProfScope ps(h, st, TVC_PROF_ROWOPS, (double)rows * d * 8.0);
            HIP_TRY(launch_layernorm(X, d, nullptr, D1, 0, w.ln2_g, w.ln2_b, H, rows, d, st, nullptr, 0, nullptr, nullptr, f16));
        }
        // FC1 fuses QuickGELU into its epilogue.  Gradient mode keeps the pre-activation U (what gelu' needs) and erf GELU (the
        // SD-2.x text encoder) has no fused form: both store only, the activation is one streaming pass after the GEMM
        uint16_t* U = gs ? gs->u + (size_t)l * rows * a.mlp : MLP;
        g = gemm_launch(w.w1, d, a.mlp, H, d, rows, d, w.b1, U, a.mlp, gs || a.act == TVC_ACT_GELU ? TVC_EPI_BF16 : TVC_EPI_GELU_BF16);
        g.b_rows_padded = true; g.f16 = f16; g.splitk_small = gs != nullptr;
        HIP_TRY(timed_gemm(h, g, st, WS_SPLITK + wso));
        if (gs) {
            HIP_TRY(launch_gelu_fwd(U, MLP, (int64_t)rows * a.mlp, st));
        } else if (a.act == TVC_ACT_GELU) {
            ProfScope ps(h, st, TVC_PROF_ROWOPS, (double)rows * a.mlp * 4.0);
            HIP_TRY(launch_gelu_erf_16(MLP, (int64_t)rows * a.mlp, f16, st));
        }
        g = gemm_launch(w.w2, a.mlp, d, MLP, a.mlp, rows, a.mlp, w.b2, D2, d, TVC_EPI_BF16);
        g.b_rows_padded = true; g.f16 = f16; g.splitk_small = gs != nullptr;
        HIP_TRY(timed_gemm(h, g, st, WS_SPLITK + wso));
        pending = true;
    }
    return TVC_OK;
}

int ensure_tower_ws(tvc_handle* h, const tvc_tower_arch& a, int64_t rows, int n_seq, int wso) {
    int rc;
    // GEMM operands get readable rows up to the next multiple of 256 (+ one tile): the 64-deep ring form stages
    // whole 256-row tiles without clamping; what it reads beyond the last row only reaches outputs never stored
    rows = (rows + 255) / 256 * 256 + 256;
    if ((rc = ensure(h, (Slot)(WS_X + wso), (size_t)rows * a.width * 4))) return rc;
    if ((rc = ensure(h, (Slot)(WS_H + wso), (size_t)rows * a.width * 2))) return rc;
    if ((rc = ensure(h, (Slot)(WS_QKV + wso), (size_t)rows * a.width * 3 * 2))) return rc;
    if ((rc = ensure(h, (Slot)(WS_MLP + wso), (size_t)rows * a.mlp * 2))) return rc;
    if ((rc = ensure(h, (Slot)(WS_CLS + wso), (size_t)n_seq * a.width * 2))) return rc;
    if ((rc = ensure(h, (Slot)(WS_DELTA + wso), (size_t)rows * a.width * 2))) return rc;
    if ((rc = ensure(h, (Slot)(WS_DELTA2 + wso), (size_t)rows * a.width * 2))) return rc;
    // fp32 partial tiles of the split-K paths (<= 256 partial tiles of 256 KiB): small batches split
    // every tile over K, big ones (opt-in) the left-over tile columns
    if ((rc = ensure(h, (Slot)(WS_SPLITK + wso), (size_t)256 * 256 * 256 * 4))) return rc;
    if ((rc = ensure(h, (Slot)(WS_POOL + wso), pool_bytes(a, n_seq)))) return rc;
    return TVC_OK;
}

// The bf16 / fp16 stem: im2col + patch GEMM of n images -> patch_out fp32 [n * P, d] (fn names the caller in errors)
int patch_stem(tvc_handle* h, const char* fn, const float* pix, int n, bool f16, const float** patch_out, hipStream_t st) {
    const tvc_model_desc& m = h->desc;
    const int gside = m.image_size / m.patch, P = gside * gside, d = m.vision.width;
    const int Kp = (3 * m.patch * m.patch + 63) / 64 * 64;
    uint16_t* Pm = (uint16_t*)h->ws[WS_PATCH].p;
    float* po = (float*)h->ws[WS_MLP].p;    // [n*P, d] fp32 fits: mlp >= 2*d
    if ((size_t)n * P * d * 4 > h->ws[WS_MLP].n) return fail(h, TVC_E_INVALID, std::string(fn) + ": mlp < 2*width unsupported");
    HIP_TRY(launch_im2col(pix, Pm, n, m.image_size, m.patch, Kp, st, f16));
    GemmLaunch g = gemm_launch((f16 ? h->vision16 : h->vision).w.patch_w, Kp, d, Pm, Kp, n * P, Kp, nullptr, po, d, TVC_EPI_F32);
    g.b_rows_padded = true; g.f16 = f16;
    HIP_TRY(timed_gemm(h, g, st, WS_SPLITK));
    *patch_out = po;
    return TVC_OK;
}

// ---- what the tower encode drivers ask of the precision mode (TVC_OPT_TOWER_PRECISION): its weights, stem, layer loop
// and head -- 0 (bf16) and 3 (the same launches on the fp16 weight set) here, 1 in tvc_precise.cpp, 2 in tvc_split.cpp.
// Mode 1 runs dense; mode 2 packs text rows but has no pooled last layer.

// TVC_E_STATE unless the mode's weights of the tower are registered; then sizes the mode's workspace for passes of up to
// n_seq sequences.  X: the fp32 residual stream the embeddings go to.
int tower_begin(tvc_handle* h, bool text, const char* fn, int n_seq, float** X) {
    const int mode = h->tower_precision;
    auto missing = [&](const char* tail) {      // modes 1 and 2 name the tower's encode call, mode 3 the entry point
        return fail(h, TVC_E_STATE, std::string(mode == 3 ? fn : text ? "tvc_encode_text" : "tvc_encode_image") +
                                        ": TVC_OPT_TOWER_PRECISION = " + std::to_string(mode) + " needs tvc_set_weights_f" +
                                        (mode == 3 ? "16" : "32") + (text ? " (text)" : " (vision)") + tail);
    };
    const bool has32 = text ? h->text32.set : h->vision32.set;
    if (mode == 1) return has32 ? precise_ensure(h, text, n_seq, X) : missing("");
    if (mode == 2) {
        if (!has32 || !h->split_ready || (text ? h->tsplit : h->vsplit).empty()) return missing(" before the option is set");
        return split_ensure(h, text, n_seq, X);
    }
    if (mode == 3 && !(text ? h->text16.set : h->vision16.set)) return missing("");
    const tvc_model_desc& m = h->desc;
    const int gside = m.image_size / m.patch, P = gside * gside, T = P + 1;
    const int Kp = (3 * m.patch * m.patch + 63) / 64 * 64;
    int rc;
    if (text) {
        if ((rc = ensure_tower_ws(h, m.text, (int64_t)n_seq * m.ctx, n_seq, WS_TOWER_N))) return rc;
    } else {
        if ((rc = ensure_tower_ws(h, m.vision, (int64_t)n_seq * T, n_seq, 0))) return rc;
        if ((rc = ensure(h, WS_PATCH, ((size_t)n_seq * P + 512) * Kp * 2))) return rc;      // + tile padding, as ensure_tower_ws
    }
    *X = (float*)h->ws[WS_X + (text ? WS_TOWER_N : 0)].p;
    return TVC_OK;
}

// pool (modes 0, 3): the last layer computes only the pooled row of every sequence, at X + row_idx[s] * x_stride (text:
// the EOT rows) or X + s * x_stride (vision: the class rows)
int tower_layers(tvc_handle* h, bool text, int n_seq, int seq_len, const int32_t* starts, int total_rows, const int32_t* pfx,
                 bool pool, int64_t x_stride, const int32_t* row_idx, hipStream_t st) {
    if (h->tower_precision == 1) return precise_layers(h, text, n_seq, seq_len, st);
    if (h->tower_precision == 2) return split_layers(h, text, n_seq, seq_len, starts, total_rows, pfx, st);
    const bool f16 = h->tower_precision == 3;
    const tvc_layer_weights* lw = text ? (f16 ? h->text16 : h->text).w.layers : (f16 ? h->vision16 : h->vision).w.layers;
    return run_layers(h, text ? h->desc.text : h->desc.vision, lw, n_seq, seq_len, text ? 1 : 0, starts, total_rows,
                      text ? WS_TOWER_N : 0, st, pfx, pool ? (text ? 2 : 1) : 0, row_idx, x_stride, nullptr, f16);
}

// final LayerNorm (ln_post / ln_final) of `rows` rows of X, folding in the last layer's two pending deltas, then the
// projection to out [rows, embed_dim]; hidden: the LayerNorm's fp32 rows to out instead
int tower_head(tvc_handle* h, bool text, int64_t x_stride, const int32_t* row_idx, int rows, bool pool, float* out, bool hidden,
               hipStream_t st) {
    if (h->tower_precision == 1) return precise_head(h, text, x_stride, row_idx, rows, out, hidden, st);
    if (h->tower_precision == 2) return split_head(h, text, x_stride, row_idx, rows, out, hidden, st);
    const bool f16 = h->tower_precision == 3;
    const tvc_model_desc& m = h->desc;
    const tvc_tower_arch& a = text ? m.text : m.vision;
    const int d = a.width, wso = text ? WS_TOWER_N : 0;
    const tvc_vision_weights& vw = (f16 ? h->vision16 : h->vision).w;
    const tvc_text_weights& tw = (f16 ? h->text16 : h->text).w;
    const PoolBufs pb = pool ? pool_bufs(h, a, rows, wso) : PoolBufs{};    // a pooled last layer's deltas: compact, output row order
    uint16_t* Hc = hidden ? nullptr : (uint16_t*)h->ws[WS_CLS + wso].p;
    HIP_TRY(launch_layernorm((float*)h->ws[WS_X + wso].p, x_stride, row_idx, pool ? pb.D1c : (const uint16_t*)h->ws[WS_DELTA + wso].p,
                             0, text ? tw.ln_final_g : vw.ln_post_g, text ? tw.ln_final_b : vw.ln_post_b, Hc, rows, d, st,
                             pool ? pb.D2c : (const uint16_t*)h->ws[WS_DELTA2 + wso].p, pool ? 1 : 0, nullptr,
                             hidden ? out : nullptr, f16));
    if (hidden) return TVC_OK;
    GemmLaunch g = gemm_launch(text ? tw.proj : vw.proj, d, m.embed_dim, Hc, d, rows, d, nullptr, out, m.embed_dim, TVC_EPI_F32);
    g.f16 = f16;
    HIP_TRY(timed_gemm(h, g, st, WS_SPLITK + wso));
    return TVC_OK;
}

// tvc_encode_text (pooled embeddings to out_dev) and, hidden, tvc_encode_text_hidden (ln_final at every position of the
// dense rows -> out_dev [Tn, ctx, width])
int encode_text(tvc_handle* h, const char* fn, const int32_t* tok_dev, int32_t Tn, float* out_dev, int32_t normalize, bool hidden,
                void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!h->text.set) return fail(h, TVC_E_STATE, std::string(fn) + ": handle has no text tower");
    if (Tn < 0 || (Tn > 0 && (!tok_dev || !out_dev))) return fail(h, TVC_E_INVALID, std::string(fn) + ": bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const tvc_model_desc& m = h->desc;
    const int d = m.text.width, ctx = m.ctx;
    if (Tn == 0) return TVC_OK;
    int chunk = Tn < h->max_chunk_texts ? Tn : h->max_chunk_texts;
    const int mode = h->tower_precision;
    // every position is an output of a hidden-state call (the conditioning sequence of a latent-diffusion UNet): dense
    // rows, no EOT packing, no pooling; the causal mask is the tower's own
    const bool pack = h->pack_text && !hidden && mode != 1;
    const bool pool = h->pooled_last && !hidden && (mode == 0 || mode == 3);      // only the EOT row of every text is pooled
    // prefix sharing needs whole groups in a pass
    const int G = (pack && h->text_group >= 2 && Tn % h->text_group == 0) ? h->text_group : 0;
    if (G && chunk >= G) chunk = chunk / G * G;
    const bool share = G && chunk % G == 0;
    float* X;
    int rc;
    if ((rc = tower_begin(h, true, fn, chunk, &X))) return rc;
    if (share && (rc = ensure(h, WS_PFX, (size_t)chunk * 2 * 4))) return rc;
    if ((rc = ensure(h, WS_EOT, (size_t)chunk * 4))) return rc;
    if (pack && (rc = ensure(h, WS_STARTS, (size_t)(chunk + 2) * 4))) return rc;
    if (pack && (rc = ensure(h, WS_LENS, (size_t)chunk * 4))) return rc;
    int32_t* eot = (int32_t*)h->ws[WS_EOT].p;
    for (int t0 = 0; t0 < Tn; t0 += chunk) {
        const int n = (Tn - t0 < chunk) ? Tn - t0 : chunk;
        const int32_t* tok = tok_dev + (size_t)t0 * ctx;
        const int32_t* starts = nullptr;
        const int32_t* pfx = nullptr;
        int total_rows = n * ctx, max_len = ctx;
        if (pack) {
            // Keep only the tokens up to and including EOT: under the causal mask the later
            // positions cannot reach the pooled (EOT) row, so the result is bit-identical.
            // The row count sizes the GEMM grids, hence ONE 8-byte read-back per call.
            int32_t* sd = (int32_t*)h->ws[WS_STARTS].p;
            int32_t* pd = share ? (int32_t*)h->ws[WS_PFX].p : nullptr;
            HIP_TRY(launch_text_lens_scan(tok, sd, pd, n, ctx, G, st, (int32_t*)h->ws[WS_LENS].p));
            pfx = pd;
            int32_t tail[2] = {0, 0};
            HIP_TRY(hipMemcpyAsync(tail, sd + n, sizeof tail, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            total_rows = tail[0]; max_len = tail[1];
            if (total_rows < (share ? n / G : n) || total_rows > n * ctx || max_len < 1 || max_len > ctx)
                return fail(h, TVC_E_HIP, "tvc_encode_text: inconsistent sequence lengths");
            starts = sd;
        }
        auto embed = [&](const auto& w) {
            return launch_text_embed(tok, w.tok_emb, w.pos, X, eot, starts, n, ctx, d, m.vocab, st, pfx);
        };
        HIP_TRY(mode == 1 || mode == 2 ? embed(h->text32.w) : embed((mode == 3 ? h->text16 : h->text).w));
        if ((rc = tower_layers(h, true, n, max_len, starts, total_rows, pfx, pool, d, eot, st))) return rc;
        if (hidden) {
            if ((rc = tower_head(h, true, d, nullptr, n * ctx, false, out_dev + (size_t)t0 * ctx * d, true, st))) return rc;
            continue;
        }
        float* out = out_dev + (size_t)t0 * m.embed_dim;
        if ((rc = tower_head(h, true, d, eot, n, pool, out, false, st))) return rc;
        if (normalize) HIP_TRY(launch_l2norm_rows(out, n, m.embed_dim, st));
    }
    return TVC_OK;
}

}  // namespace

extern "C" {

uint32_t tvc_abi_version(void) { return TVC_ABI_VERSION; }

const char* tvc_last_error(tvc_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int tvc_create(const tvc_model_desc* desc, const tvc_vision_weights* vision, const tvc_text_weights* text,
               tvc_handle** out) {
    tvc_handle* h = nullptr;   // for HIP_TRY / fail before the handle exists
    if (!out) return fail(h, TVC_E_INVALID, "tvc_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(h, TVC_E_HIP, "tvc_create: no HIP device visible (the TVC path has no CPU fallback)");
    if ((vision || text) && !desc) return fail(h, TVC_E_INVALID, "tvc_create: weights given without a model desc");
    tvc_handle* nh = new tvc_handle();
    if (desc) nh->desc = *desc;
    if (vision) {
        const tvc_model_desc& d = *desc;
        const int Kraw = 3 * d.patch * d.patch;
        if (!tower_ok(d.vision) || d.patch <= 0 || d.image_size % d.patch != 0 || d.embed_dim % 64 != 0 ||
            Kraw <= 0 || !vision->layers) {
            delete nh;
            return fail(h, TVC_E_INVALID, "tvc_create: unsupported vision geometry (head_dim must be 64, width<=1024)");
        }
        const int T = (d.image_size / d.patch) * (d.image_size / d.patch) + 1;
        if (T > 288) { delete nh; return fail(h, TVC_E_INVALID, "tvc_create: vision sequence longer than 288 tokens"); }
        nh->vision.assign(*vision, d.vision.layers);
    }
    if (text) {
        const tvc_model_desc& d = *desc;
        if (!tower_ok(d.text) || d.ctx <= 0 || d.ctx > 288 || d.vocab <= 0 || d.embed_dim % 64 != 0 || !text->layers) {
            delete nh;
            return fail(h, TVC_E_INVALID, "tvc_create: unsupported text geometry");
        }
        nh->text.assign(*text, d.text.layers);
    }
    *out = nh;
    return TVC_OK;
}

void tvc_destroy(tvc_handle* h) {
    if (!h) return;
    tvc_sd_free(h);
    tvc_split_free(h);
    for (auto& b : h->ws) if (b.p) (void)hipFree(b.p);
    for (void* p : h->wT) if (p) (void)hipFree(p);
    for (auto& bk : h->banks) {
        if (bk.owned) (void)hipFree(bk.owned);
        if (bk.bounds) (void)hipFree(bk.bounds);
    }
    delete h;
}

uint64_t tvc_workspace_bytes(tvc_handle* h) {
    if (!h) return 0;
    uint64_t n = 0;
    for (auto& b : h->ws) n += b.n;
    return n;
}

int tvc_encode_image(tvc_handle* h, const float* pix_dev, int32_t B, float* out_dev, int32_t normalize,
                     void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!h->vision.set) return fail(h, TVC_E_STATE, "tvc_encode_image: handle has no vision tower");
    if (B < 0 || (B > 0 && (!pix_dev || !out_dev))) return fail(h, TVC_E_INVALID, "tvc_encode_image: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const tvc_model_desc& m = h->desc;
    const int gside = m.image_size / m.patch, T = gside * gside + 1, d = m.vision.width;
    const int chunk = B < h->max_chunk_images ? B : h->max_chunk_images;
    if (B == 0) return TVC_OK;
    const int mode = h->tower_precision;
    const bool pool = h->pooled_last && (mode == 0 || mode == 3);      // only the class token (row b*T) is pooled
    float* X;
    int rc;
    if ((rc = tower_begin(h, false, "tvc_encode_image", chunk, &X))) return rc;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int n = (B - b0 < chunk) ? B - b0 : chunk;
        const float* pix = pix_dev + (size_t)b0 * 3 * m.image_size * m.image_size;
        const float* patch_out;
        rc = mode == 1 ? precise_stem(h, pix, n, &patch_out, st) : mode == 2 ? split_stem(h, pix, n, &patch_out, st)
                       : patch_stem(h, "tvc_encode_image", pix, n, mode == 3, &patch_out, st);
        if (rc) return rc;
        auto assemble = [&](const auto& w) {
            return launch_assemble_lnpre(patch_out, w.cls, w.pos, w.ln_pre_g, w.ln_pre_b, X, n, T, d, st);
        };
        HIP_TRY(mode == 1 || mode == 2 ? assemble(h->vision32.w) : assemble((mode == 3 ? h->vision16 : h->vision).w));
        if ((rc = tower_layers(h, false, n, T, nullptr, 0, nullptr, pool, (int64_t)T * d, nullptr, st))) return rc;
        float* out = out_dev + (size_t)b0 * m.embed_dim;
        if ((rc = tower_head(h, false, (int64_t)T * d, nullptr, n, pool, out, false, st))) return rc;
        if (normalize) HIP_TRY(launch_l2norm_rows(out, n, m.embed_dim, st));
    }
    return TVC_OK;
}

int tvc_encode_text(tvc_handle* h, const int32_t* tok_dev, int32_t Tn, float* out_dev, int32_t normalize,
                    void* stream) {
    return encode_text(h, "tvc_encode_text", tok_dev, Tn, out_dev, normalize, false, stream);
}

int tvc_encode_text_hidden(tvc_handle* h, const int32_t* tok_dev, int32_t Tn, float* out_dev, void* stream) {
    return encode_text(h, "tvc_encode_text_hidden", tok_dev, Tn, out_dev, 0, true, stream);
}

int tvc_bank_set(tvc_handle* h, const void* bank_dev, int64_t R, int32_t D, int32_t dtype, void* stream) {
    if (!h) return TVC_E_INVALID;
    BankSlot& bk = h->banks[h->cur_bank];
    if (R < 0 || R > 0x7fffffffLL || D <= 0 || D % 64 != 0 || (R > 0 && !bank_dev))
        return fail(h, TVC_E_INVALID, "tvc_bank_set: need 0 <= R < 2^31 and D % 64 == 0");
    if (bk.owned) { HIP_TRY(hipFree(bk.owned)); bk.owned = nullptr; }
    bk.bank = nullptr; bk.R = 0; bk.D = D;
    if (dtype == TVC_DTYPE_BF16) {
        bk.bank = (const uint16_t*)bank_dev; bk.planes = 1;
    } else if (dtype == TVC_DTYPE_F32) {
        if (R > 0) {
            HIP_TRY(hipMalloc(&bk.owned, (size_t)R * 2 * D * 2));
            HIP_TRY(launch_split_planes((const float*)bank_dev, (uint16_t*)bk.owned, R, D, 2, (hipStream_t)stream));
        }
        bk.bank = (const uint16_t*)bk.owned; bk.planes = 2;
    } else {
        return fail(h, TVC_E_INVALID, "tvc_bank_set: dtype must be TVC_DTYPE_BF16 or TVC_DTYPE_F32");
    }
    if (!bk.bounds) HIP_TRY(hipMalloc((void**)&bk.bounds, 8));
    BankRows rows = bank_rows(bk);
    rows.R = R;                       // the slot holds them only once their bounds are under way
    HIP_TRY(launch_bank_bounds(rows, bk.bounds, (hipStream_t)stream));
    bk.R = R;
    return TVC_OK;
}

int tvc_bank_select(tvc_handle* h, int32_t slot) {
    if (!h) return TVC_E_INVALID;
    if (slot < 0 || slot >= TVC_MAX_BANKS) return fail(h, TVC_E_INVALID, "tvc_bank_select: slot must be in [0, TVC_MAX_BANKS)");
    h->cur_bank = slot;
    return TVC_OK;
}

int tvc_bank_search(tvc_handle* h, const float* rows_dev, int32_t M, int32_t k, float count_thr,
                    int64_t idx_offset, int32_t* topk_idx_dev, float* topk_sim_dev, float* moments_dev,
                    void* stream) {
    if (!h) return TVC_E_INVALID;
    BankSlot& bk = h->banks[h->cur_bank];
    if (!bk.bank && bk.R != 0) return fail(h, TVC_E_STATE, "tvc_bank_search: no bank registered");
    if (bk.D == 0) return fail(h, TVC_E_STATE, "tvc_bank_search: call tvc_bank_set first");
    if (M < 0 || k < 1 || k > TVC_MAX_TOPK || (M > 0 && (!rows_dev || !topk_idx_dev || !topk_sim_dev)))
        return fail(h, TVC_E_INVALID, "tvc_bank_search: need 1 <= k <= 128 and non-NULL buffers");
    if (M == 0) return TVC_OK;
    hipStream_t st = (hipStream_t)stream;
    const int D = bk.D;
    if (bk.R == 0) {
        // empty bank: retrieval_ref.py:195-197 returns no references
        HIP_TRY(hipMemsetAsync(topk_idx_dev, 0xff, (size_t)M * k * 4, st));
        HIP_TRY(hipMemsetAsync(topk_sim_dev, 0, (size_t)M * k * 4, st));
        if (moments_dev) HIP_TRY(hipMemsetAsync(moments_dev, 0, (size_t)M * 16, st));
        return TVC_OK;
    }
    BankSearchLaunch L;
    bank_plan(bk.R, M, k, &L.n_sample, &L.sample_stride, &L.S, &L.cap);
    int rc;
    if ((rc = ensure_planes(h, WS_QPLANES, M, 256, D))) return rc;
    if ((rc = ensure(h, WS_S0, (size_t)M * (L.n_sample > 256 ? L.n_sample : 256) * 4))) return rc;
    if ((rc = ensure(h, WS_TAU, (size_t)M * 4))) return rc;
    if ((rc = ensure(h, WS_CAND, (size_t)L.S * M * L.cap * 8))) return rc;
    if ((rc = ensure(h, WS_CAND_CNT, (size_t)L.S * M * 4))) return rc;
    if ((rc = ensure(h, WS_MOM_PART, (size_t)L.S * M * 16))) return rc;
    if ((rc = ensure(h, WS_OVERFLOW, 16))) return rc;
    if ((rc = split_planes(h, WS_QPLANES, rows_dev, M, D, st, &L.qplanes))) return rc;
    L.bank = bank_rows(bk);
    L.q_rows_padded = true; L.M = M; L.k = k; L.count_thr = count_thr;
    L.idx_offset = idx_offset;
    L.rows = rows_dev; L.bank_bounds = bk.bounds; L.allow_filter = h->bank_filter;
    L.s0 = (float*)h->ws[WS_S0].p; L.gmax = L.s0; L.tau = (float*)h->ws[WS_TAU].p; L.cand = h->ws[WS_CAND].p;
    L.cand_cnt = (int32_t*)h->ws[WS_CAND_CNT].p; L.mom_part = (float*)h->ws[WS_MOM_PART].p;
    L.overflow = (int32_t*)h->ws[WS_OVERFLOW].p;
    L.topk_idx = topk_idx_dev; L.topk_sim = topk_sim_dev; L.moments = moments_dev;
    {
        const bool filter = !moments_dev && h->bank_filter && D <= 2048;
        const int planes = filter ? 1 : bank_products(bk.planes);
        ProfScope ps(h, st, TVC_PROF_BANK, slot_pass_flops(bk.R, M, D, planes));
        HIP_TRY(launch_bank_search(L, st));
    }
    return TVC_OK;
}

int tvc_bank_search_dense(tvc_handle* h, const float* rows_dev, int32_t M, int32_t k, float count_thr,
                          int64_t idx_offset, int32_t* topk_idx_dev, float* topk_sim_dev, float* moments_dev,
                          void* stream) {
    if (!h) return TVC_E_INVALID;
    BankSlot& bk = h->banks[h->cur_bank];
    if (bk.D == 0 || (!bk.bank && bk.R != 0)) return fail(h, TVC_E_STATE, "tvc_bank_search_dense: call tvc_bank_set first");
    if (M < 0 || k < 1 || k > TVC_MAX_TOPK || (M > 0 && (!rows_dev || !topk_idx_dev || !topk_sim_dev)))
        return fail(h, TVC_E_INVALID, "tvc_bank_search_dense: need 1 <= k <= 128 and non-NULL buffers");
    if (M == 0) return TVC_OK;
    if (bk.R == 0) return tvc_bank_search(h, rows_dev, M, k, count_thr, idx_offset, topk_idx_dev, topk_sim_dev, moments_dev, stream);
    hipStream_t st = (hipStream_t)stream;
    const int D = bk.D;
    int block = (int)((size_t)1 << 28) / (int)(bk.R > 0 ? bk.R : 1);      // <= 1 GiB of similarities at a time
    if (block > 64) block = 64;
    if (block < 1) block = 1;
    int rc;
    if ((rc = ensure_planes(h, WS_QPLANES, M, 256, D))) return rc;
    if ((rc = ensure(h, WS_S0, (size_t)block * bk.R * 4))) return rc;
    BankSearchLaunch L;
    if ((rc = split_planes(h, WS_QPLANES, rows_dev, M, D, st, &L.qplanes))) return rc;
    L.bank = bank_rows(bk);
    L.q_rows_padded = true; L.M = M; L.k = k; L.count_thr = count_thr;
    L.idx_offset = idx_offset;
    L.topk_idx = topk_idx_dev; L.topk_sim = topk_sim_dev; L.moments = moments_dev;
    HIP_TRY(launch_bank_search_dense(L, (float*)h->ws[WS_S0].p, block, st));
    return TVC_OK;
}

int tvc_bank_status(tvc_handle* h, void* stream) {
    if (!h) return TVC_E_INVALID;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (!h->ws[WS_OVERFLOW].p) return TVC_OK;
    int32_t flag = 0;
    HIP_TRY(hipMemcpy(&flag, h->ws[WS_OVERFLOW].p, sizeof flag, hipMemcpyDeviceToHost));
    if (flag) {
        char m[160];
        snprintf(m, sizeof m, "tvc_bank_search: candidate lists overflowed (flag %d): bank has too many "
                              "near-identical rows for the sampled bound", flag);
        return fail(h, TVC_E_OVERFLOW, m);
    }
    return TVC_OK;
}

int tvc_bank_gather(tvc_handle* h, const int32_t* idx_dev, int32_t n, int64_t idx_offset, float* out_dev,
                    void* stream) {
    if (!h) return TVC_E_INVALID;
    BankSlot& bk = h->banks[h->cur_bank];
    if (bk.D == 0) return fail(h, TVC_E_STATE, "tvc_bank_gather: call tvc_bank_set first");
    if (n < 0 || (n > 0 && (!idx_dev || !out_dev))) return fail(h, TVC_E_INVALID, "tvc_bank_gather: bad arguments");
    if (n == 0) return TVC_OK;
    if (bk.R == 0) { HIP_TRY(hipMemsetAsync(out_dev, 0, (size_t)n * bk.D * 4, (hipStream_t)stream)); return TVC_OK; }
    HIP_TRY(launch_gather_rows(bank_rows(bk), idx_dev, idx_offset, n, out_dev, (hipStream_t)stream));
    return TVC_OK;
}

int tvc_topk_merge(tvc_handle* h, const int32_t* idx_parts_dev, const float* sim_parts_dev,
                   const float* feat_parts_dev, const float* mom_parts_dev, int32_t W, int32_t M, int32_t k,
                   int32_t kf, int32_t D, int32_t* idx_out_dev, float* sim_out_dev, float* feat_out_dev,
                   float* mom_out_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (M < 0 || !idx_parts_dev || !sim_parts_dev || !idx_out_dev || !sim_out_dev)
        return fail(h, TVC_E_INVALID, "tvc_topk_merge: bad arguments");
    if (W < 1 || k < 1 || k > TVC_MAX_TOPK || W * k > 256 || kf < 0 || kf > k || kf > 32 ||
        (kf > 0 && feat_parts_dev && (!feat_out_dev || D < 1)))
        return fail(h, TVC_E_INVALID, "tvc_topk_merge: limits are W * k <= 256, kf <= min(k, 32)");
    hipError_t st = launch_topk_merge(idx_parts_dev, sim_parts_dev, feat_parts_dev, mom_parts_dev, W, M, k, kf, D,
                                      idx_out_dev, sim_out_dev, feat_out_dev, mom_out_dev, (hipStream_t)stream);
    if (st != hipSuccess) return fail(h, st == hipErrorInvalidValue ? TVC_E_INVALID : TVC_E_HIP,
                                      std::string("tvc_topk_merge: ") + hipGetErrorString(st));
    return TVC_OK;
}

int tvc_cosine_matrix(tvc_handle* h, const float* x_dev, int32_t N, const float* y_dev, int32_t M, int32_t D,
                      float* out_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (N < 0 || M < 0 || D <= 0 || D % 64 != 0 || ((N > 0 && M > 0) && (!x_dev || !y_dev || !out_dev)))
        return fail(h, TVC_E_INVALID, "tvc_cosine_matrix: need D % 64 == 0 and non-NULL buffers");
    if (N == 0 || M == 0) return TVC_OK;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = ensure(h, WS_COSX, (size_t)N * D * 4))) return rc;
    if ((rc = ensure(h, WS_COSY, (size_t)M * D * 4))) return rc;
    if ((rc = ensure_planes(h, WS_COSXP, N, 1, D))) return rc;
    if ((rc = ensure_planes(h, WS_COSYP, M, 1, D))) return rc;
    float* xn = (float*)h->ws[WS_COSX].p;
    float* yn = (float*)h->ws[WS_COSY].p;
    HIP_TRY(hipMemcpyAsync(xn, x_dev, (size_t)N * D * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(yn, y_dev, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(launch_l2norm_rows(xn, N, D, st));
    HIP_TRY(launch_l2norm_rows(yn, M, D, st));
    const uint16_t *xp, *yp;
    if ((rc = split_planes(h, WS_COSXP, xn, N, D, st, &xp))) return rc;
    if ((rc = split_planes(h, WS_COSYP, yn, M, D, st, &yp))) return rc;
    // out[n, m]: "A rows" (fast output dim) = y, "B rows" = x; hi.hi + hi.lo + lo.hi
    HIP_TRY(timed_gemm(h, gemm_launch_planes(yp, 2 * (int64_t)D, M, 2, xp, N, D, out_dev, M), st));
    return TVC_OK;
}

int tvc_consistency(tvc_handle* h, const float* img_dev, const float* txt_dev, int32_t B, int32_t N, int32_t D,
                    const int32_t* ref_idx_dev, const float* ref_sim_dev, const float* ref_feat_dev, int32_t ks,
                    int32_t kf, const tvc_consistency_params* params, float* rec_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (B < 0 || N < 0 || D <= 0 || !params || (B > 0 && (!img_dev || !txt_dev || !rec_dev)))
        return fail(h, TVC_E_INVALID, "tvc_consistency: bad arguments");
    if (ks > 0 && (!ref_idx_dev || !ref_sim_dev || !ref_feat_dev || kf < 1))
        return fail(h, TVC_E_INVALID, "tvc_consistency: ks > 0 needs ref_idx, ref_sim, ref_feat and kf >= 1");
    ConsistencyParams p;
    p.reference_count = params->reference_count;
    p.similarity_threshold = params->similarity_threshold;
    p.retrieval_top_k = params->retrieval_top_k;
    p.dup_threshold = params->dup_threshold;
    p.w_text_variants = params->w_text_variants;
    p.w_consistency = params->w_consistency;
    for (int i = 0; i < 4; ++i) p.w_exp[i] = params->w_exp[i];
    if (p.retrieval_top_k > TVC_REC_MAXREF || p.retrieval_top_k < 0 || p.reference_count < 0)
        return fail(h, TVC_E_INVALID, "tvc_consistency: retrieval_top_k must be in [0, 16]");
    hipError_t st = launch_consistency(img_dev, txt_dev, B, N, D, ref_idx_dev, ref_sim_dev, ref_feat_dev, ks, kf, p,
                                       rec_dev, tvc_rec_stride(N), (hipStream_t)stream);
    if (st != hipSuccess) return fail(h, st == hipErrorInvalidValue ? TVC_E_INVALID : TVC_E_HIP,
                                      std::string("tvc_consistency: ") + hipGetErrorString(st));
    return TVC_OK;
}

// ---- input gradient of the vision tower -------------------------------------------
namespace {
int build_transposed_weights(tvc_handle* h, hipStream_t st) {
    if (!h->wT.empty()) return TVC_OK;
    const tvc_model_desc& m = h->desc;
    const tvc_tower_arch& a = m.vision;
    const int d = a.width, Kp = (3 * m.patch * m.patch + 63) / 64 * 64;
    auto tr = [&](const uint16_t* w, int R, int C, void** out) -> int {
        HIP_TRY(hipMalloc(out, (size_t)R * C * 2));
        HIP_TRY(launch_transpose_bf16(w, (uint16_t*)*out, R, C, st));
        return TVC_OK;
    };
    std::vector<void*> t((size_t)a.layers * 4 + 2, nullptr);
    int rc = TVC_OK;
    for (int l = 0; l < a.layers && !rc; ++l) {
        const tvc_layer_weights& w = h->vision.w.layers[l];
        if ((rc = tr(w.wqkv, 3 * d, d, &t[l * 4 + 0]))) break;      // [3d, d] -> [d, 3d]
        if ((rc = tr(w.wo, d, d, &t[l * 4 + 1]))) break;
        if ((rc = tr(w.w1, a.mlp, d, &t[l * 4 + 2]))) break;        // [mlp, d] -> [d, mlp]
        if ((rc = tr(w.w2, d, a.mlp, &t[l * 4 + 3]))) break;        // [d, mlp] -> [mlp, d]
    }
    if (!rc) rc = tr(h->vision.w.proj, m.embed_dim, d, &t[(size_t)a.layers * 4]);           // [D, d] -> [d, D]
    if (!rc) rc = tr(h->vision.w.patch_w, d, Kp, &t[(size_t)a.layers * 4 + 1]);             // [d, Kp] -> [Kp, d]
    if (rc) { for (void* p : t) if (p) (void)hipFree(p); return rc; }
    h->wT = t;
    return TVC_OK;
}
}  // namespace

int tvc_encode_image_grad(tvc_handle* h, const float* pix_dev, int32_t B, float* out_dev, int32_t normalize, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!h->vision.set) return fail(h, TVC_E_STATE, "tvc_encode_image_grad: handle has no vision tower");
    if (B < 1 || !pix_dev || !out_dev) return fail(h, TVC_E_INVALID, "tvc_encode_image_grad: bad arguments");
    if (B > h->max_chunk_images) return fail(h, TVC_E_INVALID, "tvc_encode_image_grad: B exceeds TVC_OPT_MAX_CHUNK_IMAGES (one pass only)");
    if (h->desc.vision.act != TVC_ACT_QUICK_GELU) return fail(h, TVC_E_INVALID, "tvc_encode_image_grad: only QuickGELU towers have a backward pass");
    hipStream_t st = (hipStream_t)stream;
    if (h->grad_precision == 2) {            // the split-bf16 path (tvc_grad_split.cpp)
        h->grad_B = 0;                       // a failed forward leaves nothing for a backward
        const int rc2 = grad_split_forward(h, pix_dev, B, out_dev, normalize, st);
        if (rc2) return rc2;
        h->grad_B = B; h->grad_normalize = normalize; h->grad_pix = pix_dev; h->grad_mode = 2;
        return TVC_OK;
    }
    const tvc_model_desc& m = h->desc;
    const tvc_tower_arch& a = m.vision;
    const int gside = m.image_size / m.patch, P = gside * gside, T = P + 1, d = a.width;
    const int Kp = (3 * m.patch * m.patch + 63) / 64 * 64;
    const int64_t rows = (int64_t)B * T;
    int rc;
    if ((rc = ensure_tower_ws(h, a, rows, B, 0))) return rc;
    if ((rc = ensure(h, WS_PATCH, ((size_t)B * P + 512) * Kp * 2))) return rc;
    const size_t per_layer = (size_t)rows * ((size_t)d * 4 + (size_t)3 * d * 2 + (size_t)d * 2 + (size_t)a.mlp * 2);
    if ((rc = ensure(h, WS_GSAVE, (size_t)a.layers * per_layer + 256))) return rc;
    GradSave gs;
    gs.x = (float*)h->ws[WS_GSAVE].p;
    gs.qkv = (uint16_t*)(gs.x + (size_t)a.layers * rows * d);
    gs.d1 = gs.qkv + (size_t)a.layers * rows * 3 * d;
    gs.u = gs.d1 + (size_t)a.layers * rows * d;
    if ((rc = ensure(h, WS_GOUT, (size_t)B * m.embed_dim * 4))) return rc;
    if ((rc = ensure(h, WS_GXL, (size_t)B * d * 4))) return rc;
    const float* patch_out;
    if ((rc = patch_stem(h, "tvc_encode_image_grad", pix_dev, B, false, &patch_out, st))) return rc;
    const tvc_vision_weights& vw = h->vision.w;
    HIP_TRY(launch_assemble_lnpre(patch_out, vw.cls, vw.pos, vw.ln_pre_g, vw.ln_pre_b, (float*)h->ws[WS_X].p, B, T, d, st));
    if ((rc = run_layers(h, a, vw.layers, B, T, 0, nullptr, 0, 0, st, nullptr, 0, nullptr, 0, &gs))) return rc;
    uint16_t* Hc = (uint16_t*)h->ws[WS_CLS].p;
    HIP_TRY(launch_layernorm((float*)h->ws[WS_X].p, (int64_t)T * d, nullptr, gs.d1 + (size_t)(a.layers - 1) * rows * d, 0,
                             vw.ln_post_g, vw.ln_post_b, Hc, B, d, st, (const uint16_t*)h->ws[WS_DELTA2].p, 0,
                             (float*)h->ws[WS_GXL].p));
    HIP_TRY(timed_gemm(h, gemm_launch(vw.proj, d, m.embed_dim, Hc, d, B, d, nullptr, h->ws[WS_GOUT].p, m.embed_dim, TVC_EPI_F32), st,
                       WS_SPLITK));
    HIP_TRY(hipMemcpyAsync(out_dev, h->ws[WS_GOUT].p, (size_t)B * m.embed_dim * 4, hipMemcpyDeviceToDevice, st));
    if (normalize) HIP_TRY(launch_l2norm_rows(out_dev, B, m.embed_dim, st));
    h->grad_B = B; h->grad_normalize = normalize; h->grad_pix = pix_dev; h->grad_mode = 0;
    return TVC_OK;
}

int tvc_encode_image_backward(tvc_handle* h, const float* grad_out_dev, float* grad_pix_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!h->vision.set || h->grad_B < 1) return fail(h, TVC_E_STATE, "tvc_encode_image_backward: call tvc_encode_image_grad first");
    if (!grad_out_dev || !grad_pix_dev) return fail(h, TVC_E_INVALID, "tvc_encode_image_backward: NULL buffer");
    if (h->grad_mode != h->grad_precision)
        return fail(h, TVC_E_STATE, "tvc_encode_image_backward: TVC_OPT_GRAD_PRECISION changed since tvc_encode_image_grad (it ran in mode " +
                                        std::to_string(h->grad_mode) + "): a forward / backward pair runs in one mode");
    hipStream_t st = (hipStream_t)stream;
    if (h->grad_mode == 2) return grad_split_backward(h, grad_out_dev, grad_pix_dev, st);
    const tvc_model_desc& m = h->desc;
    const tvc_tower_arch& a = m.vision;
    const int B = h->grad_B, gside = m.image_size / m.patch, P = gside * gside, T = P + 1, d = a.width, D = m.embed_dim;
    const int Kp = (3 * m.patch * m.patch + 63) / 64 * 64;
    const int64_t rows = (int64_t)B * T;
    const int64_t rows_pad = (rows + 255) / 256 * 256 + 256;
    int rc;
    if ((rc = build_transposed_weights(h, st))) return rc;
    if ((rc = ensure(h, WS_GDX, (size_t)rows_pad * d * 4))) return rc;
    if ((rc = ensure(h, WS_G16, (size_t)rows_pad * d * 2))) return rc;
    if ((rc = ensure(h, WS_GMLP2, (size_t)rows_pad * a.mlp * 2))) return rc;
    if ((rc = ensure(h, WS_GDQKV, (size_t)rows_pad * 3 * d * 2))) return rc;
    if ((rc = ensure(h, WS_GSTATS, (size_t)rows * a.heads * 16))) return rc;
    if ((rc = ensure(h, WS_GSMALL, ((size_t)B + 256) * (D + d) * 2))) return rc;
    if ((rc = ensure(h, WS_GPATCH, ((size_t)B * P + 512) * (size_t)(Kp > d ? Kp : d) * 4))) return rc;
    uint16_t* H = (uint16_t*)h->ws[WS_H].p;
    uint16_t* D2 = (uint16_t*)h->ws[WS_DELTA2].p;
    float* dX = (float*)h->ws[WS_GDX].p;
    uint16_t* G16 = (uint16_t*)h->ws[WS_G16].p;
    uint16_t* dM = (uint16_t*)h->ws[WS_GMLP2].p;
    uint16_t* dQKV = (uint16_t*)h->ws[WS_GDQKV].p;
    auto gemm = [&](const void* A, int64_t lda, int I, const uint16_t* Bm, int64_t ldb, int J, int K, void* out, int64_t ldo,
                    int epi) -> int {
        GemmLaunch g = gemm_launch((const uint16_t*)A, lda, I, Bm, ldb, J, K, nullptr, out, ldo, epi);
        g.b_rows_padded = true;
        // the gradient path promises no batch-position invariance of its last bits: a partial last round of tiles (FC1-shaped
        // GEMMs at 32 images: 528 tiles = 2 rounds + 16 tiles) is split over K instead of taking a third round
        g.splitk_small = true;
        HIP_TRY(timed_gemm(h, g, st, WS_SPLITK));
        return TVC_OK;
    };
    // ---- head: L2 normalise, projection, ln_post (gradient lives on the class rows only)
    uint16_t* dP16 = (uint16_t*)h->ws[WS_GSMALL].p;                 // [B(+pad), D]
    uint16_t* dHc = dP16 + ((size_t)B + 256) * D;                   // [B(+pad), d]
    HIP_TRY(launch_l2norm_bwd((const float*)h->ws[WS_GOUT].p, grad_out_dev, dP16, B, D, h->grad_normalize, st));
    if ((rc = gemm(h->wT[(size_t)a.layers * 4], D, d, dP16, D, B, D, dHc, d, TVC_EPI_BF16))) return rc;
    HIP_TRY(hipMemsetAsync(dX, 0, (size_t)rows * d * 4, st));
    HIP_TRY(hipMemsetAsync(G16, 0, (size_t)rows * d * 2, st));
    HIP_TRY(launch_layernorm_bwd((const float*)h->ws[WS_GXL].p, d, nullptr, dHc, 0, h->vision.w.ln_post_g, nullptr, dX, G16, B, d,
                                 (int64_t)T * d, st));
    // ---- layers, last to first, on what the forward kept (GradSave)
    const float* sx = (const float*)h->ws[WS_GSAVE].p;
    const uint16_t* sqkv = (const uint16_t*)(sx + (size_t)a.layers * rows * d);
    const uint16_t* sd1 = sqkv + (size_t)a.layers * rows * 3 * d;
    const uint16_t* su = sd1 + (size_t)a.layers * rows * d;
    for (int l = a.layers - 1; l >= 0; --l) {
        const tvc_layer_weights& w = h->vision.w.layers[l];
        void* const* wt = &h->wT[(size_t)l * 4];
        const float* X = sx + (size_t)l * rows * d;
        const uint16_t* QKV = sqkv + (size_t)l * rows * 3 * d;
        const uint16_t* D1 = sd1 + (size_t)l * rows * d;
        const uint16_t* U = su + (size_t)l * rows * a.mlp;
        // MLP branch: dM = dOut W2, dU = dM gelu'(U), dH2 = dU W1, ln_2 backward (+ residual)
        if ((rc = gemm(wt[3], d, a.mlp, G16, d, (int)rows, d, dM, a.mlp, TVC_EPI_BF16))) return rc;
        HIP_TRY(launch_gelu_bwd(dM, U, rows * a.mlp, st));
        if ((rc = gemm(wt[2], a.mlp, d, dM, a.mlp, (int)rows, a.mlp, D2, d, TVC_EPI_BF16))) return rc;
        HIP_TRY(launch_layernorm_bwd(X, d, D1, D2, 0, w.ln2_g, dX, dX, G16, (int)rows, d, d, st));
        // attention branch: dAO = dMid Wo, attention backward, dH1 = dQKV Wqkv, ln_1 backward (+ residual)
        if ((rc = gemm(wt[1], d, d, G16, d, (int)rows, d, H, d, TVC_EPI_BF16))) return rc;
        HIP_TRY(launch_attention_bwd(QKV, H, dQKV, (float*)h->ws[WS_GSTATS].p, B, T, a.heads, st));
        if ((rc = gemm(wt[0], 3 * d, d, dQKV, 3 * d, (int)rows, 3 * d, D2, d, TVC_EPI_BF16))) return rc;
        HIP_TRY(launch_layernorm_bwd(X, d, nullptr, D2, 0, w.ln1_g, dX, dX, G16, (int)rows, d, d, st));
    }
    // ---- stem: ln_pre, patch embedding, col2im
    uint16_t* Pm = (uint16_t*)h->ws[WS_PATCH].p;
    float* patch_out = (float*)h->ws[WS_GPATCH].p;                  // fp32 [B*P, d], then reused as dcols [B*P, Kp]
    HIP_TRY(launch_im2col(h->grad_pix, Pm, B, m.image_size, m.patch, Kp, st));
    if ((rc = gemm(h->vision.w.patch_w, Kp, d, Pm, Kp, B * P, Kp, patch_out, d, TVC_EPI_F32))) return rc;
    uint16_t* dpatch = (uint16_t*)h->ws[WS_GDQKV].p;               // bf16 [B*P, d]
    HIP_TRY(launch_lnpre_bwd(patch_out, h->vision.w.pos, h->vision.w.ln_pre_g, dX, dpatch, B, T, d, st));
    if ((rc = gemm(h->wT[(size_t)a.layers * 4 + 1], d, Kp, dpatch, d, B * P, d, patch_out, Kp, TVC_EPI_F32))) return rc;
    HIP_TRY(launch_col2im(patch_out, grad_pix_dev, B, m.image_size, m.patch, Kp, st));
    return TVC_OK;
}

int tvc_pgd_step(tvc_handle* h, float* adv_dev, const float* clean_dev, const float* grad_dev, float* momentum_dev, int32_t B,
                 int64_t n, float eps, float alpha, float mu, float clip_min, float clip_max, int32_t targeted, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (B < 0 || n < 0 || (B > 0 && n > 0 && (!adv_dev || !clean_dev || !grad_dev)))
        return fail(h, TVC_E_INVALID, "tvc_pgd_step: bad arguments");
    HIP_TRY(launch_pgd_step(adv_dev, clean_dev, grad_dev, momentum_dev, B, n, eps, alpha, mu, clip_min, clip_max, targeted,
                            (hipStream_t)stream));
    return TVC_OK;
}

int tvc_l2_step(tvc_handle* h, float* adv_dev, const float* clean_dev, const float* grad_dev, int32_t B, int64_t n, float eps,
                float step, float clip_min, float clip_max, int32_t descent, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (B < 0 || n < 0 || (B > 0 && n > 0 && (!adv_dev || !clean_dev || !grad_dev)))
        return fail(h, TVC_E_INVALID, "tvc_l2_step: bad arguments");
    HIP_TRY(launch_l2_step(adv_dev, clean_dev, grad_dev, B, n, eps, step, clip_min, clip_max, descent, (hipStream_t)stream));
    return TVC_OK;
}

int tvc_attention_backward(tvc_handle* h, const uint16_t* qkv_dev, const uint16_t* dout_dev, uint16_t* dqkv_dev, int32_t n_seq,
                           int32_t seq_len, int32_t heads, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!qkv_dev || !dout_dev || !dqkv_dev) return fail(h, TVC_E_INVALID, "tvc_attention_backward: NULL buffer");
    // a negative count would reach ensure() as a size near 2^64, which frees the workspace before the allocation fails
    if (n_seq < 0 || seq_len < 0 || heads < 0)
        return fail(h, TVC_E_INVALID, "tvc_attention_backward: n_seq, seq_len and heads must not be negative");
    int rc;
    if ((rc = ensure(h, WS_GSTATS, (size_t)n_seq * seq_len * heads * 16))) return rc;
    HIP_TRY(launch_attention_bwd(qkv_dev, dout_dev, dqkv_dev, (float*)h->ws[WS_GSTATS].p, n_seq, seq_len, heads, (hipStream_t)stream));
    return TVC_OK;
}

int tvc_layernorm_backward(tvc_handle* h, const float* x_dev, const uint16_t* dy_dev, const float* g_dev, const float* dres_dev,
                           float* dx_dev, int32_t rows, int32_t d, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!x_dev || !dy_dev || !g_dev || !dx_dev) return fail(h, TVC_E_INVALID, "tvc_layernorm_backward: NULL buffer");
    HIP_TRY(launch_layernorm_bwd(x_dev, d, nullptr, dy_dev, 0, g_dev, dres_dev, dx_dev, nullptr, rows, d, d, (hipStream_t)stream));
    return TVC_OK;
}

int tvc_set_option(tvc_handle* h, int32_t option, int64_t value) {
    if (!h) return TVC_E_INVALID;
    switch (option) {
        case TVC_OPT_TEXT_PACKING: h->pack_text = value != 0; return TVC_OK;
        case TVC_OPT_BANK_FILTER: h->bank_filter = value != 0; return TVC_OK;
        case TVC_OPT_POOLED_LAST_LAYER: h->pooled_last = value != 0; return TVC_OK;
        case TVC_OPT_TOWER_PRECISION: {
            if (value < 0 || value > 3)
                return fail(h, TVC_E_INVALID, "tvc_set_option: TVC_OPT_TOWER_PRECISION must be 0 (bf16), 1 (fp32), 2 (split-bf16) or 3 (fp16)");
            if (value == 3) {
                // (TVC_E_INVALID, not TVC_E_STATE: before fp16 weights exist the value is outside what the handle offers,
                // as it was before the mode existed)
                if (!h->vision16.set && !h->text16.set)
                    return fail(h, TVC_E_INVALID, "tvc_set_option: TVC_OPT_TOWER_PRECISION = 3 needs tvc_set_weights_f16 first");
                h->tower_precision = 3; return TVC_OK;
            }
            if (value != 0 && !h->vision32.set && !h->text32.set)
                return fail(h, TVC_E_STATE, "tvc_set_option: TVC_OPT_TOWER_PRECISION = 1 / 2 needs tvc_set_weights_f32 first");
            if (value == 2) {
                const int rc = tvc_split_prepare(h);        // builds the weight planes once (synchronises the device)
                if (rc) return rc;
            }
            h->tower_precision = (int)value; return TVC_OK;
        }
        case TVC_OPT_GRAD_PRECISION:
            if (value != 0 && value != 2)
                return fail(h, TVC_E_INVALID, "tvc_set_option: TVC_OPT_GRAD_PRECISION must be 0 (bf16) or 2 (split-bf16)");
            // the weight planes are the tower mode's: built here once when the fp32 weights are there (synchronises the device);
            // without them the option is recorded and tvc_encode_image_grad reports what is missing
            if (value == 2 && h->vision32.set) {
                const int rc = tvc_split_prepare(h);
                if (rc) return rc;
            }
            h->grad_precision = (int)value; return TVC_OK;
        case TVC_OPT_TEXT_GROUP:
            if (value < 0 || value > 4096) return fail(h, TVC_E_INVALID, "tvc_set_option: TVC_OPT_TEXT_GROUP out of range");
            h->text_group = (int)value; return TVC_OK;
        case TVC_OPT_MAX_CHUNK_IMAGES:
            if (value < 1) return fail(h, TVC_E_INVALID, "tvc_set_option: chunk must be >= 1");
            h->max_chunk_images = (int)value; return TVC_OK;
        case TVC_OPT_MAX_CHUNK_TEXTS:
            if (value < 1) return fail(h, TVC_E_INVALID, "tvc_set_option: chunk must be >= 1");
            h->max_chunk_texts = (int)value; return TVC_OK;
        case TVC_OPT_SD_ARENA_BYTES:
            if (value < ((int64_t)1 << 28)) return fail(h, TVC_E_INVALID, "tvc_set_option: TVC_OPT_SD_ARENA_BYTES must be >= 256 MiB");
            h->sd_arena_bytes = (size_t)value; return TVC_OK;
        case TVC_OPT_SD_STREAMS:
            if (value < 1 || value > 2) return fail(h, TVC_E_INVALID, "tvc_set_option: TVC_OPT_SD_STREAMS must be 1 or 2");
            h->sd_streams = (int)value; return TVC_OK;
        case TVC_OPT_SD_PRECISION:
            if (value < 0 || value > 1) return fail(h, TVC_E_INVALID, "tvc_set_option: TVC_OPT_SD_PRECISION must be 0 (bf16) or 1 (fp16)");
            // the tensors registered by tvc_sd_load are one format: the option moves only while no model is loaded
            if (h->sd && (int)value != h->sd_precision)
                return fail(h, TVC_E_STATE, "tvc_set_option: TVC_OPT_SD_PRECISION cannot change while a latent-diffusion model is loaded");
            h->sd_precision = (int)value; return TVC_OK;
        default: return fail(h, TVC_E_INVALID, "tvc_set_option: unknown option");
    }
}

int tvc_profile_begin(tvc_handle* h) {
    if (!h) return TVC_E_INVALID;
    for (auto& r : h->prof_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    h->prof_recs.clear();
    h->prof = true;
    return TVC_OK;
}

int tvc_profile_end(tvc_handle* h, double* ms, double* work, int64_t* launches, double* big_gemm) {
    if (!h) return TVC_E_INVALID;
    if (!ms || !work || !launches) return fail(h, TVC_E_INVALID, "tvc_profile_end: NULL output");
    h->prof = false;
    HIP_TRY(hipDeviceSynchronize());
    for (int c = 0; c < TVC_PROF_NCAT; ++c) { ms[c] = 0; work[c] = 0; launches[c] = 0; }
    if (big_gemm) big_gemm[0] = big_gemm[1] = big_gemm[2] = 0;
    // diagnostics (scripts/gemm_shape_table.py): TVC_PROF_DUMP=<file> appends one line per GEMM launch -- I J K planes split ms
    FILE* dump = nullptr;
    if (const char* path = getenv("TVC_PROF_DUMP")) dump = fopen(path, "a");
    for (auto& r : h->prof_recs) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess && r.cat >= 0 && r.cat < TVC_PROF_NCAT) {
            ms[r.cat] += t; work[r.cat] += r.work; launches[r.cat] += 1;
            if (big_gemm && r.big_bytes > 0) { big_gemm[0] += r.big_bytes; big_gemm[1] += 1; big_gemm[2] += t; }
            if (dump && r.cat == TVC_PROF_GEMM) fprintf(dump, "%d %d %d %d %d %.6f\n", r.gI, r.gJ, r.gK, r.gP, r.gS, t);
        }
        (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
    }
    h->prof_recs.clear();
    if (dump) fclose(dump);
    return TVC_OK;
}

}  // extern "C"

namespace {
int gemm16(tvc_handle* h, const char* name, bool f16, const uint16_t* a_dev, const uint16_t* b_dev, const float* bias_dev,
           void* out_dev, int32_t I, int32_t J, int32_t K, int64_t lda, int64_t ldb, int32_t ld_out, int32_t epilogue,
           void* stream) {
    if (!h) return TVC_E_INVALID;
    if (lda == 0) lda = K;
    if (ldb == 0) ldb = K;
    if (I <= 0 || J <= 0 || K <= 0 || K % 64 != 0 || !a_dev || !b_dev || !out_dev || ld_out < I ||
        epilogue < 0 || epilogue > 3 || lda < K || ldb < K || lda % 8 != 0 || ldb % 8 != 0)
        return fail(h, TVC_E_INVALID, std::string(name) + ": need K % 64 == 0, ld_out >= I, lda / ldb >= K and multiples of 8");
    // the kernels load and store 16 bytes per lane from the buffers' bases, and the ring forms compute a lane's row offset
    // (row * pitch, in elements) in 32 bits
    auto misaligned = [](const void* p) { return ((uintptr_t)p & 15) != 0; };
    if (misaligned(a_dev) || misaligned(b_dev) || misaligned(out_dev) || (bias_dev && misaligned(bias_dev)))
        return fail(h, TVC_E_INVALID, std::string(name) + ": a, b, out and bias must be 16-byte aligned");
    if (lda >= ((int64_t)1 << 23) || ldb >= ((int64_t)1 << 23))
        return fail(h, TVC_E_INVALID, std::string(name) + ": lda / ldb must be below 2^23");
    GemmLaunch g = gemm_launch(a_dev, lda, I, b_dev, ldb, J, K, bias_dev, out_dev, ld_out, epilogue);
    g.f16 = f16;
    {
        int rc = ensure(h, WS_SPLITK, (size_t)256 * 256 * 256 * 4);       // split-K scratch (small or tail tiles)
        if (rc) return rc;
        g.splitk_ws = (float*)h->ws[WS_SPLITK].p; g.splitk_ws_bytes = h->ws[WS_SPLITK].n;
    }
    HIP_TRY(launch_gemm_bf16(g, (hipStream_t)stream));
    return TVC_OK;
}
}  // namespace

extern "C" {

int tvc_gemm_bf16(tvc_handle* h, const uint16_t* a_dev, const uint16_t* b_dev, const float* bias_dev, void* out_dev,
                  int32_t I, int32_t J, int32_t K, int64_t lda, int64_t ldb, int32_t ld_out, int32_t epilogue,
                  void* stream) {
    return gemm16(h, "tvc_gemm_bf16", false, a_dev, b_dev, bias_dev, out_dev, I, J, K, lda, ldb, ld_out, epilogue, stream);
}

int tvc_gemm_f16(tvc_handle* h, const uint16_t* a_dev, const uint16_t* b_dev, const float* bias_dev, void* out_dev,
                 int32_t I, int32_t J, int32_t K, int64_t lda, int64_t ldb, int32_t ld_out, int32_t epilogue,
                 void* stream) {
    return gemm16(h, "tvc_gemm_f16", true, a_dev, b_dev, bias_dev, out_dev, I, J, K, lda, ldb, ld_out, epilogue, stream);
}

int tvc_attention(tvc_handle* h, const uint16_t* qkv_dev, uint16_t* out_dev, int32_t n_seq, int32_t seq_len,
                  int32_t heads, int32_t causal, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!qkv_dev || !out_dev) return fail(h, TVC_E_INVALID, "tvc_attention: NULL buffer");
    HIP_TRY(launch_attention(qkv_dev, out_dev, nullptr, n_seq, seq_len, heads, causal, (hipStream_t)stream));
    return TVC_OK;
}

int tvc_attention_f16(tvc_handle* h, const uint16_t* qkv_dev, uint16_t* out_dev, const int32_t* starts_dev, int32_t n_seq,
                      int32_t seq_len, int32_t heads, int32_t causal, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!qkv_dev || !out_dev) return fail(h, TVC_E_INVALID, "tvc_attention_f16: NULL buffer");
    HIP_TRY(launch_attention(qkv_dev, out_dev, starts_dev, n_seq, seq_len, heads, causal, (hipStream_t)stream, nullptr, 0,
                             nullptr, 1));
    return TVC_OK;
}

int tvc_attention_ex(tvc_handle* h, const uint16_t* qkv_dev, uint16_t* out_dev, const int32_t* starts_dev, const int32_t* pfx_dev,
                     int32_t n_seq, int32_t seq_len, int32_t heads, int32_t causal, int32_t pool_mode, const int32_t* pool_row_dev,
                     int32_t f16, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!qkv_dev || !out_dev) return fail(h, TVC_E_INVALID, "tvc_attention_ex: NULL buffer");
    // what launch_attention refuses (or, for a prefix on a non-causal launch, would silently drop), checked here so that a
    // refused call launches nothing whatever the launcher does
    if (n_seq < 0 || seq_len < 1 || seq_len > 288 || heads < 1 || pool_mode < 0 || pool_mode > 2)
        return fail(h, TVC_E_INVALID, "tvc_attention_ex: need n_seq >= 0, 1 <= seq_len <= 288, heads >= 1 and pool_mode 0 / 1 / 2");
    if (pfx_dev && (!starts_dev || !causal))
        return fail(h, TVC_E_INVALID, "tvc_attention_ex: pfx needs packed rows (starts) and the causal mask");
    if (pool_mode == 2 && !starts_dev && !pool_row_dev)
        return fail(h, TVC_E_INVALID, "tvc_attention_ex: pool_mode 2 on dense rows needs pool_row");
    HIP_TRY(launch_attention(qkv_dev, out_dev, starts_dev, n_seq, seq_len, heads, causal, (hipStream_t)stream, pfx_dev, pool_mode,
                             pool_row_dev, f16 != 0));
    return TVC_OK;
}

int tvc_layernorm(tvc_handle* h, const float* x_dev, const float* g_dev, const float* b_dev, uint16_t* y_dev,
                  int32_t rows, int32_t d, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!x_dev || !g_dev || !b_dev || !y_dev) return fail(h, TVC_E_INVALID, "tvc_layernorm: NULL buffer");
    HIP_TRY(launch_layernorm(const_cast<float*>(x_dev), d, nullptr, nullptr, 0, g_dev, b_dev, y_dev, rows, d,
                             (hipStream_t)stream));
    return TVC_OK;
}

int tvc_layernorm_f16(tvc_handle* h, const float* x_dev, const float* g_dev, const float* b_dev, uint16_t* y_dev,
                      int32_t rows, int32_t d, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!x_dev || !g_dev || !b_dev || !y_dev) return fail(h, TVC_E_INVALID, "tvc_layernorm_f16: NULL buffer");
    HIP_TRY(launch_layernorm(const_cast<float*>(x_dev), d, nullptr, nullptr, 0, g_dev, b_dev, y_dev, rows, d,
                             (hipStream_t)stream, nullptr, 0, nullptr, nullptr, 1));
    return TVC_OK;
}

int tvc_set_weights_f16(tvc_handle* h, const tvc_vision_weights* vision, const tvc_text_weights* text) {
    if (!h) return TVC_E_INVALID;
    if (vision) {
        if (!h->vision.set) return fail(h, TVC_E_STATE, "tvc_set_weights_f16: handle was created without a vision tower");
        if (!vision->layers || !vision->patch_w || !vision->proj) return fail(h, TVC_E_INVALID, "tvc_set_weights_f16: NULL vision weights");
        h->vision16.assign(*vision, h->desc.vision.layers);
    }
    if (text) {
        if (!h->text.set) return fail(h, TVC_E_STATE, "tvc_set_weights_f16: handle was created without a text tower");
        if (!text->layers || !text->tok_emb || !text->proj) return fail(h, TVC_E_INVALID, "tvc_set_weights_f16: NULL text weights");
        h->text16.assign(*text, h->desc.text.layers);
    }
    return TVC_OK;
}

}  // extern "C"
