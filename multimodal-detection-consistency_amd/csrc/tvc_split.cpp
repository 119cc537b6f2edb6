// Split-bf16 CLIP towers (TVC_OPT_TOWER_PRECISION = 2, include/tvc.h), the fast <= 1e-4 mode: the mode's workspace,
// stem, layer loop and head, driven by the tower encode drivers of tvc_abi.cpp, the weight planes and the parity entry
// points.  Same arithmetic as the reference's fp32 towers (src/detector.py:461-485 via CLIPModel.encode_*) with every
// activation and weight carried to the matrix cores as hi | lo bf16 planes and every product formed from three bf16
// MFMAs (split.hip): embeddings within ~1e-5 of the fp32 CPU path at about a third of the bf16 mode's matrix rate --
// against the 1/16 of the exact-f32 mode (tvc_precise.cpp, TVC_OPT_TOWER_PRECISION = 1), which stays the exact reference.
//
// Per layer:   Hs = split(LN1(X [+ D1 + D2 of the previous layer, written back]))       ln_split
//              QKV = Wqkv_s x Hs + b            (3 planes, fp32 out)                      gemm_ring4_kernel<F32>
//              Hs = split(attention(QKV))                                                 attention_split
//              D1 = Wo_s x Hs + b               (fp32)
//              Hs = split(LN2(X + D1))
//              U = W1_s x Hs + b                (fp32);  Ms = split(QuickGELU(U))         rows_split(gelu)
//              D2 = W2_s x Ms + b               (fp32)
// The residual projections are store-only GEMMs (as in the bf16 tower): the LayerNorm passes fold the fp32 deltas into X.
// The drivers EOT-pack text rows with variant prefix sharing exactly as in the bf16 mode (TVC_OPT_TEXT_PACKING / _GROUP):
// the work skipped is work whose results the causal tower never reads.  No pooled last layer (the mode is for parity).
#include "handle.hpp"

// out fp32 [J, ldo] = (W_hi + W_lo)[I, K] x (B_hi + B_lo)[J, K]^T + bias, without the lo x lo term
int split_gemm3(tvc_handle* h, const uint16_t* Ws, int I, int K, const uint16_t* Bs, int64_t J, const float* bias, float* out, int64_t ldo,
          hipStream_t st) {
    GemmLaunch g = gemm_launch(Ws, 2 * (int64_t)K, I, Bs, 2 * (int64_t)K, (int)J, K, bias, out, ldo, TVC_EPI_F32);
    g.planes = 3;                                       // small terms first, the hi x hi products last
    g.a_plane_off[0] = 0; g.b_plane_off[0] = K;         // A_hi x B_lo
    g.a_plane_off[1] = K; g.b_plane_off[1] = 0;         // A_lo x B_hi
    g.a_plane_off[2] = 0; g.b_plane_off[2] = 0;         // A_hi x B_hi
    g.a_rows_padded = true; g.b_rows_padded = true;     // split weights / workspaces are allocated to whole tiles
    HIP_TRY(timed_gemm(h, g, st));
    return TVC_OK;
}

namespace {

struct SBufs { float *X, *QKV, *U, *D1, *D2, *CLS; uint16_t *Hs, *Ms; };

SBufs split_bufs(tvc_handle* h, bool text) {
    const int wso = text ? WS_S_N : 0;
    SBufs b;
    b.X = (float*)h->ws[WS_SX + wso].p; b.Hs = (uint16_t*)h->ws[WS_SH + wso].p;
    b.QKV = (float*)h->ws[WS_SQKV + wso].p; b.U = (float*)h->ws[WS_SU + wso].p;
    b.Ms = (uint16_t*)h->ws[WS_SM + wso].p; b.D1 = (float*)h->ws[WS_SDELTA1 + wso].p;
    b.D2 = (float*)h->ws[WS_SDELTA2 + wso].p; b.CLS = (float*)h->ws[WS_SCLS + wso].p;
    return b;
}

// fp32 [I, K] -> handle-owned hi | lo planes [round_up(I, 256), 2 * Kp] (zero rows / columns beyond I / K)
int split_weight(tvc_handle* h, const float* w, int I, int K, int Kp, uint16_t** out, hipStream_t st) {
    const size_t rows = ((size_t)I + 255) / 256 * 256;
    void* p = nullptr;
    if (hipMalloc(&p, rows * 2 * Kp * 2) != hipSuccess) return fail(h, TVC_E_NOMEM, "split weights: allocation failed");
    h->split_owned.push_back(p);
    HIP_TRY(hipMemsetAsync(p, 0, rows * 2 * Kp * 2, st));
    HIP_TRY(launch_rows_split(w, K, (uint16_t*)p, I, K, Kp, 0, st));
    *out = (uint16_t*)p;
    return TVC_OK;
}

int split_tower(tvc_handle* h, const tvc_tower_arch& a, const tvc_layer_weights_f32* lw, std::vector<SplitLayer>& out, hipStream_t st) {
    out.resize(a.layers);
    int rc;
    for (int l = 0; l < a.layers; ++l) {
        if ((rc = split_weight(h, lw[l].wqkv, 3 * a.width, a.width, a.width, &out[l].wqkv, st))) return rc;
        if ((rc = split_weight(h, lw[l].wo, a.width, a.width, a.width, &out[l].wo, st))) return rc;
        if ((rc = split_weight(h, lw[l].w1, a.mlp, a.width, a.width, &out[l].w1, st))) return rc;
        if ((rc = split_weight(h, lw[l].w2, a.width, a.mlp, a.mlp, &out[l].w2, st))) return rc;
    }
    return TVC_OK;
}

}  // namespace

void tvc_split_free(tvc_handle* h) {
    for (void* p : h->split_owned) if (p) (void)hipFree(p);
    h->split_owned.clear();
    h->vsplit.clear(); h->tsplit.clear();
    h->vsplit_patch = nullptr;
    h->vsplit_t.clear();
    h->vsplit_proj_t = h->vsplit_patch_t = nullptr;
    h->split_ready = false;
}

// Build the hi | lo planes of every GEMM weight from the fp32 copies registered by tvc_set_weights_f32 (1.7 GB at
// ViT-L/14); synchronises the device once.  Called by tvc_set_option(TVC_OPT_TOWER_PRECISION, 2).
int tvc_split_prepare(tvc_handle* h) {
    if (h->split_ready) return TVC_OK;
    {
        // the split attention keeps K and V of a head as hi | lo images in LDS: at most 272 tokens per sequence (the bf16
        // and fp32 modes take 288, which tvc_create already enforces together with head_dim 64)
        const tvc_model_desc& md = h->desc;
        const int Tv = h->vision.set ? (md.image_size / md.patch) * (md.image_size / md.patch) + 1 : 0;
        if (Tv > 272 || (h->text.set && md.ctx > 272))
            return fail(h, TVC_E_INVALID, "TVC_OPT_TOWER_PRECISION = 2: sequences longer than 272 tokens are not supported by the split attention");
    }
    tvc_split_free(h);
    hipStream_t st = nullptr;
    int rc;
    const tvc_model_desc& m = h->desc;
    if (h->vision32.set) {
        if ((rc = split_tower(h, m.vision, h->vision32.w.layers, h->vsplit, st))) { tvc_split_free(h); return rc; }
        const int K = 3 * m.patch * m.patch, Kp = (K + 63) / 64 * 64;
        if ((rc = split_weight(h, h->vision32.w.patch_w, m.vision.width, K, Kp, &h->vsplit_patch, st))) { tvc_split_free(h); return rc; }
    }
    if (h->text32.set && (rc = split_tower(h, m.text, h->text32.w.layers, h->tsplit, st))) { tvc_split_free(h); return rc; }
    HIP_TRY(hipStreamSynchronize(st));
    h->split_ready = true;
    return TVC_OK;
}

int split_ensure(tvc_handle* h, bool text, int n_seq, float** X) {
    const tvc_model_desc& m = h->desc;
    const tvc_tower_arch& a = text ? m.text : m.vision;
    const int P = (m.image_size / m.patch) * (m.image_size / m.patch), K = 3 * m.patch * m.patch, Kp = (K + 63) / 64 * 64;
    const int64_t rp = tile_rows((int64_t)n_seq * (text ? m.ctx : P + 1));     // GEMM operands: readable rows to the next tile (+ one)
    const int wso = text ? WS_S_N : 0;
    size_t u_bytes = (size_t)rp * a.mlp * 4, m_bytes = (size_t)rp * a.mlp * 2 * 2;
    if (!text) {
        // the stem parks its fp32 im2col rows in U, their planes in Ms and the patch embeddings in QKV ([n * P, d] fits [rows, 3d])
        const size_t u_min = (size_t)tile_rows((int64_t)n_seq * P) * K * 4, m_min = (size_t)tile_rows((int64_t)n_seq * P) * 2 * Kp * 2;
        if (u_bytes < u_min) u_bytes = u_min;
        if (m_bytes < m_min) m_bytes = m_min;
    }
    int rc;
    if ((rc = ensure(h, (Slot)(WS_SX + wso), (size_t)rp * a.width * 4))) return rc;
    if ((rc = ensure(h, (Slot)(WS_SH + wso), (size_t)rp * a.width * 2 * 2))) return rc;
    if ((rc = ensure(h, (Slot)(WS_SQKV + wso), (size_t)rp * a.width * 3 * 4))) return rc;
    if ((rc = ensure(h, (Slot)(WS_SU + wso), u_bytes))) return rc;
    if ((rc = ensure(h, (Slot)(WS_SM + wso), m_bytes))) return rc;
    if ((rc = ensure(h, (Slot)(WS_SDELTA1 + wso), (size_t)rp * a.width * 4))) return rc;
    if ((rc = ensure(h, (Slot)(WS_SDELTA2 + wso), (size_t)rp * a.width * 4))) return rc;
    if ((rc = ensure(h, (Slot)(WS_SCLS + wso), (size_t)(n_seq + 8) * a.width * 4))) return rc;
    *X = split_bufs(h, text).X;
    return TVC_OK;
}

int split_stem(tvc_handle* h, const float* pix, int n, const float** patch_out, hipStream_t st) {
    const tvc_model_desc& m = h->desc;
    const int P = (m.image_size / m.patch) * (m.image_size / m.patch), d = m.vision.width, K = 3 * m.patch * m.patch;
    const int Kp = (K + 63) / 64 * 64;
    const SBufs b = split_bufs(h, false);
    float* cols = b.U;                   // [n * P, K] fp32
    HIP_TRY(launch_im2col_f32(pix, cols, n, m.image_size, m.patch, st));
    HIP_TRY(launch_rows_split(cols, K, b.Ms, (int64_t)n * P, K, Kp, 0, st));
    *patch_out = b.QKV;                  // [n * P, d] fp32
    return split_gemm3(h, h->vsplit_patch, d, Kp, b.Ms, (int64_t)n * P, nullptr, b.QKV, d, st);
}

namespace {
// keep (the split-bf16 input gradient's forward; dense vision rows): layer l's QKV, out-projection output and FC1 pre-activation go
// to its slices of *keep instead of the workspace, and the layer's input rows are copied there once ln_1 has folded the pending
// deltas into X.  d1_last / d2_last: where the last layer's deltas are.
int layers_impl(tvc_handle* h, bool text, int n_seq, int seq_len, const int32_t* starts, int total_rows, const int32_t* pfx,
                const SplitKeep* keep, const float** d1_last, const float** d2_last, hipStream_t st) {
    const tvc_tower_arch& a = text ? h->desc.text : h->desc.vision;
    const SplitLayer* sw = (text ? h->tsplit : h->vsplit).data();
    const tvc_layer_weights_f32* lw = text ? h->text32.w.layers : h->vision32.w.layers;
    SBufs b = split_bufs(h, text);
    const int causal = text ? 1 : 0;
    const int d = a.width;
    const int rows = starts ? total_rows : n_seq * seq_len;
    int rc;
    bool pending = false;
    for (int l = 0; l < a.layers; ++l) {
        const tvc_layer_weights_f32& w = lw[l];
        {
            ProfScope ps(h, st, TVC_PROF_ROWOPS, (double)rows * d * (pending ? 24.0 : 8.0));
            HIP_TRY(launch_ln_split(b.X, d, nullptr, pending ? b.D1 : nullptr, pending ? b.D2 : nullptr, 1, w.ln1_g, w.ln1_b, b.Hs,
                                    nullptr, rows, d, st));
        }
        if (keep) {
            HIP_TRY(hipMemcpyAsync(keep->x + (size_t)l * rows * d, b.X, (size_t)rows * d * 4, hipMemcpyDeviceToDevice, st));
            b.QKV = keep->qkv + (size_t)l * rows * 3 * d;
            b.D1 = keep->d1 + (size_t)l * rows * d;        // read again by the next layer's ln_1 (or the caller's final LayerNorm)
            b.U = keep->u + (size_t)l * rows * a.mlp;
        }
        if ((rc = split_gemm3(h, sw[l].wqkv, 3 * d, d, b.Hs, rows, w.bqkv, b.QKV, 3 * d, st))) return rc;
        {
            const double avg_len = starts ? (double)rows / n_seq : (double)seq_len;
            ProfScope ps(h, st, TVC_PROF_ATTENTION, 3.0 * 4.0 * n_seq * a.heads * avg_len * avg_len * 64 * (causal ? 0.5 : 1.0));
            HIP_TRY(launch_attention_split(b.QKV, b.Hs, starts, n_seq, seq_len, a.heads, causal, st, pfx));
        }
        if ((rc = split_gemm3(h, sw[l].wo, d, d, b.Hs, rows, w.bo, b.D1, d, st))) return rc;
        {
            ProfScope ps(h, st, TVC_PROF_ROWOPS, (double)rows * d * 12.0);
            HIP_TRY(launch_ln_split(b.X, d, nullptr, b.D1, nullptr, 0, w.ln2_g, w.ln2_b, b.Hs, nullptr, rows, d, st));
        }
        if ((rc = split_gemm3(h, sw[l].w1, a.mlp, d, b.Hs, rows, w.b1, b.U, a.mlp, st))) return rc;
        {
            ProfScope ps(h, st, TVC_PROF_ROWOPS, (double)rows * a.mlp * 8.0);
            HIP_TRY(launch_rows_split(b.U, a.mlp, b.Ms, rows, a.mlp, a.mlp, a.act == TVC_ACT_GELU ? 2 : 1, st));
        }
        if ((rc = split_gemm3(h, sw[l].w2, d, a.mlp, b.Ms, rows, w.b2, b.D2, d, st))) return rc;
        pending = true;
    }
    if (d1_last) *d1_last = b.D1;
    if (d2_last) *d2_last = b.D2;
    return TVC_OK;
}
}  // namespace

int split_layers(tvc_handle* h, bool text, int n_seq, int seq_len, const int32_t* starts, int total_rows,
                 const int32_t* pfx, hipStream_t st) {
    return layers_impl(h, text, n_seq, seq_len, starts, total_rows, pfx, nullptr, nullptr, nullptr, st);
}

int split_layers_keep(tvc_handle* h, int n_seq, int seq_len, const SplitKeep& keep, const float** d1_last, const float** d2_last,
                      hipStream_t st) {
    return layers_impl(h, false, n_seq, seq_len, nullptr, 0, nullptr, &keep, d1_last, d2_last, st);
}

// the LayerNorm folds in the last layer's two pending deltas; the projection runs exact f32 (rows is small)
int split_head(tvc_handle* h, bool text, int64_t x_stride, const int32_t* row_idx, int rows, float* out, bool hidden,
               hipStream_t st) {
    const tvc_model_desc& m = h->desc;
    const int d = text ? m.text.width : m.vision.width;
    const SBufs b = split_bufs(h, text);
    const float* g = text ? h->text32.w.ln_final_g : h->vision32.w.ln_post_g;
    const float* beta = text ? h->text32.w.ln_final_b : h->vision32.w.ln_post_b;
    HIP_TRY(launch_ln_split(b.X, x_stride, row_idx, b.D1, b.D2, 0, g, beta, nullptr, hidden ? out : b.CLS, rows, d, st));
    if (hidden) return TVC_OK;
    return timed_gemm_f32(h, text ? h->text32.w.proj : h->vision32.w.proj, m.embed_dim, d, b.CLS, rows, nullptr, out, m.embed_dim, 0, st);
}

// ---- building blocks exported for parity tests (include/tvc.h)
extern "C" int tvc_gemm_split(tvc_handle* h, const float* w_dev, const float* x_dev, const float* bias_dev, float* out_dev, int32_t I,
                              int32_t J, int32_t K, int32_t ld_out, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (I <= 0 || J <= 0 || K <= 0 || K % 4 != 0 || !w_dev || !x_dev || !out_dev || ld_out < I || ld_out % 4 != 0)
        return fail(h, TVC_E_INVALID, "tvc_gemm_split: need K % 4 == 0, ld_out >= I and a multiple of 4");
    hipStream_t st = (hipStream_t)stream;
    const int Kp = (K + 63) / 64 * 64;
    const int64_t Ip = ((int64_t)I + 255) / 256 * 256, Jp = tile_rows(J);
    int rc;
    if ((rc = ensure(h, WS_SH, (size_t)Ip * 2 * Kp * 2))) return rc;
    if ((rc = ensure(h, WS_SM, (size_t)Jp * 2 * Kp * 2))) return rc;
    uint16_t* ws = (uint16_t*)h->ws[WS_SH].p;
    uint16_t* xs = (uint16_t*)h->ws[WS_SM].p;
    HIP_TRY(hipMemsetAsync(ws, 0, (size_t)Ip * 2 * Kp * 2, st));
    HIP_TRY(launch_rows_split(w_dev, K, ws, I, K, Kp, 0, st));
    HIP_TRY(launch_rows_split(x_dev, K, xs, J, K, Kp, 0, st));
    return split_gemm3(h, ws, I, Kp, xs, J, bias_dev, out_dev, ld_out, st);
}

extern "C" int tvc_attention_split(tvc_handle* h, const float* qkv_dev, uint16_t* out_planes_dev, const int32_t* starts_dev,
                                   int32_t n_seq, int32_t seq_len, int32_t heads, int32_t causal, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!qkv_dev || !out_planes_dev || seq_len < 1 || seq_len > 272 || heads < 1 || n_seq < 0)
        return fail(h, TVC_E_INVALID, "tvc_attention_split: need 1 <= seq_len <= 272 and non-NULL buffers");
    HIP_TRY(launch_attention_split(qkv_dev, out_planes_dev, starts_dev, n_seq, seq_len, heads, causal, (hipStream_t)stream, nullptr));
    return TVC_OK;
}

extern "C" int tvc_attention_split_ex(tvc_handle* h, const float* qkv_dev, uint16_t* out_planes_dev, const int32_t* starts_dev,
                                      const int32_t* pfx_dev, int32_t n_seq, int32_t seq_len, int32_t heads, int32_t causal,
                                      void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!qkv_dev || !out_planes_dev || seq_len < 1 || seq_len > 272 || heads < 1 || n_seq < 0)
        return fail(h, TVC_E_INVALID, "tvc_attention_split_ex: need 1 <= seq_len <= 272 and non-NULL buffers");
    if (pfx_dev && (!starts_dev || !causal))
        return fail(h, TVC_E_INVALID, "tvc_attention_split_ex: pfx needs packed rows (starts) and the causal mask");
    HIP_TRY(launch_attention_split(qkv_dev, out_planes_dev, starts_dev, n_seq, seq_len, heads, causal, (hipStream_t)stream, pfx_dev));
    return TVC_OK;
}
