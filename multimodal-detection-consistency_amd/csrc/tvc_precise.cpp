// fp32-grade CLIP towers (TVC_OPT_TOWER_PRECISION = 1, include/tvc.h): the mode's workspace, stem, layer loop and head,
// driven by the tower encode drivers of tvc_abi.cpp, and its parity entry points.  Same arithmetic as the bf16 towers --
// pre-LN blocks, QuickGELU, class / EOT pooling, projection -- but every tensor stays fp32 and every GEMM runs on the
// exact-f32 matrix instruction (precise.hip), so the result equals the reference's fp32 CPU towers up to the order of
// fp32 additions.  The drivers run this mode dense: no EOT packing, prefix sharing or pooled last layer (the mode exists
// for parity -- validation, attack generation -- not for speed).
#include "handle.hpp"

namespace {

struct P32Bufs { float *X, *H, *QKV, *MLP, *CLS; };

P32Bufs p32_bufs(tvc_handle* h, bool text) {
    const int wso = text ? WS_P_N : 0;
    return {(float*)h->ws[WS_PX + wso].p, (float*)h->ws[WS_PH + wso].p, (float*)h->ws[WS_PQKV + wso].p,
            (float*)h->ws[WS_PMLP + wso].p, (float*)h->ws[WS_PCLS + wso].p};
}

}  // namespace

int precise_ensure(tvc_handle* h, bool text, int n_seq, float** X) {
    const tvc_model_desc& m = h->desc;
    const tvc_tower_arch& a = text ? m.text : m.vision;
    const int P = (m.image_size / m.patch) * (m.image_size / m.patch);
    const int64_t rows = (int64_t)n_seq * (text ? m.ctx : P + 1);
    const int wso = text ? WS_P_N : 0;
    int rc;
    if ((rc = ensure(h, (Slot)(WS_PX + wso), (size_t)rows * a.width * 4))) return rc;
    if ((rc = ensure(h, (Slot)(WS_PH + wso), (size_t)rows * a.width * 4))) return rc;
    size_t qkv_bytes = (size_t)rows * a.width * 3 * 4;
    const size_t cols_bytes = text ? 0 : (size_t)n_seq * P * 3 * m.patch * m.patch * 4;
    if (qkv_bytes < cols_bytes) qkv_bytes = cols_bytes;     // the vision stem parks its im2col rows here
    if ((rc = ensure(h, (Slot)(WS_PQKV + wso), qkv_bytes))) return rc;
    if ((rc = ensure(h, (Slot)(WS_PMLP + wso), (size_t)rows * a.mlp * 4))) return rc;
    if ((rc = ensure(h, (Slot)(WS_PCLS + wso), (size_t)n_seq * a.width * 4 * 2))) return rc;
    *X = p32_bufs(h, text).X;
    return TVC_OK;
}

int precise_stem(tvc_handle* h, const float* pix, int n, const float** patch_out, hipStream_t st) {
    const tvc_model_desc& m = h->desc;
    const int P = (m.image_size / m.patch) * (m.image_size / m.patch), d = m.vision.width, K = 3 * m.patch * m.patch;
    const P32Bufs b = p32_bufs(h, false);
    float* cols = b.QKV;                 // [n*P, K] fp32
    HIP_TRY(launch_im2col_f32(pix, cols, n, m.image_size, m.patch, st));
    *patch_out = b.MLP;                  // [n*P, d]
    return timed_gemm_f32(h, h->vision32.w.patch_w, d, K, cols, (int64_t)n * P, nullptr, b.MLP, d, 0, st);
}

int precise_layers(tvc_handle* h, bool text, int n_seq, int T, hipStream_t st) {
    const tvc_tower_arch& a = text ? h->desc.text : h->desc.vision;
    const tvc_layer_weights_f32* lw = text ? h->text32.w.layers : h->vision32.w.layers;
    const P32Bufs b = p32_bufs(h, text);
    const int causal = text ? 1 : 0;
    const int d = a.width;
    const int64_t rows = (int64_t)n_seq * T;
    int rc;
    for (int l = 0; l < a.layers; ++l) {
        const tvc_layer_weights_f32& w = lw[l];
        HIP_TRY(launch_layernorm(b.X, d, nullptr, nullptr, 0, w.ln1_g, w.ln1_b, nullptr, (int)rows, d, st, nullptr, 0, nullptr, b.H));
        if ((rc = timed_gemm_f32(h, w.wqkv, 3 * d, d, b.H, rows, w.bqkv, b.QKV, 3 * d, 0, st))) return rc;
        {
            ProfScope ps(h, st, TVC_PROF_ATTENTION, 4.0 * n_seq * a.heads * (double)T * T * 64 * (causal ? 0.5 : 1.0));
            HIP_TRY(launch_attention_f32(b.QKV, b.H, n_seq, T, a.heads, causal, st));
        }
        if ((rc = timed_gemm_f32(h, w.wo, d, d, b.H, rows, w.bo, b.X, d, 2, st))) return rc;          // X += out-proj
        HIP_TRY(launch_layernorm(b.X, d, nullptr, nullptr, 0, w.ln2_g, w.ln2_b, nullptr, (int)rows, d, st, nullptr, 0, nullptr, b.H));
        if ((rc = timed_gemm_f32(h, w.w1, a.mlp, d, b.H, rows, w.b1, b.MLP, a.mlp, a.act == TVC_ACT_GELU ? 0 : 1, st))) return rc; // QuickGELU in the epilogue
        if (a.act == TVC_ACT_GELU) HIP_TRY(launch_gelu_erf_f32(b.MLP, rows * a.mlp, st));                                   // erf GELU: a row pass
        if ((rc = timed_gemm_f32(h, w.w2, d, a.mlp, b.MLP, rows, w.b2, b.X, d, 2, st))) return rc;     // X += fc2
    }
    return TVC_OK;
}

int precise_head(tvc_handle* h, bool text, int64_t x_stride, const int32_t* row_idx, int rows, float* out, bool hidden,
                 hipStream_t st) {
    const tvc_model_desc& m = h->desc;
    const int d = text ? m.text.width : m.vision.width;
    const P32Bufs b = p32_bufs(h, text);
    const float* g = text ? h->text32.w.ln_final_g : h->vision32.w.ln_post_g;
    const float* beta = text ? h->text32.w.ln_final_b : h->vision32.w.ln_post_b;
    HIP_TRY(launch_layernorm(b.X, x_stride, row_idx, nullptr, 0, g, beta, nullptr, rows, d, st, nullptr, 0, nullptr,
                             hidden ? out : b.CLS));
    if (hidden) return TVC_OK;
    const float* proj = text ? h->text32.w.proj : h->vision32.w.proj;
    return timed_gemm_f32(h, proj, m.embed_dim, d, b.CLS, rows, nullptr, out, m.embed_dim, 0, st);
}

extern "C" int tvc_set_weights_f32(tvc_handle* h, const tvc_vision_weights_f32* vision, const tvc_text_weights_f32* text) {
    if (!h) return TVC_E_INVALID;
    if (vision) {
        if (!h->vision.set) return fail(h, TVC_E_STATE, "tvc_set_weights_f32: handle was created without a vision tower");
        if (!vision->layers || !vision->patch_w || !vision->proj) return fail(h, TVC_E_INVALID, "tvc_set_weights_f32: NULL vision weights");
        h->vision32.assign(*vision, h->desc.vision.layers);
    }
    if (text) {
        if (!h->text.set) return fail(h, TVC_E_STATE, "tvc_set_weights_f32: handle was created without a text tower");
        if (!text->layers || !text->tok_emb || !text->proj) return fail(h, TVC_E_INVALID, "tvc_set_weights_f32: NULL text weights");
        h->text32.assign(*text, h->desc.text.layers);
    }
    // the split-bf16 planes (TVC_OPT_TOWER_PRECISION = 2) are derived from these tensors: rebuild them when in use
    if (vision || text) {
        tvc_split_free(h);
        if (h->tower_precision == 2) return tvc_split_prepare(h);
    }
    return TVC_OK;
}

extern "C" int tvc_gemm_f32(tvc_handle* h, const float* w_dev, const float* x_dev, const float* bias_dev, float* out_dev, int32_t I,
                            int32_t J, int32_t K, int32_t ld_out, int32_t epilogue, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (I <= 0 || J <= 0 || K <= 0 || K % 4 != 0 || !w_dev || !x_dev || !out_dev || ld_out < I || epilogue < 0 || epilogue > 2)
        return fail(h, TVC_E_INVALID, "tvc_gemm_f32: need K % 4 == 0, ld_out >= I, epilogue in [0, 2]");
    HIP_TRY(launch_gemm_f32(w_dev, K, x_dev, K, bias_dev, out_dev, ld_out, I, J, K, epilogue, (hipStream_t)stream));
    return TVC_OK;
}

extern "C" int tvc_attention_f32(tvc_handle* h, const float* qkv_dev, float* out_dev, int32_t n_seq, int32_t seq_len, int32_t heads,
                                 int32_t causal, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!qkv_dev || !out_dev || seq_len < 1 || seq_len > 288 || heads < 1 || n_seq < 0)
        return fail(h, TVC_E_INVALID, "tvc_attention_f32: need 1 <= seq_len <= 288 and non-NULL buffers");
    HIP_TRY(launch_attention_f32(qkv_dev, out_dev, n_seq, seq_len, heads, causal, (hipStream_t)stream));
    return TVC_OK;
}
