// The input gradient of the vision tower at fp32 grade (TVC_OPT_GRAD_PRECISION = 2, include/tvc.h): the split-bf16 tower
// (tvc_split.cpp) run forward with what every layer's backward reads KEPT in fp32, then the backward of
// tvc_encode_image_backward (tvc_abi.cpp) step for step with fp32 gradients: every dX GEMM is split_gemm3 on hi | lo
// planes of the TRANSPOSED weight against the gradient rows split to planes by rows_split; the attention backward is
// attention_split_bwd.hip; the row kernels are the fp32 forms of backward.hip.  Same scope as the bf16 path: vision
// tower, QuickGELU, one pass, input gradient only, no atomics.
//
// Kept (grad_split_keep_plan, host_plan.hpp; WS_GS_KEEP): per layer the input rows, QKV rows, out-projection output and
// FC1 pre-activation; the ln_post input and the un-normalised embedding.
// Backward, per layer (dX = the fp32 gradient of the residual stream, Gp = its planes):
//     dM = W2^T_s x Gp              dU = dM gelu'(U)           R = W1^T_s x split(dU)        dX += ln_2'(X + D1; R)
//     dAO = Wo^T_s x Gp             dQKV = attention'(QKV, dAO)   R = Wqkv^T_s x split(dQKV)   dX += ln_1'(X; R)
// The two drivers are declared in handle.hpp; tvc_abi.cpp owns the argument checks they share with the bf16 path.
#include "handle.hpp"

#include <initializer_list>

namespace {

constexpr const char* FWD = "tvc_encode_image_grad";
constexpr const char* BWD = "tvc_encode_image_backward";

struct Geo {
    int B, P, T, d, mlp, D, K, Kp, layers, heads;
    int64_t rows;
};
Geo geo(const tvc_handle* h, int B) {
    const tvc_model_desc& m = h->desc;
    Geo g;
    const int gside = m.image_size / m.patch;
    g.B = B; g.P = gside * gside; g.T = g.P + 1; g.d = m.vision.width; g.mlp = m.vision.mlp; g.D = m.embed_dim;
    g.K = 3 * m.patch * m.patch; g.Kp = (g.K + 63) / 64 * 64; g.layers = m.vision.layers; g.heads = m.vision.heads;
    g.rows = (int64_t)B * g.T;
    return g;
}

// fp32 W [I, K] -> handle-owned planes of W^T: [round_up(K, 256), 2 * I] (I % 64 == 0: it is the GEMM's reduction)
int split_weight_t(tvc_handle* h, const float* w, int I, int K, uint16_t** out, hipStream_t st) {
    const size_t bytes = ((size_t)K + 255) / 256 * 256 * 2 * I * 2;
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return fail(h, TVC_E_NOMEM, "transposed split weights: allocation failed");
    h->split_owned.push_back(p);
    HIP_TRY(hipMemsetAsync(p, 0, bytes, st));
    HIP_TRY(launch_rows_split_t(w, K, (uint16_t*)p, I, K, I, st));
    *out = (uint16_t*)p;
    return TVC_OK;
}

// once per set of split planes (tvc_split_free drops both): 1.2 GB more at ViT-L/14
int build_transposed_planes(tvc_handle* h, hipStream_t st) {
    if (!h->vsplit_t.empty()) return TVC_OK;
    const Geo g = geo(h, 1);
    const tvc_vision_weights_f32& vw = h->vision32.w;
    std::vector<SplitLayer> t(g.layers);
    int rc = TVC_OK;
    for (int l = 0; l < g.layers && !rc; ++l) {
        const tvc_layer_weights_f32& w = vw.layers[l];
        if ((rc = split_weight_t(h, w.wqkv, 3 * g.d, g.d, &t[l].wqkv, st))) break;       // [3d, d] -> [d, 2 * 3d]
        if ((rc = split_weight_t(h, w.wo, g.d, g.d, &t[l].wo, st))) break;
        if ((rc = split_weight_t(h, w.w1, g.mlp, g.d, &t[l].w1, st))) break;             // [mlp, d] -> [d, 2 * mlp]
        if ((rc = split_weight_t(h, w.w2, g.d, g.mlp, &t[l].w2, st))) break;             // [d, mlp] -> [mlp, 2 * d]
    }
    if (!rc) rc = split_weight_t(h, vw.proj, g.D, g.d, &h->vsplit_proj_t, st);            // [D, d] -> [d, 2 * D]
    if (!rc) rc = split_weight_t(h, vw.patch_w, g.d, g.K, &h->vsplit_patch_t, st);        // [d, K] -> [K (rows to 256), 2 * d]
    if (rc) { h->vsplit_proj_t = h->vsplit_patch_t = nullptr; return rc; }               // the blocks stay owned by split_owned
    h->vsplit_t = t;
    return TVC_OK;
}

struct Keep { SplitKeep layers; float *xl, *emb; };
Keep keep_of(tvc_handle* h, const GradSplitKeepPlan& p) {
    float* base = (float*)h->ws[WS_GS_KEEP].p;
    Keep k;
    k.layers.x = base + p.x_off; k.layers.qkv = base + p.qkv_off; k.layers.d1 = base + p.d1_off; k.layers.u = base + p.u_off;
    k.xl = base + p.xl_off; k.emb = base + p.emb_off;
    return k;
}

}  // namespace

int grad_split_forward(tvc_handle* h, const float* pix, int B, float* out, int normalize, hipStream_t st) {
    if (!h->vision32.set)
        return fail(h, TVC_E_STATE, std::string(FWD) + ": TVC_OPT_GRAD_PRECISION = 2 needs tvc_set_weights_f32 (vision)");
    if (!h->split_ready || h->vsplit.empty() || !h->vsplit_patch)
        return fail(h, TVC_E_STATE, std::string(FWD) + ": TVC_OPT_GRAD_PRECISION = 2 needs the split planes of the vision weights: set the "
                                                       "option (or TVC_OPT_TOWER_PRECISION = 2) after tvc_set_weights_f32");
    const Geo g = geo(h, B);
    const GradSplitKeepPlan plan = grad_split_keep_plan(B, g.T, g.d, g.mlp, g.layers, g.D);
    if (!plan.ok) return fail(h, TVC_E_INVALID, std::string(FWD) + ": the kept state does not fit size_t");
    int rc;
    float* X;
    if ((rc = split_ensure(h, false, B, &X))) return rc;
    if ((rc = ensure(h, WS_GS_KEEP, plan.total_bytes))) return rc;
    const Keep k = keep_of(h, plan);
    const float* patch_out;
    if ((rc = split_stem(h, pix, B, &patch_out, st))) return rc;
    const tvc_vision_weights_f32& vw = h->vision32.w;
    HIP_TRY(launch_assemble_lnpre(patch_out, vw.cls, vw.pos, vw.ln_pre_g, vw.ln_pre_b, X, B, g.T, g.d, st));
    const float *d1, *d2;
    if ((rc = split_layers_keep(h, B, g.T, k.layers, &d1, &d2, st))) return rc;
    // ln_post on the class rows, as split_head: the sum X + D1 + D2 (its input) is written back to X's class rows and kept
    float* cls = (float*)h->ws[WS_SCLS].p;
    HIP_TRY(launch_ln_split(X, (int64_t)g.T * g.d, nullptr, d1, d2, 1, vw.ln_post_g, vw.ln_post_b, nullptr, cls, B, g.d, st));
    HIP_TRY(hipMemcpy2DAsync(k.xl, (size_t)g.d * 4, X, (size_t)g.T * g.d * 4, (size_t)g.d * 4, B, hipMemcpyDeviceToDevice, st));
    if ((rc = timed_gemm_f32(h, vw.proj, g.D, g.d, cls, B, nullptr, k.emb, g.D, 0, st))) return rc;
    HIP_TRY(hipMemcpyAsync(out, k.emb, (size_t)B * g.D * 4, hipMemcpyDeviceToDevice, st));
    if (normalize) HIP_TRY(launch_l2norm_rows(out, B, g.D, st));
    return TVC_OK;
}

int grad_split_backward(tvc_handle* h, const float* grad_out, float* grad_pix, hipStream_t st) {
    if (!h->vision32.set || !h->split_ready || h->vsplit.empty() || !h->ws[WS_GS_KEEP].p)
        return fail(h, TVC_E_STATE, std::string(BWD) + ": the fp32 weights or their split planes changed since tvc_encode_image_grad");
    const Geo g = geo(h, h->grad_B);
    const GradSplitKeepPlan plan = grad_split_keep_plan(g.B, g.T, g.d, g.mlp, g.layers, g.D);
    if (!plan.ok || h->ws[WS_GS_KEEP].n < plan.total_bytes) return fail(h, TVC_E_STATE, std::string(BWD) + ": call tvc_encode_image_grad first");
    const Keep k = keep_of(h, plan);
    const int d = g.d, mlp = g.mlp, D = g.D, B = g.B;
    const int64_t rows = g.rows, BP = (int64_t)B * g.P;
    const int wide = mlp > 3 * d ? mlp : 3 * d;
    int rc;
    float* X;
    if ((rc = build_transposed_planes(h, st))) return rc;
    if ((rc = split_ensure(h, false, B, &X))) return rc;                          // the stem's workspace (patch rows again)
    size_t wide_elems = (size_t)rows * wide;
    if (wide_elems < (size_t)BP * g.Kp) wide_elems = (size_t)BP * g.Kp;
    if ((rc = ensure(h, WS_GDX, (size_t)rows * d * 4))) return rc;
    if ((rc = ensure(h, WS_GS_GP, (size_t)tile_rows(rows) * 2 * d * 2))) return rc;
    if ((rc = ensure(h, WS_GS_MP, (size_t)tile_rows(rows) * 2 * wide * 2))) return rc;
    if ((rc = ensure(h, WS_GS_WIDE, wide_elems * 4))) return rc;
    if ((rc = ensure(h, WS_GS_ROW, (size_t)rows * d * 4))) return rc;
    if ((rc = ensure(h, WS_GSTATS, (size_t)rows * g.heads * 16))) return rc;
    if ((rc = ensure(h, WS_GS_SMALL, (size_t)B * (D + d) * 4 + (size_t)tile_rows(B) * 2 * D * 2))) return rc;
    float* dX = (float*)h->ws[WS_GDX].p;
    uint16_t* Gp = (uint16_t*)h->ws[WS_GS_GP].p;            // planes [rows(+), 2d]
    uint16_t* Mp = (uint16_t*)h->ws[WS_GS_MP].p;            // planes [rows(+), 2 * mlp] / [rows(+), 2 * 3d]
    float* W = (float*)h->ws[WS_GS_WIDE].p;                 // dM [rows, mlp] / dQKV [rows, 3d] / dcols [B * P, Kp]
    float* R = (float*)h->ws[WS_GS_ROW].p;                  // [rows, d]: a GEMM's output on its way into a LayerNorm backward / dAO
    float* stats = (float*)h->ws[WS_GSTATS].p;
    auto split = [&](const float* x, uint16_t* planes, int64_t n, int K) -> int {
        ProfScope ps(h, st, TVC_PROF_ROWOPS, (double)n * K * 8.0);
        HIP_TRY(launch_rows_split(x, K, planes, n, K, K, 0, st));
        return TVC_OK;
    };
    // ---- head: L2 normalise, projection, ln_post (the gradient lives on the class rows only)
    float* dP = (float*)h->ws[WS_GS_SMALL].p;               // [B, D]
    float* dHc = dP + (size_t)B * D;                        // [B, d]
    uint16_t* dPp = (uint16_t*)(dHc + (size_t)B * d);       // planes [B(+), 2D]
    HIP_TRY(launch_l2norm_bwd_f32(k.emb, grad_out, dP, B, D, h->grad_normalize, st));
    if ((rc = split(dP, dPp, B, D))) return rc;
    if ((rc = split_gemm3(h, h->vsplit_proj_t, d, D, dPp, B, nullptr, dHc, d, st))) return rc;
    HIP_TRY(hipMemsetAsync(dX, 0, (size_t)rows * d * 4, st));
    HIP_TRY(launch_layernorm_bwd_f32(k.xl, d, nullptr, dHc, h->vision32.w.ln_post_g, nullptr, dX, B, d, (int64_t)g.T * d, st));
    if ((rc = split(dX, Gp, rows, d))) return rc;
    // ---- layers, last to first, on what the forward kept
    for (int l = g.layers - 1; l >= 0; --l) {
        const tvc_layer_weights_f32& w = h->vision32.w.layers[l];
        const SplitLayer& wt = h->vsplit_t[l];
        const float* Xl = k.layers.x + (size_t)l * rows * d;
        const float* QKV = k.layers.qkv + (size_t)l * rows * 3 * d;
        const float* D1 = k.layers.d1 + (size_t)l * rows * d;
        const float* U = k.layers.u + (size_t)l * rows * mlp;
        // MLP branch
        if ((rc = split_gemm3(h, wt.w2, mlp, d, Gp, rows, nullptr, W, mlp, st))) return rc;
        {
            ProfScope ps(h, st, TVC_PROF_ROWOPS, (double)rows * mlp * 12.0);
            HIP_TRY(launch_gelu_bwd_f32(W, U, rows * mlp, st));
        }
        if ((rc = split(W, Mp, rows, mlp))) return rc;
        if ((rc = split_gemm3(h, wt.w1, d, mlp, Mp, rows, nullptr, R, d, st))) return rc;
        HIP_TRY(launch_layernorm_bwd_f32(Xl, d, D1, R, w.ln2_g, dX, dX, (int)rows, d, d, st));
        if ((rc = split(dX, Gp, rows, d))) return rc;
        // attention branch
        if ((rc = split_gemm3(h, wt.wo, d, d, Gp, rows, nullptr, R, d, st))) return rc;
        {
            ProfScope ps(h, st, TVC_PROF_ATTENTION, 3.0 * 14.0 * B * g.heads * (double)g.T * g.T * 64);
            HIP_TRY(launch_attention_split_bwd(QKV, R, W, stats, B, g.T, g.heads, st));
        }
        if ((rc = split(W, Mp, rows, 3 * d))) return rc;
        if ((rc = split_gemm3(h, wt.wqkv, d, 3 * d, Mp, rows, nullptr, R, d, st))) return rc;
        HIP_TRY(launch_layernorm_bwd_f32(Xl, d, nullptr, R, w.ln1_g, dX, dX, (int)rows, d, d, st));
        if (l > 0 && (rc = split(dX, Gp, rows, d))) return rc;
    }
    // ---- stem: ln_pre, patch embedding, col2im (the patch rows are computed again, as in the bf16 path)
    const float* patch_out;
    if ((rc = split_stem(h, h->grad_pix, B, &patch_out, st))) return rc;
    HIP_TRY(launch_lnpre_bwd_f32(patch_out, h->vision32.w.pos, h->vision32.w.ln_pre_g, dX, R, B, g.T, d, st));
    if ((rc = split(R, Gp, BP, d))) return rc;
    if ((rc = split_gemm3(h, h->vsplit_patch_t, g.Kp, d, Gp, BP, nullptr, W, g.Kp, st))) return rc;
    HIP_TRY(launch_col2im(W, grad_pix, B, h->desc.image_size, h->desc.patch, g.Kp, st));
    return TVC_OK;
}

// ---- building blocks exported for parity tests (include/tvc.h)
// tvc_grad_split_op: ONE fp32 row kernel of the split-bf16 backward on the caller's buffers, under tvc_tower_op's rules -- every
// case checks its own pointers, alignments and extents (TVC_E_INVALID, nothing launched), then calls ONE launcher; no handle state.
extern "C" int tvc_grad_split_op(tvc_handle* h, int32_t op, const tvc_tower_op_args* a, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!a) return fail(h, TVC_E_INVALID, "tvc_grad_split_op: NULL arguments");
    if (op < 0 || op >= TVC_GRAD_SPLIT_OP_COUNT) return fail(h, TVC_E_INVALID, "tvc_grad_split_op: unknown op");
    const hipStream_t st = (hipStream_t)stream;
    const int64_t* i = a->i;
    bool ok = true;
    auto req = [&](const void* p, int al) { ok = ok && p && !((uintptr_t)p & (uintptr_t)(al - 1)); return const_cast<void*>(p); };
    auto opt = [&](const void* p, int al) { ok = ok && !((uintptr_t)p & (uintptr_t)(al - 1)); return const_cast<void*>(p); };
    // extents: each positive and inside int32, and so is their product
    auto dims = [&](std::initializer_list<int64_t> v) {
        int64_t prod = 1;
        for (int64_t e : v) {
            if (e < 1 || e > INT32_MAX) { ok = false; return; }
            prod *= e;
            if (prod > INT32_MAX) { ok = false; return; }
        }
    };
    auto stride = [&](int64_t ld, int64_t width, int mult) { ok = ok && ld >= width && ld <= INT32_MAX && ld % mult == 0; };
    auto bad = [&]() {
        return fail(h, TVC_E_INVALID, "tvc_grad_split_op: a NULL or misaligned pointer, a misaligned or too short row stride, an extent that "
                                      "is not positive / too large, or a flag out of range");
    };
    switch (op) {
    case TVC_GRAD_SPLIT_OP_GELU_BWD: {
        const float* u = (const float*)req(a->in[0], 16);
        float* dm = (float*)req(a->out[0], 16);
        dims({i[0]});
        if (!ok) return bad();
        HIP_TRY(launch_gelu_bwd_f32(dm, u, i[0], st));
        return TVC_OK;
    }
    case TVC_GRAD_SPLIT_OP_L2NORM_BWD: {
        ok = ok && (i[2] == 0 || i[2] == 1);
        const int normalize = (int)i[2];
        const float* x = (const float*)(normalize ? req(a->in[0], 4) : opt(a->in[0], 4));      // normalize 0 never reads x
        const float* dy = (const float*)req(a->in[1], 4);
        float* dx = (float*)req(a->out[0], 4);
        dims({i[0], i[1]});
        if (!ok) return bad();
        HIP_TRY(launch_l2norm_bwd_f32(x, dy, dx, (int)i[0], (int)i[1], normalize, st));
        return TVC_OK;
    }
    case TVC_GRAD_SPLIT_OP_LNPRE_BWD: {
        const float *patch_out = (const float*)req(a->in[0], 16), *pos = (const float*)req(a->in[1], 16);
        const float *gamma = (const float*)req(a->in[2], 16), *dy = (const float*)req(a->in[3], 16);
        float* dpatch = (float*)req(a->out[0], 16);
        dims({i[0], i[1], i[2]});
        if (!ok || i[1] < 2) return bad();
        HIP_TRY(launch_lnpre_bwd_f32(patch_out, pos, gamma, dy, dpatch, (int)i[0], (int)i[1], (int)i[2], st));
        return TVC_OK;
    }
    case TVC_GRAD_SPLIT_OP_ROWS_SPLIT_T: {
        const float* w = (const float*)req(a->in[0], 4);
        uint16_t* out = (uint16_t*)req(a->out[0], 2);
        dims({i[0], i[3]});
        dims({i[1], i[2], 2});
        stride(i[3], i[1], 1);
        if (!ok || i[2] < i[0]) return bad();
        HIP_TRY(launch_rows_split_t(w, i[3], out, (int)i[0], (int)i[1], (int)i[2], st));
        return TVC_OK;
    }
    case TVC_GRAD_SPLIT_OP_LAYERNORM_BWD: {
        const float* x = (const float*)req(a->in[0], 16);
        const float *delta = (const float*)opt(a->in[1], 16), *dy = (const float*)req(a->in[2], 16);
        const float *gamma = (const float*)req(a->in[3], 16), *dres = (const float*)opt(a->in[4], 16);
        float* dx = (float*)req(a->out[0], 16);
        dims({i[0], i[2]});
        dims({i[0], i[3]});
        dims({i[0], i[1]});
        stride(i[2], i[1], 4);
        stride(i[3], i[1], 4);
        if (!ok) return bad();
        HIP_TRY(launch_layernorm_bwd_f32(x, i[2], delta, dy, gamma, dres, dx, (int)i[0], (int)i[1], i[3], st));
        return TVC_OK;
    }
    }
    return fail(h, TVC_E_INVALID, "tvc_grad_split_op: unknown op");
}

extern "C" int tvc_attention_split_backward(tvc_handle* h, const float* qkv_dev, const float* dout_dev, float* dqkv_dev, int32_t n_seq,
                                            int32_t seq_len, int32_t heads, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!qkv_dev || !dout_dev || !dqkv_dev) return fail(h, TVC_E_INVALID, "tvc_attention_split_backward: NULL buffer");
    if (n_seq < 0 || seq_len < 1 || seq_len > 288 || heads < 1)
        return fail(h, TVC_E_INVALID, "tvc_attention_split_backward: need n_seq >= 0, 1 <= seq_len <= 288 and heads >= 1");
    if (((uintptr_t)qkv_dev | (uintptr_t)dout_dev | (uintptr_t)dqkv_dev) & 15)
        return fail(h, TVC_E_INVALID, "tvc_attention_split_backward: the buffers must be 16-byte aligned");
    if (n_seq == 0) return TVC_OK;
    int rc;
    if ((rc = ensure(h, WS_GSTATS, (size_t)n_seq * seq_len * heads * 16))) return rc;
    HIP_TRY(launch_attention_split_bwd(qkv_dev, dout_dev, dqkv_dev, (float*)h->ws[WS_GSTATS].p, n_seq, seq_len, heads, (hipStream_t)stream));
    return TVC_OK;
}
