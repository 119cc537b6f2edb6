// The latent-diffusion entry points that read no model state (include/tvc.h): tvc_preprocess_images, the streaming attention
// on the caller's buffers (tvc_sd_attention, tvc_sd_attention_ex) and tvc_sd_op, ONE row kernel of sd_ops.hip per call, for the
// parity tests.  The model, its arena and the sampling loop are tvc_sd.cpp.
#include "handle.hpp"

extern "C" {

int tvc_preprocess_images(tvc_handle* h, const float* images_dev, int32_t n, int32_t H, int32_t W, int32_t S, int32_t filter,
                          int32_t keep_aspect, const float* mean3, const float* std3, float* out_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (n < 0 || H < 1 || W < 1 || S < 1 || !mean3 || !std3 || (n > 0 && (!images_dev || !out_dev)) || filter < 0 || filter > 1)
        return fail(h, TVC_E_INVALID, "tvc_preprocess_images: bad arguments");
    int Hr = S, Wr = S;
    if (keep_aspect) {               // short side -> S (rounded as PIL does), centre crop
        if (H <= W) Wr = (int)((double)W * S / H + 0.5); else Hr = (int)((double)H * S / W + 0.5);
        if (Hr < S) Hr = S;
        if (Wr < S) Wr = S;
    }
    HIP_TRY(sd_resize_norm(images_dev, out_dev, n, H, W, Hr, Wr, (Hr - S) / 2, (Wr - S) / 2, S, filter, mean3, std3, (hipStream_t)stream));
    return TVC_OK;
}

int tvc_sd_attention(tvc_handle* h, const uint16_t* q_dev, const uint16_t* k_dev, const uint16_t* v_dev, uint16_t* out_dev, int32_t n,
                     int32_t heads, int32_t Tq, int32_t Tk, int32_t dh, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!q_dev || !k_dev || !v_dev || !out_dev || n < 1 || heads < 1 || Tq < 1 || Tk < 1 || dh < 8 || dh > 160 || dh % 8)
        return fail(h, TVC_E_INVALID, "tvc_sd_attention: need head_dim % 8 == 0 and <= 160, non-NULL buffers");
    const int64_t ld = (int64_t)heads * dh;
    HIP_TRY(sd_flash_attention(q_dev, ld, k_dev, ld, v_dev, ld, out_dev, ld, n, heads, Tq, Tk, dh, (hipStream_t)stream, h->sd_precision == 1));
    return TVC_OK;
}

int tvc_sd_attention_ex(tvc_handle* h, const uint16_t* q_dev, int64_t ldq, const uint16_t* k_dev, int64_t ldk, const uint16_t* v_dev,
                        int64_t ldv, uint16_t* out_dev, int64_t ldo, int32_t n, int32_t heads, int32_t Tq, int32_t Tk, int32_t dh,
                        void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!q_dev || !k_dev || !v_dev || !out_dev || n < 1 || heads < 1 || Tq < 1 || Tk < 1 || dh < 8 || dh > 160 || dh % 8)
        return fail(h, TVC_E_INVALID, "tvc_sd_attention_ex: need head_dim % 8 == 0 and <= 160, non-NULL buffers");
    // the alignment rule of sd_flash_attention (16-byte loads of q / k / v pieces, 8-byte stores) and rows that hold all heads
    const int64_t w = (int64_t)heads * dh;
    if (ldq < w || ldk < w || ldv < w || ldo < w || ldq % 8 || ldk % 8 || ldv % 8 || ldo % 4 ||
        ((uintptr_t)q_dev & 15) || ((uintptr_t)k_dev & 15) || ((uintptr_t)v_dev & 15) || ((uintptr_t)out_dev & 7))
        return fail(h, TVC_E_INVALID, "tvc_sd_attention_ex: need ldq / ldk / ldv % 8 == 0, ldo % 4 == 0, every stride >= heads * dh, "
                                      "q / k / v 16-byte and out 8-byte aligned");
    HIP_TRY(sd_flash_attention(q_dev, ldq, k_dev, ldk, v_dev, ldv, out_dev, ldo, n, heads, Tq, Tk, dh, (hipStream_t)stream,
                               h->sd_precision == 1));
    return TVC_OK;
}

// One row kernel on the caller's buffers (include/tvc.h, tvc_sd_op_args: which slot carries what).  Every case checks its
// own pointers and extents, then calls ONE launcher of kernels.hpp; what a launcher itself rejects comes back as TVC_E_HIP.
int tvc_sd_op(tvc_handle* h, int32_t op, const tvc_sd_op_args* a, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!a) return fail(h, TVC_E_INVALID, "tvc_sd_op: NULL arguments");
    if (op < 0 || op >= TVC_SD_OP_COUNT) return fail(h, TVC_E_INVALID, "tvc_sd_op: unknown op");
    const hipStream_t st = (hipStream_t)stream;
    const int f16 = h->sd_precision == 1;
    const int64_t* i = a->i;
    const float* f = a->f;
    bool ok = true;
    // a required pointer: non-NULL and aligned for the kernel's accesses (16-byte vectors of 16-bit tensors, fp32 words)
    auto p16 = [&](const void* p) { ok = ok && p && !((uintptr_t)p & 15); return (uint16_t*)p; };
    auto p32 = [&](const void* p) { ok = ok && p && !((uintptr_t)p & 3); return (float*)p; };
    auto opt16 = [&](const void* p) { ok = ok && !((uintptr_t)p & 15); return (uint16_t*)p; };
    auto opt32 = [&](const void* p) { ok = ok && !((uintptr_t)p & 3); return (float*)p; };
    // the first `k` extents: positive, and their product (what the kernels index rows with) inside int32
    auto dims = [&](int k, int64_t lo = 1) {
        int64_t prod = 1;
        for (int j = 0; j < k; ++j) {
            if (i[j] < lo || i[j] > INT32_MAX) { ok = false; return; }
            prod *= i[j] > 0 ? i[j] + 2 : 1;          // + 2: the padded layout's rows
            if (prod > INT32_MAX) { ok = false; return; }
        }
    };
    auto flag = [&](int j) { ok = ok && (i[j] == 0 || i[j] == 1); return (int)i[j]; };
    auto bad = [&]() { return fail(h, TVC_E_INVALID, "tvc_sd_op: a NULL or misaligned pointer, or an extent that is not positive / too large"); };
    switch (op) {
    case TVC_SD_OP_GROUPNORM: {
        const uint16_t* x = p16(a->in[0]);
        const float *tadd = opt32(a->in[1]), *g = p32(a->in[2]), *b = p32(a->in[3]);
        uint16_t* y = p16(a->out[0]);
        dims(4);
        const int silu = flag(5), in_pad = flag(6), out_pad = flag(7);
        if (!ok || i[4] < 1 || i[4] > INT32_MAX || (tadd && i[8] < i[3])) return bad();
        const int n = (int)i[0], H = (int)i[1], W = (int)i[2], C = (int)i[3], groups = (int)i[4];
        if (int rc = ensure(h, WS_SD0, sd_groupnorm_ws_floats(n, H * W, groups) * 4)) return rc;
        HIP_TRY(sd_groupnorm(x, tadd, i[8], g, b, y, n, H, W, C, groups, f[0], silu, in_pad, out_pad, (float*)h->ws[WS_SD0].p, st, f16));
        return TVC_OK;
    }
    case TVC_SD_OP_LAYERNORM: {
        const uint16_t* x = p16(a->in[0]);
        const float *g = p32(a->in[1]), *b = p32(a->in[2]);
        const uint16_t* add = opt16(a->in[3]);
        uint16_t *y = p16(a->out[0]), *sum_out = opt16(a->out[1]);
        dims(1, 0);
        if (!ok || i[1] < 1 || i[1] > INT32_MAX) return bad();
        HIP_TRY(sd_layernorm_bf16(x, g, b, y, i[0], (int)i[1], f[0], st, add, sum_out, f16));
        return TVC_OK;
    }
    case TVC_SD_OP_GEGLU: {
        const uint16_t* in = p16(a->in[0]);
        uint16_t* out = p16(a->out[0]);
        dims(2);
        if (!ok) return bad();
        HIP_TRY(sd_geglu(in, out, i[0], (int)i[1], st, f16));
        return TVC_OK;
    }
    case TVC_SD_OP_ADD: {
        const uint16_t *x = p16(a->in[0]), *y = p16(a->in[1]);
        uint16_t* out = p16(a->out[0]);
        dims(1);
        if (!ok) return bad();
        HIP_TRY(sd_add_bf16(x, y, out, i[0], st, f16));
        return TVC_OK;
    }
    case TVC_SD_OP_ADD_PADDED: {
        const uint16_t *x = p16(a->in[0]), *y = p16(a->in[1]);
        uint16_t* out = p16(a->out[0]);
        dims(4);
        if (!ok) return bad();
        HIP_TRY(sd_add_padded(x, y, out, (int)i[0], (int)i[1], (int)i[2], (int)i[3], st, f16));
        return TVC_OK;
    }
    case TVC_SD_OP_RELAYOUT: {
        const uint16_t* in = p16(a->in[0]);
        uint16_t* out = p16(a->out[0]);
        dims(4);
        const int in_pad = flag(4), out_pad = flag(5), up = flag(6);
        if (!ok) return bad();
        HIP_TRY(sd_relayout(in, out, (int)i[0], (int)i[1], (int)i[2], (int)i[3], in_pad, out_pad, up, st));
        return TVC_OK;
    }
    case TVC_SD_OP_IM2COL3X3: {
        const uint16_t* in = p16(a->in[0]);
        uint16_t* out = p16(a->out[0]);
        dims(4);
        const int up = flag(5);
        // 9 columns per source pixel of the (upsampled) source: the output's element count stays inside int32 too
        if (!ok || i[4] < 1 || i[4] > INT32_MAX || i[0] * i[1] * i[2] * i[3] * (up ? 36 : 9) > INT32_MAX) return bad();
        HIP_TRY(sd_im2col3x3(in, out, (int)i[0], (int)i[1], (int)i[2], (int)i[3], (int)i[4], up, st));
        return TVC_OK;
    }
    case TVC_SD_OP_IM2COL_IN: {
        const float* in = p32(a->in[0]);
        uint16_t* out = p16(a->out[0]);
        dims(4);
        if (!ok || i[4] < 1 || i[4] > INT32_MAX) return bad();
        HIP_TRY(sd_im2col_in(in, out, (int)i[0], (int)i[1], (int)i[2], (int)i[3], (int)i[4], f[0], st, f16));
        return TVC_OK;
    }
    case TVC_SD_OP_CONCAT: {
        const uint16_t *x = p16(a->in[0]), *y = p16(a->in[1]);
        uint16_t* out = p16(a->out[0]);
        dims(3);
        if (!ok) return bad();
        HIP_TRY(sd_concat(x, (int)i[0], y, (int)i[1], out, i[2], st));
        return TVC_OK;
    }
    case TVC_SD_OP_CAST_SILU: {
        const float* in = p32(a->in[0]);
        uint16_t* out = (uint16_t*)a->out[0];
        ok = ok && out && !((uintptr_t)out & 1);         // scalar 16-bit stores
        dims(1);
        const int silu = flag(1);
        if (!ok) return bad();
        HIP_TRY(sd_cast_silu(in, out, i[0], silu, st, f16));
        return TVC_OK;
    }
    case TVC_SD_OP_TOKENS_TO_NCHW: {
        const float* in = p32(a->in[0]);
        float* out = p32(a->out[0]);
        dims(4);
        const int clamp = flag(5), in_pad = flag(6);
        if (!ok || i[4] < i[1] || i[4] > INT32_MAX) return bad();
        HIP_TRY(sd_tokens_to_nchw(in, i[4], out, (int)i[0], (int)i[1], (int)i[2], (int)i[3], f[0], f[1], clamp, in_pad, st));
        return TVC_OK;
    }
    case TVC_SD_OP_POINTWISE_SMALL: {
        const float *in = p32(a->in[0]), *w = p32(a->in[1]), *b = p32(a->in[2]);
        float* out = p32(a->out[0]);
        dims(3);
        if (!ok) return bad();
        HIP_TRY(sd_pointwise_small(in, w, b, out, (int)i[0], (int)i[1], (int)i[2], f[0], st));
        return TVC_OK;
    }
    case TVC_SD_OP_CFG: {
        const float* e = p32(a->in[0]);
        float* out = p32(a->out[0]);
        dims(1);
        if (!ok) return bad();
        HIP_TRY(sd_cfg(e, out, i[0], f[0], st));
        return TVC_OK;
    }
    case TVC_SD_OP_LINCOMB: {
        const float *sample = p32(a->in[0]), *e0 = p32(a->in[1]);
        const float *e1 = opt32(a->in[2]), *e2 = opt32(a->in[3]), *e3 = opt32(a->in[4]);
        float* out = p32(a->out[0]);
        dims(1);
        if (!ok) return bad();
        HIP_TRY(sd_lincomb(out, sample, f[0], f[1], e0, f[2], e1, f[3], e2, f[4], e3, f[5], i[0], st));
        return TVC_OK;
    }
    case TVC_SD_OP_SOFTMAX_ROWS: {
        const float* s = p32(a->in[0]);
        uint16_t* p = (uint16_t*)a->out[0];
        ok = ok && p && !((uintptr_t)p & 1);
        dims(2);
        if (!ok || !(f[0] > 0.f)) return bad();
        HIP_TRY(sd_softmax_rows(s, p, i[0], (int)i[1], f[0], st, f16));
        return TVC_OK;
    }
    case TVC_SD_OP_NCHW_TO_TOKENS: {
        const float* in = p32(a->in[0]);
        uint16_t* out = (uint16_t*)a->out[0];
        ok = ok && out && !((uintptr_t)out & 1);
        dims(3);
        if (!ok) return bad();
        HIP_TRY(sd_nchw_to_tokens(in, out, (int)i[0], (int)i[1], (int)i[2], st, f16));
        return TVC_OK;
    }
    case TVC_SD_OP_TOKENS16_TO_NCHW: {
        const uint16_t* in = (const uint16_t*)a->in[0];
        ok = ok && in && !((uintptr_t)in & 1);
        float* out = p32(a->out[0]);
        dims(3);
        if (!ok) return bad();
        HIP_TRY(sd_tokens_bf16_to_nchw(in, out, (int)i[0], (int)i[1], (int)i[2], st, f16));
        return TVC_OK;
    }
    case TVC_SD_OP_TIMESTEP_EMBED: {
        uint16_t* out = (uint16_t*)a->out[0];
        ok = ok && out && !((uintptr_t)out & 1);
        dims(2);
        if (!ok || (i[1] & 1)) return bad();
        HIP_TRY(sd_timestep_embed(out, (int)i[0], (int)i[1], f[0], st, f16));
        return TVC_OK;
    }
    case TVC_SD_OP_TRANSPOSE: {
        const uint16_t* in = (const uint16_t*)a->in[0];
        uint16_t* out = (uint16_t*)a->out[0];
        ok = ok && in && out && !(((uintptr_t)in | (uintptr_t)out) & 1);
        dims(2);
        if (!ok) return bad();
        HIP_TRY(launch_transpose_bf16(in, out, (int)i[0], (int)i[1], st));
        return TVC_OK;
    }
    }
    return fail(h, TVC_E_INVALID, "tvc_sd_op: unknown op");
}

}  // extern "C"
