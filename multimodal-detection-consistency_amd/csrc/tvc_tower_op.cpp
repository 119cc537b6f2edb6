// tvc_tower_op (include/tvc.h, tvc_tower_op_args: which slot carries what): ONE row kernel of the CLIP towers -- forward,
// backward, split and fp32-grade modes, the text length kernels -- on the caller's buffers, for the parity tests.  Every
// case checks its own pointers, alignments and extents (TVC_E_INVALID, nothing launched), then calls ONE launcher of
// kernels.hpp; what a launcher itself rejects comes back as TVC_E_HIP.  No handle state is read: no weights, no workspace.
#include "handle.hpp"

#include <initializer_list>

extern "C" int tvc_tower_op(tvc_handle* h, int32_t op, const tvc_tower_op_args* a, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (!a) return fail(h, TVC_E_INVALID, "tvc_tower_op: NULL arguments");
    if (op < 0 || op >= TVC_TOWER_OP_COUNT) return fail(h, TVC_E_INVALID, "tvc_tower_op: unknown op");
    const hipStream_t st = (hipStream_t)stream;
    const int64_t* i = a->i;
    bool ok = true;
    // a required / an optional pointer, aligned to `al` bytes (the widest access the kernel makes through it)
    auto req = [&](const void* p, int al) { ok = ok && p && !((uintptr_t)p & (uintptr_t)(al - 1)); return const_cast<void*>(p); };
    auto opt = [&](const void* p, int al) { ok = ok && !((uintptr_t)p & (uintptr_t)(al - 1)); return const_cast<void*>(p); };
    // extents: each positive and inside int32, and so is their product (rows * columns: what a kernel may index with)
    auto dims = [&](std::initializer_list<int64_t> v) {
        int64_t prod = 1;
        for (int64_t e : v) {
            if (e < 1 || e > INT32_MAX) { ok = false; return; }
            prod *= e;
            if (prod > INT32_MAX) { ok = false; return; }
        }
    };
    // a row stride in elements: holds a row, and keeps every row as aligned as the first (`mult` elements)
    auto stride = [&](int64_t ld, int64_t width, int mult) { ok = ok && ld >= width && ld <= INT32_MAX && ld % mult == 0; };
    auto flag = [&](int j) { ok = ok && (i[j] == 0 || i[j] == 1); return (int)i[j]; };
    auto bad = [&]() {
        return fail(h, TVC_E_INVALID, "tvc_tower_op: a NULL or misaligned pointer, a misaligned or too short row stride, an extent that is "
                                      "not positive / too large, or a flag out of range");
    };
    switch (op) {
    case TVC_TOWER_OP_LAYERNORM: {
        float* x = (float*)req(a->in[0], 16);
        const int32_t* row_idx = (const int32_t*)opt(a->in[1], 4);
        const uint16_t *delta = (const uint16_t*)opt(a->in[2], 8), *delta2 = (const uint16_t*)opt(a->in[3], 8);
        const float *g = (const float*)req(a->in[4], 16), *b = (const float*)req(a->in[5], 16);
        uint16_t* y = (uint16_t*)opt(a->out[0], 8);
        float *y32 = (float*)opt(a->out[1], 16), *xsum = (float*)opt(a->out[2], 16);
        dims({i[0], i[2]});
        dims({i[0], i[1]});
        stride(i[2], i[1], 4);
        const int write_x = flag(3), compact = flag(4), f16 = flag(5);
        if (!ok || (!y && !y32)) return bad();
        HIP_TRY(launch_layernorm(x, i[2], row_idx, delta, write_x, g, b, y, (int)i[0], (int)i[1], st, delta2, compact, xsum, y32, f16));
        return TVC_OK;
    }
    case TVC_TOWER_OP_LAYERNORM_BWD: {
        const int dy32 = flag(4);
        const float* x = (const float*)req(a->in[0], 16);
        const uint16_t* delta = (const uint16_t*)opt(a->in[1], 8);
        const void* dy = req(a->in[2], dy32 ? 16 : 8);
        const float *gamma = (const float*)req(a->in[3], 16), *dres = (const float*)opt(a->in[4], 16);
        float* dx = (float*)req(a->out[0], 16);
        uint16_t* dx16 = (uint16_t*)opt(a->out[1], 8);
        dims({i[0], i[2]});
        dims({i[0], i[3]});
        dims({i[0], i[1]});
        stride(i[2], i[1], 4);
        stride(i[3], i[1], 4);
        if (!ok) return bad();
        HIP_TRY(launch_layernorm_bwd(x, i[2], delta, dy, dy32, gamma, dres, dx, dx16, (int)i[0], (int)i[1], i[3], st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_LNPRE_BWD: {
        const float *patch_out = (const float*)req(a->in[0], 16), *pos = (const float*)req(a->in[1], 16);
        const float *gamma = (const float*)req(a->in[2], 16), *dy = (const float*)req(a->in[3], 16);
        uint16_t* dpatch = (uint16_t*)req(a->out[0], 8);
        dims({i[0], i[1], i[2]});
        if (!ok || i[1] < 2) return bad();
        HIP_TRY(launch_lnpre_bwd(patch_out, pos, gamma, dy, dpatch, (int)i[0], (int)i[1], (int)i[2], st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_ASSEMBLE_LNPRE: {
        const float* patch_out = (const float*)(i[1] == 1 ? opt(a->in[0], 16) : req(a->in[0], 16));      // T = 1: class rows only
        const float *cls = (const float*)req(a->in[1], 16), *pos = (const float*)req(a->in[2], 16);
        const float *g = (const float*)req(a->in[3], 16), *b = (const float*)req(a->in[4], 16);
        float* x = (float*)req(a->out[0], 16);
        dims({i[0], i[1], i[2]});
        if (!ok) return bad();
        HIP_TRY(launch_assemble_lnpre(patch_out, cls, pos, g, b, x, (int)i[0], (int)i[1], (int)i[2], st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_IM2COL: {
        dims({i[0], 3, i[1], i[1]});
        dims({i[1], i[2]});
        const int f16 = flag(4);
        if (!ok || i[1] % i[2] != 0) return bad();
        const int64_t gside = i[1] / i[2];
        // the LDS form reads image rows as 16-byte vectors (image % 4 == 0); both forms store 16-byte pieces of rows of Kp
        const float* pix = (const float*)req(a->in[0], i[1] % 4 == 0 ? 16 : 4);
        uint16_t* out = (uint16_t*)req(a->out[0], 16);
        dims({i[0], gside * gside, i[3]});
        stride(i[3], 3 * i[2] * i[2], 8);
        if (!ok) return bad();
        HIP_TRY(launch_im2col(pix, out, (int)i[0], (int)i[1], (int)i[2], (int)i[3], st, f16));
        return TVC_OK;
    }
    case TVC_TOWER_OP_IM2COL_F32: {
        const float* pix = (const float*)req(a->in[0], 4);
        float* out = (float*)req(a->out[0], 4);
        dims({i[0], 3, i[1], i[1]});
        dims({i[1], i[2]});
        if (!ok || i[1] % i[2] != 0) return bad();
        HIP_TRY(launch_im2col_f32(pix, out, (int)i[0], (int)i[1], (int)i[2], st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_COL2IM: {
        const float* dcols = (const float*)req(a->in[0], 4);
        float* dpix = (float*)req(a->out[0], 4);
        dims({i[0], 3, i[1], i[1]});
        dims({i[1], i[2]});
        if (!ok || i[1] % i[2] != 0) return bad();
        const int64_t gside = i[1] / i[2];
        dims({i[0], gside * gside, i[3]});
        stride(i[3], 3 * i[2] * i[2], 1);
        if (!ok) return bad();
        HIP_TRY(launch_col2im(dcols, dpix, (int)i[0], (int)i[1], (int)i[2], (int)i[3], st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_GELU_FWD: {
        const uint16_t* u = (const uint16_t*)req(a->in[0], 16);
        uint16_t* out = (uint16_t*)req(a->out[0], 16);
        dims({i[0]});
        if (!ok) return bad();
        HIP_TRY(launch_gelu_fwd(u, out, i[0], st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_GELU_BWD: {
        const uint16_t* u = (const uint16_t*)req(a->in[0], 16);
        uint16_t* dm = (uint16_t*)req(a->out[0], 16);
        dims({i[0]});
        if (!ok) return bad();
        HIP_TRY(launch_gelu_bwd(dm, u, i[0], st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_GELU_ERF_16: {
        uint16_t* x = (uint16_t*)req(a->out[0], 16);
        const int f16 = flag(1);
        dims({i[0]});
        if (!ok) return bad();
        HIP_TRY(launch_gelu_erf_16(x, i[0], f16, st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_GELU_ERF_F32: {
        float* x = (float*)req(a->out[0], 16);
        dims({i[0]});
        if (!ok) return bad();
        HIP_TRY(launch_gelu_erf_f32(x, i[0], st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_L2NORM_ROWS: {
        float* x = (float*)req(a->out[0], 4);
        dims({i[0], i[1]});
        if (!ok) return bad();
        HIP_TRY(launch_l2norm_rows(x, (int)i[0], (int)i[1], st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_L2NORM_BWD: {
        const int normalize = flag(2);
        const float* x = (const float*)(normalize ? req(a->in[0], 4) : opt(a->in[0], 4));      // normalize 0 never reads x
        const float* dy = (const float*)req(a->in[1], 4);
        uint16_t* dx16 = (uint16_t*)req(a->out[0], 2);
        dims({i[0], i[1]});
        if (!ok) return bad();
        HIP_TRY(launch_l2norm_bwd(x, dy, dx16, (int)i[0], (int)i[1], normalize, st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_LN_SPLIT: {
        float* x = (float*)req(a->in[0], 16);
        const int32_t* row_idx = (const int32_t*)opt(a->in[1], 4);
        const float *d1 = (const float*)opt(a->in[2], 16), *d2 = (const float*)opt(a->in[3], 16);
        const float *g = (const float*)req(a->in[4], 16), *b = (const float*)req(a->in[5], 16);
        uint16_t* planes = (uint16_t*)opt(a->out[0], 8);
        float* y32 = (float*)opt(a->out[1], 16);
        dims({i[0], i[2]});
        dims({i[0], i[1], 2});
        stride(i[2], i[1], 4);
        const int write_x = flag(3);
        if (!ok || (!planes && !y32)) return bad();
        HIP_TRY(launch_ln_split(x, i[2], row_idx, d1, d2, write_x, g, b, planes, y32, (int)i[0], (int)i[1], st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_ROWS_SPLIT: {
        const float* x = (const float*)req(a->in[0], 16);
        uint16_t* out = (uint16_t*)req(a->out[0], 8);
        dims({i[0], i[3]});
        dims({i[0], i[2], 2});
        dims({i[1]});
        stride(i[3], i[1], 4);
        if (!ok || i[4] < 0 || i[4] > 2) return bad();
        HIP_TRY(launch_rows_split(x, i[3], out, i[0], (int)i[1], (int)i[2], (int)i[4], st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_SPLIT_PLANES: {
        const float* x = (const float*)req(a->in[0], 16);
        uint16_t* out = (uint16_t*)req(a->out[0], 8);
        dims({i[0], i[1], 2});
        if (!ok || i[2] < 1 || i[2] > 2) return bad();
        HIP_TRY(launch_split_planes(x, out, i[0], (int)i[1], (int)i[2], st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_GATHER_ROWS: {
        const uint16_t* bank = (const uint16_t*)req(a->in[0], 2);
        const int32_t* idx = (const int32_t*)req(a->in[1], 4);
        float* out = (float*)req(a->out[0], 4);
        dims({i[0], i[1]});
        dims({i[2], i[3]});
        if (!ok || i[4] < 1 || i[4] > 2 || i[5] < 0) return bad();
        stride(i[3], i[4] * i[1], 1);
        if (!ok) return bad();
        HIP_TRY(launch_gather_rows(BankRows{bank, i[3], i[2], (int)i[1], (int)i[4]}, idx, i[5], (int)i[0], out, st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_GATHER_F32_ROWS: {
        const float* x = (const float*)req(a->in[0], 16);
        const int32_t* idx = (const int32_t*)opt(a->in[1], 4);
        float* out = (float*)req(a->out[0], 16);
        dims({i[0], i[1]});
        stride(i[2], i[1], 4);
        if (!ok || i[3] < 0 || i[3] > INT32_MAX) return bad();
        HIP_TRY(launch_gather_f32_rows(x, i[2], idx, i[3], out, (int)i[0], (int)i[1], st));
        return TVC_OK;
    }
    case TVC_TOWER_OP_TEXT_LENS_SCAN: {
        const int32_t* tok = (const int32_t*)req(a->in[0], 4);
        int32_t* starts = (int32_t*)req(a->out[0], 4);
        int32_t* pfx = (int32_t*)opt(a->out[1], 4);
        int32_t* lens = (int32_t*)(pfx ? opt(a->out[2], 4) : req(a->out[2], 4));      // with pfx its second half is the scratch
        dims({i[0], i[1]});
        if (!ok || i[2] < 0 || i[2] > INT32_MAX) return bad();
        HIP_TRY(launch_text_lens_scan(tok, starts, pfx, (int)i[0], (int)i[1], (int)i[2], st, lens));
        return TVC_OK;
    }
    case TVC_TOWER_OP_TEXT_EMBED: {
        const int32_t* tok = (const int32_t*)req(a->in[0], 4);
        const float *emb = (const float*)req(a->in[1], 16), *pos = (const float*)req(a->in[2], 16);
        const int32_t *starts = (const int32_t*)opt(a->in[3], 4), *pfx = (const int32_t*)opt(a->in[4], 4);
        float* x = (float*)req(a->out[0], 16);
        int32_t* eot = (int32_t*)req(a->out[1], 4);
        dims({i[0], i[1], i[2]});
        dims({i[3], i[2]});
        if (!ok || (pfx && !starts)) return bad();
        HIP_TRY(launch_text_embed(tok, emb, pos, x, eot, starts, (int)i[0], (int)i[1], (int)i[2], (int)i[3], st, pfx));
        return TVC_OK;
    }
    }
    return fail(h, TVC_E_INVALID, "tvc_tower_op: unknown op");
}
