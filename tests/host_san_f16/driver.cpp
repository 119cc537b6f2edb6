// Host-only sanitizer driver of the fp16 tower mode (tests/test_fp16_host.py): the same build as
// tests/host_san/driver.cpp -- tests/host_san_build.py's, the product's host sources under ASan / UBSan
// against tests/host_san's HIP stand-in, whose GEMM launcher checks every operand / output range -- walking
// TVC_OPT_TOWER_PRECISION = 3: refused before tvc_set_weights_f16, then image / text (dense, packed, grouped, pooled on and
// off, chunked) and hidden-state encodes on the fp16 weight set, the switch back to bf16, and a leak-free tvc_destroy.
#include "driver_common.hpp"

#include <vector>

int main() {
    tvc_handle* h = nullptr;
    // toy two-tower geometry (ViT-T/16-test): widths 256 / 128, 2 layers; the text tower uses erf GELU (the fp16 gelu pass)
    tvc_model_desc m{};
    m.image_size = 64; m.patch = 16; m.vocab = 49408; m.ctx = 77; m.embed_dim = 128;
    m.vision = {256, 2, 4, 512, TVC_ACT_QUICK_GELU}; m.text = {128, 2, 2, 256, TVC_ACT_GELU};
    const int Kp = 768;                                       // 3 * 16 * 16, already a multiple of 64
    std::vector<void*> keep;
    // weights are sized exactly (GEMM weight rows padded to whole 256-row tiles, as tvc_create's contract asks), so the
    // stub's range check sees any slip in the fp16 set's addressing
    auto buf = [&](size_t elems, size_t es) { void* p = dev(elems * es); keep.push_back(p); return p; };
    auto rows256 = [](int r) { return (size_t)(r + 255) / 256 * 256; };
    auto layers = [&](const tvc_tower_arch& a) {
        std::vector<tvc_layer_weights> L(a.layers);
        for (auto& l : L) {
            l.ln1_g = (float*)buf(a.width, 4); l.ln1_b = (float*)buf(a.width, 4); l.ln2_g = (float*)buf(a.width, 4); l.ln2_b = (float*)buf(a.width, 4);
            l.wqkv = (uint16_t*)buf(rows256(3 * a.width) * a.width, 2); l.bqkv = (float*)buf(3 * a.width, 4);
            l.wo = (uint16_t*)buf(rows256(a.width) * a.width, 2); l.bo = (float*)buf(a.width, 4);
            l.w1 = (uint16_t*)buf(rows256(a.mlp) * a.width, 2); l.b1 = (float*)buf(a.mlp, 4);
            l.w2 = (uint16_t*)buf(rows256(a.width) * a.mlp, 2); l.b2 = (float*)buf(a.width, 4);
        }
        return L;
    };
    auto vl = layers(m.vision), tl = layers(m.text);
    tvc_vision_weights vw{};
    vw.patch_w = (uint16_t*)buf(rows256(256) * Kp, 2); vw.cls = (float*)buf(256, 4); vw.pos = (float*)buf(17 * 256, 4);
    vw.ln_pre_g = (float*)buf(256, 4); vw.ln_pre_b = (float*)buf(256, 4); vw.ln_post_g = (float*)buf(256, 4); vw.ln_post_b = (float*)buf(256, 4);
    vw.proj = (uint16_t*)buf(rows256(128) * 256, 2); vw.layers = vl.data();
    tvc_text_weights tw{};
    tw.tok_emb = (float*)buf((size_t)49408 * 128, 4); tw.pos = (float*)buf(77 * 128, 4); tw.ln_final_g = (float*)buf(128, 4);
    tw.ln_final_b = (float*)buf(128, 4); tw.proj = (uint16_t*)buf(rows256(128) * 128, 2); tw.layers = tl.data();
    CHECK(tvc_create(&m, &vw, &tw, &h) == TVC_OK && h);
    // ---- mode 3 is refused until fp16 weights are registered; the refusal leaves the handle in bf16
    CHECK(tvc_set_option(h, TVC_OPT_TOWER_PRECISION, 3) == TVC_E_INVALID && strstr(tvc_last_error(h), "tvc_set_weights_f16"));
    CHECK(tvc_set_option(h, TVC_OPT_TOWER_PRECISION, 4) == TVC_E_INVALID);
    const int B = 5, N = 3;
    float* pix = (float*)buf((size_t)B * 3 * 64 * 64, 4);
    int32_t* tok = (int32_t*)buf((size_t)B * (N + 1) * 77, 4);
    memset(tok, 0, (size_t)B * (N + 1) * 77 * 4);
    float* fi = (float*)buf(B * 128, 4); float* ft = (float*)buf(B * (N + 1) * 128, 4);
    float* hid = (float*)buf((size_t)B * 77 * 128, 4);
    OK(tvc_encode_image(h, pix, B, fi, 1, nullptr));
    // ---- the fp16 weight set: its own GEMM weights, fp32 tensors aliasing the bf16 set's
    auto vl16 = layers(m.vision), tl16 = layers(m.text);
    for (int l = 0; l < m.vision.layers; ++l) {
        vl16[l].ln1_g = vl[l].ln1_g; vl16[l].ln1_b = vl[l].ln1_b; vl16[l].bqkv = vl[l].bqkv; vl16[l].b2 = vl[l].b2;
    }
    tvc_vision_weights vw16 = vw;
    vw16.patch_w = (uint16_t*)buf(rows256(256) * Kp, 2); vw16.proj = (uint16_t*)buf(rows256(128) * 256, 2); vw16.layers = vl16.data();
    tvc_text_weights tw16 = tw;
    tw16.proj = (uint16_t*)buf(rows256(128) * 128, 2); tw16.layers = tl16.data();
    {
        tvc_vision_weights bad = vw16; bad.layers = nullptr;
        CHECK(tvc_set_weights_f16(h, &bad, nullptr) == TVC_E_INVALID);
        CHECK(tvc_set_weights_f16(nullptr, &vw16, &tw16) == TVC_E_INVALID);
    }
    // only the vision set: the text tower refuses mode 3 instead of reading missing weights
    OK(tvc_set_weights_f16(h, &vw16, nullptr));
    OK(tvc_set_option(h, TVC_OPT_TOWER_PRECISION, 3));
    OK(tvc_encode_image(h, pix, B, fi, 1, nullptr));
    CHECK(tvc_encode_text(h, tok, B * (N + 1), ft, 1, nullptr) == TVC_E_STATE);
    CHECK(tvc_encode_text_hidden(h, tok, B, hid, nullptr) == TVC_E_STATE);
    OK(tvc_set_weights_f16(h, nullptr, &tw16));
    // ---- fp16 towers: dense, packed, grouped, pooled on / off, chunked, hidden states
    for (int pooled = 0; pooled < 2; ++pooled)
        for (int pack = 0; pack < 2; ++pack) {
            OK(tvc_set_option(h, TVC_OPT_POOLED_LAST_LAYER, pooled));
            OK(tvc_set_option(h, TVC_OPT_TEXT_PACKING, pack));
            OK(tvc_set_option(h, TVC_OPT_TEXT_GROUP, pack ? N + 1 : 0));
            OK(tvc_encode_image(h, pix, B, fi, 1, nullptr));
            OK(tvc_encode_text(h, tok, B * (N + 1), ft, 1, nullptr));
        }
    OK(tvc_set_option(h, TVC_OPT_MAX_CHUNK_IMAGES, 2)); OK(tvc_set_option(h, TVC_OPT_MAX_CHUNK_TEXTS, 7));
    OK(tvc_encode_image(h, pix, B, fi, 0, nullptr)); OK(tvc_encode_text(h, tok, B * (N + 1), ft, 0, nullptr));
    OK(tvc_encode_text_hidden(h, tok, B, hid, nullptr));
    OK(tvc_set_option(h, TVC_OPT_MAX_CHUNK_IMAGES, 512)); OK(tvc_set_option(h, TVC_OPT_MAX_CHUNK_TEXTS, 4608));
    OK(tvc_encode_text_hidden(h, tok, B, hid, nullptr));
    // the input-gradient path keeps running bf16 in mode 3
    float* gout = (float*)buf(B * 128, 4); float* gpix = (float*)buf((size_t)B * 3 * 64 * 64, 4);
    OK(tvc_encode_image_grad(h, pix, B, fi, 1, nullptr)); OK(tvc_encode_image_backward(h, gout, gpix, nullptr));
    // ---- parity building blocks (argument checks; the stub checks the GEMM ranges)
    uint16_t* a16 = (uint16_t*)buf(256 * 128, 2); uint16_t* b16 = (uint16_t*)buf(300 * 128, 2); float* o32 = (float*)buf(300 * 256, 4);
    OK(tvc_gemm_f16(h, a16, b16, nullptr, o32, 256, 300, 128, 0, 0, 256, 0, nullptr));
    OK(tvc_gemm_f16(h, a16, b16, nullptr, o32, 256, 300, 128, 0, 0, 256, 1, nullptr));
    CHECK(tvc_gemm_f16(h, a16, b16, nullptr, o32, 256, 300, 100, 0, 0, 256, 0, nullptr) == TVC_E_INVALID);
    // ---- the 16-bit GEMM contract (include/tvc.h): padded operand rows, output pitches beyond I, a ragged I, every epilogue;
    // the stub checks each launch's A, B, bias and output ranges against these exactly sized blocks.  Misaligned pointers
    // and pitches of 2^23 or more are refused before any launch.
    {
        const int gI = 301, gJ = 300, gK = 128, ldo = gI + 4;
        const int64_t lda = gK + 8, ldb = gK + 64;
        std::vector<void*> blocks;
        auto exact = [&](size_t bytes) { void* p = dev(bytes); blocks.push_back(p); return p; };
        uint16_t* ga = (uint16_t*)exact(((size_t)(gI - 1) * lda + gK) * 2);
        uint16_t* gb = (uint16_t*)exact(((size_t)(gJ - 1) * ldb + gK) * 2);
        float* gbias = (float*)exact((size_t)gI * 4);
        char* go = (char*)exact(((size_t)(gJ - 1) * ldo + gI) * 4);
        for (int epi = 0; epi < 4; ++epi) {
            OK(tvc_gemm_f16(h, ga, gb, gbias, go, gI, gJ, gK, lda, ldb, ldo, epi, nullptr));
            OK(tvc_gemm_f16(h, ga, gb, nullptr, go, gI, gJ, gK, lda, ldb, gI + 1, epi, nullptr));
        }
        OK(tvc_gemm_f16(h, ga, gb, gbias, go, gI, gJ, gK, gK, ldb, gI, 1, nullptr));
        OK(tvc_gemm_f16(h, ga, gb, gbias, go, 1, gJ, gK, ((int64_t)1 << 23) - 8, ldb, ldo, 0, nullptr));   // one row: any pitch below 2^23
        const int64_t big = (int64_t)1 << 23;
        CHECK(tvc_gemm_f16(h, ga, gb, gbias, go, 1, gJ, gK, big, ldb, ldo, 0, nullptr) == TVC_E_INVALID && strlen(tvc_last_error(h)) > 0);
        CHECK(tvc_gemm_f16(h, ga, gb, gbias, go, gI, 1, gK, lda, big + 64, ldo, 0, nullptr) == TVC_E_INVALID);
        CHECK(tvc_gemm_f16(h, ga + 1, gb, gbias, go, gI, gJ, gK, lda, ldb, ldo, 0, nullptr) == TVC_E_INVALID);
        CHECK(tvc_gemm_f16(h, ga, gb + 4, gbias, go, gI, gJ, gK, lda, ldb, ldo, 0, nullptr) == TVC_E_INVALID);
        CHECK(tvc_gemm_f16(h, ga, gb, gbias + 1, go, gI, gJ, gK, lda, ldb, ldo, 0, nullptr) == TVC_E_INVALID);
        CHECK(tvc_gemm_f16(h, ga, gb, gbias, go + 8, gI, gJ, gK, lda, ldb, ldo, 1, nullptr) == TVC_E_INVALID);
        CHECK(tvc_gemm_f16(h, ga, gb, gbias, go, gI, gJ, gK, gK + 4, ldb, ldo, 0, nullptr) == TVC_E_INVALID);   // not a multiple of 8
        CHECK(tvc_gemm_f16(h, ga, gb, gbias, go, gI, gJ, gK, lda, ldb, gI - 1, 0, nullptr) == TVC_E_INVALID);   // ld_out < I
        for (void* p : blocks) (void)hipFree(p);
    }
    uint16_t* qkv = (uint16_t*)buf((size_t)2 * 77 * 3 * 128, 2); uint16_t* ao = (uint16_t*)buf((size_t)2 * 77 * 128, 2);
    OK(tvc_attention_f16(h, qkv, ao, nullptr, 2, 77, 2, 1, nullptr));
    CHECK(tvc_attention_f16(h, nullptr, ao, nullptr, 2, 77, 2, 1, nullptr) == TVC_E_INVALID);
    OK(tvc_layernorm_f16(h, o32, vw.ln_pre_g, vw.ln_pre_b, ao, 2, 128, nullptr));
    // ---- the attention entry points with every launch option: the stub launchers accept anything, so TVC_E_INVALID here
    // means the call was refused before any launch
    {
        int32_t* st = (int32_t*)buf(3, 4); int32_t* pf = (int32_t*)buf(4, 4); int32_t* pr = (int32_t*)buf(2, 4);
        float* q32 = (float*)buf((size_t)2 * 77 * 3 * 128, 4); uint16_t* pl = (uint16_t*)buf((size_t)2 * 77 * 2 * 128, 2);
        for (int f16 = 0; f16 < 2; ++f16) {
            OK(tvc_attention_ex(h, qkv, ao, nullptr, nullptr, 2, 77, 2, 1, 0, nullptr, f16, nullptr));
            OK(tvc_attention_ex(h, qkv, ao, st, pf, 2, 77, 2, 1, 2, nullptr, f16, nullptr));
            OK(tvc_attention_ex(h, qkv, ao, nullptr, nullptr, 2, 77, 2, 0, 2, pr, f16, nullptr));
            OK(tvc_attention_ex(h, qkv, ao, nullptr, nullptr, 2, 288, 2, 0, 1, nullptr, f16, nullptr));
            CHECK(tvc_attention_ex(h, qkv, ao, nullptr, pf, 2, 77, 2, 1, 0, nullptr, f16, nullptr) == TVC_E_INVALID);   // pfx without starts
            CHECK(tvc_attention_ex(h, qkv, ao, st, pf, 2, 77, 2, 0, 0, nullptr, f16, nullptr) == TVC_E_INVALID);        // pfx without causal
            CHECK(tvc_attention_ex(h, qkv, ao, nullptr, nullptr, 2, 77, 2, 1, 2, nullptr, f16, nullptr) == TVC_E_INVALID && strlen(tvc_last_error(h)) > 0);
            CHECK(tvc_attention_ex(h, qkv, ao, nullptr, nullptr, 2, 77, 2, 1, 3, nullptr, f16, nullptr) == TVC_E_INVALID);
            CHECK(tvc_attention_ex(h, qkv, ao, nullptr, nullptr, 2, 0, 2, 1, 0, nullptr, f16, nullptr) == TVC_E_INVALID);
            CHECK(tvc_attention_ex(h, qkv, ao, nullptr, nullptr, 2, 289, 2, 1, 0, nullptr, f16, nullptr) == TVC_E_INVALID);
            CHECK(tvc_attention_ex(h, qkv, ao, nullptr, nullptr, 2, 77, 0, 1, 0, nullptr, f16, nullptr) == TVC_E_INVALID);
            CHECK(tvc_attention_ex(h, nullptr, ao, nullptr, nullptr, 2, 77, 2, 1, 0, nullptr, f16, nullptr) == TVC_E_INVALID);
        }
        OK(tvc_attention_split_ex(h, q32, pl, st, pf, 2, 77, 2, 1, nullptr));
        OK(tvc_attention_split_ex(h, q32, pl, nullptr, nullptr, 2, 272, 2, 0, nullptr));
        CHECK(tvc_attention_split_ex(h, q32, pl, nullptr, pf, 2, 77, 2, 1, nullptr) == TVC_E_INVALID);
        CHECK(tvc_attention_split_ex(h, q32, pl, st, pf, 2, 77, 2, 0, nullptr) == TVC_E_INVALID);
        CHECK(tvc_attention_split_ex(h, q32, pl, st, nullptr, 2, 273, 2, 1, nullptr) == TVC_E_INVALID);
        CHECK(tvc_attention_split_ex(h, q32, pl, st, nullptr, 2, 0, 2, 1, nullptr) == TVC_E_INVALID);
        CHECK(tvc_attention_split_ex(h, q32, nullptr, st, nullptr, 2, 77, 2, 1, nullptr) == TVC_E_INVALID);
        // streaming attention: 2 heads of 24 in rows of 56 / 64 / 72 / 52 elements
        OK(tvc_sd_attention_ex(h, qkv, 56, qkv, 64, qkv, 72, ao, 52, 2, 2, 5, 7, 24, nullptr));
        CHECK(tvc_sd_attention_ex(h, qkv, 52, qkv, 64, qkv, 72, ao, 52, 2, 2, 5, 7, 24, nullptr) == TVC_E_INVALID);     // ldq % 8
        CHECK(tvc_sd_attention_ex(h, qkv, 56, qkv, 68, qkv, 72, ao, 52, 2, 2, 5, 7, 24, nullptr) == TVC_E_INVALID);     // ldk % 8
        CHECK(tvc_sd_attention_ex(h, qkv, 56, qkv, 64, qkv, 76, ao, 52, 2, 2, 5, 7, 24, nullptr) == TVC_E_INVALID);     // ldv % 8
        CHECK(tvc_sd_attention_ex(h, qkv, 56, qkv, 64, qkv, 72, ao, 50, 2, 2, 5, 7, 24, nullptr) == TVC_E_INVALID);     // ldo % 4
        CHECK(tvc_sd_attention_ex(h, qkv, 40, qkv, 64, qkv, 72, ao, 52, 2, 2, 5, 7, 24, nullptr) == TVC_E_INVALID);     // ldq < heads * dh
        CHECK(tvc_sd_attention_ex(h, qkv + 4, 56, qkv, 64, qkv, 72, ao, 52, 2, 2, 5, 7, 24, nullptr) == TVC_E_INVALID); // q not 16-byte aligned
        CHECK(tvc_sd_attention_ex(h, qkv, 56, qkv, 64, qkv, 72, ao + 2, 52, 2, 2, 5, 7, 24, nullptr) == TVC_E_INVALID); // out not 8-byte aligned
        CHECK(tvc_sd_attention_ex(h, qkv, 56, qkv, 64, qkv, 72, ao, 52, 2, 2, 5, 7, 20, nullptr) == TVC_E_INVALID);     // head_dim % 8
    }
    // ---- profiling bracket in mode 3, then back to bf16
    double ms[TVC_PROF_NCAT], work[TVC_PROF_NCAT], big[3]; int64_t launches[TVC_PROF_NCAT];
    OK(tvc_profile_begin(h)); OK(tvc_encode_image(h, pix, B, fi, 1, nullptr)); OK(tvc_profile_end(h, ms, work, launches, big));
    CHECK(launches[TVC_PROF_GEMM] > 0);
    OK(tvc_set_option(h, TVC_OPT_TOWER_PRECISION, 0));
    OK(tvc_encode_image(h, pix, B, fi, 1, nullptr)); OK(tvc_encode_text(h, tok, B * (N + 1), ft, 1, nullptr));
    OK(tvc_set_option(h, TVC_OPT_TOWER_PRECISION, 3));           // registered weights stay registered
    OK(tvc_encode_text(h, tok, B * (N + 1), ft, 1, nullptr));
    OK(tvc_set_option(h, TVC_OPT_TOWER_PRECISION, 0));
    tvc_destroy(h);
    for (void* p : keep) (void)hipFree(p);
    CHECK(hip_stub_blocks().empty());                               // every handle-owned device block was released
    printf("HOST_SAN_F16_OK\n");
    return 0;
}
