// Host-only sanitizer driver of the split-bf16 input gradient (tests/test_grad_split_host.py), built by
// tests/host_san_build.py under ASan / UBSan against tests/host_san's HIP stand-in (kernels are no-ops, "device" blocks are exactly
// sized host blocks, the GEMM stub checks every operand / output range against its block).  Walks TVC_OPT_GRAD_PRECISION's
// values, every refusal of the two gradient entry points in mode 2 (no fp32 weights, no split planes, backward before grad, the
// option changed between grad and backward, B above the chunk limit, an erf-GELU tower), valid forward / backward pairs of both
// modes at B = 1 and B = 5 (every workspace and plane range of the mode-2 path goes through the stub's checks), the free path
// of the transposed planes (tvc_set_weights_f32 again, tvc_destroy) and tvc_attention_split_backward's refusals.
#include "driver_common.hpp"

#include <vector>

static std::vector<void*> g_keep;
template <class T> static T* buf(size_t elems) { g_keep.push_back(dev(elems * sizeof(T))); return (T*)g_keep.back(); }

template <class L, class W>
static std::vector<L> layers(const tvc_tower_arch& a) {
    std::vector<L> v(a.layers);
    for (auto& l : v) {
        l.ln1_g = buf<float>(a.width); l.ln1_b = buf<float>(a.width); l.ln2_g = buf<float>(a.width); l.ln2_b = buf<float>(a.width);
        l.wqkv = buf<W>((size_t)3 * a.width * a.width); l.bqkv = buf<float>(3 * a.width);
        l.wo = buf<W>((size_t)a.width * a.width); l.bo = buf<float>(a.width);
        l.w1 = buf<W>((size_t)a.mlp * a.width); l.b1 = buf<float>(a.mlp);
        l.w2 = buf<W>((size_t)a.width * a.mlp); l.b2 = buf<float>(a.width);
    }
    return v;
}

int main() {
    tvc_handle* h = nullptr;
    // the toy geometry (ViT-T/16-test): 64 x 64 images, patch 16 -> 17 tokens, width 256, 2 layers, 4 heads, mlp 512, D = 128
    tvc_model_desc m{};
    m.image_size = 64; m.patch = 16; m.vocab = 49408; m.ctx = 77; m.embed_dim = 128;
    m.vision = {256, 2, 4, 512, TVC_ACT_QUICK_GELU};
    auto vl = layers<tvc_layer_weights, uint16_t>(m.vision);
    tvc_vision_weights vw{};
    vw.patch_w = buf<uint16_t>((size_t)256 * 768); vw.cls = buf<float>(256); vw.pos = buf<float>(17 * 256);
    vw.ln_pre_g = buf<float>(256); vw.ln_pre_b = buf<float>(256); vw.ln_post_g = buf<float>(256); vw.ln_post_b = buf<float>(256);
    vw.proj = buf<uint16_t>(128 * 256); vw.layers = vl.data();
    auto vl32 = layers<tvc_layer_weights_f32, float>(m.vision);
    tvc_vision_weights_f32 v32{};
    v32.patch_w = buf<float>((size_t)256 * 768); v32.cls = vw.cls; v32.pos = vw.pos; v32.ln_pre_g = vw.ln_pre_g; v32.ln_pre_b = vw.ln_pre_b;
    v32.ln_post_g = vw.ln_post_g; v32.ln_post_b = vw.ln_post_b; v32.proj = buf<float>(128 * 256); v32.layers = vl32.data();
    const int B = 5, S = 64, D = 128;
    float* pix = buf<float>((size_t)B * 3 * S * S);
    float *fi = buf<float>(B * D), *gout = buf<float>(B * D), *gpix = buf<float>((size_t)B * 3 * S * S);
    const char* FWD = "tvc_encode_image_grad";
    const char* BWD = "tvc_encode_image_backward";

    // ---- an erf-GELU tower has no backward pass, in either mode
    {
        tvc_model_desc g = m;
        g.vision.act = TVC_ACT_GELU;
        CHECK(tvc_create(&g, &vw, nullptr, &h) == TVC_OK && h);
        REFUSED(tvc_encode_image_grad(h, pix, B, fi, 1, nullptr), TVC_E_INVALID, "QuickGELU");
        OK(tvc_set_option(h, TVC_OPT_GRAD_PRECISION, 2));
        REFUSED(tvc_encode_image_grad(h, pix, B, fi, 1, nullptr), TVC_E_INVALID, "QuickGELU");
        tvc_destroy(h);
        h = nullptr;
    }

    CHECK(tvc_create(&m, &vw, nullptr, &h) == TVC_OK && h);
    CHECK(tvc_abi_version() == 4);
    // ---- the option's values
    REFUSED(tvc_set_option(h, TVC_OPT_GRAD_PRECISION, 1), TVC_E_INVALID, "TVC_OPT_GRAD_PRECISION");
    REFUSED(tvc_set_option(h, TVC_OPT_GRAD_PRECISION, 3), TVC_E_INVALID, "TVC_OPT_GRAD_PRECISION");
    REFUSED(tvc_set_option(h, TVC_OPT_GRAD_PRECISION, -1), TVC_E_INVALID, "TVC_OPT_GRAD_PRECISION");
    OK(tvc_set_option(h, TVC_OPT_GRAD_PRECISION, 0));
    // ---- backward before any grad
    REFUSED(tvc_encode_image_backward(h, gout, gpix, nullptr), TVC_E_STATE, FWD);
    // ---- mode 2 without fp32 weights: the option is recorded, the forward names what is missing, nothing is left to differentiate
    OK(tvc_set_option(h, TVC_OPT_GRAD_PRECISION, 2));
    REFUSED(tvc_encode_image_grad(h, pix, B, fi, 1, nullptr), TVC_E_STATE, "tvc_set_weights_f32");
    REFUSED(tvc_encode_image_backward(h, gout, gpix, nullptr), TVC_E_STATE, FWD);
    // ---- mode 2 with fp32 weights registered AFTER the option: no split planes yet
    OK(tvc_set_weights_f32(h, &v32, nullptr));
    REFUSED(tvc_encode_image_grad(h, pix, B, fi, 1, nullptr), TVC_E_STATE, "split planes");
    // ---- setting the option again builds them; B above the chunk limit is refused in mode 2 as in mode 0
    OK(tvc_set_option(h, TVC_OPT_GRAD_PRECISION, 2));
    OK(tvc_set_option(h, TVC_OPT_MAX_CHUNK_IMAGES, 2));
    REFUSED(tvc_encode_image_grad(h, pix, B, fi, 1, nullptr), TVC_E_INVALID, "TVC_OPT_MAX_CHUNK_IMAGES");
    OK(tvc_set_option(h, TVC_OPT_MAX_CHUNK_IMAGES, 512));
    REFUSED(tvc_encode_image_grad(h, nullptr, B, fi, 1, nullptr), TVC_E_INVALID, FWD);
    // ---- valid pairs: mode 2 (twice the backward: the transposed planes are built once), then mode 0, then mode 2 at B = 1
    const uint64_t ws0 = tvc_workspace_bytes(h);
    OK(tvc_encode_image_grad(h, pix, B, fi, 1, nullptr));
    REFUSED(tvc_encode_image_backward(h, nullptr, gpix, nullptr), TVC_E_INVALID, BWD);
    OK(tvc_encode_image_backward(h, gout, gpix, nullptr));
    OK(tvc_encode_image_backward(h, gout, gpix, nullptr));
    CHECK(tvc_workspace_bytes(h) > ws0);
    // the kept state of the toy tower at B = 5: 4 * (2 layers * 85 rows * (5 * 256 + 512) + 5 * (256 + 128)) bytes, inside the workspace
    CHECK(tvc_workspace_bytes(h) - ws0 >= (uint64_t)4 * (2 * 85 * (5 * 256 + 512) + 5 * (256 + 128)));
    // ---- the option changed between grad and backward: refused both ways, nothing mixed
    OK(tvc_set_option(h, TVC_OPT_GRAD_PRECISION, 0));
    REFUSED(tvc_encode_image_backward(h, gout, gpix, nullptr), TVC_E_STATE, "TVC_OPT_GRAD_PRECISION");
    OK(tvc_set_option(h, TVC_OPT_GRAD_PRECISION, 2));
    OK(tvc_encode_image_backward(h, gout, gpix, nullptr));       // back in the forward's mode: the kept state is still there
    OK(tvc_set_option(h, TVC_OPT_GRAD_PRECISION, 0));
    OK(tvc_encode_image_grad(h, pix, B, fi, 0, nullptr));
    OK(tvc_set_option(h, TVC_OPT_GRAD_PRECISION, 2));
    REFUSED(tvc_encode_image_backward(h, gout, gpix, nullptr), TVC_E_STATE, "TVC_OPT_GRAD_PRECISION");
    OK(tvc_set_option(h, TVC_OPT_GRAD_PRECISION, 0));
    OK(tvc_encode_image_backward(h, gout, gpix, nullptr));
    OK(tvc_set_option(h, TVC_OPT_GRAD_PRECISION, 2));
    OK(tvc_encode_image_grad(h, pix, 1, fi, 0, nullptr));
    OK(tvc_encode_image_backward(h, gout, gpix, nullptr));
    // ---- independent of the tower mode: bf16 towers between a mode-2 forward and its backward
    OK(tvc_encode_image_grad(h, pix, 3, fi, 1, nullptr));
    OK(tvc_encode_image(h, pix, B, fi, 1, nullptr));
    OK(tvc_set_option(h, TVC_OPT_TOWER_PRECISION, 2));
    OK(tvc_encode_image(h, pix, B, fi, 1, nullptr));
    OK(tvc_set_option(h, TVC_OPT_TOWER_PRECISION, 0));
    OK(tvc_encode_image_backward(h, gout, gpix, nullptr));
    // ---- the free path of the transposed planes: registering the fp32 weights again drops every plane (forward refused until
    // the option is set again), the next backward rebuilds the transposed ones
    OK(tvc_set_weights_f32(h, &v32, nullptr));
    REFUSED(tvc_encode_image_grad(h, pix, B, fi, 1, nullptr), TVC_E_STATE, "split planes");
    REFUSED(tvc_encode_image_backward(h, gout, gpix, nullptr), TVC_E_STATE, FWD);
    OK(tvc_set_option(h, TVC_OPT_GRAD_PRECISION, 2));
    OK(tvc_encode_image_grad(h, pix, B, fi, 1, nullptr));
    OK(tvc_encode_image_backward(h, gout, gpix, nullptr));

    // ---- tvc_attention_split_backward
    {
        const int n_seq = 2, T = 17, heads = 4, W = heads * 64;
        float *qkv = buf<float>((size_t)n_seq * T * 3 * W), *dao = buf<float>((size_t)n_seq * T * W), *dqkv = buf<float>((size_t)n_seq * T * 3 * W);
        const char* AB = "tvc_attention_split_backward";
        CHECK(tvc_attention_split_backward(nullptr, qkv, dao, dqkv, n_seq, T, heads, nullptr) == TVC_E_INVALID);
        REFUSED(tvc_attention_split_backward(h, nullptr, dao, dqkv, n_seq, T, heads, nullptr), TVC_E_INVALID, AB);
        REFUSED(tvc_attention_split_backward(h, qkv, nullptr, dqkv, n_seq, T, heads, nullptr), TVC_E_INVALID, AB);
        REFUSED(tvc_attention_split_backward(h, qkv, dao, nullptr, n_seq, T, heads, nullptr), TVC_E_INVALID, AB);
        REFUSED(tvc_attention_split_backward(h, qkv, dao, dqkv, -1, T, heads, nullptr), TVC_E_INVALID, AB);
        REFUSED(tvc_attention_split_backward(h, qkv, dao, dqkv, n_seq, 0, heads, nullptr), TVC_E_INVALID, AB);
        REFUSED(tvc_attention_split_backward(h, qkv, dao, dqkv, n_seq, 289, heads, nullptr), TVC_E_INVALID, AB);
        REFUSED(tvc_attention_split_backward(h, qkv, dao, dqkv, n_seq, T, 0, nullptr), TVC_E_INVALID, AB);
        REFUSED(tvc_attention_split_backward(h, qkv + 1, dao, dqkv, n_seq, T, heads, nullptr), TVC_E_INVALID, "aligned");
        OK(tvc_attention_split_backward(h, qkv, dao, dqkv, 0, T, heads, nullptr));
        OK(tvc_attention_split_backward(h, qkv, dao, dqkv, n_seq, T, heads, nullptr));
    }
    tvc_destroy(h);
    h = nullptr;
    for (void* p : g_keep) (void)hipFree(p);
    CHECK(hip_stub_blocks().empty());                               // every handle-owned device block was released
    printf("HOST_SAN_GRAD_SPLIT_OK\n");
    return 0;
}
