// Host-only sanitizer driver of the latent-diffusion model's fp16 mode (tests/test_sd_fp16_host.py): the same build as
// tests/host_san/driver.cpp -- tests/host_san_build.py's, the product's host sources under ASan / UBSan
// against tests/host_san's HIP stand-in, whose GEMM launcher checks every operand / output range -- walking
// TVC_OPT_SD_PRECISION: its values and refused transitions, then a toy model loaded in mode 1 through tvc_sd_unet,
// tvc_sd_vae_decode, a 2-step tvc_sd_generate with both stream settings, the block and attention entry points, and a
// leak-free tvc_destroy.  argv[1]: file of SD tensor names (one "name rows cols element_size" per line).
#include "driver_common.hpp"

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

int main(int argc, char** argv) {
    CHECK(argc >= 2);
    tvc_handle* h = nullptr;
    CHECK(tvc_create(nullptr, nullptr, nullptr, &h) == TVC_OK && h);          // a handle without towers: the SD model needs none
    std::vector<void*> keep;
    auto buf = [&](size_t elems, size_t es) { void* p = dev(elems * es); keep.push_back(p); return p; };
    // ---- the option before any model: 0 and 1 are accepted in any order, anything else is TVC_E_INVALID and changes nothing
    OK(tvc_set_option(h, TVC_OPT_SD_PRECISION, 0));
    CHECK(tvc_set_option(h, TVC_OPT_SD_PRECISION, 2) == TVC_E_INVALID && strstr(tvc_last_error(h), "TVC_OPT_SD_PRECISION"));
    CHECK(tvc_set_option(h, TVC_OPT_SD_PRECISION, -1) == TVC_E_INVALID);
    OK(tvc_set_option(h, TVC_OPT_SD_PRECISION, 1));
    OK(tvc_set_option(h, TVC_OPT_SD_PRECISION, 0));
    OK(tvc_set_option(h, TVC_OPT_SD_PRECISION, 1));
    // ---- the toy model of tests/host_san/driver.cpp, tensors sized exactly (GEMM weight rows padded to whole 256-row tiles, as
    // tvc_sd_load's contract asks): the stub's range check sees any slip in the fp16 mode's addressing
    std::vector<std::string> names; std::vector<tvc_named_tensor> nt;
    {
        std::ifstream f(argv[1]);
        std::string line;
        while (std::getline(f, line)) {
            std::istringstream ss(line);
            std::string name; long rows_ = 0, cols = 0; int es = 0;
            if (!(ss >> name >> rows_ >> cols >> es)) continue;
            names.push_back(name);
            const long rp = es == 2 ? (rows_ + 255) / 256 * 256 : rows_;
            nt.push_back({nullptr, buf((size_t)rp * cols, es)});
        }
        for (size_t i = 0; i < names.size(); ++i) nt[i].name = names[i].c_str();
    }
    CHECK(nt.size() > 100);
    tvc_sd_desc d{};
    d.in_channels = 4; d.out_channels = 4; d.n_blocks = 2; d.block_out_channels[0] = 64; d.block_out_channels[1] = 128;
    d.down_block_attn[0] = 1; d.down_block_attn[1] = 0; d.layers_per_block = 1; d.heads = 8; d.cross_attention_dim = 128;
    d.norm_groups = 32; d.norm_eps = 1e-5f; d.vae_n_blocks = 2; d.vae_block_out_channels[0] = 64; d.vae_block_out_channels[1] = 128;
    d.vae_layers_per_block = 1; d.latent_channels = 4; d.vae_scaling = 0.18215f; d.ctx = 77; d.beta_start = 0.00085f; d.beta_end = 0.012f;
    d.num_train_timesteps = 1000; d.steps_offset = 1;
    float* lat = (float*)buf((size_t)3 * 4 * 16 * 16, 4); float* ctx = (float*)buf((size_t)3 * 77 * 128, 4);
    float* eps = (float*)buf((size_t)3 * 4 * 16 * 16, 4); float* img = (float*)buf((size_t)3 * 3 * 32 * 32, 4);
    // a failed load leaves no model behind: the option still moves
    { tvc_sd_desc bad = d; bad.n_blocks = 5; CHECK(tvc_sd_load(h, &bad, nt.data(), (int)nt.size(), nullptr) == TVC_E_INVALID); }
    OK(tvc_set_option(h, TVC_OPT_SD_PRECISION, 0));
    OK(tvc_set_option(h, TVC_OPT_SD_PRECISION, 1));
    OK(tvc_sd_load(h, &d, nt.data(), (int)nt.size(), nullptr));
    // ---- a model is loaded: the same value is accepted, another is TVC_E_STATE, a bad one stays TVC_E_INVALID
    OK(tvc_set_option(h, TVC_OPT_SD_PRECISION, 1));
    CHECK(tvc_set_option(h, TVC_OPT_SD_PRECISION, 0) == TVC_E_STATE && strstr(tvc_last_error(h), "loaded"));
    CHECK(tvc_set_option(h, TVC_OPT_SD_PRECISION, 2) == TVC_E_INVALID);
    OK(tvc_set_option(h, TVC_OPT_SD_PRECISION, 1));
    // ---- the fp16 model through every evaluation entry point
    OK(tvc_sd_unet(h, lat, 2, 16, 16, 951.f, ctx, eps, nullptr));
    OK(tvc_sd_unet(h, lat, 3, 8, 24, 1.f, ctx, eps, nullptr));
    OK(tvc_sd_vae_decode(h, lat, 3, 16, 16, img, nullptr));
    OK(tvc_set_option(h, TVC_OPT_SD_STREAMS, 2));
    OK(tvc_sd_generate(h, ctx, ctx, lat, 3, 16, 16, 2, 7.5f, img, nullptr));
    OK(tvc_set_option(h, TVC_OPT_SD_STREAMS, 1));
    OK(tvc_sd_generate(h, ctx, ctx, lat, 3, 16, 16, 2, 7.5f, img, nullptr));
    OK(tvc_set_option(h, TVC_OPT_SD_STREAMS, 2));
    OK(tvc_set_option(h, TVC_OPT_SD_ARENA_BYTES, (int64_t)1 << 28));            // chunked generation
    OK(tvc_sd_generate(h, ctx, ctx, lat, 3, 16, 16, 2, 7.5f, nullptr, nullptr));
    float* x = (float*)buf((size_t)2 * 256 * 16 * 16, 4); float* y = (float*)buf((size_t)2 * 128 * 32 * 32, 4); float* temb = (float*)buf(2 * 256, 4);
    OK(tvc_sd_block(h, 0, "down_blocks.0.resnets.0.", x, 2, 64, 16, 16, temb, nullptr, 64, 0, y, nullptr));
    OK(tvc_sd_block(h, 0, "up_blocks.0.resnets.0.", x, 2, 256, 8, 8, temb, nullptr, 128, 0, y, nullptr));
    OK(tvc_sd_block(h, 1, "down_blocks.0.attentions.0.", x, 2, 64, 16, 16, nullptr, ctx, 64, 0, y, nullptr));
    OK(tvc_sd_block(h, 2, "decoder.mid_block.attentions.0.", x, 2, 128, 8, 8, nullptr, nullptr, 128, 1, y, nullptr));
    OK(tvc_sd_block(h, 3, "down_blocks.0.resnets.0.conv1.", x, 2, 64, 16, 16, nullptr, nullptr, 64, 0, y, nullptr));
    OK(tvc_sd_block(h, 4, "down_blocks.0.downsamplers.0.conv.", x, 2, 64, 16, 16, nullptr, nullptr, 64, 0, y, nullptr));
    OK(tvc_sd_block(h, 5, "up_blocks.0.upsamplers.0.conv.", x, 2, 128, 8, 8, nullptr, nullptr, 128, 0, y, nullptr));
    // streaming attention reads its operands in the handle's format: same argument rules in both
    uint16_t* qkv = (uint16_t*)buf((size_t)2 * 7 * 72, 2); uint16_t* ao = (uint16_t*)buf((size_t)2 * 7 * 52, 2);
    OK(tvc_sd_attention(h, qkv, qkv, qkv, ao, 2, 2, 7, 7, 24, nullptr));
    OK(tvc_sd_attention_ex(h, qkv, 56, qkv, 64, qkv, 72, ao, 52, 2, 2, 5, 7, 24, nullptr));
    CHECK(tvc_sd_attention_ex(h, qkv, 52, qkv, 64, qkv, 72, ao, 52, 2, 2, 5, 7, 24, nullptr) == TVC_E_INVALID);
    // ---- reloading in the same format is a plain reload; the tower option is independent of this one
    OK(tvc_sd_load(h, &d, nt.data(), (int)nt.size(), nullptr));
    CHECK(tvc_set_option(h, TVC_OPT_SD_PRECISION, 0) == TVC_E_STATE);
    OK(tvc_set_option(h, TVC_OPT_TOWER_PRECISION, 0));
    OK(tvc_sd_unet(h, lat, 2, 16, 16, 951.f, ctx, eps, nullptr));
    tvc_destroy(h);
    for (void* p : keep) (void)hipFree(p);
    CHECK(hip_stub_blocks().empty());                               // every handle-owned device block was released
    printf("HOST_SAN_SD_F16_OK\n");
    return 0;
}
