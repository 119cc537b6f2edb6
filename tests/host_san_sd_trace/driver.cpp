// Host-only trace driver of the latent-diffusion host code (tests/test_sd_trace_host.py): the same build as
// tests/host_san_sd_f16/driver.cpp -- tests/host_san_build.py's, against tests/host_san's HIP stand-in -- with the
// stubs of gen_stubs.py --trace, so that every launch, its arguments, its stream and its arena offsets, every allocation and
// every copy of each SD entry point land in the file HIP_STUB_TRACE names, one "# ..." marker line before each call.  The
// test compares that file with the one recorded before tvc_sd.cpp was refactored.  Both 16-bit formats, the toy geometry of
// the other host drivers.  argv[1]: file of SD tensor names (one "name rows cols element_size" per line).
#define DRIVER_BEFORE_OK(text) hip_trace_line("# " text)        // one marker line in the trace before each call
#include "driver_common.hpp"

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

static int run(const char* names_file, int precision) {
    tvc_handle* h = nullptr;
    CHECK(tvc_create(nullptr, nullptr, nullptr, &h) == TVC_OK && h);          // a handle without towers: the SD model needs none
    std::vector<void*> keep;
    auto buf = [&](size_t elems, size_t es) { void* p = dev(elems * es); keep.push_back(p); return p; };
    OK(tvc_set_option(h, TVC_OPT_SD_PRECISION, precision));
    std::vector<std::string> names; std::vector<tvc_named_tensor> nt;
    {
        std::ifstream f(names_file);
        std::string line;
        while (std::getline(f, line)) {
            std::istringstream ss(line);
            std::string name; long rows_ = 0, cols = 0; int es = 0;
            if (!(ss >> name >> rows_ >> cols >> es)) continue;
            names.push_back(name);
            const long rp = es == 2 ? (rows_ + 255) / 256 * 256 : rows_;      // tvc_sd_load's contract: whole 256-row tiles
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
    float* unc = (float*)buf((size_t)3 * 77 * 128, 4);
    float* eps = (float*)buf((size_t)3 * 4 * 16 * 16, 4); float* img = (float*)buf((size_t)3 * 3 * 32 * 32, 4);
    OK(tvc_sd_load(h, &d, nt.data(), (int)nt.size(), nullptr));
    OK(tvc_sd_unet(h, lat, 2, 16, 16, 951.f, ctx, eps, nullptr));
    OK(tvc_sd_unet(h, lat, 3, 8, 24, 1.f, ctx, eps, nullptr));
    OK(tvc_sd_vae_decode(h, lat, 3, 16, 16, img, nullptr));
    // 2, 3 and 6 steps: the history ring reaches all four slots; both stream settings, with and without the decode
    OK(tvc_set_option(h, TVC_OPT_SD_STREAMS, 2));
    OK(tvc_sd_generate(h, ctx, unc, lat, 3, 16, 16, 2, 7.5f, img, nullptr));
    OK(tvc_sd_generate(h, ctx, unc, lat, 2, 16, 16, 3, 7.5f, nullptr, nullptr));
    OK(tvc_sd_generate(h, ctx, unc, lat, 3, 16, 16, 6, 5.0f, nullptr, nullptr));
    OK(tvc_set_option(h, TVC_OPT_SD_STREAMS, 1));
    OK(tvc_sd_generate(h, ctx, unc, lat, 3, 16, 16, 2, 7.5f, nullptr, nullptr));
    OK(tvc_sd_generate(h, ctx, unc, lat, 1, 16, 16, 3, 7.5f, img, nullptr));
    OK(tvc_sd_generate(h, ctx, unc, lat, 2, 8, 24, 6, 7.5f, nullptr, nullptr));
    OK(tvc_set_option(h, TVC_OPT_SD_STREAMS, 2));
    // chunked generation: at 96 x 96 latents one (unconditional | conditional) pair needs about 120 MB, so the smallest arena
    // budget holds two and 3 images run as chunks of 2 + 1 (two sampling loops: two pairs of text-state copies in the trace)
    OK(tvc_set_option(h, TVC_OPT_SD_ARENA_BYTES, (int64_t)1 << 28));
    float* lat96 = (float*)buf((size_t)3 * 4 * 96 * 96, 4);
    OK(tvc_sd_generate(h, ctx, unc, lat96, 3, 96, 96, 2, 7.5f, nullptr, nullptr));
    OK(tvc_set_option(h, TVC_OPT_SD_ARENA_BYTES, (int64_t)48 << 30));
    float* x = (float*)buf((size_t)2 * 256 * 16 * 16, 4); float* y = (float*)buf((size_t)2 * 128 * 32 * 32, 4); float* temb = (float*)buf(2 * 256, 4);
    OK(tvc_sd_block(h, 0, "down_blocks.0.resnets.0.", x, 2, 64, 16, 16, temb, nullptr, 64, 0, y, nullptr));
    OK(tvc_sd_block(h, 0, "up_blocks.0.resnets.0.", x, 2, 256, 8, 8, temb, nullptr, 128, 0, y, nullptr));
    OK(tvc_sd_block(h, 1, "down_blocks.0.attentions.0.", x, 2, 64, 16, 16, nullptr, ctx, 64, 0, y, nullptr));
    OK(tvc_sd_block(h, 2, "decoder.mid_block.attentions.0.", x, 2, 128, 8, 8, nullptr, nullptr, 128, 1, y, nullptr));
    OK(tvc_sd_block(h, 3, "down_blocks.0.resnets.0.conv1.", x, 2, 64, 16, 16, nullptr, nullptr, 64, 0, y, nullptr));
    OK(tvc_sd_block(h, 4, "down_blocks.0.downsamplers.0.conv.", x, 2, 64, 16, 16, nullptr, nullptr, 64, 0, y, nullptr));
    OK(tvc_sd_block(h, 5, "up_blocks.0.upsamplers.0.conv.", x, 2, 128, 8, 8, nullptr, nullptr, 128, 0, y, nullptr));
    // which launches the profiler sees, with what category and work
    {
        double ms[TVC_PROF_NCAT], work[TVC_PROF_NCAT], big[3];
        int64_t launches[TVC_PROF_NCAT];
        OK(tvc_profile_begin(h));
        OK(tvc_sd_unet(h, lat, 2, 16, 16, 500.f, ctx, eps, nullptr));
        OK(tvc_profile_end(h, ms, work, launches, big));
        for (int c = 0; c < TVC_PROF_NCAT; ++c) hip_trace_line("profile", c, ms[c], work[c], launches[c]);
        hip_trace_line("profile big_gemm", big[0], big[1], big[2]);
    }
    // v-prediction: the same tensors under another scheduler rule
    d.prediction_type = 1;
    OK(tvc_sd_load(h, &d, nt.data(), (int)nt.size(), nullptr));
    OK(tvc_sd_generate(h, ctx, unc, lat, 2, 16, 16, 3, 7.5f, nullptr, nullptr));
    hip_trace_line("# tvc_destroy");
    tvc_destroy(h);
    for (void* p : keep) (void)hipFree(p);
    CHECK(hip_stub_blocks().empty());                               // every handle-owned device block was released
    return 0;
}

int main(int argc, char** argv) {
    CHECK(argc >= 2);
    CHECK(hip_trace());                                             // HIP_STUB_TRACE must name a writable file
    for (int precision = 0; precision < 2; ++precision) {
        hip_trace_line(precision ? "## TVC_OPT_SD_PRECISION 1" : "## TVC_OPT_SD_PRECISION 0");
        if (run(argv[1], precision)) return 1;
    }
    fclose(hip_trace());
    printf("HOST_SAN_SD_TRACE_OK\n");
    return 0;
}
