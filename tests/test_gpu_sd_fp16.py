"""GPU: the latent-diffusion model's fp16 mode (TVC_OPT_SD_PRECISION = 1; ``SDKernels(..., precision="fp16")``) -- IEEE
fp16 weights and activations, products on v_mfma_f32_16x16x32_f16 -- against ``oracle/sd_oracle.py`` (PyTorch fp32 on the
CPU, on the same fp32 weights), side by side with the bf16 mode on a second engine fed the same inputs.

Every parity case asserts three things:
  * finite: the fp16 output is finite;
  * ordering: fp16 error <= bf16 error, measured here on the same inputs (unit roundoff 2^-11 against 2^-8: a case where
    this fails is a bug to find, not a bound to loosen);
  * an absolute bound on the fp16 error at 2x the value measured on the MI355X (written next to each assertion, printed as
    ``[measured] ...`` with ``pytest -s``, tabulated in EXPERIMENTS.md, "SD: an fp16 mode").

Geometry: the smallest that reaches every instantiation -- "mid" (widths 320 / 640: not multiples of 256, padded weight
rows, head dims 40 and 80, the 9-plane, stride-2 and upsample convolutions) and the v-prediction "toy" arch of
test_gpu_sd.py (per-level heads, head dim 64, linear projections).  **Parity unpinned against the reference**, as
test_gpu_sd.py's header says of the oracle.
"""
import importlib

import pytest
import torch

from oracle import sd_oracle

pytestmark = pytest.mark.gpu


def rel(got: torch.Tensor, ref: torch.Tensor):
    """(relative L2 error, max |d| / std(ref))."""
    d = got.double().cpu() - ref.double()
    return (d.norm() / ref.double().norm()).item(), (d.abs().max() / ref.double().std()).item()


def parity(name, got16, gotbf, ref, bound):
    """The three-part rule of the module docstring on the relative L2 error; returns (fp16, bf16) errors."""
    e16, ebf = rel(got16, ref), rel(gotbf, ref)
    print(f"[measured] {name}: fp16 rel L2 {e16[0]:.2e} max|d|/std {e16[1]:.2e}  |  bf16 rel L2 {ebf[0]:.2e} max|d|/std {ebf[1]:.2e}"
          f"  (fp16 / bf16 = {e16[0] / ebf[0]:.3f})")
    assert torch.isfinite(got16).all(), name
    assert e16[0] <= ebf[0], (name, e16, ebf)
    assert e16[0] < bound, (name, e16[0], bound)
    return e16[0], ebf[0]


class Pair:
    """One model on two engines: ``.bf`` (bf16) and ``.fp`` (fp16) SDKernels of the same fp32 weights."""

    def __init__(self, pkg, arch, seed):
        self.arch = arch
        self.uw, self.vw = pkg.make_sd_weights(arch, seed=seed)
        self.engines = [pkg.TVCEngine(), pkg.TVCEngine()]
        self.bf = pkg.SDKernels(self.engines[0], arch, self.uw, self.vw)
        self.fp = pkg.SDKernels(self.engines[1], arch, self.uw, self.vw, precision="fp16")

    def close(self):
        for e in self.engines:
            e.close()


def mid_arch(pkg):
    return pkg.SDArch(block_out_channels=(320, 640), down_block_attn=(True, True), layers_per_block=1, heads=8,
                      cross_attention_dim=768, vae_block_out_channels=(128, 256), vae_layers_per_block=1, sample_size=16)


def toy_arch(pkg):
    return pkg.SDArch(block_out_channels=(64, 128), down_block_attn=(True, True), layers_per_block=1, heads=8, heads_per_block=(1, 2),
                      linear_projection=True, prediction_type="v_prediction", cross_attention_dim=128,
                      vae_block_out_channels=(64, 128), vae_layers_per_block=1, sample_size=16)


@pytest.fixture(scope="module")
def mid(pkg):
    p = Pair(pkg, mid_arch(pkg), 0)
    assert p.bf.precision == "bf16" and p.fp.precision == "fp16"
    assert p.fp.tensors["conv_in.weight"].dtype == torch.float16 and p.bf.tensors["conv_in.weight"].dtype == torch.bfloat16
    yield p
    p.close()


@pytest.fixture(scope="module")
def toy(pkg):
    p = Pair(pkg, toy_arch(pkg), 4)
    yield p
    p.close()


# ---- 1. streaming attention ----------------------------------------------------------------------------------------
def attention_fp64(q, k, v, n, heads, dh, Tq, Tk):
    sp = lambda t, T: t.double().view(n, T, heads, dh).transpose(1, 2)
    s = sp(q, Tq) @ sp(k, Tk).transpose(-1, -2) * dh ** -0.5
    return (s.softmax(-1) @ sp(v, Tk)).transpose(1, 2).reshape(n * Tq, heads * dh)


@pytest.mark.parametrize("n,heads,dh,Tq,Tk", [(3, 8, 160, 64, 64), (2, 8, 160, 64, 77), (1, 2, 64, 100, 50), (1, 3, 8, 70, 130),
                                             (2, 8, 40, 1024, 77), (2, 8, 80, 1024, 1024),
                                             # the eight-wave, two-workgroups-per-CU form: ragged query blocks, a ragged last key tile
                                             (22, 8, 40, 700, 700), (24, 8, 32, 520, 130)])
def test_streaming_attention_fp16_vs_fp64(pkg, mid, n, heads, dh, Tq, Tk):
    g = torch.Generator().manual_seed(Tq + dh)
    C = heads * dh
    q32, k32, v32 = (torch.randn((n * T, C), generator=g) for T in (Tq, Tk, Tk))
    err = {}
    for name, kern, dt in (("fp16", mid.fp, torch.float16), ("bf16", mid.bf, torch.bfloat16)):
        q, k, v = (t.to(dt) for t in (q32, k32, v32))                 # each mode's reference: from its own rounded inputs
        out = kern.attention(q, k, v, n, heads)
        assert out.dtype == dt
        err[name] = (out, attention_fp64(q, k, v, n, heads, dh, Tq, Tk))
    e16, ebf = rel(*err["fp16"]), rel(*err["bf16"])
    print(f"[measured] streaming attention n={n} heads={heads} dh={dh} Tq={Tq} Tk={Tk}: fp16 rel L2 {e16[0]:.2e} max|d|/std {e16[1]:.2e}"
          f"  |  bf16 rel L2 {ebf[0]:.2e} max|d|/std {ebf[1]:.2e}")
    assert torch.isfinite(err["fp16"][0]).all()
    assert e16[0] <= ebf[0] and e16[1] <= ebf[1]
    assert e16[0] < 6e-4 and e16[1] < 1.3e-2        # measured 2.6e-4 .. 2.9e-4 / 1.6e-3 .. 6.3e-3 (bf16 here: 2.1e-3 .. 2.3e-3 / 1.2e-2 .. 4.7e-2)


def test_streaming_attention_fp16_strided_fused_projection_buffers(pkg, mid):
    """``ld = (ldq, ldk, ldv, ldo)``: q in the first C columns of a fused [rows, 3C] buffer, k in a fused [rows, 2C] one, v and
    out in rows wider than C; the columns beyond heads * dh of ``out`` keep what they held."""
    n, heads, dh, Tq, Tk = 2, 8, 40, 150, 77
    C = heads * dh
    g = torch.Generator().manual_seed(7)
    qb, kb, vb = torch.randn((n * Tq, 3 * C), generator=g), torch.randn((n * Tk, 2 * C), generator=g), torch.randn((n * Tk, C + 8), generator=g)
    ld = (3 * C, 2 * C, C + 8, C + 4)
    res = {}
    for name, kern, dt in (("fp16", mid.fp, torch.float16), ("bf16", mid.bf, torch.bfloat16)):
        q, k, v = (t.to(dt) for t in (qb, kb, vb))
        out = torch.full((n * Tq, C + 4), 3.0, dtype=dt, device="cuda")
        got = kern.attention(q, k, v, n, heads, ld=ld, dh=dh, out=out)
        assert got is out and (out[:, C:] == 3.0).all()
        ref = attention_fp64(q[:, :C], k[:, :C], v[:, :C], n, heads, dh, Tq, Tk)
        res[name] = rel(out[:, :C].float(), ref)
        assert torch.equal(out[:, :C], kern.attention(q[:, :C], k[:, :C], v[:, :C], n, heads))          # = the dense call, bit for bit
    print(f"[measured] strided streaming attention: fp16 rel L2 {res['fp16'][0]:.2e}  |  bf16 rel L2 {res['bf16'][0]:.2e}")
    assert res["fp16"][0] <= res["bf16"][0] and res["fp16"][0] < 6e-4          # measured 2.65e-4 (bf16 2.14e-3)


# ---- 2. blocks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,prefix,cin,cout,hw", [(3, "down_blocks.0.resnets.0.conv1.", 320, 320, 16),
                                                     (4, "down_blocks.0.downsamplers.0.conv.", 320, 320, 16),
                                                     (5, "up_blocks.0.upsamplers.0.conv.", 640, 640, 8)])
def test_conv_kinds_fp16_vs_oracle(pkg, mid, kind, prefix, cin, cout, hw):
    x = torch.randn((2, cin, hw, hw), generator=torch.Generator().manual_seed(kind))
    F = torch.nn.functional
    xs = F.interpolate(x, scale_factor=2.0, mode="nearest") if kind == 5 else x
    ref = F.conv2d(xs, mid.uw[prefix + "weight"], mid.uw[prefix + "bias"], stride=2 if kind == 4 else 1, padding=1)
    got16, gotbf = mid.fp.block(kind, prefix, x, cout), mid.bf.block(kind, prefix, x, cout)
    assert got16.shape == ref.shape
    parity(f"conv kind {kind} {prefix}", got16, gotbf, ref, 7.2e-4)          # measured 3.6e-4 (bf16 2.9e-3; fp32 inputs, so both include the input rounding)


@pytest.mark.parametrize("prefix,cin,cout,hw,vae", [("down_blocks.0.resnets.0.", 320, 320, 16, False),          # no shortcut
                                                    ("up_blocks.1.resnets.0.", 960, 320, 16, False),            # 1x1 shortcut, concatenated input
                                                    ("decoder.up_blocks.1.resnets.0.", 256, 128, 16, True)])    # the VAE's eps (1e-6), no time embedding
def test_resnet_block_fp16_vs_oracle(pkg, mid, prefix, cin, cout, hw, vae):
    g = torch.Generator().manual_seed(cin)
    x = torch.randn((2, cin, hw, hw), generator=g)
    temb = None if vae else torch.randn((2, mid.arch.time_dim), generator=g)
    with torch.no_grad():
        ref = sd_oracle.resnet(mid.vw if vae else mid.uw, prefix, x, temb, mid.arch.norm_groups, 1e-6 if vae else mid.arch.norm_eps)
    parity(f"resnet {prefix}", mid.fp.block(0, prefix, x, cout, temb=temb, vae=vae), mid.bf.block(0, prefix, x, cout, temb=temb, vae=vae),
           ref, 1e-3)                                                      # measured 3.6e-4 .. 4.9e-4 (bf16 2.9e-3 .. 3.9e-3)


@pytest.mark.parametrize("prefix,c,hw", [("down_blocks.0.attentions.0.", 320, 16), ("mid_block.attentions.0.", 640, 8)])
def test_transformer_block_fp16_vs_oracle(pkg, mid, prefix, c, hw):
    g = torch.Generator().manual_seed(c)
    x = torch.randn((2, c, hw, hw), generator=g)
    ctx = torch.randn((2, mid.arch.ctx, mid.arch.cross_attention_dim), generator=g)
    with torch.no_grad():
        ref = sd_oracle.transformer(mid.uw, prefix, x, ctx, mid.arch.heads, mid.arch.norm_groups)
    parity(f"transformer {prefix} (head_dim {c // mid.arch.heads})", mid.fp.block(1, prefix, x, c, ctx=ctx), mid.bf.block(1, prefix, x, c, ctx=ctx),
           ref, 8.6e-4)                                                    # measured 4.2e-4 .. 4.3e-4 (bf16 3.4e-3)


def test_linear_projection_transformer_fp16_vs_oracle(pkg, toy):
    """The toy arch's Transformer2DModel: linear proj_in / proj_out, 2 heads of 64 at the 128-wide level."""
    prefix, c, hw, heads = "down_blocks.1.attentions.0.", 128, 8, 2
    g = torch.Generator().manual_seed(c)
    x = torch.randn((2, c, hw, hw), generator=g)
    ctx = torch.randn((2, toy.arch.ctx, toy.arch.cross_attention_dim), generator=g)
    with torch.no_grad():
        ref = sd_oracle.transformer(toy.uw, prefix, x, ctx, heads, toy.arch.norm_groups)
    parity("transformer (linear projections, 2 heads of 64)", toy.fp.block(1, prefix, x, c, ctx=ctx), toy.bf.block(1, prefix, x, c, ctx=ctx),
           ref, 8.6e-4)                                                    # measured 4.3e-4 (bf16 3.4e-3)


def test_vae_attention_block_fp16_vs_oracle(pkg, mid):
    x = torch.randn((2, 256, 16, 16), generator=torch.Generator().manual_seed(9))
    p = "decoder.mid_block.attentions.0."
    with torch.no_grad():
        ref = sd_oracle.vae_attention(mid.vw, p, x, mid.arch.norm_groups)
    parity("VAE attention block", mid.fp.block(2, p, x, 256, vae=True), mid.bf.block(2, p, x, 256, vae=True), ref, 6e-4)      # measured 2.95e-4 (bf16 2.4e-3)


# ---- 3. UNet forward, VAE decode -----------------------------------------------------------------------------------
def test_unet_forward_fp16_vs_oracle(pkg, mid):
    g = torch.Generator().manual_seed(4)
    lat = torch.randn((2, 4, 16, 16), generator=g)
    ctx = torch.randn((2, mid.arch.ctx, mid.arch.cross_attention_dim), generator=g)
    outs = {}
    for t in (951, 1):
        with torch.no_grad():
            ref = sd_oracle.unet_forward(mid.uw, mid.arch, lat, t, ctx)
        outs[t] = mid.fp.unet(lat, float(t), ctx)
        parity(f"UNet forward (mid arch, 16 x 16 latents, t = {t})", outs[t], mid.bf.unet(lat, float(t), ctx), ref, 3e-3)      # measured 1.46e-3 / 1.45e-3 (bf16 1.12e-2 / 1.15e-2)
    assert (outs[1] - outs[951]).abs().max().item() > 1e-3          # another timestep goes through the time embedding differently


def test_vae_decode_fp16_vs_oracle(pkg, mid):
    lat = torch.randn((2, 4, 16, 16), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        ref = (sd_oracle.vae_decode(mid.vw, mid.arch, lat / mid.arch.vae_scaling) / 2 + 0.5).clamp(0, 1)
    got16, gotbf = mid.fp.vae_decode(lat), mid.bf.vae_decode(lat)
    d16, dbf = (got16.cpu() - ref).abs(), (gotbf.cpu() - ref).abs()
    print(f"[measured] VAE decode (16 x 16 latents -> 32 x 32 pixels in [0, 1]): fp16 max |d| {d16.max().item():.2e} mean |d| {d16.mean().item():.2e}"
          f"  |  bf16 max |d| {dbf.max().item():.2e} mean |d| {dbf.mean().item():.2e}")
    assert got16.shape == (2, 3, 32, 32) and torch.isfinite(got16).all()
    assert d16.max().item() <= dbf.max().item() and d16.mean().item() <= dbf.mean().item()
    assert d16.max().item() < 1.8e-3 and d16.mean().item() < 3.1e-4      # measured 8.8e-4 / 1.5e-4 (bf16 7.5e-3 / 1.2e-3)


# ---- 4. / 5. sampling loops ----------------------------------------------------------------------------------------
def test_sampling_loop_fp16_vs_oracle(pkg, mid):
    """PNDM (PLMS) + classifier-free guidance on the mid arch: 5 scheduler steps (6 UNet evaluations on 2n samples)."""
    g = torch.Generator().manual_seed(6)
    n, steps, guidance = 2, 5, 7.5
    cond, uncond = (torch.randn((n, mid.arch.ctx, mid.arch.cross_attention_dim), generator=g) for _ in range(2))
    lat0 = torch.randn((n, 4, 16, 16), generator=g)
    lat16, img16 = mid.fp.generate(cond, uncond, lat0, steps, guidance, decode=True)
    latbf, _ = mid.bf.generate(cond, uncond, lat0, steps, guidance, decode=False)
    with torch.no_grad():
        ref = sd_oracle.generate(mid.uw, mid.vw, mid.arch, cond, uncond, lat0, steps, guidance, return_latents=True)
    parity(f"sampling loop (mid arch, {steps} PLMS steps, guidance {guidance}), final latents", lat16, latbf, ref, 3.6e-3)      # measured 1.78e-3 (bf16 1.40e-2)
    assert img16.shape == (n, 3, 32, 32) and torch.isfinite(img16).all() and float(img16.min()) >= 0.0 and float(img16.max()) <= 1.0


def test_v_prediction_sampling_loop_fp16_vs_oracle(pkg, toy):
    """The loop whose bf16 drift (4.1e-2 after 6 steps) could not be told from amplification without a higher-precision
    mode: both modes' rel-L2 from the oracle side by side.  The v update amplifies whatever rounding noise the UNet adds; with
    8x less of it, the drift shrinks by about as much if it is amplified kernel noise, and stays if it is anything else."""
    g = torch.Generator().manual_seed(26)
    n, steps, guidance = 2, 6, 6.0
    cond, uncond = (torch.randn((n, toy.arch.ctx, toy.arch.cross_attention_dim), generator=g) for _ in range(2))
    lat0 = torch.randn((n, 4, 16, 16), generator=g)
    lat16, img16 = toy.fp.generate(cond, uncond, lat0, steps, guidance, decode=True)
    latbf, _ = toy.bf.generate(cond, uncond, lat0, steps, guidance, decode=False)
    with torch.no_grad():
        ref = sd_oracle.generate(toy.uw, toy.vw, toy.arch, cond, uncond, lat0, steps, guidance, return_latents=True)
    parity(f"v-prediction sampling loop (toy arch, {steps} PLMS steps, guidance {guidance}), final latents", lat16, latbf, ref, 1.04e-2)      # measured 5.17e-3 (bf16 4.08e-2: ratio 0.127, the 2^-3 of the two roundoffs)
    assert img16.shape == (n, 3, 32, 32) and torch.isfinite(img16).all()


# ---- 6. bit-identity -----------------------------------------------------------------------------------------------
def test_fp16_generation_is_bit_identical_across_batching_chunking_and_streams(pkg, mid):
    """The bf16 mode's guarantees hold in fp16: an image does not depend on its batch mates, on the arena chunking
    (TVC_OPT_SD_ARENA_BYTES) or on the stream count (TVC_OPT_SD_STREAMS)."""
    k = mid.fp
    g = torch.Generator().manual_seed(19)
    n, steps = 3, 3
    cond, uncond = (torch.randn((n, mid.arch.ctx, mid.arch.cross_attention_dim), generator=g) for _ in range(2))
    lat0 = torch.randn((n, 4, 16, 16), generator=g)
    lat, img = k.generate(cond, uncond, lat0, steps, 7.5, decode=True)
    assert torch.isfinite(lat).all() and torch.isfinite(img).all()
    for i in range(n):
        l1, i1 = k.generate(cond[i:i + 1], uncond[i:i + 1], lat0[i:i + 1], steps, 7.5, decode=True)
        assert torch.equal(l1, lat[i:i + 1]) and torch.equal(i1, img[i:i + 1]), i
    # the one-image arena of the dry run: a budget of 256 MiB (the option's minimum) must split the batch for the check to mean anything
    k.engine.set_option(pkg._lib.TVC_OPT_SD_ARENA_BYTES, 1 << 28)
    try:
        lc, ic = k.generate(cond, uncond, lat0, steps, 7.5, decode=True)
    finally:
        k.engine.set_option(pkg._lib.TVC_OPT_SD_ARENA_BYTES, 48 << 30)
    assert torch.equal(lc, lat) and torch.equal(ic, img)
    k.engine.set_option(pkg._lib.TVC_OPT_SD_STREAMS, 1)
    try:
        ls, is_ = k.generate(cond, uncond, lat0, steps, 7.5, decode=True)
    finally:
        k.engine.set_option(pkg._lib.TVC_OPT_SD_STREAMS, 2)
    assert torch.equal(ls, lat) and torch.equal(is_, img)


# ---- 7. option semantics -------------------------------------------------------------------------------------------
def test_sd_precision_option_semantics(pkg, toy):
    L = pkg._lib
    eng = pkg.TVCEngine()
    try:
        assert eng.sd_precision == "bf16"
        # default = bf16 behaviour: a bf16 attention call on a fresh handle equals the bf16 model's engine, bit for bit
        g = torch.Generator().manual_seed(1)
        q, k, v = (torch.randn((2 * 70, 64), generator=g).to(torch.bfloat16) for _ in range(3))
        sdm = importlib.import_module(pkg.__name__ + ".sd_model")
        assert torch.equal(sdm.streaming_attention(eng, q, k, v, 2, 2), toy.bf.attention(q, k, v, 2, 2))
        with pytest.raises(pkg.TVCError) as e:
            eng.set_option(L.TVC_OPT_SD_PRECISION, 2)
        assert e.value.code == L.TVC_E_INVALID and eng.sd_precision == "bf16"
        eng.set_option(L.TVC_OPT_SD_PRECISION, 1)
        eng.set_option(L.TVC_OPT_SD_PRECISION, 0)                 # no model loaded: moves freely
        kern = pkg.SDKernels(eng, toy.arch, toy.uw, None, precision="fp16")
        assert kern.precision == "fp16" and eng.sd_precision == "fp16"
        with pytest.raises(pkg.TVCError) as e:
            eng.set_option(L.TVC_OPT_SD_PRECISION, 0)             # the registered tensors are one format
        assert e.value.code == L.TVC_E_STATE and eng.sd_precision == "fp16"
        eng.set_option(L.TVC_OPT_SD_PRECISION, 1)                 # the value it has
        with pytest.raises(ValueError):
            pkg.SDKernels(eng, toy.arch, toy.uw, None, precision="int8")
        # a bf16 tensor on an fp16 handle: refused before any launch (and the other way round)
        with pytest.raises(ValueError):
            kern.attention(q, k, v, 2, 2)
        with pytest.raises(ValueError):
            toy.bf.attention(q.to(torch.float16), k.to(torch.float16), v.to(torch.float16), 2, 2)
        out = kern.attention(q.to(torch.float16), k.to(torch.float16), v.to(torch.float16), 2, 2)
        assert out.dtype == torch.float16 and torch.isfinite(out).all()
    finally:
        eng.close()


# ---- 8. range ------------------------------------------------------------------------------------------------------
def test_fp16_range_is_never_clamped(pkg, mid):
    """An input of 7e4 is beyond fp16's 65504: it becomes +inf on the way in and the convolution's output goes non-finite;
    the bf16 handle (range 3e38) stays finite."""
    prefix = "down_blocks.0.resnets.0.conv1."
    x = torch.randn((1, 320, 16, 16), generator=torch.Generator().manual_seed(2))
    x[0, 5, 7, 7] = 7e4
    assert not torch.isfinite(mid.fp.block(3, prefix, x, 320)).all()
    assert torch.isfinite(mid.bf.block(3, prefix, x, 320)).all()
    x[0, 5, 7, 7] = 6e4                                           # inside the range: finite again
    assert torch.isfinite(mid.fp.block(3, prefix, x, 320)).all()


# ---- 9. full pipeline ----------------------------------------------------------------------------------------------
def test_stable_diffusion_model_fp16_full_pipeline_vs_oracle(pkg):
    """prompts -> tokens -> CLIP text states -> PNDM loop -> VAE -> pixels with ``SDModelConfig(precision="fp16")``, as
    test_gpu_sd.py's toy-geometry pipeline test does in bf16, against clip_oracle.text_hidden + sd_oracle.generate."""
    from oracle import clip_oracle
    arch = toy_arch(pkg)
    carch = pkg.get_arch("ViT-T/16-test")                     # text width 128 = the toy UNet's cross_attention_dim
    cw = pkg.synth.make_clip_weights(carch, seed=0)
    prompts, seeds, steps, guidance = ["a red cube on a table", "two birds"], [11, 12], 6, 5.0
    imgs = {}
    for precision in ("fp16", "bf16"):                        # one CLIP engine each: a handle holds one model, in one format
        clip = pkg.CLIPModel(pkg.CLIPConfig(model_name=carch.name), weights=cw)
        try:
            sd = pkg.StableDiffusionModel(pkg.SDModelConfig(precision=precision, random_init=True), clip_model=clip, arch=arch)
            assert sd.kernels.precision == precision and sd.text_engine is clip.engine
            imgs[precision] = sd.generate_batch(prompts, seeds, steps, guidance, 32, 32, negative_prompts=["blurry", "blurry"]).cpu()
            tok, ntok, lat0 = sd.tokenize(prompts).long(), sd.tokenize(["blurry", "blurry"]).long(), sd.initial_latents(seeds, 4, 16, 16)
            device, seed = str(sd.device), sd.config.seed
        finally:
            clip.engine.close()
    # the weights random_init drew: same seed, same device (the device's generator); returned on the host, where the oracle runs
    uw, vw = pkg.make_sd_weights(arch, seed, device=device)
    with torch.no_grad():
        cond = clip_oracle.text_hidden(cw[1], tok, carch.text.heads)
        unc = clip_oracle.text_hidden(cw[1], ntok, carch.text.heads)
        ref = sd_oracle.generate(uw, vw, arch, cond, unc, lat0, steps, guidance)
    d16, dbf = (imgs["fp16"] - ref).abs(), (imgs["bf16"] - ref).abs()
    print(f"[measured] full SD pipeline, toy geometry, {steps} steps, pixels in [0, 1]: fp16 max |d| {d16.max().item():.2e} mean |d| {d16.mean().item():.2e}"
          f"  |  bf16 max |d| {dbf.max().item():.2e} mean |d| {dbf.mean().item():.2e}  (the text states come from the bf16 tower in both)")
    assert imgs["fp16"].shape == (2, 3, 32, 32) and torch.isfinite(imgs["fp16"]).all()
    assert d16.max().item() <= dbf.max().item() and d16.mean().item() <= dbf.mean().item()
    assert d16.max().item() < 9.6e-3 and d16.mean().item() < 1.7e-3        # measured 4.76e-3 / 8.17e-4 (bf16 3.81e-2 / 6.23e-3)


def test_reference_generator_passes_precision_through(pkg, monkeypatch):
    """``SDReferenceConfig.precision`` reaches the kernels; the default config builds bf16 and ``torch_dtype`` selects nothing.
    The generator builds its model from the model name alone, so the name's architecture is swapped for the toy one here
    (0.9 G random parameters per case otherwise)."""
    monkeypatch.setattr(pkg.SDArch, "sd15", staticmethod(lambda: toy_arch(pkg)))
    carch = pkg.get_arch("ViT-T/16-test")                     # text width 128 = the toy UNet's cross_attention_dim
    kw = dict(num_images_per_prompt=1, num_inference_steps=2, use_text_variants=False, filter_low_quality=False, enable_cache=False,
              random_init=True, height=32, width=32)
    for precision, cfg in (("fp16", pkg.SDReferenceConfig(precision="fp16", **kw)), ("bf16", pkg.SDReferenceConfig(**kw))):
        assert cfg.torch_dtype == "float16"                   # the compatibility field selects nothing
        clip = pkg.CLIPModel(pkg.CLIPConfig(model_name=carch.name), weights=pkg.synth.make_clip_weights(carch, seed=0))
        try:
            gen = pkg.SDReferenceGenerator(cfg, clip_model=clip)
            assert gen.sd_model is not None and gen.sd_model.arch.block_out_channels == (64, 128)
            assert gen.sd_model.kernels.precision == precision
            assert gen.sd_model.kernels.tensors["conv_in.weight"].dtype == (torch.float16 if precision == "fp16" else torch.bfloat16)
            out = gen.generate_reference_images("a red cube", seeds=[3])
            assert "error" not in out, out.get("error")
        finally:
            clip.engine.close()
