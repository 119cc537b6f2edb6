"""GPU: the fp16 tower mode -- ``TVCEngine(precision="fp16")`` / ``CLIPConfig(precision="fp16")``
(``TVC_OPT_TOWER_PRECISION = 3``): the bf16 path's launches with IEEE fp16 weights and 16-bit activations, the products on
v_mfma_f32_16x16x32_f16 (the bf16 rate).  The reference runs its towers in fp16 (configs/defenses/tvc.yaml: precision).

fp16 rounds with 10 mantissa bits against bf16's 7, so every kernel's rounding error should be ~1/8 of the bf16 one: the
relative assertions below (fp16 error <= 0.3 / 0.35 x the bf16 error on the same inputs) hold on any box.  fp16's range ends
at 65504: overflow must show as inf, never be clamped.  Measured numbers are printed (pytest -s) and recorded in DESIGN.md
section 2.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import clip_oracle, tvc_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMM_KEYS = {"patch_w", "proj", "wqkv", "wo", "w1", "w2"}
SCORE_COLS = ((0, "original_similarity"), (1, "variant_mean"), (2, "variant_std"), (5, "score_src"),
              (6, "retrieval_consistency"), (10, "overall_exp"))


def round_gemm_weights(w, dtype):
    """Copy of a weight dict whose GEMM operands are rounded to ``dtype`` and back (what the HIP path multiplies with)."""
    rnd = lambda t: t.to(dtype).to(torch.float32)      # noqa: E731
    out = {}
    for k, v in w.items():
        if k == "layers":
            out[k] = [{kk: (rnd(vv) if kk in GEMM_KEYS else vv) for kk, vv in lw.items()} for lw in v]
        else:
            out[k] = rnd(v) if k in GEMM_KEYS else v
    return out


# ---------------------------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("I,J,K", [(128, 128, 64), (200, 333, 576), (3072, 257, 1024), (1024, 1000, 4096), (768, 7, 768),
                                   (320, 2000, 128), (1024, 1280, 640), (1024, 16384, 1024)])
def test_gemm_f16_vs_fp64(pkg, I, J, K):
    """fp16 operands (exact in fp64), fp32 accumulation: every epilogue against fp64 on the SAME fp16 operands.  The
    shapes cover the one-tile kernel (< 8 tiles), ring form 1 (8-63 tiles / ragged rows) and the 64-deep ring form
    (>= 64 whole tiles), K = 640 (the ViT-L/14 patch embedding)."""
    eng = pkg.TVCEngine()
    g = torch.Generator().manual_seed(I + J + K)
    a = (torch.randn((I, K), generator=g) * K ** -0.5).half()
    b = torch.randn((J, K), generator=g).half()
    bias = torch.randn((I,), generator=g)
    ref = b.double() @ a.double().t() + bias.double()
    out32 = eng.gemm_f16(a.cuda(), b.cuda(), bias.cuda(), 0).cpu()
    out = out32.double()
    e32 = (out - ref).abs().max().item()
    assert e32 < 2e-6 * (1 + ref.abs().max().item()), e32
    # fp16 store: the same fp32 sums (same K order in every epilogue), rounded once to nearest even
    o16 = eng.gemm_f16(a.cuda(), b.cuda(), bias.cuda(), 1).cpu()
    assert o16.dtype == torch.float16 and torch.equal(o16, out32.half())
    gel = ref * torch.sigmoid(1.702 * ref)
    og = eng.gemm_f16(a.cuda(), b.cuda(), bias.cuda(), 2).cpu().double()
    # one fp16 rounding (half an ulp; a whole one where the fp32 sum's own error crosses a rounding boundary)
    assert ((og - gel).abs() <= gel.abs() * 2.0 ** -10 + 1e-5).all()
    res = torch.randn((J, I), generator=g)
    acc = eng.gemm_f16(a.cuda(), b.cuda(), bias.cuda(), 3, out=res.clone().cuda()).cpu().double()
    assert (acc - (res.double() + ref)).abs().max().item() < 2e-6 * (1 + ref.abs().max().item() + res.abs().max().item())
    print(f"[measured] fp16 GEMM I={I} J={J} K={K}: fp32-store max|err| {e32:.2e}")
    eng.close()


def test_gemm_f16_subnormal_operands(pkg):
    """Operands of magnitude ~1e-5 are fp16 subnormals (< 6.1e-5).  Measured on gfx950: the f16 MFMA
    honours subnormal inputs -- the products match fp64 to the fp32 accumulation error, nothing is flushed to zero."""
    eng = pkg.TVCEngine()
    g = torch.Generator().manual_seed(5)
    I, J, K = 256, 512, 256
    a = (torch.randn((I, K), generator=g) * 1e-5).half()
    b = torch.ones((J, K)).half()
    assert (a.float().abs() < 6.1e-5).float().mean() > 0.99                # subnormal operands
    ref = b.double() @ a.double().t()
    out = eng.gemm_f16(a.cuda(), b.cuda(), None, 0).cpu().double()
    err = (out - ref).abs().max().item()
    flushed = out.abs().max().item() == 0.0
    print(f"[measured] fp16 GEMM on subnormal operands: max|ref| {ref.abs().max().item():.2e} max|err| {err:.2e} "
          f"({'FLUSHED to zero' if flushed else 'honoured'})")
    assert not flushed and err < 1e-6 * ref.abs().max().item() + 1e-12
    eng.close()


def test_gemm_f16_store_overflows_to_inf(pkg):
    """The fp16-store epilogue rounds to nearest even: 65519 -> 65504, anything >= 65520 -> +inf (-inf below), never a
    clamp to 65504."""
    eng = pkg.TVCEngine()
    I, J, K = 256, 64, 64
    a = torch.zeros((I, K)).half().cuda()
    b = torch.ones((J, K)).half().cuda()
    bias = torch.zeros(I)
    bias[0], bias[1], bias[2], bias[3], bias[4] = 65519.0, 65520.0, 1e5, -1e5, 3e38
    for epi in (1, 2):
        o = eng.gemm_f16(a, b, bias.cuda(), epi).float().cpu()
        assert (o[:, 0] == 65504.0).all() and (o[:, 1] == float("inf")).all() and (o[:, 2] == float("inf")).all()
        assert (o[:, 4] == float("inf")).all()
        if epi == 1:
            assert (o[:, 3] == float("-inf")).all()
        else:                                                  # QuickGELU(-1e5) = -0
            assert (o[:, 3] == 0).all()
    eng.close()


def _child(code, env):
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return [ln for ln in r.stdout.splitlines() if ln.startswith("checksum")]


# The shapes of _FORMS and the form each reaches per child (csrc/host_plan.hpp gemm_form; tests/test_gemm_form.py asserts
# these labels).  Ring forms 4 and 1 meet on four shapes; (3072, 300) has ragged token rows and runs ring form 1 in both
# processes, (1024, 131072, 64) and (768, 7) the one-tile kernel in both: for those three the bit comparison shows
# determinism only.  Split-K runs on (768, 7) under TVC_GEMM_SPLITK_SMALL=1, the split-K tail on (4096, 33024) under
# TVC_GEMM_SPLITK_TAIL=1.
_FORM_SHAPES = ((1024, 131072, 1024, 1), (4096, 33024, 1024, 2), (1024, 131072, 64, 1), (512, 65536, 640, 0),
                (768, 7, 768, 1), (3072, 300, 1024, 2), (1024, 2304, 4096, 1))
_FORM_LABELS = {
    "": ("RING4", "RING4", "ONE_TILE", "RING4", "ONE_TILE", "RING1", "RING4"),
    "TVC_GEMM_RING_FORM=1": ("RING1", "RING1", "ONE_TILE", "RING1", "ONE_TILE", "RING1", "RING1"),
    "TVC_GEMM_SPLITK_SMALL=1": ("RING4", "RING4", "ONE_TILE", "RING4", "SPLITK_SMALL", "RING1", "RING4"),
    "TVC_GEMM_SPLITK_TAIL=1": ("RING4", "SPLITK_TAIL", "ONE_TILE", "RING4", "ONE_TILE", "RING1", "RING4"),
    "TVC_GEMM_VARIANT=0": ("ONE_TILE",) * 7,
}
_FORMS = r'''
import torch, tvc_amd as pkg
eng = pkg.TVCEngine()
g = torch.Generator(device="cuda:0").manual_seed(11)
for I, J, K, epi in ''' + repr(_FORM_SHAPES) + r''':
    a = (torch.randn(I, K, device="cuda:0", generator=g) * K ** -0.5).half()
    b = torch.randn(J, K, device="cuda:0", generator=g).half()
    bias = torch.randn(I, device="cuda:0", generator=g) * 3.0
    out = eng.gemm_f16(a, b, bias, epi)
    rows = torch.cat([torch.arange(0, min(J, 512)), torch.arange(max(0, J - 512), J)]).cuda()
    ref = b[rows].double() @ a.double().t() + bias.double()
    if epi == 2:
        ref = ref * torch.sigmoid(1.702 * ref)
    err = ((out[rows].double() - ref).abs() - ref.abs() * (2.0 ** -11 if epi else 0.0)).max().item()
    assert err < 1e-4, (I, J, K, epi, err)
    bits = out.view(torch.int16 if out.dtype == torch.float16 else torch.int32).to(torch.int64)
    print("checksum", I, J, K, epi, int((bits * (torch.arange(bits.numel(), device="cuda:0").view(bits.shape) % 1000003 + 1)).sum().item()))
print("CHILD_OK")
'''


def test_gemm_f16_forms_bit_identical_and_variants_correct():
    """Ring forms 1 and 4 (TVC_GEMM_RING_FORM, read once per process) return the same fp16 BITS, as in bf16 (four of the
    seven shapes compare form 4 with form 1; see _FORM_LABELS for what each shape reaches); split-K small
    (TVC_GEMM_SPLITK_SMALL, on the 768 x 7 shape) and the one-tile kernel everywhere (TVC_GEMM_VARIANT=0) are correct in
    fp16 too, and so is the split-K tail (TVC_GEMM_SPLITK_TAIL, on the 4096 x 33024 shape)."""
    s4 = _child(_FORMS, {})
    s1 = _child(_FORMS, {"TVC_GEMM_RING_FORM": "1"})
    assert len(s4) == 7 and s1 == s4
    for env in ({"TVC_GEMM_SPLITK_SMALL": "1"}, {"TVC_GEMM_SPLITK_TAIL": "1"}, {"TVC_GEMM_VARIANT": "0"}):
        assert len(_child(_FORMS, env)) == 7


# ------------------------------------------------------------------------------------------------ attention, LayerNorm
def _attn_ref(qkv, n_seq, T, heads, causal):
    d = heads * 64
    q, k, v = qkv.double().view(n_seq, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) * 0.125
    if causal:
        s = s + torch.full((T, T), float("-inf"), dtype=torch.float64).triu(1)
    return (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(n_seq * T, d)


@pytest.mark.parametrize("n_seq,T,heads,causal", [(3, 257, 4, False), (5, 77, 2, True), (2, 50, 12, False), (1, 1, 1, True),
                                                  (40, 17, 4, False), (3, 272, 2, True), (2, 257, 16, False)])
def test_attention_f16_vs_fp64(pkg, n_seq, T, heads, causal):
    eng = pkg.TVCEngine()
    g = torch.Generator().manual_seed(T)
    d = heads * 64
    qkv = torch.randn((n_seq * T, 3 * d), generator=g)
    q16, qb = qkv.half(), qkv.bfloat16()
    e16 = (eng.attention_f16(q16.cuda(), n_seq, T, heads, causal).cpu().double() - _attn_ref(q16, n_seq, T, heads, causal)).abs().max().item()
    eb = (eng.attention(qb.cuda(), n_seq, T, heads, causal).cpu().double() - _attn_ref(qb, n_seq, T, heads, causal)).abs().max().item()
    print(f"[measured] attention n_seq={n_seq} T={T} heads={heads} causal={causal}: fp16 max|err| {e16:.2e}, bf16 {eb:.2e}")
    assert e16 < 2e-3 and e16 <= 0.3 * eb
    # packed (ragged) sequences, as the text tower (causal) and a packed vision batch see them
    if T >= 50:
        lens = [T, T - 13, 7][:n_seq]
        starts = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
        rows = int(starts[-1])
        got = eng.attention_f16(q16[:rows].cuda(), len(lens), T, heads, causal, starts=starts.cuda()).cpu()
        for i, L in enumerate(lens):
            blk = q16[int(starts[i]):int(starts[i]) + L]
            r = _attn_ref(blk, 1, L, heads, causal)
            assert (got[int(starts[i]):int(starts[i]) + L].double() - r).abs().max().item() < 2e-3
    eng.close()


@pytest.mark.parametrize("rows,d", [(300, 768), (77, 1024), (5, 128), (1, 64), (5, 260), (7, 1024)])      # + piece-loop edges
def test_layernorm_f16_vs_fp64(pkg, rows, d):
    eng = pkg.TVCEngine()
    g = torch.Generator().manual_seed(rows + d)
    x = torch.randn((rows, d), generator=g) * 3 + 1
    gam, bet = torch.randn(d, generator=g), torch.randn(d, generator=g)
    ref = torch.nn.functional.layer_norm(x.double(), (d,), gam.double(), bet.double(), eps=1e-5)
    y16 = eng.layernorm_f16(x.cuda(), gam.cuda(), bet.cuda()).cpu()
    yb = eng.layernorm(x.cuda(), gam.cuda(), bet.cuda()).cpu()
    assert y16.dtype == torch.float16
    e16, eb = (y16.double() - ref).abs().max().item(), (yb.double() - ref).abs().max().item()
    print(f"[measured] LayerNorm rows={rows} d={d}: fp16 max|err| {e16:.2e}, bf16 {eb:.2e}")
    assert ((y16.double() - ref).abs() <= ref.abs() * 2.0 ** -11 * 1.01 + 1e-5).all() and e16 <= 0.3 * eb
    eng.close()


# ------------------------------------------------------------------------------------------------------ mode semantics
def test_fp16_mode_needs_weights_and_tracks_the_oracle(pkg):
    """ViT-T/16-test: the fp16 embeddings against the fp32 oracle on fp16-rounded weights (the kernels' own arithmetic)
    and on the fp32 weights (end to end), each <= 0.35 x the bf16 mode's deviation on the same inputs."""
    arch = pkg.get_arch("ViT-T/16-test")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    eng = pkg.TVCEngine(arch, vw, tw)
    with pytest.raises(pkg.TVCError):                       # the C-ABI refuses mode 3 before tvc_set_weights_f16
        eng.set_option(pkg._lib.TVC_OPT_TOWER_PRECISION, 3)
    imgs = pkg.synth.make_images(6, arch.image_size, seed=1)
    toks = pkg.synth.make_tokens(3, 3, arch.ctx, seed=2).view(-1, arch.ctx)
    ib, tb, hb = eng.encode_image(imgs.cuda()).cpu(), eng.encode_text(toks.cuda()).cpu(), eng.encode_text_hidden(toks.cuda()).cpu()
    eng.set_precision("fp16")
    assert eng.precision == "fp16"
    i16, t16, h16 = eng.encode_image(imgs.cuda()).cpu(), eng.encode_text(toks.cuda()).cpu(), eng.encode_text_hidden(toks.cuda()).cpu()
    with torch.no_grad():
        def oracle(w_v, w_t):
            return (clip_oracle.vision_forward(w_v, imgs, arch.vision.heads, arch.patch),
                    clip_oracle.text_forward(w_t, toks.long(), arch.text.heads),
                    clip_oracle.text_hidden(w_t, toks.long(), arch.text.heads))
        r16 = oracle(round_gemm_weights(vw, torch.float16), round_gemm_weights(tw, torch.float16))
        rb = oracle(round_gemm_weights(vw, torch.bfloat16), round_gemm_weights(tw, torch.bfloat16))
        r32 = oracle(vw, tw)
    for name, got16, gotb, i in (("image", i16, ib, 0), ("text", t16, tb, 1), ("hidden", h16, hb, 2)):
        k16, kb = (got16 - r16[i]).abs().max().item(), (gotb - rb[i]).abs().max().item()
        e16, eb = (got16 - r32[i]).abs().max().item(), (gotb - r32[i]).abs().max().item()
        print(f"[measured] fp16 mode ViT-T/16-test {name}: vs oracle on rounded weights {k16:.2e} (bf16 {kb:.2e}); "
              f"vs fp32 weights {e16:.2e} (bf16 {eb:.2e})")
        assert torch.isfinite(got16).all() and k16 <= 0.35 * kb and e16 <= 0.35 * eb
    eng.close()


@pytest.mark.parametrize("model", ["ViT-T/16-test", "ViT-B/32"])
def test_fp16_pooled_last_layer_and_packing_are_bit_identical(pkg, model):
    """fp16 twin of test_gpu_path.py::test_pooled_last_layer_is_bit_identical: pooled last layer on == off, text packed ==
    prefix-shared == dense, all bit for bit."""
    arch = pkg.get_arch(model)
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    eng = pkg.TVCEngine(arch, vw, tw, precision="fp16")
    imgs = pkg.synth.make_images(5, arch.image_size, seed=1).cuda()
    toks = pkg.synth.make_tokens(6, 3, arch.ctx, seed=5, min_len=1, max_len=60)
    toks[1, 2] = toks[1, 0]                                   # a variant equal to its original
    toks[2, 1, 1:70] = 17; toks[2, 1, 70] = 49407; toks[2, 1, 71:] = 0     # a long one
    toks = toks.reshape(-1, arch.ctx).cuda()
    out = {}
    for pooled in (1, 0):
        eng.set_option(pkg._lib.TVC_OPT_POOLED_LAST_LAYER, pooled)
        res = [eng.encode_image(imgs), eng.encode_image(imgs, normalize=False)]
        for packing in (1, 0):
            eng.set_option(pkg._lib.TVC_OPT_TEXT_PACKING, packing)
            res.append(eng.encode_text(toks))
            res.append(eng.encode_text(toks, group=4))
        eng.set_option(pkg._lib.TVC_OPT_TEXT_PACKING, 1)
        out[pooled] = [r.cpu() for r in res]
    for a, b in zip(out[1], out[0]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert torch.equal(out[1][2], out[1][3]) and torch.equal(out[1][2], out[1][4])      # packed == shared == dense
    eng.close()


def test_precision_round_trips_reproduce_each_mode(pkg):
    """bf16 -> fp16 -> split -> fp16 -> bf16: every mode's outputs are reproduced exactly when it comes back."""
    arch = pkg.get_arch("ViT-T/16-test")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    eng = pkg.TVCEngine(arch, vw, tw)
    imgs = pkg.synth.make_images(3, arch.image_size, seed=1).cuda()
    toks = pkg.synth.make_tokens(2, 3, arch.ctx, seed=2).view(-1, arch.ctx).cuda()
    seen = {}
    for mode in ("bf16", "fp16", "split", "fp16", "bf16"):
        eng.set_precision(mode)
        r = [eng.encode_image(imgs).cpu(), eng.encode_text(toks, group=4).cpu(), eng.encode_text_hidden(toks).cpu()]
        if mode in seen:
            assert all(torch.equal(a, b) for a, b in zip(r, seen[mode])), mode
        seen[mode] = r
    assert not torch.equal(seen["fp16"][0], seen["bf16"][0])
    eng.close()


def test_fp16_overflow_shows_as_non_finite_embeddings(pkg):
    """A layer-0 fc2 bias of 1e5 (beyond fp16's 65504) makes the fp16 towers' embeddings non-finite (the delta becomes
    inf, it is not clamped), while the bf16 towers (range ~3e38) stay finite."""
    arch = pkg.get_arch("ViT-T/16-test")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    for w in (vw, tw):
        w["layers"][0]["b2"] = w["layers"][0]["b2"].clone()
        w["layers"][0]["b2"][3] = 1e5
    imgs = pkg.synth.make_images(2, arch.image_size, seed=1).cuda()
    toks = pkg.synth.make_tokens(1, 2, arch.ctx, seed=2).view(-1, arch.ctx).cuda()
    eng = pkg.TVCEngine(arch, vw, tw)
    assert torch.isfinite(eng.encode_image(imgs)).all() and torch.isfinite(eng.encode_text(toks)).all()
    eng.set_precision("fp16")
    assert not torch.isfinite(eng.encode_image(imgs)).all() and not torch.isfinite(eng.encode_text(toks)).all()
    eng.close()


# ---------------------------------------------------------------------------------------------------------- end to end
def _errs(rec, ref):
    return {key: float(np.abs(rec[:, col] - ref[key]).max()) for col, key in SCORE_COLS}


# End-to-end bounds, ~2x the deviations measured on an MI355X:
#   configs[0] (8 queries):  original_similarity 9.8e-5, score_src 8.0e-5, overall_exp 1.25e-3 (bf16: 8.1e-4, 2.6e-4, 1.8e-3)
#   configs[2] (12 queries): original_similarity 4.4e-5, score_src 3.0e-5, overall_exp 0        (bf16: 7.8e-4, 3.0e-4, 0)
# The retrieval fields (retrieval_consistency, hence overall_exp) of configs[0] deviate by about as much in fp16 as in bf16:
# they follow the DISCRETE reference choice of the bank search, which a 1e-4 change of an embedding can flip; the queries
# whose references differ from the oracle's are printed.  The continuous scores follow the towers' rounding (~1/8 of bf16).
CONFIG0_BOUND = {"original_similarity": 2e-4, "score_src": 1.6e-4, "overall_exp": 2.5e-3}
CONFIG2_BOUND = {"original_similarity": 1e-4, "score_src": 6e-5, "overall_exp": 2e-5}
SMOOTH = ("original_similarity", "variant_mean", "variant_std", "score_src")


def _ref_flips(a, b):
    """Queries whose retrieved reference indices differ between two detect_batch results."""
    ia, ib = np.asarray(a["retrieval_indices"]), np.asarray(b["retrieval_indices"])
    return int((ia.reshape(ia.shape[0], -1) != ib.reshape(ib.shape[0], -1)).any(axis=1).sum())


def test_fp16_config0_end_to_end(pkg):
    """BASELINE configs[0]: ViT-B/32, B = 8, N = 4, 1 k-row bank, every query; fp16 and bf16 on the same inputs."""
    arch = pkg.get_arch("ViT-B/32")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    eng = pkg.TVCEngine(arch, vw, tw)
    B, N, R = 8, 4, 1000
    images = pkg.synth.make_images(B, arch.image_size, seed=1)
    tokens = pkg.synth.make_tokens(B, N, arch.ctx, seed=2)
    with torch.no_grad():
        ri = clip_oracle.vision_forward(vw, images, arch.vision.heads, arch.patch)
        rt = clip_oracle.text_forward(tw, tokens.view(-1, arch.ctx).long(), arch.text.heads).view(B, N + 1, -1)
    bank = pkg.synth.plant_neighbours(pkg.synth.make_bank(R, arch.embed_dim, seed=7), rt.reshape(-1, arch.embed_dim), per_anchor=2)
    bank16 = bank.to(torch.bfloat16)
    eng.set_bank(bank16.cuda())
    ref = tvc_oracle.detect_batch(ri.numpy(), rt.numpy(), bank16.float().numpy(),
                                  checker=tvc_oracle.ConsistencyCheckerOracle(adaptive_threshold=False))
    errs = {}
    for mode in ("bf16", "fp16"):
        eng.set_precision(mode)
        fi = eng.encode_image(images.cuda())
        ft = eng.encode_text(tokens.view(-1, arch.ctx).cuda(), group=N + 1).view(B, N + 1, -1)
        rec = eng.detect_embeddings(fi, ft, pkg.ConsistencyConfig()).cpu().numpy()
        eng.bank_status()
        same = tvc_oracle.detect_batch(fi.cpu().numpy(), ft.cpu().numpy(), bank16.float().numpy(),
                                       checker=tvc_oracle.ConsistencyCheckerOracle(adaptive_threshold=False))
        assert max(_errs(rec, same).values()) < 1e-4          # consistency + bank search on identical embeddings
        errs[mode] = _errs(rec, ref)
        print(f"[measured] {mode} mode, configs[0] end to end vs the fp32 CPU path: "
              + "  ".join(f"|d {k}| {v:.2e}" for k, v in errs[mode].items())
              + f"; queries with other references than the oracle's: {_ref_flips(same, ref)} of {B}")
    for k, bound in CONFIG0_BOUND.items():
        assert errs["fp16"][k] < bound, (k, errs["fp16"][k])
    for k in errs["fp16"]:
        ratio = 0.35 if k in SMOOTH else 1.0
        assert errs["fp16"][k] <= ratio * errs["bf16"][k] + 2e-6, (k, errs["fp16"][k], errs["bf16"][k])
    eng.close()


def test_fp16_config2_step_sampled_queries(pkg):
    """The configs[2] step (ViT-L/14, B = 512, N = 8, 1 M-row bf16 bank) in bf16 and fp16 on the same inputs; 12 of its
    queries against the fp32 CPU towers + reference arithmetic."""
    arch = pkg.get_arch("ViT-L/14")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    eng = pkg.TVCEngine(arch, vw, tw)
    B, N, R, D = 512, 8, 1_000_000, arch.embed_dim
    images = pkg.synth.make_images(B, arch.image_size, seed=1).cuda()
    tokens = pkg.synth.make_tokens(B, N, arch.ctx, seed=2).cuda()
    cfg = pkg.ConsistencyConfig()
    k = max(cfg.search_k, cfg.reference_count)
    sub = np.linspace(0, B - 1, 12).astype(int)
    with torch.no_grad():
        ri = clip_oracle.vision_forward(vw, images[sub].cpu(), arch.vision.heads, arch.patch)
        rt = clip_oracle.text_forward(tw, tokens[sub].reshape(-1, arch.ctx).cpu().long(), arch.text.heads).view(len(sub), N + 1, D)
    bank = None
    errs = {}
    for mode in ("bf16", "fp16"):
        eng.set_precision(mode)
        ft = eng.encode_text(tokens.view(B * (N + 1), arch.ctx), group=N + 1)
        fi = eng.encode_image(images)
        if bank is None:
            bank = pkg.synth.make_bank(R, D, seed=7, device="cuda:0", dtype=torch.bfloat16)
            bank = pkg.synth.plant_neighbours(bank, ft.cpu(), per_anchor=1, seed=11)
            eng.set_bank(bank)
            ref = tvc_oracle.detect_batch(ri.numpy(), rt.numpy(), bank.float().cpu().numpy(),
                                          checker=tvc_oracle.ConsistencyCheckerOracle(adaptive_threshold=False))
        rows = torch.cat([fi, ft])
        idx, sim, _ = eng.bank_search(rows, k, cfg.similarity_threshold, want_moments=False)
        eng.bank_status()
        tidx, tsim = idx[B:], sim[B:]
        feat = eng.bank_gather(tidx[:, :cfg.reference_count].contiguous())
        rec = eng.consistency(fi, ft.view(B, N + 1, D), cfg, tidx.contiguous(), tsim.contiguous(), feat).cpu().numpy()
        assert np.isfinite(rec[:, :11]).all()
        same = tvc_oracle.detect_batch(fi.cpu().numpy()[sub], ft.view(B, N + 1, D).cpu().numpy()[sub], bank.float().cpu().numpy(),
                                       checker=tvc_oracle.ConsistencyCheckerOracle(adaptive_threshold=False))
        assert max(_errs(rec[sub], same).values()) < 1e-4
        errs[mode] = _errs(rec[sub], ref)
        print(f"[measured] {mode} mode, configs[2] step ({len(sub)} of 512 queries) vs the fp32 CPU path: "
              + "  ".join(f"|d {k_}| {v:.2e}" for k_, v in errs[mode].items())
              + f"; queries with other references than the oracle's: {_ref_flips(same, ref)} of {len(sub)}")
    for k_, bound in CONFIG2_BOUND.items():
        assert errs["fp16"][k_] < bound, (k_, errs["fp16"][k_])
    for k_ in errs["fp16"]:
        ratio = 0.35 if k_ in SMOOTH else 1.0
        assert errs["fp16"][k_] <= ratio * errs["bf16"][k_] + 2e-6, (k_, errs["fp16"][k_], errs["bf16"][k_])
    eng.close()


def test_pipeline_on_an_fp16_clip_model(pkg):
    """CLIPConfig(precision="fp16") reaches the pipeline through clip_model=: its decisions on the configs[0] queries equal
    those of the same pipeline on the fp32-grade towers (precision="split", the mode within 1e-4 of the fp32 CPU path),
    wherever the score is not within the two modes' difference of the threshold."""
    images = pkg.synth.make_images(8, 224, seed=1)
    texts = [f"a photo of a {w} on a {p}" for w, p in zip(("dog", "cat", "car", "boat", "bird", "horse", "chair", "tree"),
                                                           ("street", "sofa", "road", "lake", "branch", "field", "floor", "hill"))]
    out = {}
    for prec in ("fp16", "split"):
        clip = pkg.CLIPModel(pkg.CLIPConfig(model_name="ViT-B/32", precision=prec))
        assert clip.engine.precision == prec
        pc = pkg.PipelineConfig(enable_sd_reference=False,
                                detector_config=pkg.DetectorConfig(clip_model="ViT-B/32", num_text_variants=3))
        pipe = pkg.create_detection_pipeline(pc, clip_model=clip)
        out[prec] = pipe.detect(images=images, texts=texts)
        clip.engine.close()
    s16, s32 = np.array(out["fp16"]["scores"]), np.array(out["split"]["scores"])
    diff = float(np.abs(s16 - s32).max())
    print(f"[measured] pipeline on ViT-B/32: max |score fp16 - score split| {diff:.2e}")
    assert diff < 5e-3
    thr = np.array(out["split"]["scores"]) * 0 + 0.5
    clear = np.abs(s32 - thr) > 2 * diff
    assert (np.array(out["fp16"]["predictions"])[clear] == np.array(out["split"]["predictions"])[clear]).all()
