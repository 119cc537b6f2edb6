"""GPU: the split-bf16 input gradient (TVC_OPT_GRAD_PRECISION = 2; ``CLIPConfig(grad_precision="split")``) -- the attention
backward and the fp32 row kernels alone, the transposed weight planes, the forward with keep, the whole gradient, its
determinism and independence of mode 0, the attack loops and the Python surface.  The reference for every number is fp64 on
the CPU (tests/grad_split_ref.py, tests/tower_ops_ref.py): fp32 autograd's own error is of the size being measured.  Operands
as the kernels see them are hi + lo of the fp32 values (``grad_split_ref.operands``).  Measured figures print with -s."""
from pathlib import Path

import numpy as np
import pytest
import torch

import attack_ref
import grad_split_ref as R
import tower_ops_ref as T
from oracle import clip_oracle, synth_pgd

pytestmark = pytest.mark.gpu
F64 = torch.float64
GOLDEN = Path(__file__).resolve().parent / "golden" / "fsta_sma_t16.npz"

# ---------------------------------------------------------------------------------------------------------------------
# 1. attention backward alone
# ---------------------------------------------------------------------------------------------------------------------
ATT_SHAPES = [(1, 2, 3), (17, 3, 5), (32, 2, 2), (33, 2, 2), (50, 12, 3), (256, 2, 2), (257, 16, 2), (288, 2, 1)]
U_LOLO = 2.0 ** -18        # the dropped lo x lo term of a product of two split operands: |a_lo| <= 2^-9 |a|, |b_lo| <= 2^-9 |b|
U_SPLIT = 2.0 ** -17       # hi + lo of a value split INSIDE the kernel (P, dS) against the value: the issue's per-operand figure
U_ACC = 2.0 ** -23         # one fp32 accumulation step of the matrix pipe (round to nearest would be 2^-24)


def attention_bound(qkv, dout, heads, n_seq, Tn):
    """Element-wise error bound of dQ | dK | dV [rows, 3 W], first order, from the three-product form (fp64 tensors in, the
    operands the kernel sees).  For a product c = sum_k a_k b_k of n terms on hi | lo planes (3 n accumulated MFMA terms):
        |err c| <= (U_LOLO + 3 n U_ACC) sum_k |a_k| |b_k|          (+ U_SPLIT when one operand was split inside the kernel)
    Q, K, V and dO are the reference's own operands, so their split costs nothing; P and dS are split in the kernel.
      S  = Q K^T (n = 64):      eS  = (U_LOLO + 192 U_ACC) |Q| |K|^T
      P  = softmax(S / 8):      relative error rP_i = 2 max_j eS_ij / 8 (the shift of a row's logits, twice: numerator and sum)
                                + (T + 32) 2^-24 (exp2, the fp32 row sum over T, the division) + 2^-21 max_j |S_ij| / 8 (the fp32
                                scale constant and fma of the exponent's argument)
      dP = dO V^T (n = 64):     eP  = (U_LOLO + 192 U_ACC) |dO| |V|^T
      delta_i = sum_j P dP:     eD_i = sum_j P_ij (rP_i |dP_ij| + eP_ij) + (T + 8) 2^-24 sum_j P_ij |dP_ij|      (fp32 fma chain)
      dS = P (dP - delta) / 8:  eDS = (P (eP + eD) + (rP + 2^-22) P |dP - delta|) / 8
      dQ = dS K, dK = dS^T Q (n = T' = T rounded up to the 16- / 32-row tile):
                                e = eDS |K| + (U_SPLIT + U_LOLO + 3 T' U_ACC) |dS| |K|      (and with Q, transposed)
      dV = P^T dO:              e = (rP P)^T |dO| + (U_SPLIT + U_LOLO + 3 T' U_ACC) P^T |dO|
    plus one fp32 rounding of the stored result.  Second-order terms are below 1e-9 of these."""
    q, k, v, p = R.attention_parts64(qkv, heads, n_seq, Tn)
    do = dout.reshape(n_seq, Tn, heads, 64).transpose(1, 2)
    tp = (Tn + 31) // 32 * 32
    mm = lambda a, b: a @ b
    s = mm(q, k.transpose(-1, -2))
    e_s = (U_LOLO + 192 * U_ACC) * mm(q.abs(), k.abs().transpose(-1, -2))
    r_p = 2 * e_s.max(-1, keepdim=True).values / 8 + (Tn + 32) * 2.0 ** -24 + 2.0 ** -21 * s.abs().max(-1, keepdim=True).values / 8
    dp = mm(do, v.transpose(-1, -2))
    e_p = (U_LOLO + 192 * U_ACC) * mm(do.abs(), v.abs().transpose(-1, -2))
    delta = (p * dp).sum(-1, keepdim=True)
    e_d = (p * (r_p * dp.abs() + e_p)).sum(-1, keepdim=True) + (Tn + 8) * 2.0 ** -24 * (p * dp.abs()).sum(-1, keepdim=True)
    ds = p * (dp - delta) / 8
    e_ds = (p * (e_p + e_d) + (r_p + 2.0 ** -22) * p * (dp - delta).abs()) / 8
    c = U_SPLIT + U_LOLO + 3 * tp * U_ACC
    e_q = mm(e_ds, k.abs()) + c * mm(ds.abs(), k.abs())
    e_k = mm(e_ds.transpose(-1, -2), q.abs()) + c * mm(ds.abs().transpose(-1, -2), q.abs())
    e_v = mm((r_p * p).transpose(-1, -2), do.abs()) + c * mm(p.transpose(-1, -2), do.abs())
    back = lambda x: x.transpose(1, 2).reshape(n_seq * Tn, heads * 64)
    return torch.cat([back(e_q), back(e_k), back(e_v)], dim=1)


@pytest.mark.parametrize("Tn,heads,n_seq", ATT_SHAPES)
def test_attention_split_backward_vs_fp64(gpu_engine, Tn, heads, n_seq):
    """Every element of dQ, dK and dV inside ``attention_bound`` (derived there), outputs finite.
    Measured on an MI355X: worst |got - ref| / bound 0.032 (dV at T = 17; the bound is a worst case over every accumulation
    step), relative L2 error 3.7e-6 ... 5e-6 on all three outputs at every shape."""
    qkv, dout, ref = R.attention_case(Tn, heads, n_seq)
    got = gpu_engine.attention_split_backward(qkv.cuda(), dout.cuda(), n_seq, Tn, heads).cpu()
    assert torch.isfinite(got).all()
    bound = attention_bound(R.operands(qkv), R.operands(dout), heads, n_seq, Tn) + 2.0 ** -23 * ref.abs()
    W = heads * 64
    err = (got.double() - ref).abs()
    for name, sl in (("dq", slice(0, W)), ("dk", slice(W, 2 * W)), ("dv", slice(2 * W, 3 * W))):
        ratio = (err[:, sl] / bound[:, sl].clamp_min(1e-300)).max().item()
        print(f"[measured] attention split backward T={Tn} heads={heads} n_seq={n_seq} {name}: worst |got - ref| / bound = {ratio:.4f}; "
              f"rel L2 {R.rel_l2(got[:, sl], ref[:, sl]):.2e}  max/max {R.max_max(got[:, sl], ref[:, sl]):.2e}")
        assert bool((err[:, sl] <= bound[:, sl]).all()), (name, ratio)


@pytest.mark.parametrize("Tn,heads,n_seq", [(50, 2, 2), (257, 2, 1)])
def test_attention_split_backward_needle(gpu_engine, Tn, heads, n_seq):
    """dO is zero except one element and so is V (same sequence, head and head dim): dV is that column of the head (P^T dO), dP has
    one non-zero element, so dS fills the needle's query row, dQ that row of the head and dK every key of the head.  The non-zero
    pattern of the kernel's dQ | dK | dV is exactly the fp64 one."""
    W = heads * 64
    g0 = torch.Generator().manual_seed(7 + Tn)
    qkv = torch.randn(n_seq * Tn, 3 * W, generator=g0) * 0.7
    qkv[:, 2 * W:] = 0.0
    dout = torch.zeros(n_seq * Tn, W)
    seq, head, qi, ki, c = n_seq - 1, heads - 1, Tn // 3, Tn - 1, 37
    dout[seq * Tn + qi, head * 64 + c] = 0.83
    qkv[seq * Tn + ki, 2 * W + head * 64 + c] = -1.27
    ref = R.attention_backward64(R.operands(qkv), R.operands(dout), heads, n_seq, Tn)
    got = gpu_engine.attention_split_backward(qkv.cuda(), dout.cuda(), n_seq, Tn, heads).cpu()
    assert torch.isfinite(got).all()
    nz_ref, nz_got = ref != 0, got != 0
    assert nz_ref[:, :W].sum().item() == 64 and nz_ref[:, W:2 * W].sum().item() == 64 * Tn and nz_ref[:, 2 * W:].sum().item() == Tn
    assert torch.equal(nz_got, nz_ref), f"{(nz_got != nz_ref).sum().item()} elements differ in zero / non-zero"
    nzv = nz_ref.double()
    assert R.rel_l2(got.double() * nzv, ref) < 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# 2. row kernels alone, at the piece-loop edges
# ---------------------------------------------------------------------------------------------------------------------
ROW_SHAPES = [(1, 64), (5, 260), (7, 1024), (33, 192)]


@pytest.mark.parametrize("rows,d", ROW_SHAPES)
def test_gelu_bwd_f32_vs_fp64(gpu_engine, rows, d):
    """dm *= s + 1.702 u s (1 - s) on fp32, u = 0 and |u| = 20 planted.  Bound per element, from fp32 arithmetic:
    |dm| (2^-21 (s + |t|) + 1.702 |u| 2^-23): a few roundings of the two terms (expf, the division, three products), and 1 - s
    carries the absolute error 2^-24 of s into t = 1.702 u s (1 - s).  Nothing is read or written beyond n."""
    u = T.f32v(T.rnd(300 + d, rows, d) * 3.0)
    u.view(-1)[:4] = torch.tensor([0.0, 20.0, -20.0, -0.0], dtype=F64)
    dm = T.f32v(T.rnd(301 + d, rows, d))
    g, mag = T.quick_gelu_grad(u, parts=True)
    ref = dm * g
    buf = torch.full((rows * d + 64,), float("nan"), device="cuda")
    buf[:rows * d] = dm.float().reshape(-1).cuda()
    gpu_engine.grad_split_op("gelu_bwd", ins=[u.float().cuda()], outs=[buf], i=[rows * d])
    got = buf[:rows * d].cpu().double().reshape(rows, d)
    assert torch.isnan(buf[rows * d:]).all() and torch.isfinite(got).all()
    bound = dm.abs() * (2.0 ** -21 * mag + 1.702 * u.abs() * 2.0 ** -23)
    worst = ((got - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"[measured] gelu_bwd_f32 rows={rows} d={d}: worst |got - ref| / bound = {worst:.4f}")
    assert bool(((got - ref).abs() <= bound).all())
    assert got.view(-1)[0].item() == 0.5 * dm.view(-1)[0].item()          # u = 0: s = 1/2 exactly, t = 0


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("rows,d", ROW_SHAPES)
def test_l2norm_bwd_f32_vs_fp64(gpu_engine, rows, d, normalize):
    """(dy - y (y . dy)) / |x| in fp32; normalize 0: dy, bit for bit.  Bound 2^-19 M, M = (|dy| + |y| sum |y dy|) / |x|
    (tower_ops_ref.l2norm_bwd): the two row sums are chains of at most d / 64 fma steps and 6 shuffle adds per lane (<= 22
    roundings of 2^-24), the square root, the reciprocal and four more products."""
    x, dy = T.rows_of(310 + d, rows, d), T.f32v(T.rnd(311 + d, rows, d))
    out = torch.full((rows * d + 16,), float("nan"), device="cuda")
    gpu_engine.grad_split_op("l2norm_bwd", ins=[x.float().cuda() if normalize else None, dy.float().cuda()], outs=[out], i=[rows, d, normalize])
    got = out[:rows * d].cpu().double().reshape(rows, d)
    assert torch.isnan(out[rows * d:]).all()
    if not normalize:
        assert torch.equal(got, dy)
        return
    ref, mag = T.l2norm_bwd(x, dy, parts=True)
    worst = ((got - ref).abs() / (2.0 ** -19 * mag)).max().item()
    print(f"[measured] l2norm_bwd_f32 rows={rows} d={d}: worst |got - ref| = {worst:.4f} of 2^-19 M")
    assert worst <= 1.0


@pytest.mark.parametrize("B,Tn,d", [(1, 2, 64), (1, 6, 260), (7, 2, 1024), (3, 12, 192)])
def test_lnpre_bwd_f32_vs_fp64(gpu_engine, B, Tn, d):
    """The fp32-writing form of lnpre_bwd: B * (T - 1) patch rows (1, 5, 7 and 33 rows at the four widths of the piece loop).
    Bound 2^-20 M of tower_ops_ref.layernorm_bwd, the bound the bf16-writing form is held to before its rounding."""
    gamma = T.f32v(T.rnd(320 + d, d) * 0.2 + 1.0)
    patch_out = T.f32v(T.rnd(321 + d, B, Tn - 1, d) + 0.3)
    cls, pos = T.f32v(T.rnd(322, d)), T.f32v(T.rnd(323 + d, Tn, d) * 0.5)
    dy = T.f32v(T.rnd(324 + d, B, Tn, d))
    ref, mag = T.lnpre_bwd(patch_out, cls, pos, gamma, dy, parts=True)
    n = B * (Tn - 1)
    out = torch.full((n * d + 64,), float("nan"), device="cuda")
    f = lambda t: t.float().cuda().contiguous()
    gpu_engine.grad_split_op("lnpre_bwd", ins=[f(patch_out.reshape(-1, d)), f(pos), f(gamma), f(dy.reshape(-1, d))], outs=[out], i=[B, Tn, d])
    got = out[:n * d].cpu().double().reshape(ref.shape)
    assert torch.isnan(out[n * d:]).all() and torch.isfinite(got).all()
    worst = ((got - ref).abs() / (2.0 ** -20 * mag)).max().item()
    print(f"[measured] lnpre_bwd_f32 B={B} T={Tn} d={d}: worst |got - ref| = {worst:.4f} of 2^-20 M")
    assert worst <= 1.0


@pytest.mark.parametrize("rows,d", ROW_SHAPES)
def test_layernorm_bwd_f32_delta_vs_fp64(gpu_engine, rows, d):
    """LayerNorm backward with an fp32 delta folded into x, fp32 dy and the residual gradient added in place (ln_2 of the
    split-bf16 backward).  Bound 2^-20 M, as the bf16-delta form's."""
    x, delta = T.rows_of(330 + d, rows, d), T.f32v(T.rnd(331 + d, rows, d) * 0.3)
    gamma, dy, dres = T.f32v(T.rnd(332 + d, d) * 0.2 + 1.0), T.f32v(T.rnd(333 + d, rows, d)), T.f32v(T.rnd(334 + d, rows, d))
    ref, mag = T.layernorm_bwd(T.f32(x + delta), dy, gamma, dres, parts=True)
    f = lambda t: t.float().cuda().contiguous()
    dx = f(dres)
    gpu_engine.grad_split_op("layernorm_bwd", ins=[f(x), f(delta), f(dy), f(gamma), dx], outs=[dx], i=[rows, d, d, d])
    worst = ((dx.cpu().double() - ref).abs() / (2.0 ** -20 * mag)).max().item()
    print(f"[measured] layernorm_bwd_f32 rows={rows} d={d}: worst |got - ref| = {worst:.4f} of 2^-20 M")
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 3. transposed split planes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,K", [(192, 64), (200, 130)])
def test_transposed_split_planes(gpu_engine, I, K):
    """W [I, K] -> planes of W^T padded to the tiles the dX GEMM reads ([round_up(K, 256), 2 * round_up(I, 64)], zeroed by the
    caller as the product does): hi + lo read back equals hi + lo of W^T exactly, the padding stays zero."""
    Ip, Kr = (I + 63) // 64 * 64, (K + 255) // 256 * 256
    w = torch.randn(I, K, generator=torch.Generator().manual_seed(I + K)) * 0.05
    guard = torch.full((Kr + 2, 2 * Ip), 7.0, dtype=torch.bfloat16, device="cuda")
    guard[1:-1] = 0
    gpu_engine.grad_split_op("rows_split_t", ins=[w.cuda()], outs=[guard[1:-1]], i=[I, K, Ip, K])
    planes = guard[1:-1].cpu()
    assert bool((guard[0] == 7).all() and (guard[-1] == 7).all())
    hi, lo = planes[:, :Ip].float(), planes[:, Ip:].float()
    wt = w.t().contiguous()
    want_hi = wt.bfloat16().float()
    want_lo = (wt - want_hi).bfloat16().float()
    assert torch.equal(hi[:K, :I], want_hi) and torch.equal(lo[:K, :I], want_lo)
    assert torch.equal(hi[:K, :I].double() + lo[:K, :I].double(), R.operands(wt))
    pad = torch.ones(Kr, Ip, dtype=torch.bool)
    pad[:K, :I] = False
    assert (hi[pad] == 0).all() and (lo[pad] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. - 7. the tower
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(pkg):
    arch = pkg.get_arch("ViT-T/16-test")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    eng = pkg.TVCEngine(arch, vw, tw)
    yield arch, vw, tw, eng
    eng.close()


def test_forward_with_keep_matches_the_split_tower(pkg, toy):
    """Mode-2 encode_image_grad runs tower mode 2's forward over every token of every layer: its unit-row embeddings are within
    1e-6 (the project's per-unit-row cosine bound) of encode_image in precision "split"."""
    arch, vw, tw, eng = toy
    x = pkg.synth.make_images(3, arch.image_size, seed=5).cuda()
    f2 = eng.encode_image_grad(x, True, precision="split")
    eng.set_precision("split")
    try:
        fs = eng.encode_image(x, True)
    finally:
        eng.set_precision("bf16")
    d = (f2 - fs).abs().max().item()
    cosd = (1 - (f2 * fs).sum(-1)).abs().max().item()
    print(f"[measured] mode-2 grad forward vs split encode_image: max |d| {d:.2e}, max |1 - cos| {cosd:.2e}")
    assert d <= 1e-6 and cosd <= 1e-6
    with torch.no_grad():
        ref = clip_oracle.vision_forward(R.to_double(vw), x.cpu().double(), arch.vision.heads, arch.patch)
    assert (f2.cpu().double() - ref).abs().max().item() < 5e-5


def _compare_modes(pkg, arch, vw, eng, B, normalize, seed):
    x = pkg.synth.make_images(B, arch.image_size, seed=seed)
    t = torch.randn(arch.embed_dim, generator=torch.Generator().manual_seed(seed + 1))
    f64, g64, gp64 = R.tower_grad64(vw, x, t, arch.vision.heads, arch.patch, bool(normalize))
    xd, gd = x.cuda(), g64.float().cuda()
    out = {}
    for mode in ("split", "bf16"):
        f = eng.encode_image_grad(xd, bool(normalize), precision=mode)
        gp = eng.encode_image_backward(gd).cpu()
        assert torch.isfinite(gp).all()
        out[mode] = dict(rel=R.rel_l2(gp, gp64), mx=R.max_max(gp, gp64), flips=R.sign_flips(gp, gp64),
                         femb=(f.cpu().double() - f64).abs().max().item())
    return out


# rel L2 error of mode 2's grad_pix against fp64 per (B, normalize), first measured on an MI355X (the test allows twice this;
# mode 0 on the same inputs: 5.7e-3, 5.6e-3, 6.3e-3, 6.3e-3)
TOY_MEASURED_REL_L2 = {(1, 0): 9.118e-06, (1, 1): 9.753e-06, (3, 0): 1.033e-05, (3, 1): 1.025e-05}


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
def test_whole_gradient_vs_fp64(pkg, toy, B, normalize):
    """grad_pix of d(sum_b cos(f_b, t))/d pixels for a fixed text row, mode 2 and mode 0 on the same input against the double
    oracle.  Mode 2's relative L2 error is at most 1/16 of mode 0's (eight more significand bits are 256x in principle) and at
    most twice TOY_MEASURED_REL_L2 (first measured on an MI355X: 9.1e-6 ... 1.03e-5, 550 to 620 times below mode 0; no pixel's
    sign differs from fp64, against 0.14 % ... 0.22 % in mode 0); its share of sign flips is no larger than mode 0's."""
    arch, vw, tw, eng = toy
    r = _compare_modes(pkg, arch, vw, eng, B, normalize, 40 + B)
    for mode in ("split", "bf16"):
        m = r[mode]
        print(f"[measured] toy B={B} normalize={normalize} {mode}: grad_pix rel L2 {m['rel']:.3e}  max/max {m['mx']:.3e}  "
              f"sign flips {m['flips']:.2e}  |f - f64| {m['femb']:.2e}")
    assert r["split"]["rel"] <= r["bf16"]["rel"] / 16
    assert r["split"]["flips"] <= r["bf16"]["flips"]
    assert r["split"]["rel"] <= 2 * TOY_MEASURED_REL_L2[(B, normalize)]


B32_MEASURED_REL_L2 = 1.099e-05       # first measured on an MI355X (mode 0 on the same input: 6.68e-3)


def test_whole_gradient_vit_b32_geometry(pkg):
    """ViT-B/32 geometry, all 12 layers (the fp64 CPU reference takes about a second), B = 2, random weights: T = 50, 12 heads,
    768- and 3072-wide GEMMs (three and twelve 256-row weight tiles, a ragged token tile).  The same comparison, once."""
    arch = pkg.get_arch("ViT-B/32")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=3)
    eng = pkg.TVCEngine(arch, vw, None)
    try:
        r = _compare_modes(pkg, arch, vw, eng, 2, 1, 60)
    finally:
        eng.close()
    for mode in ("split", "bf16"):
        m = r[mode]
        print(f"[measured] ViT-B/32 B=2 {mode}: grad_pix rel L2 {m['rel']:.3e}  max/max {m['mx']:.3e}  sign flips {m['flips']:.2e}  "
              f"|f - f64| {m['femb']:.2e}")
    assert r["split"]["rel"] <= r["bf16"]["rel"] / 16
    assert r["split"]["flips"] <= r["bf16"]["flips"]
    assert r["split"]["rel"] <= 2 * B32_MEASURED_REL_L2


def test_determinism_and_independence_of_the_modes(pkg, toy):
    arch, vw, tw, eng = toy
    x = pkg.synth.make_images(3, arch.image_size, seed=9).cuda()
    g0 = torch.Generator().manual_seed(10)
    ga, gb = (torch.randn(3, arch.embed_dim, generator=g0).cuda() for _ in range(2))

    def pair(mode, g):
        f = eng.encode_image_grad(x, True, precision=mode)
        return f.clone(), eng.encode_image_backward(g).clone()

    f0, p0 = pair("bf16", ga)
    f2, p2 = pair("split", ga)
    f2b, p2b = pair("split", ga)
    f0b, p0b = pair("bf16", ga)
    assert torch.equal(p2, p2b) and torch.equal(f2, f2b), "two mode-2 pairs on the same input are bit-equal"
    assert torch.equal(p0, p0b) and torch.equal(f0, f0b), "mode 0 is untouched by a mode-2 pair in between (shared workspaces)"
    assert not torch.equal(p0, p2)
    # backward twice with different grad_out after ONE forward = two separate pairs
    eng.encode_image_grad(x, True, precision="split")
    qa, qb = eng.encode_image_backward(ga).clone(), eng.encode_image_backward(gb).clone()
    assert torch.equal(qa, p2) and torch.equal(qb, pair("split", gb)[1])
    assert eng.grad_precision == "bf16"                      # the per-call precision left the engine's own setting alone


# ---------------------------------------------------------------------------------------------------------------------
# 8. the loops
# ---------------------------------------------------------------------------------------------------------------------
def test_pgd_loop_vs_oracle_recipe(pkg):
    """PGDAttacker on the toy tower against oracle/synth_pgd.pgd_images on the same 4 images, text rows from the fp32 CPU tower
    for both runs: the share of bit-identical pixels with grad_precision="split" is at least the bf16 path's, and the final
    mean cos(text) (CPU oracle tower on both image sets) is within 1e-5 of the oracle's."""
    arch = pkg.get_arch("ViT-T/16-test")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    Q = 4
    clean = pkg.synth.make_images(Q, arch.image_size, seed=1)
    tokens = pkg.synth.make_tokens(Q, 1, arch.ctx, seed=2)[:, 0]
    want = synth_pgd.pgd_images(vw, tw, clean, tokens.long(), arch.vision.heads, arch.text.heads, arch.patch, seed=42)
    with torch.no_grad():
        tf = clip_oracle.text_forward(tw, tokens.long(), arch.text.heads)
    cos = lambda imgs: torch.nn.functional.cosine_similarity(
        clip_oracle.vision_forward(vw, imgs, arch.vision.heads, arch.patch), tf).mean().item()
    share, final = {}, {}
    for mode in ("bf16", "split"):
        clip = pkg.CLIPModel(pkg.CLIPConfig(model_name=arch.name, grad_precision=mode), weights=(vw, tw))
        try:
            assert clip.engine.grad_precision == mode
            atk = pkg.PGDAttacker(clip, pkg.PGDAttackConfig(batch_size=Q, random_seed=42))
            got = atk._steps(clean.cuda(), tf.cuda(), None).cpu()
        finally:
            clip.engine.close()
        share[mode] = (got == want).float().mean().item()
        with torch.no_grad():
            final[mode] = cos(got)
    with torch.no_grad():
        cw = cos(want)
    print(f"[measured] PGD toy, 4 images: bit-identical pixels bf16 {share['bf16']:.6f}  split {share['split']:.6f}; "
          f"final mean cos oracle {cw:.6f}  bf16 {final['bf16']:.6f}  split {final['split']:.6f}")
    assert share["split"] >= share["bf16"]
    assert abs(final["split"] - cw) <= 1e-5


@pytest.mark.parametrize("run", ["fsta", "sma"])
def test_fsta_sma_loops_vs_fixture(pkg, run):
    """FSTA and SMA (the L-inf runs of tests/golden/fsta_sma_t16.npz) with grad_precision="split": the identical-pixel share is at
    least the 99.5 % that EXPERIMENTS.md records for the bf16 gradient (0.9959 / 0.9951)."""
    A = pkg.attacks
    arch = pkg.get_arch("ViT-T/16-test")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    z = np.load(GOLDEN)
    clean, text, target = (torch.from_numpy(z[k]) for k in ("clean", "text", "target"))
    cfg = attack_ref.fixture_config(z, run)
    names = {k: cfg[k] for k in cfg if k not in ("num_iter",)}
    clip = pkg.CLIPModel(pkg.CLIPConfig(model_name=arch.name, grad_precision="split"), weights=(vw, tw))
    try:
        if run == "sma":
            atk = A.SMAAttacker(clip, A.SMAAttackConfig(num_iter=int(cfg["num_iter"]), enable_cache=False, **names))
            got = atk._loop(clean.cuda(), text.cuda(), target.cuda(), "batch").cpu()
        else:
            atk = A.FSTAAttacker(clip, A.FSTAAttackConfig(num_iter=int(cfg["num_iter"]), enable_cache=False, **names))
            got = atk._fsta_attack(clean, text, target).cpu()
    finally:
        clip.engine.close()
    want = torch.from_numpy(z[f"{run}_adv"])
    same = ((got - want).abs() < 1e-6).float().mean().item()
    print(f"[measured] {run} with the split-bf16 gradient vs the fixture: share of pixels within 1e-6 = {same:.6f}")
    assert torch.isfinite(got).all() and same >= 0.995


def test_pgd_concurrent_batches_bit_equal_in_mode_2(pkg):
    arch = pkg.get_arch("ViT-T/16-test")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    Q = 12                                          # batches of 8: a full one and a ragged one
    clean = pkg.synth.make_images(Q, arch.image_size, seed=5).cuda()
    texts = [f"a photo of thing {i}" for i in range(Q)]
    clip = pkg.CLIPModel(pkg.CLIPConfig(model_name=arch.name, grad_precision="split"), weights=(vw, tw))
    outs = {}
    try:
        for nc in (1, 2):
            atk = pkg.PGDAttacker(clip, pkg.PGDAttackConfig(batch_size=8, random_seed=7, num_steps=3, concurrent_batches=nc))
            outs[nc] = atk.perturb(clean, texts)
            torch.cuda.synchronize()
            if nc == 2:
                assert all(e.grad_precision == "split" for e in atk._pool)
            atk.close()
    finally:
        clip.engine.close()
    assert torch.isfinite(outs[1]).all() and (outs[1] - clean.clamp(0, 1)).abs().max().item() > 1e-3
    assert torch.equal(outs[2], outs[1])


# ---------------------------------------------------------------------------------------------------------------------
# 9. the Python surface
# ---------------------------------------------------------------------------------------------------------------------
def test_api(pkg):
    L = pkg._lib
    with pytest.raises(ValueError):
        pkg.CLIPConfig(grad_precision="fp64")
    arch = pkg.get_arch("ViT-T/16-test")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    x = pkg.synth.make_images(2, arch.image_size, seed=3).cuda()
    g = torch.randn(2, arch.embed_dim, generator=torch.Generator().manual_seed(4)).cuda()
    clip = pkg.CLIPModel(pkg.CLIPConfig(model_name=arch.name), weights=(vw, tw))
    eng = clip.engine
    try:
        with pytest.raises(ValueError):
            eng.set_grad_precision("fp32")
        with pytest.raises(ValueError):
            eng.encode_image_grad(x, True, precision="fp64")
        with pytest.raises(L.TVCError) as e:
            eng.set_option(L.TVC_OPT_GRAD_PRECISION, 1)
        assert e.value.code == L.TVC_E_INVALID
        # the default config runs the bf16 path: bit-equal to a direct pair with the option untouched
        assert eng.grad_precision == "bf16"
        f_direct = eng.encode_image_grad(x, True).clone()
        p_direct = eng.encode_image_backward(g).clone()
        xa = x.clone().requires_grad_(True)
        fa = clip.encode_image_tensor(xa, requires_grad=True)
        fa.backward(g)
        assert torch.equal(fa.detach(), f_direct) and torch.equal(xa.grad, p_direct)
        f_named, p_named = eng.encode_image_grad(x, True, precision="bf16").clone(), eng.encode_image_backward(g).clone()
        assert torch.equal(f_named, f_direct) and torch.equal(p_named, p_direct)
        # mode 2 on a model whose fp32 weights were never registered: the engine's state error, the C message
        eng.set_option(L.TVC_OPT_GRAD_PRECISION, 2)
        with pytest.raises(L.TVCError) as e:
            eng.encode_image_grad(x, True)
        assert e.value.code == L.TVC_E_STATE and "tvc_set_weights_f32" in str(e.value) and "TVC_OPT_GRAD_PRECISION" in str(e.value)
        # the option changed between a forward and its backward: refused, not mixed
        eng.set_option(L.TVC_OPT_GRAD_PRECISION, 0)
        eng.encode_image_grad(x, True)
        eng.set_option(L.TVC_OPT_GRAD_PRECISION, 2)
        with pytest.raises(L.TVCError) as e:
            eng.encode_image_backward(g)
        assert e.value.code == L.TVC_E_STATE and "changed" in str(e.value)
        eng.set_option(L.TVC_OPT_GRAD_PRECISION, 0)
        assert torch.equal(eng.encode_image_backward(g), p_direct)
        # set_grad_precision uploads what mode 2 needs; precision "bf16" with grad_precision "split" is a legal pair
        eng.set_grad_precision("split")
        assert eng.precision == "bf16" and eng.grad_precision == "split"
        xs = x.clone().requires_grad_(True)
        fs = clip.encode_image_tensor(xs, requires_grad=True)
        fs.backward(g)
        assert torch.isfinite(xs.grad).all() and not torch.equal(xs.grad, p_direct)
        assert (fs.detach() - f_direct).abs().max().item() < 5e-3             # the same tower, fp32-grade against bf16
    finally:
        eng.close()
