"""CPU: the fp64 references of tests/tower_ops_ref.py against torch's own fp64 ops and autograd, the integer text references
against torch.argmax / cumsum and hand-worked cases, and the CPU emulation of the kernels' LayerNorm summation order against
fp64.  tests/test_gpu_tower_ops.py judges the towers' row kernels with these."""
import math

import pytest
import torch
import torch.nn.functional as F

import tower_ops_ref as T

torch.manual_seed(0)
TOL = 1e-12
F64 = torch.float64


def _close(a, b, tol=TOL):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (a - b).abs().max().item() <= tol * (1 + b.abs().max().item())


def _rows(rows, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, d, dtype=F64, generator=g)
    return x * (0.5 + torch.arange(rows, dtype=F64)[:, None]) + torch.arange(rows, dtype=F64)[:, None] * 0.7 - 1.0


@pytest.mark.parametrize("d", [64, 260])
def test_layernorm_forward_and_magnitudes(d):
    x, g, b = _rows(5, d), torch.randn(d, dtype=F64), torch.randn(d, dtype=F64)
    y, mag = T.layernorm(x, g, b, parts=True)
    _close(y, F.layer_norm(x, (d,), g, b, T.LN_EPS))
    assert bool((mag >= y.abs()).all()) and bool((mag >= b.abs()).all())
    assert T.LN_EPS == float(torch.tensor(1e-5, dtype=torch.float32)) != 1e-5


@pytest.mark.parametrize("with_dres", [False, True])
def test_layernorm_backward_is_autograd(with_dres):
    d = 260
    x, g, b = _rows(5, d, 1).requires_grad_(), torch.randn(d, dtype=F64), torch.randn(d, dtype=F64)
    dy = torch.randn(5, d, dtype=F64)
    dres = torch.randn(5, d, dtype=F64) if with_dres else None
    F.layer_norm(x, (d,), g, b, T.LN_EPS).backward(dy)
    dx, mag = T.layernorm_bwd(x.detach(), dy, g, dres, parts=True)
    _close(dx, x.grad + (dres if with_dres else 0))
    assert bool((mag >= dx.abs()).all())
    # the three terms are all there: dropping mean(g) or the xhat term is far outside the comparison's tolerance
    rstd = 1.0 / torch.sqrt(x.detach().var(-1, unbiased=False, keepdim=True) + T.LN_EPS)
    assert ((rstd * (dy * g)) - x.grad).abs().max().item() > 1e-3


def test_lnpre_forward_and_backward_against_autograd():
    B, Tn, d = 3, 5, 64
    patch_out = torch.randn(B, Tn - 1, d, dtype=F64).float().double().requires_grad_()
    cls, pos = torch.randn(d, dtype=F64).float().double(), torch.randn(Tn, d, dtype=F64).float().double()
    g, b = torch.randn(d, dtype=F64), torch.randn(d, dtype=F64)
    rows = torch.cat([cls.expand(B, 1, -1), patch_out], dim=1) + pos
    y = F.layer_norm(rows, (d,), g, b, T.LN_EPS)
    # the references normalise the fp32 sum: 2^-24 relative away from the exact sum
    _close(T.assemble_lnpre(patch_out.detach(), cls, pos, g, b), y.detach(), 1e-6)
    assert torch.equal(T.lnpre_input(patch_out.detach(), cls, pos)[:, 0], T.f32(cls + pos[0]).expand(B, -1))
    dy = torch.randn(B, Tn, d, dtype=F64)
    y.backward(dy)
    _close(T.lnpre_bwd(patch_out.detach(), cls, pos, g, dy), patch_out.grad, 1e-5)
    dy2 = dy.clone()
    dy2[:, 0] = 1e9                                                     # the class rows of dy play no part
    assert torch.equal(T.lnpre_bwd(patch_out.detach(), cls, pos, g, dy2), T.lnpre_bwd(patch_out.detach(), cls, pos, g, dy))


def test_fold_deltas_order():
    x, d1, d2 = torch.tensor([1.0], dtype=F64), torch.tensor([2.0 ** -24], dtype=F64), torch.tensor([2.0 ** -24], dtype=F64)
    assert T.fold_deltas(x, d1, d2).item() == 1.0                       # (1 + 2^-24) ties to 1, twice
    assert T.f32(x + (d1 + d2)).item() == 1.0 + 2.0 ** -23              # the other order differs
    assert T.fold_deltas(x).item() == 1.0 and T.fold_deltas(x, d1 * 4).item() == 1.0 + 2.0 ** -22


@pytest.mark.parametrize("geom", [(32, 8), (28, 14), (30, 10)])
def test_im2col_and_col2im_are_unfold_and_fold(geom):
    S, patch = geom
    B, K = 3, 3 * patch * patch
    pix = torch.randn(B, 3, S, S, dtype=F64)
    cols = T.im2col(pix, patch)
    want = F.unfold(pix, patch, stride=patch).transpose(1, 2).reshape(-1, K)
    assert torch.equal(cols, want)
    Kp = (K + 63) // 64 * 64
    padded = T.im2col(pix, patch, Kp)
    assert torch.equal(padded[:, :K], want) and bool((padded[:, K:] == 0).all())
    junk = torch.full((cols.shape[0], Kp), float("nan"), dtype=F64)
    junk[:, :K] = cols
    back = T.col2im(junk, B, S, patch)
    assert torch.equal(back, pix)
    assert torch.equal(back, F.fold(cols.reshape(B, -1, K).transpose(1, 2), (S, S), patch, stride=patch))


def test_gelu_forms_and_gradient():
    u = torch.cat([torch.linspace(-12, 12, 4001, dtype=F64), torch.tensor([-0.75, 0.0, -0.0], dtype=F64)]).requires_grad_()
    y = T.quick_gelu(u)
    _close(y.detach(), (u * torch.sigmoid(1.702 * u)).detach())
    y.sum().backward()
    gr, mag = T.quick_gelu_grad(u.detach(), parts=True)
    _close(gr, u.grad)
    assert bool((mag >= gr.abs() - 1e-15).all())
    _close(T.gelu_erf(u.detach()), F.gelu(u.detach()))


@pytest.mark.parametrize("D", [8, 100])
def test_l2norm_and_its_backward(D):
    x = _rows(5, D, 3).requires_grad_()
    dy = torch.randn(5, D, dtype=F64)
    y = x / x.norm(dim=-1, keepdim=True)
    _close(T.l2norm(x.detach()), F.normalize(x.detach(), dim=-1, eps=0.0))
    y.backward(dy)
    dx, mag = T.l2norm_bwd(x.detach(), dy, parts=True)
    _close(dx, x.grad)
    assert bool((mag >= dx.abs() - 1e-15).all())


def test_split_planes_rounds_twice():
    x = torch.randn(4096, dtype=F64).float().double() * 37.0
    hi, lo = T.split_planes(x)
    assert torch.equal(hi, x.to(torch.bfloat16).double())
    assert torch.equal(lo, (x - hi).to(torch.bfloat16).double())
    assert ((hi + lo - x).abs() <= 2.0 ** -16 * x.abs()).all()


def test_gathers():
    bank = torch.randn(6, 24, dtype=F64).to(torch.bfloat16)
    idx = torch.tensor([3, 8, 2, 9, -1, 5], dtype=torch.int32)
    out = T.gather_rows(bank, 2, 10, idx, 3)
    assert torch.equal(out[0], bank[0, :10].float() + bank[0, 10:20].float())
    assert torch.equal(out[1], bank[5, :10].float() + bank[5, 10:20].float())
    assert bool((out[2] == 0).all()) and bool((out[3] == 0).all()) and bool((out[4] == 0).all())      # below, at R + offset, negative
    assert torch.equal(T.gather_rows(bank, 1, 10, idx, 3)[5], bank[2, :10].float())
    x = torch.randn(40, 12, dtype=F64)
    assert torch.equal(T.gather_f32_rows(x, torch.tensor([7, 7, 0], dtype=torch.int32), 0, 3, 8), x[[7, 7, 0], :8])
    assert torch.equal(T.gather_f32_rows(x, None, 5, 4, 8), x[[0, 5, 10, 15], :8])


def test_text_lengths_against_torch_and_by_hand():
    g = torch.Generator().manual_seed(5)
    tok = torch.randint(0, 50, (37, 9), generator=g)
    tok[3] = 0
    tok[4, 2] = tok[4, 6] = 99
    starts, pfx, lens = T.text_lens_scan(tok.tolist())
    assert pfx is None and lens == (tok.argmax(1) + 1).tolist() and lens[3] == 1 and lens[4] == 3
    assert starts[:37] == (torch.tensor(lens).cumsum(0) - torch.tensor(lens)).tolist()
    assert starts[37] == sum(lens) and starts[38] == max(lens)
    # one group of five by hand: base of length 4; identical; differs at 0; longer and equal on all of the base; shorter
    base = [5, 6, 7, 90, 0, 0]
    grp = [base, list(base), [4, 6, 7, 90, 0, 0], [5, 6, 7, 90, 91, 0], [5, 80, 0, 0, 0, 0]]
    starts, pfx, lens = T.text_lens_scan(grp, G=5)
    assert lens == [4, 4, 4, 5, 2]
    assert pfx[:5] == [0, 4, 0, 4, 1]                # the longer text first differs at 4 = the base's length
    assert starts == [0, 4, 4, 8, 9, 10, 5] and pfx[5:] == [0] * 5


def test_text_prefix_is_capped_by_the_base_length():
    base = [5, 90, 0, 0, 0]
    longer = [5, 90, 0, 0, 95]                       # equal to the base on positions 0..3, length 5, base length 2
    starts, pfx, lens = T.text_lens_scan([base, longer], G=2)
    assert lens == [2, 5] and pfx[:2] == [0, 2] and starts == [0, 2, 5, 5]


def test_text_embed_rows_and_eot():
    emb = torch.arange(40, dtype=torch.float32).reshape(10, 4)
    pos = torch.arange(24, dtype=torch.float32).reshape(6, 4) * 100
    base = [5, 6, 7, 9, 0, 0]
    grp = [base, list(base), [4, 6, 7, 9, 0, 0], [-1, 10, 0, 0, 0, 0]]
    rows, eot = T.text_embed(grp, emb, pos, 10)
    assert len(rows) == 24 and eot == [3, 9, 15, 19]
    assert torch.equal(rows[18], emb[0] + pos[0]) and torch.equal(rows[19], emb[9] + pos[1])          # -1 -> 0, 10 -> vocab - 1
    starts, pfx, _ = T.text_lens_scan(grp, G=4)
    rows, eot = T.text_embed(grp, emb, pos, 10, starts, pfx)
    assert starts[:5] == [0, 4, 4, 8, 10] and sorted(rows) == list(range(10))
    assert eot == [3, 3, 7, 9]                       # the identical text borrows its base's EOT row
    assert torch.equal(rows[4], emb[4] + pos[0]) and torch.equal(rows[8], emb[0] + pos[0])
    rows, eot = T.text_embed(grp, emb, pos, 10, *T.text_lens_scan(grp)[:2])
    assert sorted(rows) == list(range(14)) and eot == [3, 7, 11, 13]


@pytest.mark.parametrize("d", [64, 260, 768, 1024])
def test_emulated_summation_order_stays_inside_the_slack(d):
    """The kernels' fp32 order of sums on the CPU against fp64: its error must fit 2^-20 M with room to spare (the GPU tests
    use that coefficient; the emulation, not a GPU result, is what backs it).  rsqrt is taken as exact here."""
    x = _rows(7, d, 11).float()
    g, b = (1.0 + 0.5 * torch.randn(d, dtype=F64)).float(), (0.5 * torch.randn(d, dtype=F64)).float()
    got = T.layernorm_emulated(x, g, b).double()
    ref, mag = T.layernorm(x.double(), g.double(), b.double(), parts=True)
    worst = ((got - ref).abs() / mag).max().item()
    print(f"[measured] emulated LayerNorm d={d}: worst |emu - ref| / M = 2^{torch.log2(torch.tensor(worst)).item():.2f}")
    assert worst <= 2.0 ** -21
    mean, _ = T.ln_stats_emulated(x)
    _close(mean.double(), x.double().mean(-1), 1e-6)


def test_exact_coefficients_cover_the_cpu_fp32_forms():
    """C_EXACT (the slacks of the erff / expf / IEEE-division kernels) is at least twice the worst deviation of the same formula in
    fp32 torch on the CPU, on the GPU tests' inputs.  The ratio is printed: with this torch build every coefficient is below four
    times the deviation, i.e. the next power of two."""
    for k, v in sorted(T.cpu_fp32_deviation().items()):
        print(f"[measured] CPU fp32 {k}: worst deviation 2^{math.log2(v):.2f} M, C = 2^{math.log2(T.C_EXACT[k]):.0f}, C / deviation = {T.C_EXACT[k] / v:.2f}")
        assert 2.0 * v <= T.C_EXACT[k], (k, v, T.C_EXACT[k])


def test_text_prefix_is_capped_by_the_own_length():
    base = [5, 60, 0, 62]
    member = [5, 60, 0, 0]                           # first mismatch 3, own length 2, base length 4
    starts, pfx, lens = T.text_lens_scan([base, member], G=2)
    assert lens == [4, 2] and pfx[:2] == [0, 2] and starts == [0, 4, 4, 4]
    _, eot = T.text_embed([base, member], torch.zeros(64, 4), torch.zeros(4, 4), 64, starts, pfx)
    assert eot == [3, 1]                             # no own rows: the EOT row is the base's row of position 1


def _scan_with_one_cap_dropped(tok, G, drop):
    lens = [T.first_max(r) + 1 for r in tok]
    pref = []
    for n in range(len(tok)):
        bn = n // G * G
        mis = next((t for t in range(len(tok[n])) if tok[n][t] != tok[bn][t]), len(tok[n]))
        pref.append(0 if bn == n else min([mis] + [v for k, v in (("own", lens[n]), ("base", lens[bn])) if k != drop]))
    return pref


@pytest.mark.parametrize("drop", ["own", "base"])
def test_text_inputs_make_both_prefix_caps_bind(drop):
    """A prefix rule without the own-length cap, or without the base-length cap, gives another answer on the inputs of the GPU
    test at every large shape, with both group sizes: a kernel that lacks either cap cannot pass test_text_lens_scan."""
    for ctx, n_text in [(c, n) for c in (63, 64, 65, 77) for n in (1024, 1025, 2500)]:
        for G in (2, 8):
            tok = T.make_texts(n_text, ctx, G, 3000 + ctx + n_text)
            assert _scan_with_one_cap_dropped(tok, G, drop) != T.text_lens_scan(tok, G)[1][:n_text], (ctx, n_text, G)
            assert _scan_with_one_cap_dropped(tok, G, None) == T.text_lens_scan(tok, G)[1][:n_text]
