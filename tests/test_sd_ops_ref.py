"""CPU: the fp64 references of tests/sd_ops_ref.py against torch's own ops in fp64, and its 16-bit rounding bit for bit
against torch's conversions.  tests/test_gpu_sd_ops.py judges the row kernels of csrc/sd_ops.hip with these."""
import math

import pytest
import torch
import torch.nn.functional as F

import sd_ops_ref as R

torch.manual_seed(0)
TOL = 1e-12


def _close(a, b, tol=TOL):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (a - b).abs().max().item() <= tol * (1 + b.abs().max().item())


def _sweep(fmt):
    """fp32-representable values (torch converts a double through fp32): every finite 16-bit number, the midpoints
    between neighbours (ties), points just off them, the overflow threshold, subnormals, zeros, inf, nan."""
    dt = R.FORMATS[fmt]["dtype"]
    allbits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    v = allbits.view(dt).double()
    v = v[torch.isfinite(v)].sort().values
    mid = (v[1:] + v[:-1]) / 2
    near = torch.cat([mid * (1 + 2.0 ** -20), mid * (1 - 2.0 ** -20)])
    top = R.max_finite(fmt)
    extra = torch.tensor([0.0, -0.0, 65504.0, 65520.0, 65519.99, -65520.0, 65536.0, top, top * (1 + 2.0 ** -(R.FORMATS[fmt]["p"] + 1)),
                          top * (1 + 2.0 ** -(R.FORMATS[fmt]["p"])), -top * (1 + 2.0 ** -(R.FORMATS[fmt]["p"])), 1e-45, 6e-8, 2.98e-8,
                          2.99e-8, math.inf, -math.inf, math.nan, 3.3e38], dtype=torch.float64)
    x = torch.cat([v, mid, near, extra, torch.randn(4096, dtype=torch.float64) * 100])
    return x.float().double()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_round16_matches_torch_bit_for_bit(fmt):
    dt = R.FORMATS[fmt]["dtype"]
    x = _sweep(fmt)
    want = x.float().to(dt)
    got = R.round16(x, fmt)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan].to(dt).view(torch.int16), want[~nan].view(torch.int16))
    assert torch.equal(got[~nan], want[~nan].double())                       # the value itself, not only after a cast
    assert torch.equal(R.bits16(x[~nan], fmt), want[~nan].view(torch.int16))
    one = lambda v: R.round16(torch.tensor([v], dtype=torch.float64), fmt).item()
    assert one(65520.0) == (math.inf if fmt == "fp16" else 65536.0) and one(65504.0) == (65504.0 if fmt == "fp16" else 65536.0)
    assert math.copysign(1.0, one(-1e-60)) == -1.0 and one(-1e-60) == 0.0


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_ulp16_is_the_distance_to_the_next_number(fmt):
    dt = R.FORMATS[fmt]["dtype"]
    bits = torch.arange(0, 32768, dtype=torch.int32).to(torch.int16)
    v = bits.view(dt).double()
    fin = torch.isfinite(v)
    v = v[fin]
    gap = v[1:] - v[:-1]                                                       # value(b + 1) - value(b), b >= 0
    assert torch.equal(R.ulp16(v[:-1], fmt), gap)
    assert torch.equal(R.ulp16(-v[:-1], fmt), gap)
    inside = (v[:-1] + gap * 0.37)                                             # anywhere inside the gap: the same spacing
    assert torch.equal(R.ulp16(inside, fmt), gap)
    big = torch.tensor([R.max_finite(fmt) * 4, math.inf], dtype=torch.float64)
    assert torch.equal(R.ulp16(big, fmt), gap[-1].expand(2))


@pytest.mark.parametrize("n,H,W,C,groups,eps,act,tadd", [(2, 3, 4, 8, 1, 1e-5, False, False), (2, 5, 7, 32, 32, 1e-6, True, True),
                                                         (3, 5, 5, 320, 32, 1e-5, True, True), (1, 2, 2, 96, 32, 1e-6, False, True)])
def test_groupnorm(n, H, W, C, groups, eps, act, tadd):
    x = torch.randn(n, H, W, C, dtype=torch.float64) * 2 + 3
    ta = torch.randn(n, C, dtype=torch.float64) if tadd else None
    g, b = torch.randn(C, dtype=torch.float64), torch.randn(C, dtype=torch.float64)
    xs = x if ta is None else x + ta[:, None, None, :]
    want = F.group_norm(xs.permute(0, 3, 1, 2), groups, g, b, eps)
    want = (F.silu(want) if act else want).permute(0, 2, 3, 1)
    y, pre, mag = R.groupnorm(x, ta, g, b, groups, eps, act, parts=True)
    _close(y, want)
    _close(R.groupnorm(x, ta, g, b, groups, eps, act), want)
    assert bool((mag >= pre.abs() * (1 - 1e-12)).all())
    # the emulation of the kernel's summation order is the same function up to fp32 rounding
    x16 = R.round16(x, "bf16")
    ta32 = None if ta is None else ta.float().double()
    em = R.gn_emulated(x16, ta32, g.float().double(), b.float().double(), groups, eps)
    ref = R.groupnorm(x16, ta32, g.float().double(), b.float().double(), groups, eps)
    assert (em - ref).abs().max().item() < 1e-5 * (1 + ref.abs().max().item())


def test_gn_emulated_shows_the_cancellation():
    """At a large mean / std ratio E[x^2] - mean^2 in fp32 partial sums loses digits: the emulation deviates from fp64 by
    far more than at mean 0 (what the conditioning test of the GPU suite sizes its slack with)."""
    g, b = torch.ones(320, dtype=torch.float64), torch.zeros(320, dtype=torch.float64)
    base = torch.randn(1, 25, 25, 320, dtype=torch.float64)
    dev = {}
    for ratio in (0.0, 100.0):
        x = R.round16(base + ratio, "bf16")
        dev[ratio] = (R.gn_emulated(x, None, g, b, 32, 1e-5) - R.groupnorm(x, None, g, b, 32, 1e-5)).abs().max().item()
    assert dev[0.0] < 2e-6 and dev[100.0] > 20 * dev[0.0], dev


@pytest.mark.parametrize("rows,C,eps", [(1, 8, 1e-5), (5, 320, 1e-6), (3, 1536, 1e-5)])
def test_layernorm(rows, C, eps):
    x = torch.randn(rows, C, dtype=torch.float64) * 3 + 1
    g, b = torch.randn(C, dtype=torch.float64), torch.randn(C, dtype=torch.float64)
    y, mag = R.layernorm(x, g, b, eps, parts=True)
    _close(y, F.layer_norm(x, (C,), g, b, eps))
    assert bool((mag >= y.abs() * (1 - 1e-12)).all())


def test_geglu_gelu_silu_softmax():
    x = torch.randn(3, 32, dtype=torch.float64) * 3
    _close(R.gelu_erf(x), F.gelu(x))
    _close(R.geglu(x), x[:, :16] * F.gelu(x[:, 16:]))
    _close(R.silu(x), F.silu(x))
    s = torch.randn(3, 257, dtype=torch.float64) * 30
    s[1, 5] = 4000.0
    s[2, ::3] = -math.inf
    _close(R.softmax_rows(s, 1 / math.sqrt(512)), torch.softmax(s / math.sqrt(512), -1))
    assert bool((R.softmax_rows(s, 0.1)[2, ::3] == 0).all())
    g = torch.tensor([40.0, -40.0], dtype=torch.float64)
    assert R.gelu_erf(g)[0].item() == 40.0 and R.gelu_erf(g)[1].item() == 0.0          # erf saturates exactly


@pytest.mark.parametrize("n,Hi,Wi,C,stride,up", [(2, 5, 7, 16, 1, False), (2, 5, 7, 16, 2, False), (1, 3, 2, 8, 1, True),
                                                 (1, 1, 1, 8, 1, False), (1, 4, 6, 8, 2, False)])
def test_im2col3x3_is_unfold_in_tap_major_order(n, Hi, Wi, C, stride, up):
    x = torch.randn(n, Hi, Wi, C, dtype=torch.float64)
    src = x.permute(0, 3, 1, 2)
    if up:
        src = F.interpolate(src, scale_factor=2, mode="nearest")
        _close(R.upsample2(x), src.permute(0, 2, 3, 1))
    u = F.unfold(src, 3, padding=1, stride=stride)                            # [n, C * 9, L], row c * 9 + ky * 3 + kx
    L = u.shape[-1]
    want = u.reshape(n, C, 9, L).permute(0, 3, 2, 1).reshape(n * L, 9 * C)      # column tap * C + c
    got = R.im2col3x3(x, stride, up)
    assert torch.equal(got, want)
    assert R.im2col_column(2, 1, 3, C) == 7 * C + 3


def test_im2col_in():
    x = torch.randn(2, 4, 5, 7, dtype=torch.float64)
    scale = 1 / 0.18215
    u = F.unfold(x * scale, 3, padding=1)
    want = u.reshape(2, 4, 9, 35).permute(0, 3, 2, 1).reshape(70, 36)
    got = R.im2col_in(x, 64, scale)
    assert got.shape == (70, 64) and torch.equal(got[:, :36], want) and bool((got[:, 36:] == 0).all())


def test_layouts_and_moves():
    n, H, W, C = 2, 3, 5, 8
    x = torch.randn(n, H, W, C, dtype=torch.float64)
    xp = R.to_padded(x, math.nan)
    rows_d, rows_p = x.reshape(-1, C), xp.reshape(-1, C)
    for img in range(n):
        for t in range(H * W):
            assert R.tok_row(img, t, H, W, 0) == img * H * W + t
            assert torch.equal(rows_p[R.tok_row(img, t, H, W, 1)], rows_d[R.tok_row(img, t, H, W, 0)])
    m = R.border_mask(n, H, W)
    assert int(m.sum()) == n * ((H + 2) * (W + 2) - H * W) and bool(torch.isnan(xp[m]).all()) and torch.equal(R.interior(xp), x)
    assert torch.equal(R.relayout(xp, True, False, False), x)
    assert torch.equal(R.relayout(x, False, True, False), R.to_padded(x, 0.0))
    up = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(R.relayout(xp, True, True, True), R.to_padded(up, 0.0))
    a, b = torch.randn(7, 8, dtype=torch.float64), torch.randn(7, 16, dtype=torch.float64)
    assert torch.equal(R.concat(a, b), torch.cat([a, b], 1))
    z = torch.randn(2, 24, 35, dtype=torch.float64)
    assert torch.equal(R.nchw_to_tokens(z), z.permute(0, 2, 1).reshape(-1, 24))
    assert torch.equal(R.tokens_to_nchw16(R.nchw_to_tokens(z), 2), z)


def test_fp32_ops():
    rows = torch.randn(2 * 5 * 7, 8, dtype=torch.float64)
    v, mag = R.tokens_to_nchw(rows, 2, 7, 3, 5, 0.5, 0.5, True, True)
    g = rows.reshape(2, 5, 7, 8)[:, 1:-1, 1:-1, :7].permute(0, 3, 1, 2)
    _close(v, (g * 0.5 + 0.5).clamp(0, 1))
    assert v.shape == (2, 7, 3, 5) and bool((mag >= (g * 0.5 + 0.5).abs() - 1e-12).all())
    x, w, b = torch.randn(2, 4, 35, dtype=torch.float64), torch.randn(4, 4, dtype=torch.float64), torch.randn(4, dtype=torch.float64)
    v, _ = R.pointwise_small(x, w, b, 2.0)
    _close(v, F.conv1d(x * 2.0, w[:, :, None], b))
    e = torch.randn(20, dtype=torch.float64)
    _close(R.cfg(e, 7.5)[0], torch.lerp(e[:10], e[10:], 7.5))
    es = [torch.randn(10, dtype=torch.float64) for _ in range(4)]
    v, _ = R.lincomb(e[:10], 1.01, 0.02, es, (55 / 24, -59 / 24, 37 / 24, -9 / 24))
    _close(v, 1.01 * e[:10] - 0.02 * (torch.stack(es) * torch.tensor([55, -59, 37, -9], dtype=torch.float64)[:, None] / 24).sum(0))
    row, ang = R.timestep_embed(500.5, 320)
    k = torch.arange(160, dtype=torch.float64)
    want = 500.5 * 10000.0 ** (-k / 160)
    _close(ang[:160], want)
    _close(row, torch.cat([torch.cos(want), torch.sin(want)]))
