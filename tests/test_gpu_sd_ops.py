"""GPU: every row kernel of the latent-diffusion generator (csrc/sd_ops.hip, and the transpose the VAE attention uses) ALONE,
through tvc_sd_op, against the fp64 references of tests/sd_ops_ref.py (checked on the CPU by tests/test_sd_ops_ref.py), in
both 16-bit formats.

Harness (the GEMM contract test's): every output is a view inside a buffer of NaN bit patterns (0x7FA5 / 0x7FA5A5A5) with
at least 16 guard rows on each side, and every bit outside the op's defined output must survive the launch; every 16-bit
and fp32 input sits in such a buffer too, and a padded-layout input carries the NaN pattern in all its border rows and
columns -- a kernel that reads a border, a guard row or a pitch column shows as NaN in the result.  A padded-layout output
must hold 0x0000 in every border element.

Error rule for 16-bit results: |got - ref64| <= 0.5 * ulp16(ref64) + S, S the fp32 arithmetic slack of the op, stated at each
test (S = 0: the bits of round16(ref64)); where ref64 rounds to +-inf the output must be that inf.  fp32 results: a number
of fp32 ulps of the reference's magnitude sum.  Pure moves: equal bit patterns.  Every test prints one ``[measured]`` line:
the worst error beyond the slack in units of the 16-bit ulp (fp32 results: in fp32 ulps) and the slack in force."""
import ctypes as C
import importlib
import itertools
import math
from types import SimpleNamespace

import pytest
import torch

import sd_ops_ref as R
from gpu_ops_harness import (DEV, F32, G, SENT16, SENT32, U32, Buf, _pairwise, check16, check32, check_bits, in16, in32,
                             ulp32)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def E(request, pkg):
    """One engine without weights per 16-bit format: bf16 is the handle's default, fp16 is TVC_OPT_SD_PRECISION = 1."""
    sdm = importlib.import_module(pkg.__name__ + ".sd_model")
    eng = pkg.TVCEngine(device=DEV)
    if request.param == "fp16":
        eng.set_sd_precision("fp16")
    e = SimpleNamespace(eng=eng, fmt=request.param, dt=R.FORMATS[request.param]["dtype"], lib=pkg._lib,
                        op=lambda name, **kw: sdm.sd_op(eng, name, **kw))
    yield e
    eng.close()


# ------------------------------------------------------------------------------------------------------------ harness
def q16(x64, fmt):
    """The values the kernel sees: x rounded to the format, as fp64."""
    return R.round16(x64, fmt)


def f32v(x64):
    return x64.to(F32).double()


def eps32(eps):
    return float(torch.tensor(eps, dtype=F32))


def rnd(seed, *shape):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def plant(x, fmt, extra=()):
    """Put +-0, the largest finite value (both signs), one subnormal and ``extra`` into the first elements of x (flat)."""
    sub = {"bf16": 2.0 ** -130, "fp16": 2.0 ** -20}[fmt]
    v = [0.0, -0.0, R.max_finite(fmt), -R.max_finite(fmt), sub, -3 * sub] + list(extra)
    flat = x.reshape(-1)
    flat[:len(v)] = torch.tensor(v, dtype=torch.float64)[:flat.numel()]
    return x


def refused(E, name, outs, **kw):
    """The call raises (a non-zero return code) and no bit of the output buffers changed."""
    with pytest.raises(E.lib.TVCError):
        E.op(name, outs=[o.t for o in outs], **kw)
    torch.cuda.synchronize()
    for o in outs:
        assert o.untouched(), f"{name}: a refused call wrote its output"


def measured(family, E, worst, slack, unit="ulp16 (allowed 0.5)"):
    print(f"[measured] {family} {E.fmt}: worst |got - ref| - S = {worst:.4f} {unit}, S = {slack}")


# ---------------------------------------------------------------------------------------------------------- GroupNorm
GN_SHAPES = [(2, 3, 4, 8, 1), (2, 5, 7, 32, 32), (2, 8, 8, 96, 32), (3, 25, 25, 320, 32), (1, 9, 5, 2112, 32), (1, 2, 2, 4096, 32)]
GN_VARIANTS = _pairwise(dict(in_pad=(0, 1), out_pad=(0, 1), silu=(0, 1), tadd=(0, 1), eps=(1e-5, 1e-6)))


def _gn_run(E, x, tadd, gamma, beta, groups, eps, silu, in_pad, out_pad, what):
    """Launch GroupNorm on x [n, H, W, C] (fp64 values of the format); returns the output's interior as a CPU tensor of the
    16-bit dtype after the guard / border checks."""
    n, H, W, C = x.shape
    xb = in16(x, E.fmt, nan_border=bool(in_pad))
    ld_t = C + 24
    tb = None
    if tadd is not None:                              # a slice of a wider fp32 matrix: the columns beyond C are NaN
        full = torch.zeros((n, ld_t), dtype=F32)
        full[:, :C] = tadd.to(F32)
        mask = torch.zeros((n, ld_t), dtype=torch.bool)
        mask[:, C:] = True
        tb = in32(full, mask)
    gb, bb = in32(gamma), in32(beta)
    Ho, Wo = (H + 2, W + 2) if out_pad else (H, W)
    yb = Buf((n, Ho, Wo, C), E.dt)
    E.op("groupnorm", ins=[xb.t, None if tb is None else tb.t, gb.t, bb.t], outs=[yb.t],
         i=[n, H, W, C, groups, silu, in_pad, out_pad, ld_t], f=[eps])
    torch.cuda.synchronize()
    yb.guards_ok(what)
    y = yb.t.cpu()
    if out_pad:
        border = y.view(torch.int16)[R.border_mask(n, H, W)]
        assert bool((border == 0).all()), f"{what}: {int((border != 0).sum())} border elements of the padded output are not 0x0000"
        y = R.interior(y)
    return y


def _gn_inputs(E, shape, seed):
    n, H, W, C, groups = shape
    x = rnd(seed, n, H, W, C)
    for img in range(n):                              # another scale and mean per image: a wrong image index shows
        x[img] = x[img] * (0.5 + 0.75 * img) + (0.6 * img - 0.4)
    x = q16(x, E.fmt)
    x.reshape(-1)[:3] = torch.tensor([0.0, -0.0, {"bf16": 2.0 ** -130, "fp16": 2.0 ** -20}[E.fmt]], dtype=torch.float64)
    tadd = f32v(rnd(seed + 1, n, C) * 0.5 + torch.arange(n, dtype=torch.float64)[:, None] * 0.3 - 0.2)
    gamma = f32v(1.0 + 0.5 * rnd(seed + 2, C))
    beta = f32v(0.5 * rnd(seed + 3, C))
    return x, tadd, gamma, beta


@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm(E, shape):
    """S = 2^-20 (|ref| + |x' rstd gamma| + |mean rstd gamma| + |beta|) (a handful of fp32 operations on terms of these sizes); with
    SiLU the pre-activation's slack passes through the activation (|silu'| <= 1.1) and the fast exponential adds
    2^-15 |ref|."""
    n, H, W, C, groups = shape
    x, tadd, gamma, beta = _gn_inputs(E, shape, 100 + C)
    worst = 0.0
    for v in GN_VARIANTS:
        ta = tadd if v["tadd"] else None
        eps = eps32(v["eps"])
        what = f"groupnorm {E.fmt} {shape} {v}"
        y = _gn_run(E, x, ta, gamma, beta, groups, eps, v["silu"], v["in_pad"], v["out_pad"], what)
        ref, pre, mag = R.groupnorm(x, ta, gamma, beta, groups, eps, bool(v["silu"]), parts=True)
        S = 2.0 ** -20 * (pre.abs() + mag)
        if v["silu"]:
            S = 1.1 * S + 2.0 ** -15 * ref.abs()
        worst = max(worst, check16(y, ref, S, E.fmt, what))
    measured(f"groupnorm {shape}", E, worst, "2^-20 (|ref| + terms) [+ 2^-15 |ref| with SiLU]")


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_groupnorm_and_layernorm_use_the_eps_they_are_given(E, eps):
    """A variance of 2^-18 (3.8e-6), below both values of eps: the UNet's 1e-5 in place of the VAE's 1e-6 would change every
    output by a factor 1.7.  The rules and slacks of test_groupnorm / test_layernorm."""
    e32 = eps32(eps)
    shape = (2, 8, 8, 96, 32)
    x, _, gamma, beta = _gn_inputs(E, shape, 300)
    x = q16(rnd(301, *shape[:4]) * 2.0 ** -9, E.fmt)
    y = _gn_run(E, x, None, gamma, beta, 32, e32, 0, 1, 1, f"groupnorm eps {eps}")
    ref, pre, mag = R.groupnorm(x, None, gamma, beta, 32, e32, False, parts=True)
    w1 = check16(y, ref, 2.0 ** -20 * (pre.abs() + mag), E.fmt, f"groupnorm {E.fmt} small variance eps {eps}")
    xl = x.reshape(-1, 96)[:5].repeat(1, 5)[:, :320].contiguous()
    g64, b64 = f32v(1.0 + 0.5 * rnd(302, 320)), f32v(0.5 * rnd(303, 320))
    yb, _ = _ln(E, in16(xl, E.fmt), in32(g64), in32(b64), 5, 320, e32)
    ref, mag = R.layernorm(xl, g64, b64, e32, parts=True)
    w2 = check16(yb.t, ref, 2.0 ** -20 * (ref.abs() + mag), E.fmt, f"layernorm {E.fmt} small variance eps {eps}")
    measured(f"groupnorm / layernorm small variance eps={eps}", E, max(w1, w2), "2^-20 (|ref| + terms)")


def test_groupnorm_refusals(E):
    """groups = 64, C % groups != 0, C % 8 != 0, C = 4104, and what the entry itself refuses: nothing is launched."""
    for C_, groups in ((64, 64), (24, 32), (12, 4), (4104, 1)):
        x = in16(rnd(1, 1, 2, 2, C_), E.fmt)
        g, b = in32(torch.ones(C_)), in32(torch.zeros(C_))
        y = Buf((1, 2, 2, C_), E.dt)
        refused(E, "groupnorm", [y], ins=[x.t, None, g.t, b.t], i=[1, 2, 2, C_, groups, 0, 0, 0, 0], f=[1e-5])
    x = in16(rnd(1, 1, 2, 2, 8), E.fmt)
    g, b = in32(torch.ones(8)), in32(torch.zeros(8))
    y = Buf((1, 2, 2, 8), E.dt)
    refused(E, "groupnorm", [y], ins=[None, None, g.t, b.t], i=[1, 2, 2, 8, 1, 0, 0, 0, 0], f=[1e-5])      # NULL x
    refused(E, "groupnorm", [y], ins=[x.t, None, g.t, b.t], i=[1, 0, 2, 8, 1, 0, 0, 0, 0], f=[1e-5])       # H = 0
    refused(E, "groupnorm", [y], ins=[x.t, None, g.t, b.t], i=[1, 2, 2, 8, 0, 0, 0, 0, 0], f=[1e-5])       # groups = 0
    refused(E, "groupnorm", [y], ins=[x.t, g.t, g.t, b.t], i=[1, 2, 2, 8, 1, 0, 0, 0, 4], f=[1e-5])        # ld_t < C
    a = E.lib.SDOpArgs()
    assert E.eng.lib.tvc_sd_op(E.eng.handle, 99, C.byref(a), None) == E.lib.TVC_E_INVALID                  # unknown op
    assert E.eng.lib.tvc_sd_op(E.eng.handle, 0, None, None) == E.lib.TVC_E_INVALID                         # NULL arguments
    torch.cuda.synchronize()
    assert y.untouched()


def test_groupnorm_conditioning(E):
    """Input mean / std = ratio per channel (half of the shift through tadd), 10 channels per group, 10 slabs: the kernel keeps
    fp32 sums and sums of squares per slab and forms the variance as E[x^2] - mean^2.  Bound: 0.5 ulp16 + 4 E, E = the largest
    deviation of sd_ops_ref.gn_emulated (the same summation order, on the CPU) from fp64 on the same input -- the reference
    sizes the slack, not the kernel.  Ratios 0 and 30, and 300 in fp16 only (bf16 cannot hold a unit spread at 150)."""
    for ratio in (0, 30) + ((300,) if E.fmt == "fp16" else ()):
        _gn_conditioning(E, ratio)


def _gn_conditioning(E, ratio):
    n, H, W, C, groups = 2, 25, 25, 320, 32
    x = rnd(7, n, H, W, C)
    x[0] += ratio / 2.0
    x[1] -= ratio / 2.0                                   # the other image: the shift with the other sign
    x = q16(x, E.fmt)
    sign = torch.tensor([1.0, -1.0], dtype=torch.float64)[:, None]
    tadd = f32v(sign * ratio / 2.0 + 0.01 * rnd(8, n, C))
    gamma, beta = f32v(1.0 + 0.1 * rnd(9, C)), f32v(0.1 * rnd(10, C))
    eps = eps32(1e-5)
    what = f"groupnorm conditioning {E.fmt} mean/std {ratio}"
    y = _gn_run(E, x, tadd, gamma, beta, groups, eps, 0, 0, 0, what)
    ref = R.groupnorm(x, tadd, gamma, beta, groups, eps)
    emu = (R.gn_emulated(x, tadd, gamma, beta, groups, eps) - ref).abs().max().item()
    g = y.double()
    excess = ((g - ref).abs() - 0.5 * R.ulp16(ref, E.fmt)).clamp(min=0).max().item()
    print(f"[measured] groupnorm conditioning {E.fmt} mean/std {ratio}: CPU-emulated E = {emu:.3e}, GPU |got - ref| beyond "
          f"0.5 ulp16 = {excess:.3e} (allowed 4 E = {4 * emu:.3e}), worst |got - ref| = {(g - ref).abs().max().item():.3e}")
    check16(y, ref, 4.0 * emu, E.fmt, what)


# ---------------------------------------------------------------------------------------------------------- LayerNorm
LN_C = (8, 320, 512, 520, 1280, 1536)
LN_ROWS = (1, 5, 257)


def _ln(E, xb, gb, bb, rows, C_, eps, add=None):
    yb = Buf((rows, C_), E.dt)
    sb = Buf((rows, C_), E.dt) if add is not None else None
    E.op("layernorm", ins=[xb.t, gb.t, bb.t, None if add is None else add.t], outs=[yb.t, None if sb is None else sb.t],
         i=[rows, C_], f=[eps])
    torch.cuda.synchronize()
    yb.guards_ok("layernorm y")
    if sb is not None:
        sb.guards_ok("layernorm sum_out")
    return yb, sb


@pytest.mark.parametrize("C_", LN_C)
def test_layernorm(E, C_):
    """S = 2^-20 (|ref| + |x - mean| rstd |g| + |b|): two wave sums and three fp32 operations per element."""
    worst = 0.0
    g64, b64 = f32v(1.0 + 0.5 * rnd(20, C_)), f32v(0.5 * rnd(21, C_))
    gb, bb = in32(g64), in32(b64)
    for rows in LN_ROWS:
        x = rnd(22 + rows, rows, C_) * 2.0 + 1.0
        x.reshape(-1)[:3] = torch.tensor([0.0, -0.0, {"bf16": 2.0 ** -130, "fp16": 2.0 ** -20}[E.fmt]], dtype=torch.float64)
        x = q16(x, E.fmt)
        xb = in16(x, E.fmt)
        for eps in (eps32(1e-5), eps32(1e-6)):
            yb, _ = _ln(E, xb, gb, bb, rows, C_, eps)
            ref, mag = R.layernorm(x, g64, b64, eps, parts=True)
            worst = max(worst, check16(yb.t, ref, 2.0 ** -20 * (ref.abs() + mag), E.fmt, f"layernorm {E.fmt} rows {rows} C {C_} eps {eps}"))
    measured(f"layernorm C={C_}", E, worst, "2^-20 (|ref| + terms)")


@pytest.mark.parametrize("C_", LN_C)
def test_layernorm_with_folded_add(E, C_):
    """sum_out = round16(x + add) bit for bit (S = 0: the fp32 sum of two 16-bit numbers is exact), and y bit for bit what the
    add op followed by the plain LayerNorm op gives on the same engine.  fp16: a row whose sum overflows stores inf."""
    g64, b64 = f32v(1.0 + 0.5 * rnd(30, C_)), f32v(0.5 * rnd(31, C_))
    gb, bb = in32(g64), in32(b64)
    for rows, eps in ((1, 1e-5), (5, 1e-6), (257, 1e-5)):
        x = q16(rnd(32 + rows, rows, C_) * 2.0 + 1.0, E.fmt)
        a = q16(rnd(33 + rows, rows, C_), E.fmt)
        if rows > 1:                                      # the last row: +-0, the largest finite value, a subnormal; fp16: overflow
            plant(x[-1], E.fmt)
            plant(a[-1], E.fmt)
        xb, ab = in16(x, E.fmt), in16(a, E.fmt)
        yb, sb = _ln(E, xb, gb, bb, rows, C_, eps, add=ab)
        what = f"layernorm+add {E.fmt} rows {rows} C {C_}"
        want = R.bits16(x + a, E.fmt)
        check_bits(sb.bits(), want, what + " sum_out")
        if rows > 1 and E.fmt == "fp16":
            assert math.isinf(sb.t[-1, 2].item()) and math.isinf(sb.t[-1, 3].item()), "max + max must come out as inf"
        tb = Buf((rows, C_), E.dt)
        E.op("add", ins=[xb.t, ab.t], outs=[tb.t], i=[rows * C_])
        check_bits(tb.bits(), want, what + " add op")
        y2, _ = _ln(E, tb, gb, bb, rows, C_, eps)
        check_bits(yb.bits(), y2.bits().cpu(), what + " y against add -> layernorm")
        keep = rows - 1 if rows > 1 else rows             # the planted row is not finite after the sum of maxima
        s = q16(x + a, E.fmt)[:keep]
        ref, mag = R.layernorm(s, g64, b64, eps32(eps), parts=True)
        check16(yb.t[:keep], ref, 2.0 ** -20 * (ref.abs() + mag), E.fmt, what)
    measured(f"layernorm+add C={C_}", E, 0.0, "0 (bits of round16(x + add), bits of add -> layernorm)")


def test_layernorm_refusals_and_zero_rows(E):
    x = in16(rnd(1, 2, 1544), E.fmt)
    g, b = in32(torch.ones(1544)), in32(torch.zeros(1544))
    y, s = Buf((2, 1544), E.dt), Buf((2, 1544), E.dt)
    refused(E, "layernorm", [y], ins=[x.t, g.t, b.t, None], i=[2, 1544], f=[1e-5])                        # C > 1536
    refused(E, "layernorm", [y], ins=[x.t, g.t, b.t, None], i=[2, 12], f=[1e-5])                          # C % 8
    refused(E, "layernorm", [y], ins=[x.t, g.t, b.t, x.t], i=[2, 8], f=[1e-5])                            # add without sum_out
    refused(E, "layernorm", [y, s], ins=[x.t, g.t, b.t, None], i=[2, 8], f=[1e-5])                        # sum_out without add
    refused(E, "layernorm", [y], ins=[x.t, g.t, b.t, None], i=[-1, 8], f=[1e-5])
    refused(E, "layernorm", [y], ins=[x.t, None, b.t, None], i=[2, 8], f=[1e-5])
    E.op("layernorm", ins=[x.t, g.t, b.t, None], outs=[y.t, None], i=[0, 8], f=[1e-5])                      # rows = 0: succeeds
    torch.cuda.synchronize()
    assert y.untouched(), "layernorm with rows = 0 wrote something"


# -------------------------------------------------------------------------------------------------------------- GEGLU
@pytest.mark.parametrize("Ch", [8, 1280])
def test_geglu(E, Ch):
    """S = 2^-20 (|ref| + |value gate|): value * (0.5 gate (1 + erf)), four fp32 operations and erff.  Gates of +-40 saturate erf
    in fp64 as well: the output is exactly value * gate, or a zero."""
    rows = 3
    x = rnd(40, rows, 2 * Ch) * 1.5
    gates = [0.0, -0.0, 0.5, -0.5, 6.0, -6.0, 40.0, -40.0]
    x[1, Ch:Ch + 8] = torch.tensor(gates, dtype=torch.float64)
    x[1, :8] = torch.tensor([1.5, -2.0, 3.0, 0.75, -1.25, 2.5, 1.75, -3.5], dtype=torch.float64)
    plant(x[2], E.fmt)                                    # values: +-0, +-max, a subnormal (their gates are random)
    x = q16(x, E.fmt)
    xb = in16(x, E.fmt)
    ob = Buf((rows, Ch), E.dt)
    E.op("geglu", ins=[xb.t], outs=[ob.t], i=[rows, Ch])
    torch.cuda.synchronize()
    ob.guards_ok("geglu")
    ref = R.geglu(x)
    mag = (x[:, :Ch] * x[:, Ch:]).abs()
    worst = check16(ob.t, ref, 2.0 ** -20 * (ref.abs() + mag), E.fmt, f"geglu {E.fmt} Ch {Ch}")
    got = ob.t.cpu().double()
    assert got[1, 6].item() == q16(x[1, 6] * 40.0, E.fmt).item() and got[1, 7].item() == 0.0
    assert got[1, 0].item() == 0.0 and got[1, 1].item() == 0.0
    measured(f"geglu Ch={Ch}", E, worst, "2^-20 (|ref| + |value gate|)")


def test_geglu_refusal(E):
    x = in16(rnd(1, 3, 24), E.fmt)
    o = Buf((3, 12), E.dt)
    refused(E, "geglu", [o], ins=[x.t], i=[3, 12])
    refused(E, "geglu", [o], ins=[x.t], i=[0, 8])


# ----------------------------------------------------------------------------------------------------- add, add_padded
@pytest.mark.parametrize("n", [8, 8 * 1000 + 8])
def test_add(E, n):
    """S = 0: the fp32 sum of two 16-bit numbers is exact, so the output is round16(a + b) bit for bit; fp16: max + max = inf."""
    a, b = rnd(50, n) * 3.0, rnd(51, n) * 3.0
    plant(a, E.fmt)
    plant(b, E.fmt)
    b[5] = 7.0                                            # against a's -3 subnormals: a subnormal lost in a normal number
    a, b = q16(a, E.fmt), q16(b, E.fmt)
    ab, bb = in16(a, E.fmt), in16(b, E.fmt)
    ob = Buf((n,), E.dt)
    E.op("add", ins=[ab.t, bb.t], outs=[ob.t], i=[n])
    torch.cuda.synchronize()
    ob.guards_ok("add")
    check_bits(ob.bits(), R.bits16(a + b, E.fmt), f"add {E.fmt} n {n}")
    if E.fmt == "fp16":
        assert ob.t[2].item() == math.inf and ob.t[3].item() == -math.inf
    measured(f"add n={n}", E, 0.0, "0 (bits)")


def test_add_refusal(E):
    a = in16(rnd(1, 16), E.fmt)
    o = Buf((16,), E.dt)
    refused(E, "add", [o], ins=[a.t, a.t], i=[12])
    refused(E, "add", [o], ins=[a.t, None], i=[8])


@pytest.mark.parametrize("shape", [(2, 3, 5, 16), (1, 1, 1, 8)])
def test_add_padded(E, shape):
    """out[dense] = a[dense] + b[padded], S = 0 (bits); b carries the NaN pattern in every border element."""
    n, H, W, C_ = shape
    a, b = rnd(60, *shape) * 2.0, rnd(61, *shape) * 2.0
    plant(a, E.fmt)
    plant(b, E.fmt)
    a, b = q16(a, E.fmt), q16(b, E.fmt)
    ab, bb = in16(a, E.fmt), in16(b, E.fmt, nan_border=True)
    ob = Buf(shape, E.dt)
    E.op("add_padded", ins=[ab.t, bb.t], outs=[ob.t], i=[n, H, W, C_])
    torch.cuda.synchronize()
    ob.guards_ok("add_padded")
    check_bits(ob.bits(), R.bits16(a + b, E.fmt), f"add_padded {E.fmt} {shape}")
    measured(f"add_padded {shape}", E, 0.0, "0 (bits)")


# ----------------------------------------------------------------------------------------------------------- relayout
def _relayout(E, x, in_pad, out_pad, up):
    """x [n, Hi, Wi, C] (dense values); returns (bits of the whole output grid on the CPU, the reference's bits)."""
    n, Hi, Wi, C_ = x.shape
    H, W = (2 * Hi, 2 * Wi) if up else (Hi, Wi)
    xb = in16(x, E.fmt, nan_border=bool(in_pad))
    ob = Buf((n, H + 2, W + 2, C_) if out_pad else (n, H, W, C_), E.dt)
    E.op("relayout", ins=[xb.t], outs=[ob.t], i=[n, H, W, C_, in_pad, out_pad, up])
    torch.cuda.synchronize()
    ob.guards_ok("relayout")
    src = R.to_padded(x, math.nan) if in_pad else x
    want = R.bits16(R.relayout(src, in_pad, out_pad, up), E.fmt)       # zero borders: 0x0000
    return ob.bits().cpu(), want


@pytest.mark.parametrize("case", [(2, 3, 5, 16, 0, 0, 0), (2, 3, 5, 16, 0, 1, 0), (2, 3, 5, 16, 1, 0, 0), (2, 3, 5, 16, 1, 1, 0),
                                  (2, 3, 5, 8, 0, 1, 1), (2, 3, 5, 8, 1, 1, 1), (1, 1, 1, 8, 0, 1, 0), (1, 1, 1, 8, 1, 0, 0),
                                  (1, 1, 1, 8, 1, 1, 0)], ids=lambda c: "x".join(map(str, c)))
def test_relayout(E, case):
    """A pure move: equal bit patterns, 0x0000 in every border element of a padded output, the NaN borders of a padded input
    never read.  (n, Hi, Wi, C, in_pad, out_pad, up): with up the output is (2 Hi) x (2 Wi)."""
    n, Hi, Wi, C_, in_pad, out_pad, up = case
    x = q16(plant(rnd(70, n, Hi, Wi, C_) * 2.0, E.fmt), E.fmt)
    got, want = _relayout(E, x, in_pad, out_pad, up)
    check_bits(got, want, f"relayout {E.fmt} {case}")
    if out_pad:
        H, W = (2 * Hi, 2 * Wi) if up else (Hi, Wi)
        assert bool((got[R.border_mask(n, H, W)] == 0).all())
    measured(f"relayout {case}", E, 0.0, "0 (bits)")


def test_relayout_refusals(E):
    x = in16(rnd(1, 1, 4, 4, 16), E.fmt)
    o = Buf((1, 8, 8, 16), E.dt)
    refused(E, "relayout", [o], ins=[x.t], i=[1, 3, 4, 8, 0, 0, 1])        # up with odd H
    refused(E, "relayout", [o], ins=[x.t], i=[1, 2, 2, 12, 0, 0, 0])       # C % 8
    refused(E, "relayout", [o], ins=[x.t], i=[1, 2, 2, 8, 0, 2, 0])        # a flag that is no flag


# ------------------------------------------------------------------------------------------------------------- im2col
@pytest.mark.parametrize("case", [(2, 5, 7, 16, 1, 0), (2, 5, 7, 16, 2, 0), (1, 3, 2, 8, 1, 1), (1, 1, 1, 8, 1, 0)],
                         ids=lambda c: "x".join(map(str, c)))
def test_im2col3x3(E, case):
    """A pure move: row (img, y, x), column (ky * 3 + kx) * C + c; taps outside the (upsampled) source are 0x0000."""
    n, Hi, Wi, C_, stride, up = case
    if n * Hi * Wi == 1:
        x = q16(rnd(80, n, Hi, Wi, C_).abs() + 1.0, E.fmt)      # no zeros in the one pixel: the eight outer taps are the only zeros
    else:
        x = q16(plant(rnd(80, n, Hi, Wi, C_) * 2.0, E.fmt), E.fmt)
    want = R.bits16(R.im2col3x3(x, stride, bool(up)), E.fmt)
    xb = in16(x, E.fmt)
    ob = Buf(want.shape, E.dt)
    E.op("im2col3x3", ins=[xb.t], outs=[ob.t], i=[n, Hi, Wi, C_, stride, up])
    torch.cuda.synchronize()
    ob.guards_ok("im2col3x3")
    check_bits(ob.bits(), want, f"im2col3x3 {E.fmt} {case}")
    if n * Hi * Wi == 1:
        got = ob.bits().cpu().reshape(9, C_)
        assert bool((got[[0, 1, 2, 3, 5, 6, 7, 8]] == 0).all()) and bool((got[4] != 0).all())
    if stride == 2:
        assert want.shape[0] == n * 3 * 4
    measured(f"im2col3x3 {case}", E, 0.0, "0 (bits)")


def test_im2col_refusals(E):
    x = in16(rnd(1, 1, 4, 4, 8), E.fmt)
    o = Buf((64, 72), E.dt)
    refused(E, "im2col3x3", [o], ins=[x.t], i=[1, 4, 4, 8, 3, 0])          # stride 3
    refused(E, "im2col3x3", [o], ins=[x.t], i=[1, 4, 4, 8, 2, 1])          # up with stride 2
    xf = in32(torch.randn(1, 8, 2, 2))
    o2 = Buf((4, 64), E.dt)
    refused(E, "im2col_in", [o2], ins=[xf.t], i=[1, 8, 2, 2, 64], f=[1.0])  # 9 * Cin > Kp


def test_im2col_in(E):
    """fp32 NCHW -> 16-bit rows of Kp = 64 columns, the input times the VAE's 1 / scaling factor.  S = 2^-24 |ref|: ONE fp32
    product (ref64 uses the same fp32 scale) before the 16-bit rounding.  Columns 36 .. 63 are 0x0000."""
    n, Cin, H, W, Kp = 2, 4, 5, 7, 64
    scale = float(torch.tensor(1 / 0.18215, dtype=F32))
    x = f32v(rnd(90, n, Cin, H, W) * 3.0)
    x.reshape(-1)[:4] = torch.tensor([0.0, -0.0, 1e-30, -2.5e4], dtype=torch.float64)      # -2.5e4 / 0.18215 overflows fp16
    x = f32v(x)
    xb = in32(x)
    ob = Buf((n * H * W, Kp), E.dt)
    E.op("im2col_in", ins=[xb.t], outs=[ob.t], i=[n, Cin, H, W, Kp], f=[scale])
    torch.cuda.synchronize()
    ob.guards_ok("im2col_in")
    ref = R.im2col_in(x, Kp, scale)
    worst = check16(ob.t, ref, 2.0 ** -24 * ref.abs(), E.fmt, f"im2col_in {E.fmt}")
    assert bool((ob.bits()[:, 9 * Cin:] == 0).all()), "columns 36 .. 63 are not exact zeros"
    measured("im2col_in", E, worst, "2^-24 |ref|")


# ------------------------------------------------------------------------------------------------------------- concat
@pytest.mark.parametrize("Ca,Cb", [(8, 16), (320, 8)])
def test_concat(E, Ca, Cb):
    tokens = 7
    a = q16(plant(rnd(100, tokens, Ca), E.fmt), E.fmt)
    b = q16(plant(rnd(101, tokens, Cb), E.fmt), E.fmt)
    ab, bb = in16(a, E.fmt), in16(b, E.fmt)
    ob = Buf((tokens, Ca + Cb), E.dt)
    E.op("concat", ins=[ab.t, bb.t], outs=[ob.t], i=[Ca, Cb, tokens])
    torch.cuda.synchronize()
    ob.guards_ok("concat")
    check_bits(ob.bits(), R.bits16(R.concat(a, b), E.fmt), f"concat {E.fmt} {Ca}+{Cb}")
    measured(f"concat {Ca}+{Cb}", E, 0.0, "0 (bits)")


def test_concat_refusal(E):
    a = in16(rnd(1, 7, 16), E.fmt)
    o = Buf((7, 32), E.dt)
    refused(E, "concat", [o], ins=[a.t, a.t], i=[12, 8, 7])


# ---------------------------------------------------------------------------------------------------------- cast_silu
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_cast_silu(E, n):
    """Without SiLU: S = 0, the bits of round16(in).  With it: S = 2^-15 |ref| (the fast exponential).  silu(-100) is -0 or a tiny
    negative number, whatever the reference rounds to; silu(100) = 100."""
    worst = 0.0
    for silu in (0, 1):
        x = f32v(rnd(110 + n, n) * 4.0)
        v = [-100.0, 100.0, 0.0, -0.0, 1e5, -1e5] + ([1e-40, R.max_finite(E.fmt)] if not silu else [])
        x[:min(n, len(v))] = torch.tensor(v, dtype=torch.float64)[:n]
        x = f32v(x)
        xb = in32(x)
        ob = Buf((n,), E.dt)
        E.op("cast_silu", ins=[xb.t], outs=[ob.t], i=[n, silu])
        torch.cuda.synchronize()
        ob.guards_ok("cast_silu")
        what = f"cast_silu {E.fmt} n {n} silu {silu}"
        if silu:
            ref = R.silu(x)
            worst = max(worst, check16(ob.t, ref, 2.0 ** -15 * ref.abs(), E.fmt, what))
            got0 = ob.t[0].item()
            assert got0 == 0.0 or -1e-30 < got0 < 0.0
        else:
            check_bits(ob.bits(), R.bits16(x, E.fmt), what)
    measured(f"cast_silu n={n}", E, worst, "0 (bits) without SiLU, 2^-15 |ref| with")


# ------------------------------------------------------------------------------------------------------ fp32 <-> NCHW
@pytest.mark.parametrize("in_pad", [0, 1])
@pytest.mark.parametrize("clamp", [0, 1])
def test_tokens_to_nchw(E, in_pad, clamp):
    """fp32 rows of pitch 8 (7 channels; column 7 is NaN, and so is every border row of the padded form) -> NCHW, * 0.5 + 0.5,
    clamped or not: within 2 fp32 ulps of |x mul| + |add|."""
    n, C_, H, W, ld = 2, 7, 3, 5, 8
    x = f32v(rnd(120, n, H, W, ld) * 1.5)
    x.reshape(-1)[:6] = torch.tensor([-3.0, 3.0, -1.0, 1.0, 0.0, -0.0], dtype=torch.float64)      # below 0 and above 1 after 0.5 x + 0.5
    grid = R.to_padded(x) if in_pad else x
    mask = torch.zeros(grid.shape, dtype=torch.bool)
    mask[..., C_:] = True
    if in_pad:
        mask |= R.border_mask(n, H, W)[..., None]
    xb = in32(grid, mask)
    ob = Buf((n, C_, H, W), F32)
    E.op("tokens_to_nchw", ins=[xb.t], outs=[ob.t], i=[n, C_, H, W, ld, clamp, in_pad], f=[0.5, 0.5])
    torch.cuda.synchronize()
    ob.guards_ok("tokens_to_nchw")
    ref, mag = R.tokens_to_nchw(grid.reshape(-1, ld), n, C_, H, W, 0.5, 0.5, bool(clamp), bool(in_pad))
    worst = check32(ob.t, ref, mag, 2, f"tokens_to_nchw pad {in_pad} clamp {clamp}")
    if clamp:
        g = ob.t.cpu()
        assert float(g.min()) == 0.0 and float(g.max()) == 1.0
    measured(f"tokens_to_nchw pad={in_pad} clamp={clamp}", E, worst, "allowed 2, of |x mul| + |add|", U32)


def test_nchw_tokens_round_trip(E):
    """nchw_to_tokens: S = 0, the bits of round16(in); tokens16_to_nchw: the exact values; a round trip of representable values is
    the identity."""
    n, C_, HW = 2, 24, 35
    x = f32v(rnd(130, n, C_, HW) * 3.0)
    x.reshape(-1)[:6] = torch.tensor([0.0, -0.0, 1e5, -1e5, 1e-40, 65519.0], dtype=torch.float64)
    x = f32v(x)
    xb = in32(x)
    tb = Buf((n * HW, C_), E.dt)
    E.op("nchw_to_tokens", ins=[xb.t], outs=[tb.t], i=[n, C_, HW])
    torch.cuda.synchronize()
    tb.guards_ok("nchw_to_tokens")
    check_bits(tb.bits(), R.bits16(R.nchw_to_tokens(x), E.fmt), f"nchw_to_tokens {E.fmt}")
    ob = Buf((n, C_, HW), F32)
    E.op("tokens16_to_nchw", ins=[tb.t], outs=[ob.t], i=[n, C_, HW])
    torch.cuda.synchronize()
    ob.guards_ok("tokens16_to_nchw")
    want = q16(x, E.fmt).to(F32)
    check_bits(ob.bits(), want.view(torch.int32), f"tokens16_to_nchw {E.fmt}")
    t2 = Buf((n * HW, C_), E.dt)
    E.op("nchw_to_tokens", ins=[ob.t], outs=[t2.t], i=[n, C_, HW])
    check_bits(t2.bits(), tb.bits().cpu(), "round trip")
    measured("nchw_to_tokens / tokens16_to_nchw", E, 0.0, "0 (bits)")


@pytest.mark.parametrize("C_", [4, 8])
def test_pointwise_small(E, C_):
    """bias + C products accumulated in fp32: within (C + 2) fp32 ulps of the magnitude sum."""
    n, HW = 2, 35
    scale = float(torch.tensor(1 / 0.18215, dtype=F32))
    x, w, b = f32v(rnd(140, n, C_, HW)), f32v(rnd(141, C_, C_) * 0.5), f32v(rnd(142, C_))
    xb, wb, bb = in32(x), in32(w), in32(b)
    ob = Buf((n, C_, HW), F32)
    E.op("pointwise_small", ins=[xb.t, wb.t, bb.t], outs=[ob.t], i=[n, C_, HW], f=[scale])
    torch.cuda.synchronize()
    ob.guards_ok("pointwise_small")
    ref, mag = R.pointwise_small(x, w, b, scale)
    worst = check32(ob.t, ref, mag, C_ + 2, f"pointwise_small C {C_}")
    measured(f"pointwise_small C={C_}", E, worst, f"allowed {C_ + 2}", U32)


def test_pointwise_small_refusal(E):
    x = in32(torch.randn(1, 9, 4))
    w, b = in32(torch.randn(9, 9)), in32(torch.randn(9))
    o = Buf((1, 9, 4), F32)
    refused(E, "pointwise_small", [o], ins=[x.t, w.t, b.t], i=[1, 9, 4], f=[1.0])


# ------------------------------------------------------------------------------------------------------ cfg, lincomb
def test_cfg(E):
    n = 1000
    e = f32v(rnd(150, 2 * n))
    g = 7.5
    eb = in32(e)
    ob = Buf((n,), F32)
    E.op("cfg", ins=[eb.t], outs=[ob.t], i=[n], f=[g])
    torch.cuda.synchronize()
    ob.guards_ok("cfg")
    ref, mag = R.cfg(e, g)
    measured("cfg", E, check32(ob.t, ref, mag, 2, "cfg"), "allowed 2, of |eu| + |g| (|ec| + |eu|)", U32)


@pytest.mark.parametrize("terms", [1, 2, 4])
@pytest.mark.parametrize("alias", [0, 1])
def test_lincomb(E, terms, alias):
    """The PLMS combination with one, two and four noise terms (the others NULL with coefficient 0), into a buffer of its own and
    -- as the sampling loop calls it on all but its second step -- into ``sample`` itself: within 2 fp32 ulps of the magnitude sum."""
    n = 1000
    coef = {1: (1.0,), 2: (1.5, -0.5), 4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}[terms]
    coef = tuple(float(torch.tensor(c, dtype=F32)) for c in coef)
    cs, ce = float(torch.tensor(1.0123, dtype=F32)), float(torch.tensor(0.0231, dtype=F32))
    sample = f32v(rnd(160, n))
    es = [f32v(rnd(161 + k, n)) for k in range(terms)]
    sb = in32(sample)
    ebs = [in32(e) for e in es]
    ob = sb if alias else Buf((n,), F32)
    E.op("lincomb", ins=[sb.t] + [b.t for b in ebs] + [None] * (4 - terms), outs=[ob.t], i=[n],
         f=[cs, ce] + list(coef) + [0.0] * (4 - terms))
    torch.cuda.synchronize()
    ob.guards_ok("lincomb")
    ref, mag = R.lincomb(sample, cs, ce, es, coef)
    measured(f"lincomb terms={terms} alias={alias}", E, check32(ob.t, ref, mag, 2, f"lincomb {terms} terms alias {alias}"),
             "allowed 2", U32)


# ------------------------------------------------------------------------------------------------------- softmax_rows
@pytest.mark.parametrize("T", [1, 63, 64, 255, 256, 257, 4096])
def test_softmax_rows(E, T):
    """S = 2^-15 |ref| (the fast exponential).  Row 0: scores randn * 30; row 1: one dominant score; row 2: -inf entries, whose
    probability is exactly +0.  Every output row sums (in fp64) to 1 within T * 0.5 ulp16(max p) + 2^-14."""
    rows, scale = 3, float(torch.tensor(1 / math.sqrt(512), dtype=F32))
    s = f32v(rnd(170 + T, rows, T) * 30.0)
    s[1, T // 2] = 4000.0
    s[2, 1::3] = -math.inf
    sb = in32(s)
    ob = Buf((rows, T), E.dt)
    E.op("softmax_rows", ins=[sb.t], outs=[ob.t], i=[rows, T], f=[scale])
    torch.cuda.synchronize()
    ob.guards_ok("softmax_rows")
    ref = R.softmax_rows(s, scale)
    worst = check16(ob.t, ref, 2.0 ** -15 * ref, E.fmt, f"softmax_rows {E.fmt} T {T}")
    got = ob.t.cpu()
    assert bool((got.view(torch.int16)[2, 1::3] == 0).all()), "a -inf score did not get probability +0"
    gd = got.double()
    tol = T * 0.5 * R.ulp16(gd.max(-1).values, E.fmt) + 2.0 ** -14
    assert bool(((gd.sum(-1) - 1.0).abs() <= tol).all()), (gd.sum(-1), tol)
    measured(f"softmax_rows T={T}", E, worst, "2^-15 |ref|")


# ----------------------------------------------------------------------------------------------------- timestep_embed
@pytest.mark.parametrize("dim", [320, 8])
def test_timestep_embed(E, dim):
    """[cos | sin] of t * 10000^(-j / half); S = |angle| 2^-21 absolute: the angle is an fp32 number, and sin / cos of up to ~1000 rad
    inherit its error.  Both rows are equal."""
    worst = 0.0
    for t in (0.0, 1.0, 500.5, 999.0):
        ob = Buf((2, dim), E.dt)
        E.op("timestep_embed", outs=[ob.t], i=[2, dim], f=[t])
        torch.cuda.synchronize()
        ob.guards_ok("timestep_embed")
        row, ang = R.timestep_embed(t, dim)
        got = ob.t.cpu()
        assert torch.equal(got[0].view(torch.int16), got[1].view(torch.int16)), "the two rows differ"
        worst = max(worst, check16(ob.t[0], row, ang.abs() * 2.0 ** -21, E.fmt, f"timestep_embed {E.fmt} dim {dim} t {t}"))
        if t == 0.0:
            assert bool((got[0, :dim // 2] == 1).all()) and bool((got[0, dim // 2:] == 0).all())
    measured(f"timestep_embed dim={dim}", E, worst, "|angle| 2^-21")


# ---------------------------------------------------------------------------------------------------------- transpose
@pytest.mark.parametrize("R_,C_", [(33, 40), (64, 64), (1, 8)])
def test_transpose(E, R_, C_):
    """The 16-bit transpose the VAE attention takes V through: a pure move."""
    x = q16(plant(rnd(180, R_, C_), E.fmt), E.fmt)
    xb = in16(x, E.fmt)
    ob = Buf((C_, R_), E.dt)
    E.op("transpose", ins=[xb.t], outs=[ob.t], i=[R_, C_])
    torch.cuda.synchronize()
    ob.guards_ok("transpose")
    check_bits(ob.bits(), R.bits16(x.t().contiguous(), E.fmt), f"transpose {E.fmt} {R_}x{C_}")
    measured(f"transpose {R_}x{C_}", E, 0.0, "0 (bits)")
