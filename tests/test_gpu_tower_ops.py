"""GPU: every row kernel of the CLIP towers (csrc/elementwise.hip, backward.hip, the row kernels of split.hip and precise.hip)
ALONE, through tvc_tower_op, against the fp64 / integer references of tests/tower_ops_ref.py (checked on the CPU by
tests/test_tower_ops_ref.py).

Harness (tests/gpu_ops_harness.py, shared with test_gpu_sd_ops.py): every tensor a kernel sees is a view inside a buffer of NaN
bit patterns with guard rows on both sides; pitch gaps, unaddressed rows of strided / indexed tensors and padding columns of
inputs hold the NaN pattern too.  After a launch every input buffer must equal its snapshot bit for bit, and every bit of an
output buffer outside the op's defined output must still be the pattern.

Error rules: 16-bit results |got - ref64| <= 0.5 ulp16(ref64) + S, fp32 results |got - ref64| <= S; S = 0 (bit
patterns) for moves, casts and single chains of fp32 additions; S = 2^-20 M for the LayerNorm family (M: the magnitude sum of
the terms, tower_ops_ref), 2^-15 M behind the fast exponential and reciprocal, C_EXACT M for the erff / expf / IEEE-division
forms (tower_ops_ref.C_EXACT).  Every test prints one ``[measured]`` line: the worst |got - ref| - S in units of the 16-bit ulp (allowed
0.5), or for fp32 results the worst |got - ref| / S (allowed 1)."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import sd_ops_ref as R
import tower_ops_ref as T
from gpu_ops_harness import DEV, F32, SENT16, SENT32, Buf, _pairwise, check16, check_bits
from tower_ops_ref import (C_EXACT, EOT, L2_D, NS, SUB32, TEXT_G, TEXT_SHAPES, VOCAB, _l2_x, _rows_by, _rs_x, _u16, f32v, gelu_erf_mag,
                           make_texts, plant, rnd, rows_of, specials)

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF16 = torch.bfloat16
C_LN = 2.0 ** -20
C_FAST = 2.0 ** -15

@pytest.fixture(scope="module")
def E(pkg):
    eng = pkg.TVCEngine(device=DEV)
    e = SimpleNamespace(eng=eng, lib=pkg._lib, op=lambda name, **kw: eng.tower_op(name, **kw))
    yield e
    eng.close()


# ------------------------------------------------------------------------------------------------------------ helpers


def gb(seed, d):
    return f32v(1.0 + 0.5 * rnd(seed, d)), f32v(0.5 * rnd(seed + 1, d))


class Tensors:
    """The buffers of one launch: inputs are snapshotted and must come back unchanged."""

    def __init__(self):
        self.ins = []

    def keep(self, b):
        self.ins.append((b, b.raw.clone()))
        return b

    def f32(self, x, ld=None, total_rows=None, row_map=None):
        """fp32 values [rows, d] at rows ``row_map`` (default 0 ..) and columns [0, d) of a NaN-filled [total_rows, ld]."""
        x = x.to(F32)
        rows, d = x.shape if x.dim() == 2 else (1, x.numel())
        b = Buf((total_rows or rows, ld or d) if x.dim() == 2 else (x.numel(),), F32)
        if x.dim() == 2:
            b.t[(torch.arange(rows) if row_map is None else row_map).to(DEV), :d] = x.to(DEV)
        else:
            b.t.copy_(x)
        return self.keep(b)

    def b16(self, x64, fmt, ld=None, total_rows=None, row_map=None):
        bits = R.bits16(x64, fmt)
        rows, d = bits.shape
        b = Buf((total_rows or rows, ld or d), R.FORMATS[fmt]["dtype"])
        b.bits()[(torch.arange(rows) if row_map is None else row_map).to(DEV), :d] = bits.to(DEV)
        return self.keep(b)

    def i32(self, vals):
        v = torch.as_tensor(vals, dtype=torch.int32).reshape(-1)
        b = Buf((v.numel(),), F32)
        b.bits().copy_(v)
        return self.keep(b)

    def inputs_unchanged(self, what):
        torch.cuda.synchronize()
        for k, (b, snap) in enumerate(self.ins):
            assert torch.equal(b.raw, snap), f"{what}: input buffer {k} was written"


def ptr32(b):
    return b.bits()


def out_region(b, rows, d, what):
    """The [rows, d] corner of an output buffer [rows, ld]: returns it (CPU) after checking that the guards and every pitch
    element still hold the pattern."""
    torch.cuda.synchronize()
    b.guards_ok(what)
    if b.t.shape[1] > d:
        assert bool((b.bits()[:, d:] == b.sent).all()), f"{what}: a write between the rows of a strided output"
    return b.t[:rows, :d].cpu()


def check_abs(got, ref64, S, what):
    """fp32 result: |got - ref| <= S.  Returns the worst |got - ref| / S."""
    torch.cuda.synchronize()
    g = got.cpu().double().reshape(ref64.shape)
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output (a guard / pitch / unaddressed element read?)"
    err = (g - ref64).abs()
    over = err - S
    if over.max().item() > 0:
        k = int(over.argmax())
        raise AssertionError(f"{what}: |got - ref| = {err.reshape(-1)[k].item():.6e} > S = {S.reshape(-1)[k].item():.3e} at ref "
                             f"{ref64.reshape(-1)[k].item():.9e}; {int((over > 0).sum())} of {over.numel()} elements over")
    return (err / S.clamp(min=1e-300)).max().item()


def f32_bits(x64):
    return x64.to(F32).view(torch.int32)


def measured(family, worst, slack, unit="ulp16 (allowed 0.5)"):
    print(f"[measured] {family}: worst |got - ref| - S = {worst:.4f} {unit}, S = {slack}")


REL = "of S (fp32 result, allowed 1)"


def refused(E, name, watch, code=None, **kw):
    """The call raises with ``code`` (default TVC_E_INVALID) and no bit of the buffers ``watch`` changed."""
    snaps = [o.raw.clone() for o in watch]
    with pytest.raises(E.lib.TVCError) as ei:
        E.op(name, **kw)
    assert ei.value.code == (E.lib.TVC_E_INVALID if code is None else code), (name, kw.get("i"), ei.value)
    torch.cuda.synchronize()
    for o, s in zip(watch, snaps):
        assert torch.equal(o.raw, s), f"{name}: a refused call wrote its output"


# ---------------------------------------------------------------------------------------------------------- LayerNorm
LN_D = [64, 260, 768, 1024]            # one partial piece; pieces 0 and 1 ragged; three pieces; four full pieces
LN_ROWS = [1, 5, 7]                    # one wave alone; a full workgroup plus one; a ragged last workgroup
LN_VARIANTS = _pairwise(dict(addr=("dense", "strided", "idx"), deltas=(0, 1, 2), compact=(0, 1), write_x=(0, 1), xsum=(0, 1),
                             outs=("y", "y32", "both"), fmt=("bf16", "fp16")))


def _addressing(addr, rows, d, seed):
    """(ld, total_rows, row_map or None, row_idx values or None)"""
    if addr == "dense":
        return d, rows, None, None
    if addr == "strided":
        return 3 * d, rows, None, None
    total = rows + 3
    perm = torch.randperm(total, generator=torch.Generator().manual_seed(seed))[:rows]
    return d, total, perm, perm


def _ln_deltas(v, fmt, rows, d, seed):
    """The 16-bit deltas of a variant, with +-65504 (+-65536 in bf16) and a subnormal planted into the first row."""
    big = 65504.0 if fmt == "fp16" else 65536.0
    sub = {"bf16": 2.0 ** -130, "fp16": 2.0 ** -20}[fmt]
    ds = []
    for k in range(v["deltas"]):
        dl = R.round16(rnd(seed + k, rows, d) * 0.5 + 0.25 * k, fmt)
        plant(dl, [big, -big, sub] if k == 0 else [-big, sub, big])
        ds.append(dl)
    return ds


def _ln_slack(xs, g, b, ref, M):
    """max(2^-20 M, twice the deviation of the CPU emulation of the kernel's summation order) per element, and how many
    elements the second term widened, by what factor at most.  It binds only in the row where +65504 and -65504 are planted:
    they cancel in the row's mean, whose fp32 sum carries roundings of size ulp(65504) that M -- built from |mean|, not from the
    mean's terms -- does not see (1.2e-9 against 6.5e-10 at d = 260; any fp32 sum has this).  DESIGN.md 4.9 has the rule."""
    base = C_LN * M
    dev = 2.0 * (T.layernorm_emulated(xs.to(F32), g.to(F32), b.to(F32)).double() - ref).abs()
    wide = dev > base
    return torch.maximum(base, dev), int(wide.sum()), (dev / base)[wide].max().item() if bool(wide.any()) else 1.0


@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("d", LN_D)
def test_layernorm_options(E, d, rows):
    """Every option of layernorm_kernel in an all-pairs selection.  What catches what: the addressing, delta layout
    (compact / x's) and their order by xsum == fp32 (x + d1) + d2 and by y (a wrong row or a NaN); write_x by x's
    addressed rows == that sum, or x == its snapshot without it; y32 by the fp32 rule and y == round16(y32); unaddressed rows and
    pitch elements of x by the whole-buffer comparison."""
    g, b = gb(10 + d, d)
    worst16 = worst32 = 0.0
    widened, factor = 0, 1.0
    for n, v in enumerate(LN_VARIANTS):
        what = f"layernorm d={d} rows={rows} {v}"
        fmt = v["fmt"]
        ld, total, row_map, row_idx = _addressing(v["addr"], rows, d, 50 + n)
        x = rows_of(100 + n, rows, d)
        x[0, 2] = 0.0                                              # meets the planted subnormal delta
        ds = _ln_deltas(v, fmt, rows, d, 200 + 2 * n)
        tt = Tensors()
        xb = tt.f32(x, ld, total, row_map)
        x_before = tt.ins.pop()[1]                                 # x may be written: compared separately below
        ib = tt.i32(row_idx) if row_idx is not None else None
        dbs = [tt.b16(dl, fmt) if v["compact"] else tt.b16(dl, fmt, ld, total, row_map) for dl in ds]
        gbuf, bbuf = tt.f32(g), tt.f32(b)
        yb = Buf((rows, d), R.FORMATS[fmt]["dtype"]) if v["outs"] != "y32" else None
        y32b = Buf((rows, d), F32) if v["outs"] != "y" else None
        sb = Buf((rows, d), F32) if v["xsum"] else None
        E.op("layernorm", ins=[xb.t, None if ib is None else ptr32(ib)] + [db.t for db in dbs] + [None] * (2 - len(dbs)) +
             [gbuf.t, bbuf.t], outs=[None if yb is None else yb.t, None if y32b is None else y32b.t, None if sb is None else sb.t],
             i=[rows, d, ld, v["write_x"], v["compact"], int(fmt == "fp16")])
        tt.inputs_unchanged(what)
        xs = T.fold_deltas(x, *ds)
        ref, M = T.layernorm(xs, g, b, parts=True)
        S, nw, fw = _ln_slack(xs, g, b, ref, M)
        widened, factor = widened + nw, max(factor, fw)
        if yb is not None:
            worst16 = max(worst16, check16(out_region(yb, rows, d, what + " y"), ref, S, fmt, what + " y"))
        if y32b is not None:
            y32 = out_region(y32b, rows, d, what + " y32")
            worst32 = max(worst32, check_abs(y32, ref, S, what + " y32"))
            if yb is not None:
                check_bits(yb.bits(), R.bits16(y32.double(), fmt), what + ": y is not the rounding of y32")
        if sb is not None:
            check_bits(out_region(sb, rows, d, what + " xsum").view(torch.int32), f32_bits(xs), what + " xsum")
        # x: the whole buffer, guards, pitch and unaddressed rows included
        want = x_before.clone()
        if v["write_x"] and ds:
            img = want[xb.g:xb.g + xb.numel].view(total, ld)
            img[(torch.arange(rows) if row_map is None else row_map).to(DEV), :d] = f32_bits(xs).to(DEV)
        assert torch.equal(xb.raw, want), f"{what}: x differs from {'the folded sum' if v['write_x'] and ds else 'its snapshot'}"
    measured(f"layernorm d={d} rows={rows} y", worst16, "2^-20 M")
    measured(f"layernorm d={d} rows={rows} y32", worst32, "2^-20 M", REL)
    print(f"[measured] layernorm d={d} rows={rows}: {widened} of {len(LN_VARIANTS) * rows * d} elements have a slack above 2^-20 M (twice "
          f"the emulated deviation), at most {factor:.2f} times it")


LNS_VARIANTS = _pairwise(dict(addr=("dense", "strided", "idx"), deltas=(0, 1, 2), write_x=(0, 1), outs=("planes", "y32", "both")))


@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("d", LN_D)
def test_ln_split_options(E, d, rows):
    """ln_split_kernel: fp32 deltas in x's layout.  y32 under the fp32 rule; the hi plane under the 16-bit rule; the lo plane
    under the 16-bit rule against ref - hi (that is: hi + lo within the fp32 slack plus lo's own rounding); with both outputs
    hi == bf16(y32) and lo == bf16(y32 - hi) bit for bit."""
    g, b = gb(20 + d, d)
    worst16 = worst32 = 0.0
    for n, v in enumerate(LNS_VARIANTS):
        what = f"ln_split d={d} rows={rows} {v}"
        ld, total, row_map, row_idx = _addressing(v["addr"], rows, d, 70 + n)
        x = rows_of(300 + n, rows, d)
        ds = [f32v(rnd(400 + 2 * n + k, rows, d) * 0.5 + 0.25 * k) for k in range(v["deltas"])]
        tt = Tensors()
        xb = tt.f32(x, ld, total, row_map)
        x_before = tt.ins.pop()[1]
        ib = tt.i32(row_idx) if row_idx is not None else None
        dbs = [tt.f32(dl, ld, total, row_map) for dl in ds]
        gbuf, bbuf = tt.f32(g), tt.f32(b)
        pb = Buf((rows, 2 * d), BF16) if v["outs"] != "y32" else None
        y32b = Buf((rows, d), F32) if v["outs"] != "planes" else None
        E.op("ln_split", ins=[xb.t, None if ib is None else ptr32(ib)] + [db.t for db in dbs] + [None] * (2 - len(dbs)) +
             [gbuf.t, bbuf.t], outs=[None if pb is None else pb.t, None if y32b is None else y32b.t], i=[rows, d, ld, v["write_x"]])
        tt.inputs_unchanged(what)
        xs = T.fold_deltas(x, *ds)
        ref, M = T.layernorm(xs, g, b, parts=True)
        S = C_LN * M
        if y32b is not None:
            y32 = out_region(y32b, rows, d, what + " y32")
            worst32 = max(worst32, check_abs(y32, ref, S, what + " y32"))
        if pb is not None:
            planes = out_region(pb, rows, 2 * d, what + " planes")
            hi, lo = planes[:, :d], planes[:, d:]
            worst16 = max(worst16, check16(hi, ref, S, "bf16", what + " hi"))
            worst16 = max(worst16, check16(lo, ref - hi.double(), S, "bf16", what + " lo"))
            if y32b is not None:
                h64, l64 = T.split_planes(y32.double())
                check_bits(hi.contiguous().view(torch.int16), R.bits16(h64, "bf16"), what + ": hi is not bf16(y32)")
                check_bits(lo.contiguous().view(torch.int16), R.bits16(l64, "bf16"), what + ": lo is not bf16(y32 - hi)")
        want = x_before.clone()
        if v["write_x"] and ds:
            img = want[xb.g:xb.g + xb.numel].view(total, ld)
            img[(torch.arange(rows) if row_map is None else row_map).to(DEV), :d] = f32_bits(xs).to(DEV)
        assert torch.equal(xb.raw, want), f"{what}: x differs from {'the folded sum' if v['write_x'] and ds else 'its snapshot'}"
    measured(f"ln_split d={d} rows={rows} planes", worst16, "2^-20 M")
    measured(f"ln_split d={d} rows={rows} y32", worst32, "2^-20 M", REL)


LNB_VARIANTS = _pairwise(dict(delta=(0, 1), dy=("bf16", "fp32"), dres=("none", "separate", "alias"), dx16=(0, 1),
                              strides=("dense", "x", "out", "both")))


@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("d", LN_D)
def test_layernorm_bwd_options(E, d, rows):
    """Every path of layernorm_bwd_kernel, the DY32 instantiation included.  What catches what: delta (read in x's layout:
    row * x_row_stride) by dx -- a compact read meets the NaN pitch or another row; the three terms of the formula by dx
    against autograd's formula; dres separate / in place by dx; out_row_stride by the skipped elements of dx and dx16 keeping the
    pattern; dx16 == bf16(dx) bit for bit."""
    gamma, _ = gb(30 + d, d)
    worst = 0.0
    for n, v in enumerate(LNB_VARIANTS):
        what = f"layernorm_bwd d={d} rows={rows} {v}"
        xs_ld = 3 * d if v["strides"] in ("x", "both") else d
        o_ld = 3 * d if v["strides"] in ("out", "both") else d
        x = rows_of(500 + n, rows, d)
        delta = R.round16(rnd(600 + n, rows, d) * 0.5, "bf16") if v["delta"] else None
        dy = rnd(700 + n, rows, d) * (1.0 + torch.arange(rows, dtype=F64)[:, None])
        dy = R.round16(dy, "bf16") if v["dy"] == "bf16" else f32v(dy)
        dres = f32v(rnd(800 + n, rows, d)) if v["dres"] != "none" else None
        tt = Tensors()
        xb = tt.f32(x, xs_ld)
        db = tt.b16(delta, "bf16", xs_ld) if delta is not None else None
        dyb = tt.b16(dy, "bf16") if v["dy"] == "bf16" else tt.f32(dy)
        gbuf = tt.f32(gamma)
        dxb = Buf((rows, o_ld), F32)
        rb = None
        if v["dres"] == "separate":
            rb = tt.f32(dres, o_ld)
        elif v["dres"] == "alias":
            dxb.t[:, :d] = dres.to(F32).to(DEV)
        d16b = Buf((rows, o_ld), BF16) if v["dx16"] else None
        E.op("layernorm_bwd", ins=[xb.t, None if db is None else db.t, dyb.t, gbuf.t,
                                   dxb.t if v["dres"] == "alias" else (None if rb is None else rb.t)],
             outs=[dxb.t, None if d16b is None else d16b.t], i=[rows, d, xs_ld, o_ld, int(v["dy"] == "fp32")])
        tt.inputs_unchanged(what)
        ref, M = T.layernorm_bwd(T.fold_deltas(x, delta), dy, gamma, dres, parts=True)
        dx = out_region(dxb, rows, d, what + " dx")
        worst = max(worst, check_abs(dx, ref, C_LN * M, what + " dx"))
        if d16b is not None:
            check_bits(out_region(d16b, rows, d, what + " dx16").view(torch.int16), R.bits16(dx.double(), "bf16"), what + ": dx16 is not bf16(dx)")
    measured(f"layernorm_bwd d={d} rows={rows}", worst, "2^-20 M", REL)


BT = [(1, 2), (3, 5), (2, 17)]


@pytest.mark.parametrize("bt", BT + [(3, 1)], ids=lambda s: f"B{s[0]}T{s[1]}")
@pytest.mark.parametrize("d", LN_D)
def test_assemble_lnpre(E, d, bt):
    B, Tn = bt
    g, b = gb(40 + d, d)
    patch_out = f32v(rnd(41, B, Tn - 1, d) * (1.0 + torch.arange(B, dtype=F64)[:, None, None]) + 0.3)
    cls, pos = f32v(rnd(42, d) + 2.0), f32v(rnd(43, Tn, d) * 0.5 + torch.arange(Tn, dtype=F64)[:, None] * 0.2)
    tt = Tensors()
    pb = tt.f32(patch_out.reshape(-1, d)) if Tn > 1 else None
    cb, pob, gbuf, bbuf = tt.f32(cls), tt.f32(pos), tt.f32(g), tt.f32(b)
    xb = Buf((B * Tn, d), F32)
    what = f"assemble_lnpre d={d} B={B} T={Tn}"
    E.op("assemble_lnpre", ins=[None if pb is None else pb.t, cb.t, pob.t, gbuf.t, bbuf.t], outs=[xb.t], i=[B, Tn, d])
    tt.inputs_unchanged(what)
    ref, M = T.assemble_lnpre(patch_out, cls, pos, g, b, parts=True)
    worst = check_abs(out_region(xb, B * Tn, d, what), ref.reshape(-1, d), C_LN * M.reshape(-1, d), what)
    measured(what, worst, "2^-20 M", REL)


@pytest.mark.parametrize("bt", BT, ids=lambda s: f"B{s[0]}T{s[1]}")
@pytest.mark.parametrize("d", LN_D)
def test_lnpre_bwd(E, d, bt):
    """The class rows of dy hold the NaN pattern: they must not be read."""
    B, Tn = bt
    gamma, _ = gb(44 + d, d)
    patch_out = f32v(rnd(45, B, Tn - 1, d) * (1.0 + torch.arange(B, dtype=F64)[:, None, None]) + 0.3)
    cls, pos = f32v(rnd(46, d)), f32v(rnd(47, Tn, d) * 0.5 + torch.arange(Tn, dtype=F64)[:, None] * 0.2)
    dy = f32v(rnd(48, B, Tn, d))
    tt = Tensors()
    pb, pob, gbuf = tt.f32(patch_out.reshape(-1, d)), tt.f32(pos), tt.f32(gamma)
    live = torch.arange(B * Tn)[torch.arange(B * Tn) % Tn != 0]
    dyb = tt.f32(dy.reshape(-1, d)[live], d, B * Tn, live)
    ob = Buf((B * (Tn - 1), d), BF16)
    what = f"lnpre_bwd d={d} B={B} T={Tn}"
    E.op("lnpre_bwd", ins=[pb.t, pob.t, gbuf.t, dyb.t], outs=[ob.t], i=[B, Tn, d])
    tt.inputs_unchanged(what)
    ref, M = T.lnpre_bwd(patch_out, cls, pos, gamma, dy, parts=True)
    worst = check16(out_region(ob, B * (Tn - 1), d, what), ref.reshape(-1, d), C_LN * M.reshape(-1, d), "bf16", what)
    measured(what, worst, "2^-20 M")


# ------------------------------------------------------------------------------------------------------- stem gathers
GEOMS = [(32, 8, 1), (32, 8, 3), (28, 14, 1), (28, 14, 3), (30, 10, 1), (30, 10, 3), (384, 32, 1)]
GEOM_IDS = [f"{s}p{p}B{b}" for s, p, b in GEOMS]


def _pix(S, B, seed, fmt):
    pix = rnd(seed, B, 3, S, S) + (torch.arange(B * 3, dtype=F64).reshape(B, 3, 1, 1) * 0.37 - 0.5)
    return f32v(plant(pix, specials(fmt) + [1e6, -1e6]))


def _kp(patch):
    return (3 * patch * patch + 63) // 64 * 64


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_im2col(E, geom, fmt):
    """(32, 8) and (28, 14): the LDS form, without and with zero padding columns; (30, 10): image % 4 != 0 and (384, 32): 72 KiB
    of LDS image -- the per-element kernel.  A cast: bit patterns, 0x0000 in the padding."""
    S, patch, B = geom
    Kp = _kp(patch)
    pix = _pix(S, B, 900 + S, fmt)
    tt = Tensors()
    pb = tt.f32(pix.reshape(B * 3 * S, S))
    P = (S // patch) ** 2
    ob = Buf((B * P, Kp), R.FORMATS[fmt]["dtype"])
    what = f"im2col {fmt} {geom}"
    E.op("im2col", ins=[pb.t], outs=[ob.t], i=[B, S, patch, Kp, int(fmt == "fp16")])
    tt.inputs_unchanged(what)
    ob.guards_ok(what)
    check_bits(ob.bits(), R.bits16(T.im2col(pix, patch, Kp), fmt), what)
    measured(what, 0.0, "0 (bit patterns)")


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_im2col_f32_and_col2im(E, geom):
    """Moves: bit patterns.  col2im reads rows of Kp = K + 16 columns whose padding holds the NaN pattern."""
    S, patch, B = geom
    K, P = 3 * patch * patch, (S // patch) ** 2
    pix = _pix(S, B, 950 + S, "fp32")
    tt = Tensors()
    pb = tt.f32(pix.reshape(B * 3 * S, S))
    ob = Buf((B * P, K), F32)
    what = f"im2col_f32 {geom}"
    E.op("im2col_f32", ins=[pb.t], outs=[ob.t], i=[B, S, patch])
    tt.inputs_unchanged(what)
    ob.guards_ok(what)
    cols = T.im2col(pix, patch)
    check_bits(ob.bits(), f32_bits(cols), what)
    tt = Tensors()
    cb = tt.f32(cols, K + 16)
    ib = Buf((B * 3 * S, S), F32)
    what = f"col2im {geom}"
    E.op("col2im", ins=[cb.t], outs=[ib.t], i=[B, S, patch, K + 16])
    tt.inputs_unchanged(what)
    ib.guards_ok(what)
    check_bits(ib.bits(), f32_bits(pix), what)
    measured(f"im2col_f32 / col2im {geom}", 0.0, "0 (bit patterns)", "(bit patterns)")


# ------------------------------------------------------------------------------------------------------- elementwise


@pytest.mark.parametrize("n", NS)
def test_gelu_fwd_and_bwd(E, n):
    """quick_gelu and its gradient behind v_exp_f32 / v_rcp_f32: S = 2^-15 M, M = |ref| forward and |dm| (s + |1.702 u s (1 - s)|)
    backward (the two terms cancel near u = -0.75).  quick_gelu of the most negative bf16 number is an exact -0; its gradient there
    and at the most positive one is 0 and 1 (1.702 u overflows fp32 on the way)."""
    u = _u16(1000 + n, n, "bf16")
    tt = Tensors()
    ub = tt.b16(u.reshape(-1, 8), "bf16")
    ob = Buf((n // 8, 8), BF16)
    E.op("gelu_fwd", ins=[ub.t], outs=[ob.t], i=[n])
    tt.inputs_unchanged("gelu_fwd")
    ref = T.quick_gelu(u)
    got = out_region(ob, n // 8, 8, "gelu_fwd").reshape(-1)
    w1 = check16(got, ref, C_FAST * ref.abs(), "bf16", f"gelu_fwd n={n}")
    assert got.view(torch.int16)[3].item() == -32768, "quick_gelu of the most negative value must be an exact -0"
    dm = plant(R.round16(rnd(1100 + n, n) * 2.0, "bf16"), [8.0, -8.0, 1.0, 1.0, 1.0, R.max_finite("bf16"), 0.0, -0.0])
    tt = Tensors()
    ub = tt.b16(u.reshape(-1, 8), "bf16")
    db = Buf((n // 8, 8), BF16)
    db.bits().copy_(R.bits16(dm.reshape(-1, 8), "bf16"))
    E.op("gelu_bwd", ins=[ub.t], outs=[db.t], i=[n])
    tt.inputs_unchanged("gelu_bwd")
    gr, gm = T.quick_gelu_grad(u, parts=True)
    w2 = check16(out_region(db, n // 8, 8, "gelu_bwd").reshape(-1), dm * gr, C_FAST * dm.abs() * gm, "bf16", f"gelu_bwd n={n}")
    measured(f"gelu_fwd / gelu_bwd n={n}", max(w1, w2), "2^-15 M")


@pytest.mark.parametrize("fmt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("n", NS)
def test_gelu_erf(E, n, fmt):
    """In place.  S = C_EXACT M, M = 0.5 |x| (1 + |erf|) (1 + erf cancels for negative x); fp32 results also get SUB32."""
    if fmt == "fp32":
        x = f32v(plant(rnd(1200 + n, n) * 3.0, specials("fp32")))
        xb = Buf((n // 4, 4), F32)
        xb.t.copy_(x.reshape(-1, 4).to(F32))
        E.op("gelu_erf_f32", outs=[xb.t], i=[n])
        worst = check_abs(out_region(xb, n // 4, 4, "gelu_erf_f32").reshape(-1), R.gelu_erf(x), C_EXACT["gelu_erf"] * gelu_erf_mag(x) + SUB32,
                          f"gelu_erf_f32 n={n}")
        measured(f"gelu_erf_f32 n={n}", worst, "C_EXACT M", REL)
        return
    x = _u16(1300 + n, n, fmt)
    xb = Buf((n // 8, 8), R.FORMATS[fmt]["dtype"])
    xb.bits().copy_(R.bits16(x.reshape(-1, 8), fmt))
    E.op("gelu_erf_16", outs=[xb.t], i=[n, int(fmt == "fp16")])
    worst = check16(out_region(xb, n // 8, 8, "gelu_erf_16").reshape(-1), R.gelu_erf(x), C_EXACT["gelu_erf"] * gelu_erf_mag(x), fmt, f"gelu_erf_16 {fmt} n={n}")
    measured(f"gelu_erf_16 {fmt} n={n}", worst, "C_EXACT M")


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("n", NS)
def test_split_planes(E, n, planes):
    """hi = bf16(x), lo = bf16(x - hi): bit patterns."""
    rows, d = _rows_by(n)
    x = f32v(plant(rnd(1400 + n, rows, d) * 5.0, specials("fp32") + [R.max_finite("bf16"), -R.max_finite("bf16")]))
    tt = Tensors()
    xb = tt.f32(x)
    ob = Buf((rows, planes * d), BF16)
    what = f"split_planes n={n} planes={planes}"
    E.op("split_planes", ins=[xb.t], outs=[ob.t], i=[rows, d, planes])
    tt.inputs_unchanged(what)
    ob.guards_ok(what)
    hi, lo = T.split_planes(x)
    check_bits(ob.bits(), R.bits16(torch.cat([hi, lo][:planes], dim=1), "bf16"), what)
    measured(what, 0.0, "0 (bit patterns)")


@pytest.mark.parametrize("gelu", [0, 1, 2])
@pytest.mark.parametrize("n", NS)
def test_rows_split(E, n, gelu):
    """ld_in > K (NaN beyond K) and Kp > K (zeros in columns K .. Kp of both planes).  gelu 0: bit patterns.  gelu 1 (expf and an
    IEEE division), 2 (erff): the hi plane under the 16-bit rule, the lo plane under it against ref - hi, S = C_EXACT M."""
    rows, K = _rows_by(n)
    Kp, ld = K + 8, K + 4
    x = _rs_x(n)
    tt = Tensors()
    xb = tt.f32(x, ld)
    ob = Buf((rows, 2 * Kp), BF16)
    what = f"rows_split n={n} gelu={gelu}"
    E.op("rows_split", ins=[xb.t], outs=[ob.t], i=[rows, K, Kp, ld, gelu])
    tt.inputs_unchanged(what)
    ob.guards_ok(what)
    got = ob.t.cpu()
    pad = torch.cat([got[:, K:Kp], got[:, Kp + K:]], dim=1).contiguous().view(torch.int16)
    assert bool((pad == 0).all()), f"{what}: padding columns are not 0x0000"
    hi, lo = got[:, :K], got[:, Kp:Kp + K]
    if gelu == 0:
        h64, l64 = T.split_planes(x)
        check_bits(hi.contiguous().view(torch.int16), R.bits16(h64, "bf16"), what + " hi")
        check_bits(lo.contiguous().view(torch.int16), R.bits16(l64, "bf16"), what + " lo")
        measured(what, 0.0, "0 (bit patterns)")
        return
    ref = T.quick_gelu(x) if gelu == 1 else R.gelu_erf(x)
    S = C_EXACT["quick_gelu_exact"] * ref.abs() if gelu == 1 else C_EXACT["gelu_erf"] * gelu_erf_mag(x)
    worst = max(check16(hi, ref, S, "bf16", what + " hi"), check16(lo, ref - hi.double(), S, "bf16", what + " lo"))
    measured(what, worst, "C_EXACT M")


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("D", L2_D)
def test_l2norm_rows(E, D, rows):
    """In place, x / |x| with an IEEE square root and division: S = C_EXACT |ref| + SUB32."""
    x = _l2_x(1600 + D, rows, D)
    xb = Buf((rows, D), F32)
    xb.t.copy_(x.to(F32))
    what = f"l2norm_rows D={D} rows={rows}"
    E.op("l2norm_rows", outs=[xb.t], i=[rows, D])
    ref = T.l2norm(x)
    worst = check_abs(out_region(xb, rows, D, what), ref, C_EXACT["l2norm"] * ref.abs() + SUB32, what)
    measured(what, worst, "C_EXACT |ref|", REL)


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("D", L2_D)
def test_l2norm_bwd(E, D, rows, normalize):
    """normalize 0: a cast of dy (bit patterns; x is NULL).  normalize 1: S = C_EXACT M, M = (|dy| + |y| sum |y dy|) / |x|."""
    x = _l2_x(1700 + D, rows, D)
    dy = f32v(plant(rnd(1800 + D, rows, D), specials("fp32") if not normalize else [0.0, -0.0, 8.0, -8.0]))
    tt = Tensors()
    xb, db = tt.f32(x), tt.f32(dy)
    ob = Buf((rows, D), BF16)
    what = f"l2norm_bwd D={D} rows={rows} normalize={normalize}"
    E.op("l2norm_bwd", ins=[xb.t if normalize else None, db.t], outs=[ob.t], i=[rows, D, normalize])
    tt.inputs_unchanged(what)
    if not normalize:
        ob.guards_ok(what)
        check_bits(ob.bits(), R.bits16(dy, "bf16"), what)
        measured(what, 0.0, "0 (bit patterns)")
        return
    ref, M = T.l2norm_bwd(x, dy, parts=True)
    measured(what, check16(out_region(ob, rows, D, what), ref, C_EXACT["l2norm_bwd"] * M, "bf16", what), "C_EXACT M")


@pytest.mark.parametrize("planes", [1, 2])
def test_gather_rows(E, planes):
    """ld > planes * D (NaN beyond), idx_offset 3, a repeated index and the three zero-row cases: an index below the offset,
    one at R + offset, a negative one.  Bit patterns (hi + lo is one fp32 addition)."""
    D, Rr, off = 100, 6, 3
    ld = planes * D + 12
    vals = plant(R.round16(rnd(1900 + planes, Rr, planes * D) * 4.0, "bf16"), specials("bf16"))
    idx = torch.tensor([3, 8, 2, 9, -1, 5, 8, 4, 3 + Rr - 1], dtype=torch.int32)
    tt = Tensors()
    bb, ib = tt.b16(vals, "bf16", ld), tt.i32(idx)
    ob = Buf((len(idx), D), F32)
    what = f"gather_rows planes={planes}"
    E.op("gather_rows", ins=[bb.t, ptr32(ib)], outs=[ob.t], i=[len(idx), D, Rr, ld, planes, off])
    tt.inputs_unchanged(what)
    ob.guards_ok(what)
    want = T.gather_rows(vals.to(BF16), planes, D, idx, off)
    check_bits(ob.bits(), want.view(torch.int32), what)
    assert bool((want[[2, 3, 4]] == 0).all()) and bool((want[[0, 1]] != 0).any())
    measured(what, 0.0, "0 (bit patterns)", "(bit patterns)")


@pytest.mark.parametrize("form", ["idx", "idx_mul"])
def test_gather_f32_rows(E, form):
    """The index form with a repeated index, and the idx_mul form (row r * T of [*, ld]); ld > d."""
    d, ld, n, Tn = 260, 264, 6, 5
    x = f32v(plant(rows_of(2000, 40, d), specials("fp32")))
    idx = torch.tensor([7, 7, 0, 39, 12, 7], dtype=torch.int32) if form == "idx" else None
    tt = Tensors()
    xb = tt.f32(x, ld)
    ib = tt.i32(idx) if idx is not None else None
    ob = Buf((n, d), F32)
    what = f"gather_f32_rows {form}"
    E.op("gather_f32_rows", ins=[xb.t, None if ib is None else ptr32(ib)], outs=[ob.t], i=[n, d, ld, 0 if idx is not None else Tn])
    tt.inputs_unchanged(what)
    ob.guards_ok(what)
    check_bits(ob.bits(), f32_bits(T.gather_f32_rows(x, idx, Tn, n, d)), what)
    measured(what, 0.0, "0 (bit patterns)", "(bit patterns)")


# ------------------------------------------------------------------------------------- the second grid-stride iteration
# Each capped kernel once with its item count just above cap * 256 (the cap is in its launcher): workgroup 0's thread 0 runs
# a second trip of the loop.  References are vectorised torch conversions (test_sd_ops_ref.py holds round16 equal to them).
ITEMS_16K = 16384 * 256


def _big_u(seed, n, dt):
    return (torch.randn(n, dtype=F32, generator=torch.Generator().manual_seed(seed)) * 3.0).to(dt)


@pytest.mark.parametrize("op", ["gelu_fwd", "gelu_bwd", "gelu_erf_bf16", "gelu_erf_fp16", "gelu_erf_f32"])
def test_second_stride_gelu(E, op):
    """n = 8 (16384 * 256 + 1) 16-bit elements (4 (..) fp32): a strided sample of the first trip and the whole tail beyond
    cap * 256 items under the rules of the small tests."""
    f32op = op == "gelu_erf_f32"
    per = 4 if f32op else 8
    n = per * (ITEMS_16K + 1)
    fmt = "fp16" if op.endswith("fp16") else "bf16"
    dt = F32 if f32op else R.FORMATS[fmt]["dtype"]
    u = _big_u(2100, n, dt)
    pick = torch.cat([torch.arange(0, n - per, 4099), torch.arange(n - per, n)])
    tt = Tensors()
    ub = Buf((n // per, per), dt)
    ub.t.copy_(u.reshape(-1, per))
    us = u[pick].double()
    if op in ("gelu_fwd", "gelu_bwd"):
        tt.keep(ub)
        ob = Buf((n // per, per), dt)
        if op == "gelu_bwd":
            dm = _big_u(2101, n, dt)
            ob.t.copy_(dm.reshape(-1, per))
        E.op(op, ins=[ub.t], outs=[ob.t], i=[n])
        tt.inputs_unchanged(op)
        if op == "gelu_fwd":
            ref = T.quick_gelu(us)
            S = C_FAST * ref.abs()
        else:
            gr, gm = T.quick_gelu_grad(us, parts=True)
            ref, S = dm[pick].double() * gr, C_FAST * dm[pick].double().abs() * gm
    else:
        ob = ub
        E.op("gelu_erf_f32" if f32op else "gelu_erf_16", outs=[ob.t], i=[n] if f32op else [n, int(fmt == "fp16")])
        ref, S = R.gelu_erf(us), C_EXACT["gelu_erf"] * gelu_erf_mag(us)
    torch.cuda.synchronize()
    ob.guards_ok(op)
    got = ob.t.reshape(-1)[pick.to(DEV)].cpu()
    if f32op:
        measured(f"second stride {op}", check_abs(got, ref, S + SUB32, op), "C_EXACT M", REL)
    else:
        measured(f"second stride {op}", check16(got, ref, S, fmt, op), "2^-15 M" if "erf" not in op else "C_EXACT M")


def test_second_stride_split_planes(E):
    d, rows = 8, ITEMS_16K // 2 + 1                      # rows * d / 4 = cap * 256 + 2 items
    x = torch.randn(rows, d, dtype=F32, generator=torch.Generator().manual_seed(2200)) * 5.0
    xb = Buf((rows, d), F32)
    xb.t.copy_(x)
    snap = xb.raw.clone()
    ob = Buf((rows, 2 * d), BF16)
    E.op("split_planes", ins=[xb.t], outs=[ob.t], i=[rows, d, 2])
    torch.cuda.synchronize()
    assert torch.equal(xb.raw, snap)
    ob.guards_ok("split_planes")
    hi = x.to(BF16)
    lo = (x - hi.float()).to(BF16)
    check_bits(ob.bits(), torch.cat([hi, lo], dim=1).view(torch.int16), "second stride split_planes")
    measured("second stride split_planes", 0.0, "0 (bit patterns)")


def test_second_stride_rows_split(E):
    K, Kp, ld = 4, 16, 8
    rows = 32768 * 256 // (Kp // 4) + 1                  # rows * Kp / 4 = cap * 256 + 4 items (cap 32768)
    x = torch.randn(rows, K, dtype=F32, generator=torch.Generator().manual_seed(2300)) * 5.0
    xb = Buf((rows, ld), F32)
    xb.t[:, :K] = x.to(DEV)
    snap = xb.raw.clone()
    ob = Buf((rows, 2 * Kp), BF16)
    E.op("rows_split", ins=[xb.t], outs=[ob.t], i=[rows, K, Kp, ld, 0])
    torch.cuda.synchronize()
    assert torch.equal(xb.raw, snap)
    ob.guards_ok("rows_split")
    hi = x.to(BF16)
    want = torch.zeros((rows, 2 * Kp), dtype=torch.int16)
    want[:, :K] = hi.view(torch.int16)
    want[:, Kp:Kp + K] = (x - hi.float()).to(BF16).view(torch.int16)
    check_bits(ob.bits(), want, "second stride rows_split")
    measured("second stride rows_split", 0.0, "0 (bit patterns)")


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_second_stride_im2col_per_element(E, fmt):
    S, patch, Kp = 10, 2, 16                             # image % 4 != 0: the per-element kernel (cap 8192); 50 items per image
    B = 8192 * 256 // 50 + 1
    dt = R.FORMATS[fmt]["dtype"]
    pix = torch.randn(B, 3, S, S, dtype=F32, generator=torch.Generator().manual_seed(2400))
    pb = Buf((B * 3 * S, S), F32)
    pb.t.copy_(pix.reshape(-1, S))
    snap = pb.raw.clone()
    ob = Buf((B * 25, Kp), dt)
    E.op("im2col", ins=[pb.t], outs=[ob.t], i=[B, S, patch, Kp, int(fmt == "fp16")])
    torch.cuda.synchronize()
    assert torch.equal(pb.raw, snap)
    ob.guards_ok("im2col")
    check_bits(ob.bits(), T.im2col(pix, patch, Kp).to(dt).view(torch.int16), f"second stride im2col {fmt}")
    measured(f"second stride im2col {fmt}", 0.0, "0 (bit patterns)")


def test_second_stride_im2col_f32_and_col2im(E):
    S, patch = 32, 8
    B = ITEMS_16K // (3 * S * S) + 1                     # B * 3 * S * S items, cap 16384 for both kernels
    K = 3 * patch * patch
    pix = torch.randn(B, 3, S, S, dtype=F32, generator=torch.Generator().manual_seed(2500))
    pb = Buf((B * 3 * S, S), F32)
    pb.t.copy_(pix.reshape(-1, S))
    snap = pb.raw.clone()
    ob = Buf((B * 16, K), F32)
    E.op("im2col_f32", ins=[pb.t], outs=[ob.t], i=[B, S, patch])
    torch.cuda.synchronize()
    assert torch.equal(pb.raw, snap)
    ob.guards_ok("im2col_f32")
    cols = T.im2col(pix, patch)
    check_bits(ob.bits(), cols.view(torch.int32), "second stride im2col_f32")
    cb = Buf((B * 16, K + 16), F32)
    cb.t[:, :K] = cols.to(DEV)
    snap = cb.raw.clone()
    ib = Buf((B * 3 * S, S), F32)
    E.op("col2im", ins=[cb.t], outs=[ib.t], i=[B, S, patch, K + 16])
    torch.cuda.synchronize()
    assert torch.equal(cb.raw, snap)
    ib.guards_ok("col2im")
    check_bits(ib.bits(), pix.view(torch.int32), "second stride col2im")
    measured("second stride im2col_f32 / col2im", 0.0, "0 (bit patterns)", "(bit patterns)")


def test_second_stride_gather_f32_rows(E):
    d, ld = 64, 68
    n = 8192 * 256 // (d // 4) + 1                       # n * d / 4 = cap * 256 + 16 items (cap 8192)
    x = rows_of(2600, 97, d)
    idx = torch.randint(0, 97, (n,), generator=torch.Generator().manual_seed(2601), dtype=torch.int32)
    tt = Tensors()
    xb, ib = tt.f32(x, ld), tt.i32(idx)
    ob = Buf((n, d), F32)
    E.op("gather_f32_rows", ins=[xb.t, ptr32(ib)], outs=[ob.t], i=[n, d, ld, 0])
    tt.inputs_unchanged("gather_f32_rows")
    ob.guards_ok("gather_f32_rows")
    check_bits(ob.bits(), T.gather_f32_rows(x.to(F32), idx, 0, n, d).view(torch.int32), "second stride gather_f32_rows")
    measured("second stride gather_f32_rows", 0.0, "0 (bit patterns)", "(bit patterns)")


# ------------------------------------------------------------------------------------------------------ text kernels


@pytest.mark.parametrize("G", TEXT_G)
@pytest.mark.parametrize("shape", TEXT_SHAPES, ids=lambda s: f"ctx{s[0]}n{s[1]}")
def test_text_lens_scan(E, shape, G):
    """Exact equality with the integer reference: lengths by the first maximum, shared prefixes bounded by both lengths, the
    exclusive scan across chunks of 1024 texts (n_text 1025 and 2500 carry), the maximum length, the base rows."""
    ctx, n_text = shape
    tok = make_texts(n_text, ctx, G, 3000 + ctx + n_text)
    starts, pfx, lens = T.text_lens_scan(tok, G)
    if G and ctx >= 63 and n_text >= 1024:                 # the planted kinds are all there
        own = [starts[n + 1] - starts[n] for n in range(n_text)]
        base_len = [lens[n // G * G] for n in range(n_text)]
        assert any(o == 0 for o in own) and any(pfx[n] == 0 and n % G for n in range(n_text))
        assert any(pfx[n] == base_len[n] < lens[n] for n in range(n_text)) and any(lens[n] < base_len[n] for n in range(n_text))
        mis = [next((t for t in range(ctx) if tok[n][t] != tok[n // G * G][t]), ctx) for n in range(n_text)]
        assert any(pfx[n] == lens[n] < min(mis[n], base_len[n]) for n in range(n_text)), "no text whose own length caps its prefix"
    tt = Tensors()
    tb = tt.i32(torch.tensor(tok, dtype=torch.int32))
    sb = Buf((n_text + 2,), F32)
    pb = Buf((2 * n_text,), F32) if G else None
    wb = None if G else Buf((n_text,), F32)
    what = f"text_lens_scan ctx={ctx} n_text={n_text} G={G}"
    E.op("text_lens_scan", ins=[ptr32(tb)], outs=[ptr32(sb), None if pb is None else ptr32(pb), None if wb is None else ptr32(wb)],
         i=[n_text, ctx, G])
    tt.inputs_unchanged(what)
    for b in (sb, pb, wb):
        if b is not None:
            b.guards_ok(what)
    check_bits(sb.bits(), torch.tensor(starts, dtype=torch.int32), what + " starts")
    if G:
        check_bits(pb.bits(), torch.tensor(pfx, dtype=torch.int32), what + " pfx")
    measured(what, 0.0, "0 (integers)", "(exact)")


@pytest.mark.parametrize("mode", ["dense", "packed", "pfx2", "pfx8"])
@pytest.mark.parametrize("d", [64, 260])
@pytest.mark.parametrize("shape", [(1, 5), (63, 9), (64, 5), (65, 12), (77, 21)], ids=lambda s: f"ctx{s[0]}n{s[1]}")
def test_text_embed(E, shape, d, mode):
    """x rows = tok_emb[clamp(id)] + pos[t], one fp32 addition: bit patterns over the WHOLE row buffer -- packed rows no text owns
    keep the NaN pattern -- and eot_row exactly.  Ids -1 and vocab are planted (they clamp to 0 and vocab - 1; vocab is also a
    maximum, so it moves that text's length).  starts / pfx come from the integer reference, not from the other kernel."""
    ctx, n_text = shape
    G = {"pfx2": 2, "pfx8": 8}.get(mode, 0)                # 9, 5, 12 and 21 texts: the last group is ragged
    tok = make_texts(n_text, ctx, G, 4000 + ctx)
    tok[0][0] = -1
    tok[n_text - 1][ctx // 2] = VOCAB
    emb = (rnd(4100, VOCAB, d) + torch.arange(VOCAB, dtype=F64)[:, None] * 0.1).to(F32)
    pos = (rnd(4101, ctx, d) * 0.3 + torch.arange(ctx, dtype=F64)[:, None] * 0.05).to(F32)
    starts, pfx, lens = T.text_lens_scan(tok, G) if mode != "dense" else (None, None, None)
    rows, eot = T.text_embed(tok, emb, pos, VOCAB, starts, pfx)
    tt = Tensors()
    tb, eb, pb = tt.i32(torch.tensor(tok, dtype=torch.int32)), tt.f32(emb), tt.f32(pos)
    stb = tt.i32(starts) if starts is not None else None
    pfb = tt.i32(pfx) if pfx is not None else None
    xb = Buf((n_text * ctx, d), F32)
    ob = Buf((n_text,), F32)
    what = f"text_embed ctx={ctx} n_text={n_text} d={d} {mode}"
    E.op("text_embed", ins=[ptr32(tb), eb.t, pb.t, None if stb is None else ptr32(stb), None if pfb is None else ptr32(pfb)],
         outs=[xb.t, ptr32(ob)], i=[n_text, ctx, d, VOCAB])
    tt.inputs_unchanged(what)
    xb.guards_ok(what)
    ob.guards_ok(what)
    want = torch.full((n_text * ctx, d), SENT32, dtype=torch.int32)
    for r, v in rows.items():
        want[r] = v.view(torch.int32)
    if mode != "dense":
        assert len(rows) == starts[n_text]
    if G:                                                  # a text with no own rows: its EOT position among its base's rows
        assert all(eot[n] == starts[n // G * G] + lens[n] - 1 for n in range(n_text) if starts[n + 1] == starts[n])
    check_bits(xb.bits(), want, what + " x")
    check_bits(ob.bits(), torch.tensor(eot, dtype=torch.int32), what + " eot_row")
    measured(what, 0.0, "0 (bit patterns)", "(bit patterns)")


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals(E):
    """What the entry refuses (TVC_E_INVALID) and what a launcher rejects (TVC_E_HIP): nothing is launched, no output bit
    changes."""
    INV, HIP = E.lib.TVC_E_INVALID, E.lib.TVC_E_HIP
    d, rows = 64, 5
    tt = Tensors()
    x, g, b = tt.f32(rows_of(1, rows, 3 * d)), tt.f32(gb(2, d)[0]), tt.f32(gb(2, d)[1])
    dl = tt.b16(R.round16(rnd(3, rows, 3 * d), "bf16"), "bf16")
    y, y32 = Buf((rows, d), BF16), Buf((rows, d), F32)
    outs = [x, y, y32]
    ln = lambda ins, o, i, code=INV: refused(E, "layernorm", outs, code, ins=ins, outs=o, i=i)
    ok_ins = [x.t, None, dl.t, None, g.t, b.t]
    ln([None] + ok_ins[1:], [y.t, y32.t], [rows, d, d, 1, 0, 0])                                 # NULL x
    ln(ok_ins, [None, None], [rows, d, d, 1, 0, 0])                                              # neither y nor y32
    ln([x.t.reshape(-1)[1:]] + ok_ins[1:], [y.t, y32.t], [rows, d, d, 1, 0, 0])                  # x at 4 bytes
    ln(ok_ins[:2] + [dl.t.reshape(-1)[2:]] + ok_ins[3:], [y.t, y32.t], [rows, d, d, 1, 0, 0])    # delta at 4 bytes
    ln(ok_ins, [y.t.reshape(-1)[2:], None], [rows, d, d, 1, 0, 0])                               # y at 4 bytes
    ln(ok_ins, [y.t, y32.t], [rows, d, d + 2, 1, 0, 0])                                          # x_row_stride % 4
    ln(ok_ins, [y.t, y32.t], [rows, d, d - 4, 1, 0, 0])                                          # x_row_stride < d
    ln(ok_ins, [y.t, y32.t], [0, d, d, 1, 0, 0])                                                 # rows = 0
    ln(ok_ins, [y.t, y32.t], [1 << 22, 1024, 1024, 1, 0, 0])                                     # rows * d leaves int32
    ln(ok_ins, [y.t, y32.t], [rows, d, d, 2, 0, 0])                                              # a flag of 2
    ln(ok_ins, [y.t, y32.t], [rows, 62, 64, 1, 0, 0], HIP)                                       # d % 4: the launcher's
    ln(ok_ins, [y.t, y32.t], [1, 1028, 1028, 1, 0, 0], HIP)                                      # d > 1024
    dx, dx16 = Buf((rows, d), F32), Buf((rows, d), BF16)
    bw = lambda ins, o, i, code=INV: refused(E, "layernorm_bwd", [dx, dx16], code, ins=ins, outs=o, i=i)
    bw([x.t, None, dl.t, g.t, None], [None, dx16.t], [rows, d, d, d, 0])                         # NULL dx
    bw([x.t, None, dl.t.reshape(-1)[4:], g.t, None], [dx.t, dx16.t], [rows, d, d, d, 1])         # fp32 dy at 8 bytes
    bw([x.t, None, dl.t, g.t, None], [dx.t, dx16.t], [rows, d, d, d + 2, 0])                     # out_row_stride % 4
    bw([x.t, None, dl.t, g.t, None], [dx.t, dx16.t], [rows, 1028, 1028, 1028, 0], HIP)
    o16, o32 = Buf((64, 64), BF16), Buf((64, 64), F32)
    ob = [o16, o32]
    refused(E, "im2col", ob, ins=[x.t], outs=[o16.t], i=[1, 30, 8, 192, 0])                      # image % patch
    refused(E, "im2col", ob, ins=[x.t], outs=[o16.t], i=[1, 32, 8, 190, 0])                      # Kp < K
    refused(E, "im2col", ob, ins=[x.t], outs=[o16.t], i=[1, 32, 8, 196, 0])                      # Kp % 8
    refused(E, "im2col", ob, ins=[x.t.reshape(-1)[1:]], outs=[o16.t], i=[1, 32, 8, 192, 0])      # pix at 4 bytes, image % 4 == 0
    refused(E, "im2col_f32", ob, ins=[x.t], outs=[o32.t], i=[1, 30, 8])
    refused(E, "col2im", ob, ins=[x.t], outs=[o32.t], i=[1, 30, 8, 192])
    refused(E, "col2im", ob, ins=[x.t], outs=[o32.t], i=[0, 32, 8, 192])
    refused(E, "lnpre_bwd", ob, ins=[x.t, x.t, g.t, x.t], outs=[o16.t], i=[2, 1, d])             # T = 1: no patch rows
    refused(E, "assemble_lnpre", ob, ins=[None, x.t, x.t, g.t, b.t], outs=[o32.t], i=[2, 2, d])  # NULL patch_out with T > 1
    refused(E, "gelu_fwd", ob, ins=[dl.t], outs=[o16.t.reshape(-1)[4:]], i=[64])                 # out at 8 bytes
    refused(E, "gelu_fwd", ob, HIP, ins=[dl.t], outs=[o16.t], i=[12])                            # n % 8
    refused(E, "gelu_bwd", ob, HIP, ins=[dl.t], outs=[o16.t], i=[12])
    refused(E, "gelu_erf_16", ob, HIP, outs=[o16.t], i=[12, 0])
    refused(E, "gelu_erf_f32", ob, HIP, outs=[o32.t], i=[10])
    refused(E, "gelu_erf_f32", ob, outs=[o32.t], i=[-4])
    refused(E, "l2norm_rows", ob, outs=[o32.t], i=[4, 0])
    refused(E, "l2norm_bwd", ob, ins=[None, x.t], outs=[o16.t], i=[4, 8, 1])                     # NULL x with normalize
    refused(E, "ln_split", ob, ins=[x.t, None, None, None, g.t, b.t], outs=[None, None], i=[rows, d, d, 0])
    refused(E, "rows_split", ob, ins=[x.t], outs=[o16.t], i=[4, 8, 8, 6, 0])                     # ld_in < K
    refused(E, "rows_split", ob, ins=[x.t], outs=[o16.t], i=[4, 8, 8, 8, 3])                     # gelu = 3
    refused(E, "rows_split", ob, HIP, ins=[x.t], outs=[o16.t], i=[4, 8, 4, 8, 0])                # Kp < K: the launcher's
    refused(E, "split_planes", ob, ins=[x.t], outs=[o16.t], i=[4, 8, 3])                         # planes = 3
    refused(E, "split_planes", ob, ins=[x.t], outs=[o16.t], i=[4, 8, (1 << 32) + 1])             # planes beyond int32
    refused(E, "gather_rows", ob, ins=[dl.t, ptr32(x)], outs=[o32.t], i=[4, 8, 4, 12, 2, 0])     # ld < planes * D
    refused(E, "gather_rows", ob, ins=[dl.t, ptr32(x)], outs=[o32.t], i=[4, 8, 4, 16, 3, 0])     # planes = 3
    refused(E, "gather_f32_rows", ob, ins=[x.t, None], outs=[o32.t], i=[4, 8, 10, 1])            # ld % 4
    refused(E, "text_lens_scan", ob, ins=[ptr32(x)], outs=[o32.t, None, None], i=[4, 8, 0])      # neither pfx nor the scratch
    refused(E, "text_lens_scan", ob, HIP, ins=[ptr32(x)], outs=[o32.t, o32.t[8:], None], i=[4, 8, 1])      # G < 2 with pfx
    refused(E, "text_embed", ob, ins=[ptr32(x), x.t, x.t, None, ptr32(x)], outs=[o32.t, o32.t[32:]], i=[2, 4, 8, 16])      # pfx without starts
    a = E.lib.TowerOpArgs()
    assert E.eng.lib.tvc_tower_op(E.eng.handle, 99, C.byref(a), None) == INV                     # unknown op
    assert E.eng.lib.tvc_tower_op(E.eng.handle, -1, C.byref(a), None) == INV
    assert E.eng.lib.tvc_tower_op(E.eng.handle, 0, None, None) == INV                            # NULL arguments
    tt.inputs_unchanged("refusals")
    for o in (y, y32, dx, dx16, o16, o32):
        assert o.untouched()
