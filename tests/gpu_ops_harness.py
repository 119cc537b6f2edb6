"""What the isolated-kernel GPU tests share (tests/test_gpu_sd_ops.py, tests/test_gpu_tower_ops.py): buffers of NaN bit
patterns with guard rows around every tensor a kernel sees, the comparisons against an fp64 reference (16-bit results within
0.5 ulp16 + S, fp32 results within fp32 ulps of a magnitude sum, moves as bit patterns) and the all-pairs selection of option
combinations."""
import itertools
import math

import torch

import sd_ops_ref as R

DEV = "cuda:0"
G = 16                                  # guard rows on each side
SENT16, SENT32 = 0x7FA5, 0x7FA5A5A5     # NaN bit patterns in bf16, fp16 and fp32
F32 = torch.float32


def _pairwise(space):
    """Greedy all-pairs selection over the dict of value lists ``space`` (deterministic; as in test_gpu_gemm_contract.py)."""
    names = list(space)
    vals = [space[n] for n in names]
    combos = list(itertools.product(*[range(len(v)) for v in vals]))
    pairs = lambda c: {(i, c[i], j, c[j]) for i in range(len(c)) for j in range(i + 1, len(c))}
    todo = set().union(*(pairs(c) for c in combos))
    rows = []
    while todo:
        best = max(combos, key=lambda c: len(pairs(c) & todo))
        todo -= pairs(best)
        rows.append({n: vals[i][best[i]] for i, n in enumerate(names)})
    return rows

class Buf:
    """A tensor ``t`` of ``shape`` / ``dtype`` inside a sentinel-filled buffer with G guard rows (of the last extent, at
    least 8 elements, rounded to 8 so that ``t`` stays 16-byte aligned) before and after it."""

    def __init__(self, shape, dtype):
        shape = tuple(int(s) for s in shape)
        self.numel = math.prod(shape)
        self.g = G * ((max(shape[-1], 8) + 7) // 8 * 8)
        self.idt, self.sent = (torch.int32, SENT32) if dtype == F32 else (torch.int16, SENT16)
        self.raw = torch.full((self.g + self.numel + self.g,), self.sent, dtype=self.idt, device=DEV)
        self.t = self.raw[self.g:self.g + self.numel].view(dtype).view(shape)

    def bits(self):
        return self.t.view(self.idt)

    def guards_ok(self, what):
        assert bool((self.raw[:self.g] == self.sent).all()), f"{what}: a write into the guard rows before the output"
        assert bool((self.raw[self.g + self.numel:] == self.sent).all()), f"{what}: a write into the guard rows after the output"

    def untouched(self):
        return bool((self.raw == self.sent).all())


def in16(x64, fmt, nan_border=False):
    """x (fp64, CPU) rounded to the format, in a guarded buffer; ``nan_border``: x is [n, H, W, C] and goes into the padded
    layout with the NaN pattern in every border element."""
    if nan_border:
        n, H, W, _ = x64.shape
        bits = R.bits16(R.to_padded(x64), fmt)
        bits[R.border_mask(n, H, W)] = SENT16
    else:
        bits = R.bits16(x64, fmt)
    b = Buf(bits.shape, R.FORMATS[fmt]["dtype"])
    b.bits().copy_(bits)
    return b


def in32(x, nan_where=None):
    """fp32 values in a guarded buffer; ``nan_where``: a bool mask of elements that get the NaN pattern instead."""
    x = x.to(F32)
    b = Buf(x.shape, F32)
    b.t.copy_(x)
    if nan_where is not None:
        b.bits()[nan_where.to(DEV)] = SENT32
    return b

def check16(got, ref64, S, fmt, what):
    """|got - ref| <= 0.5 ulp16(ref) + S where ref rounds to a finite number, got == that inf / a NaN where it does not.
    Returns the worst (|got - ref| - S) in units of ulp16(ref): at most 0.5 (an error in units of the ulp alone says little where
    the reference is next to zero and S is the whole bound)."""
    torch.cuda.synchronize()
    g = got.cpu().double().reshape(ref64.shape)
    r16 = R.round16(ref64, fmt)
    special = ~torch.isfinite(r16)
    if bool(special.any()):
        gs, rs = g[special], r16[special]
        assert torch.equal(torch.isnan(gs), torch.isnan(rs)), f"{what}: NaN where the reference has none (or the reverse)"
        assert torch.equal(gs[~torch.isnan(gs)], rs[~torch.isnan(rs)]), f"{what}: an overflow did not come out as the reference's inf"
    fin = ~special
    assert bool(torch.isfinite(g[fin]).all()), f"{what}: non-finite output where the reference is finite (a border / guard / pitch element read?)"
    err = (g - ref64).abs()[fin]
    ulp = R.ulp16(ref64, fmt)[fin]
    S = S if isinstance(S, float) else S[fin]
    over = err - (0.5 * ulp + S)
    if over.numel() and over.max().item() > 0:
        k = int(over.argmax())
        raise AssertionError(f"{what}: |got - ref| = {err[k].item():.6e} > 0.5 ulp ({0.5 * ulp[k].item():.3e}) + S "
                             f"({(S if isinstance(S, float) else S[k]).__float__():.3e}) at ref {ref64[fin][k].item():.9e}; "
                             f"{int((over > 0).sum())} of {over.numel()} elements over")
    return ((err - S) / ulp).max().item() if err.numel() else 0.0


def check_bits(got_bits, want_bits, what):
    torch.cuda.synchronize()
    g, w = got_bits.cpu().reshape(-1), want_bits.reshape(-1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} bit patterns differ, first at {int(bad.nonzero()[0])}"


def ulp32(x64):
    """fp32 spacing at |x| (normal range)."""
    _, e = torch.frexp(x64.abs().clamp(min=2.0 ** -126))
    return torch.ldexp(torch.ones_like(x64), e.to(torch.int64) - 1 - 23)


U32 = "fp32 ulps of the magnitude sum (S = 0)"


def check32(got, ref64, mag64, ulps, what):
    """fp32 result within ``ulps`` fp32 ulps of the magnitude sum of the reference's terms; returns the worst, in those ulps."""
    torch.cuda.synchronize()
    g = got.cpu().double().reshape(ref64.shape)
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output (a border / guard / pitch element read?)"
    u = ulp32(mag64)
    r = ((g - ref64).abs() / u).max().item()
    assert r <= ulps, f"{what}: {r:.2f} fp32 ulps of the magnitude sum (allowed {ulps})"
    return r
