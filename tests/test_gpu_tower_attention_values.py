"""GPU: the softmax VALUES of the tower attention kernels, element by element against fp64: csrc/attention.hip in bf16 and
fp16 through every template of its launcher (packed rows, shared prefixes, both pooled forms), attention_split
(csrc/split.hip, compared with hi + lo of its planes) and attention_f32 (csrc/precise.hip).

The mask witnesses of tests/attn_witness.py stand at the two ends of the softmax (q = 0: every weight 1 / n; a 12-nat
needle: one weight 1) and the parity tests of test_gpu_kernels.py allow a third of the signal; here every output element
must be finite and within the bound of tests/tower_attn_ref.py (derived from the formats and the kernels' arithmetic;
DESIGN.md, "Tower attention: values"), on score profiles with about 100, 5 and 1 keys per softmax and with a 40- to 96-nat
offset that only the subtraction of the row maximum survives; no element is left out.  tests/test_tower_attn_ref.py shows
on the CPU that a correct kernel of this arithmetic meets the bound on exactly these cases and that a softmax scale off by
1 % -- which the parity tests let through -- does not.

The tower kernel writes into a NaN-filled buffer with guard rows (test_gpu_attention_witness._tower_kernel).  Every test
prints one ``[measured]`` line: the worst |got - ref| / bound (allowed 1)."""
import pytest
import torch

import tower_attn_ref as A
from test_gpu_attention_witness import _dev, _tower_kernel

pytestmark = pytest.mark.gpu

CASES = {c.id: c for c in A.gpu_cases()}


def _kernel(eng, c):
    """qkv fp64 [rows, 3 * width] holding values of the format -> the kernel's output [n_out, width] on the CPU."""
    cfg = c.cfg
    if c.precision in ("bf16", "fp16"):
        k = _tower_kernel(eng, cfg, c.precision == "fp16")
        return lambda qkv: k(qkv.float())                                     # exact: the values are the format's
    if c.precision == "split":
        starts, pfx = _dev(cfg.starts_tensor()), _dev(cfg.pfx_tensor())
        return lambda qkv: eng.attention_split_ex(qkv.float().cuda(), cfg.n_seq, cfg.seq_len, cfg.heads, cfg.causal,
                                                  starts=starts, pfx=pfx).cpu()
    return lambda qkv: eng.attention_f32(qkv.float().cuda(), cfg.n_seq, cfg.seq_len, cfg.heads, cfg.causal).cpu()


def _ratio(c, got, ref, bound):
    g = got.double()
    assert g.shape == ref.shape, (c.id, g.shape, ref.shape)
    assert bool(torch.isfinite(g).all()), f"{c.id}: {int((~torch.isfinite(g)).sum())} non-finite outputs where the reference is finite"
    r = (g - ref).abs() / bound
    worst = r.max().item()
    if worst > 1.0:
        i, col = divmod(int(r.argmax()), r.shape[1])
        seq, pos = A.where(c.cfg, i)
        raise AssertionError(f"{c.id}: |got - ref| / bound = {worst:.3f} at output row {i} head {col // A.DH} ({c.profiles[col // A.DH]}) "
                             f"column {col % A.DH}, sequence {seq} position {pos}, template {c.template}: got {g[i, col].item()!r}, "
                             f"ref {ref[i, col].item()!r}, bound {bound[i, col].item():.3e}; {int((r > 1).sum())} of {r.numel()} elements over")
    return worst


def _check(eng, c):
    qkv = c.inputs()
    ref, bound = A.reference(qkv, c.cfg, c.precision)
    assert bool(torch.isfinite(A.to_format(ref, c.precision)).all())
    worst = _ratio(c, _kernel(eng, c)(qkv), ref, bound)
    print(f"[measured] {c.precision} attention values {c.cfg.name} {c.template} {'/'.join(c.profiles)}: "
          f"worst |got - ref| / bound {worst:.3f}")


def _ids(precision):
    return [i for i, c in CASES.items() if c.precision == precision]


@pytest.mark.parametrize("case", _ids("bf16") + _ids("fp16"))
def test_tower_attention_values(gpu_engine, case):
    _check(gpu_engine, CASES[case])


@pytest.mark.parametrize("case", _ids("split"))
def test_split_attention_values(gpu_engine, case):
    _check(gpu_engine, CASES[case])


@pytest.mark.parametrize("case", _ids("fp32"))
def test_f32_attention_values(gpu_engine, case):
    _check(gpu_engine, CASES[case])


@pytest.mark.parametrize("precision", A.PRECISIONS)
def test_attention_values_are_deterministic(gpu_engine, precision):
    c = A.determinism_case(precision)
    qkv = c.inputs()
    ref, bound = A.reference(qkv, c.cfg, c.precision)
    kernel = _kernel(gpu_engine, c)
    one, two = kernel(qkv), kernel(qkv)
    worst = _ratio(c, one, ref, bound)
    assert one.dtype == two.dtype == torch.float32                            # the 16-bit outputs widened exactly; split: hi + lo
    assert torch.equal(one.view(torch.int32), two.view(torch.int32)), f"{c.id}: two runs differ"
    print(f"[measured] {c.precision} attention values determinism: worst |got - ref| / bound {worst:.3f} ({c.id})")
