"""GPU: the VALUES of the streaming attention (csrc/sd_attention.hip), element by element against fp64, on inputs that make
its online softmax work: the lazy reference maximum moves (rise3 / rise5 / rise9: every third, second, every key tile),
stays just below and just above its 2^8 threshold (threshold), falls so that late probabilities vanish (fall9), or jumps
at the sample's last key (late_spike) -- with moving, flat and falling rows inside every 16-query block.

Every output element must be finite and within the bound of tests/sd_attn_ref.py (derived from the formats and the
kernel's arithmetic; DESIGN.md, "Streaming attention: values"); no element is left out.  tests/test_sd_attn_ref.py shows
on the CPU that a correct tile loop meets this bound on exactly these cases, that the cases reach the rescale branch
(the random inputs of test_gpu_sd.py never do after tile 0), and which defects of the bookkeeping each one catches.

Inputs sit in buffers of NaN bit patterns with guard rows (gpu_ops_harness.Buf); every second case also writes into such
a buffer through the separate-stride entry point and must leave the guards alone.  Every test prints one ``[measured]``
line: the worst |got - ref| / bound (allowed 1)."""
import importlib
from types import SimpleNamespace

import pytest
import torch

import sd_attn_ref as A
import sd_ops_ref as R
from attn_witness import SD_HEAD_DIMS
from gpu_ops_harness import DEV, SENT16, Buf, in16
from test_gpu_attention_witness import _shape

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def E(request, pkg):
    """One engine without weights per 16-bit format: bf16 is the handle's default, fp16 is TVC_OPT_SD_PRECISION = 1."""
    sdm = importlib.import_module(pkg.__name__ + ".sd_model")
    eng = pkg.TVCEngine(device=DEV)
    if request.param == "fp16":
        eng.set_sd_precision("fp16")
    yield SimpleNamespace(eng=eng, fmt=request.param, dt=R.FORMATS[request.param]["dtype"], sa=sdm.streaming_attention)
    eng.close()


def _padded(x64, fmt, pad):
    """x [rows, C] in a guarded buffer of [rows, C + pad]; the pad columns keep the NaN pattern."""
    b = Buf((x64.shape[0], x64.shape[1] + pad), R.FORMATS[fmt]["dtype"])
    b.bits()[:, :x64.shape[1]] = R.bits16(x64, fmt).to(DEV)
    return b


def _run(E, c, q, k, v, pads=None):
    """The kernel's output as a CPU tensor of the format, [n * Tq, C].  pads = None: the one-stride entry point on guarded
    inputs.  pads = (pq, pk, pv, po): the separate-stride one, rows padded by that many NaN columns, into a guarded output
    whose pad columns and guard rows must keep their bits."""
    C = c.heads * c.dh
    if pads is None:
        bufs = [in16(t, c.fmt) for t in (q, k, v)]
        out = E.sa(E.eng, *(b.t for b in bufs), c.n, c.heads)
        torch.cuda.synchronize()
        return out.cpu()
    bufs = [_padded(t, c.fmt, p) for t, p in zip((q, k, v), pads)]
    ob = Buf((c.n * c.Tq, C + pads[3]), E.dt)
    E.sa(E.eng, *(b.t for b in bufs), c.n, c.heads, ld=tuple(C + p for p in pads), dh=c.dh, out=ob.t)
    torch.cuda.synchronize()
    ob.guards_ok(c.id)
    assert bool((ob.bits()[:, C:] == SENT16).all()), f"{c.id}: the output's pad columns were written"
    return ob.t[:, :C].contiguous().cpu()


def _ratio(c, got, ref, bound):
    g = got.double()
    assert bool(torch.isfinite(g).all()), f"{c.id}: {int((~torch.isfinite(g)).sum())} non-finite outputs where the reference is finite"
    r = (g - ref).abs() / bound
    worst = r.max().item()
    if worst > 1.0:
        i, col = divmod(int(r.argmax()), r.shape[1])
        b, row, h = i // c.Tq, i % c.Tq, col // c.dh
        raise AssertionError(f"{c.id}: |got - ref| / bound = {worst:.3f} at sample {b} query {row} (class {(1, 0, -1)[row % 3]}) head {h} "
                             f"column {col % c.dh}: got {g[i, col].item()!r}, ref {ref[i, col].item()!r}, bound {bound[i, col].item():.3e}; "
                             f"{int((r > 1).sum())} of {r.numel()} elements over")
    return worst


def _check(E, c, pads=None):
    assert c.fmt == E.fmt
    q, k, v = c.inputs()
    ref, bound = A.reference(q, k, v, c.n, c.heads, c.fmt)
    assert bool(torch.isfinite(R.round16(ref, c.fmt)).all())
    return _ratio(c, _run(E, c, q, k, v, pads), ref, bound)


@pytest.mark.parametrize("dh", SD_HEAD_DIMS)
def test_streaming_attention_values_every_head_dim(E, dh):
    """Shape 1 (4 waves x 1 block; n * heads = 6, Tq = 65): every profile against a Tk of 65 / 129 / 193 / 320 / 449 / 1088
    (2 / 3 / 4 / 5 / 8 / 17 key tiles), rotated by the head dim."""
    cases = A.every_head_dim_cases(dh, E.fmt)
    assert all(_shape(c.n * c.heads, c.Tq, c.dh) == 1 for c in cases)
    worst = {c.id: _check(E, c, pads=(0, 0, 0, 0) if j % 2 else None) for j, c in enumerate(cases)}
    w = max(worst, key=worst.get)
    print(f"[measured] streaming attention values {E.fmt} dh {dh}: worst |got - ref| / bound {worst[w]:.3f} ({w})")


@pytest.mark.parametrize("Tq,shape", A.WIDE_TQ)
@pytest.mark.parametrize("dh", A.WIDE_DH)
def test_streaming_attention_values_wide_workgroups(E, dh, Tq, shape):
    """n * heads = 256 items: 4 waves x 2 blocks at Tq = 130, 8 waves x 2 blocks at Tq = 257 (one staging register set at
    head dim 40, two at 80); rise5 and threshold over 4 key tiles, the last of one key."""
    worst = {}
    for c in A.wide_cases(dh, E.fmt, Tq):
        assert _shape(c.n * c.heads, c.Tq, c.dh) == shape
        worst[c.id] = _check(E, c)
    w = max(worst, key=worst.get)
    print(f"[measured] streaming attention values {E.fmt} dh {dh} shape {shape}: worst |got - ref| / bound {worst[w]:.3f} ({w})")


def test_streaming_attention_values_with_separate_strides(E):
    """ldq != ldk != ldv != ldo (rows padded by 8 / 16 / 24 / 4 columns); the q / k / v pad columns hold NaN."""
    c = A.stride_case(E.fmt)
    worst = _check(E, c, pads=A.PADS)
    print(f"[measured] streaming attention values {E.fmt} separate strides: worst |got - ref| / bound {worst:.3f} ({c.id})")


def test_streaming_attention_contains_non_finite_inputs(E):
    """One NaN key and one +inf value row in ONE (sample, head): that item's outputs are non-finite wherever the fp64
    reference is, every other (sample, head) has the bits of the clean run."""
    c = A.containment_case(E.fmt)
    q, k, v = c.inputs()
    clean = _run(E, c, q, k, v)
    b, h = 1, 1
    cols = slice(h * c.dh, (h + 1) * c.dh)
    k2, v2 = k.clone(), v.clone()
    k2[b * c.Tk + 70, cols] = float("nan")
    v2[b * c.Tk + 200, cols] = float("inf")
    ref, _ = A.reference(q, k2, v2, c.n, c.heads, c.fmt)
    bad = ~torch.isfinite(ref)
    item = torch.zeros_like(bad)
    item[b * c.Tq:(b + 1) * c.Tq, cols] = True
    assert torch.equal(bad, item)                                   # the reference: the whole item and nothing else
    got = _run(E, c, q, k2, v2)
    assert bool((~torch.isfinite(got.double()))[item].all()), f"{c.id}: finite outputs in the item with a NaN key"
    same = got.view(torch.int16) == clean.view(torch.int16)
    assert bool(same[~item].all()), f"{c.id}: {int((~same[~item]).sum())} outputs of other (sample, head) items changed"


def test_streaming_attention_values_are_deterministic(E):
    c = A.determinism_case(E.fmt)
    q, k, v = c.inputs()
    ref, bound = A.reference(q, k, v, c.n, c.heads, c.fmt)
    one, two = _run(E, c, q, k, v), _run(E, c, q, k, v)
    assert torch.equal(one.view(torch.int16), two.view(torch.int16))
    print(f"[measured] streaming attention values {E.fmt} determinism: worst |got - ref| / bound {_ratio(c, one, ref, bound):.3f} ({c.id})")
