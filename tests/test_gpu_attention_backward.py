"""GPU: the attention backward (csrc/attention_bwd.hip) read back exactly, bounded against fp64, and held to its contract.

Every launch goes through ``attention_backward(..., out=)`` with a NaN-filled buffer and GUARD rows behind it: an element
the kernels do not write stays NaN and fails whatever reads it, a store past the last row breaks the guard.

* masks    the three exact read-backs and the needle of tests/attn_bwd_witness.py at every length of ``SEQ_LENS``
           (dq<4> with one to four tiles, the <4> | <18> switch at 64 | 65, dq<18> with an odd tile count, dkv<18, 4, 0> up
           to 8 pairs, the straight-line dkv<18, 8, 9> with 17 and 18 tiles), heads = 3, 3 or 2 sequences.
           tests/test_attn_bwd_witness.py proves on the CPU that these checks flag every defect of ``BWD_DEFECTS``.
* values   every element of dQ, dK, dV against the fp64 model within the bound DERIVED in attn_bwd_witness's docstring
           (never tuned here), on the random inputs of test_gpu_grad.py and on spiky scores (q times 32).  The worst
           |err| / bound per output is printed (``pytest -s``); EXPERIMENTS.md keeps it beside the emulator's.
* contract all elements written, guard rows untouched, NaN containment per (sequence, head), equal bits on a second call,
           every item bit-equal to itself run alone, and what the C entry point refuses.
"""
import ctypes as C

import pytest
import torch

import attn_bwd_witness as B

pytestmark = pytest.mark.gpu

GUARD = 2
HEADS = B.HEADS


def _launch(eng, qkv, dout, n_seq, T, heads):
    """dqkv bf16 [rows, 3 * width] on the GPU, written into a NaN buffer whose guard rows must stay NaN."""
    rows, w = n_seq * T, heads * 64
    buf = torch.full((rows + GUARD, 3 * w), float("nan"), dtype=torch.bfloat16, device="cuda")
    got = eng.attention_backward(qkv.to(torch.bfloat16).cuda(), dout.to(torch.bfloat16).cuda(), n_seq, T, heads, out=buf[:rows])
    assert got.data_ptr() == buf.data_ptr()
    assert torch.isnan(buf[rows:]).all(), f"T {T}: rows past the output were written"
    return buf[:rows]


def _kernel(eng, n_seq, T, heads):
    return lambda qkv, dout: _launch(eng, qkv, dout, n_seq, T, heads).float().cpu()


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("T", B.SEQ_LENS)
def test_attention_backward_masks(gpu_engine, T):
    n_seq = B.n_seq_of(T)
    fails = B.check_all(_kernel(gpu_engine, n_seq, T, HEADS), T, n_seq, HEADS)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("T,spiky", B.value_cases(), ids=[f"{T}{'-spiky' if s else ''}" for T, s in B.value_cases()])
def test_attention_backward_values_vs_fp64(gpu_engine, T, spiky):
    n_seq = B.n_seq_of(T)
    got = _kernel(gpu_engine, n_seq, T, HEADS)(*B.value_input(T, n_seq, HEADS, spiky))
    fails, worst = B.check_values(got, T, n_seq, HEADS, spiky)
    print(f"[measured] attention backward T={T}{' spiky' if spiky else ''}: worst |err| / bound  " +
          "  ".join(f"{g} {worst[g]:.3f}" for g in B.GRADS))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("T", B.CONTRACT)
def test_every_element_is_written_and_a_second_call_gives_equal_bits(gpu_engine, T):
    n_seq = B.n_seq_of(T)
    qkv, dout = B.value_input(T, n_seq, HEADS)
    a = _launch(gpu_engine, qkv, dout, n_seq, T, HEADS)
    b = _launch(gpu_engine, qkv, dout, n_seq, T, HEADS)
    assert torch.isfinite(a).all(), f"T {T}: {int((~torch.isfinite(a)).sum())} elements unwritten or not finite"
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("T", B.CONTRACT)
def test_nan_stays_inside_its_sequence_and_head(gpu_engine, T):
    """One NaN in q, k, v or dO of (sequence 1, head 1) -- at the first row, the last row of the last full tile and the
    last row (the one the kernels clamp padded rows to; at 49, 65 and 257 rows it is the whole ragged tile) -- leaves every
    other (sequence, head) block bit-equal."""
    n_seq, w = B.n_seq_of(T), HEADS * 64
    qkv, dout = B.value_input(T, n_seq, HEADS)
    base = _bits(_launch(gpu_engine, qkv, dout, n_seq, T, HEADS)).cpu().view(n_seq, T, 3, HEADS, 64)
    s, h = 1, 1
    other = torch.ones((n_seq, HEADS), dtype=torch.bool)
    other[s, h] = False
    for pos in sorted({0, (T - 1) // 16 * 16 - 1, T - 1}):
        for which in range(4):
            x, g = qkv.clone(), dout.clone()
            (g if which == 3 else x)[s * T + pos, (0 if which == 3 else which * w) + h * 64 + 5] = float("nan")
            got = _bits(_launch(gpu_engine, x, g, n_seq, T, HEADS)).cpu().view(n_seq, T, 3, HEADS, 64)
            same = (got == base).all(-1).all(1).all(1)              # [n_seq, heads]: over columns, rows, dq | dk | dv
            assert same[other].all(), (f"T {T}: a NaN in {('q', 'k', 'v', 'dO')[which]} at position {pos} of sequence {s} "
                                       f"head {h} changed (sequence, head) {(~same & other).nonzero().tolist()}")


@pytest.mark.parametrize("T,n_seq,heads", [(T, 3, 3) for T in B.CONTRACT] + [(49, 2, 16)])
def test_every_item_equals_itself_run_alone(gpu_engine, T, n_seq, heads):
    """The XCD-contiguous item order and the addressing of the statistics between the passes: an item's bits do not depend
    on where it stands in the launch."""
    w = heads * 64
    qkv, dout = B.value_input(T, n_seq, heads)
    batch = _launch(gpu_engine, qkv, dout, n_seq, T, heads).cpu().view(n_seq, T, 3, heads, 64)
    for s in range(n_seq):
        for h in range(heads):
            x = qkv.view(n_seq, T, 3, heads, 64)[s, :, :, h].reshape(T, 3 * 64).contiguous()
            g = dout.view(n_seq, T, heads, 64)[s, :, h].contiguous()
            solo = _launch(gpu_engine, x, g, 1, T, 1).cpu().view(T, 3, 64)
            assert torch.equal(_bits(solo), _bits(batch[s, :, :, h])), f"T {T}: item (sequence {s}, head {h}) differs from its solo run"


def test_entry_point_refusals(pkg, gpu_engine):
    eng, lib = gpu_engine, gpu_engine.lib
    T, n_seq, heads = 20, 2, 2
    w = heads * 64
    qkv = torch.zeros((n_seq * 289, 3 * w), dtype=torch.bfloat16, device="cuda")      # large enough for every refused shape
    dout = torch.zeros((n_seq * 289, w), dtype=torch.bfloat16, device="cuda")
    buf = torch.full((n_seq * 289, 3 * w), float("nan"), dtype=torch.bfloat16, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(q, d, o, n, t, hd):
        rc = lib.tvc_attention_backward(eng.handle, q, d, o, n, t, hd, stream)
        torch.cuda.synchronize()
        return rc, (lib.tvc_last_error(eng.handle) or b"").decode()

    for n, t, hd in ((n_seq, 0, heads), (n_seq, 289, heads), (n_seq, T, 0)):
        rc, msg = call(p(qkv), p(dout), p(buf), n, t, hd)
        assert rc != pkg._lib.TVC_OK and "attention_b" in msg, (n, t, hd, rc, msg)
    for n, t, hd in ((-1, T, heads), (n_seq, -1, heads), (n_seq, T, -1)):                # never reach the workspace as a huge size
        rc, msg = call(p(qkv), p(dout), p(buf), n, t, hd)
        assert rc == pkg._lib.TVC_E_INVALID and "tvc_attention_backward" in msg, (n, t, hd, rc, msg)
    for args in ((None, p(dout), p(buf)), (p(qkv), None, p(buf)), (p(qkv), p(dout), None)):
        rc, msg = call(*args, n_seq, T, heads)
        assert rc == pkg._lib.TVC_E_INVALID and "NULL" in msg
    assert call(p(qkv), p(dout), p(buf), 0, T, heads)[0] == pkg._lib.TVC_OK
    assert torch.isnan(buf).all()                                                        # nothing was launched
    with pytest.raises(ValueError):
        eng.attention_backward(qkv[:n_seq * T], dout[:n_seq * T], n_seq, T, heads, out=buf[:n_seq * T].float())
    with pytest.raises(ValueError):
        eng.attention_backward(qkv[:n_seq * T], dout[:n_seq * T], n_seq, T, heads, out=buf[:n_seq * T + 1])
    with pytest.raises(ValueError):
        eng.attention_backward(qkv[:n_seq * T], dout[:n_seq * T], n_seq, T, heads, out=buf[:n_seq * T].cpu())
    with pytest.raises(ValueError):
        eng.attention_backward(qkv[:n_seq * T], dout[:n_seq * T], n_seq, T, heads, out=buf[:2 * n_seq * T:2])
    assert torch.isnan(buf).all()
    assert torch.isfinite(eng.attention_backward(qkv[:n_seq * T], dout[:n_seq * T], n_seq, T, heads)).all()     # and it still works
