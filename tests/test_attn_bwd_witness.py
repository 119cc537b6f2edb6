"""CPU: the attention-backward witnesses of tests/attn_bwd_witness.py are themselves right, and catch what they are for.

1. ``model`` (no defect) equals torch autograd in fp64 to 1e-12.
2. ``check_all`` is silent on the defect-free model rounded to bf16.
3. Every defect of ``BWD_DEFECTS`` -- injected into the fp64 model, whose output is then rounded to bf16 as the kernel's
   would be -- is flagged by a read-back or the needle at cases that tests/test_gpu_attention_backward.py runs too (it runs
   every length of ``SEQ_LENS``).  ``test_every_defect_is_caught`` prints (``pytest -s``) the table that EXPERIMENTS.md
   keeps: per defect and case which probes flag it, and whether the random-input criterion of
   test_gpu_grad.py::test_attention_backward_vs_autograd (rel L2 < 5e-3 and max / max < 8e-3 per output, its inputs at this
   shape) would have PASSED it.
4. ``emulate`` -- fp32 with bf16 at the kernel's pack points -- is inside the derived value bound at every GPU case, and
   its worst |err| / bound is printed; below 0.25 the derivation would be too loose.
"""
import pytest
import torch

import attn_bwd_witness as B
import attn_witness as W


def _bf16(f):
    return lambda qkv, dout: f(qkv, dout).to(torch.bfloat16)


@pytest.mark.parametrize("T", [1, 17, 49, 65])
def test_model_equals_autograd(T):
    n_seq, heads = 2, 3
    w = heads * 64
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn((n_seq * T, 3 * w), generator=g, dtype=torch.float64)
    dout = torch.randn((n_seq * T, w), generator=g, dtype=torch.float64)
    x = qkv.clone().requires_grad_(True)
    q, k, v = (x[:, i * w:(i + 1) * w].view(n_seq, T, heads, 64).transpose(1, 2) for i in range(3))
    o = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v).transpose(1, 2).reshape(n_seq * T, w)
    o.backward(dout)
    assert (B.model(qkv, dout, T, n_seq, heads) - x.grad).abs().max().item() < 1e-12


@pytest.mark.parametrize("T", [1, 17, 65, 257])
def test_witnesses_pass_on_the_defect_free_model(T):
    n_seq = B.n_seq_of(T)
    assert B.check_all(_bf16(lambda qkv, dout: B.model(qkv, dout, T, n_seq, B.HEADS)), T, n_seq, B.HEADS) == []


# defect -> the sequence lengths (all run on the GPU too, heads = 3, n_seq_of(T) sequences) at which it must be flagged
DEFECT_CASES = {
    "last_key_dropped_in_last_query_block_A": (49, 257),
    "last_key_dropped_in_last_query_block_B": (49, 257),
    "padded_key_copy_of_row_T_minus_1_A": (49, 257),
    "next_sequence_first_row_visible_A": (65, 257),
    "next_sequence_first_row_visible_B": (65, 257),
    "previous_sequence_last_row_visible_A": (64, 273),
    "previous_sequence_last_row_visible_B": (64, 273),
    "query_row_T_minus_1_counted_twice_B": (17, 257),
    "last_query_block_missing_B": (33, 288),
    "odd_last_key_tile_twice_in_dq_A": (48, 80, 257),
    "item_reads_next_heads_v": (32, 197),
    "item_reads_next_heads_dout": (32, 197),
    "pass_b_statistics_of_next_head": (81, 256),
    "pass_b_statistics_of_row_plus_1": (81, 256),
    "last_item_repeats_the_item_before": (15, 272),
    "dk_dv_columns_swapped": (16, 257),
    "head_halves_swapped": (1, 81),
}


def _old_criterion(T, n_seq, heads, defect):
    """test_attention_backward_vs_autograd's two norms per output on its inputs at this shape: (passes, text)."""
    qkv, dout = B.value_input(T, n_seq, heads)
    want = B.value_reference(T, n_seq, heads)[0]
    got = B.model(qkv, dout, T, n_seq, heads, defect).to(torch.bfloat16).double()
    w, ok, text = heads * 64, True, []
    for g in range(3):
        a, b = got[:, g * w:(g + 1) * w], want[:, g * w:(g + 1) * w]
        rel = (a - b).norm().item() / max(b.norm().item(), 1e-12)
        mx = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)
        ok = ok and rel < 5e-3 and mx < 8e-3
        text.append(f"{rel:.1e}/{mx:.1e}")
    return ok, " ".join(text)


def test_every_defect_is_caught():
    assert set(DEFECT_CASES) == set(B.BWD_DEFECTS)
    assert all(T in B.SEQ_LENS for c in DEFECT_CASES.values() for T in c)
    b = W.PRECISION["bf16"]
    lines = [f"{'defect':40s} {'T':>3s}  dv-rb  dq-rb  dk-rb  needle  old criterion (rel / max of dq dk dv)"]
    for defect in B.BWD_DEFECTS:
        for T in DEFECT_CASES[defect]:
            n_seq, heads = B.n_seq_of(T), B.HEADS
            broken = _bf16(lambda qkv, dout: B.model(qkv, dout, T, n_seq, heads, defect))
            hit = [bool(B.check_readback(broken, p, T, n_seq, heads, b["rel"])) for p in B.PROBES]
            hit.append(bool(B.check_needle(broken, T, n_seq, heads, b["max_abs"], b["mean_abs"])))
            ok, text = _old_criterion(T, n_seq, heads, defect)
            lines.append(f"{defect:40s} {T:3d}  " + "  ".join(f"{'caught' if x else 'passes':6s}" for x in hit[:3]) +
                         f"  {'caught' if hit[3] else 'passes':6s}  {'PASSES' if ok else 'caught'} ({text})")
            assert any(hit), (defect, T)
    print("\n" + "\n".join(lines))


def test_emulator_is_inside_the_value_bound():
    lines = [f"{'case':12s} worst |emulate - model| / bound:  dq     dk     dv"]
    top = {g: 0.0 for g in B.GRADS}
    for T, spiky in B.value_cases():
        n_seq, heads = B.n_seq_of(T), B.HEADS
        got = B.emulate(*B.value_input(T, n_seq, heads, spiky), T, n_seq, heads)
        fails, worst = B.check_values(got, T, n_seq, heads, spiky)
        lines.append(f"{str(T) + (' spiky' if spiky else ''):12s}                                  " +
                     "  ".join(f"{worst[g]:.3f}" for g in B.GRADS))
        assert not fails, "\n".join(fails)
        top = {g: max(top[g], worst[g]) for g in B.GRADS}
    print("\n" + "\n".join(lines))
    print("worst over all cases: " + "  ".join(f"{g} {top[g]:.3f}" for g in B.GRADS))
    assert all(0.25 <= top[g] <= 1.0 for g in B.GRADS), top       # below 0.25 the derivation would be too loose
