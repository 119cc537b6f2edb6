"""CPU: the value check of the streaming attention (tests/sd_attn_ref.py) is itself right, and it catches what it is for.

1. ``reference`` equals ``oracle/sd_oracle.attention`` in fp64.
2. The defect-free fp32 emulation of the kernel's tile loop is within the per-element bound on EVERY case the GPU file
   runs (``sd_attn_ref.gpu_cases()``), so the bound is one a correct kernel of this design can meet.
3. The cases reach the arithmetic they are for: where a rise* profile climbs 10 bits over full tiles, class +1 rows move
   their reference after tile 0 and share a 16-query block with rows that stay; every class +1 row of a ``threshold``
   head is on the stated side of 2^8.
4. The inputs of test_gpu_sd.py::test_streaming_attention_vs_fp64 (same seeds, shapes with Tk <= 1024) never move the
   reference after tile 0: the gap the new cases close.
5. Every value defect of ``sd_attn_ref.DEFECTS`` -- injected into the emulation -- violates the bound, or gives a
   non-finite output where the reference is finite, at cases the GPU file runs.

The table below is what ``test_every_defect_is_caught`` prints (``pytest -s``): per defect and format, at how many of the
150 shape-1 cases (n = 2, heads = 3, Tq = 65; 75 per format: the rotation over every head dim, the separate-stride, containment
and determinism cases) the worst |out - ref| / bound exceeds 1, the largest ratio,
and the case that shows it.

defect                                   format caught  worst ratio  at
sum_not_rescaled                         bf16    69 / 75    1.7e+02  fall9-bf16-n2h3d40-Tq65-Tk129
sum_not_rescaled                         fp16    69 / 75    1.2e+03  late_spike-fp16-n2h3d8-Tq65-Tk449
output_not_rescaled                      bf16    69 / 75    1.2e+07  fall9-bf16-n2h3d64-Tq65-Tk449
output_not_rescaled                      fp16    69 / 75    3.5e+07  rise9-fp16-n2h3d80-Tq65-Tk449
alpha_squared                            bf16    50 / 75    7.3e+02  rise3-bf16-n2h3d128-Tq65-Tk449
alpha_squared                            fp16    69 / 75    4.5e+03  rise3-fp16-n2h3d80-Tq65-Tk193
staying_lanes_rescale_output_only        bf16    60 / 75    1.4e+02  rise5-bf16-n2h3d56-Tq65-Tk129
staying_lanes_rescale_output_only        fp16    68 / 75    1.1e+03  rise5-fp16-n2h3d56-Tq65-Tk129
reference_never_moves_after_first_tile   bf16     4 / 75        inf  fall9-bf16-n2h3d24-Tq65-Tk1088
reference_never_moves_after_first_tile   fp16    33 / 75        inf  rise9-fp16-n2h3d8-Tq65-Tk193
threshold_compares_nats_not_bits         bf16     0 / 75    5.9e-01  rise9-bf16-n2h3d8-Tq65-Tk193
threshold_compares_nats_not_bits         fp16     0 / 75    6.1e-01  late_spike-fp16-n2h3d80-Tq65-Tk65
ragged_tile_duplicates_counted           bf16    48 / 75    7.8e+02  rise3-bf16-n2h3d128-Tq65-Tk449
ragged_tile_duplicates_counted           fp16    48 / 75    5.8e+03  rise9-fp16-n2h3d40-Tq65-Tk65
last_key_tile_skipped_when_odd           bf16    39 / 75    7.1e+03  late_spike-bf16-n2h3d96-Tq65-Tk129
last_key_tile_skipped_when_odd           fp16    39 / 75    2.8e+04  late_spike-fp16-n2h3d96-Tq65-Tk129

``reference_never_moves_after_first_tile`` need only be caught in fp16 (probabilities beyond 65504 become inf once the
reference lags 16 bits); in bf16 it shows only where the lag passes fp32's own range (128 bits: the 17-tile stream).

``threshold_compares_nats_not_bits`` is NOT caught, by this or any value check, and should not be: o / l does not depend
on where the reference stands, only the range of the probabilities does.  Without log2(e) the reference lags by up to
8 / ln 2 = 11.5 bits instead of 8; probabilities up to 2^11.5 are far inside fp16 and the result is as accurate as
before (the same holds for a threshold in the raw units of q.k, which only moves earlier).  What the test asserts for
it is what is true: it changes when the reference moves (fewer moves on the rise9 stream) and stays within the bound.
A threshold that is wrong by enough to matter is ``reference_never_moves_after_first_tile``.
"""
from functools import lru_cache

import pytest
import torch

import sd_attn_ref as A
from attn_witness import SD_HEAD_DIMS
from oracle import sd_oracle

CASES = A.gpu_cases()
SMALL = [c for c in CASES if c.n == 2]
VALUE_DEFECTS = tuple(d for d in A.DEFECTS if d != "threshold_compares_nats_not_bits")
# the shapes of test_gpu_sd.py::test_streaming_attention_vs_fp64 with Tk <= 1024
RANDOM_SHAPES = [(2, 8, 80, 1024, 1024), (2, 8, 160, 256, 256), (3, 8, 160, 64, 64), (2, 8, 40, 1024, 77), (2, 8, 160, 64, 77),
                 (1, 2, 64, 100, 50), (1, 3, 8, 70, 130), (22, 8, 40, 700, 700), (22, 8, 40, 600, 77), (24, 8, 32, 520, 130),
                 (22, 8, 80, 700, 200)]


@lru_cache(maxsize=None)
def _small(case):
    """Inputs, reference and bound of a shape-1 case: computed once, shared, never modified."""
    q, k, v = case.inputs()
    return (q, k, v) + A.reference(q, k, v, case.n, case.heads, case.fmt)


def _full(case):
    if case.n == 2:
        return _small(case)
    q, k, v = case.inputs()
    return (q, k, v) + A.reference(q, k, v, case.n, case.heads, case.fmt)


def test_cases_are_the_ones_the_issue_sets():
    for fmt in A.FMTS:
        met = {(c.profile, c.Tk) for dh in SD_HEAD_DIMS for c in A.every_head_dim_cases(dh, fmt)}
        assert met == {(p, Tk) for p in A.PROFILES for Tk in A.TKS}              # every profile meets every Tk
        assert all(len(A.every_head_dim_cases(dh, fmt)) == len(A.PROFILES) for dh in SD_HEAD_DIMS)
    assert len(CASES) == len(set(CASES)) and all(c.fmt in A.FMTS for c in CASES)


def test_inputs_are_values_of_the_format_with_the_stated_offsets():
    for c in (A.Case("rise5", "bf16", 2, 3, 40, 65, 193), A.Case("threshold", "fp16", 2, 4, 24, 65, 129),
              A.Case("late_spike", "fp16", 2, 3, 160, 65, 65), A.Case("fall9", "bf16", 2, 3, 8, 65, 1088)):
        q, k, v = c.inputs()
        for t in (q, k, v):
            assert torch.equal(t, t.to(A.R.FORMATS[c.fmt]["dtype"]).double())
        qs, ks = A._split(q, c.n, c.heads), A._split(k, c.n, c.heads)
        bits = qs[..., :1] @ ks[..., :1].transpose(-1, -2) / (c.dh ** 0.5 * A.LN2)          # what column 0 adds, in bits
        want = A.class_of_query(c.Tq)[None, None, :, None] * A.profile_bits(c.profile, c.heads, c.Tk)[None, :, None, :]
        tol = want.abs() * 2.0 ** -8 + 1e-12                                           # a_j is rounded to the format once
        assert ((bits - want).abs() <= tol).all()
        assert abs(v.mean().item() - 0.5) < 0.1 and abs(v.std().item() - 2.0) < 0.1


def test_reference_equals_the_oracle():
    c = A.Case("rise3", "bf16", 2, 3, 40, 33, 130)
    g = torch.Generator().manual_seed(5)
    C = c.heads * c.dh
    q, k, v = (torch.randn((c.n * T, C), generator=g, dtype=torch.float64) for T in (c.Tq, c.Tk, c.Tk))
    ref, bound = A.reference(q, k, v, c.n, c.heads, c.fmt)
    want = sd_oracle.attention(q.view(c.n, c.Tq, C), k.view(c.n, c.Tk, C), v.view(c.n, c.Tk, C), c.heads).reshape(-1, C)
    assert want.dtype == torch.float64 and (ref - want).abs().max().item() < 1e-13
    assert (bound > 0).all() and torch.isfinite(bound).all()


GROUPS = [(fmt, dh) for fmt in A.FMTS for dh in SD_HEAD_DIMS]


@pytest.mark.parametrize("fmt,dh", GROUPS)
def test_emulation_within_bound_every_head_dim(fmt, dh):
    worst = 0.0
    for c in A.every_head_dim_cases(dh, fmt):
        q, k, v, ref, bound = _small(c)
        out, _ = A.emulate(q, k, v, c.n, c.heads, c.fmt)
        r = A.worst_ratio(out, ref, bound)
        worst = max(worst, r)
        assert r <= 1.0, (c.id, r)
    print(f"[measured] emulation {fmt} dh {dh}: worst |out - ref| / bound {worst:.3f}")


@pytest.mark.parametrize("case", [c for c in CASES if c not in {x for f, d in GROUPS for x in A.every_head_dim_cases(d, f)}],
                         ids=lambda c: c.id)
def test_emulation_within_bound_other_cases(case):
    q, k, v, ref, bound = _full(case)
    out, moves = A.emulate(q, k, v, case.n, case.heads, case.fmt)
    r = A.worst_ratio(out, ref, bound)
    print(f"[measured] emulation {case.id}: worst |out - ref| / bound {r:.3f}")
    assert r <= 1.0
    _check_moves(case, moves)


def _check_moves(c, moves):
    """moves int64 [n, heads, Tq] of the defect-free emulation."""
    plus = moves[..., 0::3]
    if A.climbs(c):
        frac = (plus >= 1).double().mean().item()
        assert frac >= 0.99, (c.id, frac)                               # class +1 rows move (all but a 3-sigma tail)
        moved = torch.zeros((c.n, c.heads, (c.Tq + 15) // 16 * 16), dtype=torch.bool)
        moved[..., :c.Tq] = moves >= 1
        real = torch.zeros(moved.shape[-1], dtype=torch.bool)
        real[:c.Tq] = True
        blocks, real = moved.view(c.n, c.heads, -1, 16), real.view(-1, 16)
        mixed = blocks.any(-1) & (~blocks & real).any(-1)               # a block with a moving and a staying row
        assert mixed.any(), c.id
        full = real.all(-1)
        assert mixed[..., full].all(), c.id                             # in fact every full block of every (sample, head)
    if c.profile == "threshold":
        assert (plus[:, 0::2] == 0).all(), c.id                         # even heads: 2^7.75, no move
        assert (plus[:, 1::2] == 1).all(), c.id                         # odd heads: 2^8.25, one move
        assert (moves[..., 1::3] == 0).all() and (moves[..., 2::3] == 0).all(), c.id
    if c.profile == "fall9":
        assert (plus == 0).all(), c.id                                  # class +1 falls: tile 0 stays the reference


def test_cases_reach_the_rescale_branch():
    most = {}
    for c in SMALL:
        q, k, v, _, _ = _small(c)
        _, moves = A.emulate(q, k, v, c.n, c.heads, c.fmt)
        _check_moves(c, moves)
        if c.profile in A.RISE:
            key = (c.profile, c.fmt)
            most[key] = max(most.get(key, 0), int(moves[..., 0::3].min()))
    # the 17-tile stream moves every class +1 row again and again: rise3 about every third tile, rise5 every second, rise9
    # every tile -- and, whatever the randn columns add, no later than one tile after that (every 4th / 3rd / 2nd of 16)
    for fmt in A.FMTS:
        assert most[("rise3", fmt)] >= 4 and most[("rise5", fmt)] >= 5 and most[("rise9", fmt)] >= 8, most
    assert sum(A.climbs(c) for c in CASES) >= 40


def test_random_inputs_never_move_the_reference_after_the_first_tile():
    """The inputs of test_gpu_sd.py::test_streaming_attention_vs_fp64: scores of about N(0, 1) nats, a later move would need
    one 5.5 nats above the largest of the first 64.  The rescale runs once per row, from -inf on zeros, and never again."""
    for n, heads, dh, Tq, Tk in RANDOM_SHAPES:
        g = torch.Generator().manual_seed(Tq + dh)
        C = heads * dh
        q, k, v = (torch.randn((n * T, C), generator=g).to(torch.bfloat16).double() for T in (Tq, Tk, Tk))
        _, moves = A.emulate(q, k, v, n, heads, "bf16")
        assert int(moves.sum()) == 0, (n, heads, dh, Tq, Tk, int(moves.sum()))


def test_every_defect_is_caught():
    lines = [f"{'defect':40s} format caught  worst ratio  at"]
    clean = {}
    for d in A.DEFECTS:
        for fmt in A.FMTS:
            caught, worst, at = 0, 0.0, None
            cases = [c for c in SMALL if c.fmt == fmt]
            for c in cases:
                q, k, v, ref, bound = _small(c)
                assert torch.isfinite(ref).all()
                out, moves = A.emulate(q, k, v, c.n, c.heads, c.fmt, defect=d)
                r = A.worst_ratio(out, ref, bound)
                caught += r > 1.0
                if r > worst:
                    worst, at = r, c.id
                if d == "threshold_compares_nats_not_bits" and c.profile == "rise9" and c.Tk == 1088:
                    clean[fmt] = (int(moves.sum()), int(A.emulate(q, k, v, c.n, c.heads, c.fmt)[1].sum()))
            lines.append(f"{d:40s} {fmt}   {caught:3d} / {len(cases)}   {worst:8.1e}  {at}")
            if d in VALUE_DEFECTS and (fmt == "fp16" or d != "reference_never_moves_after_first_tile"):
                assert caught >= 1 and worst > 2.0, (d, fmt, worst)
            if d == "threshold_compares_nats_not_bits":
                assert caught == 0, (d, fmt, worst)                     # harmless to the values (module docstring)
                assert clean[fmt][0] < clean[fmt][1], clean               # but not the same kernel: fewer moves
    print("\n" + "\n".join(lines))
