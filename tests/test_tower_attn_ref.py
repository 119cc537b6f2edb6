"""CPU: the value check of the tower attention kernels (tests/tower_attn_ref.py) is itself right, and it catches what it is for.

1. ``reference`` is ``attn_witness.model`` and its weights reproduce it; the bounds are positive and finite.
2. The defect-free fp32 emulation of each kernel's arithmetic (attention.hip in bf16 and fp16, the split kernel, the fp32
   kernel) is within the per-element bound on EVERY element of EVERY case the GPU file runs
   (``tower_attn_ref.gpu_cases()``), and the reference stays finite after rounding to the format.
3. Every template of the launchers meets every profile, in every precision.
4. The profiles reach what they claim: ``flat`` about 100 effective keys at 288 tokens, ``peaked`` about 5, ``spiky``
   scores tens of nats apart with fp16 probabilities below 2^-24, ``offset`` scores whose exponential overflows without the
   subtraction of the maximum.
5. Every value defect of ``tower_attn_ref.DEFECTS`` -- injected into the emulation -- exceeds the bound or goes non-finite
   on cases the GPU file runs, in bf16 and in fp16; the table is printed (``pytest -s``).
   ``denominator_over_unrounded_probabilities`` is NOT caught and need not be: numerator and denominator then differ by one
   rounding per probability, which the bound's 2 eps allows; the test asserts what is true, that it stays inside.
6. THE GAP THIS CLOSES.  test_gpu_kernels.py::test_attention asserts max |err| < 3e-2 and mean |err| < 3e-3 in bf16
   (attn_witness.PRECISION) on unit-variance random inputs, where about T / e keys share a softmax and |out| is about 0.1.
   A softmax scale that is 1 % too large or too small passes that criterion on its own inputs at T = 17, 77 and 257
   (emulated: max |err| 2.0e-2 to 2.7e-2, mean 1.0e-3 to 2.2e-3), while the per-element bound is exceeded 2.4 to 3.8 times
   on those same inputs and up to 11 times (bf16) / 66 times (fp16) on the cases of the GPU file: on every one of them that
   has 16 tokens or more and is not pooled.
"""
from functools import lru_cache

import torch

import attn_witness as W
import sd_ops_ref as R
import tower_attn_ref as A

CASES = A.gpu_cases()
VALUE_DEFECTS = tuple(d for d in A.DEFECTS if d not in A.HARMLESS)


@lru_cache(maxsize=None)
def _scan():
    """case id -> {None or defect: worst |out - ref| / bound}; one pass, the reference of a case computed once."""
    res = {}
    for c in CASES:
        qkv = c.inputs()
        ref, bound = A.reference(qkv, c.cfg, c.precision)
        assert ref.shape == bound.shape == (c.cfg.n_out, c.cfg.width) and ref.dtype == bound.dtype == torch.float64
        assert bool(torch.isfinite(bound).all()) and bool((bound > 0).all()), c.id
        assert bool(torch.isfinite(A.to_format(ref, c.precision)).all()), c.id
        res[c.id] = {None: A.worst_ratio(A.emulate(qkv, c.cfg, c.precision), ref, bound)}
        if c.precision in A.EPS:
            for d in A.DEFECTS:
                res[c.id][d] = A.worst_ratio(A.emulate(qkv, c.cfg, c.precision, d), ref, bound)
    return res


def test_cases_cover_every_config_and_every_template_meets_every_profile():
    names = lambda p: list(dict.fromkeys(c.cfg.name for c in CASES if c.precision == p))
    assert names("bf16") == names("fp16") == [c.name for c in W.tower_configs()]
    assert names("split") == list(dict.fromkeys(c.name for c in W.split_configs()))
    assert names("fp32") == [c.name for c in W.f32_configs()]
    assert len(CASES) <= len(W.tower_configs()) * 2 + len(W.split_configs()) + len(W.f32_configs()) + 4
    assert len({c.id for c in CASES}) == len(CASES)
    assert max(c.cfg.seq_len for c in CASES) == 288 and max(c.cfg.heads for c in CASES) == 3      # nothing larger
    for p in A.PRECISIONS:
        met = {}
        for c in CASES:
            if c.precision == p:
                met.setdefault(c.template, set()).update(c.profiles)
                assert len(set(c.profiles)) == c.cfg.heads                    # every head of a case has its own profile
        assert all(v == set(A.PROFILES) for v in met.values()), (p, met)
    tower = {c.template for c in CASES if c.precision == "bf16"}
    assert tower == {"<2, causal>", "<6, causal>", "<18, causal>", "<17, full, EXACT>", "<4, full, EXACT>", "<2, full>",
                     "<4, full>", "<6, full>", "<18, full>"}                 # every branch of launch_attention_t


def test_inputs_are_values_of_the_format():
    for c in CASES[::7]:
        qkv = c.inputs()
        assert torch.equal(qkv, A.to_format(qkv, c.precision)) and torch.equal(qkv, c.inputs())
        v = qkv[:, 2 * c.cfg.width:]
        if v.numel() >= 10000:
            assert abs(v.mean().item() - 0.5) < 0.1 and abs(v.std().item() - 2.0) < 0.1


def test_reference_is_the_model_over_the_plans_weights():
    for c in CASES[::5]:
        qkv = c.inputs()
        ref, _ = A.reference(qkv, c.cfg, c.precision)
        assert torch.equal(ref, W.model(qkv, c.cfg))
        p = W._plan(c.cfg)
        for h, w in enumerate(A.weights(qkv, c.cfg)):
            assert (w.sum(1) - 1).abs().max().item() < 1e-12
            assert bool((w[~p.vis] == 0).all())                               # nothing outside the visibility of attn_witness
            v = qkv[:, 2 * c.cfg.width + h * A.DH: 2 * c.cfg.width + (h + 1) * A.DH]
            assert (w @ v - ref[p.out_row][:, h * A.DH:(h + 1) * A.DH]).abs().max().item() < 1e-12, c.id
        for i in range(0, c.cfg.n_out, 37):
            s, pos = A.where(c.cfg, i)
            assert 0 <= s < c.cfg.n_seq and 0 <= pos < c.cfg.seq_len


def test_causal_rows_with_one_key_collapse_to_the_output_rounding_and_one_weight():
    c = next(x for x in CASES if x.id.startswith("bf16-causal_dense_17"))
    qkv = c.inputs()
    ref, bound = A.reference(qkv, c.cfg, c.precision)
    v0 = qkv[0, 2 * c.cfg.width:]                                             # position 0 sees itself only: w = 1, ref = v
    assert torch.equal(ref[0], v0)
    lim = 0.5 * R.ulp16(v0, "bf16") * (1 + 2.0 ** -8) + (2 * A.EPS["bf16"] + 1e-3) * v0.abs()      # 2 ds <= 1e-3 even at 96 nats
    assert bool((bound[0] <= lim).all())


def test_emulation_within_bound_on_every_case():
    scan = _scan()
    for p in A.PRECISIONS:
        ids = [c.id for c in CASES if c.precision == p]
        w = max(ids, key=lambda i: scan[i][None])
        print(f"[measured] emulation {p}: worst |out - ref| / bound {scan[w][None]:.3f} ({w}), {len(ids)} cases")
        for i in ids:
            assert scan[i][None] <= 1.0, (i, scan[i][None])                  # every element of every case; inf = non-finite


def test_profiles_reach_what_they_claim():
    log2e = torch.tensor(A.LOG2E)                                                             # s below is in nats already
    seen = set()
    for c in CASES:
        qkv = c.inputs()
        p = W._plan(c.cfg)
        ws = A.weights(qkv, c.cfg)
        for (h, q, k, _), w, prof in zip(A._heads(qkv, c.cfg, torch.float64), ws, c.profiles):
            s = torch.where(p.vis, q @ k.t() * 0.125, torch.full((), -float("inf"), dtype=torch.float64))
            top = s.max(1).values
            big = c.cfg.name in ("full_dense_257", "full_dense_272", "full_dense_288")      # T / e = 95 to 106 for N(0, 1) nats
            n_eff = A.effective_keys(w)
            if prof == "flat" and big:
                assert 85 <= n_eff.mean().item() <= 125, (c.id, n_eff.mean().item())
                seen.add((c.precision, prof))
            if prof == "peaked" and big:
                assert 2 <= n_eff.median().item() <= 10, (c.id, n_eff.median().item())
                seen.add((c.precision, prof))
            if prof == "spiky" and big:
                spread = top - torch.where(p.vis, s, torch.full_like(s, float("nan"))).nanmedian(1).values
                assert spread.median().item() >= 20, (c.id, spread.median().item())          # the maximum is tens of nats above the bulk
                assert n_eff.median().item() < 2.5                                              # one or two keys hold the softmax
                if c.precision == "fp16":
                    tiny = torch.exp(s - top[:, None])[p.vis] < 2.0 ** -24
                    assert tiny.double().mean().item() > 0.5, c.id                            # most probabilities are in the flush range
                seen.add((c.precision, prof))
            if prof == "offset":                                                              # on every case, whatever its size
                e = torch.exp2(top.float() * log2e)                                           # exp2 without the subtraction
                if c.precision == "fp16":
                    assert bool((e > R.max_finite("fp16")).all()) and bool(torch.isinf(e.half()).all()), c.id
                else:
                    assert bool(torch.isinf(e).all()), c.id
                near = top - torch.where(p.vis, s, torch.full_like(s, float("inf"))).min(1).values
                assert near.max().item() < 12, c.id                                           # the offset is shared: the row stays flat
                seen.add((c.precision, prof))
    assert seen == {(p, prof) for p in A.PRECISIONS for prof in A.PROFILES}, seen


def test_every_value_defect_is_caught():
    scan = _scan()
    lines = [f"{'defect':42s} format caught  worst ratio  at"]
    for d in A.DEFECTS:
        for fmt in ("bf16", "fp16"):
            ids = [c.id for c in CASES if c.precision == fmt]
            caught = sum(scan[i][d] > 1.0 for i in ids)
            w = max(ids, key=lambda i: scan[i][d])
            lines.append(f"{d:42s} {fmt}   {caught:3d} / {len(ids)}   {scan[w][d]:8.1e}  {w}")
            if d in VALUE_DEFECTS:
                assert caught >= 1 and scan[w][d] > 2.0, (d, fmt, scan[w][d])
            else:
                assert caught == 0, (d, fmt, w, scan[w][d])                  # harmless to the values (module docstring)
    print("\n" + "\n".join(lines))
    # the 1 % scale errors are not a matter of one lucky case: every case with more than a handful of keys shows them
    for fmt in ("bf16", "fp16"):
        ids = [c.id for c in CASES if c.precision == fmt and c.cfg.pool_mode == 0 and c.cfg.seq_len >= 16]
        for d in ("scale_plus_1_percent", "scale_minus_1_percent"):
            assert all(scan[i][d] > 2.0 for i in ids), (d, fmt, min((scan[i][d], i) for i in ids))


def test_present_criterion_passes_a_one_percent_scale_error_in_bf16():
    """The inputs of test_gpu_kernels.py::test_attention (same seed, three of its shapes) and its bounds."""
    b = W.PRECISION["bf16"]
    for n_seq, T, heads, causal in ((3, 17, 4, False), (5, 77, 2, True), (2, 257, 16, False)):
        cfg = W.Config(f"test_attention_{T}", T, n_seq, heads=heads, causal=causal)
        g = torch.Generator().manual_seed(8)
        qkv = torch.randn((n_seq * T, 3 * heads * 64), generator=g).to(torch.bfloat16).double()
        ref, bound = A.reference(qkv, cfg, "bf16")
        assert A.worst_ratio(A.emulate(qkv, cfg, "bf16"), ref, bound) <= 1.0
        for d in ("scale_plus_1_percent", "scale_minus_1_percent"):
            out = A.emulate(qkv, cfg, "bf16", d)
            err = (out - ref).abs()
            ratio = A.worst_ratio(out, ref, bound)
            print(f"[measured] {d} T = {T}: max |err| {err.max().item():.2e} (allowed {b['max_abs']:.0e}), mean "
                  f"{err.mean().item():.2e} (allowed {b['mean_abs']:.0e}); new criterion: {ratio:.1f} times the bound")
            assert err.max().item() < b["max_abs"] and err.mean().item() < b["mean_abs"]      # today's test lets it through
            assert ratio > 2.0                                                                 # the per-element bound does not
