"""CPU: the bank-search witnesses of tests/bank_witness.py are themselves right, and catch what they are for.

1. ``plan`` equals csrc/host_plan.hpp's ``bank_plan`` at every probe shape (through tests/gemm_form/driver.cpp).
2. ``model`` without a defect equals brute force -- a stable sort of the similarity matrix -- at every CPU-sized probe, in
   every form the probe is run in.
3. Every probe is valid by the model alone (``validate``): exact values, decided lists, caps reached only where aimed at;
   the planted winners of the position read-back reach what tests/test_gpu_bank_witness.py claims for them.
4. Every defect of ``BANK_DEFECTS``, run as the "kernel", is flagged by a probe the GPU suite runs too.
   ``test_every_defect_is_caught`` prints (``pytest -s``) the table that EXPERIMENTS.md keeps, with the verdict of the old
   criterion beside it: the same defect on tests/test_gpu_path.py's unit-vector data at (1000, 48, 512, 5) and
   (4097, 257, 256, 32), judged by its ``_check_topk`` (1e-5) and its moment bounds.
"""
import subprocess

import numpy as np
import pytest
import torch

import bank_witness as B
from test_gemm_form import gemm_form  # noqa: F401  (the fixture that builds tests/gemm_form/driver.cpp)

CPU_PROBES = [n for n in B.CATALOG if B.cpu_sized(n)]


def test_plan_is_bank_plan(gemm_form):  # noqa: F811
    shapes = {(B.probe(n).shape[0], B.probe(n).shape[1], B.probe(n).k) for n in CPU_PROBES}
    shapes |= {(70001, 64, 20), (90001, 770, 5), (70001, 1, 20), (70001, 2, 20), (40000, 1, 5), (1000, 48, 5), (4097, 257, 32)}
    for R, M, k in sorted(shapes):
        r = subprocess.run([str(gemm_form.exe), "bank_plan", str(R), str(M), str(k)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-3000:]
        got = dict(kv.split("=") for kv in r.stdout.split())
        P = B.plan(R, M, k)
        mine = {"n_sample": P["n_sample"], "stride": P["stride"], "S": P["S"], "nQt": P["nqt"], "bank_tiles": P["nbt"],
                "tiles_per_chunk": P["tpc"]}
        assert {key: int(got[key]) for key in mine} == mine, (R, M, k, r.stdout)


@pytest.mark.parametrize("name", CPU_PROBES)
def test_probe_is_valid_and_model_is_brute_force(name):
    p = B.probe(name)
    for form, _ in p.forms() + [("dense", None)]:
        r = B.validate(p, form) if form != "dense" else B.reference(p, form)
        assert r.exact
        if p.overflow and form != "dense":
            continue
        idx, sim = B.brute(p.bank, p.q, p.k, p.idx_offset, filt=B.FORMS[form][0])
        assert np.array_equal(r.idx, idx) and np.array_equal(r.sim.view(np.int32), sim.view(np.int32)), (name, form)


def test_planted_winners_reach_every_position():
    """What the GPU position read-back claims: over the queries of the two large-M probes every tile-row position meets every
    wave column and every query position both wave rows; the named rows are there; the skinny shapes reach every row mod 16
    and every query position they have."""
    for name, form in (("code(4097,257,64,5)", "filter"), ("code(4097,257,64,32)", "filter")):
        c = B.coverage(B.probe(name), form)
        assert c["confirmed"] == c["planted"] and len(c["row_x_wn"]) == 1024 and len(c["query_x_wm"]) == 512, c
        assert c["last_row"] and c["ragged_tile"] >= 1 and c["chunk_first"] >= 2 and c["chunk_last"] >= 2 and c["past_sample"] >= 1
    c = B.coverage(B.probe("code(255,70,64,7)"), "filter")           # one ragged tile: all of its 255 rows
    assert c["ragged_tile"] == 255 and {r for r, _ in c["row_x_wn"]} == set(range(255))
    for M in B.SKINNY_M:
        c = B.coverage(B.probe(f"code(4097,{M},128,7)"), "skinny")
        assert c["confirmed"] == c["planted"] and c["last_row"] and c["past_sample"] >= 1
        assert {q for q, _ in c["query_x_wm"]} == set(range(M))
        assert M < 16 or {r for r, _ in c["row16_x_q64"]} == set(range(16))


# defect -> (probe, search arguments) at which it must be flagged; all of them run on the GPU too
_F, _P, _M = dict(want_moments=False, allow_filter=True), dict(want_moments=False, allow_filter=False), dict(want_moments=True, allow_filter=True)
DEFECT_CASES = {
    "sample_ignores_stride": [("stride(D=64)", _F), ("stride(D=128)", _F), ("stride(D=64)", _M)],
    "sample_clamped_row_in_two_groups": [("tight_tau(k=16,D=128,bf16)", _F), ("tight_tau(k=128,D=128,bf16)", _F)],
    "rank_off_by_one": [("tight_tau(k=16,D=64,bf16)", _F), ("tight_tau(k=128,D=128,bf16)", _F), ("tight_tau(k=17,D=128,f32)", _M)],
    # (the all-products forms: in the filter forms the margin, ~1 on this data, hides the slack)
    "slack_dropped": [("tight_tau(k=17,D=64,bf16)", _M), ("tight_tau(k=16,D=128,bf16)", _P), ("tight_tau(k=128,D=64,bf16)", _P)],
    "margin_lacks_bl_qh": [("margin_bl_qh(R=4099,D=64,row=4098)", _F), ("margin_bl_qh(R=4099,D=128,row=4098)", _F)],
    "margin_lacks_bh_ql": [("margin_bh_ql(R=4099,D=64,row=4098)", _F), ("margin_bh_ql(R=4099,D=128,row=4098)", _F)],
    "bounds_skip_last_row": [("margin_bl_qh(R=4099,D=64,row=4098)", _F), ("margin_bl_qh(R=20001,D=128,row=20000)", _F)],
    "bounds_hi_plane_only": [("margin_bl_qh(R=20001,D=64,row=16421)", _F)],
    "ragged_last_row_dropped": [("code(4097,257,64,5)", _F), ("code(4097,33,128,7)", _F), ("code(4097,257,64,5)", _M)],
    "rows_past_R_listed": [("negative(1000,70,64,bf16)", _F), ("negative(1000,5,128,bf16)", _F), ("negative(255,70,64,bf16)", _M)],
    "first_tile_of_chunk_only": [("code(90001,770,64,5)", _F)],
    "chunk_first_row_dropped": [("code(4097,257,64,5)", _F), ("code(4097,64,128,7)", _F)],
    "padded_lane_appends": [("negative(1000,70,64,bf16)", _F), ("negative(1000,5,128,bf16)", _F)],
    "cap_minus_one": [("cap(128,D=64)", _F), ("cap(128,D=128)", _F), ("cap(128,D=64)", _M)],
    "cap_plus_one": [("cap(129,D=64)", _F), ("cap(129,D=128)", _F)],
    "overflow_not_flagged": [("cap(129,D=64)", _M), ("cap(129,D=128)", _F)],
    "skinny_forgets_idx_offset": [("code(4097,33,128,7,+1000003)", _F)],
    "k_block_dropped": [("code(4097,257,64,5)", _F), ("code(4097,33,128,7)", _F)],
    "moments_count_masked_rows": [("moment(4097,257,64,thr=-1.0)", _M)],
    "moments_wm_half_dropped": [("moment(4097,257,64,thr=2.5)", _M)],
    "moments_last_chunk_missing": [("moment(4097,257,64,thr=3.0)", _M)],
    "moments_max_from_survivors": [("cap(129,D=64)", _M)],
    "rescore_ignores_lo": [("code32(4097,257,64,5)", _F), ("code32(4097,33,128,7)", _F)],
    "ties_by_list_slot": [("cap(128,D=64)", _F), ("tight_tau(k=16,D=128,bf16)", _F)],
    "pool_truncated_silently": [("pool(6145,D=64)", _F), ("pool(6145,D=128)", _F)],
    "wrong_slot_struck": [("code(4097,257,64,5)", _F), ("code(4097,1,128,7)", _F)],
    "no_padding_beyond_candidates": [("small(100,3,64,128)", _F), ("small(100,3,128,128)", _F)],
    "rescore_forgets_idx_offset": [("code(4097,257,64,5,+1000003)", _F), ("code(4097,33,128,7,+1000003)", _F)],
}
MERGE_DEFECTS = ("merge_ties_by_shard", "merge_padding_first", "merge_last_shard_moments_dropped")
QSEL_LARGE = list(range(0, 770, 16))          # the large shape's defect run: every 16th query (the plan is the whole batch's)


def _unit(shape, seed):          # tests/test_gpu_path.py's data
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    return x / x.norm(dim=-1, keepdim=True)


_OLD = {}


def _old_data(R, M, D, k, dtype):
    if (R, M) not in _OLD:
        bank, q = _unit((R, D), 100 + R).to(dtype), _unit((M, D), 200 + M)
        _OLD[(R, M)] = bank, q, (q.double() @ bank.double().t()).numpy()
    return _OLD[(R, M)]


def _old_criterion(defect):
    """test_bank_search (moments form) and test_bank_search_filter_form (default form) of tests/test_gpu_path.py on the
    model with the defect: True = their assertions pass."""
    from test_gpu_path import _check_topk
    for R, M, D, k, dtype in ((1000, 48, 512, 5, torch.bfloat16), (4097, 257, 256, 32, torch.float32)):
        bank, q, Sx = _old_data(R, M, D, k, dtype)
        for want_moments in (True, False):
            form = B.form_of(R, M, D, dtype == torch.bfloat16, want_moments)
            r = B.model(bank, q, k, 0.05, form, 0, defect)
            if r.overflow:
                return False                                       # bank_status raises
            try:
                _check_topk(r.idx, r.sim.astype(np.float64), Sx, k, 1e-5)
                if want_moments:
                    mom = r.mom.astype(np.float64)
                    assert np.abs(mom[:, 0] - Sx.sum(1)).max() < 1e-3 * max(1.0, np.sqrt(R))
                    assert np.abs(mom[:, 1] - (Sx * Sx).sum(1)).max() < 1e-3 * max(1.0, R / D)
                    assert np.abs(mom[:, 2] - Sx.max(1)).max() < 1e-5
                    assert np.abs(mom[:, 3] - (Sx >= 0.05).sum(1)).max() <= 1
            except (AssertionError, IndexError):
                return False
    return True


def test_every_defect_is_caught():
    assert set(DEFECT_CASES) | set(MERGE_DEFECTS) == set(B.BANK_DEFECTS)
    lines = [f"{'defect':34s} {'old criterion':13s}  new probes"]
    for defect, cases in DEFECT_CASES.items():
        hits = []
        for name, kwargs in cases:
            assert name in B.CATALOG
            p, qsel = B.probe(name), None
            if not B.cpu_sized(name):
                qsel = QSEL_LARGE
            form = B.form_of(p.shape[0], p.shape[1], p.shape[2], p.bank.dtype == torch.bfloat16, **kwargs)
            if qsel is None:
                B.validate(p, form)
            clean = B.check_search(B.defective(None), p, form, kwargs, qsel=qsel)
            assert clean == [], clean
            fails = B.check_search(B.defective(defect), p, form, kwargs, qsel=qsel)
            hits.append(f"{'caught' if fails else 'PASSES'} {name} [{form}]")
            assert fails, (defect, name, form)
        old = "passes" if _old_criterion(defect) else "caught"
        lines.append(f"{defect:34s} {old:13s}  " + "; ".join(hits))
    for defect in MERGE_DEFECTS:
        fails = B.check_merge(lambda *a: B.merge_model(*a, defect=defect))
        lines.append(f"{defect:34s} {'(no old test)':13s}  {'caught' if fails else 'PASSES'} merge probe (h)")
        assert fails, defect
    assert B.check_merge(B.merge_model) == []
    print("\n" + "\n".join(lines))


def test_degenerate_bank_overflows_by_the_model():
    """tests/test_gpu_path.py::test_bank_search_overflow_is_reported asserts the outcome this model predicts for its bank of
    40 000 identical rows.  Grid-exact rows: decided in both forms, every list overflows.  Unit-vector rows (not exact): the
    one-product form clears tau by far more than the fp32 accumulation bound D * 2^-24 * sum |b||q|, the all-products form
    does not -- the model says so instead of guessing."""
    from test_gpu_path import overflow_bank
    for exact, want_moments, decided in ((True, True, True), (True, False, True), (False, False, True), (False, True, False)):
        bank, q, acc_err = overflow_bank(exact)
        r = B.model(bank, q, 5, 0.3, B.form_of(40000, 1, 128, True, want_moments), acc_err=acc_err)
        assert r.decided == decided and r.overflow and r.list_max > B.CAP, (exact, want_moments, r.decided, r.list_max)
        if exact:
            B.assert_exact(bank, q)
