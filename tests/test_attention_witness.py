"""CPU: the attention witnesses of tests/attn_witness.py are themselves right, and they catch what they are for.

1. ``spec_visible`` / ``model`` (no defect) equal the dense ``_attn_ref`` of test_gpu_kernels.py on dense configs, a
   per-sequence reference on packed configs, and the un-shared full-length sequences on prefix configs.
2. Every defect of ``attn_witness.DEFECTS`` -- injected into the fp64 model, whose output is then rounded to bf16 as the
   kernel's would be -- is flagged by the read-back or the needle at a case the GPU tests also run
   (tests/test_gpu_attention_witness.py runs every config of ``tower_configs()``).
3. The three ``_ex`` entry points are declared in include/tvc.h, bound in _lib.SIGNATURES and exported (what they refuse
   is checked on the host by tests/host_san_f16/driver.cpp and on the device by the GPU file).

The table below is what ``test_every_defect_is_caught`` prints (``pytest -s``): for each defect and case, whether the
read-back and the needle flag it, and -- measured, not asserted in either direction -- whether the existing random-input
criterion of the bf16 kernel (test_gpu_kernels.py::test_attention: max |err| < 3e-2 and mean |err| < 3e-3 on randn
inputs, here against the defect-free model at the same shape) flags it, with the max / mean error it sees.

defect                                   case                     read-back needle  random-input criterion (max / mean |err|)
last_key_dropped_in_last_query_block     full_dense_257           caught    caught  caught (3.2e-02 / 1.3e-04)
last_key_dropped_in_last_query_block     causal_packed_97         caught    caught  caught (9.2e-01 / 1.5e-03)
one_key_past_the_end                     full_packed_257          caught    caught  caught (2.3e+00 / 1.2e-02)
previous_sequence_last_row               causal_packed_97         caught    caught  caught (4.1e+00 / 8.1e-02)
causal_one_too_wide                      causal_dense_97          caught    caught  caught (6.7e-01 / 1.4e-02)
causal_one_too_narrow                    causal_dense_97          caught    caught  caught (8.7e-01 / 1.5e-02)
prefix_length_plus_1                     prefix_P17               caught    caught  caught (5.8e-01 / 1.9e-02)
prefix_length_minus_1                    prefix_P17               caught    caught  caught (1.0e+00 / 2.1e-02)
prefix_base_row_plus_1                   prefix_P17               caught    caught  caught (9.1e-01 / 3.3e-02)
prefix_base_row_minus_1                  prefix_long              caught    caught  caught (9.0e-01 / 5.0e-03)
own_tile_boundary_key_dropped            prefix_long              caught    caught  caught (2.5e-01 / 8.3e-03)
pooled_eot_query_from_T_minus_2          pool2_causal_packed_97   caught    caught  caught (1.4e+00 / 2.2e-01)
pooled_eot_query_from_T_minus_2          pool2_full_dense_257     passes    caught  caught (3.2e-01 / 5.2e-02)
pooled_output_row_plus_1                 pool2_causal_packed_97   caught    caught  caught (2.8e+00 / 4.8e-01)
pooled_output_row_minus_1                pool1_full_dense_257     caught    caught  caught (4.4e-01 / 1.1e-01)
head_reads_next_heads_v                  causal_dense_33          caught    caught  caught (4.8e+00 / 4.5e-01)
last_item_computed_as_the_item_before    full_dense_49            caught    caught  caught (1.2e+00 / 2.9e-02)

So at these shapes the 3e-2 bound on the maximum does see each of these defects once a test reaches the launch form at
all: the softmax weights of randn inputs are heavy-tailed, and a defect that touches a few hundred (query, key) pairs hits
a heavy one somewhere (the weakest is the first line, 3.2e-2 against 3e-2).  What the witnesses add is that the forms are
reached (before them no test ran the bf16 ragged form, any pfx form, either pooled form or the causal ragged split form
at kernel level), that the answer is exact instead of one draw away from the bound, and that a failure names the
(query, key, head) that is wrong.
"""
import re
import subprocess
from pathlib import Path

import pytest
import torch

import attn_witness as W
from test_gpu_kernels import _attn_ref

ROOT = Path(__file__).resolve().parents[1]
EX = {"tvc_attention_ex", "tvc_attention_split_ex", "tvc_sd_attention_ex"}
CONFIGS = {c.name: c for c in W.tower_configs()}


def _rand_qkv(cfg, seed=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((cfg.rows, 3 * cfg.width), generator=g).to(torch.bfloat16).float()


def _seq_ref(qkv, rows, heads, causal, n_queries):
    """Plain attention of ONE sequence given as a list of packed rows; the output of its last n_queries positions."""
    x = qkv[torch.tensor(rows)].double().view(len(rows), 3, heads, 64).permute(1, 2, 0, 3)
    s = x[0] @ x[1].transpose(-1, -2) * 0.125
    if causal:
        s = s + torch.full((len(rows), len(rows)), float("-inf"), dtype=torch.float64).triu(1)
    o = (s.softmax(-1) @ x[2]).permute(1, 0, 2).reshape(len(rows), heads * 64)
    return o[len(rows) - n_queries:]


@pytest.mark.parametrize("name", [n for n, c in CONFIGS.items() if c.pool_mode == 0])
def test_model_equals_plain_references(name):
    cfg = CONFIGS[name]
    qkv = _rand_qkv(cfg)
    got = W.model(qkv, cfg)
    st = cfg.starts
    if cfg.lens is None:
        ref = _attn_ref(qkv, cfg.n_seq, cfg.seq_len, cfg.heads, cfg.causal).double()
        vis = torch.block_diag(*[torch.ones(cfg.seq_len, cfg.seq_len).tril() if cfg.causal else torch.ones(cfg.seq_len, cfg.seq_len)
                                 for _ in range(cfg.n_seq)]).bool()
        assert torch.equal(W.spec_visible(cfg), vis)
        assert (got - ref).abs().max().item() < 1e-5                        # _attn_ref is fp32
        return
    for s in range(cfg.n_seq):
        own = list(range(st[s], st[s + 1]))
        P, b = cfg.prefix[s] if cfg.prefix is not None else (0, 0)
        full = list(range(st[b], st[b] + P)) + own                           # the un-shared sequence: the base's first P rows, then its own
        if own:
            assert (got[st[s]:st[s + 1]] - _seq_ref(qkv, full, cfg.heads, cfg.causal, len(own))).abs().max().item() < 1e-12


@pytest.mark.parametrize("name", [n for n, c in CONFIGS.items() if c.pool_mode != 0])
def test_pooled_model_is_the_pooled_row_of_the_full_output(name):
    cfg = CONFIGS[name]
    qkv = _rand_qkv(cfg)
    got = W.model(qkv, cfg)
    st = cfg.starts
    for s in range(cfg.n_seq):
        P, b = cfg.prefix[s] if cfg.prefix is not None else (0, 0)
        full = list(range(st[b], st[b] + P)) + list(range(st[s], st[s + 1]))
        pos = 0 if cfg.pool_mode == 1 else (len(full) - 1 if cfg.lens is not None else cfg.pool_rows[s] - st[s])
        assert (got[s] - _seq_ref(qkv, full, cfg.heads, cfg.causal, len(full))[pos]).abs().max().item() < 1e-12


def test_witnesses_pass_on_the_defect_free_model():
    for cfg in (CONFIGS["prefix_P17"], CONFIGS["pool2_prefix_empty"], CONFIGS["full_packed_49"]):
        for prec in W.PRECISION:
            assert W.check_both(lambda qkv: W.model(qkv, cfg), cfg, prec) == []


# defect -> the cases (all run on the GPU too) at which the witnesses must flag it
DEFECT_CASES = {
    "last_key_dropped_in_last_query_block": ("full_dense_257", "causal_packed_97"),
    "one_key_past_the_end": ("full_packed_257",),
    "previous_sequence_last_row": ("causal_packed_97",),
    "causal_one_too_wide": ("causal_dense_97",),
    "causal_one_too_narrow": ("causal_dense_97",),
    "prefix_length_plus_1": ("prefix_P17",),
    "prefix_length_minus_1": ("prefix_P17",),
    "prefix_base_row_plus_1": ("prefix_P17",),
    "prefix_base_row_minus_1": ("prefix_long",),
    "own_tile_boundary_key_dropped": ("prefix_long",),
    "pooled_eot_query_from_T_minus_2": ("pool2_causal_packed_97", "pool2_full_dense_257"),
    "pooled_output_row_plus_1": ("pool2_causal_packed_97",),
    "pooled_output_row_minus_1": ("pool1_full_dense_257",),
    "head_reads_next_heads_v": ("causal_dense_33",),
    "last_item_computed_as_the_item_before": ("full_dense_49",),
}


def test_every_defect_is_caught():
    assert set(DEFECT_CASES) == set(W.DEFECTS)
    b = W.PRECISION["bf16"]
    lines = [f"{'defect':40s} {'case':24s} read-back needle  random-input criterion (max / mean |err|)"]
    for defect in W.DEFECTS:
        for name in DEFECT_CASES[defect]:
            cfg = CONFIGS[name]
            broken = lambda qkv: W.model(qkv, cfg, defect).to(torch.bfloat16)
            rb = bool(W.check_readback(broken, cfg, b["rel"]))
            nd = bool(W.check_needle(broken, cfg, b["max_abs"], b["mean_abs"]))
            qkv = _rand_qkv(cfg)
            d = (broken(qkv).double() - W.model(qkv, cfg)).abs()
            rnd = not (d.max().item() < 3e-2 and d.mean().item() < 3e-3)
            lines.append(f"{defect:40s} {name:24s} {'caught' if rb else 'passes':9s} {'caught' if nd else 'passes':7s} "
                         f"{'caught' if rnd else 'PASSES'} ({d.max().item():.1e} / {d.mean().item():.1e})")
            assert rb or nd, (defect, name)
    print("\n" + "\n".join(lines))


def test_ex_entry_points_declared_bound_and_exported(pkg):
    h = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tvc.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(tvc_[a-z0-9_]+)\s*\(", h))
    assert EX <= declared
    assert EX <= set(pkg._lib.SIGNATURES)
    lib = pkg._lib.load()
    for name in EX:
        assert hasattr(lib, name)
    out = subprocess.run(["nm", "-D", "--defined-only", str(pkg._lib.LIB_PATH)], capture_output=True, text=True).stdout
    assert EX <= set(re.findall(r"\bT (tvc_[a-z0-9_]+)", out))
    assert lib.tvc_abi_version() == 4                        # additive: no ABI version bump
    for name in ("attention_ex", "attention_split_ex"):
        assert callable(getattr(pkg.TVCEngine, name))
