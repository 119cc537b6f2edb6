"""Witnesses of the attention BACKWARD (csrc/attention_bwd.hip; plain helper module: no GPU, no fixtures).

The kernel family differentiates the dense, non-causal tower attention of ``n_seq`` sequences of ``T`` rows: pass A
(lane = query) writes dQ and the per-(row, head) softmax statistics, pass B (lane = key) rebuilds P from those
statistics and writes dK and dV.  ``kernel`` arguments below are callables
``(qkv fp32 [rows, 3 * width], dout fp32 [rows, width]) -> dqkv [rows, 3 * width]`` (dQ | dK | dV, any float dtype).

* ``model``          fp64, from the documented semantics -- S = Q K^T / 8, P = softmax(S), dV = P^T dO, dP = dO V^T,
                     delta = rowsum(P o dP), dS = P o (dP - delta), dQ = dS K / 8, dK = dS^T Q / 8 -- with no tiles and no
                     lanes, but in the kernel's two passes: pass B takes log-sum-exp and delta from what pass A stored.
                     ``defect=`` applies one of ``BWD_DEFECTS``, each a one-line change (what a slipped index does).
* ``check_readback`` three exact probes.  Every input value is exact in bf16; pass r puts 1.0 into column c of head h of
                     packed row 64 r + ((c + 7 h) mod 64) (attn_witness's placement), ceil(rows / 64) passes.
                       "dv": q = k = v = 0, dO the indicator: P is uniform, dV[j, h, c] is exactly 0.0 where the indicator's
                             row is not a query of key j's sequence and 1 / T where it is; dQ = dK = 0 exactly.
                       "dq": q = 0, K the indicator, dO = e_0 on every row, V = e_0 on one key j* per sequence
                             (T - 1 - head, so that a head reading its neighbour's V shows): dP_ij = [j = j*],
                             delta = 1 / T, dQ[i, h, c] is exactly 0.0 for an invisible key row,
                             -1 / (8 T^2) for a visible one and (1 - 1 / T) / (8 T) for j*; dK = 0 exactly, dV = e_0.
                       "dk": k = 0, Q the indicator, the same dO and V: dK[j, h, c] is exactly 0.0 where the indicator's
                             query is not in key j's sequence, otherwise ([j = j*] - 1 / T) / (8 T); dQ = 0 exactly.
                     All three outputs of every launch are compared with ``model``: entries that are zero there must be
                     == 0, the others lie within ``rel`` (relative): each is one fp32 expression after at most two bf16
                     roundings (the packed P or dS, and the store).  A row counted twice doubles an entry, a foreign row
                     fills one that must be 0.0.
* ``check_needle``   K rows are attn_witness's +-1 codes, q_i = 8 k_target(i), dO rows spell (packed row, head) in bits of
                     +-1/4, V rows the same bits of +-1/64.  Allowed kinds: ``target`` is a permutation of the sequence's
                     rows, the target holds the softmax to within 288 e^-12 (margin asserted here), so dV[target(i)]
                     decodes to query i -- the hand-over of the statistics between the passes, checked at O(1) size.
                     Forbidden kinds: four queries of every sequence point at the nearest row of a neighbouring sequence;
                     all three outputs must equal ``model``, which never sees that row.  With these scales |dP| <= 1/4,
                     |dS_ij| <= P_ij / 2, and the rounded terms of an output sum to at most 2 in magnitude (dK: four
                     forbidden queries on one key, |q| = 8), so the kernel's own error stays below 2 * 2^-7 < 3e-2 (see
                     the value bound below): the forward needle's bf16 bounds hold.
* ``value_bound``    the element-wise bound of the value test, derived below.
* ``emulate``        the kernel's arithmetic in torch fp32 with ``.to(torch.bfloat16)`` exactly at its pack points.

The value bound.  The kernel rounds (csrc/attention_bwd.hip):
  pass A  P stays fp32 for lsum and delta = rowsum(P dP) / lsum; dS / 8 = P (dP - delta) / (8 lsum) goes to bf16
          (pack8) before the dQ product; dQ goes to bf16 at the store.
  pass B  P = exp2(s c - m c) / lsum goes to bf16 (pack8) before the dV product; dS / 8 goes to bf16 before the dK
          product; dK and dV go to bf16 at the store.
  The rest is fp32: MFMA accumulation of 64 (scores, dP) or at most 288 terms (outputs, sums), one fma and the hardware
  exp2 per score.
A bf16 rounding to nearest (8 significant bits) moves a value by at most 2^-8 of itself.  So with M = the sum of the absolute values of the
terms whose factor is packed -- M_dQ[i, c] = sum_j |dS_ij| |K_jc| / 8, M_dV[j, c] = sum_i P_ij |dO_ic|,
M_dK[j, c] = sum_i |dS_ij| |Q_ic| / 8 -- the pack moves an output by at most 2^-8 M, and the store by at most 2^-8 of
what was accumulated, itself at most (1 + 2^-8) M:  C16 = 2^-7 (1 + 2^-7).
The fp32 part F is small beside it but not nothing on spiky scores.  An unnormalised p_ij is off by (relative)
  e_ij <= 8 * 2^-24 A_ij [64-term accumulation of s, A_ij = sum_d |q_id| |k_jd|, in nats after / 8]
          + 2^-23 |S_ij - max_j S_ij| [the fma's rounding] + 2^-22 [v_exp_f32],
the row maximum's own rounding is common to p and lsum (and to both passes) and cancels; normalising at most doubles
it: eps_i = 2 max_j e_ij + 2^-15 (the 288-term sums).  With adP_ij = sum_d |dO_id| |V_jd| >= |dP_ij| and
adl_i = sum_k P_ik adP_ik >= |delta_i|, dS_ij is off by at most P_ij eps_i (adP_ij + 2 adl_i), and
  F_dQ = sum_j P_ij eps_i (adP_ij + 2 adl_i) |K_jc| / 8 + 2^-15 M_dQ,   F_dK likewise with |Q_ic|,
  F_dV = sum_i P_ij eps_i |dO_ic| + 2^-15 M_dV.
bound = C16 * M + F + 1e-30 (values below the normal range may be flushed).  Nothing in it was tuned on a GPU.  It is a
worst-case sum of absolute errors: an element with hundreds of comparable terms sits near 1 / sqrt(terms) of it, an element
that one term dominates (few keys, or a near one-hot softmax) can reach half of it through the store rounding alone, so the
worst ratio over a case is what tests/test_attn_bwd_witness.py prints and holds above 0.25.
"""
from __future__ import annotations

from functools import lru_cache
from typing import Callable, Dict, List, Optional, Tuple

import torch

import attn_witness as W

DH = W.DH
GRADS = ("dq", "dk", "dv")
C16 = 2.0 ** -7 * (1.0 + 2.0 ** -7)
SCALE_LOG2 = 0.125 * 1.4426950408889634        # ATT_SCALE_LOG2 (csrc/attn_frag.hpp)

# 1, 15 .. 49: dq<4> with one to four tiles; 64 | 65: the dq<4> | dq<18> switch; 80, 81: dq<18> with an odd tile count;
# 197, 256: dkv<18, 4, 0> up to 8 pairs; 257 .. 288: the straight-line dkv<18, 8, 9> with 17 and 18 tiles
SEQ_LENS = (1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 197, 256, 257, 272, 273, 288)
HEADS = 3                                      # a spare item in the last group of the XCD order
SPIKY = (49, 81, 257)
CONTRACT = (49, 65, 257)


def n_seq_of(T: int) -> int:
    return 3 if T < 197 else 2


BWD_DEFECTS = (
    "last_key_dropped_in_last_query_block_A",     # dQ and the statistics of the last 16 queries miss key T - 1
    "last_key_dropped_in_last_query_block_B",     # key T - 1 gets nothing from the last 16 queries
    "padded_key_copy_of_row_T_minus_1_A",         # T % 16 != 0: the clamped pad row counted as one more key
    "next_sequence_first_row_visible_A",
    "next_sequence_first_row_visible_B",          # the item also computes and stores that foreign key row
    "previous_sequence_last_row_visible_A",
    "previous_sequence_last_row_visible_B",
    "query_row_T_minus_1_counted_twice_B",        # T % 16 != 0: the clamped pad query contributes to dK / dV
    "last_query_block_missing_B",                 # dK / dV lack the last 16-query block
    "odd_last_key_tile_twice_in_dq_A",            # odd tile count: the unpaired tile's partner is itself, not zeros
    "item_reads_next_heads_v",
    "item_reads_next_heads_dout",
    "pass_b_statistics_of_next_head",
    "pass_b_statistics_of_row_plus_1",
    "last_item_repeats_the_item_before",          # the launch's last (sequence, head) item computes head - 1 again
    "dk_dv_columns_swapped",
    "head_halves_swapped",                        # the two 32-column halves of every stored 64-column head
)


def model(qkv: torch.Tensor, dout: torch.Tensor, T: int, n_seq: int, heads: int, defect: Optional[str] = None,
          parts: bool = False):
    """fp64 dqkv [rows, 3 * width]; ``parts``: also (M, F) of the module docstring, same shape."""
    assert defect is None or defect in BWD_DEFECTS, defect
    rows, w = n_seq * T, heads * DH
    assert tuple(qkv.shape) == (rows, 3 * w) and tuple(dout.shape) == (rows, w)
    x = qkv.double()
    Q, K, V = (x[:, i * w:(i + 1) * w].reshape(rows, heads, DH) for i in range(3))
    dO = dout.double().reshape(rows, heads, DH)
    out = torch.zeros((rows, 3, heads, DH), dtype=torch.float64)
    M, F = torch.zeros_like(out), torch.zeros_like(out)
    lse, delta = torch.zeros((rows, heads), dtype=torch.float64), torch.zeros((rows, heads), dtype=torch.float64)
    eps, adl = torch.zeros_like(lse), torch.zeros_like(lse)
    NT, ragged = (T + 15) // 16, T % 16 != 0
    last = (T - 1) // 16 * 16                                    # first row of the last 16-row block
    items = [(s, h) for s in range(n_seq) for h in range(heads)]
    one = lambda r: torch.tensor([r], dtype=torch.int64)

    def src(s, h):
        """the heads an item reads q / k, v, dO and the statistics from"""
        hq = hv = hd = hs = h
        if defect == "last_item_repeats_the_item_before" and (s, h) == items[-1] and heads > 1:
            hq = hv = hd = hs = h - 1
        if defect == "item_reads_next_heads_v":
            hv = (h + 1) % heads
        if defect == "item_reads_next_heads_dout":
            hd = (h + 1) % heads
        if defect == "pass_b_statistics_of_next_head":
            hs = (h + 1) % heads
        return hq, hv, hd, hs

    # ---- pass A: dQ, log-sum-exp and delta of every (row, head)
    for s, h in items:
        r0 = s * T
        own = torch.arange(r0, r0 + T)
        hq, hv, hd, _ = src(s, h)
        keys = own
        if defect == "padded_key_copy_of_row_T_minus_1_A" and ragged:
            keys = torch.cat([own, one(r0 + T - 1)])
        if defect == "next_sequence_first_row_visible_A" and s + 1 < n_seq:
            keys = torch.cat([own, one(r0 + T)])
        if defect == "previous_sequence_last_row_visible_A" and s > 0:
            keys = torch.cat([one(r0 - 1), own])
        q, do, k, v = Q[own, hq], dO[own, hd], K[keys, hq], V[keys, hv]
        S = q @ k.t() * 0.125
        if defect == "last_key_dropped_in_last_query_block_A" and T > 1:
            S[last:, T - 1] = float("-inf")
        L = torch.logsumexp(S, 1)
        P = torch.exp(S - L[:, None])
        dP = do @ v.t()
        dl = (P * dP).sum(1)
        dS = P * (dP - dl[:, None])
        dq = dS @ k * 0.125
        if defect == "odd_last_key_tile_twice_in_dq_A" and NT % 2 == 1:
            dq = dq + dS[:, 16 * (NT - 1):] @ k[16 * (NT - 1):] * 0.125
        out[own, 0, h], lse[own, h], delta[own, h] = dq, L, dl
        if parts:
            A = q.abs() @ k.abs().t()
            e = 8 * 2.0 ** -24 * A + 2.0 ** -23 * (S - S.max(1, keepdim=True).values).abs() + 2.0 ** -22
            ei = 2 * e.max(1).values + 2.0 ** -15
            adP = do.abs() @ v.abs().t()
            al = (P * adP).sum(1)
            M[own, 0, h] = dS.abs() @ k.abs() * 0.125
            F[own, 0, h] = (P * ei[:, None] * (adP + 2 * al[:, None])) @ k.abs() * 0.125 + 2.0 ** -15 * M[own, 0, h]
            eps[own, h], adl[own, h] = ei, al

    # ---- pass B: dK, dV from the stored statistics; stores to a foreign row land after every item's own
    late = []
    for s, h in items:
        r0 = s * T
        own = torch.arange(r0, r0 + T)
        hq, hv, hd, hs = src(s, h)
        qrows = own
        if defect == "query_row_T_minus_1_counted_twice_B" and ragged:
            qrows = torch.cat([own, one(r0 + T - 1)])
        if defect == "last_query_block_missing_B":
            qrows = own[:last]
        srow = (qrows + 1).clamp(max=rows - 1) if defect == "pass_b_statistics_of_row_plus_1" else qrows
        q, do = Q[qrows, hq], dO[qrows, hd]

        def grads(keys):
            k, v = K[keys, hq], V[keys, hv]
            P = torch.exp(q @ k.t() * 0.125 - lse[srow, hs][:, None])
            if defect == "last_key_dropped_in_last_query_block_B" and T > 1 and len(keys) == T:
                P[last:, T - 1] = 0.0
            dP = do @ v.t()
            dS = P * (dP - delta[srow, hs][:, None])
            return P, dS, v

        P, dS, v = grads(own)
        out[own, 1, h], out[own, 2, h] = dS.t() @ q * 0.125, P.t() @ do
        if parts:
            adP = do.abs() @ v.abs().t()
            ei, al = eps[srow, hs][:, None], adl[srow, hs][:, None]
            M[own, 1, h], M[own, 2, h] = dS.abs().t() @ q.abs() * 0.125, P.t() @ do.abs()
            F[own, 1, h] = (P * ei * (adP + 2 * al)).t() @ q.abs() * 0.125 + 2.0 ** -15 * M[own, 1, h]
            F[own, 2, h] = (P * ei).t() @ do.abs() + 2.0 ** -15 * M[own, 2, h]
        foreign = None
        if defect == "next_sequence_first_row_visible_B" and s + 1 < n_seq:
            foreign = one(r0 + T)
        if defect == "previous_sequence_last_row_visible_B" and s > 0:
            foreign = one(r0 - 1)
        if foreign is not None:
            P, dS, _ = grads(foreign)
            late.append((foreign, h, dS.t() @ q * 0.125, P.t() @ do))
    for row, h, dk, dv in late:
        out[row, 1, h], out[row, 2, h] = dk, dv

    if defect == "dk_dv_columns_swapped":
        out = out[:, [0, 2, 1]]
    if defect == "head_halves_swapped":
        out = torch.cat([out[..., DH // 2:], out[..., :DH // 2]], -1)
    res = out.reshape(rows, 3 * w)
    return (res, M.reshape(rows, 3 * w), F.reshape(rows, 3 * w)) if parts else res


def value_bound(M: torch.Tensor, F: torch.Tensor) -> torch.Tensor:
    return C16 * M + F + 1e-30


def emulate(qkv: torch.Tensor, dout: torch.Tensor, T: int, n_seq: int, heads: int) -> torch.Tensor:
    """The kernel's arithmetic in fp32 (sums in torch's order, not the MFMA's), bf16 exactly where the kernel packs."""
    rows, w = n_seq * T, heads * DH
    bf = lambda t: t.to(torch.bfloat16).float()
    x, g = qkv.float(), dout.float()
    assert torch.equal(bf(x), x) and torch.equal(bf(g), g)
    Q, K, V = (x[:, i * w:(i + 1) * w].reshape(rows, heads, DH) for i in range(3))
    dO = g.reshape(rows, heads, DH)
    out = torch.zeros((rows, 3, heads, DH))
    c = torch.tensor(SCALE_LOG2, dtype=torch.float32)
    for s in range(n_seq):
        own = torch.arange(s * T, s * T + T)
        for h in range(heads):
            q, k, v, do = Q[own, h], K[own, h], V[own, h], dO[own, h]
            sc = q @ k.t()                                          # unscaled, as the MFMA leaves it
            mxs = sc.max(1, keepdim=True).values * c
            p = torch.exp2(sc * c - mxs)
            inv = 1.0 / p.sum(1, keepdim=True)
            dP = do @ v.t()
            dlt = (p * dP).sum(1, keepdim=True) * inv
            e = bf(p * (0.125 * inv) * (dP - dlt))                  # pass A: dS / 8 packed; P itself never is
            out[own, 0, h] = bf(e @ k)
            pB = p * inv                                            # pass B: P from the statistics
            pb, sb = bf(pB), bf(pB * 0.125 * (dP - dlt))
            out[own, 1, h], out[own, 2, h] = bf(sb.t() @ q), bf(pb.t() @ do)
    return out.reshape(rows, 3 * w)


# ------------------------------------------------------------------------------------------------- reporting
def _where(idx: int, T: int, heads: int) -> str:
    w = heads * DH
    return f"{GRADS[idx // w]} head {idx % w // DH} column {idx % DH}"


def _compare(tag: str, got: torch.Tensor, want: torch.Tensor, T: int, heads: int, rel: float, fails: List[str], limit: int):
    """model zero <-> kernel == 0 (NaN fails), the rest within rel."""
    got = got.double().cpu()
    zero = want.abs() < 1e-12                                       # the smallest probe value is 1 / (8 * 288^2) = 1.5e-6
    bad = (zero & ~(got == 0)) | (~zero & ~((got - want).abs() <= rel * want.abs()))
    for i, c in bad.nonzero()[:max(limit - len(fails), 0)].tolist():
        fails.append(f"{tag}: row {i} (sequence {i // T}, position {i % T}) {_where(c, T, heads)}: got {got[i, c].item()!r}, "
                     f"model {'exactly 0' if zero[i, c] else repr(want[i, c].item())}")
    if int(bad.sum()) > limit and len(fails) == limit:
        fails.append(f"{tag}: ... ({int(bad.sum())} mismatches in this launch)")


# ------------------------------------------------------------------------------------------------- exact read-backs
PROBES = ("dv", "dq", "dk")


def readback_passes(T: int, n_seq: int) -> int:
    return (n_seq * T + DH - 1) // DH


def readback_input(probe: str, T: int, n_seq: int, heads: int, r: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(qkv, dout) of pass r."""
    rows, w = n_seq * T, heads * DH
    pr = W._probe_rows(r, heads)
    ind = torch.zeros((rows, w))
    for h in range(heads):
        ok = pr[h] < rows
        ind[pr[h][ok], h * DH + torch.arange(DH)[ok]] = 1.0
    qkv, dout = torch.zeros((rows, 3 * w)), torch.zeros((rows, w))
    if probe == "dv":
        return qkv, ind
    dout[:, ::DH] = 1.0                                             # e_0 in every head
    hh = torch.arange(heads)
    jstar = torch.arange(n_seq)[:, None] * T + (T - 1 - hh).clamp(min=0)[None, :]       # [n_seq, heads]
    qkv[jstar, 2 * w + hh[None, :] * DH] = 1.0
    if probe == "dq":
        qkv[:, w:2 * w] = ind
    else:
        qkv[:, :w] = ind
    return qkv, dout


@lru_cache(maxsize=64)           # one length's passes of all three probes; shared, never modified
def _readback_model(probe: str, T: int, n_seq: int, heads: int, r: int) -> torch.Tensor:
    return model(*readback_input(probe, T, n_seq, heads, r), T, n_seq, heads)


def check_readback(kernel: Callable, probe: str, T: int, n_seq: int, heads: int, rel: float, limit: int = 12) -> List[str]:
    fails: List[str] = []
    for r in range(readback_passes(T, n_seq)):
        qkv, dout = readback_input(probe, T, n_seq, heads, r)
        _compare(f"T {T} {probe} read-back pass {r}", kernel(qkv, dout), _readback_model(probe, T, n_seq, heads, r), T, heads,
                 rel, fails, limit)
        if len(fails) >= limit:
            break
    return fails


# ------------------------------------------------------------------------------------------------- needle
ALLOWED_KINDS = ("reverse", "shift_17")
FORBIDDEN_KINDS = ("previous_sequence_last_row", "next_sequence_first_row")
DOUT_SCALE, V_SCALE = 0.25, 1.0 / 64


@lru_cache(maxsize=None)
def needle_input(T: int, n_seq: int, heads: int, kind: str):
    """(qkv, dout, target row per query row, target visible per query row); cached and shared, never modified.
    Asserts the 12-nat margin of every visible target."""
    cfg = W.Config("bwd", T, n_seq, heads, causal=False)
    k, bits = W._codes(cfg)                                         # [rows, heads, 64] each
    rows, w = cfg.rows, cfg.width
    i = torch.arange(T)
    tgt = torch.cat([s * T + ((i + 17) % T if kind == "shift_17" else T - 1 - i) for s in range(n_seq)])
    if kind in FORBIDDEN_KINDS:
        for s in range(n_seq):
            f = s * T - 1 if kind == "previous_sequence_last_row" else s * T + T
            if 0 <= f < rows:
                tgt[s * T + torch.tensor(sorted({0, T - 1, min(16, T - 1), T // 2}))] = f
    seq = torch.arange(rows) // T
    tvis = seq[tgt] == seq
    qkv = torch.cat([W.NEEDLE_A * k[tgt].reshape(rows, w), k.reshape(rows, w), V_SCALE * bits.reshape(rows, w)], 1)
    for h in range(heads):
        s = (qkv[:, h * DH:(h + 1) * DH] @ k[:, h].t()) * 0.125
        s = torch.where(seq[:, None] == seq[None, :], s, torch.full((), float("-inf")))
        top = s[torch.arange(rows), tgt].clone()
        s[torch.arange(rows), tgt] = float("-inf")
        margin = top - s.max(1).values
        assert (margin[tvis] >= W.NEEDLE_MARGIN).all(), (T, kind, h, margin[tvis].min().item())
    return qkv, DOUT_SCALE * bits.reshape(rows, w), tgt, tvis


@lru_cache(maxsize=None)
def _needle_model(T: int, n_seq: int, heads: int, kind: str) -> torch.Tensor:
    qkv, dout, _, _ = needle_input(T, n_seq, heads, kind)
    return model(qkv, dout, T, n_seq, heads)


def check_needle(kernel: Callable, T: int, n_seq: int, heads: int, max_abs: float, mean_abs: Optional[float],
                 kinds=ALLOWED_KINDS + FORBIDDEN_KINDS, limit: int = 12) -> List[str]:
    fails: List[str] = []
    rows, w = n_seq * T, heads * DH
    for kind in kinds:
        qkv, dout, tgt, tvis = needle_input(T, n_seq, heads, kind)
        got = kernel(qkv, dout).double().cpu()
        if kind in ALLOWED_KINDS:                                  # dV[target(i)] spells (i, head)
            row, head, clean = W._decode(got[:, 2 * w:].reshape(rows, heads, DH))
            query = torch.empty(rows, dtype=torch.int64)
            query[tgt] = torch.arange(rows)
            wrong = ~(clean & (row == query[:, None]) & (head == torch.arange(heads)))
            for j, h in wrong.nonzero()[:max(limit - len(fails), 0)].tolist():
                fails.append(f"T {T} needle [{kind}]: dV of row {j} head {h} is the target of query row {int(query[j])} and decodes "
                             f"to (row {int(row[j, h])}, head {int(head[j, h])}{'' if clean[j, h] else ', unclean'})")
        d = (got - _needle_model(T, n_seq, heads, kind)).abs()
        for g, name in enumerate(GRADS):
            dg = d[:, g * w:(g + 1) * w]
            if not (dg.max().item() < max_abs and (mean_abs is None or dg.mean().item() < mean_abs)) and len(fails) < limit:
                i = int(dg.max(1).values.argmax())
                fails.append(f"T {T} needle [{kind}]: {name} max |out - model| {dg.max().item():.3e} (bound {max_abs:.1e}), mean "
                             f"{dg.mean().item():.3e} (bound {mean_abs}); worst row {i}, whose query points at row {int(tgt[i])}")
    return fails


def check_all(kernel: Callable, T: int, n_seq: int, heads: int) -> List[str]:
    """The three read-backs and the needle; readable failures, [] when the kernel is right."""
    b = W.PRECISION["bf16"]
    fails: List[str] = []
    for probe in PROBES:
        fails += check_readback(kernel, probe, T, n_seq, heads, b["rel"])
    return fails + check_needle(kernel, T, n_seq, heads, b["max_abs"], b["mean_abs"])


# ------------------------------------------------------------------------------------------------- values
@lru_cache(maxsize=None)
def value_input(T: int, n_seq: int, heads: int, spiky: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Random bf16 inputs (those of test_gpu_grad.py: scores within about +-3 nats); ``spiky``: q times 32, scores span
    tens of nats and most rows' softmax is near one-hot.  Cached and shared, never modified."""
    g = torch.Generator().manual_seed(T)
    w = heads * DH
    qkv = (torch.randn(n_seq * T, 3 * w, generator=g) * 0.7).to(torch.bfloat16).float()
    dout = torch.randn(n_seq * T, w, generator=g).to(torch.bfloat16).float()
    if spiky:
        qkv[:, :w] *= 32.0
    return qkv, dout


@lru_cache(maxsize=None)
def value_reference(T: int, n_seq: int, heads: int, spiky: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(fp64 model, bound) of ``value_input``; computed once, shared, never modified."""
    want, M, F = model(*value_input(T, n_seq, heads, spiky), T, n_seq, heads, parts=True)
    return want, value_bound(M, F)


def value_cases() -> List[Tuple[int, bool]]:
    return [(T, False) for T in SEQ_LENS] + [(T, True) for T in SPIKY]


def check_values(got: torch.Tensor, T: int, n_seq: int, heads: int, spiky: bool = False) -> Tuple[List[str], Dict[str, float]]:
    """|got - model| <= bound for every element; failures as text, and the worst |err| / bound per output."""
    want, bound = value_reference(T, n_seq, heads, spiky)
    got = got.double().cpu()
    w = heads * DH
    ratio = (got - want).abs() / bound
    fails: List[str] = []
    worst: Dict[str, float] = {}
    tag = f"T {T}{' spiky' if spiky else ''}"
    if not torch.isfinite(got).all():
        fails.append(f"{tag}: {int((~torch.isfinite(got)).sum())} outputs are not finite")
    for g, name in enumerate(GRADS):
        r = ratio[:, g * w:(g + 1) * w]
        bad = ~(r <= 1.0)
        worst[name] = r.nan_to_num(nan=float("inf")).max().item()
        for i, c in bad.nonzero()[:4].tolist():
            c += g * w
            fails.append(f"{tag}: row {i} (sequence {i // T}, position {i % T}) {_where(c, T, heads)}: got {got[i, c].item()!r}, "
                         f"model {want[i, c].item()!r}, bound {bound[i, c].item():.3e} (ratio {ratio[i, c].item():.2f})")
        if int(bad.sum()) > 4:
            fails.append(f"{tag}: ... {name} has {int(bad.sum())} elements outside the bound")
    return fails, worst
