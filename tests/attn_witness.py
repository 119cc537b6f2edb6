"""Exact witnesses of WHICH KEYS A QUERY SEES in the attention kernels (plain helper module: no GPU, no fixtures).

A mask is a yes / no property, so it is read back exactly instead of being inferred from a tolerance on random inputs:

* ``Config``           one launch of the tower attention (dense / packed rows, shared prefixes, causal, pooled forms).
* ``spec_visible``     bool [output rows, packed rows]: output row i sees packed row r.  Written from the documented
                       semantics (csrc/kernels.hpp "attention.hip", the comments on launch_attention_t and on the pooled
                       form in csrc/attention.hip), in terms of sequences and positions -- no tiles, no lanes.
* ``model``            fp64 attention over ``spec_visible``; ``defect=`` applies one of ``DEFECTS``, each a one-line change
                       of the visibility matrix or of the row / head mapping (what a slipped index in a kernel does).
* ``check_readback``   visibility read-back: q = 0 (all scores exactly 0), V an indicator.  In pass r packed row
                       64 r + ((c + 7 h) mod 64) carries 1.0 in column c of head h, so output[i, h, c] is exactly 0.0 where
                       the row is invisible and 1 / n_i where visible; ceil(rows / 64) passes read the whole matrix.
* ``check_needle``     K rows are +-1 codes, V rows spell (packed row, head) in +-1 bits, q_i = 8 k_target(i): a visible
                       target takes the whole softmax (>= 12 nats over every other key, asserted here) and the output
                       decodes to it; a forbidden target (the nearest INVISIBLE rows) must leave the output equal to
                       ``model``, which never sees it.
* ``sd_*``             the same two witnesses for the streaming kernel (separate q / k / v, n samples, any head dim).
                       The needle does NOT check the streaming kernel's softmax VALUES: its 12-nat margin makes
                       everything accumulated before a move of the reference e^-12 of the result, so a wrong rescale
                       passes it.  That is tests/sd_attn_ref.py and tests/test_gpu_sd_attention_values.py.
                       Nor do the two witnesses check the TOWER kernels' softmax values: they stand at its two ends (q = 0,
                       every weight 1 / n; the needle, one weight 1), where a wrong scale or a stale denominator changes
                       nothing.  That is tests/tower_attn_ref.py and tests/test_gpu_tower_attention_values.py: every
                       config below, per-element fp64 bounds, for attention.hip, the split and the fp32 kernel.

``kernel`` arguments are callables ``qkv fp32 [rows, 3 * width] -> out [output rows, width]`` (any float dtype); every
probe value is exact in bf16 and fp16.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from functools import lru_cache
from typing import Callable, List, Optional, Sequence, Tuple

import torch

DH = 64
NEEDLE_A = 8.0          # q = a * k_target: scores are <k_t, k_j> * a / 8 = the code correlation itself, the target's is 64
NEEDLE_MARGIN = 12.0    # nats between the target and every other visible key: they share <= 288 e^-12 = 1.8e-3 of the softmax

# Value bounds from the storage formats (a visible read-back entry is 1 / n_i after at most two roundings), and for the
# needle's forbidden targets the bounds the existing parity tests of each precision use on random inputs
# (test_gpu_kernels.py::test_attention, test_gpu_fp16_mode.py, test_gpu_fp32_mode.py): a leak is an O(1) error.
PRECISION = {
    "bf16": dict(rel=2.0 ** -7, max_abs=3e-2, mean_abs=3e-3),
    "fp16": dict(rel=2.0 ** -9, max_abs=2e-3, mean_abs=None),
    "split": dict(rel=1e-4, max_abs=5e-5, mean_abs=None),
    "fp32": dict(rel=1e-6, max_abs=5e-6, mean_abs=None),
}


@dataclass(frozen=True)
class Config:
    name: str
    seq_len: int                                    # the launch's seq_len: dense length, or the bound on prefix + own rows
    n_seq: int
    heads: int = 3
    causal: bool = True
    lens: Optional[Tuple[int, ...]] = None          # packed: own rows per sequence (None = dense n_seq x seq_len)
    prefix: Optional[Tuple[Tuple[int, int], ...]] = None   # per sequence (P, base sequence): P rows of the base's are shared
    pool_mode: int = 0
    pool_rows: Optional[Tuple[int, ...]] = None     # pool_mode 2 on dense rows: the packed row of every sequence's EOT

    def __post_init__(self):
        if self.lens is not None:
            assert len(self.lens) == self.n_seq
        if self.prefix is not None:
            assert self.lens is not None and self.causal and len(self.prefix) == self.n_seq
            for (P, b), own in zip(self.prefix, self.lens):
                assert 0 <= P <= self.lens[b] and (P == 0 or self.prefix[b][0] == 0) and 1 <= P + own <= self.seq_len
        elif self.lens is not None:
            assert all(1 <= n <= self.seq_len for n in self.lens)
        assert self.pool_rows is None or (self.pool_mode == 2 and self.lens is None)

    @property
    def width(self) -> int:
        return self.heads * DH

    @property
    def starts(self) -> List[int]:
        own = self.lens if self.lens is not None else (self.seq_len,) * self.n_seq
        out = [0]
        for n in own:
            out.append(out[-1] + n)
        return out

    @property
    def rows(self) -> int:
        return self.starts[-1]

    @property
    def n_out(self) -> int:
        return self.n_seq if self.pool_mode else self.rows

    def starts_tensor(self) -> Optional[torch.Tensor]:
        return None if self.lens is None else torch.tensor(self.starts, dtype=torch.int32)

    def pfx_tensor(self) -> Optional[torch.Tensor]:
        """int32 [2 * n_seq] as kernels.hpp documents it: [s] = prefix length, [n_seq + s] = packed row of the prefix's position 0."""
        if self.prefix is None:
            return None
        st = self.starts
        return torch.tensor([P for P, _ in self.prefix] + [st[b] for _, b in self.prefix], dtype=torch.int32)

    def pool_row_tensor(self) -> Optional[torch.Tensor]:
        return None if self.pool_rows is None else torch.tensor(self.pool_rows, dtype=torch.int32)


DEFECTS = (
    "last_key_dropped_in_last_query_block",   # the sequence's last key invisible to its last 16-query block
    "one_key_past_the_end",                   # the next sequence's first row visible (where the causal rule allows position T)
    "previous_sequence_last_row",             # the row before the sequence's first own row visible
    "causal_one_too_wide",                    # key position qpos + 1 visible, queries at positions >= 16 only
    "causal_one_too_narrow",                  # key position qpos invisible, queries at positions >= 16 only
    "prefix_length_plus_1",
    "prefix_length_minus_1",
    "prefix_base_row_plus_1",
    "prefix_base_row_minus_1",
    "own_tile_boundary_key_dropped",          # key positions P + 16 k (k >= 1) invisible when P % 16 != 0
    "pooled_eot_query_from_T_minus_2",
    "pooled_output_row_plus_1",
    "pooled_output_row_minus_1",
    "head_reads_next_heads_v",
    "last_item_computed_as_the_item_before",  # the launch's last (sequence, head) item repeats head - 1 of its sequence
)


@dataclass
class Plan:
    """What every output row computes: where it is stored, which packed row its query comes from, which rows it sees."""
    out_row: torch.Tensor      # int64 [m]: row of the output buffer (rows never named stay unwritten)
    q_row: torch.Tensor        # int64 [m]
    seq: torch.Tensor          # int64 [m]
    vis: torch.Tensor          # bool [m, rows]
    q_head: List[List[int]]    # [seq][h] -> head whose q / k columns the item reads
    v_head: List[List[int]]    # [seq][h] -> head whose v columns the item reads


@lru_cache(maxsize=None)
def _plan(cfg: Config, defect: Optional[str] = None) -> Plan:
    """Cached: the tensors of a Plan are shared and never modified."""
    assert defect is None or defect in DEFECTS, defect
    st, rows = cfg.starts, cfg.rows
    out_row, q_row, seqs, vis = [], [], [], []
    for s in range(cfg.n_seq):
        row0, own = st[s], st[s + 1] - st[s]
        P, prow0 = (cfg.prefix[s][0], st[cfg.prefix[s][1]]) if cfg.prefix is not None else (0, 0)
        if P > 0:
            P += {"prefix_length_plus_1": 1, "prefix_length_minus_1": -1}.get(defect, 0)
            prow0 += {"prefix_base_row_plus_1": 1, "prefix_base_row_minus_1": -1}.get(defect, 0)
        T = P + own
        # the sequence: P shared rows of its base (keys only), then its own rows (keys and queries)
        row_of = [prow0 + t if t < P else row0 + (t - P) for t in range(T)]
        if cfg.pool_mode == 0:
            queries = [(P + j, row0 + j) for j in range(own)]              # (position, output row): every own row
        else:
            pos = 0 if cfg.pool_mode == 1 else (T - 1 if cfg.lens is not None else cfg.pool_rows[s] - row0)
            if cfg.pool_mode == 2 and defect == "pooled_eot_query_from_T_minus_2" and pos >= 1:
                pos -= 1
            o = s + {"pooled_output_row_plus_1": 1, "pooled_output_row_minus_1": -1}.get(defect, 0)
            queries = [(pos, o)] if 0 <= o < cfg.n_seq else []             # the pooled token only, compact row s
        for pos, o in queries:
            v = torch.zeros(rows, dtype=torch.bool)
            last = pos if cfg.causal else T - 1                             # causal: keys up to the query's own position
            if defect == "causal_one_too_wide" and cfg.causal and pos >= 16:
                last = min(pos + 1, T - 1)
            seen = torch.tensor(row_of[:last + 1], dtype=torch.int64)
            v[seen[(seen >= 0) & (seen < rows)]] = True
            if defect == "causal_one_too_narrow" and cfg.causal and pos >= 16:
                v[row_of[pos]] = False
            if defect == "last_key_dropped_in_last_query_block" and pos - P >= (own - 1) // 16 * 16 and v.sum() > 1:
                v[row_of[T - 1]] = False
            if defect == "one_key_past_the_end" and not cfg.causal and row0 + own < rows:
                v[row0 + own] = True
            if defect == "previous_sequence_last_row" and row0 >= 1:
                v[row0 - 1] = True
            if defect == "own_tile_boundary_key_dropped" and P % 16 != 0:
                for t in range(P + 16, last + 1, 16):
                    if v.sum() > 1:
                        v[row_of[t]] = False
            out_row.append(o); q_row.append(row_of[pos]); seqs.append(s); vis.append(v)
    qh = [list(range(cfg.heads)) for _ in range(cfg.n_seq)]
    vh = [list(range(cfg.heads)) for _ in range(cfg.n_seq)]
    if defect == "head_reads_next_heads_v":
        vh = [[(h + 1) % cfg.heads for h in range(cfg.heads)] for _ in range(cfg.n_seq)]
    if defect == "last_item_computed_as_the_item_before" and cfg.heads > 1:
        qh[-1][-1] = vh[-1][-1] = cfg.heads - 2
    return Plan(torch.tensor(out_row, dtype=torch.int64), torch.tensor(q_row, dtype=torch.int64),
                torch.tensor(seqs, dtype=torch.int64), torch.stack(vis) if vis else torch.zeros((0, rows), dtype=torch.bool), qh, vh)


def spec_visible(cfg: Config) -> torch.Tensor:
    """bool [output rows, packed rows]; every output row of a valid Config is written and sees at least one key."""
    p = _plan(cfg)
    out = torch.zeros((cfg.n_out, cfg.rows), dtype=torch.bool)
    out[p.out_row] = p.vis
    assert sorted(p.out_row.tolist()) == list(range(cfg.n_out)) and out.any(1).all()
    return out


def model(qkv: torch.Tensor, cfg: Config, defect: Optional[str] = None) -> torch.Tensor:
    """fp64 attention of qkv [rows, 3 * width] (q | k | v) over the plan; unwritten output rows are zero."""
    p = _plan(cfg, defect)
    w = cfg.width
    x = qkv.double()
    out = torch.zeros((cfg.n_out, w), dtype=torch.float64)
    neg = torch.full((), float("-inf"), dtype=torch.float64)
    seq_l = p.seq.tolist()
    for h in range(cfg.heads):
        qh = torch.tensor([p.q_head[s][h] for s in seq_l], dtype=torch.int64)
        vh = torch.tensor([p.v_head[s][h] for s in seq_l], dtype=torch.int64)
        cols = torch.arange(DH)
        xq = x[p.q_row[:, None], qh[:, None] * DH + cols]                               # [m, 64]
        res = torch.zeros((len(seq_l), DH), dtype=torch.float64)
        for kh in sorted(set(qh.tolist())):
            for vv in sorted(set(vh[qh == kh].tolist())):
                m = (qh == kh) & (vh == vv)
                s = xq[m] @ x[:, w + kh * DH: w + (kh + 1) * DH].t() * 0.125
                s = torch.where(p.vis[m], s, neg)
                res[m] = s.softmax(-1) @ x[:, 2 * w + vv * DH: 2 * w + (vv + 1) * DH]
        out[p.out_row, h * DH:(h + 1) * DH] = res
    return out


# ------------------------------------------------------------------------------------------- visibility read-back
def readback_passes(cfg: Config) -> int:
    return (cfg.rows + DH - 1) // DH


def _probe_rows(r: int, heads: int) -> torch.Tensor:
    """int64 [heads, 64]: the packed row whose value sits in column c of head h in pass r."""
    c = torch.arange(DH)
    return torch.stack([DH * r + (c + 7 * h) % DH for h in range(heads)])


def readback_input(cfg: Config, r: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(1000 + r)
    w = cfg.width
    qkv = torch.zeros((cfg.rows, 3 * w))
    qkv[:, w:2 * w] = torch.randn((cfg.rows, w), generator=g).to(torch.bfloat16).float()       # K: random, finite, never matters
    pr = _probe_rows(r, cfg.heads)
    for h in range(cfg.heads):
        ok = pr[h] < cfg.rows
        qkv[pr[h][ok], 2 * w + h * DH + torch.arange(DH)[ok]] = 1.0
    return qkv


def check_readback(kernel: Callable[[torch.Tensor], torch.Tensor], cfg: Config, rel: float, limit: int = 12) -> List[str]:
    """Failures as text: every (output row, packed row, head) whose visibility differs from the spec, and every visible
    entry further than ``rel`` (relative) from 1 / n_i."""
    vis = spec_visible(cfg)
    n_i = vis.sum(1).double()
    fails: List[str] = []
    for r in range(readback_passes(cfg)):
        got = kernel(readback_input(cfg, r)).double().cpu().view(cfg.n_out, cfg.heads, DH)
        pr = _probe_rows(r, cfg.heads)
        inside = pr < cfg.rows
        want = vis[:, pr.clamp(max=cfg.rows - 1)] & inside                    # [n_out, heads, 64]
        bad = (got != 0) != want                                              # NaN != 0: an unwritten row is a mismatch too
        off = want & ~((got - 1.0 / n_i[:, None, None]).abs() <= rel / n_i[:, None, None])
        for i, h, c in bad.nonzero()[:limit].tolist():
            if len(fails) < limit:
                fails.append(f"{cfg.name}: output row {i} head {h} {'MISSES' if want[i, h, c] else 'SEES'} packed row "
                             f"{int(pr[h, c])} (got {got[i, h, c].item()!r}, spec {'visible' if want[i, h, c] else 'invisible'})")
        for i, h, c in (off & ~bad).nonzero()[:limit].tolist():
            if len(fails) < limit:
                fails.append(f"{cfg.name}: output row {i} head {h} packed row {int(pr[h, c])}: {got[i, h, c].item()!r} is not "
                             f"1 / {int(n_i[i])} within {rel:.1e}")
        if int(bad.sum()) + int((off & ~bad).sum()) and len(fails) >= limit:
            fails.append(f"{cfg.name}: ... ({int(bad.sum())} visibility and {int((off & ~bad).sum())} value mismatches in pass {r})")
            break
    return fails


# ------------------------------------------------------------------------------------------- needle
ALLOWED_KINDS = ("first_visible", "last_prefix_row", "first_own_row", "own_key_15", "own_key_16", "own_key_17", "itself",
                 "last_visible")
FORBIDDEN_KINDS = ("next_position", "previous_sequence_last_row", "next_sequence_first_row", "base_row_P")
_ROW_BITS, _HEAD_BITS = 13, 3


@lru_cache(maxsize=None)
def _codes(cfg: Config) -> Tuple[torch.Tensor, torch.Tensor]:
    """K codes [rows, heads, 64] (random +-1, seed chosen so that the margin assert holds) and V codes [rows, heads, 64]:
    bit b of (row | head << 13) as +-1 in the columns b, b + 16, b + 32, b + 48."""
    assert cfg.rows < 2 ** _ROW_BITS and cfg.heads <= 2 ** _HEAD_BITS
    g = torch.Generator().manual_seed(77)
    k = torch.randint(0, 2, (cfg.rows, cfg.heads, DH), generator=g).float() * 2 - 1
    word = torch.arange(cfg.rows)[:, None] | (torch.arange(cfg.heads)[None, :] << _ROW_BITS)
    bits = (word[:, :, None] >> (torch.arange(DH) % 16)) & 1
    return k, bits.float() * 2 - 1


def _decode(o: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """[..., 64] outputs -> (row, head, clean): the word spelt by the signs; clean = all four replicas agree, no zero / NaN."""
    b = (o > 0).long().view(*o.shape[:-1], 4, 16)
    clean = (b == b[..., :1, :]).all(-1).all(-1) & (o != 0).all(-1) & torch.isfinite(o).all(-1)
    word = (b[..., 0, :] << torch.arange(16)).sum(-1)
    return word & (2 ** _ROW_BITS - 1), word >> _ROW_BITS, clean


@lru_cache(maxsize=None)
def _all_targets(cfg: Config) -> dict:
    """kind -> the packed row every output row's query points at.  A candidate that does not exist for a row (or, for a
    forbidden kind, is visible after all) falls back to the row's last visible key."""
    p = _plan(cfg)
    st, rows = cfg.starts, cfg.rows
    kinds = ALLOWED_KINDS + FORBIDDEN_KINDS
    tgt = {k: [0] * len(p.seq) for k in kinds}
    q_rows = p.q_row.tolist()
    for i, s in enumerate(p.seq.tolist()):
        row0, own = st[s], st[s + 1] - st[s]
        P, prow0 = (cfg.prefix[s][0], st[cfg.prefix[s][1]]) if cfg.prefix is not None else (0, 0)
        vis_i = p.vis[i].tolist()
        order = [prow0 + t for t in range(P)] + [row0 + j for j in range(own)]          # by position
        seen = [r for r in order if vis_i[r]]
        at = order.index(q_rows[i])
        cand = {"first_visible": seen[0], "last_prefix_row": prow0 + P - 1 if P else -1, "first_own_row": row0,
                "own_key_15": row0 + 15, "own_key_16": row0 + 16, "own_key_17": row0 + 17, "itself": q_rows[i],
                "last_visible": seen[-1], "next_position": order[at + 1] if at + 1 < len(order) else row0 + own,
                "previous_sequence_last_row": row0 - 1, "next_sequence_first_row": row0 + own,
                "base_row_P": prow0 + P if P else -1}
        for kind in kinds:
            c = cand[kind]
            ok = 0 <= c < rows and (vis_i[c] == (kind in ALLOWED_KINDS)) and \
                (kind not in ("own_key_15", "own_key_16", "own_key_17") or c < row0 + own)
            tgt[kind][i] = c if ok else seen[-1]
    # pooled sequences that share all their rows (own length 0, or the first token of a shared prefix) share the packed row
    # of their query as well: one query, one target -- the first one's
    for kind in kinds:
        first = {}
        tgt[kind] = torch.tensor([first.setdefault(r, t) for r, t in zip(q_rows, tgt[kind])], dtype=torch.int64)
    return tgt


def _targets(cfg: Config, kind: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per output row: the packed row the query points at, and whether that row is visible to it."""
    p = _plan(cfg)
    tgt = _all_targets(cfg)[kind]
    return tgt, p.vis[torch.arange(len(tgt)), tgt]


@lru_cache(maxsize=None)
def needle_input(cfg: Config, kind: str) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(qkv, target row per output row, target visible per output row); cached and shared, never modified.  Asserts the 12-nat margin for every visible target."""
    k, v = _codes(cfg)
    p = _plan(cfg)
    tgt, tvis = _targets(cfg, kind)
    w = cfg.width
    qkv = torch.zeros((cfg.rows, 3 * w))
    qkv[:, w:2 * w] = k.reshape(cfg.rows, w)
    qkv[:, 2 * w:] = v.reshape(cfg.rows, w)
    # a packed row is the query of exactly one output row in every form but pooled ones, where other rows' q is never read
    qkv[p.q_row, :w] = NEEDLE_A * k[tgt].reshape(len(tgt), w)
    for h in range(cfg.heads):
        s = (qkv[p.q_row, h * DH:(h + 1) * DH] @ k[:, h].t()) * 0.125                  # [m, rows] scores
        s = torch.where(p.vis, s, torch.full((), float("-inf")))
        top = s[torch.arange(len(tgt)), tgt].clone()
        s[torch.arange(len(tgt)), tgt] = float("-inf")
        margin = top - s.max(1).values
        assert (margin[tvis] >= NEEDLE_MARGIN).all(), (cfg.name, kind, h, margin[tvis].min().item())
    return qkv, tgt, tvis


def check_needle(kernel: Callable[[torch.Tensor], torch.Tensor], cfg: Config, max_abs: float, mean_abs: Optional[float],
                 kinds: Sequence[str] = ALLOWED_KINDS + FORBIDDEN_KINDS, limit: int = 12) -> List[str]:
    p = _plan(cfg)
    fails: List[str] = []
    for kind in kinds:
        qkv, tgt, tvis = needle_input(cfg, kind)
        got = kernel(qkv).double().cpu()
        row, head, clean = _decode(got.view(cfg.n_out, cfg.heads, DH))
        o = p.out_row
        wrong = tvis[:, None] & ~(clean[o] & (row[o] == tgt[:, None]) & (head[o] == torch.arange(cfg.heads)))
        for j, h in wrong.nonzero()[:limit].tolist():
            i = int(o[j])
            if len(fails) < limit:
                fails.append(f"{cfg.name} [{kind}]: output row {i} head {h} points at packed row {int(tgt[j])} and decodes to "
                             f"(row {int(row[i, h])}, head {int(head[i, h])}{'' if clean[i, h] else ', unclean'})")
        if kind in FORBIDDEN_KINDS:
            d = (got - _needle_model(cfg, kind)).abs()
            if not (d.max().item() < max_abs and (mean_abs is None or d.mean().item() < mean_abs)):      # NaN fails
                i = int(d.max(1).values.argmax())
                if len(fails) < limit:
                    fails.append(f"{cfg.name} [{kind}]: max |out - model| {d.max().item():.3e} (bound {max_abs:.1e}), mean "
                                 f"{d.mean().item():.3e} (bound {mean_abs}); worst output row {i}, whose query points at "
                                 f"packed row {int(tgt[(p.out_row == i).nonzero()[0, 0]])}")
    return fails


@lru_cache(maxsize=None)
def _needle_model(cfg: Config, kind: str) -> torch.Tensor:
    """The reference of a forbidden pass: computed once per (config, kind), shared by every precision, never modified."""
    return model(needle_input(cfg, kind)[0], cfg)


def check_both(kernel, cfg: Config, precision: str) -> List[str]:
    b = PRECISION[precision]
    return check_readback(kernel, cfg, b["rel"]) + check_needle(kernel, cfg, b["max_abs"], b["mean_abs"])


# ------------------------------------------------------------------------------------------- the cases
_MIX = (1, 15, 16, 17, 31, 32)


def _packed(name: str, seq_len: int, causal: bool, **kw) -> Config:
    lens = tuple(n for n in _MIX if n < seq_len) + (seq_len,)
    return Config(name, seq_len, len(lens), causal=causal, lens=lens, **kw)


def tower_configs() -> List[Config]:
    """Every template the tower launcher can choose, entered from both sides of its limit, with heads = 3 and item counts
    (9 dense, 3 * n_seq packed, odd) that leave a spare item in the last workgroup of the 4- and 2-item forms."""
    out: List[Config] = []
    for T in (1, 16, 17, 32, 33, 96, 97, 288):                     # causal NT <= 2 / <= 6 / 18
        out.append(Config(f"causal_dense_{T}", T, 3))
        out.append(_packed(f"causal_packed_{T}", T, True))
    for T in (257, 272, 49, 64):                                     # non-causal: EXACT 17 / EXACT 4 dense, the general forms packed
        out.append(Config(f"full_dense_{T}", T, 3, causal=False))
        out.append(_packed(f"full_packed_{T}", T, False))
    for T in (17, 32, 96, 288):                                      # non-causal general forms NT <= 2 / <= 6 / 18 on dense rows
        out.append(Config(f"full_dense_{T}", T, 3, causal=False))
    # prefix groups of 3 (base, two variants): P in {0, 1, 15, 16, 17, base length}, T on and one past a tile boundary,
    # variants longer and shorter than their base, own length 0
    B = 20
    for P in (1, 15, 16, 17, B):
        out.append(Config(f"prefix_P{P}", 33, 3, lens=(B, 32 - P, 33 - P), prefix=((0, 0), (P, 0), (P, 0))))
    out.append(Config("prefix_short_and_empty", 33, 6, lens=(B, 2, 0, B, 0, 13),
                      prefix=((0, 0), (1, 0), (17, 0), (0, 3), (B, 3), (B, 3))))
    out.append(Config("prefix_P0_variant", 33, 3, lens=(B, 5, 33), prefix=((0, 0), (0, 0), (0, 0))))
    out.append(Config("prefix_two_tiles", 32, 3, lens=(B, 17, 1), prefix=((0, 0), (15, 0), (16, 0))))
    out.append(Config("prefix_long", 288, 3, lens=(100, 188, 59), prefix=((0, 0), (100, 0), (37, 0))))
    out.append(Config("prefix_mid", 96, 3, lens=(40, 56, 59), prefix=((0, 0), (40, 0), (37, 0))))
    # pooled forms
    out.append(Config("pool1_full_dense_257", 257, 3, causal=False, pool_mode=1))
    out.append(Config("pool1_full_dense_49", 49, 3, causal=False, pool_mode=1))
    out.append(Config("pool1_causal_dense_77", 77, 3, pool_mode=1))
    out.append(_packed("pool1_causal_packed_97", 97, True, pool_mode=1))
    out.append(_packed("pool1_full_packed_49", 49, False, pool_mode=1))
    out.append(_packed("pool2_causal_packed_97", 97, True, pool_mode=2))
    out.append(_packed("pool2_causal_packed_32", 32, True, pool_mode=2))
    out.append(_packed("pool2_full_packed_64", 64, False, pool_mode=2))
    out.append(Config("pool2_causal_dense_77", 77, 3, pool_mode=2, pool_rows=(0 * 77 + 76, 1 * 77 + 16, 2 * 77 + 15)))
    out.append(Config("pool2_causal_dense_17", 17, 3, pool_mode=2, pool_rows=(0, 17 + 16, 34 + 1)))
    out.append(Config("pool2_full_dense_257", 257, 3, causal=False, pool_mode=2, pool_rows=(256, 257 + 17, 514)))
    out.append(Config("pool2_prefix_empty", 33, 6, lens=(B, 2, 0, B, 0, 13), pool_mode=2,
                      prefix=((0, 0), (1, 0), (17, 0), (0, 3), (B, 3), (B, 3))))
    out.append(Config("pool1_prefix", 33, 3, lens=(B, 15, 16), pool_mode=1, prefix=((0, 0), (17, 0), (17, 0))))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def split_configs() -> List[Config]:
    """The split kernel takes starts and pfx but neither pooled form, and at most 272 tokens."""
    return [c if c.seq_len <= 272 else _shrink(c) for c in tower_configs() if c.pool_mode == 0]


def _shrink(c: Config) -> Config:
    if c.lens is None:
        return replace(c, name=c.name.replace("288", "272"), seq_len=272)
    if c.prefix is None:
        return replace(c, name=c.name.replace("288", "272"), seq_len=272, lens=c.lens[:-1] + (272,))
    return Config("prefix_long", 272, 3, lens=(100, 172, 59), prefix=((0, 0), (100, 0), (37, 0)))


def f32_configs() -> List[Config]:
    return [Config(f"{'causal' if causal else 'full'}_dense_{T}", T, 3, causal=causal)
            for causal in (True, False) for T in (1, 16, 17, 33, 257, 288)]


# ------------------------------------------------------------------------------------------- streaming kernel
SD_HEAD_DIMS = (8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 128, 160)
SD_REL = 2.0 ** -7                                  # bf16 output of 1 / Tk
SD_REL_L2, SD_MAX_STD = 5e-3, 5e-2                  # test_gpu_sd.py::test_streaming_attention_vs_fp64


def sd_readback_passes(Tk: int, dh: int) -> int:
    return (Tk + dh - 1) // dh


def _sd_probe_keys(r: int, n: int, heads: int, dh: int) -> torch.Tensor:
    """int64 [n, heads, dh]: the key (within its sample) whose value sits in column c of head h of sample b in pass r --
    shifted by 7 per head and 3 per sample, so a read across heads or samples shows."""
    c = torch.arange(dh)
    return torch.stack([torch.stack([dh * r + (c + 7 * h + 3 * b) % dh for h in range(heads)]) for b in range(n)])


def sd_readback_input(r: int, n: int, heads: int, dh: int, Tq: int, Tk: int):
    g = torch.Generator().manual_seed(2000 + r)
    C = heads * dh
    q = torch.zeros((n * Tq, C))
    k = torch.randn((n * Tk, C), generator=g).to(torch.bfloat16).float()
    v = torch.zeros((n, Tk, heads, dh))
    pk = _sd_probe_keys(r, n, heads, dh)
    b, h, c = torch.meshgrid(torch.arange(n), torch.arange(heads), torch.arange(dh), indexing="ij")
    ok = pk < Tk
    v[b[ok], pk[ok], h[ok], c[ok]] = 1.0
    want = ok[:, None].expand(n, Tq, heads, dh).reshape(n * Tq, C)                    # every query sees every key of its sample
    return q, k, v.reshape(n * Tk, C), want


def sd_check_readback(kernel, n: int, heads: int, dh: int, Tq: int, Tk: int, limit: int = 8) -> List[str]:
    """kernel(q, k, v) -> out [n * Tq, heads * dh]."""
    fails: List[str] = []
    for r in range(sd_readback_passes(Tk, dh)):
        q, k, v, want = sd_readback_input(r, n, heads, dh, Tq, Tk)
        got = kernel(q, k, v).double().cpu()
        bad = (got != 0) != want
        off = want & ~((got - 1.0 / Tk).abs() <= SD_REL / Tk) & ~bad
        pk = _sd_probe_keys(r, n, heads, dh)
        for i, col in (bad | off).nonzero()[:max(limit - len(fails), 0)].tolist():
            b, h, c = i // Tq, col // dh, col % dh
            fails.append(f"dh {dh} Tq {Tq} Tk {Tk}: sample {b} query {i % Tq} head {h} key {int(pk[b, h, c])}: got {got[i, col].item()!r}, "
                         f"spec {'1 / ' + str(Tk) if want[i, col] else 'exactly 0'}")
    return fails


def sd_needle_input(n: int, heads: int, dh: int, Tq: int, Tk: int, shift: int):
    """K codes: +-1, the key's own 8 bits in the first 8 columns (so that no two codes of a sample are equal at any head
    dim) and seeded random bits after them; V codes: the bits of key + 37 head + 101 sample, so neighbouring samples and
    heads differ; query i of a sample points at key (i + shift) mod Tk with q = a k_target, a the power of two that gives
    the 12-nat margin.  The target then holds >= 1 - Tk e^-12 of the softmax: |out - v_target| <= 2 Tk e^-12 + 2^-8 (the
    bf16 roundings of the probabilities and of the output) < 2^-6 for Tk <= 256."""
    g = torch.Generator().manual_seed(dh)
    assert Tk <= 256
    kc = torch.randint(0, 2, (n, Tk, heads, dh), generator=g).float() * 2 - 1
    kc[..., :8] = (((torch.arange(Tk)[:, None] >> torch.arange(8)) & 1).float() * 2 - 1)[None, :, None, :]
    word = torch.arange(Tk)[None, :, None] + 37 * torch.arange(heads)[None, None, :] + 101 * torch.arange(n)[:, None, None]
    vc = ((word[..., None] >> (torch.arange(dh) % 16)) & 1).float() * 2 - 1
    tgt = (torch.arange(Tq) + shift) % Tk
    corr = torch.einsum("bihd,bjhd->bhij", kc, kc)
    corr.diagonal(dim1=-2, dim2=-1).fill_(float("-inf"))
    cmax = corr.max().item() if Tk > 1 else -float(dh)
    a = 2.0 ** math.ceil(math.log2(NEEDLE_MARGIN * math.sqrt(dh) / (dh - cmax)))
    assert a * (dh - cmax) / math.sqrt(dh) >= NEEDLE_MARGIN and a <= 128, (dh, Tk, cmax, a)      # the margin, in nats
    q = a * kc[:, tgt]                                                                        # [n, Tq, heads, dh]
    C = heads * dh
    return q.reshape(n * Tq, C), kc.reshape(n * Tk, C), vc.reshape(n * Tk, C), vc[:, tgt].reshape(n * Tq, C)


def sd_check_needle(kernel, n: int, heads: int, dh: int, Tq: int, Tk: int, limit: int = 8) -> List[str]:
    fails: List[str] = []
    for shift in (0, Tk - 1, Tk // 2 + 1):                    # the last key (ragged tile) and the first meet every query block
        q, k, v, want = sd_needle_input(n, heads, dh, Tq, Tk, shift)
        got = kernel(q, k, v).double().cpu()
        bad = (torch.sign(got) != want) | ~((got - want).abs() < 2.0 ** -6)
        for i, col in bad.nonzero()[:max(limit - len(fails), 0)].tolist():
            fails.append(f"dh {dh} Tq {Tq} Tk {Tk}: sample {i // Tq} query {i % Tq} head {col // dh} points at key "
                         f"{(i % Tq + shift) % Tk}: column {col % dh} is {got[i, col].item()!r}, its value is {want[i, col].item()}")
    return fails
