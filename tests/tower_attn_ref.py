"""The tower attention's softmax VALUES against fp64, element by element (plain helper module: no GPU, no fixtures).
tests/test_tower_attn_ref.py checks everything here on the CPU, tests/test_gpu_tower_attention_values.py runs the kernels
(csrc/attention.hip in bf16 and fp16, attention_split in csrc/split.hip, attention_f32 in csrc/precise.hip) on the same cases.

* ``reference``   (ref, bound): ref = attn_witness.model(qkv, cfg) in fp64 on the values the kernel reads; the weights w of
                  every output row come from the same plan and visibility (dense, packed, shared prefixes, both pooled
                  forms need no second statement of the spec).  The bound on |got - ref| holds for EVERY output element and
                  is derived from the formats and each kernel's code ("Tower attention: values"):

                  bf16 / fp16 (attention.hip) -- the formula of sd_attn_ref.reference with dh = 64 and no moving reference:
                      0.5 ulp16(ref) (1 + 2^-8) + sum_j w_ij (2 eps + 2 ds_ij) |v_jc| + 2 flush sum_j |v_jc|
                  split (split.hip) -- hi | lo operands, probabilities split for the numerator only, fp32 row sum:
                      sum_j w_ij (2^-15 + 3 n_i 2^-24) |v_jc| + sum_j w_ij d_ij |v_jc - ref_ic|
                      + |ref_ic| (n_i 2^-24 + 2^-22 + 2^-17),   d_ij = (2^-15 + 192 2^-24) sum_d |q_id k_jd| / 8 + X_ij
                  fp32 (precise.hip) -- fmaf chains, expf, one rescale of o and l per key:
                      sum_j w_ij d_ij |v_jc - ref_ic| + 2 n_i 2^-24 (sum_j w_ij |v_jc| + |ref_ic|) + 2^-22 |ref_ic|,
                      d_ij = 18 2^-24 sum_d |q_id k_jd| / 8 + X_ij + 2^-22 (moves of the running maximum after key j)
                  X_ij = 2^-23 |s_ij - m_i| + 2^-22: the exponent's argument and the exponential.  n_i = visible keys.
                  The last two carry a factor 1.01 for the second-order terms.

* ``make_inputs`` score profiles, one per head (``Case.profiles``); everything already rounded to the format;
                  v = 2 randn + 0.5 so that a mis-weighted row shows.
* ``emulate``     the kernels' arithmetic in fp32 as read from their code: fp32 scores, exp2(fma(s, c, -m c)), probabilities
                  rounded once to the format, the denominator summed over the ROUNDED probabilities, one output rounding
                  (tower); the three-product hi | lo form (split); the per-key online loop (fp32).  ``defect=`` applies one of
                  ``DEFECTS`` to the tower arithmetic: value defects that the mask witnesses of attn_witness cannot see.
* ``gpu_cases``   the cases of the GPU file, shared so that the CPU file proves its claims on exactly those.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

import attn_witness as W
import sd_ops_ref as R
from sd_attn_ref import EPS, FLUSH, worst_ratio          # the 16-bit constants are stated once, there

DH = W.DH
QBLOCK = 16                                     # queries per block: one wave's step
LOG2E = 1.4426950408889634
PRECISIONS = ("bf16", "fp16", "split", "fp32")
PROFILES = ("flat", "peaked", "spiky", "offset")
Q_SCALE = {"flat": 1.0, "peaked": 3.0, "spiky": 8.0, "offset": 1.0}
# ``offset``: q[:, 0] = a and k[:, 0] = b in every row add a b / 8 nats to every score.  40 nats (2^57.7) is what overflows
# fp16 when a probability is packed; bf16 and fp32 probabilities have fp32's exponent range, where only exp2 itself can
# overflow: past 2^128 = 88.7 nats, hence 96 there.  All four numbers are exact in every format.
OFFSET_AB = {"fp16": (16.0, 20.0), "bf16": (32.0, 24.0), "split": (32.0, 24.0), "fp32": (32.0, 24.0)}

DEFECTS = (
    "scale_plus_1_percent",
    "scale_minus_1_percent",
    "log2e_missing_from_scale",                 # exp2(s / 8 - m / 8): the softmax of s ln 2
    "scores_rounded_to_16_bits",                # the MFMA's fp32 scores rounded to the format before the exponent
    "row_maximum_not_subtracted",
    "denominator_of_previous_query_block",      # 1 / l of the sequence's previous 16-query block, lane for lane
    "denominator_over_unrounded_probabilities", # l summed in fp32 before the probabilities are rounded.  NOT caught, and need
                                                # not be: numerator and denominator then differ by one rounding per term,
                                                # which the bound's 2 eps covers (the twin of sd_attn_ref's
                                                # threshold_compares_nats_not_bits; test_tower_attn_ref.py shows it inside)
)
HARMLESS = ("denominator_over_unrounded_probabilities",)


def to_format(x64: torch.Tensor, precision: str) -> torch.Tensor:
    return R.round16(x64, precision) if precision in EPS else x64.float().double()


def template_of(cfg: W.Config, precision: str) -> str:
    """The kernel template a config reaches: the launchers' rules (launch_attention_t in csrc/attention.hip,
    launch_attention_split in csrc/split.hip) restated to name it."""
    NT = (cfg.seq_len + 15) // 16
    if precision == "fp32":
        return "f32"
    if precision == "split":
        return f"split<{2 if NT <= 2 else 6 if NT <= 6 else 18}, {'causal' if cfg.causal else 'full'}>"
    if cfg.causal:
        return f"<{2 if NT <= 2 else 6 if NT <= 6 else 18}, causal>"
    if cfg.lens is None and NT in (17, 4):
        return f"<{NT}, full, EXACT>"
    return f"<{2 if NT <= 2 else 4 if NT <= 4 else 6 if NT <= 6 else 18}, full>"


# ----------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    cfg: W.Config
    precision: str
    rot: int

    @property
    def id(self) -> str:
        return f"{self.precision}-{self.cfg.name}-r{self.rot}"

    @property
    def profiles(self) -> Tuple[str, ...]:
        """Head h runs profile (rot + h) mod 4."""
        return tuple(PROFILES[(self.rot + h) % len(PROFILES)] for h in range(self.cfg.heads))

    @property
    def template(self) -> str:
        return template_of(self.cfg, self.precision)

    def inputs(self) -> torch.Tensor:
        return make_inputs(self.cfg, self.precision, self.profiles)


def make_inputs(cfg: W.Config, precision: str, profiles: Tuple[str, ...]) -> torch.Tensor:
    """qkv fp64 [rows, 3 * width] (q | k | v) holding values of the format; every head has its own profile and seed."""
    assert len(profiles) == cfg.heads
    w = cfg.width
    qkv = torch.zeros((cfg.rows, 3 * w), dtype=torch.float64)
    for h, prof in enumerate(profiles):
        g = torch.Generator().manual_seed(zlib.crc32(f"{cfg.name}/{precision}/{h}/{prof}".encode()))
        q = torch.randn((cfg.rows, DH), generator=g, dtype=torch.float64) * Q_SCALE[prof]
        k = torch.randn((cfg.rows, DH), generator=g, dtype=torch.float64)
        v = torch.randn((cfg.rows, DH), generator=g, dtype=torch.float64) * 2 + 0.5
        if prof == "offset":
            q[:, 0], k[:, 0] = OFFSET_AB[precision]
        for part, t in enumerate((q, k, v)):
            qkv[:, part * w + h * DH: part * w + (h + 1) * DH] = t
    return to_format(qkv, precision)


def _rotated(configs: List[W.Config], precision: str, first: int) -> List[Case]:
    """One case per config; the configs of one template take consecutive rotations, so that any two neighbours put all four
    profiles on the template (a case's three heads carry three)."""
    seen: Dict[str, int] = {}
    out = []
    for c in configs:
        t = template_of(c, precision)
        out.append(Case(c, precision, (first + seen.get(t, 0)) % len(PROFILES)))
        seen[t] = seen.get(t, 0) + 1
    for c in configs:                               # a template with one config only (<6, full>) runs it a second time
        if seen[template_of(c, precision)] == 1:
            out.append(Case(c, precision, (first + 1) % len(PROFILES)))
    return out


def tower_cases(precision: str) -> List[Case]:
    return _rotated(W.tower_configs(), precision, 0 if precision == "bf16" else 2)


def split_cases() -> List[Case]:
    by_name = {c.name: c for c in W.split_configs()}           # the shrunk full_dense_288 is the list's full_dense_272 again
    return _rotated(list(by_name.values()), "split", 1)


def f32_cases() -> List[Case]:
    return _rotated(W.f32_configs(), "fp32", 3)


def determinism_case(precision: str) -> Case:
    by_name = {c.cfg.name: c for c in gpu_cases() if c.precision == precision}
    return by_name["full_dense_257" if precision in ("fp32", "split") else "causal_packed_97"]


def gpu_cases() -> List[Case]:
    """Every case tests/test_gpu_tower_attention_values.py compares with the bound, once."""
    return tower_cases("bf16") + tower_cases("fp16") + split_cases() + f32_cases()


# ------------------------------------------------------------------------------------------------------- reference
def where(cfg: W.Config, out_row: int) -> Tuple[int, int]:
    """(sequence, position of the query within the sequence's keys) of an output row."""
    p = W._plan(cfg)
    i = int((p.out_row == out_row).nonzero()[0, 0])
    s = int(p.seq[i])
    st = cfg.starts
    P, prow0 = (cfg.prefix[s][0], st[cfg.prefix[s][1]]) if cfg.prefix is not None else (0, 0)
    q = int(p.q_row[i])
    return s, (P + q - st[s]) if st[s] <= q < st[s + 1] else q - prow0      # an own row, or a row of the shared prefix


def _heads(qkv: torch.Tensor, cfg: W.Config, dtype):
    """Per head: the queries of the plan's rows [m, 64], the keys and the values of every packed row [rows, 64]."""
    p = W._plan(cfg)
    w = cfg.width
    x = qkv.to(dtype)
    for h in range(cfg.heads):
        c = slice(h * DH, (h + 1) * DH)
        yield h, x[p.q_row][:, c], x[:, w:2 * w][:, c], x[:, 2 * w:][:, c]


def weights(qkv: torch.Tensor, cfg: W.Config) -> List[torch.Tensor]:
    """fp64 [m, rows] per head, rows in the plan's order: the softmax over the visible keys."""
    p = W._plan(cfg)
    out = []
    for _, q, k, _ in _heads(qkv, cfg, torch.float64):
        s = q @ k.t() * 0.125
        out.append(torch.where(p.vis, s, torch.full_like(s, -math.inf)).softmax(-1))
    return out


def _moves_after(s: torch.Tensor, vis: torch.Tensor) -> torch.Tensor:
    """[m, rows]: how often a running maximum over the visible keys, taken in row order, still rises after key j."""
    sm = torch.where(vis, s, torch.full_like(s, -math.inf))
    before = torch.cat([torch.full_like(sm[:, :1], -math.inf), sm.cummax(1).values[:, :-1]], 1)
    rises = (sm > before).double()
    return rises.sum(1, keepdim=True) - rises.cumsum(1)


def reference(qkv: torch.Tensor, cfg: W.Config, precision: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ref, bound), both fp64 [cfg.n_out, width]."""
    assert precision in PRECISIONS
    p = W._plan(cfg)
    ref = W.model(qkv, cfg)
    bound = torch.zeros_like(ref)
    vis = p.vis
    n_i = vis.sum(1, keepdim=True).double()
    for (h, q, k, v), w in zip(_heads(qkv, cfg, torch.float64), weights(qkv, cfg)):
        c = slice(h * DH, (h + 1) * DH)
        r = ref[p.out_row][:, c]                                                   # [m, 64]
        s = torch.where(vis, q @ k.t() * 0.125, torch.zeros((), dtype=torch.float64))
        qk = q.abs() @ k.abs().t() * 0.125                                         # sum_d |q_id k_jd| / sqrt(dh)
        av = v.abs()
        if precision in EPS:
            ds = DH * 2.0 ** -24 * qk + 2.0 ** -22 * (1.0 + s.abs())
            b = (w * (2.0 * EPS[precision] + 2.0 * ds)) @ av + 2.0 * FLUSH[precision] * (vis.double() @ av)
            b = b + 0.5 * R.ulp16(r, precision) * (1.0 + 2.0 ** -8)
        else:
            m = torch.where(vis, s, torch.full_like(s, -math.inf)).max(1, keepdim=True).values
            x = 2.0 ** -23 * torch.where(vis, (s - m).abs(), torch.zeros_like(s)) + 2.0 ** -22
            # sum_j w_ij d_ij |v_jc - ref_ic| <= (w d) @ |v| + (w d).sum |ref|, without the [m, rows, 64] tensor
            if precision == "split":
                d = w * ((2.0 ** -15 + 192 * 2.0 ** -24) * qk + x)
                b = (w * (2.0 ** -15 + 3 * n_i * 2.0 ** -24)) @ av + _spread(d, v, r) \
                    + r.abs() * (n_i * 2.0 ** -24 + 2.0 ** -22 + 2.0 ** -17)
            else:
                d = w * (18 * 2.0 ** -24 * qk + x + 2.0 ** -22 * _moves_after(s, vis))
                b = _spread(d, v, r) + 2 * n_i * 2.0 ** -24 * (w @ av + r.abs()) + 2.0 ** -22 * r.abs()
            b = 1.01 * b
        bound[p.out_row, c] = b
    return ref, bound


def _spread(d: torch.Tensor, v: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """sum_j d_ij |v_jc - r_ic| for d [m, rows], v [rows, 64], r [m, 64], in slabs of output rows."""
    out = torch.empty_like(r)
    for a in range(0, r.shape[0], 64):
        out[a:a + 64] = (d[a:a + 64, :, None] * (v[None] - r[a:a + 64, None]).abs()).sum(1)
    return out


# ------------------------------------------------------------------------------------------------------- emulation
def _f32(x: float) -> torch.Tensor:
    return torch.tensor(x, dtype=torch.float32)


def _fma(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fp32 fmaf: the product of two fp32 numbers is exact in fp64, one rounding at the end."""
    return (a.double() * b.double() + c.double()).float()


def _index_in_sequence(p: W.Plan) -> torch.Tensor:
    """int64 [m]: the plan's rows of one sequence are its queries in order."""
    seq = p.seq.tolist()
    out, run = [], 0
    for i, s in enumerate(seq):
        run = run + 1 if i and seq[i - 1] == s else 0
        out.append(run)
    return torch.tensor(out, dtype=torch.int64)


def _hi_lo(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def emulate(qkv: torch.Tensor, cfg: W.Config, precision: str, defect: Optional[str] = None) -> torch.Tensor:
    """fp64 [cfg.n_out, width] holding what the kernel of ``precision`` stores (split: hi + lo).  Rows the plan does not
    name stay NaN.  ``defect`` applies to the tower kernel's arithmetic (bf16 / fp16) only."""
    assert defect is None or (defect in DEFECTS and precision in EPS), (defect, precision)
    p = W._plan(cfg)
    out = torch.full((cfg.n_out, cfg.width), math.nan, dtype=torch.float64)
    if precision == "fp32":
        return _emulate_f32(qkv, cfg, out)
    scale = _f32(0.125) * _f32(LOG2E)                                            # ATT_SCALE_LOG2
    scale = {"scale_plus_1_percent": scale * _f32(1.01), "scale_minus_1_percent": scale * _f32(0.99),
             "log2e_missing_from_scale": _f32(0.125)}.get(defect, scale)
    ninf = torch.full((), -math.inf, dtype=torch.float32)
    for h, q, k, v in _heads(qkv, cfg, torch.float32):
        c = slice(h * DH, (h + 1) * DH)
        if precision == "split":
            (qh, ql), (kh, kl), (vh, vl) = _hi_lo(q), _hi_lo(k), _hi_lo(v)
            s = (ql @ kh.t() + qh @ kl.t()) + qh @ kh.t()                       # small terms first; lo . lo is dropped
        else:
            s = q @ k.t()
            dt = R.FORMATS[precision]["dtype"]
            if defect == "scores_rounded_to_16_bits":
                s = s.to(dt).float()
        s = torch.where(p.vis, s, ninf)                                          # raw scores: the maximum is taken before the scale
        mxs = s.max(1, keepdim=True).values * scale
        if defect == "row_maximum_not_subtracted":
            mxs = torch.zeros_like(mxs)
        e = torch.exp2(_fma(s, scale, -mxs))
        if precision == "split":
            l = e.sum(1, keepdim=True)                                           # over the un-rounded probabilities
            ph, pl = _hi_lo(e)
            o = ((pl @ vh + ph @ vl) + ph @ vh) * (1.0 / l)
            oh, ol = _hi_lo(o)
            out[p.out_row, c] = oh.double() + ol.double()
            continue
        pr = e.to(dt).float()
        l = (e if defect == "denominator_over_unrounded_probabilities" else pr).sum(1, keepdim=True)
        if defect == "denominator_of_previous_query_block" and cfg.pool_mode == 0:
            j = _index_in_sequence(p)
            src = torch.where(j >= QBLOCK, torch.arange(len(j)) - QBLOCK, torch.arange(len(j)))
            l = l[src]
        out[p.out_row, c] = ((pr @ v) * (1.0 / l)).to(dt).double()
    return out


def _emulate_f32(qkv: torch.Tensor, cfg: W.Config, out: torch.Tensor) -> torch.Tensor:
    """attention_f32_kernel: dense rows, one query per thread, the keys in order with a running maximum."""
    assert cfg.lens is None and cfg.pool_mode == 0
    n, T, H = cfg.n_seq, cfg.seq_len, cfg.heads
    x = qkv.float().view(n, T, 3, H, DH)
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]                                  # [n, T, H, 64]
    m = torch.full((n, T, H), -math.inf)
    l = torch.zeros((n, T, H))
    o = torch.zeros((n, T, H, DH))
    qi = torch.arange(T)[None, :, None]
    for j in range(T):
        s = (q * k[:, j:j + 1]).sum(-1) * 0.125
        mn = torch.maximum(m, s)
        alpha, pj = torch.exp(m - mn), torch.exp(s - mn)
        live = (qi >= j) if cfg.causal else torch.ones_like(qi, dtype=torch.bool)
        l = torch.where(live, l * alpha + pj, l)
        o = torch.where(live[..., None], pj[..., None] * v[:, j:j + 1] + o * alpha[..., None], o)
        m = torch.where(live, mn, m)
    return (o * (1.0 / l)[..., None]).reshape(n * T, H * DH).double()


def effective_keys(w: torch.Tensor) -> torch.Tensor:
    """1 / sum_j w_ij^2 per row: how many keys share the softmax."""
    return 1.0 / (w * w).sum(1)
