"""The streaming attention's online softmax (csrc/sd_attention.hip) against fp64, element by element (plain helper module:
no GPU, no fixtures).  tests/test_sd_attn_ref.py checks everything here on the CPU, tests/test_gpu_sd_attention_values.py
runs the kernel on the same cases.

* ``reference``     w = softmax(q k^T / sqrt(dh)), ref = w v in fp64 on the 16-bit values the kernel reads, and a bound on
                    |got - ref| for EVERY output element, derived from the formats and the kernel's arithmetic (DESIGN.md,
                    "Streaming attention: values"):

                        0.5 ulp16(ref) (1 + 2^-8)                    the output's rounding, after an fp32 multiply by 1 / l
                      + sum_j w_ij (2 eps + 2 ds_ij) |v_jc|          eps = 2^-9 (bf16) / 2^-12 (fp16): one rounding of each
                                                                     probability, in numerator and denominator alike
                      + 2 flush sum_j |v_jc|                         flush = 2^-25 in fp16 (a probability below 2^-24 becomes 0;
                                                                     the largest probability of a row is >= 1, so l >= 1), 0 in bf16
                      ds_ij = dh 2^-24 sum_d |q_id k_jd| / sqrt(dh)  the fp32 accumulation of the score, in nats
                            + 2^-22 (1 + |s_ij|)                     the fmaf into the exponent and the exp2 instruction

* ``make_inputs``   score profiles that make the lazy reference maximum MOVE, stay just below its threshold, fall, or jump
                    at the last key.  Column 0 of every head carries k[j, 0] = a_j and q[i, 0] = 4 c_i, so key j's score
                    gets 4 c_i a_j / sqrt(dh) nats; a_j is chosen so that this is the profile's number of BITS (nats / ln 2)
                    for the query class c_i = +1, which is i % 3 == 0; i % 3 == 1 is class 0 (flat) and i % 3 == 2 class -1
                    (the mirrored profile), so one 16-query block holds rows that move, stay and fall.  The other columns
                    are randn, v is randn * 2 + 0.5 (a mean, so that a mis-weighted row shows); everything is built
                    already rounded to the format.
* ``emulate``       the kernel's tile loop in fp32: tiles of 64 keys, the lazy rule behind a per-16-query-block "any lane
                    moves", probabilities rounded to the format, the row sum over the ROUNDED probabilities;
                    ``defect=`` applies one of ``DEFECTS``.  Also returns each row's number of moves after tile 0.
* ``gpu_cases``     the cases of the GPU file, shared so that the CPU file proves its claims on exactly those.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

import sd_ops_ref as R
from attn_witness import SD_HEAD_DIMS

TILE = 64                   # keys per LDS tile
QBLOCK = 16                 # queries behind one wave-uniform "does any lane move" ballot
LAZY_BITS = 8.0             # the reference moves when the true maximum has grown by more than this, in bits
EPS = {"bf16": 2.0 ** -9, "fp16": 2.0 ** -12}           # half an ulp of a probability, relative
FLUSH = {"bf16": 0.0, "fp16": 2.0 ** -25}               # half the subnormal spacing of fp16: the absolute error of a tiny probability
LN2 = math.log(2.0)

PROFILES = ("rise3", "rise5", "rise9", "fall9", "late_spike", "threshold")
THRESHOLD_BITS = (7.75, 8.25)                           # tile 1 of even heads (no move) / odd heads (move)
# ``threshold`` only: the randn columns of q are scaled by 2^-6.  The profile needs every class +1 row of a head on ONE
# side of 2^8.  A row moves when (max of tile 1) - (max of tile 0) > 8 bits, and with unit randn columns the two tile
# maxima of the random part differ by about +-0.7 bits from row to row -- three times the 0.25-bit margin, a coin toss.
# Scaled, they differ by about +-0.01 bits (tests/test_sd_attn_ref.py asserts the sides on every case).
THRESHOLD_Q_SCALE = 2.0 ** -6

DEFECTS = (
    "sum_not_rescaled",                         # osum *= alpha dropped
    "output_not_rescaled",                      # o *= alpha dropped
    "alpha_squared",
    "staying_lanes_rescale_output_only",        # in a block where some lane moves, a staying lane's o takes exp2(m_run - m_new) too
    "reference_never_moves_after_first_tile",
    "threshold_compares_nats_not_bits",         # move = (m_new - m_run) / sqrt(dh) > 8: log2(e) missing, the reference lags by up to
                                                # 11.5 bits.  NOT a value defect: o / l does not depend on the reference, and 2^11.5
                                                # is inside fp16 (tests/test_sd_attn_ref.py shows it within the bound everywhere)
    "ragged_tile_duplicates_counted",           # the clamped re-reads of the last key are not masked
    "last_key_tile_skipped_when_odd",           # the unpaired last tile of the two-register-set loop never runs
)


def class_of_query(Tq: int) -> torch.Tensor:
    """c_i in {+1, 0, -1} by i % 3."""
    return torch.tensor([1.0, 0.0, -1.0], dtype=torch.float64)[torch.arange(Tq) % 3]


def profile_bits(profile: str, heads: int, Tk: int) -> torch.Tensor:
    """fp64 [heads, Tk]: the offset of key j's score for a class +1 query, in bits."""
    tile = (torch.arange(Tk) // TILE).double()
    bits = torch.zeros((heads, Tk), dtype=torch.float64)
    if profile in ("rise3", "rise5", "rise9", "fall9"):
        bits += tile * {"rise3": 3.0, "rise5": 5.0, "rise9": 9.0, "fall9": -9.0}[profile]
    elif profile == "late_spike":
        bits[:, Tk - 1] = 10.0
    elif profile == "threshold":
        for h in range(heads):
            bits[h, TILE:2 * TILE] = THRESHOLD_BITS[h % 2]
    else:
        raise ValueError(profile)
    return bits


def make_inputs(profile: str, fmt: str, n: int, heads: int, dh: int, Tq: int, Tk: int, seed: int = 0):
    """(q [n * Tq, C], k, v [n * Tk, C]) as fp64 holding values of the format."""
    g = torch.Generator().manual_seed(1000 * PROFILES.index(profile) + 7 * dh + 3 * Tk + Tq + seed)
    q = torch.randn((n, Tq, heads, dh), generator=g, dtype=torch.float64)
    k = torch.randn((n, Tk, heads, dh), generator=g, dtype=torch.float64)
    v = torch.randn((n, Tk, heads, dh), generator=g, dtype=torch.float64) * 2 + 0.5
    if profile == "threshold":
        q *= THRESHOLD_Q_SCALE
    q[..., 0] = 4.0 * class_of_query(Tq)[None, :, None]
    k[..., 0] = (profile_bits(profile, heads, Tk) * (LN2 * math.sqrt(dh) / 4.0)).t()[None]
    C = heads * dh
    return tuple(R.round16(t, fmt).reshape(-1, C) for t in (q, k, v))


def _split(t: torch.Tensor, n: int, heads: int) -> torch.Tensor:
    """[n * T, heads * dh] -> [n, heads, T, dh]"""
    return t.view(n, t.shape[0] // n, heads, t.shape[1] // heads).transpose(1, 2)


def _merge(t: torch.Tensor) -> torch.Tensor:
    n, heads, T, dh = t.shape
    return t.transpose(1, 2).reshape(n * T, heads * dh)


def reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, n: int, heads: int, fmt: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ref, bound), both fp64 [n * Tq, C]."""
    dh = q.shape[1] // heads
    qs, ks, vs = (_split(t.double(), n, heads) for t in (q, k, v))
    s = qs @ ks.transpose(-1, -2) / math.sqrt(dh)                               # nats
    w = s.softmax(-1)
    ref = w @ vs
    ds = dh * 2.0 ** -24 * (qs.abs() @ ks.abs().transpose(-1, -2)) / math.sqrt(dh) + 2.0 ** -22 * (1.0 + s.abs())
    bound = (w * (2.0 * EPS[fmt] + 2.0 * ds)) @ vs.abs() + 2.0 * FLUSH[fmt] * vs.abs().sum(-2, keepdim=True)
    ref, bound = _merge(ref), _merge(bound.expand_as(ref))
    return ref, bound + 0.5 * R.ulp16(ref, fmt) * (1.0 + 2.0 ** -8)


def worst_ratio(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """max |got - ref| / bound over every element; inf where got is not finite."""
    g = got.double().reshape(ref.shape)
    r = (g - ref).abs() / bound
    return torch.where(torch.isfinite(g), r, torch.full_like(r, math.inf)).max().item()


def emulate(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, n: int, heads: int, fmt: str,
            defect: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out fp64 [n * Tq, C] holding values of the format, moves int64 [n, heads, Tq]: moves of the reference after tile 0)."""
    assert defect is None or defect in DEFECTS, defect
    dt = R.FORMATS[fmt]["dtype"]
    f32 = torch.float32
    dh = q.shape[1] // heads
    Tq, Tk = q.shape[0] // n, k.shape[0] // n
    scale_log2 = torch.tensor(1.4426950408889634, dtype=f32) / torch.sqrt(torch.tensor(float(dh), dtype=f32))
    nkt = (Tk + TILE - 1) // TILE
    last = nkt - 1 if defect == "last_key_tile_skipped_when_odd" and nkt % 2 == 1 else nkt
    nblk = (Tq + QBLOCK - 1) // QBLOCK
    outs, counts = [], []
    for b in range(n):
        qs, ks, vs = (_split(t, n, heads)[b].to(f32) for t in (q, k, v))          # [heads, T, dh]
        m_run = torch.full((heads, Tq), -math.inf, dtype=f32)
        o = torch.zeros((heads, Tq, dh), dtype=f32)
        osum = torch.zeros((heads, Tq), dtype=f32)
        moves = torch.zeros((heads, Tq), dtype=torch.int64)
        for kt in range(last):
            kj = torch.arange(kt * TILE, (kt + 1) * TILE)
            if defect == "ragged_tile_duplicates_counted":
                kj = kj.clamp(max=Tk - 1)
            else:
                kj = kj[kj < Tk]
            s = qs @ ks[:, kj].transpose(-1, -2)                                    # raw dot products, fp32
            m_new = torch.maximum(m_run, s.max(-1).values)
            if defect == "threshold_compares_nats_not_bits":
                move = (m_new - m_run) / math.sqrt(dh) > LAZY_BITS
            else:
                move = (m_new - m_run) * scale_log2 > LAZY_BITS
            if defect == "reference_never_moves_after_first_tile" and kt > 0:
                move = torch.zeros_like(move)
            pad = torch.zeros((heads, nblk * QBLOCK), dtype=torch.bool)
            pad[:, :Tq] = move
            block_any = pad.view(heads, nblk, QBLOCK).any(-1).repeat_interleave(QBLOCK, dim=1)[:, :Tq]
            m_use = torch.where(move, m_new, m_run)
            alpha = torch.exp2((m_run - m_use) * scale_log2)                        # 1 for the lanes that stay, 0 in a row's first tile
            if defect == "alpha_squared":
                alpha = alpha * alpha
            alpha_o = alpha
            if defect == "staying_lanes_rescale_output_only":
                alpha_o = torch.where(block_any & ~move, torch.exp2((m_run - m_new) * scale_log2), alpha)
            if defect != "sum_not_rescaled":
                osum = osum * alpha
            if defect != "output_not_rescaled":
                o = o * alpha_o[..., None]
            m_run = m_use
            if kt > 0:
                moves += move
            mns = m_run * scale_log2
            e = (s.double() * scale_log2.double() - mns.double()[..., None]).to(f32)   # fmaf: one rounding
            p = torch.exp2(e).to(dt).to(f32)
            o = o + p @ vs[:, kj]
            osum = osum + p.sum(-1)
        outs.append((o * (1.0 / osum)[..., None]).to(dt).double())
        counts.append(moves)
    return _merge(torch.stack(outs)), torch.stack(counts)


# ----------------------------------------------------------------------------------------------- the GPU file's cases
@dataclass(frozen=True)
class Case:
    profile: str
    fmt: str
    n: int
    heads: int
    dh: int
    Tq: int
    Tk: int

    @property
    def id(self) -> str:
        return f"{self.profile}-{self.fmt}-n{self.n}h{self.heads}d{self.dh}-Tq{self.Tq}-Tk{self.Tk}"

    def inputs(self):
        return make_inputs(self.profile, self.fmt, self.n, self.heads, self.dh, self.Tq, self.Tk)


FMTS = ("bf16", "fp16")
# 2, 3, 4, 5, 8 and 17 key tiles: 129, 320 and 1088 leave the last tile of the two-register-set loop unpaired; 65, 129, 193
# and 449 end in a ragged tile of ONE key (where late_spike puts its spike), 320 and 1088 in a full one
TKS = (65, 129, 193, 320, 449, 1088)
WIDE_TQ = ((130, 2), (257, 3))                  # (Tq, workgroup shape) at n * heads = 256
WIDE_DH = (40, 80)
WIDE_PROFILES = ("rise5", "threshold")
PADS = (8, 16, 24, 4)


RISE = {"rise3": 3.0, "rise5": 5.0, "rise9": 9.0}
CLIMB_BITS = 10.0


def climbs(case: "Case") -> bool:
    """A rise* case whose profile puts a FULL key tile at least 10 bits above tile 0: the 2^8 threshold plus 2 bits, three
    standard deviations of what the randn columns add (the maxima of two tiles of 64 scores of about N(0, 1) nats differ
    by about +-0.65 bits).  There nearly every class +1 row must move; a shorter sample cannot reach the threshold by
    construction (rise3 needs 5 tiles, rise5 4, rise9 3) and is in the rotation for its tile count and ragged tile."""
    return case.profile in RISE and RISE[case.profile] * (case.Tk // TILE - 1) >= CLIMB_BITS


def every_head_dim_cases(dh: int, fmt: str) -> List[Case]:
    """Shape 1 (n * heads = 6, Tq = 65): every profile against a Tk, rotated by the head dim so that the twelve head dims
    between them meet all 36 (profile, Tk) pairs twice."""
    i = SD_HEAD_DIMS.index(dh)
    return [Case(p, fmt, 2, 3, dh, 65, TKS[(j + i) % len(TKS)]) for j, p in enumerate(PROFILES)]


def wide_cases(dh: int, fmt: str, Tq: int) -> List[Case]:
    return [Case(p, fmt, 32, 8, dh, Tq, 193) for p in WIDE_PROFILES]


def stride_case(fmt: str) -> Case:
    return Case("rise5", fmt, 2, 3, 40, 65, 320)


def containment_case(fmt: str) -> Case:
    return Case("rise5", fmt, 2, 3, 56, 65, 320)


def determinism_case(fmt: str) -> Case:
    return Case("rise9", fmt, 2, 3, 24, 65, 320)


def gpu_cases() -> List[Case]:
    """Every case tests/test_gpu_sd_attention_values.py compares with the bound, once."""
    out: List[Case] = []
    for fmt in FMTS:
        for dh in SD_HEAD_DIMS:
            out += every_head_dim_cases(dh, fmt)
        for dh in WIDE_DH:
            for Tq, _ in WIDE_TQ:
                out += wide_cases(dh, fmt, Tq)
        out += [stride_case(fmt), containment_case(fmt), determinism_case(fmt)]
    return list(dict.fromkeys(out))
