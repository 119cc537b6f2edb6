"""The image preprocessing (``tvc_preprocess_images``: resize_norm_kernel of csrc/sd_ops.hip) against fp64, element by element
(plain helper module: no GPU, no fixtures).  tests/test_resize_ref.py checks everything here on the CPU,
tests/test_gpu_preprocess_values.py runs the kernel on the same cases, tests/test_preprocess_host.py holds the host path
(``CLIPModel.preprocess``, Pillow on 8-bit pixels) to the same reference.

* ``resized_size`` the size rule of include/tvc.h as a spec: short side to S, long side floor(long * S / short + 1/2) in exact
                   integer arithmetic, never below S, crop offset (resized - S) // 2.
* ``weights``      one axis of the separable filter, fp64 [S, n_in], rows normalised: scale = n_in / n_resized, f = max(scale, 1),
                   support (2 if cubic else 1) f, centre c = (o + offset + 0.5) scale, window
                   [max(int(c - sup + 0.5), 0), min(int(c + sup + 0.5), n_in)), tap argument (i + 0.5 - c) / f, cubic a = -0.5.
* ``reference``    (out, bound): out = (Wy x Wx^T - mean) / std in fp64 on the values the kernel reads (fp32 pixels, fp32 mean
                   and std).  The bound on |got - out| holds for EVERY element and is a function of reference quantities only
                   ("Image preprocessing: values"); u = 2^-24, per axis and per tap of the window widened by one:

                       e = (L u (2 c / f + 3 |t|) + E) / sum(w)      L = 1, E = u (bilinear); L = 25 / 18, E = 24 u (cubic)
                       A = |W| + e,  k = taps + 2,  m = the mean of the image's channel,  r = Wy x Wx^T
                       rw = sum(ey) sum(|Wx|) + sum(Ay) sum(ex)                      (weight errors act on x - r only:
                       rr = (ky - 1) u sum(Ay) + (kx - 1) u sum(Ax) + u               they cancel on a constant image)
                       b = (ey |x - m| |Wx|^T + Ay |x - m| ex^T + |r - m| rw + (ky + kx) u Ay |x| Ax^T) (1 + rw + rr)
                           + |r| (rr + u)
                       bound = 1.01 ((b + u |r - mean|) / std + u |out|)

                   ``reach`` is the widened window itself: an output whose reach holds only zeros is exactly 0.
* ``emulate``      the kernel's arithmetic in numpy float32 in the kernel's order, one rounding per operation (the compiler may
                   contract a * b + c, which only removes roundings).  ``defect=`` applies one of ``DEFECTS``.
* ``gpu_cases``    the cases of the GPU file, shared so that the CPU file proves its claims on exactly those.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from functools import lru_cache
from typing import List, Optional, Tuple

import numpy as np

U = 2.0 ** -24
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
UNIT_MEAN, UNIT_STD = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)

DEFECTS = (
    "cubic_a_minus_0_75",                       # the other common bicubic
    "support_not_scaled_when_shrinking",        # f = 1: no antialiasing
    "weights_not_normalised",
    "centre_without_half",                      # c = (o + offset) scale
    "crop_offset_rounded_up",                   # (resized - S + 1) // 2
    "row_scale_used_for_columns",
    "upper_window_clamp_at_n_in_minus_1",
    "mean_std_from_wrong_channel",              # channel (c + 1) % 3
    "long_side_truncated",                      # floor(long * S / short)
    "long_side_rounded_half_to_even",           # Python's round
)
# a GPU case on which ``emulate`` with the defect leaves the bound (test_resize_ref.py asserts each)
DEFECT_CASE = {
    "cubic_a_minus_0_75": "values-512x512-S224-cubic-crop",
    "support_not_scaled_when_shrinking": "values-512x512-S224-linear-full",
    "weights_not_normalised": "witness-512x512-S224-linear-full",
    "centre_without_half": "witness-128x128-S224-cubic-crop",
    "crop_offset_rounded_up": "values-449x448-S224-linear-crop",      # Hr - S = 1 is odd (300 x 420: 90, no difference)
    "row_scale_used_for_columns": "values-2000x37-S64-linear-full",
    "upper_window_clamp_at_n_in_minus_1": "witness-7x5-S32-linear-full",
    "mean_std_from_wrong_channel": "values-100x150-S7-cubic-crop",
    "long_side_truncated": "values-449x448-S224-cubic-crop",
    "long_side_rounded_half_to_even": "values-449x448-S224-linear-crop",
}


# ------------------------------------------------------------------------------------------------------- the size rule
def resized_size(H: int, W: int, S: int, keep_aspect: bool, defect: Optional[str] = None) -> Tuple[int, int, int, int]:
    """(Hr, Wr, oy, ox): the size the image is resized to and where the S x S crop starts."""
    def long_side(long: int, short: int) -> int:
        if defect == "long_side_truncated":
            r = long * S // short
        elif defect == "long_side_rounded_half_to_even":
            q, rem = divmod(2 * long * S, 2 * short)
            r = q + (1 if rem > short or (rem == short and q % 2 == 1) else 0)
        else:
            r = (2 * long * S + short) // (2 * short)
        return max(r, S)

    Hr = Wr = S
    if keep_aspect:
        if H <= W:
            Wr = long_side(W, H)
        else:
            Hr = long_side(H, W)
    up = 1 if defect == "crop_offset_rounded_up" else 0
    return Hr, Wr, (Hr - S + up) // 2, (Wr - S + up) // 2


# ------------------------------------------------------------------------------------------------------------ one axis
def _filter(t, cubic: bool, a: float):
    t = np.abs(t)
    one = t.dtype.type(1)
    if not cubic:
        return np.where(t < 1, one - t, 0 * t)
    a = t.dtype.type(a)
    near = ((a + 2) * t - (a + 3)) * t * t + one
    far = (((t - 5) * t + 8) * t - 4) * a
    return np.where(t < 1, near, np.where(t < 2, far, 0 * t))


def _axis(n_in: int, n_resized: int, offset: int, S: int, cubic: bool, dtype, defect: Optional[str] = None,
          scale_of: Optional[Tuple[int, int]] = None):
    """The kernel's statements for one axis in ``dtype``: (w [S, n_in] unnormalised and 0 outside the window, lo [S], hi [S],
    c [S], f, t [S, n_in]).  ``scale_of``: (n_in, n_resized) the scale is taken from (a defect)."""
    T = dtype
    si, sr = scale_of or (n_in, n_resized)
    scale = T(si) / T(sr)
    f = T(1) if (scale <= 1 or defect == "support_not_scaled_when_shrinking") else scale
    sup = T(2 if cubic else 1) * f
    o = (np.arange(S) + offset).astype(T)
    c = (o if defect == "centre_without_half" else o + T(0.5)) * scale
    lo = np.maximum(np.trunc(c - sup + T(0.5)).astype(np.int64), 0)
    hi = np.minimum(np.trunc(c + sup + T(0.5)).astype(np.int64), n_in - 1 if defect == "upper_window_clamp_at_n_in_minus_1" else n_in)
    i = np.arange(n_in)
    t = ((i.astype(T) + T(0.5))[None, :] - c[:, None]) / f
    w = _filter(t, cubic, -0.75 if defect == "cubic_a_minus_0_75" else -0.5)
    w = np.where((i[None, :] >= lo[:, None]) & (i[None, :] < hi[:, None]), w, T(0))
    assert w.dtype == T and c.dtype == T and t.dtype == T
    return w, lo, hi, c, f, t


def weights(n_in: int, n_resized: int, offset: int, S: int, cubic: bool) -> np.ndarray:
    """fp64 [S, n_in]: the normalised taps of output pixels offset .. offset + S - 1 of an n_in -> n_resized resize."""
    w = _axis(n_in, n_resized, offset, S, cubic, np.float64)[0]
    return w / w.sum(1, keepdims=True)


def _widened(lo: np.ndarray, hi: np.ndarray, n_in: int) -> np.ndarray:
    i = np.arange(n_in)[None, :]
    return (i >= lo[:, None] - 1) & (i < hi[:, None] + 1)


def _axis_bound(n_in: int, n_resized: int, offset: int, S: int, cubic: bool):
    """(W normalised, e, A = |W| + e, k) of the module docstring."""
    w, lo, hi, c, f, t = _axis(n_in, n_resized, offset, S, cubic, np.float64)
    ws = w.sum(1, keepdims=True)
    assert (ws > 0.25).all()                                         # the tap nearest the centre is always inside
    L, E = (25.0 / 18.0, 24 * U) if cubic else (1.0, U)
    e = np.where(_widened(lo, hi, n_in), L * U * (2 * c[:, None] / f + 3 * np.abs(t)) + E, 0.0) / ws
    return w / ws, e, np.abs(w / ws) + e, (hi - lo) + 2


def reach(n_in: int, n_resized: int, offset: int, S: int, cubic: bool) -> np.ndarray:
    """bool [S, n_in]: the taps an fp32 evaluation of the window can read (the fp64 window widened by one tap on each side)."""
    _, lo, hi = _axis(n_in, n_resized, offset, S, cubic, np.float64)[:3]
    return _widened(lo, hi, n_in)


def _sep(Ly: np.ndarray, x: np.ndarray, Lx: np.ndarray) -> np.ndarray:
    return np.matmul(np.matmul(Ly, x), Lx.T)                         # [S, H] [n, 3, H, W] [W, S] -> [n, 3, S, S]


def _f32(v) -> np.ndarray:
    return np.asarray(v, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)


def reference(x: np.ndarray, S: int, cubic: bool, keep_aspect: bool, mean, std) -> Tuple[np.ndarray, np.ndarray]:
    """x fp32 [n, 3, H, W] -> (out, bound), both fp64 [n, 3, S, S]."""
    assert x.dtype == np.float32 and x.ndim == 4 and x.shape[1] == 3
    H, W = x.shape[2:]
    Hr, Wr, oy, ox = resized_size(H, W, S, keep_aspect)
    Wy, ey, Ay, ky = _axis_bound(H, Hr, oy, S, cubic)
    Wx, ex, Ax, kx = _axis_bound(W, Wr, ox, S, cubic)
    x64 = x.astype(np.float64)
    mid = x64.mean((2, 3), keepdims=True)
    ax, dx = np.abs(x64), np.abs(x64 - mid)
    r = _sep(Wy, x64, Wx)
    col, rowv = (lambda v: v.sum(1)[:, None]), (lambda v: v.sum(1)[None, :])
    rw = col(ey) * rowv(np.abs(Wx)) + col(Ay) * rowv(ex)
    rr = (ky[:, None] - 1) * U * col(Ay) + (kx[None, :] - 1) * U * rowv(Ax) + U
    K = (ky[:, None] + kx[None, :]).astype(np.float64)
    b = ((_sep(ey, dx, np.abs(Wx)) + _sep(Ay, dx, ex) + np.abs(r - mid) * rw + K * U * _sep(Ay, ax, Ax)) * (1 + rw + rr)
         + np.abs(r) * (rr + U))
    m, s = _f32(mean), _f32(std)
    out = (r - m) / s
    return out, 1.01 * ((b + U * np.abs(r - m)) / s + U * np.abs(out))


# --------------------------------------------------------------------------------------------------- the kernel in fp32
def _running(w: np.ndarray, lo: np.ndarray, hi: np.ndarray, term) -> np.ndarray:
    """sum over the window, tap by tap from ``lo`` in fp32: acc += term(tap index [S], tap weight [S])."""
    acc = None
    for k in range(int((hi - lo).max())):
        idx = np.minimum(lo + k, w.shape[1] - 1)
        wk = np.where(lo + k < hi, w[np.arange(len(lo)), idx], np.float32(0))
        acc = term(idx, wk) if acc is None else acc + term(idx, wk)
    return acc


def emulate(x: np.ndarray, S: int, cubic: bool, keep_aspect: bool, mean, std, defect: Optional[str] = None) -> np.ndarray:
    """resize_norm_kernel statement by statement in float32: x fp32 [n, 3, H, W] -> fp32 [n, 3, S, S]."""
    assert x.dtype == np.float32 and (defect is None or defect in DEFECTS)
    H, W = x.shape[2:]
    Hr, Wr, oy, ox = resized_size(H, W, S, keep_aspect, defect)
    wy, ylo, yhi = _axis(H, Hr, oy, S, cubic, np.float32, defect)[:3]
    wx, xlo, xhi = _axis(W, Wr, ox, S, cubic, np.float32, defect,
                         scale_of=(H, Hr) if defect == "row_scale_used_for_columns" else None)[:3]
    wys = _running(wy, ylo, yhi, lambda idx, wk: wk)
    wxs = _running(wx, xlo, xhi, lambda idx, wk: wk)
    row = _running(wx, xlo, xhi, lambda idx, wk: wk * x[:, :, :, idx])                           # [n, 3, H, S(x)]
    acc = _running(wy, ylo, yhi, lambda idx, wk: wk[:, None] * row[:, :, idx, :])                # [n, 3, S(y), S(x)]
    if defect != "weights_not_normalised":
        with np.errstate(divide="ignore", invalid="ignore"):         # a defect's empty window: 0 / 0, as in the kernel
            acc = acc / (wys[:, None] * wxs[None, :])
    m, s = (np.asarray(v, dtype=np.float32).reshape(1, 3, 1, 1) for v in (mean, std))
    if defect == "mean_std_from_wrong_channel":
        m, s = np.roll(m, -1, axis=1), np.roll(s, -1, axis=1)
    out = (acc - m) / s
    assert out.dtype == np.float32
    return out


# --------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    kind: str               # values | witness | identity | shrink2 | grid
    H: int
    W: int
    S: int
    cubic: bool
    keep_aspect: bool
    n: int = 0              # grid only

    @property
    def id(self) -> str:
        return f"{self.kind}-{self.H}x{self.W}-S{self.S}-{'cubic' if self.cubic else 'linear'}-{'crop' if self.keep_aspect else 'full'}"

    @property
    def mean_std(self):
        if self.kind != "values":
            return UNIT_MEAN, UNIT_STD                                # the output is the resampled value itself
        return (CLIP_MEAN, CLIP_STD) if self.cubic else (IMAGENET_MEAN, IMAGENET_STD)

    @property
    def images(self) -> Tuple[str, ...]:
        """What image i of the batch holds."""
        return {"values": ("smooth", "noise"), "witness": WITNESS_IMAGES, "identity": ("noise",), "shrink2": ("integers",),
                "grid": ("noise",) * self.n}[self.kind]

    def inputs(self) -> np.ndarray:
        return _inputs(self)

    def reference(self) -> Tuple[np.ndarray, np.ndarray]:
        return _reference(self)


WITNESS_IMAGES = ("constant", "impulse_first", "impulse_last", "impulse_centre", "ramp_x", "ramp_y")
CONSTANT = 0.3


def impulse_at(name: str, H: int, W: int) -> Tuple[int, int]:
    return {"impulse_first": (0, 0), "impulse_last": (H - 1, W - 1), "impulse_centre": (H // 2, W // 2)}[name]


def image(name: str, H: int, W: int, g: np.random.Generator) -> np.ndarray:
    """fp32 [3, H, W], finite, in [0, 1] (``integers``: 0 .. 7)."""
    i, j = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))      # i: column, j: row
    if name == "noise":
        v = g.random((3, H, W))
    elif name == "smooth":                                            # three channels with distinct means and spreads
        v = np.stack([0.5 + a * np.sin(2 * np.pi * (fx * i / W + fy * j / H) + ph)
                      for a, fx, fy, ph in ((0.45, 1.0, 2.0, 0.3), (0.25, 3.0, 1.0, 1.1), (0.1, 2.0, 5.0, 2.0))])
        v = v + np.array([0.0, 0.15, -0.3]).reshape(3, 1, 1)
    elif name == "integers":
        v = g.integers(0, 8, (3, H, W)).astype(np.float64)
    elif name == "constant":
        v = np.full((3, H, W), CONSTANT)
    elif name == "ramp_x":
        v = np.broadcast_to(i / W, (3, H, W))
    elif name == "ramp_y":
        v = np.broadcast_to(j / H, (3, H, W))
    else:
        v = np.zeros((3, H, W))
        v[(slice(None),) + impulse_at(name, H, W)] = 1.0
    return np.ascontiguousarray(v, dtype=np.float32)


@lru_cache(maxsize=2)
def _inputs(c: Case) -> np.ndarray:
    g = np.random.default_rng(zlib.crc32(c.id.encode()))
    x = np.stack([image(name, c.H, c.W, g) for name in c.images])
    x.setflags(write=False)
    return x


@lru_cache(maxsize=2)
def _reference(c: Case) -> Tuple[np.ndarray, np.ndarray]:
    ref, bound = reference(c.inputs(), c.S, c.cubic, c.keep_aspect, *c.mean_std)
    ref.setflags(write=False)
    bound.setflags(write=False)
    return ref, bound


# (H, W, S, keep_aspect values); a shape without a stated mode runs the product's pairing: bicubic + crop, bilinear + both sides
_PRODUCT = ((True, True), (False, False))                             # (cubic, keep_aspect)
_CROP = ((True, True), (False, True))
_ALL = ((True, True), (True, False), (False, True), (False, False))
SHAPES = (
    (512, 512, 224, _PRODUCT),          # the product's shape (64 x 64 latents)
    (128, 128, 224, _PRODUCT),          # upscaling (toy geometries)
    (32, 32, 64, _PRODUCT),
    (300, 420, 224, _CROP),             # crop along x: Wr = 314, odd offset 45
    (420, 300, 224, _CROP),             # crop along y
    (449, 448, 224, _CROP),             # the x.5 size case: Hr = 225
    (2000, 37, 64, _ALL),               # both sides: a 31x shrink, ~125 cubic taps; crop: Wr = S, Hr = 3459
    (7, 5, 32, _PRODUCT),               # windows clamped on both sides
    (2, 3, 8, _PRODUCT),
    (1, 1, 8, _PRODUCT),
    (1, 9, 8, _PRODUCT),
    (100, 150, 7, _PRODUCT),            # S not a multiple of anything
)
GRID = Case("grid", 2, 2, 224, False, False, n=112)                   # n 3 S^2 = 16 859 136 > 65536 * 256: a second grid-stride trip


@lru_cache(maxsize=1)
def gpu_cases() -> Tuple[Case, ...]:
    out: List[Case] = []
    for S in (8, 33):
        out += [Case("identity", S, S, S, cubic, keep) for cubic, keep in _ALL]
    out.append(Case("shrink2", 16, 16, 8, False, False))
    for H, W, S, modes in SHAPES:
        for cubic, keep in modes:
            out += [Case("values", H, W, S, cubic, keep), Case("witness", H, W, S, cubic, keep)]
    out.append(GRID)
    assert len({c.id for c in out}) == len(out)
    return tuple(out)


def case(case_id: str) -> Case:
    return next(c for c in gpu_cases() if c.id == case_id)


def worst(got: np.ndarray, ref: np.ndarray, bound: np.ndarray) -> Tuple[float, Tuple[int, ...], int]:
    """(max |got - ref| / bound, its index, the count over the bound); 0 / 0 = 0 and d / 0 = inf."""
    d = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(d == 0, 0.0, d / bound)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)                  # a non-finite output is outside every bound
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(v) for v in at), int((ratio > 1).sum())


def check_witnesses(c: Case, x: np.ndarray, got: np.ndarray, ref: np.ndarray, bound: np.ndarray) -> None:
    """The equalities a witness case must meet beyond the bound (got fp32 [n, 3, S, S])."""
    if c.kind == "identity":
        assert np.array_equal(got.view(np.int32), x.view(np.int32)), f"{c.id}: the taps are (.., 0, 1, 0, ..): output bits != input bits"
    if c.kind == "shrink2":
        # pixels 0 .. 7 and taps 1 3 3 1 (/ 8): every sum is exact; at the border the divisor is 3.5 or 3.0625, one rounding
        assert np.array_equal(got, ref.astype(np.float32)), f"{c.id}: not the rounded exact value"
        assert np.array_equal(got[:, :, 1:-1, 1:-1].astype(np.float64), ref[:, :, 1:-1, 1:-1]), f"{c.id}: interior not exact"
    if c.kind == "witness":
        Hr, Wr, oy, ox = resized_size(c.H, c.W, c.S, c.keep_aspect)
        k = c.images.index("constant")
        # the weight errors cancel on a constant: what is left is one rounding per tap (window + 2 per axis) of 0.3
        ylo, yhi = _axis(c.H, Hr, oy, c.S, c.cubic, np.float64)[1:3]
        xlo, xhi = _axis(c.W, Wr, ox, c.S, c.cubic, np.float64)[1:3]
        taps = int((yhi - ylo).max() + (xhi - xlo).max() + 4)
        assert bound[k].max() <= taps * U, (c.id, bound[k].max() / U, taps)
        assert np.abs(ref[k] - np.float64(np.float32(CONSTANT))).max() < 1e-15            # so |got - ref| <= bound is |got - c|
        for name in ("impulse_first", "impulse_last", "impulse_centre"):
            k, (h, w) = c.images.index(name), impulse_at(name, c.H, c.W)
            zero = ~(reach(c.H, Hr, oy, c.S, c.cubic)[:, h][:, None] & reach(c.W, Wr, ox, c.S, c.cubic)[:, w][None, :])
            assert (ref[k][:, zero] == 0).all() and (got[k][:, zero] == 0).all(), f"{c.id}: {name} leaks outside its taps"
