"""The similarity-metric kernels restated on the host (tvc_sim_rows / tvc_sim_flat / tvc_topk_overlap, include/tvc.h).

Three things, all pure numpy / Python:
  ``centred_ranks`` / ``rank_sums`` / ``spearman``   the exact integer Spearman: c = lo + hi - n from ``searchsorted`` on the
      sorted row, the three sums of products as Python ints, rho by the interface's closing formula.
  ``restate``   the interface's outputs (fp64 [5], int [4]) with every sum taken EXACTLY (``math.fsum``: the correctly rounded
      sum) and the closing formulas, specials and the one quiet NaN as documented -- equal to the kernels bit for bit wherever
      the kernels' own fp64 sums are exact (integer data whose means are integers).
  ``truth``     the exact metrics of the fp32 elements in ``np.longdouble`` (64-bit mantissa; numpy sums pairwise, so an
      n-term sum is good to about log2(n) 2^-64), with kappa, for the error bounds ``B`` / ``Bk`` / ``pearson_bound`` / ....
``strided_sum`` replays the kernels' summation order (thread-strided partials, a butterfly per wave, the waves in order) and
``pearson_one_pass`` is the formula the interface rules out; tests/test_similarity_ref.py tells the two apart."""
import math

import numpy as np

QNAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]
MAX_D, MAX_N = 4096, 1 << 20
NAMES = ("cosine_similarity", "euclidean_distance", "manhattan_distance", "pearson_correlation", "spearman_correlation")


# ---- bounds (include/tvc.h) -----------------------------------------------------------------------------------------------
def row_threads(n: int) -> int:
    return 64 if n <= 256 else 256


def chain(n: int, flat: bool = False) -> int:
    """c(n): the rounding additions a term passes through at most"""
    return min(n - 1, 33) if flat else min(n - 1, -(-n // row_threads(n)) + 8)


def B(n: int) -> float:
    return 2.0 ** -52 * (2 * n + 16)


def Bk(n: int, flat: bool = False) -> float:
    return 2.0 ** -52 * (chain(n, flat) + 2)


def pearson_bound(n: int, kappa: float) -> float:
    return B(n) + (2.0 ** -52 * n * kappa) ** 2


def pearson_kernel_bound(n: int, kappa: float, flat: bool = False) -> float:
    c = chain(n, flat)
    return 2.0 ** -52 * (c + 5) + (2.0 ** -52 * (c + 1) * kappa) ** 2


# ---- exact integer Spearman -----------------------------------------------------------------------------------------------
def centred_ranks(v) -> np.ndarray:
    """int64 [n]: c = lo + hi - n, lo = #(row < v_i), hi = #(row <= v_i); -0.0 ties with 0.0; integers compare as integers"""
    v = np.asarray(v).reshape(-1)
    if v.dtype.kind == "f":
        v = v + v.dtype.type(0)               # -0.0 -> 0.0 (searchsorted would tie them anyway)
    s = np.sort(v)
    return (np.searchsorted(s, v, "left") + np.searchsorted(s, v, "right") - v.size).astype(np.int64)


def rank_sums(x, y):
    """(sum cx cy, sum cx cx, sum cy cy) as Python ints; int64 sums are exact here: |c| <= n - 1 and n (n - 1)^2 < 2^63 up to
    n = 2^20 (pinned against Python-int sums by tests/test_similarity_ref.py)"""
    cx, cy = centred_ranks(x), centred_ranks(y)
    assert cx.size <= MAX_N
    return int((cx * cy).sum()), int((cx * cx).sum()), int((cy * cy).sum())


def spearman_from_sums(sxy: int, sxx: int, syy: int, n: int) -> float:
    if n < 2 or sxx == 0 or syy == 0:
        return QNAN
    return float(sxy) / math.sqrt(float(sxx) * float(syy))          # float(int) rounds to nearest even, as (double)int64


def spearman(x, y) -> float:
    return spearman_from_sums(*rank_sums(x, y), np.asarray(x).size)


# ---- the interface restated with exact sums -------------------------------------------------------------------------------
def _sum(t: np.ndarray) -> float:
    return math.fsum(t) if np.isfinite(t).all() else float(np.sum(t))


def _canon(v: float) -> float:
    return QNAN if v != v else float(v)


def restate(x, y):
    """-> (values fp64 [5], ints object [4]) of ONE pair of fp32 or integer rows, as tvc_sim_rows documents them"""
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    n = x.size
    integer = x.dtype.kind in "iu"
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    nan = 0 if integer else int(np.isnan(x).sum() + np.isnan(y).sum())
    with np.errstate(all="ignore"):
        sxy, sxx, syy = _sum(xd * yd), _sum(xd * xd), _sum(yd * yd)
        d = xd - yd
        cos = np.float64(sxy) / np.sqrt(np.float64(sxx) * np.float64(syy))
        if nan == 0 and (sxx == 0.0 or syy == 0.0):
            cos = 0.0
        l2, l1 = np.sqrt(np.float64(_sum(d * d))), _sum(np.abs(d))
        r = QNAN
        if n >= 2 and np.nanmin(xd, initial=np.inf) != np.nanmax(xd, initial=-np.inf) and \
                np.nanmin(yd, initial=np.inf) != np.nanmax(yd, initial=-np.inf):
            mx, my = np.float64(_sum(xd)) / np.float64(n), np.float64(_sum(yd)) / np.float64(n)
            cx, cy = xd - mx, yd - my
            r = np.float64(_sum(cx * cy)) / np.sqrt(np.float64(_sum(cx * cx)) * np.float64(_sum(cy * cy)))
            r = 1.0 if r > 1.0 else (-1.0 if r < -1.0 else r)
    ints = [0, 0, 0, nan]
    rho = QNAN
    if nan == 0:
        ints[:3] = rank_sums(x, y)
        rho = spearman_from_sums(*ints[:3], n)
    return np.array([_canon(cos), _canon(l2), _canon(l1), _canon(r), _canon(rho)], dtype=np.float64), ints


def restate_rows(X, Y):
    """-> (values fp64 [B, 5], ints int64 [B, 4]) of the pairs (X[b], Y[b])"""
    out = [restate(x, y) for x, y in zip(X, Y)]
    return (np.array([v for v, _ in out], dtype=np.float64).reshape(len(out), 5),
            np.array([i for _, i in out], dtype=np.int64).reshape(len(out), 4))


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the exact values, for the bounds -------------------------------------------------------------------------------------
def truth(x, y):
    """-> dict of the five exact values (longdouble; Spearman from the integers) and 'kappa' of one pair of finite rows"""
    L = np.longdouble
    xl, yl = np.asarray(x).reshape(-1).astype(L), np.asarray(y).reshape(-1).astype(L)
    n = xl.size
    d = xl - yl
    with np.errstate(all="ignore"):                   # a zero row: 0 / 0, the caller's case
        out = {"cosine_similarity": (xl * yl).sum() / np.sqrt((xl * xl).sum() * (yl * yl).sum()),
               "euclidean_distance": np.sqrt((d * d).sum()), "manhattan_distance": np.abs(d).sum()}
    cx, cy = xl - xl.sum() / L(n), yl - yl.sum() / L(n)
    vx, vy = (cx * cx).sum(), (cy * cy).sum()
    out["pearson_correlation"] = (cx * cy).sum() / np.sqrt(vx * vy) if n >= 2 and vx > 0 and vy > 0 else L("nan")
    out["spearman_correlation"] = L(spearman(x, y))
    with np.errstate(all="ignore"):
        out["kappa"] = float(max(np.abs(xl).mean() / np.sqrt(vx / L(n)), np.abs(yl).mean() / np.sqrt(vy / L(n)))) if n >= 2 else 0.0
    return out


# ---- the two Pearson forms, in fp64 ---------------------------------------------------------------------------------------
def strided_sum(t: np.ndarray, T: int) -> np.float64:
    """sum of the fp64 terms in the kernels' order: thread i adds t[i], t[i + T], ...; a butterfly (distances 32 .. 1) inside
    every wave of 64 threads; then the waves' sums in wave order"""
    t = np.asarray(t, dtype=np.float64)
    pad = -t.size % T
    acc = np.zeros(T, dtype=np.float64)
    for row in np.concatenate([t, np.zeros(pad)]).reshape(-1, T):
        acc = acc + row
    lane = np.arange(T)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lane ^ o]
    s = acc[0]
    for w in range(1, T // 64):
        s = s + acc[64 * w]
    return np.float64(s)


def pearson_two_pass(x, y) -> np.float64:
    """the interface's Pearson in the row kernel's summation order"""
    xd, yd = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, T = xd.size, row_threads(xd.size)
    cx, cy = xd - strided_sum(xd, T) / np.float64(n), yd - strided_sum(yd, T) / np.float64(n)
    r = strided_sum(cx * cy, T) / np.sqrt(strided_sum(cx * cx, T) * strided_sum(cy * cy, T))
    return np.float64(min(max(r, -1.0), 1.0))


def pearson_one_pass(x, y) -> np.float64:
    """the textbook one-pass form (sums of x, y, x y, x x, y y; then the subtraction): NOT what the interface allows"""
    xd, yd = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = np.float64(xd.size)
    sx, sy, sxy, sxx, syy = xd.sum(), yd.sum(), (xd * yd).sum(), (xd * xd).sum(), (yd * yd).sum()
    return np.float64((sxy - sx * sy / n) / np.sqrt((sxx - sx * sx / n) * (syy - sy * sy / n)))


# ---- data -----------------------------------------------------------------------------------------------------------------
def offset_rows(n: int, offset: float, seed: int):
    """x = offset + g / 8, y = -offset + g' / 8 in fp32, g' correlated with g: kappa is about 8 * offset"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n)
    h = 0.6 * g + 0.8 * rng.standard_normal(n)
    return (offset + g / 8).astype(np.float32), (-offset + h / 8).astype(np.float32)


def integer_rows(B: int, D: int, seed: int):
    """-> (X, Y) fp32 [B, D] with entries in {-2 .. 2}, 0.0 / -0.0 planted, and every row's MEAN an integer (a row is values of
    {-1, 0, 1} that sum to 0, plus an offset in {-1, 0, 1}): means, centred values and every sum of the kernels are then exact
    in fp64 in any order, so the kernels must equal ``restate`` bit for bit.  Rows are full of ties."""
    rng = np.random.default_rng(seed)

    def rows():
        M = rng.integers(-1, 2, size=(B, D)).astype(np.int64)
        for r in M:                                    # move the row's sum to 0 one element at a time
            s = int(r.sum())
            idx = np.flatnonzero(r > -1) if s > 0 else np.flatnonzero(r < 1)
            take = rng.permutation(idx)
            k = 0
            while s != 0 and D > 1:
                j = take[k % take.size]
                if s > 0 and r[j] > -1:
                    r[j] -= 1; s -= 1
                elif s < 0 and r[j] < 1:
                    r[j] += 1; s += 1
                k += 1
            if D == 1:
                r[0] = 0
        M = (M + rng.integers(-1, 2, size=(B, 1))).astype(np.float32)
        zero = M == 0
        M[zero & (rng.random((B, D)) < 0.5)] = -0.0
        return M

    return rows(), rows()


def overlap(a, b, k: int) -> int:
    return len(set(np.asarray(a)[:k].tolist()) & set(np.asarray(b)[:k].tolist()))
