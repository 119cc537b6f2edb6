"""CPU: the restatement of the similarity-metric kernels (tests/similarity_ref.py) pinned to scipy, to the reference's edge
behaviour and to the separation between a one-pass and a two-pass Pearson that the GPU tests rely on."""
import math
from pathlib import Path

import numpy as np
import pytest
from scipy import stats
from scipy.spatial.distance import cosine as scipy_cosine

import similarity_ref as ref


def kinds(n, seed):
    rng = np.random.default_rng(seed)
    yield "gauss", rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    yield "half-grid", (np.round(rng.standard_normal(n) * 4) / 2).astype(np.float32), (np.round(rng.standard_normal(n) * 4) / 2).astype(np.float32)
    yield "small-int", rng.integers(-2, 3, n).astype(np.float32), rng.integers(-2, 3, n).astype(np.float32)


@pytest.mark.parametrize("n", [2, 3, 5, 17, 64, 257, 1000, 4096, 20000, 100000])
def test_integer_spearman_equals_scipy(n):
    worst = 0.0
    for kind, x, y in kinds(n, 100 + n):
        for v in (x, y):
            assert int((ref.centred_ranks(v) + (n + 1)).sum()) == n * (n + 1), kind          # the doubled ranks sum to n (n + 1)
            assert np.array_equal(ref.centred_ranks(v) + (n + 1), np.round(2 * stats.rankdata(v)).astype(np.int64)), kind
        if np.ptp(x) == 0 or np.ptp(y) == 0:
            continue
        got, want = ref.spearman(x, y), stats.spearmanr(x.astype(np.float64), y.astype(np.float64))[0]
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= 2.0 ** -50, (kind, got, want)
    print(f"n = {n}: worst |integer Spearman - scipy| = {worst:.2e}")


def test_int64_rank_sums_equal_python_int_sums():
    rng = np.random.default_rng(5)
    for n in (1, 2, 77, 5000):
        x, y = rng.integers(-50, 50, n).astype(np.int32), rng.integers(-50, 50, n).astype(np.int32)
        cx, cy = [int(c) for c in ref.centred_ranks(x)], [int(c) for c in ref.centred_ranks(y)]
        assert ref.rank_sums(x, y) == (sum(a * b for a, b in zip(cx, cy)), sum(a * a for a in cx), sum(b * b for b in cy))
        assert max(map(abs, cx), default=0) <= n - 1
    n = ref.MAX_N                                     # the largest sums the interface admits stay inside int64
    x = np.arange(n, dtype=np.float32)
    sxy, sxx, syy = ref.rank_sums(x, x[::-1])
    want = n * (n * n - 1) // 3                       # the sum over i < n of (2 i - (n - 1))^2
    assert sxx == syy == want == -sxy and want < 2 ** 63 and n * (n - 1) ** 2 < 2 ** 63


# ---- what the reference's five functions do at the edges (thin wrappers of scipy; restated here, the reference is not read)
def reference_like(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out = {}
    with np.errstate(all="ignore"):
        out["cosine_similarity"] = 0.0 if np.linalg.norm(x) == 0 or np.linalg.norm(y) == 0 else 1 - scipy_cosine(x, y)
        for name, fn in (("pearson_correlation", stats.pearsonr), ("spearman_correlation", stats.spearmanr)):
            try:
                c = fn(x, y)[0]
                out[name] = 0.0 if np.isnan(c) else float(c)
            except Exception:
                out[name] = 0.0
    return out


def public(x, y):
    """the restatement as the public functions report it: an undefined correlation is 0.0"""
    v, _ = ref.restate(np.asarray(x, np.float32), np.asarray(y, np.float32))
    return {"cosine_similarity": v[0], "pearson_correlation": 0.0 if np.isnan(v[3]) else v[3],
            "spearman_correlation": 0.0 if np.isnan(v[4]) else v[4]}


@pytest.mark.filterwarnings("ignore")
def test_edge_behaviour_of_the_reference_functions():
    a = np.arange(8, dtype=np.float64)
    b = np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.float64)
    const = reference_like(np.full(8, 0.1), b)
    assert const["pearson_correlation"] == 0.0 and const["spearman_correlation"] == 0.0
    assert public(np.full(8, 0.1), b)["pearson_correlation"] == 0.0 and public(np.full(8, 0.1), b)["spearman_correlation"] == 0.0
    one = reference_like([2.0], [3.0])
    assert one["pearson_correlation"] == 0.0 and one["spearman_correlation"] == 0.0
    assert public([2.0], [3.0])["pearson_correlation"] == 0.0 and public([2.0], [3.0])["spearman_correlation"] == 0.0
    an = a.copy(); an[3] = np.nan
    wn, gn = reference_like(an, b), public(an, b)
    assert wn["pearson_correlation"] == 0.0 and wn["spearman_correlation"] == 0.0 and np.isnan(wn["cosine_similarity"])
    assert gn["pearson_correlation"] == 0.0 and gn["spearman_correlation"] == 0.0 and np.isnan(gn["cosine_similarity"])
    ai = a.copy(); ai[3] = np.inf
    wi, gi = reference_like(ai, a), public(ai, a)
    assert wi["pearson_correlation"] == 0.0 and gi["pearson_correlation"] == 0.0
    assert abs(wi["spearman_correlation"] - 0.7619047619047619) < 1e-15 and abs(gi["spearman_correlation"] - wi["spearman_correlation"]) <= 2.0 ** -50
    zero = reference_like(np.zeros(8), b)
    assert zero["cosine_similarity"] == 0.0 and public(np.zeros(8), b)["cosine_similarity"] == 0.0
    # -0.0 ties with 0.0, and a row of both is constant
    assert np.isnan(ref.restate(np.array([0.0, -0.0, 0.0], np.float32), np.array([1, 2, 3], np.float32))[0][3:]).all()
    assert ref.restate(np.array([0.0, -0.0, 1.0], np.float32), np.array([5, 5, 7], np.float32))[1][:3] == list(ref.rank_sums([0, 0, 1], [5, 5, 7]))


def test_restatement_agrees_with_scipy_and_with_the_exact_values():
    for n in (2, 3, 65, 512, 4097):
        for kind, x, y in kinds(n, 900 + n):
            v, ints = ref.restate(x, y)
            t = ref.truth(x, y)
            if np.ptp(x) == 0 or np.ptp(y) == 0:
                continue
            x64, y64 = x.astype(np.float64), y.astype(np.float64)
            assert abs(v[3] - stats.pearsonr(x64, y64)[0]) < 1e-12 and abs(v[4] - stats.spearmanr(x64, y64)[0]) <= 2.0 ** -50
            assert abs(v[0] - (1 - scipy_cosine(x64, y64))) < 1e-12
            assert abs(v[1] - np.linalg.norm(x64 - y64)) <= 1e-12 * v[1] and abs(v[2] - np.abs(x64 - y64).sum()) <= 1e-12 * v[2]
            # exact sums leave the closing formulas' few roundings only
            assert abs(v[0] - t["cosine_similarity"]) <= 2.0 ** -50 and abs(v[3] - t["pearson_correlation"]) <= 2.0 ** -50, (n, kind)
            assert ints[3] == 0 and v[4] == ref.spearman(x, y)


def test_restatement_reproduces_the_reference_fixture():
    """tests/golden/simmetrics.npz was written by the reference's own code (tests/make_simmetrics_fixture.py)"""
    g = np.load(Path(__file__).resolve().parent / "golden" / "simmetrics.npz")
    cases = [(g["E1"].reshape(-1), g["E2"].reshape(-1), g["flat"])] + list(zip(g["X"], g["Y"], g["rows"]))
    for x, y, want in cases:
        v, _ = ref.restate(x, y)
        v[3:] = np.where(np.isnan(v[3:]), 0.0, v[3:])
        tol = 2 * ref.B(x.size)
        assert abs(v[0] - want[0]) <= tol and abs(v[3] - want[3]) <= tol and abs(v[4] - want[4]) <= tol
        assert abs(v[1] - want[1]) <= tol * want[1] and abs(v[2] - want[2]) <= tol * want[2]
    assert g["rows"][5, 3] == 0.0 and g["rows"][5, 4] == 0.0 and g["rows"][7, 0] == 0.0           # the constant and the zero row
    assert np.signbit(g["X"][0, 1]) and g["X"][0, 1] == 0.0
    for a, b, score, rank, topk in zip(g["idx1"], g["idx2"], g["score"], g["rank"], g["topk"]):
        assert abs(ref.spearman(a, b) - rank) <= 2.0 ** -50
        assert [ref.overlap(a, b, int(k)) / int(k) for k in g["ks"]] == topk.tolist()
        assert len(set(a.tolist())) < a.size and set(a.tolist()) & set(b.tolist())              # repeats inside, ids shared
    for a, b, score in zip(g["s1"], g["s2"], g["score"]):
        assert abs(ref.restate(a, b)[0][3] - score) <= 2 * ref.B(a.size)


def test_integer_rows_have_integer_means_and_signed_zeros():
    for D in (1, 2, 3, 65, 1000):
        X, Y = ref.integer_rows(5, D, seed=D)
        for M in (X, Y):
            assert M.dtype == np.float32 and np.abs(M).max() <= 2 and np.array_equal(M, np.round(M))
            assert np.array_equal(M.sum(1) % D, np.zeros(5))
        if D >= 65:
            assert np.signbit(X[X == 0]).any() and not np.signbit(X[X == 0]).all()
            assert len({float(m) for m in np.r_[X.mean(1), Y.mean(1)]}) > 1            # not all means zero


def test_strided_sum_is_a_sum_in_another_order():
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 300, 4096):
        t = rng.integers(-1000, 1000, n).astype(np.float64)
        for T in (64, 256):
            assert ref.strided_sum(t, T) == t.sum()                  # exact on integers
        g = rng.standard_normal(n)
        assert abs(ref.strided_sum(g, 256) - math.fsum(g)) <= ref.chain(n) * 2.0 ** -53 * np.abs(g).sum() + 1e-300


# ---- the planted offset rows tell a one-pass Pearson from a two-pass one
@pytest.mark.parametrize("n, offset, flat", [(65, 64.0, False), (512, 64.0, False), (3072, 64.0, False), (4096, 64.0, False),
                                             (70001, 1024.0, True)])
def test_offset_rows_separate_one_pass_from_two_pass_pearson(n, offset, flat):
    x, y = ref.offset_rows(n, offset, seed=n)
    t = ref.truth(x, y)
    want, kappa = t["pearson_correlation"], t["kappa"]
    assert kappa > 4 * offset
    bound = ref.pearson_bound(n, kappa)
    one = abs(float(np.longdouble(ref.pearson_one_pass(x, y)) - want))
    # the long form adds 4 096-element chunks in the row kernel's order and then the chunks: the row order over the whole vector
    # has longer chains, so it bounds what the test needs from a two-pass sum
    two = abs(float(np.longdouble(ref.pearson_two_pass(x, y)) - want))
    print(f"n = {n}, offset {offset:g}: kappa {kappa:.0f}, bound {bound:.2e}, one-pass {one / bound:.1f} x, two-pass {two / bound:.5f} x of it")
    assert one > bound
    assert two < 0.01 * bound
    assert two <= ref.pearson_kernel_bound(n, kappa, flat) or flat
