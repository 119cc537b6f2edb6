"""GPU: the similarity-metric kernels (tvc_sim_rows, tvc_sim_flat_rank / tvc_sim_flat, tvc_topk_overlap) and the reference's names
over them, against the restatement of tests/similarity_ref.py (pinned to scipy by tests/test_similarity_ref.py) and the fixture
written by the reference's own code (tests/make_simmetrics_fixture.py).

The contract (include/tvc.h).  Where every fp64 sum is exact -- integer rows whose means are integers -- all five columns and all
four integers equal the restatement bit for bit, NaN patterns included.  Otherwise, against the exact value on the fp32
elements: cosine within Bk(n) = 2^-52 (c(n) + 2) absolute, Euclidean and Manhattan within Bk(n) relative, Pearson within
2^-52 (c(n) + 5) + (2^-52 (c(n) + 1) kappa)^2, with c(n) the kernel's chain length (the interface's looser B(n) is asserted too),
and Spearman's integers exact always.

Measured on an MI355X: see the figures each test prints, and EXPERIMENTS.md."""
import ctypes as C
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import similarity_ref as ref

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "simmetrics.npz"
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 4095, 4096]
BATCHES = [1, 3, 70]
GUARD = 0x7ff4dead7ff4beef          # a NaN pattern no kernel writes


def run_rows(eng, X, Y, key="f32"):
    r = eng.similarity_rows(X, Y, key=key)
    assert r.values.dtype == torch.float64 and tuple(r.values.shape) == (len(X), 5) and r.values.is_cuda
    assert r.ints.dtype == torch.int64 and tuple(r.ints.shape) == (len(X), 4) and r.ints.is_cuda
    return r.values.cpu().numpy(), r.ints.cpu().numpy()


def assert_rows_equal(got, want, what):
    gv, gi = got
    wv, wi = want
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:5], gi[gi != wi][:5], wi[gi != wi][:5])
    same = ref.bits(gv) == ref.bits(wv)
    assert same.all(), (what, np.argwhere(~same)[:5], gv[~same][:5], wv[~same][:5])


# ---- 1: exact, integer data -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_case(D):
    """-> (X, Y fp32 [70, D], restatement of the fp32 rows, restatement of the int32 rows); computed once, shared, never modified"""
    X, Y = ref.integer_rows(max(BATCHES), D, seed=7000 + D)
    Xi, Yi = X.astype(np.int32), Y.astype(np.int32)
    return X, Y, Xi, Yi, ref.restate_rows(X, Y), ref.restate_rows(Xi, Yi)


@pytest.mark.parametrize("key", ["f32", "i32"])
@pytest.mark.parametrize("D", SIZES)
def test_integer_rows_equal_the_restatement_bit_for_bit(gpu_engine, D, key):
    X, Y, Xi, Yi, want_f, want_i = exact_case(D)
    A, Bm, want = (X, Y, want_f) if key == "f32" else (Xi, Yi, want_i)
    assert np.isnan(want[0][:, 3]).all() == (D == 1)                                     # the cases are not all degenerate
    eng = gpu_engine
    for B in BATCHES:
        assert_rows_equal(run_rows(eng, A[:B], Bm[:B], key), (want[0][:B], want[1][:B]), (D, B, key, "dense"))
    # pitches larger than D (column views of wider buffers, two different pitches), guard bands around out and ints
    B = max(BATCHES)
    dt = torch.float32 if key == "f32" else torch.int32
    wx = torch.full((B, D + 5), 9, dtype=dt, device=eng.device)
    wy = torch.full((B, D + 64), -9, dtype=dt, device=eng.device)
    wx[:, :D] = torch.as_tensor(A).to(eng.device)
    wy[:, 3:3 + D] = torch.as_tensor(Bm).to(eng.device)
    assert_rows_equal(run_rows(eng, wx[:, :D], wy[:, 3:3 + D], key), want, (D, B, key, "pitched"))
    out = torch.full(((B + 2) * 8,), GUARD, dtype=torch.int64, device=eng.device)
    ints = torch.full(((B + 2) * 4,), GUARD, dtype=torch.int64, device=eng.device)
    xv, yv = wx[:, :D], wy[:, 3:3 + D]
    with eng._lock, torch.cuda.device(eng.device):
        eng._check(eng.lib.tvc_sim_rows(eng.handle, C.c_void_p(xv.data_ptr()), C.c_void_p(yv.data_ptr()), B, D, xv.stride(0), yv.stride(0),
                                        0 if key == "f32" else 1, C.c_void_p(out[8:].data_ptr()), C.c_void_p(ints[4:].data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    o, i = out.cpu().numpy(), ints.cpu().numpy()
    assert (o[:8] == GUARD).all() and (o[-8:] == GUARD).all() and (i[:4] == GUARD).all() and (i[-4:] == GUARD).all()
    body = o[8:-8].view(np.float64).reshape(B, 8)
    assert (o[8:-8].reshape(B, 8)[:, 5:] == 0).all()                                      # columns 5 .. 7 are +0.0
    assert_rows_equal((body[:, :5], i[4:-4].reshape(B, 4)), want, (D, B, key, "raw call"))


def test_an_empty_batch_is_legal(gpu_engine):
    r = gpu_engine.similarity_rows(np.zeros((0, 17), np.float32), np.zeros((0, 17), np.float32))
    assert tuple(r.values.shape) == (0, 5) and tuple(r.ints.shape) == (0, 4)
    with pytest.raises(ValueError):
        gpu_engine.similarity_rows(np.zeros((2, 4097), np.float32), np.zeros((2, 4097), np.float32))
    with pytest.raises(ValueError):
        gpu_engine.similarity_flat(np.zeros((1 << 20) + 1, np.float32), np.zeros((1 << 20) + 1, np.float32))


# ---- 2: the long form -------------------------------------------------------------------------------------------------------
def run_flat(eng, x, y, force_long=True):
    r = eng.similarity_flat(x, y, force_long=force_long)
    assert tuple(r.values.shape) == (1, 5) and tuple(r.ints.shape) == (1, 4)
    return r.values.cpu().numpy(), r.ints.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 65, 4096])
def test_long_form_equals_row_form(gpu_engine, n):
    X, Y, _, _, want, _ = exact_case(n)
    for b in (0, 1, 2):
        rows = run_rows(gpu_engine, X[b:b + 1], Y[b:b + 1])
        assert_rows_equal(rows, (want[0][b:b + 1], want[1][b:b + 1]), (n, b, "rows"))
        assert_rows_equal(run_flat(gpu_engine, X[b], Y[b]), rows, (n, b, "long form"))
        assert_rows_equal(run_flat(gpu_engine, X[b], Y[b], force_long=False), rows, (n, b, "dispatch"))


@pytest.mark.parametrize("n", [4097, 70001])
def test_long_form_equals_the_restatement_beyond_the_row_form(gpu_engine, n):
    X, Y = ref.integer_rows(1, n, seed=n)
    assert_rows_equal(run_flat(gpu_engine, X[0], Y[0], force_long=False), ref.restate_rows(X, Y), n)


def test_long_form_at_the_cap_keeps_the_rank_sums_inside_int64(gpu_engine):
    n = ref.MAX_N
    x = np.arange(n, dtype=np.float32) - np.float32(n // 2)                 # strictly increasing, exact in fp32
    S = n * (n * n - 1) // 3                                                # the sum of (2 i - (n - 1))^2: as large as |sum cx cy| gets
    assert S < 2 ** 63 and S > 2 ** 58
    for y, sign in ((x, 1), (x[::-1].copy(), -1)):
        v, i = run_flat(gpu_engine, x, y)
        assert i[0].tolist() == [sign * S, S, S, 0], i
        assert v[0, 4] == float(sign) and abs(v[0, 3] - sign) <= ref.pearson_kernel_bound(n, 1.0, flat=True)
        assert v[0, 2] == (0.0 if sign == 1 else float(2 * sum(range(1, n, 2))))         # Manhattan: exact integers below 2^53


# ---- 3: bounds --------------------------------------------------------------------------------------------------------------
def bound_rows(n, seed):
    """-> (X, Y fp32 [6, n]): Gaussian, scaled by 1e3 / 1e-3, both scaled by 1e-3, the offset rows, the half-integer grid"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((6, n))
    h = 0.5 * g + 0.9 * rng.standard_normal((6, n))
    g[1] *= 1e3; h[1] *= 1e-3
    g[2] *= 1e-3; h[2] *= 1e-3
    ox, oy = ref.offset_rows(n, 64.0 if n <= 4096 else 1024.0, seed)
    g[3], h[3] = ox, oy
    g[4], h[4] = np.round(g[4] * 4) / 2, np.round(h[4] * 4) / 2
    g[5] = -h[5] + 1e-3 * g[5]                                              # nearly anti-correlated
    return g.astype(np.float32), h.astype(np.float32)


def check_bounds(got, X, Y, flat, what):
    """every row of got (values, ints) against the exact values; -> the worst fraction of the kernel bound per column"""
    worst = np.zeros(4)
    for b, (x, y) in enumerate(zip(X, Y)):
        n = x.size
        t = ref.truth(x, y)
        v, ints = got[0][b], got[1][b]
        assert ints.tolist() == [*ref.rank_sums(x, y), 0], (what, b)                    # Spearman's integers are exact
        assert ref.bits(v[4]) == ref.bits(ref.spearman(x, y)), (what, b)
        def rel(got, want):                           # a distance of exactly 0 (x == y) must come out as 0
            return abs(float((np.longdouble(got) - want) / want)) if want != 0 else (0.0 if got == 0 else np.inf)

        if not x.any() or not y.any():                # a zero row (the grid rows at the smallest sizes): the documented 0.0
            assert v[0] == 0.0, (what, b)
            t["cosine_similarity"] = np.longdouble(0)
        err = [abs(float(np.longdouble(v[0]) - t["cosine_similarity"])), rel(v[1], t["euclidean_distance"]), rel(v[2], t["manhattan_distance"])]
        kb = [ref.Bk(n, flat)] * 3
        ib = [ref.B(n)] * 3
        if np.isnan(t["pearson_correlation"]):
            assert np.isnan(v[3]), (what, b)
        else:
            err.append(abs(float(np.longdouble(v[3]) - t["pearson_correlation"])))
            kb.append(ref.pearson_kernel_bound(n, t["kappa"], flat))
            ib.append(ref.pearson_bound(n, t["kappa"]))
        for j, (e, k, i) in enumerate(zip(err, kb, ib)):
            assert e <= k, (what, b, ref.NAMES[j], e, k)
            assert e <= i, (what, b, ref.NAMES[j], e, i)
            worst[j] = max(worst[j], e / k)
    return worst


@pytest.mark.parametrize("D", SIZES)
def test_float_columns_within_the_kernel_bound(gpu_engine, D):
    X, Y = bound_rows(D, seed=300 + D)
    worst = check_bounds(run_rows(gpu_engine, X, Y), X, Y, False, D)
    print(f"D = {D}: worst error / kernel bound: cosine {worst[0]:.3f}, Euclidean {worst[1]:.3f}, Manhattan {worst[2]:.3f}, Pearson {worst[3]:.3f}")


def test_float_columns_within_the_kernel_bound_long_form(gpu_engine):
    n = 70001
    X, Y = bound_rows(n, seed=71)
    worst = np.zeros(4)
    for b in range(len(X)):
        got = run_flat(gpu_engine, X[b], Y[b], force_long=False)
        worst = np.maximum(worst, check_bounds(got, X[b:b + 1], Y[b:b + 1], True, (n, b)))
    print(f"n = {n}: worst error / kernel bound: cosine {worst[0]:.3f}, Euclidean {worst[1]:.3f}, Manhattan {worst[2]:.3f}, Pearson {worst[3]:.3f}")


# ---- 4: specials ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 7, 65, 300])
def test_special_rows_behave_as_documented_and_leave_the_others_alone(gpu_engine, n):
    rng = np.random.default_rng(40 + n)
    X = rng.integers(-2, 3, (12, n)).astype(np.float32) + rng.standard_normal((12, n)).astype(np.float32)
    Y = rng.standard_normal((12, n)).astype(np.float32)
    clean = run_rows(gpu_engine, X, Y)
    Xs, Ys = X.copy(), Y.copy()
    Xs[1] = 0.0                                       # a zero row
    Xs[2] = np.float32(0.1)                           # a constant row whose mean need not round to 0.1f
    Xs[4, n // 2] = np.nan
    Xs[6, 0] = np.inf
    Ys[8, n - 1] = -np.inf
    Ys[10, 1] = np.nan; Xs[10, 1] = np.nan
    planted = (1, 2, 4, 6, 8, 10)
    got = run_rows(gpu_engine, Xs, Ys)
    for b in range(12):
        if b not in planted:
            assert_rows_equal((got[0][b:b + 1], got[1][b:b + 1]), (clean[0][b:b + 1], clean[1][b:b + 1]), (n, b, "untouched"))
    v, i = got
    nan = ref.bits(ref.QNAN)
    assert v[1, 0] == 0.0 and not np.signbit(v[1, 0]) and ref.bits(v[1, 3]) == nan and ref.bits(v[1, 4]) == nan          # zero row
    assert i[1].tolist() == [0, 0, int(ref.rank_sums(Xs[1], Ys[1])[2]), 0]
    assert np.isfinite(v[2, :3]).all() and ref.bits(v[2, 3]) == nan and ref.bits(v[2, 4]) == nan and i[2, 1] == 0        # constant row
    for b, count in ((4, 1), (10, 2)):                                                                                 # NaN elements
        assert (ref.bits(v[b]) == nan).all() and i[b].tolist() == [0, 0, 0, count]
    for b in (6, 8):                                                                                                   # +-inf elements
        assert v[b, 1] == np.inf and v[b, 2] == np.inf and ref.bits(v[b, 0]) == nan and ref.bits(v[b, 3]) == nan
        assert i[b].tolist() == [*ref.rank_sums(Xs[b], Ys[b]), 0] and ref.bits(v[b, 4]) == ref.bits(ref.spearman(Xs[b], Ys[b]))
    # the planted rows as the restatement states them (its float sums differ in the last bits on this data: classes and integers)
    wv, wi = ref.restate_rows(Xs, Ys)
    assert np.array_equal(np.isnan(v), np.isnan(wv)) and np.array_equal(np.isinf(v), np.isinf(wv)) and np.array_equal(i, wi)


def test_length_one_rows_and_keys_equal_to_the_padding(gpu_engine):
    v, i = run_rows(gpu_engine, np.array([[2.0], [0.0], [-3.0]], np.float32), np.array([[5.0], [1.0], [4.0]], np.float32))
    nan = ref.bits(ref.QNAN)
    assert v[:, 0].tolist() == [1.0, 0.0, -1.0] and v[:, 1].tolist() == [3.0, 1.0, 7.0] and v[:, 2].tolist() == [3.0, 1.0, 7.0]
    assert (ref.bits(v[:, 3:]) == nan).all() and (i == 0).all()
    # int32 keys at both ends of the range: INT32_MAX has the key the sort pads with (5 and 70 elements pad to 8 and 128)
    hi, lo = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    for n in (5, 70):
        rng = np.random.default_rng(n)
        X = rng.integers(-3, 4, (4, n)).astype(np.int32)
        Y = rng.integers(-3, 4, (4, n)).astype(np.int32)
        X[0, ::2] = hi; X[1, 1::3] = lo; X[2, 0] = hi; X[2, 1] = lo; Y[3, :] = hi; Y[0, 1] = hi
        got = run_rows(gpu_engine, X, Y, key="i32")
        wv, wi = ref.restate_rows(X, Y)
        assert np.array_equal(got[1], wi), (n, got[1], wi)
        assert np.array_equal(ref.bits(got[0][:, 4]), ref.bits(wv[:, 4]))
    # fp32 rows with +-inf and -0.0: ordered as values
    x = np.array([[np.inf, -np.inf, 0.0, -0.0, 1.0, 3.4e38, -3.4e38, 1e-45, -1e-45]], np.float32)
    y = np.array([[1, 2, 3, 4, 5, 6, 7, 8, 9]], np.float32)
    got = run_rows(gpu_engine, x, y)
    assert got[1][0].tolist() == [*ref.rank_sums(x[0], y[0]), 0]


# ---- 5: top-k overlap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 70])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 128, 1000, 1024])
def test_topk_overlap_equals_python_sets(gpu_engine, k, M):
    rng = np.random.default_rng(1000 * M + k)
    for La, Lb in ((k + 13, k + 5), (max(1, k - 1), k + 20), (k, max(1, k // 2)), (max(1, k // 3), max(1, k - 7))):
        span = max(2, k)                                  # ids in [-span, span]: repeats inside a list, negative ids, shared ids
        a = rng.integers(-span, span + 1, (M, La)).astype(np.int32)
        b = rng.integers(-span, span + 1, (M, Lb)).astype(np.int32)
        a[0, : min(La, 3)] = -1                           # -1 is an id like any other
        b[0, : min(Lb, 2)] = -1
        got = gpu_engine.topk_overlap(a, b, k)
        assert got.dtype == torch.int32 and tuple(got.shape) == (M,) and got.is_cuda
        want = [ref.overlap(a[q], b[q], k) for q in range(M)]
        assert got.cpu().tolist() == want, (k, M, La, Lb)
    assert gpu_engine.topk_overlap(np.arange(5), np.arange(5)[::-1].copy(), 3).tolist() == [1]
    with pytest.raises(ValueError):
        gpu_engine.topk_overlap(a, b, 1025)


# ---- 6: determinism ---------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_run_or_the_batch(gpu_engine):
    for D in (257, 1000, 4096):
        X, Y = bound_rows(D, seed=D)
        rng = np.random.default_rng(D)
        Xb, Yb = rng.standard_normal((70, D)).astype(np.float32), rng.standard_normal((70, D)).astype(np.float32)
        Xb[37], Yb[37] = X[3], Y[3]
        one, again = run_rows(gpu_engine, X[3:4], Y[3:4]), run_rows(gpu_engine, X[3:4], Y[3:4])
        big = run_rows(gpu_engine, Xb, Yb)
        assert_rows_equal(again, one, (D, "two calls"))
        assert_rows_equal((big[0][37:38], big[1][37:38]), one, (D, "another batch"))
    x, y = bound_rows(70001, seed=9)
    assert_rows_equal(run_flat(gpu_engine, x[0], y[0]), run_flat(gpu_engine, x[0], y[0]), "long form, two calls")


# ---- 7: the public API against the reference's own outputs -------------------------------------------------------------------
def test_public_api_reproduces_the_reference_fixture(pkg, gpu_engine):
    g = np.load(GOLDEN)
    eng = gpu_engine
    calc = pkg.metrics.SimilarityCalculator
    E1, E2, X, Y = g["E1"], g["E2"], g["X"], g["Y"]
    n, D = E1.size, X.shape[1]

    def close(got, want, n, what):
        for name, gv, wv in zip(ref.NAMES, got, want):
            tol = 2 * ref.B(n) * (1.0 if name.endswith("correlation") or name == "cosine_similarity" else abs(wv))
            assert isinstance(gv, float) and abs(gv - wv) <= tol, (what, name, gv, wv)

    m = calc.compute_all_similarities(E1, E2, engine=eng)
    assert isinstance(m, pkg.metrics.SimilarityMetrics) and list(m.to_dict()) == list(ref.NAMES)
    close(list(m.to_dict().values()), g["flat"], n, "compute_all_similarities")
    close(list(calc.compute_all_similarities(torch.as_tensor(E1), torch.as_tensor(E2), engine=eng).to_dict().values()), g["flat"], n, "tensors")
    single = [calc.cosine_similarity(X[3], Y[3], engine=eng), calc.euclidean_distance(X[3], Y[3], engine=eng),
              calc.manhattan_distance(X[3], Y[3], engine=eng), calc.pearson_correlation(X[3], Y[3], engine=eng),
              calc.spearman_correlation(X[3], Y[3], engine=eng)]
    assert abs(single[0] - g["rows"][3, 0]) < 1e-6                            # the existing fp32 cosine path, unchanged
    close(single[1:], g["rows"][3, 1:], D, "scalar functions")
    rows = calc.rowwise_similarities(X, Y, engine=eng)
    assert list(rows) == list(ref.NAMES) and all(v.shape == (24,) and v.dtype == np.float64 for v in rows.values())
    for b in range(24):
        close([float(rows[name][b]) for name in ref.NAMES], g["rows"][b], D, ("rowwise_similarities", b))
    assert rows["pearson_correlation"][5] == 0.0 and rows["spearman_correlation"][5] == 0.0 and rows["cosine_similarity"][7] == 0.0
    mc = pkg.metrics.MetricsCalculator(engine=eng)
    sim = mc.calculate_similarity_metrics(E1, E2)
    assert list(sim) == list(ref.NAMES)
    close(list(sim.values()), g["flat"], n, "calculate_similarity_metrics")
    det = np.load(GOLDEN.parent / "detection_eval.npz")
    both = mc.calculate_all_metrics(det["scores"], det["labels"], E1, E2)
    assert list(both) == ["detection", "similarity"] and both["similarity"] == sim
    assert list(both["detection"]) == ["auc", "accuracy", "precision", "recall", "f1_score", "fpr_at_95_tpr", "threshold", "confusion_matrix"]
    assert abs(both["detection"]["auc"] - float(det["auc"])) < 1e-12
    assert list(mc.calculate_all_metrics(det["scores"], det["labels"])) == ["detection"]

    cc = pkg.retrieval.ConsistencyCalculator(engine=eng)
    idx1, idx2, s1, s2, ks = g["idx1"], g["idx2"], g["s1"], g["s2"], g["ks"].tolist()
    L = idx1.shape[1]
    for q in range(len(idx1)):
        d = cc.compute_similarity_distribution(s1[q].astype(np.float64))
        assert list(d) == ["mean", "std", "min", "max", "median"] and np.allclose(list(d.values()), g["dist"][q], rtol=1e-15, atol=0)
        score, rank = cc.compute_consistency_score(s1[q], s2[q]), cc.compute_rank_correlation(idx1[q], idx2[q])
        assert isinstance(score, float) and abs(score - g["score"][q]) <= 2 * ref.B(L)
        assert isinstance(rank, float) and abs(rank - g["rank"][q]) <= 2.0 ** -50
        for j, k in enumerate(ks):
            t = cc.compute_top_k_consistency(idx1[q], idx2[q], k)
            assert isinstance(t, float) and t == g["topk"][q, j], (q, k)
    for j, k in enumerate(ks):
        assert np.array_equal(cc.batch_top_k_consistency(idx1, idx2, k), g["topk"][:, j])
    assert np.abs(cc.batch_rank_correlation(idx1, idx2) - g["rank"]).max() <= 2.0 ** -50
    assert np.abs(cc.batch_consistency_score(s1, s2) - g["score"]).max() <= 2 * ref.B(L)
    assert cc.compute_rank_correlation([4, 4, 4], [1, 2, 3]) == 0.0 and cc.compute_consistency_score([1.0], [2.0]) == 0.0
