"""GPU: the retrieval-evaluation kernels (tvc_rank_targets / tvc_rank_count / tvc_rank_metrics), ``TVCEngine.retrieval_ranks``,
``RetrievalEvaluator.evaluate_retrieval`` and ``MultiModalRetriever.evaluate_retrieval`` against the restatement of
tests/retrieval_ref.py (pinned to the reference's own outputs by tests/test_retrieval_ref.py).

Bounds.  Integer rows in [-2, 2] at D = 64: every product and every partial sum is an integer below 2^24, exact in bf16 and
fp32, so positions, rows, offsets and hits must equal the restatement and ties are everywhere.  Gaussian unit rows: tau =
1e-6 |q||x|, the project's similarity bound for these split-bf16 products (tests/test_gpu_ivf.py, tests/test_gpu_api.py); a
position lies between the count of the rows above the target by more than tau and the count of those not below it by more
than tau, in fp64 over the stored operands.  Per-query fp64 terms: 1e-12, the room of a differently ordered sum of at most
200 terms of size <= 1."""
import ctypes as C
import functools
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import retrieval_ref as R

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"
BANK = "retrieval-eval-test"
KS = (1, 5, 10, 50)

EXACT_M = [1, 37, 256, 300]
EXACT_R = [1, 255, 256, 257, 1000]
LAYOUTS = ["one-label", "lowest", "last-tile"]


def operands(X: torch.Tensor) -> np.ndarray:
    """fp64 values of rows as the kernels see them: the bf16 values, or hi + lo of the fp32 rows' bf16 planes."""
    if X.dtype == torch.bfloat16:
        return X.double().numpy()
    hi = X.bfloat16().float()
    lo = (X - hi).bfloat16().float()
    return hi.double().numpy() + lo.double().numpy()


class Slot:
    """Registers rows under the test's bank name for the duration of a ``with``."""

    def __init__(self, eng, X):
        self.eng, self.X = eng, X

    def __enter__(self):
        self.eng.set_bank(self.X.to(self.eng.device), name=BANK)
        return self.eng

    def __exit__(self, *exc):
        self.eng.release_bank(BANK)


@functools.lru_cache(maxsize=None)
def exact_case(M, R_, layout="mixed"):
    """Integer rows and labels -> (q fp32 [M, 64], x fp32 [R, 64], qlabel, glabel, the restatement's (off, rows, pos) and
    per-query terms); computed once, shared, never modified.  The mixed layout has negative query labels, negative gallery
    labels, a query label (6) on no gallery row, and -- whenever R is not a multiple of 256 -- a target in the last, partial
    bank tile (row R - 1 carries query 0's label)."""
    rng = np.random.default_rng(100 * M + R_ + len(layout))
    q = rng.integers(-2, 3, (M, 64)).astype(np.float32)
    x = rng.integers(-2, 3, (R_, 64)).astype(np.float32)
    gl = rng.integers(0, 6, R_)
    gl[rng.random(R_) < 0.1] = -1 - rng.integers(0, 3)
    ql = rng.integers(0, 7, M)                                   # 6: absent from the gallery
    ql[rng.random(M) < 0.1] = -1
    ql[0] = 2
    gl[R_ - 1] = 2
    if layout == "one-label":                                    # one label on every bank row: no irrelevant row at all
        gl[:] = 4
        ql[0] = 4
    elif layout == "lowest":                                     # query 0's targets score -256, the minimum: every other element
        q[0] = 2.0                                               # of query 0 is at or above its last target (the slow path)
        gl[gl == 2] = 3
        low = rng.choice(R_, max(1, R_ // 50), replace=False)
        gl[low] = 2
        x[low] = -2.0
    elif layout == "last-tile":                                  # every target of query 0 in the last, partial bank tile
        assert R_ % 256
        gl[gl == 2] = 3
        gl[R_ - R_ % 256:] = 2
    S = q.astype(np.float64) @ x.astype(np.float64).T
    off, rows, pos = R.positions(S, ql, gl)
    return q, x, ql, gl, S, (off, rows, pos), R.per_query(off, pos, KS)


def run_exact(eng, case, bf16):
    q, x, ql, gl, S, (off, rows, pos), (ap, rr, hits, dcg, idcg) = case
    X = torch.from_numpy(x)
    with Slot(eng, X.bfloat16() if bf16 else X):
        r = eng.retrieval_ranks(torch.from_numpy(q).to(eng.device), ql, gl, bank=BANK, k_values=KS)
    assert r.tgt_off.dtype == torch.int64 and r.tgt_row.dtype == torch.int32 and r.pos.dtype == torch.int32
    assert np.array_equal(r.tgt_off.cpu().numpy(), off)
    assert np.array_equal(r.tgt_row.cpu().numpy(), rows)
    assert np.array_equal(r.pos.cpu().numpy(), pos)
    assert np.array_equal(r.tgt_sim.cpu().numpy().astype(np.float64), S[np.repeat(np.arange(len(off) - 1), np.diff(off)), rows])
    assert np.array_equal(r.hits.cpu().numpy(), hits)
    for got, want in ((r.ap, ap), (r.rr, rr), (r.dcg, dcg), (r.idcg, idcg)):
        assert np.abs(got.cpu().numpy() - want).max(initial=0.0) <= 1e-12
    return r


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("R_", EXACT_R)
@pytest.mark.parametrize("M", EXACT_M)
def test_exact_positions_with_ties(gpu_engine, M, R_, bf16):
    case = exact_case(M, R_)
    r = run_exact(gpu_engine, case, bf16)
    ql, gl = case[2], case[3]
    assert (ql < 0).any() or M == 1
    assert int(r.n_targets[0]) >= 1                              # row R - 1 is a target of query 0


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,R_", [(37, 257), (300, 1000)])
def test_exact_positions_label_layouts(gpu_engine, M, R_, layout, bf16):
    case = exact_case(M, R_, layout)
    r = run_exact(gpu_engine, case, bf16)
    off, pos = r.tgt_off.cpu().numpy(), r.pos.cpu().numpy()
    if layout == "one-label":
        assert int(r.hist.sum()) == 0
        for i in np.flatnonzero(np.diff(off)):
            assert np.array_equal(pos[off[i]:off[i + 1]], np.arange(R_))
    elif layout == "lowest":
        P0 = off[1]
        assert np.array_equal(pos[:P0], np.arange(R_ - P0, R_))  # behind every irrelevant row
        assert int(r.hist[:P0].sum()) == R_ - P0                 # each of which counted once
    else:
        assert (r.tgt_row[:off[1]].cpu().numpy() >= R_ - R_ % 256).all() and off[1] == R_ % 256


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,R_", [(37, 1000), (300, 257)])
def test_positions_agree_with_the_bank_search(gpu_engine, M, R_, bf16):
    """Every target among the top 10 of tvc_bank_search sits at its index in that list: one order for both."""
    q, x, ql, gl, S, _, _ = exact_case(M, R_)
    X = torch.from_numpy(x)
    with Slot(gpu_engine, X.bfloat16() if bf16 else X) as eng:
        qd = torch.from_numpy(q).to(eng.device)
        r = eng.retrieval_ranks(qd, ql, gl, bank=BANK, k_values=KS)
        idx, _, _ = eng.bank_search_robust(qd, 10, want_moments=False, bank=BANK)
    idx, off, rows, pos = idx.cpu().numpy(), r.tgt_off.cpu().numpy(), r.tgt_row.cpu().numpy(), r.pos.cpu().numpy()
    seen = 0
    for i in range(M):
        where = {int(j): n for n, j in enumerate(idx[i])}
        for j, p in zip(rows[off[i]:off[i + 1]], pos[off[i]:off[i + 1]]):
            if int(j) in where:
                assert where[int(j)] == p
                seen += 1
            else:
                assert p >= 10
    assert seen > M // 2


@functools.lru_cache(maxsize=None)
def gauss_case(M, R_, D, bf16):
    rng = np.random.default_rng(M + R_ + D)
    q = rng.standard_normal((M, D))
    x = rng.standard_normal((R_, D))
    q, x = q / np.linalg.norm(q, axis=1, keepdims=True), x / np.linalg.norm(x, axis=1, keepdims=True)
    Q = torch.from_numpy(q.astype(np.float32))
    X = torch.from_numpy(x.astype(np.float32))
    if bf16:
        X = X.bfloat16()
    q64, x64 = operands(Q), operands(X)
    return Q, X, rng.integers(0, 50, M), rng.integers(-5, 50, R_), q64 @ x64.T, np.linalg.norm(q64, axis=1), np.linalg.norm(x64, axis=1)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,R_,D,max_share", [(64, 1000, 128, 0.01), (300, 4099, 192, 0.05)])
def test_positions_against_fp64(gpu_engine, M, R_, D, max_share, bf16):
    Q, X, ql, gl, S64, qn, xn = gauss_case(M, R_, D, bf16)
    with Slot(gpu_engine, X) as eng:
        r = eng.retrieval_ranks(Q.to(eng.device), ql, gl, bank=BANK, k_values=KS)
    off, rows, pos = r.tgt_off.cpu().numpy(), r.tgt_row.cpu().numpy(), r.pos.cpu().numpy()
    want_off, want_rows, _ = R.positions(S64, ql, gl)
    assert np.array_equal(off, want_off) and off[-1] > M
    open_ends = bad = 0
    for i in range(M):
        mine = rows[off[i]:off[i + 1]]
        assert np.array_equal(np.sort(mine), np.sort(want_rows[off[i]:off[i + 1]]))
        tau = 1e-6 * qn[i] * xn
        for j, p in zip(mine, pos[off[i]:off[i + 1]]):
            above = S64[i] > S64[i, j] + tau
            not_below = S64[i] >= S64[i, j] - tau
            above[j] = not_below[j] = False
            lo, hi = int(above.sum()), int(not_below.sum())
            open_ends += lo != hi
            bad += not lo <= p <= hi
    share = open_ends / off[-1]
    print(f"fp64 M={M} R={R_} D={D} {'bf16' if bf16 else 'f32'}: {off[-1]} targets, {bad} outside their bounds, "
          f"bounds differing for {share:.4%}")
    assert bad == 0
    assert share <= max_share
    sims = r.tgt_sim.cpu().numpy().astype(np.float64)
    qi = np.repeat(np.arange(M), np.diff(off))
    assert (np.abs(sims - S64[qi, rows]) <= 1e-6 * qn[qi] * xn[rows]).all()


def test_metrics_kernel_alone(gpu_engine):
    """Handmade lists: P from 0 to 200 per query, around the 64-lane chunk; the kernel's fp64 terms against the restatement."""
    rng = np.random.default_rng(3)
    sizes = np.array([0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 0, 0, 199] + list(rng.integers(0, 201, 30)))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    hist = rng.integers(0, 40, off[-1]).astype(np.int32)
    hist[rng.random(off[-1]) < 0.5] = 0
    ks = (1, 2, 5, 10, 64, 100, 1000, 100000)
    pos = np.concatenate([np.arange(n) + np.cumsum(hist[a:a + n]) for a, n in zip(off[:-1], sizes)]).astype(np.int64)
    ap, rr, hits, dcg, idcg = R.per_query(off, pos, ks)
    with Slot(gpu_engine, torch.zeros(1, 64)) as eng:
        got = eng.rank_metrics(torch.from_numpy(off).to(eng.device), torch.from_numpy(hist).to(eng.device), ks, bank=BANK)
    gpos, gap, grr, ghits, gdcg, gidcg = (t.cpu().numpy() for t in got)
    assert np.array_equal(gpos, pos) and np.array_equal(ghits, hits)
    for a, b in ((gap, ap), (grr, rr), (gdcg, dcg), (gidcg, idcg)):
        assert a.dtype == np.float64 and np.abs(a - b).max() <= 1e-12
    assert not gap[sizes == 0].any() and not gidcg[sizes == 0].any()


@pytest.fixture(scope="module")
def fx():
    z = np.load(G / "retrieval_eval.npz")
    d = {k: z[k] for k in z.files}
    d["ks"] = [int(k) for k in d["k_values"]]
    d["want"] = np.concatenate([d["recall_at_k"], d["precision_at_k"], d["ndcg_at_k"], [d["map_score"], d["mrr"]]])
    return d


def test_fixture_end_to_end(pkg, gpu_engine, fx):
    """The reference's own numbers from ``evaluate_retrieval`` on the fixture's raw rows (D = 96: padded; random norms:
    normalised), with the reference matrix's positions."""
    args = (fx["queries"], fx["gallery"], fx["qlabel"], fx["glabel"])
    m = pkg.RetrievalEvaluator.evaluate_retrieval(*args, k_values=fx["ks"], engine=gpu_engine)
    assert np.abs(R.flatten(m, fx["ks"]) - fx["want"]).max() <= 1e-12
    ranks = pkg.RetrievalEvaluator.rank_embeddings(*args, k_values=fx["ks"], engine=gpu_engine)
    off, rows, pos = R.positions(fx["cosine"], fx["qlabel"], fx["glabel"])
    assert np.array_equal(ranks.tgt_off.cpu().numpy(), off)
    assert np.array_equal(ranks.tgt_row.cpu().numpy(), rows) and np.array_equal(ranks.pos.cpu().numpy(), pos)
    assert not gpu_engine.has_bank(BANK) and not [n for n in gpu_engine._banks if n.startswith("retrieval-eval:")]
    few = pkg.MetricsCalculator(engine=gpu_engine).calculate_retrieval_metrics(*args)
    assert list(few.recall_at_k) == [1, 5, 10]
    assert np.abs(R.flatten(few, [1, 5, 10]) - R.flatten(m, [1, 5, 10])).max() <= 1e-12
    skipped = pkg.RetrievalEvaluator.evaluate_retrieval(*args, k_values=fx["ks"], engine=gpu_engine, skip_empty_queries=True)
    want = R.flatten(R.from_labels(fx["cosine"], fx["qlabel"], fx["glabel"], fx["ks"], skip_empty=True), fx["ks"])
    assert np.abs(R.flatten(skipped, fx["ks"]) - want).max() <= 1e-12
    assert skipped.map_score > m.map_score


def test_two_runs_are_bit_identical(gpu_engine):
    Q, X, ql, gl, *_ = gauss_case(64, 1000, 128, False)
    with Slot(gpu_engine, X) as eng:
        a = eng.retrieval_ranks(Q.to(eng.device), ql, gl, bank=BANK, k_values=KS)
        b = eng.retrieval_ranks(Q.to(eng.device), ql, gl, bank=BANK, k_values=KS)
    for name in ("tgt_off", "tgt_row", "tgt_sim", "pos", "hist", "ap", "rr", "hits", "dcg", "idcg"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_non_finite_target_score_raises(gpu_engine):
    q, x, ql, gl, *_ = exact_case(37, 257)
    x = x.copy()
    x[256, 0] = np.inf                                           # row R - 1 is a target of query 0
    with Slot(gpu_engine, torch.from_numpy(x)) as eng:
        with pytest.raises(ValueError, match="non-finite"):
            eng.retrieval_ranks(torch.from_numpy(q).to(eng.device), ql, gl, bank=BANK)


def test_refusals_launch_nothing(pkg, gpu_engine):
    eng, lib = gpu_engine, gpu_engine.lib
    q, x, ql, gl, *_ = exact_case(37, 257)
    dev = eng.device
    qd = torch.from_numpy(q).to(dev)
    qlabel, glabel, gpos, off = eng.rank_layout(ql, gl)
    T = int(off[-1])
    sim, row = torch.full((T,), -7.0, device=dev), torch.full((T,), -7, dtype=torch.int32, device=dev)
    hist, pos = torch.full((T,), -7, dtype=torch.int32, device=dev), torch.full((T,), -7, dtype=torch.int32, device=dev)
    f64 = [torch.full((37 * 8,), -7.0, dtype=torch.float64, device=dev) for _ in range(4)]
    hits = torch.full((37 * 8,), -7, dtype=torch.int32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    null, st = C.c_void_p(0), C.c_void_p(0)
    ks = lambda *v: (C.c_int32 * len(v))(*v)    # noqa: E731

    def targets(M=37, rows=P(qd), tgt=P(sim)):
        return lib.tvc_rank_targets(eng.handle, rows, M, P(qlabel), P(glabel), P(gpos), P(off), T, tgt, P(row), st)

    def count(M=37, h=P(hist)):
        return lib.tvc_rank_count(eng.handle, P(qd), M, P(qlabel), P(glabel), P(off), P(sim), P(row), T, h, st)

    def metrics(M=37, k=ks(1, 5), n_k=2, ap=P(f64[0])):
        return lib.tvc_rank_metrics(eng.handle, M, P(off), P(hist), T, k, n_k, P(pos), ap, P(f64[1]), P(hits), P(f64[2]), P(f64[3]), st)
    with eng._lock, torch.cuda.device(dev):
        eng._select(BANK, create=True)           # a slot without rows
        try:
            assert targets() == count() == metrics() == pkg._lib.TVC_E_STATE
        finally:
            del eng._banks[BANK]
    with Slot(eng, torch.from_numpy(x)):
        before = eng.workspace_bytes()
        with eng._lock, torch.cuda.device(dev):
            eng._select(BANK)
            bad = pkg._lib.TVC_E_INVALID
            assert targets(M=0) == targets(rows=null) == targets(tgt=null) == bad
            assert count(M=0) == count(h=null) == bad
            assert metrics(M=0) == metrics(ap=null) == bad
            assert metrics(k=ks(1, 2, 3, 4, 5, 6, 7, 8, 9), n_k=9) == metrics(k=ks(1, 0), n_k=2) == metrics(k=ks(-3), n_k=1) == bad
            torch.cuda.synchronize()
        assert eng.workspace_bytes() == before
        for t in [sim, row, hist, pos, hits] + f64:
            assert bool((t == -7).all())
        # T == 0 is legal: no label in common
        r = eng.retrieval_ranks(qd, np.full(37, 9), gl, bank=BANK, k_values=KS)
        assert r.tgt_row.numel() == 0 and int(r.tgt_off[-1]) == 0
        assert not r.ap.any() and not r.rr.any() and not r.hits.any() and not r.dcg.any() and not r.idcg.any()


def test_retriever_evaluates_its_own_slot(pkg, gpu_engine):
    Q, X, ql, gl, *_ = gauss_case(64, 1000, 128, False)
    model = types.SimpleNamespace(engine=gpu_engine, device=gpu_engine.device)
    ret = pkg.MultiModalRetriever(pkg.RetrievalConfig(bank_dtype="float32"), clip_model=model)
    ret.set_image_features(X)
    try:
        got = ret.evaluate_retrieval(Q, ql, gl, k_values=KS)
        mine = ret.rank_queries(Q, ql, gl, k_values=KS)
    finally:
        gpu_engine.release_bank(ret.bank_name)
    with Slot(gpu_engine, X) as eng:
        r = eng.retrieval_ranks(Q.to(eng.device), ql, gl, bank=BANK, k_values=KS)
    assert torch.equal(mine.pos, r.pos) and torch.equal(mine.tgt_row, r.tgt_row) and torch.equal(mine.ap, r.ap)
    want = pkg.RetrievalEvaluator.from_ranks(r)
    assert np.array_equal(R.flatten(got, KS), R.flatten(want, KS))
    assert got.map_score > 0
