"""GPU: the closest-pair kernels (tvc_closest_pair: ``TVCEngine.closest_pair``) and ``ReferenceBank``'s similarity eviction
against the fp64 restatement of tests/nearest_ref.py (pinned to a literal double loop by tests/test_nearest_ref.py).

The contract.  With c64 the fp64 cosine of the STORED rows (the bf16 values; hi + lo of an fp32 slot's planes) and tau = 1e-6:
|sim[i] - c64(i, partner[i])| <= tau and c64(i, partner[i]) >= max_{j > i} c64(i, j) - 2 tau, the same for pair / pair_sim over
all i < j; where the arithmetic is exact (rows of norm 4 with dot products k, every cosine k / 16) every output equals the
restatement bit for bit, ties included.

Measured on an MI355X: see the figures each test prints, and EXPERIMENTS.md."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import nearest_ref

pytestmark = pytest.mark.gpu
BANK = "nearest-test"
TAU = nearest_ref.TAU
GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_bank_similarity.npz"


def operands(X: torch.Tensor) -> np.ndarray:
    """fp64 values of the rows as the kernels see them: the bf16 values, or hi + lo of the fp32 rows' bf16 planes."""
    if X.dtype == torch.bfloat16:
        return X.double().numpy()
    hi = X.bfloat16().float()
    lo = (X - hi).bfloat16().float()
    return hi.double().numpy() + lo.double().numpy()


def run(eng, X, name=BANK):
    """registers X, one call -> (pair tuple, pair_sim fp32 scalar, partner int32 [R], sim fp32 [R]) as numpy"""
    eng.set_bank(X.to(eng.device), name=name)
    try:
        pair, pair_sim, partner, sim = eng.closest_pair(bank=name)
        R = X.shape[0]
        assert pair.dtype == torch.int32 and tuple(pair.shape) == (2,) and pair_sim.dtype == torch.float32 and tuple(pair_sim.shape) == (1,)
        assert partner.dtype == torch.int32 and tuple(partner.shape) == (R,) and sim.dtype == torch.float32 and tuple(sim.shape) == (R,)
        assert all(t.is_cuda for t in (pair, pair_sim, partner, sim))
        return tuple(pair.tolist()), pair_sim.cpu().numpy()[0], partner.cpu().numpy(), sim.cpu().numpy()
    finally:
        eng.release_bank(name)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1: exact, integer data -------------------------------------------------------------------------------------------------
EXACT_R = [1, 2, 3, 255, 256, 257, 511, 513, 700]
EXACT_D = [64, 192]


def moved(row: np.ndarray) -> np.ndarray:
    """the row with one of its non-zeros moved to a zero column: still 16 non-zeros, dot product 15 with the original"""
    out = row.copy()
    nz, z = np.flatnonzero(row)[0], np.flatnonzero(row == 0)[0]
    out[z], out[nz] = row[nz], 0.0
    return out


@functools.lru_cache(maxsize=None)
def exact_case(R, D):
    """-> (X fp32 [R, D], planted pairs, restatement outputs); computed once, shared, never modified.  Entries in {-1, 0, 1}
    with exactly 16 non-zeros: norm 4, every cosine k / 16.  Planted, where R has room:
      (5, 70, 130)   a triple of equal rows: row 5 takes 70 (the lowest j), row 70 takes 130, and the PAIR is (5, 70): the lowest i
      (10, 40)       inside the diagonal tile, on both sides of j > i: row 10 takes 40; row 40's duplicate sits at j < i only
      (255, 256)     across a tile edge
      (520, 600)     inside the ragged last diagonal tile of R = 700
      (R - 2, R - 1) equal; row 0 = row R - 1 with one non-zero moved: cosine 15 / 16 with both, first tile against last, and
                     the tie between R - 2 and R - 1 goes to R - 2"""
    X = nearest_ref.integer_rows(R, D, seed=1000 * D + R)
    want = {}
    if R >= 2:
        X[R - 2] = X[R - 1]
        want[R - 2] = (R - 1, 1.0)
    if R >= 131:
        X[70] = X[5]; X[130] = X[5]
        want[5], want[70] = (70, 1.0), (130, 1.0)
        X[40] = X[10]
        want[10] = (40, 1.0)
    if R >= 257:
        X[256] = X[255]
        want[255] = (256, 1.0)
    if R >= 601:
        X[600] = X[520]
        want[520] = (600, 1.0)
    if R >= 3:
        X[0] = moved(X[R - 1])
        want[0] = (R - 2, 15.0 / 16.0)
    C = nearest_ref.cosine64(X.astype(np.float64))
    partner, sim = nearest_ref.later_nearest(C)
    pair, ps = nearest_ref.closest_pair(partner, sim)
    for i, (j, c) in want.items():                                      # the plants are what the restatement finds
        assert partner[i] == j and sim[i] == c, (R, D, i, partner[i], sim[i])
    if R >= 131:
        assert pair == (5, 70) and partner[40] != 10 and partner[130] not in (5, 70)
    X.setflags(write=False)
    return X, partner, sim, pair, ps


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", EXACT_D)
@pytest.mark.parametrize("R", EXACT_R)
def test_exact_on_integer_rows(gpu_engine, R, D, bf16):
    X, partner, sim, pair, ps = exact_case(R, D)
    Xt = torch.from_numpy(np.array(X))
    g_pair, g_ps, g_partner, g_sim = run(gpu_engine, Xt.bfloat16() if bf16 else Xt)
    assert np.array_equal(g_partner, partner)
    assert np.array_equal(bits(g_sim), bits(sim))
    assert g_pair == pair and bits(g_ps) == bits(ps)
    if R == 1:
        assert g_pair == (-1, -1) and g_ps == -np.inf and g_partner[0] == -1 and g_sim[0] == -np.inf


# ---- 2: Gaussian rows against fp64 ------------------------------------------------------------------------------------------
CAP = 0.01


@functools.lru_cache(maxsize=None)
def gauss_case(R, D, bf16):
    X = torch.from_numpy(nearest_ref.scaled_gaussian(R, D, seed=R + D))
    if bf16:
        X = X.bfloat16()
    C = nearest_ref.cosine64(operands(X))
    partner, sim = nearest_ref.later_nearest(C)
    U = np.where(np.triu(np.ones((R, R), bool), 1), C, -np.inf)
    top2 = np.sort(U, axis=1)[:, -2:]
    close = float(np.mean(top2[:-2, 1] - top2[:-2, 0] <= 2 * TAU))     # rows with at least two later rows
    return X, C, U, partner, sim, close


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("R,D", [(700, 128), (513, 192)])
def test_gaussian_rows_against_fp64(gpu_engine, R, D, bf16):
    X, C, U, partner, sim, close = gauss_case(R, D, bf16)
    # the data leaves the cap room: few rows have their two best partners within 2 tau of each other
    assert close < CAP, close
    g_pair, g_ps, g_partner, g_sim = run(gpu_engine, X)
    assert g_partner[R - 1] == -1 and g_sim[R - 1] == -np.inf
    rows = np.arange(R - 1)
    p = g_partner[:-1]
    assert np.all(p > rows) and np.all(p < R)
    got = C[rows, p]
    err = np.abs(g_sim[:-1].astype(np.float64) - got)
    short = U[:-1].max(1) - got
    differ = float(np.mean(p != partner[:-1]))
    i, j = g_pair
    best = U.max()
    pair_err, pair_short = abs(float(g_ps) - C[i, j]) if 0 <= i < j < R else np.inf, best - C[i, j] if 0 <= i < j < R else np.inf
    print(f"closest pair R={R} D={D} {'bf16' if bf16 else 'f32'}: max |sim - c64| {err.max():.3e} = {err.max() / TAU:.2f} tau, worst shortfall "
          f"{short.max():.3e}, partners differing from fp64's arg-max {differ:.4f} (rows with top two within 2 tau: {close:.4f}), "
          f"pair {g_pair} |pair_sim - c64| {pair_err:.3e}, pair shortfall {pair_short:.3e}")
    assert err.max() <= TAU
    assert short.max() <= 2 * TAU
    assert differ <= CAP
    assert 0 <= i < j < R and g_partner[i] == j and bits(g_ps) == bits(g_sim[i])
    assert pair_err <= TAU and pair_short <= 2 * TAU


# ---- 3: special rows on an fp32 slot ----------------------------------------------------------------------------------------
def test_special_rows_on_an_fp32_slot(gpu_engine):
    R, D = 300, 128
    X = nearest_ref.scaled_gaussian(R, D, seed=77)
    ZERO, INF, NAN, LAST = 7, 50, 120, R - 1
    X[ZERO] = 0.0
    X[INF, 3] = np.inf
    X[NAN, 100] = np.nan
    X[LAST, 0] = np.nan                                                  # row R - 2 is left with no admissible later row
    bad = [INF, NAN, LAST]
    g_pair, g_ps, g_partner, g_sim = run(gpu_engine, torch.from_numpy(X))
    assert g_partner[ZERO] == ZERO + 1 and g_sim[ZERO] == 0.0            # cosine 0 with every row: the first later row
    for b in bad:
        assert g_partner[b] == -1 and g_sim[b] == -np.inf
    assert g_partner[R - 2] == -1 and g_sim[R - 2] == -np.inf
    assert not np.isin(g_partner, bad).any() and g_pair[0] not in bad and g_pair[1] not in bad
    assert np.all(np.isfinite(g_sim[g_partner >= 0]))
    # a zero row as a partner scores 0: the restatement on the operands agrees on every row within the contract
    C = nearest_ref.cosine64(operands(torch.from_numpy(X)))
    partner, sim = nearest_ref.later_nearest(C)
    assert np.array_equal(g_partner < 0, partner < 0)
    has = g_partner >= 0
    got = C[has.nonzero()[0], g_partner[has]]
    assert np.abs(g_sim[has] - got).max() <= TAU and (sim[has] - got).max() <= 2 * TAU
    # the rest of the slot is unaffected: the same slot with the three rows deleted, indices remapped, gives the same bits
    keep = np.array([r for r in range(R) if r not in bad])
    new_of = np.full(R, -1, np.int64)
    new_of[keep] = np.arange(len(keep))
    k_pair, k_ps, k_partner, k_sim = run(gpu_engine, torch.from_numpy(X[keep]))
    remapped = np.where(g_partner[keep] >= 0, new_of[np.maximum(g_partner[keep], 0)], -1)
    assert np.array_equal(remapped, k_partner)
    assert np.array_equal(bits(g_sim[keep]), bits(k_sim))
    assert (int(new_of[g_pair[0]]), int(new_of[g_pair[1]])) == k_pair and bits(g_ps) == bits(k_ps)


# ---- 4: determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_outputs_are_bit_identical_between_runs_and_slots(gpu_engine, bf16):
    X = gauss_case(700, 128, bf16)[0]
    a = run(gpu_engine, X)
    b = run(gpu_engine, X)
    # another slot name while a first slot stays registered: another slot of the handle, other device blocks
    gpu_engine.set_bank(X.to(gpu_engine.device), name=BANK + "-held")
    try:
        c = run(gpu_engine, X.clone(), name=BANK + "-other")
    finally:
        gpu_engine.release_bank(BANK + "-held")
    for o in (b, c):
        assert o[0] == a[0] and bits(o[1]) == bits(a[1]) and np.array_equal(o[2], a[2]) and np.array_equal(bits(o[3]), bits(a[3]))


# ---- 5: ReferenceBank -------------------------------------------------------------------------------------------------------
def replay_bank(pkg, eng, fx, strategy):
    """the recorded run through a ReferenceBank on the engine -> (removed index per step or -1, admitted, final ids)"""
    X, Q, steps = fx["vectors"], fx["queries"], fx["query_steps"].tolist()
    bank = pkg.ReferenceBank(pkg.ReferenceBankConfig(max_size=int(fx["max_size"]), similarity_threshold=float(fx["admit_t"]),
                                                     update_strategy=strategy, clustering_method="none", persistence_enabled=False,
                                                     auto_clustering=False, feature_dim=X.shape[1]), engine=eng)
    removed = np.full(len(X), -1, np.int64)
    admitted = np.zeros(len(X), bool)
    for s in range(len(X)):
        before = [r.metadata["id"] for r in bank.references]
        admitted[s] = bank.add_reference(X[s].astype(np.float64), {"id": s})
        after = [r.metadata["id"] for r in bank.references]
        gone = [k for k, i in enumerate(before) if i not in after]
        assert len(gone) <= 1 and len(after) <= int(fx["max_size"])
        if gone:
            removed[s] = gone[0]
        if s in steps:
            bank.query_similar(Q[steps.index(s)].astype(np.float64), top_k=int(fx["top_k"]), similarity_threshold=float(fx["query_t"]))
    ids = [r.metadata["id"] for r in bank.references]
    stats = bank.get_statistics()
    del bank
    return removed, admitted, ids, stats


def test_reference_bank_similarity_eviction_replays_the_reference(pkg, gpu_engine):
    """Fails on a bank whose "similarity" strategy falls back to FIFO: the recorded removals are the reference's own."""
    fx = np.load(GOLDEN)
    removed, admitted, ids, stats = replay_bank(pkg, gpu_engine, fx, "similarity")
    assert np.array_equal(admitted, fx["admitted"])
    assert np.array_equal(removed, fx["removed"])
    assert ids == fx["final_ids"].tolist()
    assert stats["total_removed"] == int((fx["removed"] >= 0).sum()) and stats["size"] == int(fx["max_size"])


def test_reference_bank_fifo_still_removes_in_fifo_order(pkg, gpu_engine):
    fx = np.load(GOLDEN)
    removed, admitted, ids, _ = replay_bank(pkg, gpu_engine, fx, "fifo")
    full = np.cumsum(admitted) > int(fx["max_size"])                     # the adds that found the bank full
    assert np.all(removed[full & admitted] == 0) and np.all(removed[~(full & admitted)] == -1)
    assert ids == np.flatnonzero(admitted)[-int(fx["max_size"]):].tolist()
