"""CPU: tests/nearest_ref.py (the fp64 restatement of the closest-pair kernels and of the similarity-eviction victim rule) against
a literal double loop in the reference's own order (src/ref_bank.py:401-427), the recorded reference run of
tests/golden/ref_bank_similarity.npz replayed through the restatement, and ``ref_bank.similarity_victim`` as a pure function."""
import math
from pathlib import Path

import numpy as np
import pytest

import nearest_ref

GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_bank_similarity.npz"


def loop_cosine(a, b):
    """src/ref_bank.py:486-503: 0.0 when either norm is zero"""
    na, nb = math.sqrt(float(a @ a)), math.sqrt(float(b @ b))
    if na == 0 or nb == 0:
        return 0.0
    return float(a @ b) / (na * nb)


def loops(X, finite):
    """per row the first strict maximum over the later finite rows, and the first strict maximum over all pairs"""
    R = len(X)
    partner, sim = np.full(R, -1, np.int32), np.full(R, -np.inf)
    best, pair = -np.inf, (-1, -1)
    for i in range(R):
        for j in range(i + 1, R):
            if not (finite[i] and finite[j]):
                continue
            c = loop_cosine(X[i], X[j])
            if c > sim[i]:
                sim[i], partner[i] = c, j
            if c > best:
                best, pair = c, (i, j)
    return partner, sim, pair, best


@pytest.mark.parametrize("R", [1, 2, 3, 17, 64])
@pytest.mark.parametrize("kind", ["integer", "gaussian", "special"])
def test_restatement_equals_the_double_loop(R, kind):
    if kind == "integer":
        X = nearest_ref.integer_rows(R, 64, seed=R).astype(np.float64)
        if R >= 17:
            X[5] = X[2]; X[9] = X[2]; X[R - 1] = X[0]                    # ties: a triple, first against last
    else:
        X = nearest_ref.scaled_gaussian(R, 64, seed=R).astype(np.float64)
    finite = np.ones(R, bool)
    if kind == "special" and R >= 3:
        X[1] = 0.0
        if R >= 17:
            X[4, 3] = np.inf; X[7, 0] = np.nan; X[R - 2] = 0.0
            finite[[4, 7]] = False
    C = nearest_ref.cosine64(X)
    partner, sim = nearest_ref.later_nearest(C)
    pair, ps = nearest_ref.closest_pair(partner, sim)
    Xf = np.where(finite[:, None], X, 0.0)
    lp, ls, lpair, lbest = loops(Xf, finite)
    assert np.array_equal(partner, lp)
    if kind == "integer":
        assert np.array_equal(sim, ls) and pair == lpair and ps == lbest       # k / 16: exact either way
    else:
        assert np.allclose(sim, ls, rtol=0, atol=1e-14) and pair == lpair
        assert ps == lbest or abs(ps - lbest) <= 1e-14
    if R == 1:
        assert pair == (-1, -1) and ps == -np.inf and partner[0] == -1
    assert np.all(np.isnan(C[~finite])) and np.all(partner[~finite] == -1) and not np.isin(partner, np.flatnonzero(~finite)).any()
    if kind == "special" and R >= 3:
        assert partner[1] == 2 and sim[1] == 0.0                                # a zero row: cosine 0, the first later row


def test_victim_rule_as_a_pure_function(pkg):
    for victim in (nearest_ref.victim, pkg.ref_bank.similarity_victim):
        assert victim([3, 5, 0], (0, 1), 0.7) == 0                              # <
        assert victim([5, 3, 0], (0, 1), 0.7) == 1                              # >
        assert victim([4, 9, 4], (0, 2), 0.7) == 0                              # equal counts: i
        assert victim([4, 9, 4], (1, 2), -0.5) == 2
        assert victim([], None, -np.inf) is None and victim([7], None, -np.inf) is None       # fewer than 2 references
        assert victim([7], (-1, -1), -np.inf) is None
        # no pair above -1: max_similarity starts at -1 and the compare is strict, so index 0 goes whatever the counts are
        assert victim([9, 0], (0, 1), -1.0) == 0
        assert victim([9, 0, 0], (-1, -1), -np.inf) == 0
        assert victim([9, 0, 0], (1, 2), float("nan")) == 0


def test_fixture_replayed_through_the_restatement():
    fx = np.load(GOLDEN)
    removed, admitted, ids, branch = nearest_ref.replay(fx)
    assert np.array_equal(removed, fx["removed"]) and np.array_equal(admitted, fx["admitted"])
    assert ids == fx["final_ids"].tolist() and branch == fx["branches"].tolist()
    assert int((removed >= 0).sum()) >= 40 and min(branch) >= 5 and float(fx["min_gap"]) > 1e-4
    # the removals are not FIFO's: a bank that falls back to FIFO cannot pass the replay
    assert np.count_nonzero(removed[removed >= 0]) >= 20
