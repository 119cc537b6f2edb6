"""fp64 numpy restatement of the closest-pair kernels (nearest.hip: ``later_nearest_kernel``, ``closest_pair_kernel``) and of
``ReferenceBank``'s similarity-eviction victim rule (src/ref_bank.py:401-427).  tests/test_nearest_ref.py pins it to a literal
double loop; the GPU tests and the fixture replay compare against it.

Conventions, as include/tvc.h states them for tvc_closest_pair: the cosine of a pair with an all-zero row is 0 (the reference's
``_cosine_similarity``), a row whose squared norm is not finite is never a partner and has no partner itself, ``partner[i]`` is
the arg-max over j > i under (value descending, j ascending), ``pair`` the best row under (sim descending, i ascending) -- the
first maximal pair in lexicographic (i, j) order."""
import numpy as np

TAU = 1e-6        # the contract's bound in cosine units


def cosine64(X64: np.ndarray) -> np.ndarray:
    """fp64 [R, R] cosines of the rows; 0 where either row is all zero, NaN where either squared norm is not finite."""
    X64 = np.asarray(X64, np.float64)
    with np.errstate(all="ignore"):
        n = np.sqrt((X64 * X64).sum(1))
        finite = np.isfinite(n)
        Z = np.where(finite[:, None], X64, 0.0)
        rinv = np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)
        C = (Z @ Z.T) * rinv[:, None] * rinv[None, :]
    C[~finite, :] = np.nan
    C[:, ~finite] = np.nan
    return C


def later_nearest(C: np.ndarray):
    """C fp64 [R, R] (cosine64) -> (partner int32 [R], sim fp64 [R]): the first arg-max over j > i, NaN never wins; -1 / -inf
    where row i has no admissible later row."""
    R = C.shape[0]
    # a row that is not finite itself has only NaN entries, so it has no admissible column
    admissible = np.triu(np.ones((R, R), bool), 1) & ~np.isnan(C)
    U = np.where(admissible, C, -np.inf)
    partner = np.full(R, -1, np.int32)
    sim = np.full(R, -np.inf)
    has = admissible.any(1)
    if R:
        # np.argmax returns the FIRST maximum; an admissible -inf cannot occur (cosines are finite)
        j = np.argmax(U, axis=1)
        partner[has] = j[has]
        sim[has] = C[np.arange(R)[has], j[has]]
    return partner, sim


def closest_pair(partner: np.ndarray, sim: np.ndarray):
    """-> ((i, j), pair_sim): the best row with a partner under (sim descending, i ascending); ((-1, -1), -inf) without one."""
    has = np.flatnonzero(partner >= 0)
    if has.size == 0:
        return (-1, -1), -np.inf
    i = int(has[np.argmax(sim[has])])                 # the first maximum: the lowest i
    return (i, int(partner[i])), float(sim[i])


def victim(access_counts, pair, pair_sim):
    """The row the reference's ``_remove_most_similar`` pops, or None: fewer than 2 references -> None; no pair whose
    similarity exceeds -1 (``max_similarity`` starts at -1, the compare is strict) -> 0; else i if count[i] <= count[j] else j."""
    if len(access_counts) < 2:
        return None
    if pair is None or pair[0] < 0 or not (pair_sim > -1.0):
        return 0
    i, j = pair
    return int(i) if access_counts[i] <= access_counts[j] else int(j)


def evict(vectors, access_counts):
    """One similarity eviction over raw vectors, restated end to end -> (victim | None, pair, pair_sim, gap): gap = the best
    pair's fp64 lead over the second-best pair (inf with fewer than two pairs)."""
    C = cosine64(np.asarray(vectors, np.float64))
    partner, sim = later_nearest(C)
    pair, ps = closest_pair(partner, sim)
    iu = np.triu_indices(C.shape[0], 1)
    vals = np.sort(C[iu][~np.isnan(C[iu])])
    gap = float(vals[-1] - vals[-2]) if vals.size >= 2 else float("inf")
    return victim(access_counts, pair, ps), pair, ps, gap


def replay(fx):
    """The run recorded in tests/golden/ref_bank_similarity.npz (make_similarity_fixture.py) through this restatement alone ->
    (removed int64 [N], admitted bool [N], final ids, branch counts): admission against every stored row, eviction at
    capacity by `evict`, and after the recorded steps a query that counts an access for every row at or above query_t."""
    X, Q = fx["vectors"].astype(np.float64), fx["queries"].astype(np.float64)
    steps = fx["query_steps"].tolist()
    max_size, admit_t, query_t = int(fx["max_size"]), float(fx["admit_t"]), float(fx["query_t"])
    assert int(fx["top_k"]) >= max_size                            # every hit is returned: no rank decides an access
    ids, counts = [], []
    removed = np.full(len(X), -1, np.int64)
    admitted = np.zeros(len(X), bool)
    branch = [0, 0]
    for s in range(len(X)):
        if ids and cosine64(np.vstack([X[s][None], X[ids]]))[0, 1:].max() > admit_t:
            continue
        if len(ids) >= max_size:
            v, pair, _, _ = evict(X[ids], counts)
            if v is not None:
                branch[0 if v == pair[0] else 1] += 1
                removed[s] = v
                ids.pop(v)
                counts.pop(v)
        ids.append(s)
        counts.append(0)
        admitted[s] = True
        if s in steps:
            c = cosine64(np.vstack([Q[steps.index(s)][None], X[ids]]))[0, 1:]
            for k in np.flatnonzero(c >= query_t):
                counts[k] += 1
    return removed, admitted, ids, branch


def integer_rows(R: int, D: int, seed: int, nnz: int = 16) -> np.ndarray:
    """fp32 [R, D] rows with entries in {-1, 0, 1} and exactly `nnz` non-zeros: norm sqrt(nnz), every dot product an integer."""
    rng = np.random.default_rng(seed)
    X = np.zeros((R, D), np.float32)
    for r in range(R):
        X[r, rng.choice(D, nnz, replace=False)] = rng.choice(np.array([-1.0, 1.0], np.float32), nnz)
    return X


def scaled_gaussian(R: int, D: int, seed: int) -> np.ndarray:
    """fp32 [R, D] Gaussian rows around 8 centres, with row norms spread over 10^+-1."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((8, D))
    X = centres[rng.integers(0, 8, R)] + 0.9 * rng.standard_normal((R, D))
    X *= (10.0 ** rng.uniform(-1, 1, R))[:, None]
    return X.astype(np.float32)
