"""GPU: the radius-graph and DBSCAN kernels (tvc_radius_graph / tvc_dbscan_sweep / tvc_dbscan_finish), ``TVCEngine.dbscan`` and
``ReferenceBank``'s DBSCAN clustering against the fp64 restatement of tests/dbscan_ref.py (pinned to sklearn and scipy by
tests/test_dbscan_ref.py).

The band.  A pair is *decided* when |d2_64 - eps^2| > tau_ij, tau_ij = 8e-6 |x_i| |x_j| + 2^-20 (|x_i|^2 + |x_j|^2): twice the
4e-6 |x| |c| score bound of tests/test_gpu_kmeans.py (the factor 2 of d^2) plus the fp32 rounding of two D-term norm sums for
D <= 1 024; d2_64 is computed from the operand values the kernel sees (the bf16 values, or hi + lo of an fp32 row's planes).
Every decided pair's bit must equal fp64; the integer work (symmetry, padding, diagonal, degrees, components, labels, member
lists) is compared with ==.

Measured on an MI355X: see the figures each test prints, and EXPERIMENTS.md."""
import functools
import logging

import numpy as np
import pytest
import torch

import dbscan_ref
import kmeans_ref

pytestmark = pytest.mark.gpu
BANK = "dbscan-test"
EPS = 0.5

GRAPH_R = [1, 2, 63, 64, 65, 255, 256, 257, 513, 1000]
GRAPH_D = [64, 128, 512, 768]
KINDS = ["blobs", "unit"]


def operands(X: torch.Tensor) -> np.ndarray:
    """fp64 values of the rows as the kernels see them: the bf16 values, or hi + lo of the fp32 rows' bf16 planes."""
    if X.dtype == torch.bfloat16:
        return X.double().numpy()
    hi = X.bfloat16().float()
    lo = (X - hi).bfloat16().float()
    return hi.double().numpy() + lo.double().numpy()


@functools.lru_cache(maxsize=None)
def case(R, D, kind, bf16):
    """-> (X cpu tensor as registered, X64 operands, fp64 graph, margin, undecided); computed once, shared, never modified."""
    X = torch.from_numpy(dbscan_ref.gen(R, D, kind, 7))
    if bf16:
        X = X.bfloat16()
    X64 = operands(X)
    margin, und = dbscan_ref.band(X64, EPS)
    return X, X64, dbscan_ref.adjacency(X64, EPS), margin, und


class Slot:
    """Registers rows under the test's bank name for the duration of a ``with``."""

    def __init__(self, eng, X):
        self.eng, self.X = eng, X

    def __enter__(self):
        self.eng.set_bank(self.X.to(self.eng.device), name=BANK)
        return self.eng

    def __exit__(self, *exc):
        self.eng.release_bank(BANK)


def bits_of(adj: torch.Tensor, R: int) -> np.ndarray:
    """the engine's int32 words -> bool [R, 32 W], padding included"""
    assert adj.dtype == torch.int32 and tuple(adj.shape) == (R, (R + 63) // 64 * 2)
    return dbscan_ref.unpack_bits(adj.cpu().numpy().view(np.uint32), R)


def check_graph(G, degree, R, A64, margin, und, finite=None):
    """The exact properties of a returned graph, then the decided pairs against fp64 -> the worst margin among differing pairs."""
    finite = np.ones(R, bool) if finite is None else finite
    assert not G[:, R:].any()                                           # padding bits
    G = G[:, :R]
    assert np.array_equal(G, G.T)                                       # symmetric bit for bit
    assert np.array_equal(np.diag(G), finite)                           # the diagonal of every finite row
    assert np.array_equal(degree, G.sum(1))                             # degree = popcount of the returned row
    differ = G != A64
    assert not (differ & ~und).any()                                    # every decided pair's bit equals fp64
    return float(margin[differ].max()) if differ.any() else 0.0


# ---- 1: the graph against fp64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", GRAPH_D)
@pytest.mark.parametrize("R", GRAPH_R)
def test_graph_against_fp64(gpu_engine, R, D, kind, bf16):
    X, X64, A64, margin, und = case(R, D, kind, bf16)
    with Slot(gpu_engine, X) as eng:
        adj, degree = eng.radius_graph(EPS, bank=BANK)
    assert degree.dtype == torch.int32 and tuple(degree.shape) == (R,)
    G = bits_of(adj, R)
    worst = check_graph(G, degree.cpu().numpy(), R, A64, margin, und)
    print(f"graph R={R} D={D} {kind} {'bf16' if bf16 else 'f32'}: {int(A64.sum())} edges, {int(und.sum()) // 2} undecided pairs, "
          f"{int((G[:, :R] != A64).sum()) // 2} pairs differ from fp64, worst |d2 - eps2| / tau among them {worst:.3f}")
    assert worst <= 1.0


# ---- 2: planted near-threshold pairs -------------------------------------------------------------------------------------
def planted(scale, eps, D=128, n_base=24, seed=3):
    """fp32 rows: per base row of norm `scale` an exact duplicate, a near duplicate (d ~ 1e-3) and two partners whose squared
    distance to the base row -- measured on the operands -- is eps^2 - 3 tau and eps^2 + 3 tau.  -> (X, pairs) with pairs =
    [(i, j, inside)]."""
    rng = np.random.default_rng(seed)
    eps = float(np.float32(eps))
    rows, pairs = [], []
    for b in range(n_base):
        x = rng.standard_normal(D)
        x = (scale * x / np.linalg.norm(x)).astype(np.float32)
        near = (x.astype(np.float64) + 1e-3 * unit(rng, D)).astype(np.float32)
        i0 = len(rows)
        rows += [x, x.copy(), near]
        pairs += [(i0, i0 + 1, True), (i0, i0 + 2, True), (i0 + 1, i0 + 2, True)]
        x64 = operands(torch.from_numpy(x[None]))[0]
        t = dbscan_ref.tau(np.stack([x64, x64]))[0, 1]
        for sign in (-1.0, 1.0):
            target = eps * eps + sign * 3.0 * t
            off = np.sqrt(target) * unit(rng, D)
            for _ in range(4):                                          # rescale until the OPERANDS are at the target
                p = (x.astype(np.float64) + off).astype(np.float32)
                d2 = ((operands(torch.from_numpy(p[None]))[0] - x64) ** 2).sum()
                off *= np.sqrt(target / d2)
            rows.append(p)
            pairs += [(i0, len(rows) - 1, sign < 0), (i0 + 1, len(rows) - 1, sign < 0)]
    return np.stack(rows), pairs


def unit(rng, D):
    u = rng.standard_normal(D)
    return u / np.linalg.norm(u)


@pytest.mark.parametrize("scale,eps", [(1.0, 0.5), (1.0, 0.01), (4.0, 0.5), (4.0, 0.05)])
def test_planted_near_threshold_pairs(gpu_engine, scale, eps):
    Xn, pairs = planted(scale, eps)
    eps32 = float(np.float32(eps))
    X = torch.from_numpy(Xn)
    X64 = operands(X)
    margin, und = dbscan_ref.band(X64, eps32)
    A64 = dbscan_ref.adjacency(X64, eps32)
    R = len(Xn)
    I, J, inside = (np.array(v) for v in zip(*pairs))
    partner = (np.arange(R) % 5) >= 3
    m = margin[I, J][partner[J]]
    assert (m > 2.0).all() and (m < 4.0).all(), "the planting missed eps^2 +- 3 tau"
    assert not und[I, J].any() and np.array_equal(A64[I, J], inside)
    with Slot(gpu_engine, X) as eng:
        adj, degree = eng.radius_graph(eps, bank=BANK)
    G = bits_of(adj, R)
    worst = check_graph(G, degree.cpu().numpy(), R, A64, margin, und)
    print(f"planted scale={scale} eps={eps}: partner margins {m.min():.2f} .. {m.max():.2f} tau, {int(und.sum()) // 2} undecided pairs "
          f"elsewhere, worst differing margin {worst:.3f}")
    assert np.array_equal(G[I, J], inside) and np.array_equal(G[J, I], inside)      # every planted pair is decided correctly
    assert worst <= 1.0


def test_a_row_of_nans_has_no_neighbours(gpu_engine):
    Xn, _ = planted(1.0, 0.5)
    R, k = len(Xn), 37
    far = Xn.copy()
    far[k] = 0.0
    far[k, 0] = 100.0                                                  # a finite row far from every other: the same graph elsewhere
    nan = Xn.copy()
    nan[k] = np.nan
    with Slot(gpu_engine, torch.from_numpy(far)) as eng:
        adj_f, deg_f = eng.radius_graph(0.5, bank=BANK)
    with Slot(gpu_engine, torch.from_numpy(nan)) as eng:
        adj_n, deg_n = eng.radius_graph(0.5, bank=BANK)
        labels, core, C, _ = eng.dbscan_labels(adj_n, deg_n, 2)
        labels_f, core_f, C_f, _ = eng.dbscan_labels(adj_f, deg_f, 2)
    Gf, Gn = bits_of(adj_f, R), bits_of(adj_n, R)
    assert deg_n[k].item() == 0 and not Gn[k].any() and not Gn[:, k].any()        # not even itself
    assert deg_f[k].item() == 1 and Gf[k, k]
    Gf[k, k] = False
    assert np.array_equal(Gf, Gn)                                       # no other row is disturbed
    assert labels[k].item() == -1 and not core[k].item()
    keep = np.arange(R) != k
    assert C == C_f and np.array_equal(labels.cpu().numpy()[keep], labels_f.cpu().numpy()[keep])
    X64 = operands(torch.from_numpy(nan))
    A64 = dbscan_ref.adjacency(X64, 0.5)
    finite = np.isfinite(X64).all(1)
    margin, und = dbscan_ref.band(np.where(finite[:, None], X64, 0.0), 0.5)
    und[k] = und[:, k] = False
    assert check_graph(Gn, deg_n.cpu().numpy(), R, A64, margin, und, finite) <= 1.0


# ---- 3: components on supplied graphs, exact -----------------------------------------------------------------------------
def chain(R, seed=11):
    pos = np.random.default_rng(seed).permutation(R)
    return np.abs(pos[:, None] - pos[None, :]) <= 1


def two_cliques_one_border():
    """rows 0 .. 4 and 6 .. 10 are cliques, row 5 touches one row of each: at min_samples 5 it is a border row of both."""
    A = np.eye(11, dtype=bool)
    A[:5, :5] = True
    A[6:, 6:] = True
    A[5, 2] = A[2, 5] = A[5, 8] = A[8, 5] = True
    return A


def star(R=21):
    A = np.eye(R, dtype=bool)
    A[7, :] = A[:, 7] = True
    return A


def gnp(R, p, seed):
    A = np.triu(np.random.default_rng(seed).random((R, R)) < p, 1)
    return A | A.T | np.eye(R, dtype=bool)


SIZES = [1, 31, 32, 33, 777, 2000]
GRAPHS = {"chain2000-ms2": (lambda: chain(2000), 2), "chain2000-ms3": (lambda: chain(2000), 3),
          "cliques-border": (two_cliques_one_border, 5), "star": (star, 3)}
for _R in SIZES:
    GRAPHS[f"identity{_R}-ms1"] = (functools.partial(np.eye, _R, dtype=bool), 1)
    GRAPHS[f"identity{_R}-ms2"] = (functools.partial(np.eye, _R, dtype=bool), 2)
    GRAPHS[f"complete{_R}"] = (functools.partial(np.ones, (_R, _R), bool), min(5, _R))
    GRAPHS[f"chain{_R}-ms3"] = (functools.partial(chain, _R), 3)
for _p in (0.004, 0.0086, 0.02):                                        # around ln(777) / 777, the connectivity threshold
    GRAPHS[f"gnp777-{_p}-ms1"] = (functools.partial(gnp, 777, _p, 5), 1)
    GRAPHS[f"gnp777-{_p}-ms4"] = (functools.partial(gnp, 777, _p, 5), 4)


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_components_on_supplied_graphs(gpu_engine, name):
    make, ms = GRAPHS[name]
    A = make()
    R = len(A)
    want_labels, want_core, want_C = dbscan_ref.labels(A, ms)
    adj = torch.from_numpy(dbscan_ref.pack_bits(A).view(np.int32)).to(gpu_engine.device)
    degree = torch.from_numpy(A.sum(1).astype(np.int32)).to(gpu_engine.device)
    labels, core, C, sweeps = gpu_engine.dbscan_labels(adj, degree, ms)
    print(f"components {name}: R={R} min_samples={ms}: {want_C} clusters, {int((~want_core & (want_labels >= 0)).sum())} border rows, "
          f"{int((want_labels < 0).sum())} noise rows, {sweeps} sweeps")
    assert labels.dtype == torch.int32 and core.dtype == torch.bool
    assert C == want_C
    assert np.array_equal(core.cpu().numpy(), want_core)
    assert np.array_equal(labels.cpu().numpy(), want_labels)
    assert 1 <= sweeps <= R
    if name == "cliques-border":
        assert C == 2 and labels[5].item() == 0 and labels[:5].tolist() == [0] * 5 and labels[6:].tolist() == [1] * 5
    if name.startswith("identity") and ms == 1:
        assert labels.tolist() == list(range(R))
    labels2, core2, C2, _ = gpu_engine.dbscan_labels(adj, degree, ms)
    assert torch.equal(labels, labels2) and torch.equal(core, core2) and C2 == C


def test_labels_argument_checks(gpu_engine):
    adj = torch.zeros((33, 2), dtype=torch.int32, device=gpu_engine.device)
    deg = torch.zeros(33, dtype=torch.int32, device=gpu_engine.device)
    with pytest.raises(ValueError):
        gpu_engine.dbscan_labels(adj, deg, 0)
    with pytest.raises(ValueError):
        gpu_engine.dbscan_labels(adj[:, :1], deg, 2)
    with pytest.raises(ValueError):
        gpu_engine.dbscan_labels(adj, deg[:5], 2)
    with Slot(gpu_engine, torch.zeros((4, 64))) as eng:
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError):
                eng.radius_graph(bad, bank=BANK)


# ---- 4: end to end, exact ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decided_case(R, D, kind, bf16):
    """case() without the higher-indexed row of every undecided pair -> (X, X64, fp64 labels, core, C, rows dropped)."""
    X, X64, _, _, und = case(R, D, kind, bf16)
    drop = np.unique(np.nonzero(np.triu(und, 1))[1])
    keep = np.setdiff1d(np.arange(R), drop)
    X, X64 = X[torch.from_numpy(keep)], X64[keep]
    assert not dbscan_ref.band(X64, EPS)[1].any()
    lab, core, C = dbscan_ref.labels(dbscan_ref.adjacency(X64, EPS), 5)
    return X, X64, lab, core, C, len(drop)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", GRAPH_D)
@pytest.mark.parametrize("R", [257, 513, 1000])
def test_dbscan_end_to_end(gpu_engine, R, D, kind, bf16):
    X, X64, want, want_core, C, dropped = decided_case(R, D, kind, bf16)
    assert dropped <= 0.01 * R
    n = len(X)
    with Slot(gpu_engine, X) as eng:
        labels, core, centres, order, offsets = eng.dbscan(EPS, 5, bank=BANK)
        again = eng.dbscan(EPS, 5, bank=BANK)
    print(f"dbscan R={R} D={D} {kind} {'bf16' if bf16 else 'f32'}: {dropped} rows dropped, {C} clusters, "
          f"{int((~want_core & (want >= 0)).sum())} border rows, {int((want < 0).sum())} noise rows")
    assert np.array_equal(labels.cpu().numpy(), want)
    assert np.array_equal(core.cpu().numpy(), want_core)
    w_off, w_order = kmeans_ref.lists(want, C)
    assert np.array_equal(offsets.cpu().numpy(), w_off)
    order = order.cpu().numpy()
    assert np.array_equal(order[:w_off[C]], w_order) and (order[w_off[C]:] == -1).all() and len(order) == n
    if C == 0:
        assert centres is None and again[2] is None
    else:
        err = np.abs(centres.cpu().numpy().astype(np.float64) - dbscan_ref.centres(X64, want, C)).max()
        print(f"    centre err {err / (2.0 ** -16 * np.abs(X64).max()):.3f} of its bound")
        assert tuple(centres.shape) == (C, D) and err <= 2.0 ** -16 * np.abs(X64).max()
        assert torch.equal(centres, again[2])                            # a second call returns identical bits
    assert torch.equal(labels, again[0]) and torch.equal(core, again[1]) and torch.equal(torch.from_numpy(order).to(again[3].device), again[3])
    assert torch.equal(offsets, again[4])


def test_all_noise_and_all_core(gpu_engine):
    rng = np.random.default_rng(2)
    X = torch.from_numpy(rng.standard_normal((300, 64)).astype(np.float32))           # rows ~11 apart
    with Slot(gpu_engine, X) as eng:
        labels, core, centres, order, offsets = eng.dbscan(EPS, 5, bank=BANK)
        assert centres is None and (labels == -1).all() and not core.any()
        assert (order == -1).all() and offsets.tolist() == [0]
        labels, core, centres, order, offsets = eng.dbscan(EPS, 1, bank=BANK)         # min_samples 1: every row is a core row
        assert core.all() and labels.tolist() == list(range(300)) and order.tolist() == list(range(300))
        assert offsets.tolist() == list(range(301))
        assert np.abs(centres.cpu().numpy().astype(np.float64) - operands(X)).max() <= 2.0 ** -16 * X.abs().max().item()


# ---- 5: ReferenceBank ------------------------------------------------------------------------------------------------------
def test_reference_bank_dbscan(pkg, gpu_engine):
    lone = np.random.default_rng(4).standard_normal((8, 64))          # 8 unit rows in random directions: ~1.4 from every other row
    X = np.concatenate([dbscan_ref.gen(592, 64, "unit", 21), (lone / np.linalg.norm(lone, axis=1, keepdims=True)).astype(np.float32)])
    X64 = operands(torch.from_numpy(X))
    und = dbscan_ref.band(X64, EPS)[1]
    keep = np.setdiff1d(np.arange(600), np.unique(np.nonzero(np.triu(und, 1))[1]))
    assert len(keep) >= 594
    X, X64 = X[keep], X64[keep]
    n = len(X)
    want, want_core, C = dbscan_ref.labels(dbscan_ref.adjacency(X64, EPS), 5)
    assert C >= 2 and (want < 0).any()
    cfg = pkg.ReferenceBankConfig(clustering_method="dbscan", dbscan_eps=EPS, feature_dim=64, max_size=n)
    bank = pkg.ReferenceBank(cfg, engine=gpu_engine)
    bank.add_references(X, [{"i": i} for i in range(n)])
    assert bank.perform_clustering() is True
    assert not gpu_engine.has_bank(bank.bank_name + ":raw")
    assert bank.clusters == {c: np.flatnonzero(want == c).tolist() for c in range(C)}
    assert [r.cluster_id for r in bank.references] == [int(l) if l >= 0 else None for l in want]
    assert np.abs(bank.get_cluster_centers() - dbscan_ref.centres(X64, want, C)).max() <= 2.0 ** -16 * np.abs(X64).max()
    assert bank.cluster_init is None and bank.stats["clustering_count"] == 1 and bank.stats["last_clustering_time"] is not None
    for c in bank.clusters:
        got = bank.query_by_cluster(c, 5)
        assert len(got) == min(5, len(bank.clusters[c])) and all(a is bank.references[i] for a, i in zip(got, bank.clusters[c]))
    assert bank.query_by_cluster(C) == []
    # eviction under fifo (src/ref_bank.py:429-450): index 0 leaves its cluster, every other index shifts down by one
    old, first = {c: list(m) for c, m in bank.clusters.items()}, bank.references[0]
    bank._remove_reference()
    assert len(bank) == n - 1 and all(r is not first for r in bank.references)
    assert bank.clusters == {c: [i - 1 for i in m if i != 0] for c, m in old.items() if [i for i in m if i != 0]}


def test_reference_bank_dbscan_all_noise_and_refusals(pkg, gpu_engine, caplog):
    V = np.random.default_rng(9).standard_normal((30, 64))
    far = pkg.ReferenceBank(pkg.ReferenceBankConfig(clustering_method="dbscan", dbscan_eps=EPS, feature_dim=64), engine=gpu_engine)
    far.add_references(V)
    assert far.perform_clustering() is True                             # the reference's behaviour: a success without clusters
    assert far.clusters == {} and far.get_cluster_centers() is None and all(r.cluster_id is None for r in far.references)
    assert far.stats["clustering_count"] == 1
    db = pkg.ReferenceBank(pkg.ReferenceBankConfig(clustering_method="dbscan", feature_dim=64), engine=gpu_engine)    # dbscan_eps=None
    db.add_references(V)
    with caplog.at_level(logging.ERROR):
        assert db.perform_clustering() is False
    assert any(r.levelno == logging.ERROR and "clustering method 'dbscan' is not built on the GPU path" in r.getMessage()
               for r in caplog.records)
    assert db.clusters == {} and db.stats["clustering_count"] == 0
    with pytest.raises(ValueError):
        pkg.ReferenceBankConfig(dbscan_eps=0.0)
    with pytest.raises(ValueError):
        pkg.ReferenceBankConfig(dbscan_min_samples=0)
