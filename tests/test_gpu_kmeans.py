"""GPU: the k-means kernels (tvc_kmeans_assign / tvc_kmeans_update), ``TVCEngine.kmeans`` and ``ReferenceBank``'s
clustering against the fp64 reference of tests/kmeans_ref.py (pinned to sklearn by tests/test_kmeans_ref.py).

Bounds.  tau = 4e-6 * max(|x|, max_j |c_j|) * max_j |c_j| per row: the project's cosine bound (1e-6 per unit-row product,
tests/test_gpu_api.py) scaled to the operands' norms, for the two scores a comparison involves, with a factor 2.  A label may
differ from the fp64 arg-max only where the two scores are within tau, and on at most 1 % of a case's rows.  Centres: 2^-16 *
max |x| per component (the plane reconstruction is within 2^-17 relative, the fp32 sum of at most 4 096 members well inside
the rest)."""
import functools
import logging
from pathlib import Path

import numpy as np
import pytest
import torch

import kmeans_ref

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"
BANK = "kmeans-test"

SHAPES = [(1, 1, 64), (257, 3, 64), (1000, 100, 512), (1000, 300, 64), (4096, 1024, 768), (300, 300, 128)]
KINDS = ["gauss", "unit", "blobs"]
PINNED = [(2000, 8, 64, 0), (1000, 100, 512, 1), (257, 3, 64, 4), (20, 20, 512, 3)]


def operands(X: torch.Tensor) -> np.ndarray:
    """fp64 values of the rows as the kernels see them: the bf16 values, or hi + lo of the fp32 rows' bf16 planes."""
    if X.dtype == torch.bfloat16:
        return X.double().numpy()
    hi = X.bfloat16().float()
    lo = (X - hi).bfloat16().float()
    return hi.double().numpy() + lo.double().numpy()


@functools.lru_cache(maxsize=None)
def case(R, K, D, kind, bf16):
    """-> (X cpu tensor as registered, X64 operands, C fp32, fp64 scores [R, K]); computed once, shared, never modified."""
    rng = np.random.default_rng(1000 * R + 10 * K + D + len(kind))
    if kind == "blobs":
        X, _ = kmeans_ref.blobs(R, K, D, 11)
        C = X[rng.choice(R, K, replace=False)] + 0.05 * rng.standard_normal((K, D))
    else:
        X, C = rng.standard_normal((R, D)), rng.standard_normal((K, D))
        if kind == "unit":
            X, C = X / np.linalg.norm(X, axis=1, keepdims=True), C / np.linalg.norm(C, axis=1, keepdims=True)
    X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))
    if bf16:
        X = X.bfloat16()
    C = np.ascontiguousarray(C, dtype=np.float32)
    X64 = operands(X)
    return X, X64, C, kmeans_ref.scores(X64, C)


def tau_rows(X64, C):
    cmax = np.linalg.norm(C.astype(np.float64), axis=1).max()
    return 4e-6 * np.maximum(np.linalg.norm(X64, axis=1), cmax) * cmax


class Slot:
    """Registers rows under the test's bank name for the duration of a ``with``."""

    def __init__(self, eng, X):
        self.eng, self.X = eng, X

    def __enter__(self):
        self.eng.set_bank(self.X.to(self.eng.device), name=BANK)
        return self.eng

    def __exit__(self, *exc):
        self.eng.release_bank(BANK)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R,K,D", SHAPES)
def test_assign_against_fp64(gpu_engine, R, K, D, kind, bf16):
    X, X64, C, S = case(R, K, D, kind, bf16)
    with Slot(gpu_engine, X) as eng:
        labels, score, dist2 = (t.cpu().numpy() for t in eng.kmeans_assign(torch.from_numpy(C).to(eng.device), bank=BANK))
    assert labels.dtype == np.int32 and labels.shape == (R,)
    assert (labels >= 0).all() and (labels < K).all()
    tau = tau_rows(X64, C)
    best, chosen = S.max(1), S[np.arange(R), labels]
    x2 = (X64 * X64).sum(1)
    deficit = ((best - chosen) / tau).max()
    differ = float((labels != S.argmax(1)).mean())
    e_score = (np.abs(score - chosen) / tau).max()
    e_dist = (np.abs(dist2 - np.maximum(0.0, x2 - 2 * chosen)) / (2 * tau + 1e-6 * x2)).max()
    print(f"assign R={R} K={K} D={D} {kind} {'bf16' if bf16 else 'f32'}: deficit {deficit:.3f} tau, labels differing {differ:.4%}, "
          f"score err {e_score:.3f} tau, dist2 err {e_dist:.3f} of its bound")
    assert deficit <= 1.0
    assert differ <= 0.01
    assert e_score <= 1.0
    assert e_dist <= 1.0


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R,K,D", SHAPES)
def test_update_against_fp64(gpu_engine, R, K, D, kind, bf16):
    X, X64, C, S = case(R, K, D, kind, bf16)
    labels = S.argmax(1)
    want_C, want_counts = kmeans_ref.update(X64, labels, C)
    want_off, want_order = kmeans_ref.lists(labels, K)
    with Slot(gpu_engine, X) as eng:
        Cin = torch.from_numpy(C).to(eng.device)
        out, counts, offsets, order = eng.kmeans_update(torch.from_numpy(labels.astype(np.int32)).to(eng.device), Cin, bank=BANK,
                                                        want_lists=True)
        out2, counts2, none_off, none_order = eng.kmeans_update(torch.from_numpy(labels.astype(np.int32)).to(eng.device), Cin, bank=BANK)
    assert none_off is None and none_order is None
    assert torch.equal(out, out2) and torch.equal(counts, counts2)        # the lists are optional, the centres the same bits
    out, counts, offsets, order = out.cpu().numpy(), counts.cpu().numpy(), offsets.cpu().numpy(), order.cpu().numpy()
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(offsets, want_off)
    assert np.array_equal(order[:offsets[K]], want_order)
    for j in range(K):
        assert (np.diff(order[offsets[j]:offsets[j + 1]]) > 0).all()
    err = np.abs(out.astype(np.float64) - want_C).max() / (2.0 ** -16 * np.abs(X64).max())
    print(f"update R={R} K={K} D={D} {kind} {'bf16' if bf16 else 'f32'}: centre err {err:.3f} of its bound, "
          f"{int((want_counts == 0).sum())} empty")
    assert err <= 1.0
    empty = want_counts == 0
    assert np.array_equal(out[empty].view(np.uint32), C[empty].view(np.uint32))      # bit for bit


def test_ties_nan_and_rows_without_a_cluster(gpu_engine):
    rng = np.random.default_rng(5)
    K, D = 12, 64
    C = rng.standard_normal((K, D)).astype(np.float32)
    C[9] = C[5]                                                         # bit-identical centres: 9 never wins
    near = np.concatenate([C[5] + 0.01 * rng.standard_normal((60, D)), C[9] + 0.01 * rng.standard_normal((60, D))])
    X = np.concatenate([near, C, rng.standard_normal((150, D))]).astype(np.float32)     # rows 120 .. 131 equal the centres
    R = len(X)
    with Slot(gpu_engine, torch.from_numpy(X)) as eng:
        labels = eng.kmeans_assign(torch.from_numpy(C).to(eng.device), bank=BANK)[0].cpu().numpy()
        assert (labels != 9).all()
        assert (labels[:120] == 5).all()
        assert labels[120:132].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 5, 10, 11]       # a row equal to a centre gets it
        Cn = C.copy()
        Cn[3, 17] = np.nan                                              # one NaN centre never wins
        labels_n = eng.kmeans_assign(torch.from_numpy(Cn).to(eng.device), bank=BANK)[0].cpu().numpy()
        assert (labels_n != 3).all() and (labels_n >= 0).all()
        keep = labels != 3
        assert np.array_equal(labels_n[keep], labels[keep])
    Xn = X.copy()
    Xn[7] = np.nan                                                      # one all-NaN row: no label, no cluster, no list
    with Slot(gpu_engine, torch.from_numpy(Xn)) as eng:
        Cd = torch.from_numpy(C).to(eng.device)
        lab, score, dist2 = eng.kmeans_assign(Cd, bank=BANK)
        assert lab[7].item() == -1 and dist2[7].item() == 0.0
        assert np.array_equal(np.delete(lab.cpu().numpy(), 7), np.delete(labels, 7))
        out, counts, offsets, order = eng.kmeans_update(lab, Cd, bank=BANK, want_lists=True)
        order = order.cpu().numpy()
        assert counts.sum().item() == R - 1 and offsets[K].item() == R - 1
        assert 7 not in order[:R - 1].tolist() and order[R - 1] == -1
        assert sorted(order[:R - 1].tolist()) == [i for i in range(R) if i != 7]
        assert torch.isfinite(out).all()
        assert np.array_equal(out[9].cpu().numpy().view(np.uint32), C[9].view(np.uint32))   # 9 is empty: its row comes back


def fit_bounds(X64, C):
    tau_max = tau_rows(X64, C).max()
    return 2.0 ** -16 * np.abs(X64).max(), len(X64) * (2 * tau_max + 1e-6 * (X64 * X64).sum(1).max())


@pytest.mark.parametrize("R,K,D,seed", PINNED)
def test_fit_matches_fp64_lloyd(gpu_engine, R, K, D, seed):
    X, C0 = kmeans_ref.blobs(R, K, D, seed)
    Xt = torch.from_numpy(X)
    X64 = operands(Xt)
    wC, wl, winertia, wit, emptied = kmeans_ref.lloyd(X64, C0)
    with Slot(gpu_engine, Xt) as eng:
        C, labels, inertia, n_iter, order, offsets = eng.kmeans(K, bank=BANK, init=torch.from_numpy(C0).to(eng.device), n_init=1)
    c_bound, i_bound = fit_bounds(X64, wC)
    c_err = np.abs(C.cpu().numpy().astype(np.float64) - wC).max()
    print(f"fit R={R} K={K} D={D}: n_iter {n_iter} (fp64 {wit}), centre err {c_err / c_bound:.3f} of its bound, "
          f"inertia err {abs(inertia - winertia) / i_bound:.3f} of its bound")
    assert emptied == 0
    assert np.array_equal(labels.cpu().numpy(), wl)
    assert n_iter == wit
    assert c_err <= c_bound
    assert abs(inertia - winertia) <= i_bound
    w_off, w_order = kmeans_ref.lists(wl, K)
    assert np.array_equal(offsets.cpu().numpy(), w_off) and np.array_equal(order.cpu().numpy()[:w_off[K]], w_order)


def test_fit_is_deterministic(gpu_engine):
    X, _ = kmeans_ref.blobs(2000, 8, 64, 0)
    with Slot(gpu_engine, torch.from_numpy(X)) as eng:
        a = eng.kmeans(8, bank=BANK, init="k-means++", n_init=3, seed=7)
        b = eng.kmeans(8, bank=BANK, init="k-means++", n_init=3, seed=7)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[4], b[4]) and torch.equal(a[5], b[5])
    assert a[2] == b[2] and a[3] == b[3]


def test_fit_keeps_the_best_restart(gpu_engine):
    X, _ = kmeans_ref.blobs(600, 12, 64, 6)
    with Slot(gpu_engine, torch.from_numpy(X)) as eng:
        runs = {}
        pair = None
        for s in range(12):          # any two consecutive seeds whose single restarts end at different inertias
            runs[s] = eng.kmeans(12, bank=BANK, init="random", n_init=1, seed=s)
            if s - 1 in runs and runs[s - 1][2] != runs[s][2]:
                pair = (s - 1, s)
                break
        assert pair is not None, "random starts never reached two different optima: the restart rule cannot be shown"
        lo = min(pair, key=lambda s: (runs[s][2], s))
        both = eng.kmeans(12, bank=BANK, init="random", n_init=2, seed=pair[0])       # restart i draws from seed + i
        listed = eng.kmeans(12, bank=BANK, init="random", n_init=2, seed=list(pair))
    for got in (both, listed):
        assert got[2] == runs[lo][2] and got[3] == runs[lo][3]
        assert torch.equal(got[0], runs[lo][0]) and torch.equal(got[1], runs[lo][1])


def test_fit_refills_an_empty_cluster(gpu_engine):
    X, C0 = kmeans_ref.blobs(2000, 8, 64, 0)
    C0 = C0.copy()
    C0[2] = 1e3
    with Slot(gpu_engine, torch.from_numpy(X)) as eng:
        C, labels, inertia, n_iter, order, offsets = eng.kmeans(8, bank=BANK, init=torch.from_numpy(C0).to(eng.device), n_init=1)
    counts = np.bincount(labels.cpu().numpy(), minlength=8)
    assert counts.min() >= 1 and counts.sum() == 2000
    assert np.array_equal(np.diff(offsets.cpu().numpy()), counts)


# ---- ReferenceBank ---------------------------------------------------------------------------------------------------
def test_reference_bank_golden_vectors_become_singletons(pkg, gpu_engine):
    g = np.load(G / "ref_bank.npz")
    V = g["vectors"]
    bank = pkg.ReferenceBank(pkg.ReferenceBankConfig(clustering_method="kmeans", num_clusters=100, feature_dim=512), engine=gpu_engine)
    bank.add_references(V)
    assert bank.perform_clustering() is True
    assert sorted(bank.clusters) == list(range(20)) and all(len(m) == 1 for m in bank.clusters.values())
    centres = bank.get_cluster_centers()
    members = np.array([bank.clusters[j][0] for j in range(20)])
    assert sorted(members.tolist()) == list(range(20))
    assert np.abs(centres - V[members]).max() <= 2.0 ** -16 * np.abs(V).max()
    assert [r.cluster_id for r in bank.references] == np.argsort(members).tolist()
    assert bank.stats["clustering_count"] == 1 and bank.stats["last_clustering_time"] is not None


def test_reference_bank_clusters_match_fp64_lloyd(pkg, gpu_engine):
    X, _ = kmeans_ref.blobs(1000, 8, 512, 5)
    bank = pkg.ReferenceBank(pkg.ReferenceBankConfig(clustering_method="kmeans", num_clusters=8, feature_dim=512, max_size=1000),
                             engine=gpu_engine)
    bank.add_references(X, [{"i": i} for i in range(1000)])
    q = X[3].astype(np.float64)
    before = [(it.metadata["i"], s) for it, s in bank.query_similar(q, top_k=10, similarity_threshold=0.2)]
    assert bank.perform_clustering() is True
    # the temporary raw-vector slot is gone and the unit-row slot answers as before
    assert not gpu_engine.has_bank(bank.bank_name + ":raw")
    assert [(it.metadata["i"], s) for it, s in bank.query_similar(q, top_k=10, similarity_threshold=0.2)] == before
    wC, wl, _, _, emptied = kmeans_ref.lloyd(X, bank.cluster_init)
    assert emptied == 0
    assert bank.clusters == {j: np.flatnonzero(wl == j).tolist() for j in range(8) if (wl == j).any()}
    assert [r.cluster_id for r in bank.references] == wl.tolist()
    assert np.abs(bank.get_cluster_centers() - wC).max() <= 2.0 ** -16 * np.abs(X).max()
    for j in bank.clusters:
        got = bank.query_by_cluster(j, 5)
        assert len(got) == min(5, len(bank.clusters[j])) and all(a is bank.references[i] for a, i in zip(got, bank.clusters[j]))
    assert bank.query_by_cluster(999) == []
    c = bank.get_cluster_centers()
    c[:] = 0.0
    assert np.abs(bank.get_cluster_centers()).max() > 0                 # a copy
    # eviction under fifo (src/ref_bank.py:429-450): index 0 leaves its cluster, every other index shifts down by one
    old, first = {j: list(m) for j, m in bank.clusters.items()}, bank.references[0]
    bank._remove_reference()
    assert len(bank) == 999 and all(r is not first for r in bank.references)
    assert bank.clusters == {j: [i - 1 for i in m if i != 0] for j, m in old.items() if [i for i in m if i != 0]}


def test_reference_bank_auto_clustering_and_refusals(pkg, gpu_engine, caplog):
    rng = np.random.default_rng(9)
    cfg = pkg.ReferenceBankConfig(clustering_method="kmeans", num_clusters=4, auto_clustering=True, clustering_interval=50,
                                  feature_dim=64, similarity_threshold=0.99)
    bank = pkg.ReferenceBank(cfg, engine=gpu_engine)
    for i in range(100):
        assert bank.add_reference(rng.standard_normal(64), {"i": i})
    assert bank.stats["clustering_count"] == 2
    assert sum(len(m) for m in bank.clusters.values()) == 100 and all(r.cluster_id is not None for r in bank.references)
    V = rng.standard_normal((30, 64))
    none = pkg.ReferenceBank(pkg.ReferenceBankConfig(feature_dim=64), engine=gpu_engine)        # the default: "none"
    none.add_references(V)
    assert none.perform_clustering() is False and none.perform_clustering(force=True) is False
    assert none.clusters == {} and none.get_cluster_centers() is None and none.stats["clustering_count"] == 0
    db = pkg.ReferenceBank(pkg.ReferenceBankConfig(clustering_method="dbscan", feature_dim=64), engine=gpu_engine)
    db.add_references(V)
    with caplog.at_level(logging.ERROR):
        assert db.perform_clustering() is False
    assert any(r.levelno == logging.ERROR and "dbscan" in r.getMessage() for r in caplog.records)
    with pytest.raises(ValueError):
        pkg.ReferenceBankConfig(clustering_method="spectral")
    one = pkg.ReferenceBank(pkg.ReferenceBankConfig(clustering_method="kmeans", feature_dim=64), engine=gpu_engine)
    one.add_references(V[:1])
    assert one.perform_clustering() is False                            # below 2 references
