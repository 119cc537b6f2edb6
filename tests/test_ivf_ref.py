"""CPU: the fp64 IVF reference of tests/ivf_ref.py against plain numpy, its ordering and padding rules on hand-made ties,
and the near-tie shares of every case tests/test_gpu_ivf.py runs -- the caps of the GPU tests (1 % of the probe's and 3 % of
the scan's (query, rank) entries may differ from the fp64 order) rest on these shares staying below 0.5 % and 1.5 %."""
import numpy as np
import pytest

import ivf_ref


def test_scan_all_lists_is_argsort():
    ix = ivf_ref.index_case(700, 128, 9, "unit", False)
    rng = np.random.default_rng(3)
    Q = rng.standard_normal((5, 128))
    probes = np.tile(np.arange(9), (5, 1))
    idx, sim, pos = ivf_ref.scan(Q, ix["X64"], probes, ix["offsets"], ix["ids"], 50)
    S = Q @ ix["X64"].T
    for q in range(5):
        o = np.argsort(-S[q], kind="stable")[:50]
        assert np.array_equal(pos[q], o)
        assert np.array_equal(idx[q], ix["ids"][o])
        assert np.allclose(sim[q], S[q, o], rtol=0, atol=1e-12)      # a row product and a matrix product round differently
    idx2, _, pos2 = ivf_ref.scan(Q, ix["X64"], probes, ix["offsets"], None, 50)
    assert np.array_equal(idx2, pos2) and np.array_equal(pos2, pos)


def test_scan_ties_padding_and_skips():
    X = np.array([[1.0, 0], [0, 1], [1, 0], [0.5, 0], [np.nan, 0], [1, 0]])
    offsets = np.array([0, 2, 2, 5, 6])                 # lists: {0, 1}, {}, {2, 3, 4}, {5}
    ids = np.array([40, 41, 7, 8, 9, 3])
    Q = np.array([[1.0, 0.0]])
    idx, sim, pos = ivf_ref.scan(Q, X, np.array([[0, 2, -1, 1]]), offsets, ids, 6)
    # equal similarities: the lower ORIGINAL id first; the NaN row never; the rest padded
    assert idx[0].tolist() == [7, 40, 8, 41, -1, -1]
    assert pos[0].tolist() == [2, 0, 3, 1, -1, -1]
    assert sim[0, :4].tolist() == [1.0, 1.0, 0.5, 0.0] and np.all(sim[0, 4:] == -np.inf)
    idx, sim, pos = ivf_ref.scan(Q, X, np.array([[-1, 1, 9, -5]]), offsets, ids, 2)      # nothing probed
    assert idx.tolist() == [[-1, -1]] and pos.tolist() == [[-1, -1]] and np.all(sim == -np.inf)


def test_probe_ties_nan_and_clamp():
    C = np.array([[1.0, 0], [1, 0], [np.nan, 0], [0, 1]])
    lists, score = ivf_ref.probe(np.array([[2.0, 0.1]]), C, 6)
    assert lists[0].tolist() == [0, 1, 3, -1, -1, -1]     # equal scores: the lower id; NaN never; nprobe > nlist: -1
    assert score[0, 0] == score[0, 1] == 1.5 and np.all(score[0, 3:] == -np.inf)


def test_search_finds_the_row_itself():
    c = ivf_ref.search_case(1000, 128, 70, 7, "unit", False)      # unit rows: a row's best inner product is with itself
    idx, sim, pos = ivf_ref.search(c["X64"][:50], c["X64"], c["C"].numpy(), c["offsets"], c["ids"], 1, 1)
    assert np.array_equal(pos[:, 0], np.arange(50))


@pytest.mark.parametrize("kind", ivf_ref.KINDS)
@pytest.mark.parametrize("M,nlist,D,nprobe", ivf_ref.PROBE_SHAPES)
def test_probe_near_ties(M, nlist, D, nprobe, kind):
    Q, C = ivf_ref.probe_case(M, nlist, D, kind)
    Q64, C64 = ivf_ref.operands(Q), C.double().numpy()
    _, score = ivf_ref.probe(Q64, C64, nprobe)
    cmax = np.linalg.norm(C64, axis=1).max()
    tau = 4e-6 * np.maximum(np.linalg.norm(Q64, axis=1), cmax) * cmax
    share = ivf_ref.near_tie_share(score, tau)
    print(f"probe {M, nlist, D, nprobe} {kind}: near-tie share {share:.4%}")
    assert share <= 0.005


def _scan_share(c, Q, probes, k):
    Q64 = ivf_ref.operands(Q)
    idx, sim, pos = ivf_ref.scan(Q64, c["X64"], probes, c["offsets"], c["ids"], k)
    xmax = np.linalg.norm(c["X64"], axis=1).max()
    return ivf_ref.near_tie_share(sim, 2e-6 * np.linalg.norm(Q64, axis=1) * xmax)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ivf_ref.KINDS)
@pytest.mark.parametrize("R,D,M,nlist,nprobe,k", ivf_ref.SEARCH_CASES)
def test_search_case_near_ties(R, D, M, nlist, nprobe, k, kind, bf16):
    c = ivf_ref.search_case(R, D, M, nlist, kind, bf16)
    lists, _ = ivf_ref.probe(ivf_ref.operands(c["Q"]), c["C"].double().numpy(), nprobe)
    share = _scan_share(c, c["Q"], lists, k)
    print(f"search {R, D, M, nlist, nprobe, k} {kind} {'bf16' if bf16 else 'f32'}: near-tie share {share:.4%}")
    assert share <= 0.015


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [128, 512, 768])
def test_edge_case_near_ties(D, bf16):
    c = ivf_ref.edge_case(D, bf16, True)
    # the planted pairs are exact ties on purpose: they are judged separately, by id order
    idx, sim, pos = ivf_ref.scan(ivf_ref.operands(c["Q"]), c["X64"], c["probes"], c["offsets"], c["ids"], 128)
    planted = {p for ab in c["dup"] for p in ab}
    keep = ~np.isin(pos, list(planted))
    sim = np.where(keep, sim, np.nan)
    tau = 2e-6 * np.linalg.norm(ivf_ref.operands(c["Q"]), axis=1) * np.linalg.norm(c["X64"], axis=1).max()
    share = ivf_ref.near_tie_share(sim, tau)
    print(f"edge D={D} {'bf16' if bf16 else 'f32'}: near-tie share {share:.4%}")
    assert share <= 0.015
    lengths = np.diff(c["offsets"])
    assert lengths[:9].tolist() == ivf_ref.EDGE_LENGTHS
    assert (c["probes"][:65] == 7).sum(1).tolist() == [1] * 65 and (c["probes"][65:98] == 8).sum(1).tolist() == [1] * 33
    for r in c["probes"]:                                 # a list is never named twice in a row
        v = r[r >= 0]
        assert len(set(v.tolist())) == len(v)
