"""GPU: the IVF kernels (tvc_ivf_probe / tvc_ivf_scan), ``TVCEngine.ivf_*`` and the retrievers' IVF configurations against
the fp64 reference of tests/ivf_ref.py.  The kernel tests use hand-made lists and centroids and never call k-means; only the
build, retriever and step tests go through ``ivf_build``.

Bounds.  Probe: tau_c = 4e-6 * max(|q|, max|c|) * max|c|, the k-means test's bound; at most 1 % of (query, rank) entries may
differ from the fp64 order.  Scan: tau = 2e-6 |q||x| for the two similarities of a comparison (the project's 1e-6 cosine
bound, tests/test_gpu_api.py), a returned similarity within 1e-6 |q||x| of fp64; at most 3 % of (query, rank) entries may
differ from the fp64 order (tests/test_ivf_ref.py keeps the reference's own near-tie shares of these inputs under 0.5 % and
1.5 %; a swap moves two entries)."""
import functools
import logging

import numpy as np
import pytest
import torch

import ivf_ref

pytestmark = pytest.mark.gpu
BANK = "ivf-test"
OFF = 1000                     # idx_offset of every scan here


def make_index(pkg, eng, c, max_list_rows=None, name=BANK):
    """Register the case's stored rows under ``name`` and describe them as an IVFIndex (no k-means)."""
    eng.set_bank(c["X"].to(eng.device), name=name)
    ids = None if c["ids"] is None else torch.from_numpy(c["ids"].astype(np.int32)).to(eng.device)
    return pkg.IVFIndex(name=name, nlist=len(c["offsets"]) - 1, centroids=c["C"].to(eng.device),
                        offsets=torch.from_numpy(np.asarray(c["offsets"]).astype(np.int32)).to(eng.device), ids=ids,
                        max_list_rows=max_list_rows or c["max_list_rows"], rows=c["X"].shape[0], dim=c["X"].shape[1])


def check_scan(c, Q, probes, k, got, ref, label, off=OFF):
    """The rules of the scan for one result (idx, sim, pos) against the fp64 result ``ref`` of the same probes."""
    idx, sim, pos = (t.cpu().numpy() for t in got)
    ridx, rsim, rpos = (a[:, :k] for a in ref)
    Q64, X64 = ivf_ref.operands(Q), c["X64"]
    qn, xn = np.linalg.norm(Q64, axis=1), np.linalg.norm(X64, axis=1)
    offsets, nlist = np.asarray(c["offsets"]), len(c["offsets"]) - 1
    ids = np.arange(len(X64)) if c["ids"] is None else c["ids"]
    assert idx.shape == sim.shape == pos.shape == (len(Q64), k) and idx.dtype == np.int32 and pos.dtype == np.int32
    worst_def, worst_err, differ, entries = 0.0, 0.0, 0, 0
    for q in range(len(Q64)):
        n = int((ridx[q] >= 0).sum())
        assert (idx[q, n:] == -1).all() and (pos[q, n:] == -1).all() and (sim[q, n:] == -np.inf).all(), f"{label}: padding of query {q}"
        assert (pos[q, :n] >= 0).all() and len(set(idx[q, :n].tolist())) == n, f"{label}: query {q} returns an id twice or too few"
        p = pos[q, :n].astype(np.int64)
        assert np.array_equal(ids[p] + off, idx[q, :n]), f"{label}: pos does not map to idx"
        lists = np.searchsorted(offsets, p, side="right") - 1
        probed = set(int(l) for l in probes[q] if 0 <= l < nlist)
        assert set(lists.tolist()) <= probed, f"{label}: query {q} returns rows of lists it did not probe"
        if n == 0:
            continue
        s64 = X64[p] @ Q64[q]
        tau = 2e-6 * qn[q] * np.maximum(xn[p], xn[rpos[q, :n]])
        worst_def = max(worst_def, float(((rsim[q, :n] - s64) / tau).max()))
        worst_err = max(worst_err, float((np.abs(sim[q, :n] - s64) / (1e-6 * qn[q] * xn[p])).max()))
        differ += int((idx[q, :n] != ridx[q, :n] + off).sum())
        entries += n
    share = differ / max(1, entries)
    print(f"{label}: deficit {worst_def:.3f} tau, sim err {worst_err:.3f} of 1e-6|q||x|, entries differing {share:.4%} of {entries}")
    assert worst_def <= 1.0
    assert worst_err <= 1.0
    assert share <= 0.03
    return share


# ---- probe --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ivf_ref.KINDS)
@pytest.mark.parametrize("M,nlist,D,nprobe", ivf_ref.PROBE_SHAPES)
def test_probe_against_fp64(gpu_engine, M, nlist, D, nprobe, kind):
    Q, C = ivf_ref.probe_case(M, nlist, D, kind)
    lists, score = (t.cpu().numpy() for t in gpu_engine.ivf_probe(Q.to(gpu_engine.device), C.to(gpu_engine.device), nprobe))
    Q64, C64 = ivf_ref.operands(Q), C.double().numpy()
    S = ivf_ref.probe_scores(Q64, C64)
    want, want_score = ivf_ref.probe(Q64, C64, nprobe)
    cmax = np.linalg.norm(C64, axis=1).max()
    tau = (4e-6 * np.maximum(np.linalg.norm(Q64, axis=1), cmax) * cmax)[:, None]
    assert lists.shape == (M, nprobe) and lists.dtype == np.int32 and (lists >= 0).all() and (lists < nlist).all()
    assert all(len(set(r.tolist())) == nprobe for r in lists)
    chosen = np.take_along_axis(S, lists.astype(np.int64), 1)
    deficit = ((want_score - chosen) / tau).max()
    e_score = (np.abs(score - chosen) / tau).max()
    differ = float((lists != want).mean())
    print(f"probe {M, nlist, D, nprobe} {kind}: deficit {deficit:.3f} tau_c, score err {e_score:.3f} tau_c, entries differing {differ:.4%}")
    assert deficit <= 1.0
    assert e_score <= 1.0
    assert differ <= 0.01


def test_probe_planted_tie_nan_and_clamp(gpu_engine):
    Q, C = ivf_ref.probe_case(65, 257, 128, "blobs")
    C = C[:9].clone()
    C[3] = C[1]                                   # two identical centroids: the lower id ranks first
    C[2, 5] = float("nan")                        # a NaN centroid is never returned
    lists, score = (t.cpu().numpy() for t in gpu_engine.ivf_probe(Q.to(gpu_engine.device), C.to(gpu_engine.device), 12))
    want, _ = ivf_ref.probe(ivf_ref.operands(Q), C.double().numpy(), 12)
    for q in range(len(lists)):
        r = lists[q].tolist()
        assert 2 not in r and r[8:] == [-1] * 4 and sorted(r[:8]) == [0, 1, 3, 4, 5, 6, 7, 8]     # nprobe clamped to the 8 real lists
        assert r.index(3) == r.index(1) + 1 and score[q, r.index(3)] == score[q, r.index(1)]
        assert (score[q, 8:] == -np.inf).all()
    assert float((lists != want).mean()) <= 0.01


# ---- scan ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_ref(D, bf16, shuffled):
    c = ivf_ref.edge_case(D, bf16, shuffled)
    return ivf_ref.scan(ivf_ref.operands(c["Q"]), c["X64"], c["probes"], c["offsets"], c["ids"], 128)


@pytest.mark.parametrize("shuffled", [True, False], ids=["ids", "noids"])
@pytest.mark.parametrize("k", [1, 20, 128])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [128, 512, 768])
def test_scan_edges_against_fp64(pkg, gpu_engine, D, bf16, k, shuffled):
    c = ivf_ref.edge_case(D, bf16, shuffled)
    eng = gpu_engine
    try:
        ix = make_index(pkg, eng, c)
        got = eng.ivf_scan(c["Q"].to(eng.device), k, torch.from_numpy(c["probes"].astype(np.int32)).to(eng.device), ix, idx_offset=OFF)
        eng.bank_status()
    finally:
        eng.release_bank(BANK)
    check_scan(c, c["Q"], c["probes"], k, got, edge_ref(D, bf16, shuffled), f"edges D={D} {'bf16' if bf16 else 'f32'} k={k} {'ids' if shuffled else 'noids'}")
    idx, sim, pos = (t.cpu().numpy() for t in got)
    n_empty = 65 + 33
    assert (idx[n_empty] == -1).all()                                            # the row of all -1
    assert int((idx[-1] >= 0).sum()) == min(k, 16)                               # 16 rows probed in all
    # planted ties: the same row stored in lists 6 and 7, both probed: bit-equal similarities, the lower original id first
    ids = np.arange(len(c["X64"])) if c["ids"] is None else c["ids"]
    for q, (a, b) in zip(c["dup_q"], c["dup"]):
        lo, hi = sorted((int(ids[a]), int(ids[b])))
        assert idx[q, 0] == lo + OFF
        if k > 1:
            assert idx[q, 1] == hi + OFF and sim[q, 0] == sim[q, 1]


NO_LDS_MAX_LIST_ROWS = 4097     # 8 probes x pitch 4112 = 32 896 floats > IVF_SELECT_LDS_FLOATS (tests/test_ivf_host.py: select_lds == 0)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_scan_select_without_lds(pkg, gpu_engine, bf16):
    """The select pass reading its segments from global memory: the edge index's first three queries (lists 6 and 7 with the
    planted ties) under a declared maximum so large that nprobe x pitch no longer fits the select's LDS.  Every other scan
    here stays below that size."""
    c = ivf_ref.edge_case(128, bf16, True)
    assert _select_floats(NO_LDS_MAX_LIST_ROWS) > 32768 >= _select_floats(c["max_list_rows"])
    eng, k = gpu_engine, 20
    Q, probes = c["Q"][:3].contiguous(), c["probes"][:3]
    try:
        ix = make_index(pkg, eng, c, max_list_rows=NO_LDS_MAX_LIST_ROWS)
        got = eng.ivf_scan(Q.to(eng.device), k, torch.from_numpy(probes.astype(np.int32)).to(eng.device), ix, idx_offset=OFF)
        eng.bank_status()
    finally:
        eng.release_bank(BANK)
    ref = tuple(a[:3] for a in edge_ref(128, bf16, True))
    check_scan(c, Q, probes, k, got, ref, f"select without LDS {'bf16' if bf16 else 'f32'}")
    idx, sim, _ = (t.cpu().numpy() for t in got)
    for q, (a, b) in zip(range(3), c["dup"]):
        lo, hi = sorted((int(c["ids"][a]), int(c["ids"][b])))
        assert idx[q, 0] == lo + OFF and idx[q, 1] == hi + OFF and sim[q, 0] == sim[q, 1]


def _select_floats(max_list_rows):
    return ivf_ref.EDGE_NPROBE * ((max_list_rows + 15) // 16 * 16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_declared_maximum_too_small(pkg, gpu_engine, bf16):
    c = ivf_ref.edge_case(128, bf16, True)
    eng = gpu_engine
    Q, probes = c["Q"].to(eng.device), torch.from_numpy(c["probes"].astype(np.int32)).to(eng.device)
    try:
        ix = make_index(pkg, eng, c, max_list_rows=599)          # the longest probed list has 600 rows
        eng.ivf_scan(Q, 20, probes, ix)
        with pytest.raises(pkg.TVCError) as e:
            eng.bank_status()
        assert e.value.code == pkg._lib.TVC_E_OVERFLOW
        ix = make_index(pkg, eng, c, max_list_rows=600)
        eng.ivf_scan(Q, 20, probes, ix)
        eng.bank_status()
    finally:
        eng.release_bank(BANK)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("R,D,M,nlist,k", [(3000, 128, 130, 40, 20), (2000, 768, 33, 12, 128)])
def test_all_lists_probed_is_the_exact_search(pkg, gpu_engine, R, D, M, nlist, k, bf16):
    """Unit rows: the 2e-6 between the two searches' similarities is a bound on cosines (twice the project's 1e-6)."""
    kind = "unit"
    c = ivf_ref.search_case(R, D, M, nlist, kind, bf16)
    eng = gpu_engine
    Q = c["Q"].to(eng.device)
    try:
        ix = make_index(pkg, eng, c)
        got = eng.ivf_search(Q, k, nlist, ix, idx_offset=OFF)
        eng.bank_status()
        eng.set_bank(c["X"].to(eng.device), name=BANK + "-flat")
        fidx, fsim, _ = eng.bank_search_robust(Q, k, want_moments=False, bank=BANK + "-flat")
    finally:
        eng.release_bank(BANK)
        eng.release_bank(BANK + "-flat")
    probes = np.tile(np.arange(nlist), (M, 1))
    ref = ivf_ref.scan(ivf_ref.operands(c["Q"]), c["X64"], probes, c["offsets"], c["ids"], k)
    check_scan(c, c["Q"], probes, k, got, ref, f"all lists {kind} {'bf16' if bf16 else 'f32'}")
    # the flat search returns stored positions (its bank is the list-ordered rows): map them to original ids
    fidx, fsim = fidx.cpu().numpy(), fsim.cpu().numpy()
    flat_ids = np.where(fidx >= 0, c["ids"][np.maximum(fidx, 0)] + OFF, -1)
    idx, sim, _ = (t.cpu().numpy() for t in got)
    err = float(np.abs(sim - fsim).max())
    differ = float((idx != flat_ids).mean())
    print(f"all lists {kind} {'bf16' if bf16 else 'f32'}: |sim - flat| max {err:.3g}, entries differing from the flat search {differ:.4%}")
    assert err <= 2e-6
    assert differ <= 0.03


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ivf_ref.KINDS)
@pytest.mark.parametrize("R,D,M,nlist,nprobe,k", ivf_ref.SEARCH_CASES)
def test_search_against_fp64_with_own_probes(pkg, gpu_engine, R, D, M, nlist, nprobe, k, kind, bf16):
    c = ivf_ref.search_case(R, D, M, nlist, kind, bf16)
    eng = gpu_engine
    Q = c["Q"].to(eng.device)
    try:
        ix = make_index(pkg, eng, c)
        lists, _ = eng.ivf_probe(Q, ix.centroids, nprobe)
        got = eng.ivf_search(Q, k, nprobe, ix, idx_offset=OFF)
        eng.bank_status()
    finally:
        eng.release_bank(BANK)
    probes = lists.cpu().numpy()
    ref = ivf_ref.scan(ivf_ref.operands(c["Q"]), c["X64"], probes, c["offsets"], c["ids"], k)
    check_scan(c, c["Q"], probes, k, got, ref, f"search {R, D, M, nlist, nprobe, k} {kind} {'bf16' if bf16 else 'f32'}")


# ---- build (k-means) ----------------------------------------------------------------------------------------------
def unit_blobs(R, nlist, D, seed):
    """Blobs, L2-normalised: the rows the retrievers hold (on unit rows a row's best inner product is with itself)."""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((nlist, D))
    X = C[rng.integers(0, nlist, R)] + 0.3 * rng.standard_normal((R, D))
    return torch.from_numpy((X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32))


def test_build(pkg, gpu_engine):
    R, nlist, D = 4096, 64, 128
    eng = gpu_engine
    X = unit_blobs(R, nlist, D, 5)
    Xd = X.to(eng.device)
    try:
        a = eng.ivf_build(Xd, nlist, BANK)
        snap = (a.centroids.clone(), a.offsets.clone(), a.ids.clone(), a.max_list_rows)
        eng.ivf_release(a)
        b = eng.ivf_build(Xd, nlist, BANK)
        assert torch.equal(snap[0], b.centroids) and torch.equal(snap[1], b.offsets) and torch.equal(snap[2], b.ids)
        assert snap[3] == b.max_list_rows and b.rows == R and b.dim == D and b.nlist == nlist and eng.bank_size(BANK) == R
        offsets, ids, C = b.offsets.cpu().numpy().astype(np.int64), b.ids.cpu().numpy().astype(np.int64), b.centroids.cpu()
        assert offsets[0] == 0 and offsets[-1] == R and (np.diff(offsets) >= 0).all()
        assert np.array_equal(np.sort(ids), np.arange(R))
        assert all((np.diff(ids[offsets[l]:offsets[l + 1]]) > 0).all() for l in range(nlist))
        assert b.max_list_rows == int(np.diff(offsets).max())
        # every stored row sits in the list the probe rule ranks first for it
        X64, C64 = ivf_ref.operands(X), C.double().numpy()
        S = ivf_ref.probe_scores(X64, C64)
        cmax = np.linalg.norm(C64, axis=1).max()
        tau = 4e-6 * np.maximum(np.linalg.norm(X64, axis=1), cmax) * cmax
        label = np.empty(R, np.int64)
        label[ids] = np.repeat(np.arange(nlist), np.diff(offsets))
        deficit = float(((S.max(1) - S[np.arange(R), label]) / tau).max())
        assert deficit <= 1.0
        # self-retrieval with one probe, except rows whose two best list scores are within tau_c
        top2 = np.sort(S, axis=1)[:, -2:]
        close = (top2[:, 1] - top2[:, 0]) <= tau
        idx, sim, pos = eng.ivf_search(Xd, 1, 1, b)
        eng.bank_status()
        hit = idx[:, 0].cpu().numpy() == np.arange(R)
        assert hit[~close].all() and close.mean() <= 0.01
        # recall@10 against the flat search: information, not a bar
        eng.set_bank(Xd, name=BANK + "-flat")
        fidx, _, _ = eng.bank_search_robust(Xd[:512], 10, want_moments=False, bank=BANK + "-flat")
        fidx = fidx.cpu().numpy()
        rec = {}
        for nprobe in (1, 8):
            got = eng.ivf_search(Xd[:512], 10, nprobe, b)[0].cpu().numpy()
            rec[nprobe] = float(np.mean([len(set(g.tolist()) & set(f.tolist())) / 10 for g, f in zip(got, fidx)]))
        print(f"build R={R} nlist={nlist} D={D}: list deficit {deficit:.3f} tau_c, rows with near-tied lists {close.mean():.4%}, "
              f"max_list_rows {b.max_list_rows}, recall@10 nprobe 1: {rec[1]:.4f}, nprobe 8: {rec[8]:.4f}")
    finally:
        eng.release_bank(BANK)
        eng.release_bank(BANK + "-flat")


# ---- retrievers and the step --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip(pkg):
    m = pkg.CLIPModel(pkg.CLIPConfig(model_name="ViT-T/16-test", device="cuda"))
    yield m
    m.engine.close()


class Calls:
    """Counts the engine's IVF entry points for the duration of a ``with``."""
    NAMES = ("ivf_build", "ivf_probe", "ivf_scan", "ivf_search")

    def __init__(self, eng):
        self.eng, self.n = eng, {n: 0 for n in self.NAMES}

    def __enter__(self):
        for name in self.NAMES:
            fn = getattr(self.eng, name)

            def wrapped(*a, _fn=fn, _name=name, **kw):
                self.n[_name] += 1
                return _fn(*a, **kw)
            setattr(self.eng, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name in self.NAMES:
            delattr(self.eng, name)


TEXTS = ["a cat on a sofa", "two dogs playing in the park", "a red car", "an old man reading a newspaper"]


def test_retrievers_ivf_equals_flat(pkg, clip):
    feats = unit_blobs(2000, 16, 128, 9)
    q = clip.encode_text(TEXTS)
    feats[7], feats[900] = q[0], q[1]
    paths = [f"img_{i}.jpg" for i in range(2000)]
    meta = [{"id": i} for i in range(2000)]
    with Calls(clip.engine) as calls:
        flat = pkg.MultiModalRetriever(pkg.RetrievalConfig(clip_model="ViT-T/16-test", bank_dtype="float32"), clip_model=clip)
        flat.set_image_features(feats, paths)
        want = flat.batch_retrieve_images_by_texts(TEXTS, top_k=10)
        gflat = pkg.RetrievalReferenceGenerator(clip, features=feats, metadata=meta)
        gwant = gflat.retrieve_references_batch(TEXTS)
        assert calls.n == {n: 0 for n in Calls.NAMES}                # the default configs never touch the IVF path
        ivf = pkg.MultiModalRetriever(pkg.RetrievalConfig(clip_model="ViT-T/16-test", bank_dtype="float32",
                                                          faiss_index_type="IndexIVFFlat", n_clusters=16, nprobe=16), clip_model=clip)
        ivf.set_image_features(feats, paths)
        got = ivf.batch_retrieve_images_by_texts(TEXTS, top_k=10)
        givf = pkg.RetrievalReferenceGenerator(clip, features=feats, metadata=meta,
                                               config=pkg.RetrievalRefConfig(faiss_index_type="IVF", nlist=16, nprobe=16))
        ggot = givf.retrieve_references_batch(TEXTS)
        assert calls.n["ivf_build"] == 2 and calls.n["ivf_search"] == 2
    for (gp, gs), (wp, ws) in zip(got, want):
        assert gp == wp
        np.testing.assert_allclose(gs, ws, atol=2e-6, rtol=0)
    for g, w in zip(ggot, gwant):
        assert [r["index"] for r in g] == [r["index"] for r in w] and [r["metadata"] for r in g] == [r["metadata"] for r in w]
        np.testing.assert_allclose([r["similarity"] for r in g], [r["similarity"] for r in w], atol=2e-6, rtol=0)
        for a, b in zip(g, w):
            np.testing.assert_array_equal(a["features"], b["features"])
    assert len(ggot[0]) > 0 and ggot[0][0]["index"] == 7


def test_hnsw_and_uncovered_width_fall_back(pkg, clip, caplog):
    feats = unit_blobs(300, 4, 128, 2)
    with Calls(clip.engine) as calls, caplog.at_level(logging.WARNING):
        r = pkg.MultiModalRetriever(pkg.RetrievalConfig(clip_model="ViT-T/16-test", faiss_index_type="IndexHNSWFlat"), clip_model=clip)
        r.set_image_features(feats)
        g = pkg.RetrievalReferenceGenerator(clip, features=unit_blobs(300, 4, 64, 2), config=pkg.RetrievalRefConfig(faiss_index_type="IVF"))
        assert calls.n["ivf_build"] == 0 and r._ivf is None and g._ivf is None
    assert len(r.batch_retrieve_images_by_features(feats[:2].cuda(), top_k=3)[0][0]) == 3


def test_detect_embeddings_with_index(pkg, gpu_engine):
    eng = gpu_engine
    B, N1, D = 6, 5, 128
    bank = unit_blobs(2000, 16, D, 21)
    rng = torch.Generator().manual_seed(4)
    txt = torch.nn.functional.normalize(bank[torch.randint(0, 2000, (B * N1,), generator=rng)] + 0.05 * torch.randn((B * N1, D), generator=rng), dim=-1)
    img = torch.nn.functional.normalize(torch.randn((B, D), generator=rng), dim=-1)
    cfg = pkg.ConsistencyConfig()
    try:
        eng.set_bank(bank.to(eng.device), name=BANK + "-flat")
        want = eng.detect_embeddings(img.to(eng.device), txt.view(B, N1, D).to(eng.device), cfg, robust=True, bank=BANK + "-flat")
        ix = eng.ivf_build(bank.to(eng.device), 16, BANK)
        got = eng.detect_embeddings(img.to(eng.device), txt.view(B, N1, D).to(eng.device), cfg, ivf=ix, nprobe=16)
        eng.bank_status()
    finally:
        eng.release_bank(BANK)
        eng.release_bank(BANK + "-flat")
    # the records' existing tolerance (1e-4: tests/test_gpu_configs.py, tests/test_gpu_fp16_mode.py)
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), atol=1e-4, rtol=0)
