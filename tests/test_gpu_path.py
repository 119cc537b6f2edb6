"""GPU parity of the hot path proper, through the C-ABI, against the CPU oracle
(``oracle/``) on the same seeded inputs: bank search (K5), consistency
(K4/K6/K7, both polarities), CLIP towers (K1/K2/K3)."""
import numpy as np
import pytest
import torch

from oracle import clip_oracle, tvc_oracle

pytestmark = pytest.mark.gpu


def _unit(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    return x / x.norm(dim=-1, keepdim=True)


def _check_topk(idx, sim, S, k, tol, order=None):
    """idx/sim: GPU result [M, k]; S: exact fp64 similarity matrix [M, R]; order: the stable descending argsort of S's
    rows (its first min(k, R) columns), for callers that check several results against one S."""
    M, R = S.shape
    kk = min(k, R)
    if order is None:
        order = np.argsort(-S, axis=1, kind="stable")
    order = order[:, :kk]
    ref_sim = np.take_along_axis(S, order, 1)
    assert np.abs(sim[:, :kk] - ref_sim).max() < tol
    if kk < k:
        assert (idx[:, kk:] == -1).all()
    # every returned index must carry the similarity reported for it, be unique, and be in the
    # true top-k unless it ties with the k-th value within tol
    for m in range(M):
        got = idx[m, :kk]
        assert len(set(got.tolist())) == kk
        assert np.abs(S[m, got] - sim[m, :kk]).max() < tol
        kth = ref_sim[m, -1]
        assert (S[m, got] >= kth - tol).all()
        assert (np.diff(sim[m, :kk]) <= 0).all()


@pytest.mark.parametrize("R,M,D,k,dtype", [
    (20, 3, 512, 10, torch.float32),       # the reference's own fixture shape (cache/ref_bank)
    (1000, 48, 512, 5, torch.bfloat16),    # BASELINE configs[0]
    (5000, 300, 128, 20, torch.bfloat16),
    (70001, 70, 768, 20, torch.bfloat16),  # ragged last tile, several chunks
    (3, 5, 128, 5, torch.bfloat16),        # R < k
    (4097, 257, 256, 32, torch.float32),   # fp32 bank (3-product split), ragged M
])
def test_bank_search(gpu_engine, R, M, D, k, dtype):
    bank = _unit((R, D), 100 + R).to(dtype)
    q = _unit((M, D), 200 + M)
    gpu_engine.set_bank(bank.cuda())
    idx, sim, mom = gpu_engine.bank_search(q.cuda(), k, count_thr=0.05)
    gpu_engine.bank_status()
    S = (q.double() @ bank.double().t()).numpy()
    # split-bf16 queries x exact bf16 bank, fp32 accumulate: 1e-5 abs (bar 1e-4, fp32-bank bar 1e-6 relaxed to 1e-5)
    _check_topk(idx.cpu().numpy(), sim.cpu().numpy().astype(np.float64), S, k, 1e-5)
    mom = mom.cpu().numpy().astype(np.float64)
    assert np.abs(mom[:, 0] - S.sum(1)).max() < 1e-3 * max(1.0, np.sqrt(R))
    assert np.abs(mom[:, 1] - (S * S).sum(1)).max() < 1e-3 * max(1.0, R / D)
    assert np.abs(mom[:, 2] - S.max(1)).max() < 1e-5
    near = np.abs(S - 0.05) < 1e-5
    cnt = (S >= 0.05).sum(1)
    assert (np.abs(mom[:, 3] - cnt) <= near.sum(1)).all()


# (tests/test_gemm_form.py::test_bank_plan_of_the_blocked_item_order_shapes pins what these two shapes reach)
@pytest.mark.parametrize("R,M,D,k,dtype", [(4000, 770, 64, 5, torch.float32), (90001, 770, 64, 5, torch.bfloat16)])
def test_bank_search_blocked_item_order(gpu_engine, R, M, D, k, dtype):
    """M = 770 is four query tiles and bank_plan cuts these banks into 16 / 176 chunks, so the (query tile, chunk) items
    of pass 1 take the blocked order (4 query tiles x 8 chunks; bank.hip, bank_item) that otherwise only the workload's own
    sizes reach -- with a ragged last bank tile, a ragged fourth query tile, one and two bank tiles per chunk.  With moments
    (all products, bank_search_kernel<false>) and without (the ring filter); ~16 / ~256 rows per query pass the filter."""
    bank = _unit((R, D), 100 + R).to(dtype)
    q = _unit((M, D), 200 + M)
    gpu_engine.set_bank(bank.cuda())
    S = (q.double().cuda() @ bank.double().cuda().t()).cpu().numpy()       # the reference, once for both searches
    order = np.argsort(-S, axis=1, kind="stable")[:, :k]
    idx, sim, mom = gpu_engine.bank_search(q.cuda(), k, count_thr=0.05)
    gpu_engine.bank_status()
    _check_topk(idx.cpu().numpy(), sim.cpu().numpy().astype(np.float64), S, k, 1e-5, order)
    mom = mom.cpu().numpy().astype(np.float64)
    assert np.abs(mom[:, 0] - S.sum(1)).max() < 1e-3 * max(1.0, np.sqrt(R))
    assert np.abs(mom[:, 1] - (S * S).sum(1)).max() < 1e-3 * max(1.0, R / D)
    assert np.abs(mom[:, 2] - S.max(1)).max() < 1e-5
    near = np.abs(S - 0.05) < 1e-5
    cnt = (S >= 0.05).sum(1)
    assert (np.abs(mom[:, 3] - cnt) <= near.sum(1)).all()
    idx, sim, mom = gpu_engine.bank_search(q.cuda(), k, want_moments=False)
    gpu_engine.bank_status()
    assert mom is None
    _check_topk(idx.cpu().numpy(), sim.cpu().numpy().astype(np.float64), S, k, 1e-5, order)


@pytest.mark.parametrize("R,M,D,k,dtype,scale", [
    (20, 3, 512, 10, torch.float32, 1.0),
    (1000, 48, 512, 5, torch.bfloat16, 1.0),
    (70001, 70, 768, 20, torch.bfloat16, 1.0),
    (3, 5, 128, 5, torch.bfloat16, 1.0),
    (4097, 257, 256, 32, torch.float32, 1.0),
    (30000, 300, 512, 5, torch.float32, 3.7),    # un-normalised bank rows: the margin scales with the row norms
    (200000, 64, 768, 5, torch.bfloat16, 1.0),
])
def test_bank_search_filter_form(gpu_engine, pkg, R, M, D, k, dtype, scale):
    """No moments requested -> one-product filter + fp32 re-scoring (tvc.h TVC_OPT_BANK_FILTER):
    same top-k as the exact fp64 product, and the same index sets as the all-products pass."""
    bank = (_unit((R, D), 100 + R) * scale).to(dtype)
    q = _unit((M, D), 200 + M)
    gpu_engine.set_bank(bank.cuda())
    idx, sim, mom = gpu_engine.bank_search(q.cuda(), k, want_moments=False)
    gpu_engine.bank_status()
    assert mom is None
    S = (q.double() @ bank.double().t()).numpy()
    _check_topk(idx.cpu().numpy(), sim.cpu().numpy().astype(np.float64), S, k, 1e-5 * scale)
    try:
        gpu_engine.set_option(pkg._lib.TVC_OPT_BANK_FILTER, 0)
        idx2, sim2, _ = gpu_engine.bank_search(q.cuda(), k, want_moments=False)
        gpu_engine.bank_status()
    finally:
        gpu_engine.set_option(pkg._lib.TVC_OPT_BANK_FILTER, 1)
    valid = idx >= 0
    assert (valid == (idx2 >= 0)).all()
    assert (sim[valid] - sim2[valid]).abs().max().item() < 2e-6 * scale
    same = (idx == idx2).all(dim=1)
    # rows may differ only where neighbouring similarities tie within the fp32 rounding of the two sums
    for m in (~same).nonzero().flatten().tolist():
        assert sorted(idx[m].tolist()) == sorted(idx2[m].tolist()) or \
            np.abs(np.diff(np.sort(S[m])[::-1][:k + 1])).min() < 2e-6 * scale


@pytest.mark.parametrize("R,D,dtype", [(1, 128, torch.bfloat16), (17, 512, torch.bfloat16), (1000, 512, torch.bfloat16),
                                       (70001, 768, torch.bfloat16), (300000, 768, torch.bfloat16), (4097, 128, torch.float32),
                                       (50000, 768, torch.float32)])
def test_bank_search_small_query_batches_skinny_form(gpu_engine, R, D, dtype):
    """M <= 64 (the reference searches one query at a time, src/retrieval.py:636-680; configs[0]: 48 rows): the filter pass
    streams the bank once against 16 / 32 / 48 / 64 query columns (bank.hip, bank_filter_skinny_kernel).  Exact against
    fp64, and IDENTICAL (indices and re-scored values) to the same rows searched inside a 65-row batch, which takes the
    256-query-tile kernels."""
    k = 7
    bank = _unit((R, D), 300 + R).to(dtype)
    gpu_engine.set_bank(bank.cuda())
    qall = _unit((65, D), 400 + D)
    big_i, big_s, _ = gpu_engine.bank_search(qall.cuda(), k, want_moments=False)
    gpu_engine.bank_status()
    for M in (1, 10, 16, 17, 32, 33, 48, 64):
        q = qall[:M]
        idx, sim, _ = gpu_engine.bank_search(q.cuda(), k, want_moments=False)
        gpu_engine.bank_status()
        S = (q.double() @ bank.double().t()).numpy()
        _check_topk(idx.cpu().numpy(), sim.cpu().numpy().astype(np.float64), S, k, 1e-5)
        assert torch.equal(idx, big_i[:M]) and torch.equal(sim, big_s[:M]), (R, D, M)
    # a NaN query row stays contained: never listed, the other rows unchanged (a NaN BANK row turns the filter's margin NaN,
    # everything is listed, the status reports the overflow: test_bank_search_nan_rows_and_ragged_query_tile, 64 rows)
    if R >= 1000:
        qb = qall[:10].clone(); qb[3, 5] = float("nan")
        i2, s2, _ = gpu_engine.bank_search(qb.cuda(), k, want_moments=False)
        gpu_engine.bank_status()
        assert (i2[3] == -1).all()
        ok = [m for m in range(10) if m != 3]
        assert torch.equal(i2[ok], big_i[ok]) and torch.equal(s2[ok], big_s[ok])


def test_bank_search_ties_and_duplicates(gpu_engine):
    """Duplicate rows: equal similarities must come back ordered by index."""
    D = 128
    base = _unit((50, D), 1)
    bank = torch.cat([base, base, base], 0).to(torch.bfloat16)     # every row three times
    q = base[:7].clone()
    gpu_engine.set_bank(bank.cuda())
    idx, sim, _ = gpu_engine.bank_search(q.cuda(), 6, want_moments=False)
    gpu_engine.bank_status()
    idx = idx.cpu().numpy()
    sim = sim.cpu().numpy()
    for m in range(7):
        assert idx[m, :3].tolist() == [m, m + 50, m + 100]
        assert sim[m, 0] == sim[m, 1] == sim[m, 2]


def test_bank_search_empty_bank(gpu_engine):
    gpu_engine.set_bank(torch.empty((0, 128), dtype=torch.bfloat16, device="cuda:0"))
    idx, sim, mom = gpu_engine.bank_search(_unit((4, 128), 3).cuda(), 5)
    assert (idx.cpu() == -1).all()


def test_bank_search_dense_fallback(gpu_engine, pkg):
    """Brute-force path: same contract as the fused search, on a normal bank (must agree) and on
    a degenerate one (40 000 identical rows + a few distinct ones) through bank_search_robust."""
    D = 128
    bank = _unit((3000, D), 41).to(torch.bfloat16).cuda()
    q = _unit((70, D), 42).cuda()
    gpu_engine.set_bank(bank)
    i1, s1, m1 = gpu_engine.bank_search(q, 7, 0.05)
    gpu_engine.bank_status()
    i2, s2, m2 = gpu_engine.bank_search_dense(q, 7, 0.05)
    assert torch.equal(i1, i2) and torch.equal(s1, s2)
    assert torch.allclose(m1, m2, rtol=1e-4, atol=1e-3)
    row = _unit((1, D), 5)
    degenerate = torch.cat([row.repeat(40000, 1), _unit((50, D), 6)]).to(torch.bfloat16).cuda()
    gpu_engine.set_bank(degenerate)
    qq = (row + 0.01 * _unit((3, D), 7)).cuda()
    qq = qq / qq.norm(dim=-1, keepdim=True)
    idx, sim, _ = gpu_engine.bank_search_robust(qq, 5)
    assert idx.cpu().tolist() == [[0, 1, 2, 3, 4]] * 3            # ties -> ascending index
    S = qq.double() @ degenerate.double().t()
    assert (sim.double() - S[:, :5]).abs().max().item() < 1e-5


def _stored64(bank):
    """fp64 values of bank rows as the kernels hold them: the bf16 values, or hi + lo of an fp32 row's bf16 planes."""
    if bank.dtype == torch.bfloat16:
        return bank.double().numpy()
    hi = bank.bfloat16().float()
    return (hi.double() + (bank - hi).bfloat16().double()).numpy()


def _dense(eng, q, k, count_thr, moments):
    idx, sim, mom = eng.bank_search_dense(q, k, count_thr, 0, moments)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sim.cpu().numpy(), None if mom is None else mom.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_bank_search_dense_degenerate_rows(gpu_engine, dtype):
    """row_topk_kernel's contract on the rows that decide its order and its admission rule: one row stored three times
    (bit-equal similarities -> ascending index), an all-NaN row (never returned), 20 rows of zeros and a zero query (every
    similarity ties at 0), and k larger than the number of admissible rows (the ranks beyond are exactly -1 / -inf).
    Bounds: the dense-fallback test's 1e-5 on similarities and rtol 1e-4 / atol 1e-3 on the moments, against fp64 products
    of the stored values (R = 100 with k = 128 runs through the dense GEMM as it is: no larger slice needed)."""
    R, D, M, NAN_ROW, DUP = 300, 128, 5, 41, (17, 60, 93)
    bank = _unit((R, D), 51)
    for j in DUP[1:]:
        bank[j] = bank[DUP[0]]
    bank[70:80] = 0.0
    bank[200:210] = 0.0
    clean = bank.to(dtype)                                # NaN-free: the moment assertions
    bank = clean.clone()
    bank[NAN_ROW] = float("nan")
    q = _unit((M, D), 52)
    q[1] = 0.0                                            # the zero query
    q[2] = _unit((1, D), 53)[0] * 0.1 + clean[DUP[0]].float()
    q[2] /= q[2].norm()                                   # aimed at the row stored three times
    qd = q.cuda()
    for rows, k in ((R, 7), (100, 128)):
        gpu_engine.set_bank(bank[:rows].contiguous().cuda())
        idx, sim, _ = _dense(gpu_engine, qd, k, 0.05, False)
        S = q.double().numpy() @ _stored64(bank[:rows]).T
        n_ok = min(k, rows - 1)                           # every row but the NaN row is admissible
        assert k == 7 or k - n_ok >= 28
        assert (idx[:, n_ok:] == -1).all() and (sim[:, n_ok:] == -np.inf).all()
        assert (idx[:, :n_ok] >= 0).all() and (idx[:, :n_ok] < rows).all() and not (idx == NAN_ROW).any()
        Sok = np.where(np.isnan(S), -np.inf, S)
        want = -np.sort(-Sok, axis=1)[:, :n_ok]
        for m in range(M):
            got = idx[m, :n_ok]
            assert len(set(got.tolist())) == n_ok
            assert (np.diff(sim[m, :n_ok]) <= 0).all()
            ties = np.diff(sim[m, :n_ok]) == 0
            assert (np.diff(got)[ties] > 0).all()         # equal similarities: ascending index
            assert np.abs(sim[m, :n_ok] - S[m, got]).max() < 1e-5 and np.abs(sim[m, :n_ok] - want[m]).max() < 1e-5
        assert idx[1, :n_ok].tolist() == [i for i in range(rows) if i != NAN_ROW][:n_ok] and (sim[1, :n_ok] == 0).all()
        dups = [j for j in DUP if j < rows]
        assert idx[2, :len(dups)].tolist() == dups and (sim[2, :len(dups)] == sim[2, 0]).all()
        # moments on the NaN-free bank
        gpu_engine.set_bank(clean[:rows].contiguous().cuda())
        idx, sim, mom = _dense(gpu_engine, qd, k, 0.05, True)
        S = q.double().numpy() @ _stored64(clean[:rows]).T
        ref = np.stack([S.sum(1), (S * S).sum(1), (S >= 0.05).sum(1).astype(np.float64)], 1)
        assert np.allclose(mom[:, [0, 1, 3]], ref, rtol=1e-4, atol=1e-3)
        assert np.array_equal(mom[:, 2].view(np.int32), sim[:, 0].view(np.int32))      # max: bit-equal to the first rank


def overflow_bank(exact=False):
    """The degenerate bank of test_bank_search_overflow_is_reported: (bank, query, fp32 accumulation bound of a similarity).
    ``exact``: the same rows on a grid of 2^-6, so that every product and partial sum is exact in fp32 (bound 0)."""
    D = 128
    row = _unit((1, D), 5)
    q = row + 0.01 * _unit((1, D), 6)
    if exact:
        row, q = torch.round(row * 64) / 64, torch.round(q * 64) / 64
    bank = row.repeat(40000, 1).to(torch.bfloat16)
    acc_err = 0.0 if exact else D * 2.0 ** -24 * float((bank[:1].double().abs() * q.double().abs()).sum())
    return bank, q, acc_err


def test_bank_search_overflow_is_reported(gpu_engine, pkg):
    """A degenerate bank (all rows identical) cannot be bounded by sampling: the overflow must be reported, never silently
    truncated.  The model of tests/bank_witness.py says which outcome is right: every row's similarity clears tau (the
    sampled value less kth_finish's slack) and every list overflows.  On the grid-exact bank that holds for both forms bit
    for bit; on the unit-vector bank the one-product form clears tau by 9e-4, far beyond the accumulation bound of 8e-6,
    while the all-products form clears it by 2e-6 only, which that bound cannot decide: there the old rule stays -- either
    outcome, never a wrong answer without an error (tests/test_bank_witness.py::test_degenerate_bank_overflows_by_the_model)."""
    import bank_witness as W
    for exact in (True, False):
        bank, q, acc_err = overflow_bank(exact)
        gpu_engine.set_bank(bank.cuda())
        for want_moments in (True, False):
            want = W.model(bank, q, 5, 0.3, W.form_of(40000, 1, 128, True, want_moments), acc_err=acc_err)
            gpu_engine.bank_search(q.cuda(), 5, want_moments=want_moments)
            try:
                gpu_engine.bank_status()
                ok = True
            except pkg.TVCError as e:
                ok = False
                assert e.code == pkg._lib.TVC_E_OVERFLOW
            if want.decided:
                assert want.overflow and not ok, (exact, want_moments)
            elif ok:
                idx, sim, _ = gpu_engine.bank_search(q.cuda(), 5, want_moments=want_moments)
                gpu_engine.bank_status()
                assert idx.cpu().numpy().tolist()[0] == [0, 1, 2, 3, 4]
    # a search after an overflowed one is clean
    gpu_engine.set_bank(_unit((300, 128), 8).to(torch.bfloat16).cuda())
    gpu_engine.bank_search(_unit((2, 128), 9).cuda(), 5)
    gpu_engine.bank_status()


@pytest.mark.parametrize("B,N,D,R", [(8, 4, 512, 1000), (33, 8, 768, 3000), (5, 0, 128, 100)])
def test_consistency_vs_oracle(gpu_engine, pkg, B, N, D, R):
    img = _unit((B, D), 11) * 3.0                       # norms != 1: cosines must normalise
    txt = _unit((B, N + 1, D), 12)
    txt = txt + 0.5 * img[:, None, :] / 3.0             # correlate text with its image
    bank = pkg.synth.make_bank(R, D, seed=7)
    tn = txt / txt.norm(dim=-1, keepdim=True)
    bank = pkg.synth.plant_neighbours(bank, tn.reshape(-1, D)[:: 2], per_anchor=3)
    bank16 = bank.to(torch.bfloat16)
    cfg = pkg.ConsistencyConfig()
    gpu_engine.set_bank(bank16.cuda())
    rec = gpu_engine.detect_embeddings(img.cuda(), tn.cuda(), cfg).cpu().numpy()
    gpu_engine.bank_status()
    ref = tvc_oracle.detect_batch(img.numpy(), tn.numpy(), bank16.float().numpy(),
                                  checker=tvc_oracle.ConsistencyCheckerOracle(adaptive_threshold=False))
    # the keep / drop decisions hang on the bank search's rounding unless every retrieved similarity is clear of the
    # threshold: 8.6e-4 (fp64) at (8, 4, 512, 1000), 1.4e-3 at (33, 8, 768, 3000), against a search error of ~1e-6
    top = (tn.reshape(-1, D).double() @ bank16.double().t()).topk(cfg.reference_count).values
    print(f"[measured] consistency ({B},{N},{D},{R}): nearest retrieved similarity is "
          f"{(top - cfg.similarity_threshold).abs().min().item():.2e} from the {cfg.similarity_threshold} threshold")
    tol = 1e-4     # BASELINE.json: consistency scores within 1e-4
    assert np.abs(rec[:, 0] - ref["original_similarity"]).max() < tol
    assert np.abs(rec[:, 1] - ref["variant_mean"]).max() < tol
    assert np.abs(rec[:, 2] - ref["variant_std"]).max() < tol
    assert np.abs(rec[:, 5] - ref["score_src"]).max() < tol
    assert np.abs(rec[:, 6] - ref["retrieval_consistency"]).max() < tol
    assert np.abs(rec[:, 7] - ref["retrieval_std"]).max() < tol
    assert np.abs(rec[:, 9] - ref["cross_modal_variance"]).max() < tol
    assert np.abs(rec[:, 10] - ref["overall_exp"]).max() < tol
    if N:
        assert np.abs(rec[:, 12:12 + N] - ref["variant_similarities"]).max() < tol
    kept = rec[:, 12 + N:12 + N + 16].copy().view(np.int32)
    assert (ref["retrieval_indices"] >= 0).sum() > 0, "test bank must produce references"
    for b in range(B):
        want = ref["retrieval_indices"][b]
        want = want[want >= 0]
        assert kept[b, :len(want)].tolist() == want.tolist()
        assert (kept[b, len(want):] == -1).all()


def test_towers_vs_oracle(pkg):
    """Tiny CLIP geometry, shared random weights.  The HIP towers multiply
    bf16-rounded weights and activations with fp32 accumulation; against the
    fp32 oracle on the same bf16-rounded weights the unit-norm embeddings agree
    within ~2x the deviation measured on MI355X (bf16 activations: 2^-9 relative per op)."""
    arch = pkg.get_arch("ViT-T/16-test")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    eng = pkg.TVCEngine(arch, vw, tw)
    imgs = pkg.synth.make_images(9, arch.image_size, seed=1)
    toks = pkg.synth.make_tokens(6, 2, arch.ctx, seed=2).reshape(-1, arch.ctx)
    gi = eng.encode_image(imgs.cuda()).cpu()
    gt = eng.encode_text(toks.cuda()).cpu()
    vr, tr = clip_oracle.round_gemm_weights_to_bf16(vw), clip_oracle.round_gemm_weights_to_bf16(tw)
    with torch.no_grad():
        ri = clip_oracle.vision_forward(vr, imgs, arch.vision.heads, arch.patch)
        rt = clip_oracle.text_forward(tr, toks, arch.text.heads)
    assert torch.isfinite(gi).all() and torch.isfinite(gt).all()
    print(f"[measured] ViT-T/16-test vs oracle (bf16w): image min cos {((gi * ri).sum(-1)).min().item():.6f} max|d| "
          f"{(gi - ri).abs().max().item():.2e}; text min cos {((gt * rt).sum(-1)).min().item():.6f} max|d| {(gt - rt).abs().max().item():.2e}")
    # bounds ~2x the measured deviation (image 7.8e-4 / min cos 0.999997, text 1.3e-3 / 0.999989); DESIGN.md section 2
    assert (gi - ri).abs().max().item() < 1.6e-3 and (gi * ri).sum(-1).min().item() > 0.99999
    assert (gt - rt).abs().max().item() < 2.6e-3 and (gt * rt).sum(-1).min().item() > 0.99997
    # unnormalised outputs too
    gi2 = eng.encode_image(imgs.cuda(), normalize=False).cpu()
    with torch.no_grad():
        ri2 = clip_oracle.vision_forward(vr, imgs, arch.vision.heads, arch.patch, normalize=False)
    assert (gi2 - ri2).abs().max().item() < 8e-3 * ri2.abs().max().item()
    eng.close()


def test_text_packing_is_bit_identical(pkg):
    """TVC_OPT_TEXT_PACKING drops the tokens after EOT; under the causal mask the
    pooled row cannot depend on them, so packed == dense bit for bit."""
    arch = pkg.get_arch("ViT-T/16-test")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    eng = pkg.TVCEngine(arch, None, tw)
    toks = pkg.synth.make_tokens(40, 2, arch.ctx, seed=5, min_len=1, max_len=75).reshape(-1, arch.ctx)
    toks[3, :] = 0; toks[3, 0] = 49406; toks[3, 1] = 49407                 # shortest legal text
    toks[5, 1:76] = 17; toks[5, 76] = 49407                                 # longest: EOT at position 76
    packed = eng.encode_text(toks.cuda()).cpu()
    eng.set_option(pkg._lib.TVC_OPT_TEXT_PACKING, 0)
    dense = eng.encode_text(toks.cuda()).cpu()
    assert torch.equal(packed, dense)
    # junk after EOT must not matter either
    toks2 = toks.clone()
    toks2[0, toks[0].argmax() + 1:] = 123
    eng.set_option(pkg._lib.TVC_OPT_TEXT_PACKING, 1)
    assert torch.equal(eng.encode_text(toks2.cuda()).cpu()[0], packed[0])
    eng.close()


@pytest.mark.parametrize("model,ctx_lens", [("ViT-T/16-test", (1, 75)), ("ViT-L/14", (5, 20))])
def test_text_prefix_sharing_is_bit_identical(pkg, model, ctx_lens):
    """TVC_OPT_TEXT_GROUP = N+1: a variant keeps only the rows from its first token that differs from
    the group's original on (the causal tower gives the shared prefix identical hidden states) and
    attends to the original's rows for the prefix.  Same embeddings bit for bit, including variants
    identical to the original, differing right after SOT, or longer / shorter than it."""
    arch = pkg.get_arch(model)
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    eng = pkg.TVCEngine(arch, None, tw)
    Q, N = (24, 3) if model != "ViT-L/14" else (64, 8)
    toks = pkg.synth.make_tokens(Q, N, arch.ctx, seed=6, min_len=ctx_lens[0], max_len=ctx_lens[1])
    toks[1, 2] = toks[1, 0]                                        # variant identical to its original
    toks[2, 1, 1] = 777                                            # differs right after SOT
    L = int(toks[3, 0].argmax())
    if L + 2 < arch.ctx:
        toks[3, 1, L] = 55; toks[3, 1, L + 1] = 49407              # one token longer than the original
    if L > 2:
        toks[3, 2] = 0; toks[3, 2, :L - 1] = toks[3, 0, :L - 1]; toks[3, 2, L - 1] = 49407   # one token shorter
    flat = toks.reshape(-1, arch.ctx).cuda()
    plain = eng.encode_text(flat).cpu()
    ws0 = eng.workspace_bytes()
    eng.set_option(pkg._lib.TVC_OPT_TEXT_GROUP, N + 1)
    shared = eng.encode_text(flat).cpu()
    assert torch.equal(shared, plain)
    # a batch that is not a whole number of groups silently falls back to the plain packed path
    assert torch.equal(eng.encode_text(flat[:-1]).cpu(), plain[:-1])
    # several passes: the chunk is cut to whole groups (here 2 groups per pass), or sharing is dropped
    # when a pass cannot hold one group
    eng.set_option(pkg._lib.TVC_OPT_MAX_CHUNK_TEXTS, 2 * (N + 1) + 1)
    assert torch.equal(eng.encode_text(flat).cpu(), plain)
    eng.set_option(pkg._lib.TVC_OPT_MAX_CHUNK_TEXTS, N)
    assert torch.equal(eng.encode_text(flat).cpu(), plain)
    eng.close()


def test_two_shard_search_equals_full_search(gpu_engine):
    """The bank-sharded path on one GPU: search each half with its global row offset,
    gather the winners' rows, merge with tvc_topk_merge -> identical to searching the
    whole bank (indices, similarities and gathered feature rows)."""
    R, D, M, k, kf = 6001, 256, 77, 8, 3
    bank = _unit((R, D), 31).to(torch.bfloat16).cuda()
    q = _unit((M, D), 32).cuda()
    gpu_engine.set_bank(bank)
    S = q.double() @ bank.double().t()
    for want_moments in (True, False):       # all-products pass with moments / filter + re-score form
        gpu_engine.set_bank(bank)
        fi, fs, _ = gpu_engine.bank_search(q, k, 0.05, want_moments=want_moments)
        ff = gpu_engine.bank_gather(fi[:, :kf].contiguous())
        gpu_engine.bank_status()
        parts_i, parts_s, parts_f, parts_m = [], [], [], []
        for lo, hi in ((0, 3000), (3000, R)):
            gpu_engine.set_bank(bank[lo:hi].contiguous())
            i, s, m = gpu_engine.bank_search(q, k, 0.05, idx_offset=lo, want_moments=want_moments)
            f = gpu_engine.bank_gather(i[:, :kf].contiguous(), idx_offset=lo)
            gpu_engine.bank_status()
            parts_i.append(i); parts_s.append(s); parts_f.append(f)
            if want_moments:
                parts_m.append(m)
        mi, ms, mf, mm = gpu_engine.topk_merge(torch.stack(parts_i), torch.stack(parts_s), torch.stack(parts_f),
                                               torch.stack(parts_m) if want_moments else None)
        assert torch.equal(mi, fi) and torch.equal(ms, fs) and torch.equal(mf, ff)
        if want_moments:
            assert (mm[:, 3].cpu() - (S >= 0.05).sum(1).cpu()).abs().max() <= 1


def _nccl_group(tmp_path, name):
    """A ONE-rank RCCL process group on cuda:0 (fresh per test): all_gather_into_tensor and all_to_all_single --
    equal and split sizes -- then execute on the GPU box exactly as they do on an 8-GPU node."""
    import torch.distributed as dist
    dist.init_process_group("nccl", init_method=f"file://{tmp_path}/{name}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    return dist


def test_sharded_search_on_gpu_over_rccl(gpu_engine, pkg, tmp_path):
    """``ShardedBankSearch`` with the product ops (``HipShardOps``) in a one-rank **nccl (RCCL)** process group: the
    fused single-collective exchange (default, no host synchronisation), the two-phase exchange (variable-size
    all_to_all_single with split sizes) and the single-phase form all return what a direct search + gather returns,
    bit for bit; ``feat_from`` skips the leading rows."""
    R, D, M, k, kf = 30011, 256, 130, 8, 5
    bank = _unit((R, D), 41).to(torch.bfloat16).cuda()
    q = _unit((M, D), 42).cuda()
    gpu_engine.set_bank(bank)
    ri, rs, _ = gpu_engine.bank_search(q, k, 0.3, want_moments=False)
    rf = gpu_engine.bank_gather(ri[:, :kf].contiguous())
    gpu_engine.bank_status()
    dist = _nccl_group(tmp_path, "pg")
    try:
        assert dist.get_backend() == "nccl"
        for mode, per in (("fused", None), ("fused", R), ("two_phase", R), ("single_phase", None)):
            s = pkg.sharding.ShardedBankSearch(pkg.sharding.HipShardOps(gpu_engine, 0, 0.3), rows_per_shard=per, mode=mode)
            i, v, f = s.search(q, k, kf)
            assert torch.equal(i, ri) and torch.equal(v, rs) and torch.equal(f, rf), mode
            if mode == "fused":
                assert s.last_exchange["host_syncs"] == 0
                s.check_status()
                i2, v2, f2 = s.search(q, k, kf, feat_from=30)
                assert torch.equal(i2, ri) and torch.equal(v2, rs) and torch.equal(f2[30:], rf[30:])
                assert float(f2[:30].abs().max()) == 0.0
    finally:
        dist.destroy_process_group()


def test_bank_search_nan_rows_and_ragged_query_tile(gpu_engine):
    """M % 256 != 0 with a zero-norm LAST query row (NaN after `x / x.norm()`, retrieval_ref.py:243 has no
    epsilon) and one NaN bank row: the padded query lanes of the last tile re-read that row.  The other
    queries' top-k must be untouched, NaN similarities are never returned, and nothing is written outside
    the candidate lists (the search after it is clean)."""
    R, M, D, k = 20000, 300, 256, 5
    bank = _unit((R, D), 41).to(torch.bfloat16)
    q = _unit((M, D), 42)
    gpu_engine.set_bank(bank.cuda())
    want_i, want_s, _ = gpu_engine.bank_search(q[:M - 1].cuda(), k, want_moments=False)
    gpu_engine.bank_status()
    q_bad = q.clone()
    q_bad[M - 1] = float("nan")                      # what l2norm makes of an all-zero embedding
    for want_moments in (False, True):
        i1, s1, _ = gpu_engine.bank_search(q_bad.cuda(), k, want_moments=want_moments)
        gpu_engine.bank_status()
        assert torch.equal(i1[:M - 1], want_i) and torch.allclose(s1[:M - 1], want_s, atol=5e-6)
        assert (i1[M - 1] == -1).all()
    # one NaN bank row: bank_bounds turns NaN, the one-product filter lists everything, the status reports the
    # overflow and the robust form recomputes by brute force -- never a wrong answer
    bank2 = bank.clone()
    bank2[777] = float("nan")
    gpu_engine.set_bank(bank2.cuda())
    i2, s2, _ = gpu_engine.bank_search_robust(q[:64].cuda(), k, want_moments=False)
    S = q[:64].double() @ bank.double().t()
    S[:, 777] = -2.0
    v, ix = S.topk(k, dim=1)
    assert torch.equal(i2.cpu().long(), ix) and (s2.cpu().double() - v).abs().max().item() < 1e-5
    gpu_engine.set_bank(bank.cuda())
    i3, s3, _ = gpu_engine.bank_search(q[:M - 1].cuda(), k, want_moments=False)
    gpu_engine.bank_status()
    assert torch.equal(i3, want_i)


@pytest.mark.parametrize("k", [33, 64, 128])
def test_bank_search_large_k(gpu_engine, k):
    """The reference accepts any top_k (src/ref_bank.py:172, src/retrieval.py:636); the kernel serves up to
    TVC_MAX_TOPK = 128 exactly and the engine raises beyond it (never a silent truncation)."""
    R, M, D = 50000, 40, 512
    bank = _unit((R, D), 51).to(torch.bfloat16)
    q = _unit((M, D), 52)
    gpu_engine.set_bank(bank.cuda())
    idx, sim, _ = gpu_engine.bank_search(q.cuda(), k, want_moments=False)
    gpu_engine.bank_status()
    S = (q.double() @ bank.double().t()).numpy()
    _check_topk(idx.cpu().numpy(), sim.cpu().numpy().astype(np.float64), S, k, 1e-5)
    with pytest.raises(ValueError):
        gpu_engine.bank_search(q.cuda(), 129, want_moments=False)


def _clustered_bank(R, D, n_clusters, seed, device="cuda:0", dup_every=997):
    """Mixture bank: `n_clusters` random unit centres, every row = normalise(centre + s * noise) with the
    per-row spread s drawn so that the cosine to its centre lies in ~[0.6, 0.95] (a von-Mises-Fisher-like
    cloud), plus exact duplicates (every `dup_every`-th row repeats its predecessor)."""
    g = torch.Generator(device=device).manual_seed(seed)
    centres = torch.randn((n_clusters, D), device=device, generator=g)
    centres /= centres.norm(dim=-1, keepdim=True)
    out = torch.empty((R, D), dtype=torch.bfloat16, device=device)
    for r0 in range(0, R, 1 << 18):
        n = min(1 << 18, R - r0)
        c = torch.randint(0, n_clusters, (n,), device=device, generator=g)
        cos = 0.6 + 0.35 * torch.rand((n, 1), device=device, generator=g)
        s = torch.sqrt(1.0 / (cos * cos) - 1.0)                      # |noise| / |centre| for that cosine
        x = centres[c] + s * torch.randn((n, D), device=device, generator=g) / (D ** 0.5)
        x /= x.norm(dim=-1, keepdim=True)
        out[r0:r0 + n] = x.to(torch.bfloat16)
    out[dup_every::dup_every] = out[dup_every - 1::dup_every][:out[dup_every::dup_every].shape[0]]
    return out, centres


def test_bank_search_clustered_1m_bank(gpu_engine):
    """A REALISTIC bank: 1 M rows in 2 000 clusters (intra-cluster cosine 0.6-0.95) + exact duplicates,
    queries near cluster centres (the case every CLIP bank presents) and far from all of them.  The sampled
    bound must stay exact (vs a chunked fp64 product), and the statistics that decide whether the dense
    fallback triggers are printed: survivors per (chunk, query) list, overflow flag, time."""
    import time
    R, D, M, k = 1_000_000, 768, 5120, 5
    bank, centres = _clustered_bank(R, D, 2000, seed=61)
    g = torch.Generator(device="cuda:0").manual_seed(62)
    q = torch.randn((M, D), device="cuda:0", generator=g)
    q /= q.norm(dim=-1, keepdim=True)
    near = centres[torch.randint(0, 2000, (M // 2,), device="cuda:0", generator=g)]
    q[:M // 2] = near + 0.5 * torch.randn((M // 2, D), device="cuda:0", generator=g) / (D ** 0.5)
    q /= q.norm(dim=-1, keepdim=True)
    gpu_engine.set_bank(bank)
    before = getattr(gpu_engine, "dense_fallbacks", 0)
    gpu_engine.bank_search(q, k, want_moments=False)                 # warm-up (workspace growth)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx, sim, _ = gpu_engine.bank_search(q, k, want_moments=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    overflow = False
    try:
        gpu_engine.bank_status()
    except Exception as e:                                           # TVC_E_OVERFLOW
        overflow = True
        print("overflow:", e)
    print(f"[measured] clustered 1M x 768 bank, M = {M}: filter search {dt * 1e3:.1f} ms, overflow = {overflow}")
    assert not overflow, "the sampled bound must hold on a clustered bank without the brute-force fallback"
    assert getattr(gpu_engine, "dense_fallbacks", 0) == before
    # exactness on 24 rows (12 near a centre, 12 random) vs fp64, the bank taken 250k rows at a time
    rows_sel = torch.cat([torch.arange(0, 12), torch.arange(M - 12, M)]).cuda()
    rows = q[rows_sel].double()
    best_v = torch.full((24, k), -2.0, dtype=torch.float64, device="cuda:0")
    best_i = torch.zeros((24, k), dtype=torch.long, device="cuda:0")
    for lo in range(0, R, 250_000):
        S = rows @ bank[lo:lo + 250_000].double().t()
        cat_v = torch.cat([best_v, S], 1)
        cat_i = torch.cat([best_i, torch.arange(lo, lo + S.shape[1], device="cuda:0").expand(24, -1)], 1)
        # (similarity desc, index asc): exact duplicates tie
        order = torch.argsort(cat_i, dim=1, stable=True)
        cat_v, cat_i = torch.gather(cat_v, 1, order), torch.gather(cat_i, 1, order)
        o2 = torch.argsort(cat_v, dim=1, descending=True, stable=True)[:, :k]
        best_v, best_i = torch.gather(cat_v, 1, o2), torch.gather(cat_i, 1, o2)
    got_s, got_i = sim[rows_sel].double(), idx[rows_sel].long()
    assert (got_s - best_v).abs().max().item() < 1e-5
    exact = (got_i == best_i)
    # differing positions only where two rows tie within the fp32 rounding of the re-scoring
    assert ((got_s - best_v).abs()[~exact] < 2e-6).all()
    assert (sim[:M // 2, 0] > 0.5).float().mean().item() > 0.9      # near-centre queries do find their cluster


@pytest.mark.parametrize("model", ["ViT-T/16-test", "ViT-B/32"])
def test_pooled_last_layer_is_bit_identical(pkg, model):
    """TVC_OPT_POOLED_LAST_LAYER: the last layer of a tower computes attention / out-proj / ln_2 / MLP for the
    pooled token only (class token, EOT token).  Same fp32 sums in the same order -> the embeddings must equal
    the all-token computation bit for bit: vision, text dense / packed / with prefix sharing (incl. a variant
    identical to its original, whose EOT row is the original's)."""
    arch = pkg.get_arch(model)
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    eng = pkg.TVCEngine(arch, vw, tw)
    imgs = pkg.synth.make_images(5, arch.image_size, seed=1).cuda()
    toks = pkg.synth.make_tokens(6, 3, arch.ctx, seed=5, min_len=1, max_len=60)
    toks[1, 2] = toks[1, 0]                                   # a variant equal to its original
    toks[2, 1, 1:70] = 17; toks[2, 1, 70] = 49407; toks[2, 1, 71:] = 0     # a long one
    toks = toks.reshape(-1, arch.ctx).cuda()
    out = {}
    for pooled in (1, 0):
        eng.set_option(pkg._lib.TVC_OPT_POOLED_LAST_LAYER, pooled)
        res = [eng.encode_image(imgs), eng.encode_image(imgs, normalize=False)]
        for packing in (1, 0):
            eng.set_option(pkg._lib.TVC_OPT_TEXT_PACKING, packing)
            res.append(eng.encode_text(toks))
            res.append(eng.encode_text(toks, group=4))
        eng.set_option(pkg._lib.TVC_OPT_TEXT_PACKING, 1)
        out[pooled] = [r.cpu() for r in res]
    for a, b in zip(out[1], out[0]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert torch.equal(out[1][2], out[1][3]) and torch.equal(out[1][2], out[1][4])      # packed == shared == dense
    eng.close()


def test_text_hidden_states_vs_oracle(pkg):
    """tvc_encode_text_hidden: ln_final of every position (CLIPTextModel.last_hidden_state, the SD conditioning).
    Dense rows, padded with the EOT id as SD does; vs the fp32 oracle on bf16-rounded weights."""
    arch = pkg.get_arch("ViT-T/16-test")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    eng = pkg.TVCEngine(arch, vw, tw)
    toks = pkg.synth.make_tokens(5, 1, arch.ctx, seed=4).reshape(-1, arch.ctx).clone()
    eot = toks.argmax(-1)
    for i in range(toks.shape[0]):
        toks[i, eot[i]:] = toks[i, eot[i]]
    got = eng.encode_text_hidden(toks.cuda()).cpu()
    with torch.no_grad():
        ref = clip_oracle.text_hidden(clip_oracle.round_gemm_weights_to_bf16(tw), toks.long(), arch.text.heads)
    assert got.shape == ref.shape == (toks.shape[0], arch.ctx, arch.text.width)
    err = (got - ref).abs().max().item()
    print(f"[measured] text hidden states vs oracle (bf16w): max |d| {err:.2e} (|ref| max {ref.abs().max().item():.2f})")
    assert err < 3e-2 * max(1.0, ref.abs().max().item() / 4)
    # the pooled EOT row, projected and normalised, is what tvc_encode_text returns
    emb = eng.encode_text(toks.cuda()).cpu()
    e2 = torch.nn.functional.normalize(got[torch.arange(toks.shape[0]), eot] @ tw["proj"].float().t(), dim=-1)
    assert (emb - e2).abs().max().item() < 2e-3
    eng.close()


def test_sharded_search_with_a_degenerate_shard(gpu_engine, pkg, tmp_path):
    """Round-1 advice: a shard whose candidate lists overflow (40 000 identical rows) must not hand the merge a
    silently truncated list.  Fused (asynchronous) form: ``check_status`` raises TVC_E_OVERFLOW on every rank;
    status-checked forms: ``HipShardOps.search`` goes through ``bank_search_robust`` (``dense_fallbacks`` counts it)
    and the shard's answer is the brute-force one -- exact.  One-rank RCCL group."""
    D, M, k, kf = 256, 40, 5, 5
    row = _unit((1, D), 5)
    bank = torch.cat([row.repeat(40000, 1), _unit((500, D), 6)]).to(torch.bfloat16).cuda()
    q = torch.cat([_unit((M - 1, D), 7), row]).cuda()
    gpu_engine.set_bank(bank)
    before = getattr(gpu_engine, "dense_fallbacks", 0)
    dist = _nccl_group(tmp_path, "pg2")
    try:
        fused = pkg.sharding.ShardedBankSearch(pkg.sharding.HipShardOps(gpu_engine, 0, 0.3))
        fused.search(q, k, kf)
        try:
            fused.check_status()
            overflowed = False
        except pkg.TVCError as e:
            overflowed = e.code == pkg._lib.TVC_E_OVERFLOW
        s = pkg.sharding.ShardedBankSearch(pkg.sharding.HipShardOps(gpu_engine, 0, 0.3), rows_per_shard=bank.shape[0], mode="two_phase")
        i, v, f = s.search(q, k, kf)
    finally:
        dist.destroy_process_group()
    assert getattr(gpu_engine, "dense_fallbacks", 0) > before, "the overflow must have been detected"
    assert overflowed, "the asynchronous form must report the overflow through check_status"
    S = q.double() @ bank.double().t()
    want_v, _ = S.topk(k, dim=1)
    assert (v.double() - want_v).abs().max().item() < 1e-5
    # ties (the identical rows) resolve to the smallest indices
    assert i[M - 1].tolist() == [0, 1, 2, 3, 4]
    assert torch.equal(f[M - 1, 0].cpu(), bank[0].float().cpu())
