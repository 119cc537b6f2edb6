"""GPU: the pair-list and pair-cosine kernels (tvc_graph_pair_count / tvc_graph_pair_fill / tvc_pair_cosine),
``TVCEngine.graph_pairs / pair_cosine / similar_pairs`` and ``DataValidator`` against the fp64 restatement of
tests/validator_ref.py (pinned to sklearn plus the reference's double loops and to the reference's own output by
tests/test_validator_ref.py).

The integer work (pair lists, offsets, totals, capacity) is compared with ==.

The cosine bound, derived, not measured: B(D) = 2^-24 (2 D + 16) on |sim - cos64(operands)|.  With u = 2^-24 a sum of D fp32 FMA
terms in ANY order is within D u sum|a_i b_i| of the exact sum, so dot is within D u |x| |y| of x.y and each squared norm within
D u of itself relatively; sqrt(nx ny) then carries D u (half of 2 D u) plus one rounding each for the product and the root, the
quotient one more: |sim - cos| <= (2 D + 3) u + O(u^2) for |cos| <= 1, and 16 leaves room for the second-order terms up to
D = 768.  The operands are the values the kernel sees (the bf16 values, or hi + lo of an fp32 row's planes: ``operands()`` of
tests/test_gpu_dbscan.py).

B(D) is the C-ABI's promise.  The kernel's own summation order gives a tighter derived bound, and test 3 asserts that one:
a lane adds n = 8 ceil(D / 128) FMA terms in a chain and the 16 lanes of a pair meet in 4 butterfly levels, so every term
passes through at most n + 4 roundings instead of D: |sim - cos| <= (2 (n + 4) + 3) u + O(u^2), stated as
Bk(D) = 2^-24 (16 ceil(D / 128) + 16) <= B(D) (32 u at D = 64, 112 u at D = 768 against B's 144 u and 1 552 u).

``similar_pairs`` decides a pair by that cosine: a pair may differ from fp64 only inside |cos64 - t| <= B(D).

Measured on an MI355X: see the figures each test prints, and EXPERIMENTS.md."""
import ctypes as C
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import validator_ref

pytestmark = pytest.mark.gpu
BANK = "validator-test"
GOLDEN = Path(__file__).resolve().parent / "golden" / "data_validator.npz"

PAIR_R = [1, 2, 31, 32, 33, 63, 64, 65, 127, 129, 257, 1000]
KINDS = ["empty", "diagonal", "full", "random"]
COS_D = [64, 128, 512, 768]


def bound(D):
    return 2.0 ** -24 * (2 * D + 16)


def kernel_bound(D):
    """Bk(D): the bound of pair_cosine_kernel's own summation order (module docstring)"""
    return 2.0 ** -24 * (16 * ((D + 127) // 128) + 16)


def operands(X: torch.Tensor) -> np.ndarray:
    """fp64 values of the rows as the kernels see them: the bf16 values, or hi + lo of the fp32 rows' bf16 planes."""
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


# ---- 1: pair lists of supplied bitmasks ----------------------------------------------------------------------------------
def words(R):
    return (R + 63) // 64 * 2


def pack(A):
    """bool [R, 32 W] -> the engine's int32 words [R, W]"""
    return torch.from_numpy(np.packbits(A, axis=1, bitorder="little").view(np.uint32).view(np.int32).copy())


@functools.lru_cache(maxsize=None)
def graph(R, kind):
    """bool [R, 32 W(R)], padding columns included.  'full' sets every bit of every word (lower triangle, diagonal and padding);
    'random' is 5 % of ALL bits, not symmetric: garbage in the lower triangle and set padding bits."""
    rng = np.random.default_rng(1000 * R + len(kind))
    A = np.zeros((R, words(R) * 32), bool)
    if kind == "diagonal":
        A[np.arange(R), np.arange(R)] = True
    elif kind == "full":
        A[:] = True
    elif kind == "random":
        A = rng.random(A.shape) < 0.05
    return A


@functools.lru_cache(maxsize=None)
def groups_of(R):
    """three groups plus -1 rows"""
    return np.random.default_rng(R).integers(-1, 3, R).astype(np.int32)


@pytest.mark.parametrize("grouped", [False, True], ids=["all", "groups"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R", PAIR_R)
def test_graph_pairs_equal_numpy(gpu_engine, R, kind, grouped):
    A = graph(R, kind)
    g = groups_of(R) if grouped else None
    want, want_off = validator_ref.pairs(A, g)
    pairs, offsets = gpu_engine.graph_pairs(pack(A).to(gpu_engine.device),
                                            groups=None if g is None else torch.from_numpy(g).to(gpu_engine.device))
    assert pairs.dtype == torch.int32 and offsets.dtype == torch.int64 and tuple(offsets.shape) == (R + 1,)
    assert np.array_equal(offsets.cpu().numpy(), want_off)                       # the prefix sums, the exact total at [R]
    assert tuple(pairs.shape) == (len(want), 2) and np.array_equal(pairs.cpu().numpy(), want)
    if kind == "full" and not grouped:
        assert len(want) == R * (R - 1) // 2
    if kind in ("empty", "diagonal"):
        assert len(want) == 0


def test_lower_triangle_and_padding_bits_are_ignored(gpu_engine):
    rng = np.random.default_rng(4)
    for R in (33, 65, 200):
        U = np.triu(rng.random((R, R)) < 0.2, 1)
        clean = np.zeros((R, words(R) * 32), bool)
        clean[:, :R] = U | U.T
        dirty = clean.copy()
        dirty[:, :R][np.tril_indices(R)] = rng.random(R * (R + 1) // 2) < 0.5     # garbage on and below the diagonal
        dirty[:, R:] = True                                                        # every padding bit set
        a = gpu_engine.graph_pairs(pack(clean).to(gpu_engine.device))
        b = gpu_engine.graph_pairs(pack(dirty).to(gpu_engine.device))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert np.array_equal(a[0].cpu().numpy(), np.argwhere(U))


# ---- 2: capacity ---------------------------------------------------------------------------------------------------------
def test_total_above_max_pairs_raises_and_names_the_total(gpu_engine):
    R = 129
    adj = pack(graph(R, "full")).to(gpu_engine.device)
    total = R * (R - 1) // 2
    with pytest.raises(ValueError, match=str(total)):
        gpu_engine.graph_pairs(adj, max_pairs=total - 1)
    pairs, _ = gpu_engine.graph_pairs(adj, max_pairs=total)
    assert len(pairs) == total


@pytest.mark.parametrize("grouped", [False, True], ids=["all", "groups"])
def test_a_short_buffer_gets_the_first_pairs_and_is_not_overrun(gpu_engine, grouped):
    eng, R = gpu_engine, 257
    A = graph(R, "random")
    g = groups_of(R) if grouped else None
    want, want_off = validator_ref.pairs(A, g)
    total = len(want)
    adj = pack(A).to(eng.device)
    gd = None if g is None else torch.from_numpy(g).to(eng.device)
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    offsets = torch.empty(R + 1, dtype=torch.int64, device=eng.device)
    assert eng.lib.tvc_graph_pair_count(eng.handle, ptr(adj), R, ptr(gd), ptr(offsets), stream) == 0
    assert np.array_equal(offsets.cpu().numpy(), want_off)
    for P in (0, 1, total // 2, total - 1, total):
        buf = torch.full((total + 8, 2), -7, dtype=torch.int32, device=eng.device)
        assert eng.lib.tvc_graph_pair_fill(eng.handle, ptr(adj), R, ptr(gd), ptr(offsets), ptr(buf), P, stream) == 0
        got = buf.cpu().numpy()
        assert np.array_equal(got[:P], want[:P])                                   # exactly the first P pairs
        assert (got[P:] == -7).all()                                               # the sentinel behind them is untouched


# ---- 3: the cosine against fp64 of the operands ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cosine_case(D, bf16):
    """-> (X as registered, operands, pairs int32 [P, 2] inside the slot): rows of norm 1e-3 .. 1e3, duplicates, scaled and near
    copies, a zero row (R - 2) and a NaN row (R - 1)."""
    rng = np.random.default_rng(D + bf16)
    R = 200
    X = rng.standard_normal((R, D)) * (10.0 ** rng.uniform(-3, 3, R))[:, None]
    X[::40] *= 1e3 / np.linalg.norm(X[::40], axis=1, keepdims=True)               # the ends of the range exactly
    X[1::40] *= 1e-3 / np.linalg.norm(X[1::40], axis=1, keepdims=True)
    for k in range(20):                                                           # near, scaled and exact copies of row 2 k
        X[100 + k] = X[2 * k] * 10.0 ** rng.uniform(-2, 2) + (k % 4) * 0.02 * np.linalg.norm(X[2 * k]) / np.sqrt(D) * rng.standard_normal(D)
    X[R - 2] = 0.0
    X = torch.from_numpy(X.astype(np.float32))
    X[R - 1] = float("nan")
    if bf16:
        X = X.bfloat16()
    P = np.concatenate([rng.integers(0, R - 2, (3000, 2)), np.stack([2 * np.arange(20), 100 + np.arange(20)], 1),
                        np.stack([np.arange(R - 2), np.arange(R - 2)], 1)]).astype(np.int32)
    return X, operands(X), P


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", COS_D)
def test_pair_cosine_against_fp64(gpu_engine, D, bf16):
    X, X64, P = cosine_case(D, bf16)
    R = len(X)
    dev = gpu_engine.device
    special = np.array([[R - 2, 5], [5, R - 2], [R - 2, R - 2], [R - 1, 5], [5, R - 1], [R - 1, R - 1], [R - 1, R - 2],
                        [-1, 5], [5, -1], [R, 5], [5, R], [-1, R], [2 ** 31 - 1, 0], [-2 ** 31, 0]], np.int64).astype(np.int32)
    with Slot(gpu_engine, X) as eng:
        sims = eng.pair_cosine(torch.from_numpy(P).to(dev), bank=BANK)
        again = eng.pair_cosine(torch.from_numpy(P).to(dev), bank=BANK)
        swapped = eng.pair_cosine(torch.from_numpy(P[:, ::-1].copy()).to(dev), bank=BANK)
        spec = eng.pair_cosine(torch.from_numpy(special).to(dev), bank=BANK).cpu().numpy()
        one = eng.pair_cosine(torch.from_numpy(P[:1]).to(dev), bank=BANK)
        none = eng.pair_cosine(torch.empty((0, 2), dtype=torch.int32, device=dev), bank=BANK)
    assert sims.dtype == torch.float32 and tuple(sims.shape) == (len(P),) and tuple(none.shape) == (0,)
    assert torch.equal(sims.view(torch.int32), again.view(torch.int32))            # bit-identical between runs
    assert torch.equal(sims.view(torch.int32), swapped.view(torch.int32))          # and for (i, j) and (j, i)
    assert torch.equal(one.view(torch.int32), sims[:1].view(torch.int32))          # whatever the launch size
    err = np.abs(sims.cpu().numpy().astype(np.float64) - validator_ref.cosine64(X64, P))
    print(f"pair_cosine D={D} {'bf16' if bf16 else 'f32'}: {len(P)} pairs, worst |sim - cos64| {err.max():.3e} = "
          f"{err.max() / bound(D):.4f} B(D) = {err.max() / kernel_bound(D):.4f} Bk(D); B(D) = {bound(D):.3e}, Bk(D) = {kernel_bound(D):.3e}")
    assert kernel_bound(D) <= bound(D)
    assert err.max() <= kernel_bound(D)                                            # the tighter bound of the kernel's own order
    assert (spec[:3] == 0).all()                                                   # a zero row: 0, with itself too
    assert np.isnan(spec[3:]).all()                                                # a NaN row; an index outside [0, R)


# ---- 4: similar_pairs with partners planted at t +- 3 B(D) ----------------------------------------------------------------
def cos64(a, b):
    return float(a @ b / np.sqrt((a @ a) * (b @ b)))


@functools.lru_cache(maxsize=None)
def planted(D, t, bf16, n_base=12, seed=5):
    """Unit rows (normalised in fp32, then rounded to bf16 for a bf16 slot): per base row an exact duplicate and two partners
    whose cosine with the base row -- measured on the operands -- lies at t + 3 B(D) and t - 3 B(D) (accepted inside
    (2 B, 4 B); a bf16 row moves in steps larger than B, so candidates are redrawn until one lands).  -> (X, [(i, j, inside)])."""
    rng = np.random.default_rng(seed)
    B = bound(D)

    def store(v):
        x = torch.from_numpy(np.asarray(v, np.float64)).float()
        x = x / torch.linalg.vector_norm(x)
        return x.bfloat16() if bf16 else x
    rows, pairs = [], []
    for _ in range(n_base):
        x = store(rng.standard_normal(D))
        x64 = operands(x[None])[0]
        xu = x64 / np.linalg.norm(x64)
        i0 = len(rows)
        rows += [x, x.clone()]
        pairs.append((i0, i0 + 1, True))
        for sign in (1.0, -1.0):
            target = t + sign * 3.0 * B
            for _attempt in range(2000):
                u = rng.standard_normal(D)
                u -= (u @ xu) * xu
                u /= np.linalg.norm(u)
                c = target
                for _ in range(6):                                               # steer until the OPERANDS are at the target
                    p = store(c * xu + np.sqrt(1 - c * c) * u)
                    got = cos64(operands(p[None])[0], x64)
                    c = min(c + target - got, 1.0 - 1e-9)
                if 2.0 * B < sign * (got - t) < 4.0 * B:
                    break
            else:
                raise AssertionError("the planting missed t +- 3 B(D)")
            rows.append(p)
            pairs += [(i0, len(rows) - 1, sign > 0), (i0 + 1, len(rows) - 1, sign > 0)]
    return torch.stack(rows), pairs


@pytest.mark.parametrize("D,bf16", [(128, False), (128, True), (512, False)], ids=["128-f32", "128-bf16", "512-f32"])
@pytest.mark.parametrize("t", [0.95, 0.85, 0.999])
def test_similar_pairs_with_planted_partners(gpu_engine, t, D, bf16):
    X, plant = planted(D, t, bf16)
    R, B = len(X), bound(D)
    X64 = operands(X)
    S64 = validator_ref.cosine64(X64)
    I, J, inside = (np.array(v) for v in zip(*plant))
    m = (S64[I, J] - t) / B
    partner = np.arange(len(plant)) % 5 != 0                                      # per base row: the duplicate, then four partner pairs
    assert (np.abs(m[partner]) > 2.0).all() and (np.abs(m[partner]) < 4.0).all() and partner.sum() == R
    assert np.array_equal(S64[I, J] >= t, inside)
    with Slot(gpu_engine, X) as eng:
        pairs, sims = eng.similar_pairs(t, bank=BANK)
    pairs, sims = pairs.cpu().numpy().astype(np.int64), sims.cpu().numpy()
    assert pairs.shape[1] == 2 and (pairs[:, 0] < pairs[:, 1]).all()
    key = pairs[:, 0] * R + pairs[:, 1]
    assert (np.diff(key) > 0).all()                                               # lexicographic, no pair twice
    G = np.zeros((R, R), bool)
    G[pairs[:, 0], pairs[:, 1]] = True
    want = np.triu(S64 >= t, 1)
    differ = G != want
    worst = float((np.abs(S64 - t)[differ] / B).max()) if differ.any() else 0.0
    err = np.abs(sims.astype(np.float64) - S64[pairs[:, 0], pairs[:, 1]]).max()
    print(f"similar_pairs t={t} D={D} {'bf16' if bf16 else 'f32'}: {len(pairs)} pairs, planted margins {np.abs(m[partner]).min():.2f} .. "
          f"{np.abs(m[partner]).max():.2f} B, {int(differ.sum())} pairs differ from fp64 (worst |cos64 - t| / B {worst:.3f}), "
          f"worst |sim - cos64| / B {err / B:.4f}")
    assert np.array_equal(G[I, J], inside)                                        # every planted pair is decided as fp64 decides it
    assert worst <= 1.0                                                           # a pair differs only inside |cos64 - t| <= B(D)
    assert err <= B and (sims >= np.float32(t)).all()


def test_similar_pairs_edge_thresholds(gpu_engine):
    X, _ = planted(128, 0.95, False)
    with Slot(gpu_engine, X) as eng:
        pairs, sims = eng.similar_pairs(1.0 + 1e-9, bank=BANK)
        assert tuple(pairs.shape) == (0, 2) and tuple(sims.shape) == (0,) and pairs.dtype == torch.int32
        for bad in (float("nan"), float("inf"), float("-inf")):
            with pytest.raises(ValueError):
                eng.similar_pairs(bad, bank=BANK)
        every, _ = eng.similar_pairs(-1.0, bank=BANK)                              # every pair has cosine >= -1
        assert len(every) == len(X) * (len(X) - 1) // 2
        with pytest.raises(ValueError, match=str(len(every))):
            eng.similar_pairs(-1.0, bank=BANK, max_pairs=10)


# ---- 5: the reference's own lists -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(GOLDEN)
    names = [str(n) for n in z["split_names"]]
    cuts = np.cumsum(z["split_sizes"])[:-1]
    splits = {n: [int(i) for i in part] for n, part in zip(names, np.split(z["split_indices"], cuts))}
    return z, names, splits


def test_validate_features_reproduces_the_reference(pkg, gpu_engine):
    """fp32 features against the reference's fp32 similarities: B(D) for the kernel, 2^-16 for the hi | lo representation of the
    stored rows (each element within 2^-18 relative), e_ref for the reference's own distance from fp64 (measured by the maker)."""
    z, names, splits = fixture()
    X = z["features"]
    tol = bound(X.shape[1]) + 2.0 ** -16 + float(z["e_ref"])
    v = pkg.DataValidator(pkg.DataValidationConfig(check_data_leakage=False), engine=gpu_engine)
    near = v.validate_features(X, threshold=float(z["near_t"]))
    assert near.total_samples == len(X) and near.potential_leakage == []
    assert [(i, j) for i, j, _ in near.near_duplicates] == [tuple(p) for p in z["near_pairs"].tolist()]
    e_near = np.abs(np.array([s for _, _, s in near.near_duplicates]) - z["near_sims"].astype(np.float64)).max()
    v = pkg.DataValidator(pkg.DataValidationConfig(check_near_duplicates=False), engine=gpu_engine)
    leak = v.validate_features(torch.from_numpy(X), split_info=splits, threshold=float(z["leak_t"]))
    got = leak.potential_leakage
    assert leak.near_duplicates == [] and all(d["type"] == "image" and set(d) == {"type", "index1", "index2", "split1", "split2", "similarity"}
                                              for d in got)
    assert [(d["index1"], d["index2"]) for d in got] == [tuple(p) for p in z["leak_idx"].tolist()]
    assert [(d["split1"], d["split2"]) for d in got] == [(names[a], names[b]) for a, b in z["leak_split"].tolist()]
    e_leak = np.abs(np.array([d["similarity"] for d in got]) - z["leak_sims"].astype(np.float64)).max()
    print(f"fixture fp32: {len(near.near_duplicates)} near duplicates, {len(got)} leaks, worst |sim - reference| {max(e_near, e_leak):.3e} "
          f"of {tol:.3e} allowed")
    assert max(e_near, e_leak) <= tol
    assert not gpu_engine.has_bank(v.bank_name)                                   # the temporary slot is released


def test_validate_features_on_a_bf16_copy(pkg, gpu_engine):
    """the bf16 copy of the normalised features is searched as it stands: the lists are fp64's on the bf16 VALUES"""
    z, names, splits = fixture()
    X = torch.from_numpy(z["features"])
    Xb = (X / torch.linalg.vector_norm(X, dim=1, keepdim=True)).bfloat16()
    X64 = Xb.double().numpy()
    B = bound(X.shape[1])
    S64 = validator_ref.cosine64(X64)
    v = pkg.DataValidator(pkg.DataValidationConfig(), engine=gpu_engine)
    for t in (float(z["near_t"]), float(z["leak_t"])):
        assert np.abs(S64[np.triu_indices(len(X64), 1)] - t).min() > B            # no pair of the copy is inside the band
        res = v.validate_features(Xb, split_info=splits, threshold=t)
        P, sims = validator_ref.near_duplicates(X64, t)
        assert [(i, j) for i, j, _ in res.near_duplicates] == [tuple(p) for p in P.tolist()]
        assert np.abs(np.array([s for _, _, s in res.near_duplicates]) - sims).max() <= B
        want = validator_ref.leakage(X64, splits, t)
        strip = lambda d: {k: d[k] for k in d if k != "similarity"}
        assert [strip(d) for d in res.potential_leakage] == [strip(d) for d in want] and len(want) >= 5
        assert max(abs(a["similarity"] - b["similarity"]) for a, b in zip(res.potential_leakage, want)) <= B
    with pytest.raises(ValueError, match="unit rows"):
        v.validate_features((3.0 * Xb.float()).bfloat16())


def test_validator_slot_errors(pkg, gpu_engine):
    v = pkg.DataValidator(pkg.DataValidationConfig(), engine=gpu_engine)
    with pytest.raises(ValueError, match="131072"):
        v._similar_pairs(torch.empty((131073, 64), dtype=torch.bfloat16, device="meta"), 0.95)
    eng = pkg.TVCEngine(device="cuda:0")
    try:
        rows = torch.nn.functional.normalize(torch.randn(8, 64), dim=1)
        for k in range(pkg._lib.TVC_MAX_BANKS):
            eng.set_bank(rows.to(eng.device), name=f"held-{k}")
        with pytest.raises(RuntimeError, match="free bank slot"):
            pkg.DataValidator(pkg.DataValidationConfig(), engine=eng).validate_features(rows)
        eng.release_bank("held-0")
        assert pkg.DataValidator(pkg.DataValidationConfig(), engine=eng).validate_features(rows).near_duplicates == []
    finally:
        eng.close()


# ---- 6: ValidationResult end to end ---------------------------------------------------------------------------------------
def test_validate_dataset_end_to_end(pkg, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(11)
    clip = pkg.CLIPModel(pkg.CLIPConfig(model_name="ViT-T/16-test", device="cuda"))
    try:
        base = [rng.integers(0, 256, (64, 64, 3), dtype=np.uint8) for _ in range(14)]
        near = [np.clip(base[k].astype(np.int16) + rng.integers(-6, 7, base[k].shape), 0, 255).astype(np.uint8) for k in (0, 1, 2)]
        imgs = base + near + [base[3].copy(), base[4].copy()]                      # 19 images: 3 near copies, 2 exact copies
        images = [Image.fromarray(a) for a in imgs] + [Image.new("RGB", (16, 16), (9, 9, 9))]
        texts = [f"caption number {i}" for i in range(len(images))]
        texts[6], texts[9] = texts[5], "abc"                                       # a repeated text, a short text
        n = len(images)
        split_info = {"train": list(range(0, 12)), "val": [12, 13, 14, 15], "test": [16, 17, 18, 19, 3, 99]}

        def run(t):
            cfg = pkg.DataValidationConfig(clip_model="ViT-T/16-test", image_similarity_threshold=t, encode_batch_size=8,
                                           report_dir=str(tmp_path))
            v = pkg.DataValidator(cfg, clip_model=clip)
            return v, v.validate_dataset(images, texts, labels=[i % 3 for i in range(n)], split_info=split_info)
        v0, _ = run(0.95)
        F = v0.last_features.cpu()
        assert tuple(F.shape) == (n, 128) and v0.last_valid_indices == list(range(n))
        # the threshold sits in the middle of the widest gap of the cosines the engine's own features have among the 40 largest
        S64 = validator_ref.cosine64(F.double().numpy())
        c = np.sort(S64[np.triu_indices(n, 1)])[::-1][:40]
        k = int(np.argmax(c[:-1] - c[1:]))
        t = float((c[k] + c[k + 1]) / 2)
        assert c[k] - c[k + 1] > 100 * bound(128), "no usable gap in the toy tower's cosines"
        v, res = run(t)
        assert torch.equal(v.last_features.cpu(), F)                               # the features do not depend on the run
        P, sims = validator_ref.near_duplicates(F.double().numpy(), t)
        leaks = validator_ref.leakage(F.double().numpy(), split_info, t)
        print(f"end to end: t = {t:.6f} (gap {c[k] - c[k + 1]:.3e}), {len(P)} near duplicates, {len(leaks)} leaks, "
              f"{len(res.exact_duplicates)} exact duplicates, score {res.overall_score}")
        assert len(P) == k + 1 and [(i, j) for i, j, _ in res.near_duplicates] == [tuple(p) for p in P.tolist()]
        assert np.abs(np.array([s for _, _, s in res.near_duplicates]) - sims).max() <= bound(128) + 2.0 ** -16 + 2.0 ** -22
        strip = lambda d: {key: d[key] for key in d if key != "similarity"}
        assert [strip(d) for d in res.potential_leakage] == [strip(d) for d in leaks]
        assert any(d["index1"] == 3 and d["index2"] == 3 for d in res.potential_leakage)
        assert res.total_samples == n and res.valid_samples == n - 2 and res.invalid_samples == 2
        assert (5, 6) in res.exact_duplicates and (3, 17) in res.exact_duplicates and (4, 18) in res.exact_duplicates
        assert res.overall_score == validator_ref.score(n, n - 2, len(res.exact_duplicates), len(P), len(leaks))
        assert len(list(tmp_path.glob("validation_report_*.json"))) >= 1
        out = v.validate_splits((images[:8], texts[:8]), (images[8:12], texts[8:12]), (images[12:], texts[12:]))
        assert out["split_stats"]["train_size"] == 8 and out["split_stats"]["test_ratio"] == (n - 12) / n
        assert isinstance(out["validation_result"], pkg.ValidationResult)
        assert not clip.engine.has_bank(v.bank_name)
    finally:
        clip.engine.close()
