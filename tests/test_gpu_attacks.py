"""GPU: the FSTA / SMA attacks -- the feature-loss gradient kernel and the step kernel against the fp64 restatement
(tests/attack_ref.py), the two attackers' loops against the committed fixture of the reference's own loops
(tests/golden/fsta_sma_t16.npz), and the public surface.

Bounds.  feature grad: |got - ref64| <= 2^-24 (D + 16) A, the classical bound of an fp32 sum of D terms plus the handful of
operations after it; A (attack_ref.feature_grad) is the per-element sum of the absolute values of the addends, every
coefficient c replaced by sum_c |x_c y_c|.  step: the momentum within 2^-22 (|mu m| + |grad| + |p (adv - clean)|) of fp64; the
L-inf image bit-equal to the fp32 formula evaluated from the kernel's own momentum (an exact product, fp32 additions, min and
max); the L2 image within 2^-19 (|clean| + |adv| + |lr m| + |d|), the form of test_pgd_and_l2_step_small_and_ragged_images (one
block sum of at most 4 terms per thread, 6 shuffle levels and 16 partial sums, halved by its square root)."""
from pathlib import Path

import numpy as np
import pytest
import torch

import attack_ref
from oracle import clip_oracle

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "fsta_sma_t16.npz"
f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))


# ---- tvc_attack_feature_grad -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("B,D", attack_ref.SHAPES)
def test_feature_grad_vs_fp64_restatement(gpu_engine, B, D, metric):
    eng = gpu_engine
    f, t, g = attack_ref.make_rows(B, D, torch.float32)
    W = {k: f32(v) for k, v in attack_ref.WEIGHTS.items()}
    want, rows, A, A_rows = attack_ref.feature_grad(f.double(), t.double(), g.double(), metric=metric, **W)
    got, got_rows = eng.attack_feature_grad(f.cuda(), t.cuda(), g.cuda(), metric=metric, **W)
    again, again_rows = eng.attack_feature_grad(f.cuda(), t.cuda(), g.cuda(), metric=metric, **W)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)) and torch.equal(got_rows.view(torch.int32), again_rows.view(torch.int32))
    assert got.shape == (B, D) and got_rows.shape == (B, 4)
    u = 2.0 ** -24 * (D + 16)
    err, err_rows = (got.cpu().double() - want).abs(), (got_rows.cpu().double() - rows).abs()
    tiny = torch.finfo(torch.float64).tiny
    worst = (err / (u * A).clamp_min(tiny)).max().item()
    worst_rows = (err_rows / (u * A_rows).clamp_min(tiny)).max().item()
    print(f"[measured] attack_feature_grad B={B} D={D} {metric}: worst |got - ref| / (2^-24 (D + 16) A) = {worst:.4f} (grad), "
          f"{worst_rows:.4f} (loss_rows); max |got - ref| / max |grad| = {err.max().item() / want.abs().max().item():.2e}")
    assert (err <= u * A).all()
    assert (err_rows <= u * A_rows).all()
    if metric == "euclidean":
        assert got_rows[0, 0].item() == 0.0                        # f_0 == g_0: the distance is 0 and its term's gradient 0, not NaN
    if B == 1:
        assert got_rows[0, 3].item() == 0.0                        # no division by B - 1
    assert torch.isfinite(got).all() and torch.isfinite(got_rows).all()


def test_feature_grad_zero_weights_and_nan_rows(gpu_engine):
    """A weight of 0 takes its term out (against the restatement without it), and a NaN row poisons what the formulas say:
    its own gradient row always, the other rows through S only -- their loss_rows column 3 always, their gradient only when
    w_div != 0."""
    eng = gpu_engine
    B, D = 5, 512
    f, t, g = attack_ref.make_rows(B, D, torch.float32)
    u = 2.0 ** -24 * (D + 16)
    for W in (dict(a_tgt=-2.0, a_txt=0.0, w_out=0.0, w_div=0.0), dict(a_tgt=0.0, a_txt=0.0, w_out=0.25, w_div=0.0),
              dict(a_tgt=0.0, a_txt=0.0, w_out=0.0, w_div=0.5), dict(a_tgt=0.0, a_txt=0.0, w_out=0.0, w_div=0.0)):
        want, _, A, _ = attack_ref.feature_grad(f.double(), t.double(), g.double(), **W)
        got, _ = eng.attack_feature_grad(f.cuda(), t.cuda(), g.cuda(), **W)
        assert ((got.cpu().double() - want).abs() <= u * A).all(), W
    fn = f.clone()
    fn[3, 7] = float("nan")
    W = dict(a_tgt=-1.0, a_txt=1.0, w_out=0.1)
    base, base_rows = eng.attack_feature_grad(f.cuda(), t.cuda(), g.cuda(), w_div=0.0, **W)
    got, rows = eng.attack_feature_grad(fn.cuda(), t.cuda(), g.cuda(), w_div=0.0, **W)
    others = [0, 1, 2, 4]
    assert torch.isnan(got[3]).all() and torch.isnan(rows[3]).all()
    assert torch.equal(got[others].view(torch.int32), base[others].view(torch.int32))
    assert torch.equal(rows[others, :3].view(torch.int32), base_rows[others, :3].view(torch.int32)) and torch.isnan(rows[:, 3]).all()
    got, _ = eng.attack_feature_grad(fn.cuda(), t.cuda(), g.cuda(), w_div=0.05, **W)
    assert torch.isnan(got).all()
    with pytest.raises(ValueError):
        eng.attack_feature_grad(f.cuda(), t.cuda(), g.cuda(), a_tgt=1.0, a_txt=1.0, metric="manhattan")
    with pytest.raises(ValueError):
        eng.attack_feature_grad(f.cuda(), t.cuda()[:, :100], g.cuda(), a_tgt=1.0, a_txt=1.0)


# ---- tvc_attack_step -------------------------------------------------------------------------------------------------
def _step_inputs(n: int):
    """B = 3: image 0 stays inside the ball, image 1 starts outside it, image 2 sits on the clean image with an all-zero gradient
    and zero momentum (sign 0; an L2 norm of 0 against the 1e-8)."""
    g0 = torch.Generator().manual_seed(70 + n)
    B = 3
    clean = torch.rand((B, n), generator=g0) * 0.5 + 0.25
    grad = torch.randn((B, n), generator=g0) * 1e-3
    mom = torch.randn((B, n), generator=g0) * 1e-3
    adv = clean + (torch.rand((B, n), generator=g0) - 0.5) * 0.01
    adv[1] = clean[1] + 0.05 * torch.where(torch.rand(n, generator=g0) < 0.5, -1.0, 1.0)
    adv[2], grad[2], mom[2] = clean[2], 0.0, 0.0
    return clean, adv, grad, mom


def _t(v):
    return torch.tensor(v, dtype=torch.float32)


@pytest.mark.parametrize("n", [1, 1023, 1025, 4096])
def test_attack_step_vs_formula(gpu_engine, n):
    """One element, one short of and one past 1024 (the scalar path: 3 n is no multiple of 4), and 4096 (the 16-byte path)."""
    eng = gpu_engine
    clean, adv, grad, mom = _step_inputs(n)
    mu, lr, lo, hi = 0.9, 0.01, 0.0, 1.0
    worst_m, worst_l2 = 0.0, 0.0
    for norm in ("inf", "l2"):
        eps = 8 / 255 if norm == "inf" else 0.02 * n ** 0.5
        lr = 0.01 if norm == "inf" else 2.0
        for p in (0.0, 0.05):
            for clip in (0.0, 5e-4):
                a, m = adv.clone().cuda(), mom.clone().cuda()
                eng.attack_step(a, clean.cuda(), grad.cuda(), m, eps, lr, mu, clip, p, lo, hi, norm)
                a, m = a.cpu(), m.cpu()
                # momentum against fp64 (the scalars as the kernel receives them)
                pix = f32(p) * (adv.double() - clean.double())
                g64 = grad.double() + pix
                if clip > 0:
                    g64 = g64.clamp(-f32(clip), f32(clip))
                    if n > 1:                                       # the clamp is active, and not everywhere
                        assert (g64.abs() == f32(clip)).any() and (g64.abs() < f32(clip)).any()
                m64 = f32(mu) * mom.double() + g64
                S = 2.0 ** -22 * ((f32(mu) * mom.double()).abs() + grad.double().abs() + pix.abs())
                err = (m.double() - m64).abs()
                assert (err <= S).all(), f"momentum n={n} {norm} p={p} clip={clip}"
                worst_m = max(worst_m, (err / S.clamp_min(1e-300)).max().item())
                assert (m[2] == 0).all() and torch.equal(a[2].view(torch.int32), clean[2].view(torch.int32))
                if norm == "inf":
                    # the image from the kernel's own momentum: the fp32 formula, bit for bit
                    w = adv - _t(lr) * m.sign()
                    dl = torch.minimum(torch.maximum(w - clean, _t(-eps)), _t(eps))
                    want = torch.minimum(torch.maximum(clean + dl, _t(lo)), _t(hi))
                    assert torch.equal(a.view(torch.int32), want.view(torch.int32)), f"inf n={n} p={p} clip={clip}"
                    assert ((want[0] - clean[0]).abs() < eps * 0.999).all() and ((want[1] - clean[1]).abs() > eps * 0.999).all()
                else:
                    c64 = clean.double()
                    stepv = f32(lr) * m.double()
                    d = adv.double() - stepv - c64
                    dn = d.norm(dim=1, keepdim=True)
                    factor = torch.clamp(f32(eps) / (dn + f32(1e-8)), max=1.0)
                    want = (c64 + d * factor).clamp(lo, hi)
                    S2 = 2.0 ** -19 * (c64.abs() + adv.double().abs() + stepv.abs() + d.abs())
                    err2 = (a.double() - want).abs()
                    assert (err2 <= S2).all(), f"l2 n={n} p={p} clip={clip}: {(err2 - S2).max().item():.3e} over"
                    worst_l2 = max(worst_l2, (err2 / S2).max().item())
                    assert dn[0].item() < eps < dn[1].item() and factor[0].item() == 1.0 and dn[2].item() == 0.0
                    assert ((want[1] - c64[1]).norm() - eps).abs().item() < 1e-6 * eps + 1e-9              # projected onto the ball
    print(f"[measured] attack_step n={n}: inf image bit-equal; momentum worst {worst_m:.3f} of 2^-22 M; l2 image worst {worst_l2:.3f} of 2^-19 M")


@pytest.mark.parametrize("norm", ["inf", "l2"])
def test_attack_step_without_its_optional_terms(gpu_engine, norm):
    """p = 0 and clip = 0 leave their operation out: the step is, bit for bit, the fp32 chain without them.  mu = 0.5 makes
    mu * m exact, so that chain has one rounding per element whatever the instruction selection; the negative clip of "no
    clamp" gives the same bits as 0."""
    eng = gpu_engine
    n = 4096
    clean, adv, grad, mom = _step_inputs(n)
    eps, lr, mu = (8 / 255, 0.01, 0.5) if norm == "inf" else (0.02 * n ** 0.5, 2.0, 0.5)
    a, m = adv.clone().cuda(), mom.clone().cuda()
    eng.attack_step(a, clean.cuda(), grad.cuda(), m, eps, lr, mu, 0.0, 0.0, 0.0, 1.0, norm)
    a2, m2 = adv.clone().cuda(), mom.clone().cuda()
    eng.attack_step(a2, clean.cuda(), grad.cuda(), m2, eps, lr, mu, -1.0, 0.0, 0.0, 1.0, norm)
    assert torch.equal(a.view(torch.int32), a2.view(torch.int32)) and torch.equal(m.view(torch.int32), m2.view(torch.int32))
    want_m = _t(mu) * mom + grad
    assert torch.equal(m.cpu().view(torch.int32), want_m.view(torch.int32))
    if norm == "inf":
        w = adv - _t(lr) * want_m.sign()
        dl = torch.minimum(torch.maximum(w - clean, _t(-eps)), _t(eps))
        want = torch.minimum(torch.maximum(clean + dl, _t(0.0)), _t(1.0))
        assert torch.equal(a.cpu().view(torch.int32), want.view(torch.int32))
    # mu = 0: the momentum is the gradient's bits
    a, m = adv.clone().cuda(), mom.clone().cuda()
    eng.attack_step(a, clean.cuda(), grad.cuda(), m, eps, lr, 0.0, 0.0, 0.0, 0.0, 1.0, norm)
    assert torch.equal(m.cpu()[:2].view(torch.int32), grad[:2].view(torch.int32))
    with pytest.raises(ValueError):
        eng.attack_step(a, clean.cuda(), grad.cuda(), None, eps, lr, mu, 0.0, 0.0, 0.0, 1.0, norm)
    with pytest.raises(ValueError):
        eng.attack_step(a, clean.cuda(), grad.cuda(), m, eps, lr, mu, 0.0, 0.0, 0.0, 1.0, "l1")


# ---- the loops against the fixture -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy_clip(pkg):
    arch = pkg.get_arch("ViT-T/16-test")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    clip = pkg.CLIPModel(pkg.CLIPConfig(model_name=arch.name), weights=(vw, tw))
    yield clip, arch, vw
    clip.engine.close()


@pytest.fixture(scope="module")
def fixture_runs(pkg, toy_clip):
    """The three runs of the fixture on the HIP path, and the CPU oracle tower's view of every image set: computed once."""
    A = pkg.attacks
    clip, arch, vw = toy_clip
    z = np.load(GOLDEN)
    clean, text, target = (torch.from_numpy(z[k]) for k in ("clean", "text", "target"))
    cos = torch.nn.functional.cosine_similarity

    def margin(x):                                                  # per image cos(., target) - cos(., text), CPU oracle tower
        with torch.no_grad():
            f = clip_oracle.vision_forward(vw, x, arch.vision.heads, arch.patch)
        return cos(f, target) - cos(f, text)

    out = {"clean": clean, "margin_clean": margin(clean)}
    for run in attack_ref.FIXTURE_RUNS:
        cfg = attack_ref.fixture_config(z, run)
        names = {k: cfg[k] for k in cfg if k not in ("num_iter",)}
        flags = None
        if run == "sma":
            atk = A.SMAAttacker(clip, A.SMAAttackConfig(num_iter=int(cfg["num_iter"]), enable_cache=False, **names))
            got = atk._loop(clean.cuda(), text.cuda(), target.cuda(), "batch")
            flags, score = atk._judge(got, text.cuda(), target.cuda())
            flags, score = flags.cpu(), score.cpu()
        else:
            atk = A.FSTAAttacker(clip, A.FSTAAttackConfig(num_iter=int(cfg["num_iter"]), enable_cache=False, **names))
            got = atk._fsta_attack(clean, text, target)
        got = got.cpu()
        want = torch.from_numpy(z[f"{run}_adv"])
        out[run] = dict(cfg=cfg, got=got, want=want, margin_got=margin(got), margin_want=margin(want), flags=flags)
    out["sma"]["fixture_flags"] = torch.from_numpy(z["sma_success"])
    out["sma"]["fixture_score"] = torch.from_numpy(z["sma_score"])
    return out


@pytest.mark.parametrize("run", attack_ref.FIXTURE_RUNS)
def test_attack_loops_vs_fixture(fixture_runs, run):
    """Measured on an MI355X: see EXPERIMENTS.md (FSTA / SMA)."""
    r, clean = fixture_runs[run], fixture_runs["clean"]
    cfg, got, want = r["cfg"], r["got"], r["want"]
    eps = cfg["epsilon"]
    # invariants
    assert torch.isfinite(got).all()
    assert got.min().item() >= cfg["clamp_min"] and got.max().item() <= cfg["clamp_max"]
    if cfg["norm_type"] == "inf":
        assert (got - clean).abs().max().item() <= eps + 1e-6
    else:
        assert ((got - clean).flatten(1).norm(dim=1) <= eps * (1 + 1e-6)).all()
    # effect: the shift of mean(cos(adv, target) - cos(adv, text)) from the clean images, CPU oracle tower on both image sets
    m0 = fixture_runs["margin_clean"].mean().item()
    shift_got, shift_want = r["margin_got"].mean().item() - m0, r["margin_want"].mean().item() - m0
    print(f"[measured] {run} HIP vs fixture: shift of mean(cos target - cos text) {shift_got:.5f} vs {shift_want:.5f}")
    if cfg["norm_type"] == "inf":
        same = ((got - want).abs() < 1e-6).float().mean().item()
        print(f"[measured] {run} HIP vs fixture: share of pixels within 1e-6 = {same:.4f}")
    else:
        pc = torch.nn.functional.cosine_similarity((got - clean).flatten(1), (want - clean).flatten(1), dim=1)
        print(f"[measured] {run} HIP vs fixture: cosine of the two perturbations per image {[round(v, 4) for v in pc.tolist()]}")
    assert abs(shift_got - shift_want) <= 0.1 * abs(shift_want) + 1e-3
    if cfg["norm_type"] == "inf":
        assert same >= 0.85


def test_sma_success_flags_vs_fixture(fixture_runs):
    """The flags are the fixture's wherever its per-image target - text margin exceeds 5e-3 (2.5 times the tower's 2e-3
    embedding tolerance); inside that margin either flag is accepted."""
    r = fixture_runs["sma"]
    sure = r["fixture_score"].abs() > 5e-3
    print(f"[measured] sma flags: HIP {r['flags'].tolist()} fixture {r['fixture_flags'].tolist()} margins {r['fixture_score'].tolist()}")
    assert r["flags"].shape == r["fixture_flags"].shape
    assert torch.equal(r["flags"][sure], r["fixture_flags"][sure])


# ---- the public surface ----------------------------------------------------------------------------------------------
REFERENCE_KEYS = {"adversarial_images", "original_images", "success_rate", "semantic_misalignment_score", "perturbation_norm",
                  "text", "target_semantic"}
DRIVER_KEYS = {"success", "adversarial_image"}


def test_attackers_public_surface(pkg, toy_clip):
    A = pkg.attacks
    clip, arch, _ = toy_clip
    Q = 5
    clean = torch.rand((Q, 3, arch.image_size, arch.image_size), generator=torch.Generator().manual_seed(3)).cuda()
    texts = [f"a photo of thing {i}" for i in range(Q)]
    targets = [f"a drawing of item {i}" for i in range(Q)]
    for Attacker, Config, create, Presets, presets in (
            (A.FSTAAttacker, A.FSTAAttackConfig, A.create_fsta_attacker, A.FSTAAttackPresets,
             ("weak_attack", "strong_attack", "targeted_attack", "paper_config")),
            (A.SMAAttacker, A.SMAAttackConfig, A.create_sma_attacker, A.SMAAttackPresets,
             ("weak_attack", "strong_attack", "semantic_targeted_attack", "paper_config", "jpeg_robust_attack"))):
        for name in presets:
            assert isinstance(getattr(Presets, name)(), Config)
        assert isinstance(create(clip), Attacker) and isinstance(create(clip, Config(num_iter=1)).config, Config)
        for tg in (targets, None):                                  # named targets, and targets drawn from the seeded generator
            mk = lambda: Attacker(clip, Config(batch_size=2, num_iter=4, random_seed=11))
            res = mk().batch_attack(clean, texts, tg)               # 2 + 2 + 1 images
            assert len(res) == Q
            for i, d in enumerate(res):
                assert REFERENCE_KEYS | DRIVER_KEYS <= set(d)
                assert d["text"] == texts[i] and d["target_semantic"] == (tg[i] if tg else None)
                assert isinstance(d["success"], bool) and d["success_rate"] == float(d["success"])
                assert d["adversarial_image"].shape == clean.shape[1:] and d["perturbation_norm"] <= 0.031 + 1e-6
            adv = torch.stack([d["adversarial_image"] for d in res])
            pert = mk().perturb(clean, texts, tg)
            assert pert.is_cuda and torch.equal(pert.cpu().view(torch.int32), adv.view(torch.int32))      # same seed, equal bits
            assert (adv - clean.cpu()).abs().max().item() > 0.01
        atk = Attacker(clip, Config(num_iter=3))
        one = atk.attack(clean[:3], texts[:3], targets[:3])
        assert {"adversarial_images", "original_images", "success_rate", "perturbation_norm"} <= set(one)
        assert one["adversarial_images"].shape == (3, 3, arch.image_size, arch.image_size) and 0.0 <= one["success_rate"] <= 1.0
        stats = atk.get_attack_stats()
        assert stats["total_attacks"] == 3 and 0.0 <= stats["success_rate"] <= 1.0 and len(atk.cache) == 1
        atk.reset_stats()
        assert atk.get_attack_stats()["total_attacks"] == 0
    assert "semantic_misalignment_score" in A.SMAAttacker(clip, A.SMAAttackConfig(num_iter=2)).attack(clean[:2], texts[:2])
    # the L2 ball and the Euclidean metric through the attacker
    l2 = A.FSTAAttacker(clip, A.FSTAAttackConfig(num_iter=4, norm_type="l2", feature_distance_metric="euclidean", epsilon=0.5,
                                                 learning_rate=2.0)).perturb(clean, texts, targets)
    assert ((l2 - clean).flatten(1).norm(dim=1) <= 0.5 * (1 + 1e-6)).all() and l2.min() >= 0 and l2.max() <= 1
    # jpeg_compression: noise from the seeded generator, the loop keeps its invariants and is reproducible
    cfg = A.SMAAttackPresets.jpeg_robust_attack()
    cfg.num_iter, cfg.batch_size = 4, 4
    j1 = A.SMAAttacker(clip, cfg).perturb(clean, texts, targets)
    j2 = A.SMAAttacker(clip, cfg).perturb(clean, texts, targets)
    assert torch.isfinite(j1).all() and (j1 - clean).abs().max().item() <= cfg.epsilon + 1e-6 and j1.min() >= 0 and j1.max() <= 1
    assert torch.equal(j1.view(torch.int32), j2.view(torch.int32)) and (j1 - clean).abs().max().item() > 0.01
