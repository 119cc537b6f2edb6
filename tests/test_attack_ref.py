"""CPU: the restatement of the FSTA / SMA attacks (tests/attack_ref.py) -- its closed-form embedding gradient against fp64
autograd of the loss as the attack files write it, its three loops against the committed fixture of the reference's own
loops (tests/golden/fsta_sma_t16.npz, written by tests/make_attack_fixture.py), and the package's learning-rate function."""
from pathlib import Path

import numpy as np
import pytest
import torch

import attack_ref
from oracle import clip_oracle

GOLDEN = Path(__file__).resolve().parent / "golden" / "fsta_sma_t16.npz"
SHAPES, WEIGHTS, make_rows = attack_ref.SHAPES, attack_ref.WEIGHTS, attack_ref.make_rows


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("B,D", SHAPES)
def test_closed_form_gradient_matches_fp64_autograd(B, D, metric):
    f, t, g = make_rows(B, D)
    want = attack_ref.feature_grad_autograd(f, t, g, metric=metric, **WEIGHTS)
    got, rows, A, A_rows = attack_ref.feature_grad(f, t, g, metric=metric, **WEIGHTS)
    err = (got - want).abs().max().item()
    print(f"[measured] closed form vs fp64 autograd B={B} D={D} {metric}: max |d| {err:.2e}")
    assert err <= 1e-12
    assert (A >= got.abs() * (1 - 1e-12)).all() and (A_rows >= rows.abs() * (1 - 1e-12)).all()
    if metric == "euclidean":
        assert rows[0, 0].item() == 0.0                             # f_0 == g_0: distance 0, gradient of that term 0
    # the loss is the means of the columns of loss_rows
    sgn = -1.0 if metric == "euclidean" else 1.0
    m = rows.mean(0)
    div = m[3] / (B - 1) if B > 1 else 0.0
    loss = sgn * (WEIGHTS["a_tgt"] * m[0] + WEIGHTS["a_txt"] * m[1]) + WEIGHTS["w_out"] * m[2] + WEIGHTS["w_div"] * div
    assert abs(float(loss) - float(attack_ref.feature_loss(f, t, g, metric=metric, **WEIGHTS))) <= 1e-12
    if B == 1:
        assert rows[0, 3].item() == 0.0
    # a weight of 0 takes its term out
    only = attack_ref.feature_grad(f, t, g, metric=metric, a_tgt=WEIGHTS["a_tgt"], a_txt=0.0)[0]
    assert (only - attack_ref.feature_grad_autograd(f, t, g, metric=metric, a_tgt=WEIGHTS["a_tgt"], a_txt=0.0)).abs().max().item() <= 1e-12


@pytest.fixture(scope="module")
def fixture_loops(pkg):
    """The restatement's three loops on the fp32 CPU oracle tower, run once."""
    z = np.load(GOLDEN)
    arch = pkg.get_arch("ViT-T/16-test")
    vw, _ = pkg.synth.make_clip_weights(arch, seed=0)
    forward = lambda x: clip_oracle.vision_forward(vw, x, arch.vision.heads, arch.patch)
    clean, text, target = (torch.from_numpy(z[k]) for k in ("clean", "text", "target"))
    out = {}
    for run in attack_ref.FIXTURE_RUNS:
        cfg = attack_ref.fixture_config(z, run)
        if run == "sma":
            lrs = pkg.attacks.attack_lr_schedule(cfg["learning_rate"], cfg["num_iter"], cfg["decay_factor"], cfg["gamma_epochs"],
                                                 cfg["adaptive_step_size"])
            consts = attack_ref.loop_constants("sma_batch", cfg)
        else:
            lrs = pkg.attacks.attack_lr_schedule(cfg["learning_rate"], cfg["num_iter"], cfg["decay_factor"], 1, cfg["adaptive_step_size"])
            consts = attack_ref.loop_constants("fsta", cfg)
        out[run] = (attack_ref.run_loop(forward, clean, text, target, lrs=lrs, **consts), torch.from_numpy(z[f"{run}_adv"]), cfg)
    return clean, out


@pytest.mark.parametrize("run", attack_ref.FIXTURE_RUNS)
def test_restated_loops_reproduce_the_fixture(fixture_loops, run):
    clean, out = fixture_loops
    got, want, cfg = out[run]
    same = ((got - want).abs() < 1e-6).float().mean().item()
    print(f"[measured] restated {run} loop vs the fixture: share of pixels within 1e-6 = {same:.6f}; "
          f"max |d| = {(got - want).abs().max().item():.2e}")
    assert same >= 0.999
    if cfg["norm_type"] == "inf":
        assert (want - clean).abs().max().item() <= cfg["epsilon"] + 1e-6
    else:
        dn = (want - clean).flatten(1).norm(dim=1)
        assert (dn <= cfg["epsilon"] * (1 + 1e-6)).all() and (dn > 0.99 * cfg["epsilon"]).any()     # an image ends on the L2 ball


def test_fixture_holds_arrays_only():
    z = np.load(GOLDEN, allow_pickle=False)
    assert GOLDEN.stat().st_size < 1_000_000
    for k in z.files:
        assert z[k].dtype.kind in "fiubU", (k, z[k].dtype)
    assert z["sma_success"].shape == (4,) and z["sma_score"].shape == (4,)


def test_learning_rate_sequences(pkg):
    sched = pkg.attacks.attack_lr_schedule

    def reference(lr, n, decay, decays_after):
        out = []
        for k in range(n):
            out.append(lr)
            if decays_after(k):
                lr *= decay
        return out

    # FSTA: after every iteration when adaptive_step_size
    assert sched(0.01, 20, 0.99, 1, True) == reference(0.01, 20, 0.99, lambda k: True)
    assert sched(0.01, 20, 0.99, 1, False) == [0.01] * 20
    # SMA attack: every gamma_epochs iterations, always
    got = sched(0.01, 15, 0.95, 5, True)
    assert got == reference(0.01, 15, 0.95, lambda k: (k + 1) % 5 == 0)
    assert got[:5] == [0.01] * 5 and got[5:10] == [0.01 * 0.95] * 5 and got[10:] == [0.01 * 0.95 * 0.95] * 5
    # SMA batch core: the same, only when adaptive_step_size
    assert sched(0.01, 15, 0.95, 5, False) == [0.01] * 15
    assert sched(0.02, 0, 0.5, 1, True) == [] and sched(0.02, 1, 0.5, 1, True) == [0.02]
    # the attackers hand the loop these sequences
    A = pkg.attacks
    f = A.FSTAAttacker.__new__(A.FSTAAttacker)
    f.config = A.FSTAAttackConfig(num_iterations=7)
    assert f.config.num_iter == 7 and f._loop_kwargs("batch")["lrs"] == sched(0.01, 7, 0.99, 1, True)
    s = A.SMAAttacker.__new__(A.SMAAttacker)
    s.config = A.SMAAttackConfig(adaptive_step_size=False, clip_value=0.5, gradient_clip_value=0.25)
    ka, kb = s._loop_kwargs("attack"), s._loop_kwargs("batch")
    assert ka["lrs"] == sched(0.01, 15, 0.95, 5, True) and kb["lrs"] == [0.01] * 15
    assert ka["clip"] == 0.5 and kb["clip"] == 0.25 and ka["a_txt"] == 2.0 * 2.5 and ka["a_tgt"] == -5.0
