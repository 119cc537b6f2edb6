#!/usr/bin/env python3
"""Writes tests/golden/fsta_sma_t16.npz: what the reference's own FSTA and SMA loops do on the toy tower.

TEST INFRASTRUCTURE ONLY, not collected by pytest; run once on a CPU (seconds), with a checkout of the reference project:

    python tests/make_attack_fixture.py /path/to/multimodal-detection-consistency

The only file that reads the reference.  It loads src/attacks/fsta_attack.py and src/attacks/sma_attack.py by path at run
time (they need torch, numpy and tqdm) and hands them a stand-in ``clip_model`` over oracle/clip_oracle.py with
``synth.make_clip_weights(ViT-T/16-test, seed=0)``; nothing of the reference is copied here.  Three loops on 4 images
drawn U[0, 1] (64 x 64):

  fsta     FSTAAttacker._fsta_attack, default config
  sma      SMAAttacker._batch_sma_attack, default config, named targets
  fsta_l2  FSTAAttacker._fsta_attack with norm_type='l2', feature_distance_metric='euclidean', and epsilon / learning_rate
           chosen so that the perturbation of at least one image ends on the L2 ball (checked below)

The file holds arrays only: the clean images, the text and target rows, and per run the final images, the config values
used (<run>_cfg_<field>), and for SMA the per-image success flags and scores.
"""
import importlib
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
OUT = ROOT / "tests" / "golden" / "fsta_sma_t16.npz"

MODEL, B = "ViT-T/16-test", 4
SEED_W, SEED_IMG, SEED_TOK_TEXT, SEED_TOK_TARGET = 0, 31, 32, 33
L2_EPSILON, L2_LEARNING_RATE = 0.5, 2.0


def load(path: Path, name: str):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class StubClip:
    """The ``clip_model`` the reference's attackers call: unit image rows from the CPU oracle tower (differentiable), text
    rows looked up by string."""

    def __init__(self, vw, arch, rows):
        self.vw, self.arch, self.rows = vw, arch, rows

    def to(self, device):
        return self

    def encode_image(self, x):
        from oracle import clip_oracle
        return clip_oracle.vision_forward(self.vw, x, self.arch.vision.heads, self.arch.patch)

    def encode_text(self, texts):
        return torch.stack([self.rows[s] for s in texts])


def main():
    import attack_ref
    from oracle import clip_oracle
    ref = Path(sys.argv[1])
    fsta = load(ref / "src" / "attacks" / "fsta_attack.py", "ref_fsta_attack")
    sma = load(ref / "src" / "attacks" / "sma_attack.py", "ref_sma_attack")
    pkg = importlib.import_module("multimodal-detection-consistency_amd")
    torch.manual_seed(0)
    arch = pkg.get_arch(MODEL)
    vw, tw = pkg.synth.make_clip_weights(arch, seed=SEED_W)
    clean = torch.rand((B, 3, arch.image_size, arch.image_size), generator=torch.Generator().manual_seed(SEED_IMG))
    with torch.no_grad():
        text = clip_oracle.text_forward(tw, pkg.synth.make_tokens(B, 0, arch.ctx, seed=SEED_TOK_TEXT)[:, 0].long(), arch.text.heads)
        target = clip_oracle.text_forward(tw, pkg.synth.make_tokens(B, 0, arch.ctx, seed=SEED_TOK_TARGET)[:, 0].long(), arch.text.heads)
    texts, targets = [f"text {i}" for i in range(B)], [f"target {i}" for i in range(B)]
    rows = {**{s: text[i] for i, s in enumerate(texts)}, **{s: target[i] for i, s in enumerate(targets)}}
    clip = StubClip(vw, arch, rows)
    out = {"clean": clean.numpy(), "text": text.numpy(), "target": target.numpy()}

    def record(run, cfg):
        for k in attack_ref.FIXTURE_FIELDS[run]:
            out[f"{run}_cfg_{k}"] = np.asarray(getattr(cfg, k))

    cfg = fsta.FSTAAttackConfig(device="cpu", enable_cache=False)
    out["fsta_adv"] = fsta.FSTAAttacker(clip, cfg)._fsta_attack(clean, text, target).numpy()
    record("fsta", cfg)

    cfg = sma.SMAAttackConfig(device="cpu", enable_cache=False)
    res = sma.SMAAttacker(clip, cfg)._batch_sma_attack(clean, texts, targets)
    out["sma_adv"] = torch.stack([r["adversarial_images"].detach() for r in res]).numpy()
    out["sma_success"] = np.asarray([r["success_rate"] > 0.5 for r in res])
    out["sma_score"] = np.asarray([r["semantic_misalignment_score"] for r in res], dtype=np.float32)
    record("sma", cfg)

    cfg = fsta.FSTAAttackConfig(device="cpu", enable_cache=False, norm_type="l2", feature_distance_metric="euclidean",
                                epsilon=L2_EPSILON, learning_rate=L2_LEARNING_RATE)
    adv = fsta.FSTAAttacker(clip, cfg)._fsta_attack(clean, text, target)
    out["fsta_l2_adv"] = adv.numpy()
    record("fsta_l2", cfg)
    dn = (adv - clean).flatten(1).norm(dim=1)
    print("fsta_l2 |adv - clean|_2 per image:", dn.tolist(), "epsilon", L2_EPSILON)
    # on the ball: the projection was active at the end (the pixel clamp after it can only shorten the perturbation a little)
    assert (dn > 0.99 * L2_EPSILON).any() and (dn <= L2_EPSILON * (1 + 1e-6)).all(), "choose epsilon / learning_rate so that an image ends on the L2 ball"

    with torch.no_grad():
        f0 = clip.encode_image(clean)
        cos = torch.nn.functional.cosine_similarity
        base = (cos(f0, target) - cos(f0, text)).mean().item()
        for run in attack_ref.FIXTURE_RUNS:
            f1 = clip.encode_image(torch.from_numpy(out[f"{run}_adv"]))
            print(f"{run}: mean(cos target - cos text) {base:.4f} -> {(cos(f1, target) - cos(f1, text)).mean().item():.4f}; "
                  f"max |adv - clean| {np.abs(out[f'{run}_adv'] - out['clean']).max():.4f}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size / 1e3:.0f} kB), arrays: {sorted(out)}")


if __name__ == "__main__":
    main()
