"""Writes tests/golden/data_validator.npz with the REFERENCE's own code (not collected by pytest; the only file that reads the
reference):

    python tests/make_validator_fixture.py <checkout of Zhang-Xin-Duke/multimodal-detection-consistency>

``src/evaluation/data_validator.py`` is loaded by path under a synthetic package whose ``models`` module is a stand-in (the
validator only constructs a CLIP model when ``use_clip_features`` is set, and it is not set here) and whose
``utils.metrics`` is the reference's own file.  ``validator.clip_model`` is then a stub whose ``encode_image`` returns the
feature row named by the pixel value of a 1 x 1 PIL image, and the reference's own ``_detect_near_duplicates`` and
``_detect_data_leakage`` run over those "images".

Inputs: 120 rows x 96 features (not a multiple of 64: the validator pads) of random norm, with planted exact duplicates, a
scaled copy, near copies on both sides of each threshold (the closest 3e-4 away), partners in different splits, an index
listed in two splits and one beyond the dataset.  No pair lies within 1e-4 of a threshold in fp64 (asserted), so the
reference's own fp32 rounding decides no pair.  The file holds arrays only: the features, the thresholds, the split lists, the
reference's pair lists and fp32 similarities, and e_ref = the reference's largest distance from fp64 on the listed pairs."""
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import validator_ref  # noqa: E402

N, D = 120, 96
NEAR_T, LEAK_T = 0.95, 0.9
SPLITS = {"train": list(range(0, 70)) + [100], "val": list(range(70, 95)), "test": list(range(95, 120)) + [5, 400]}


def load_reference(root: Path):
    src = root / "src"
    for name in ("refpkg", "refpkg.utils", "refpkg.evaluation"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    models = types.ModuleType("refpkg.models")
    models.CLIPModel = type("CLIPModel", (), {})
    models.CLIPConfig = type("CLIPConfig", (), {})
    sys.modules["refpkg.models"] = models

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    load("refpkg.utils.metrics", src / "utils" / "metrics.py")
    return load("refpkg.evaluation.data_validator", src / "evaluation" / "data_validator.py")


def features():
    rng = np.random.default_rng(20)
    X = rng.standard_normal((N, D))
    X *= (10.0 ** rng.uniform(-1, 1, N))[:, None]               # the reference normalises: the norms must not matter

    def partner(i, c):
        """a row at cosine exactly c (fp64) to row i, of another norm"""
        x = X[i] / np.linalg.norm(X[i])
        u = rng.standard_normal(D)
        u -= (u @ x) * x
        u /= np.linalg.norm(u)
        return (c * x + np.sqrt(1 - c * c) * u) * 10.0 ** rng.uniform(-1, 1)
    X[11] = X[3]                                                # exact duplicate, same split
    X[80] = X[3]                                                # exact duplicate across splits
    X[96] = 3.7 * X[20]                                         # scaled copy across splits
    for j, (i, c) in {12: (7, 0.99), 13: (8, 0.9503), 14: (9, 0.9497), 15: (10, 0.93),           # around NEAR_T, inside train
                      97: (30, 0.97), 98: (31, 0.9503), 99: (32, 0.9497),                        # train / test around NEAR_T
                      71: (40, 0.92), 72: (41, 0.9003), 73: (42, 0.8997), 74: (43, 0.85),        # train / val around LEAK_T
                      110: (75, 0.91), 111: (76, 0.89)}.items():                                 # val / test around LEAK_T
        X[j] = partner(i, c)
    return X.astype(np.float32)


def main():
    ref = load_reference(Path(sys.argv[1]))
    from PIL import Image
    X = features()
    S64 = validator_ref.cosine64(X)
    iu = np.triu_indices(N, 1)
    for t in (NEAR_T, LEAK_T):
        assert np.abs(S64[iu] - t).min() > 1e-4, "a pair of the fixture lies within 1e-4 of a threshold"

    class Stub:
        def encode_image(self, img):
            return X[img.getpixel((0, 0))]
    images = [Image.new("I", (1, 1), i) for i in range(N)]
    texts = [f"text {i}" for i in range(N)]

    def validator(t):
        v = ref.DataValidator(ref.DataValidationConfig(image_similarity_threshold=t, use_clip_features=False, use_tfidf=False,
                                                       save_reports=False))
        v.clip_model = Stub()
        return v
    near = ref.ValidationResult(total_samples=N)
    validator(NEAR_T)._detect_near_duplicates(images, texts, near)
    leak = ref.ValidationResult(total_samples=N)
    validator(LEAK_T)._detect_data_leakage(images, texts, SPLITS, leak)
    assert len(near.near_duplicates) >= 6 and len(leak.potential_leakage) >= 6
    assert all(d["type"] == "image" for d in leak.potential_leakage)

    near_pairs = np.array([(i, j) for i, j, _ in near.near_duplicates], np.int64)
    near_sims = np.array([s for _, _, s in near.near_duplicates], np.float32)
    names = list(SPLITS)
    leak_idx = np.array([(d["index1"], d["index2"]) for d in leak.potential_leakage], np.int64)
    leak_split = np.array([(names.index(d["split1"]), names.index(d["split2"])) for d in leak.potential_leakage], np.int64)
    leak_sims = np.array([d["similarity"] for d in leak.potential_leakage], np.float32)
    e_ref = max(np.abs(near_sims - S64[near_pairs[:, 0], near_pairs[:, 1]]).max(),
                np.abs(leak_sims - S64[leak_idx[:, 0], leak_idx[:, 1]]).max())
    out = HERE / "golden" / "data_validator.npz"
    np.savez_compressed(out, features=X, near_t=np.float64(NEAR_T), leak_t=np.float64(LEAK_T),
                        split_names=np.array(names), split_sizes=np.array([len(SPLITS[n]) for n in names], np.int64),
                        split_indices=np.concatenate([np.array(SPLITS[n], np.int64) for n in names]),
                        near_pairs=near_pairs, near_sims=near_sims, leak_idx=leak_idx, leak_split=leak_split, leak_sims=leak_sims,
                        e_ref=np.float64(e_ref))
    print(f"{out}: {len(near_pairs)} near-duplicate pairs, {len(leak_idx)} leaks, e_ref = {e_ref:.3e}")


if __name__ == "__main__":
    main()
