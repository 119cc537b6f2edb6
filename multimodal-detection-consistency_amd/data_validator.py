"""``DataValidator`` (``src/evaluation/data_validator.py``) with its two all-pairs checks on the GPU.

The reference's near-duplicate check (``:353-423``) and leakage check (``:425-543``) build a dense
``cosine_similarity`` matrix ``[R, R]`` and walk it with a Python double loop over ``i < j``.  Both are pure
functions of "which pairs ``i < j`` have cosine ``>= t``, and what is that cosine", which is
``TVCEngine.similar_pairs``: the radius graph of the L2-normalised feature rows at a widened radius
(``tvc_radius_graph``), its upper triangle as a pair list in the order of the reference's loops
(``tvc_graph_pair_count`` / ``tvc_graph_pair_fill``), an fp32-grade cosine of the listed pairs
(``tvc_pair_cosine``) and the final ``>= t``.  No score matrix is ever written.

The features are registered in a temporary bank slot of the engine that is released in a ``finally``; image
features come from this package's ``CLIPModel.encode_image``, batched.  ``validate_features`` is the entry that
needs no images: it takes a feature matrix and runs the GPU part alone.

The host-only checks (quality, md5 exact duplicates, distribution statistics, the score, the recommendations, the
JSON report) are restated here from the reference's rules.

Not built: the TF-IDF text path (``use_tfidf`` defaults to ``False`` here and ``True`` raises
``NotImplementedError``), datasets over 131 072 rows (``TVC_RADIUS_MAX_ROWS``), multi-GPU.
"""
from __future__ import annotations

import hashlib
import json
import logging
import math
import time
from collections import Counter
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from .engine import TVCEngine

logger = logging.getLogger(__name__)

MAX_ROWS = 131072        # include/tvc.h: TVC_RADIUS_MAX_ROWS


@dataclass
class DataValidationConfig:
    """src/evaluation/data_validator.py:27-65; ``use_tfidf`` defaults to ``False`` here (the text path is not built)."""
    image_similarity_threshold: float = 0.95
    text_similarity_threshold: float = 0.9
    cross_modal_similarity_threshold: float = 0.85
    clustering_eps: float = 0.1
    clustering_min_samples: int = 2
    use_clip_features: bool = True
    clip_model: str = "openai/clip-vit-base-patch32"
    device: str = "cuda"
    use_tfidf: bool = False
    tfidf_max_features: int = 10000
    tfidf_ngram_range: Tuple[int, int] = (1, 3)
    check_duplicates: bool = True
    check_near_duplicates: bool = True
    check_data_leakage: bool = True
    check_distribution: bool = True
    check_quality: bool = True
    min_image_size: Tuple[int, int] = (32, 32)
    max_image_size: Tuple[int, int] = (2048, 2048)
    min_text_length: int = 5
    max_text_length: int = 1000
    save_reports: bool = True
    report_dir: Optional[str] = None
    verbose: bool = True
    # --- additions ---------------------------------------------------------
    encode_batch_size: int = 256          # images per CLIPModel.encode_image call
    max_pairs: int = 1 << 27              # nominated pairs beyond this raise instead of being truncated

    def __post_init__(self):
        for name in ("image_similarity_threshold", "text_similarity_threshold", "cross_modal_similarity_threshold"):
            v = getattr(self, name)
            if not math.isfinite(float(v)):
                raise ValueError(f"{name} must be finite (got {v})")
        if int(self.encode_batch_size) < 1:
            raise ValueError(f"encode_batch_size must be >= 1 (got {self.encode_batch_size})")
        if int(self.max_pairs) < 0:
            raise ValueError(f"max_pairs must be >= 0 (got {self.max_pairs})")
        if self.min_text_length > self.max_text_length:
            raise ValueError(f"min_text_length {self.min_text_length} exceeds max_text_length {self.max_text_length}")


@dataclass
class ValidationResult:
    """src/evaluation/data_validator.py:68-110."""
    total_samples: int = 0
    valid_samples: int = 0
    invalid_samples: int = 0
    exact_duplicates: List[Tuple[int, int]] = None
    near_duplicates: List[Tuple[int, int, float]] = None
    potential_leakage: List[Dict[str, Any]] = None
    quality_issues: List[Dict[str, Any]] = None
    distribution_stats: Dict[str, Any] = None
    clusters: Dict[str, Any] = None
    overall_score: float = 0.0
    recommendations: List[str] = None

    def __post_init__(self):
        for name in ("exact_duplicates", "near_duplicates", "potential_leakage", "quality_issues", "recommendations"):
            if getattr(self, name) is None:
                setattr(self, name, [])
        for name in ("distribution_stats", "clusters"):
            if getattr(self, name) is None:
                setattr(self, name, {})


def _open(image):
    from PIL import Image
    return Image.open(image) if isinstance(image, (str, Path)) else image


class DataValidator:
    """``DataValidator(config)`` of the reference.  ``clip_model`` / ``engine`` share an existing encoder or engine; without
    them the encoder named by the configuration is created on first use (``validate_features`` needs an engine only)."""

    def __init__(self, config: Optional[DataValidationConfig] = None, clip_model=None, engine: Optional[TVCEngine] = None):
        self.config = config or DataValidationConfig()
        if self.config.use_tfidf:
            raise NotImplementedError("use_tfidf=True: the TF-IDF text path of the reference's validator is not built in this "
                                      "package (the image path runs on the GPU; set use_tfidf=False)")
        self.clip_model = clip_model
        self._engine = engine
        self.tfidf_vectorizer = None
        self.feature_cache: Dict[Any, Any] = {}
        self.bank_name = f"data_validator:{id(self):x}"

    # -- engine and features -------------------------------------------------
    @property
    def engine(self) -> TVCEngine:
        if self._engine is None:
            self._engine = self.clip_model.engine if self.clip_model is not None else TVCEngine(device=self._device())
        return self._engine

    def _device(self) -> str:
        return "cuda:0" if self.config.device in ("cuda", "auto") else self.config.device

    def _clip(self):
        if self.clip_model is None and self.config.use_clip_features:
            from .clip import CLIPConfig, CLIPModel
            self.clip_model = CLIPModel(CLIPConfig(model_name=self.config.clip_model, device=self.config.device,
                                                   batch_size=int(self.config.encode_batch_size)))
        return self.clip_model

    def _encode_images(self, images) -> Tuple[Optional[torch.Tensor], List[int]]:
        """-> (features fp32 [n_valid, D] on the device, the indices of the images they belong to); an image that does not
        load is skipped with a warning, as the reference does."""
        clip = self._clip()
        if clip is None:
            return None, []
        bs = int(self.config.encode_batch_size)
        feats, valid = [], []
        for b0 in range(0, len(images), bs):
            batch = []
            for i in range(b0, min(b0 + bs, len(images))):
                try:
                    im = _open(images[i])
                    batch.append(im if isinstance(im, torch.Tensor) else clip.preprocess(im))
                    valid.append(i)
                except Exception as e:      # an unreadable file is a property of the data, not of the run
                    logger.warning("image %d could not be loaded: %s", i, e)
            if batch:
                feats.append(clip.encode_image(torch.stack(batch).to(clip.device), normalize=False).float())
        return (torch.cat(feats) if feats else None), valid

    def _unit_rows(self, features) -> torch.Tensor:
        """features [R, D] (tensor or array) -> fp32 device rows, L2-normalised in fp32 (an all-zero row stays zero: cosine 0 with
        everything, as sklearn's normalisation leaves it), zero columns up to a multiple of 64."""
        x = features if isinstance(features, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(features))
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"features must be [R, D] with R, D >= 1 (got {tuple(x.shape)})")
        x = x.to(self.engine.device, torch.float32)
        n = torch.linalg.vector_norm(x, dim=1, keepdim=True)
        x = x / torch.where(n == 0, torch.ones_like(n), n)
        pad = -x.shape[1] % 64
        if pad:
            x = torch.nn.functional.pad(x, (0, pad))
        return x.contiguous()

    def _similar_pairs(self, rows: torch.Tensor, t: float, groups: Optional[torch.Tensor] = None):
        """rows: unit rows [R, Dp], fp32 or bf16 -> (pairs int64 numpy [P, 2], sims fp32 numpy [P]) through a temporary slot."""
        R = rows.shape[0]
        if R > MAX_ROWS:
            raise ValueError(f"{R} rows: the validator's pair search takes at most {MAX_ROWS} rows (TVC_RADIUS_MAX_ROWS); "
                             f"larger datasets are not built")
        eng = self.engine
        try:
            try:
                eng.set_bank(rows, name=self.bank_name)
            except _lib.TVCError as e:
                if e.code == _lib.TVC_E_STATE and not eng.has_bank(self.bank_name):
                    raise RuntimeError(f"DataValidator needs one free bank slot of its engine for the feature rows and all "
                                       f"{_lib.TVC_MAX_BANKS} are in use: release_bank() one first") from e
                raise
            pairs, sims = eng.similar_pairs(t, bank=self.bank_name, groups=groups, max_pairs=int(self.config.max_pairs))
            return pairs.cpu().numpy().astype(np.int64), sims.cpu().numpy()
        finally:
            eng.release_bank(self.bank_name)

    # -- the two GPU checks ----------------------------------------------------
    def _near_duplicates(self, rows: torch.Tensor, valid: List[int], t: float, result: ValidationResult) -> None:
        """:403-415 -- every pair i < j of the feature rows with cosine >= t, in the loops' order."""
        if rows.shape[0] < 2:
            return
        pairs, sims = self._similar_pairs(rows, t)
        for (i, j), s in zip(pairs.tolist(), sims.tolist()):
            result.near_duplicates.append((valid[i], valid[j], s))

    def _leakage(self, rows: torch.Tensor, row_of: Dict[int, int], n_images: int, split_info: Dict[str, List[int]], t: float,
                 result: ValidationResult) -> None:
        """:495-535 -- the rows are concatenated split by split in ``split_info``'s own order (an index listed in two splits
        appears twice and pairs with itself across them), the group of a row is the ordinal of its split."""
        cross_rows, cross_indices, cross_splits, groups = [], [], [], []
        for g, (split_name, indices) in enumerate(split_info.items()):
            for idx in indices:
                idx = int(idx)
                if idx < n_images and idx in row_of:
                    cross_rows.append(row_of[idx]); cross_indices.append(idx); cross_splits.append(split_name); groups.append(g)
        if len(cross_rows) < 2:
            return
        dev = rows.device
        sub = rows[torch.tensor(cross_rows, dtype=torch.int64, device=dev)].contiguous()
        pairs, sims = self._similar_pairs(sub, t, groups=torch.tensor(groups, dtype=torch.int32, device=dev))
        for (i, j), s in zip(pairs.tolist(), sims.tolist()):
            result.potential_leakage.append({"type": "image", "index1": cross_indices[i], "index2": cross_indices[j],
                                             "split1": cross_splits[i], "split2": cross_splits[j], "similarity": s})

    def validate_features(self, features, split_info: Optional[Dict[str, List[int]]] = None,
                          threshold: Optional[float] = None) -> ValidationResult:
        """The GPU part alone on a feature matrix [R, D] (tensor or array; a bf16 tensor is searched as a bf16 slot of its
        own values): ``near_duplicates`` = [(i, j, cosine)] over all rows and, with ``split_info``, ``potential_leakage`` =
        the cross-split pairs, both at ``threshold`` (default: ``image_similarity_threshold``) and in the reference's order.
        The host-only fields of the result keep their defaults."""
        t = float(self.config.image_similarity_threshold if threshold is None else threshold)
        if not math.isfinite(t):
            raise ValueError(f"threshold must be finite (got {t})")
        if isinstance(features, torch.Tensor) and features.dtype == torch.bfloat16:
            # a bf16 matrix is searched as it stands (normalising would round its values a second time): unit or zero rows
            if features.dim() != 2 or features.shape[0] < 1 or features.shape[1] < 1:
                raise ValueError(f"features must be [R, D] with R, D >= 1 (got {tuple(features.shape)})")
            rows = features.to(self.engine.device)
            norms = torch.linalg.vector_norm(rows.float(), dim=1)
            if not bool((((norms - 1).abs() <= 2.0 ** -7) | (norms == 0)).all()):
                raise ValueError("bf16 features must be unit rows (rounded from L2-normalised rows) or zero rows; pass fp32 "
                                 "features to have them normalised")
            pad = -rows.shape[1] % 64
            rows = (torch.nn.functional.pad(rows, (0, pad)) if pad else rows).contiguous()
        else:
            rows = self._unit_rows(features)
        n = rows.shape[0]
        result = ValidationResult(total_samples=n)
        valid = list(range(n))
        if self.config.check_near_duplicates:
            self._near_duplicates(rows, valid, t, result)
        if self.config.check_data_leakage and split_info:
            self._leakage(rows, {i: i for i in valid}, n, split_info, t, result)
        return result

    # -- the reference's entry points ------------------------------------------
    def validate_dataset(self, images: List[Any], texts: List[str], labels: Optional[List[Any]] = None,
                         split_info: Optional[Dict[str, List[int]]] = None) -> ValidationResult:
        """:169-227.  Errors of the GPU path are raised, not swallowed into an empty result."""
        cfg = self.config
        result = ValidationResult(total_samples=len(images))
        if cfg.check_quality:
            self._check_data_quality(images, texts, result)
        if cfg.check_duplicates:
            self._detect_duplicates(images, texts, result)
        want_near = cfg.check_near_duplicates and len(images) > 1
        want_leak = bool(cfg.check_data_leakage and split_info)
        if cfg.use_clip_features and (want_near or want_leak):
            feats, valid = self._encode_images(images)
            if feats is not None:
                rows = self._unit_rows(feats)
                self.last_features = feats              # the engine's own features of the valid images, [n_valid, D]
                self.last_valid_indices = valid
                t = float(cfg.image_similarity_threshold)
                if want_near:
                    self._near_duplicates(rows, valid, t, result)
                if want_leak:
                    self._leakage(rows, {idx: r for r, idx in enumerate(valid)}, len(images), split_info, t, result)
        if cfg.check_distribution:
            self._analyze_distribution(images, texts, labels, result)
        self._compute_overall_score(result)
        self._generate_recommendations(result)
        if cfg.save_reports and cfg.report_dir:
            self._save_validation_report(result)
        return result

    def validate_splits(self, train_data: Tuple[List, List], val_data: Tuple[List, List], test_data: Tuple[List, List]) -> Dict[str, Any]:
        """:748-794."""
        images = list(train_data[0]) + list(val_data[0]) + list(test_data[0])
        texts = list(train_data[1]) + list(val_data[1]) + list(test_data[1])
        n_tr, n_va, n = len(train_data[0]), len(val_data[0]), len(images)
        split_info = {"train": list(range(n_tr)), "val": list(range(n_tr, n_tr + n_va)), "test": list(range(n_tr + n_va, n))}
        result = self.validate_dataset(images, texts, split_info=split_info)
        sizes = {"train": n_tr, "val": n_va, "test": n - n_tr - n_va}
        stats: Dict[str, Any] = {f"{k}_size": v for k, v in sizes.items()}
        stats.update({f"{k}_ratio": (v / n if n else 0.0) for k, v in sizes.items()})
        return {"validation_result": result, "split_stats": stats}

    # -- host-only checks --------------------------------------------------------
    def _size_issues(self, width: int, height: int) -> List[str]:
        cfg, out = self.config, []
        if width < cfg.min_image_size[0] or height < cfg.min_image_size[1]:
            out.append(f"image too small: {width}x{height}")
        if width > cfg.max_image_size[0] or height > cfg.max_image_size[1]:
            out.append(f"image too large: {width}x{height}")
        return out

    def _check_data_quality(self, images, texts, result: ValidationResult) -> None:
        """:229-302 -- a sample is valid when its image exists, loads and is within the size limits and its text is a string
        whose stripped length is >= min_text_length and whose length is <= max_text_length."""
        cfg, valid = self.config, 0
        for i, (image, text) in enumerate(zip(images, texts)):
            issues: List[str] = []
            if isinstance(image, (str, Path)):
                if not Path(image).exists():
                    issues.append(f"image file does not exist: {image}")
                else:
                    try:
                        issues += self._size_issues(*_open(image).size)
                    except Exception as e:
                        issues.append(f"image failed to load: {e}")
            elif hasattr(image, "size") and not isinstance(image, torch.Tensor):
                issues += self._size_issues(*image.size)
            if not isinstance(text, str):
                issues.append("text is not a string")
            elif len(text.strip()) < cfg.min_text_length:
                issues.append(f"text too short: {len(text.strip())}")
            elif len(text) > cfg.max_text_length:
                issues.append(f"text too long: {len(text)}")
            if issues:
                result.quality_issues.append({"index": i, "issues": issues})
            else:
                valid += 1
        result.valid_samples = valid
        result.invalid_samples = len(images) - valid

    @staticmethod
    def _detect_duplicates(images, texts, result: ValidationResult) -> None:
        """:304-351 -- md5 of the text, then md5 of the image's 8 x 8 grey thumbnail; a repeat pairs with its first holder."""
        seen: Dict[str, int] = {}
        for i, text in enumerate(texts):
            h = hashlib.md5(text.encode()).hexdigest()
            if h in seen:
                result.exact_duplicates.append((seen[h], i))
            else:
                seen[h] = i
        seen = {}
        for i, image in enumerate(images):
            try:
                thumb = np.array(_open(image).resize((8, 8)).convert("L"))
            except Exception as e:
                logger.warning("image %d could not be hashed: %s", i, e)
                continue
            h = hashlib.md5(thumb.tobytes()).hexdigest()
            if h in seen:
                result.exact_duplicates.append((seen[h], i))
            else:
                seen[h] = i

    @staticmethod
    def _analyze_distribution(images, texts, labels, result: ValidationResult) -> None:
        """:545-615."""
        def stats(v, median=False):
            out = {"mean": float(np.mean(v)), "std": float(np.std(v)), "min": int(np.min(v)), "max": int(np.max(v))}
            if median:
                out["median"] = float(np.median(v))
            return out
        if len(texts):
            result.distribution_stats["text_length"] = stats([len(t) for t in texts], median=True)
        sizes = []
        for image in images:
            try:
                sizes.append(tuple(_open(image).size))
            except Exception:
                continue
        if sizes:
            result.distribution_stats["image_size"] = {"width": stats([s[0] for s in sizes]), "height": stats([s[1] for s in sizes])}
        if labels:
            counts = Counter(labels)
            result.distribution_stats["labels"] = {"unique_labels": len(counts), "label_distribution": dict(counts),
                                                   "most_common": counts.most_common(5)}

    @staticmethod
    def _compute_overall_score(result: ValidationResult) -> None:
        """:617-646 -- min(100, the valid share in percent) - 5 per exact duplicate - 2 per near duplicate - 10 per leak, in [0, 100]."""
        score = 100.0
        if result.total_samples > 0:
            score = min(score, result.valid_samples / result.total_samples * 100)
        score -= 5 * len(result.exact_duplicates) + 2 * len(result.near_duplicates) + 10 * len(result.potential_leakage)
        result.overall_score = max(0.0, min(100.0, score))

    @staticmethod
    def _generate_recommendations(result: ValidationResult) -> None:
        """:648-698 (the wording is this package's)."""
        rec: List[str] = []
        if result.invalid_samples > 0:
            rec.append(f"{result.invalid_samples} invalid samples: check and repair the data quality issues")
        if result.exact_duplicates:
            rec.append(f"{len(result.exact_duplicates)} exact duplicate pairs: remove the repeated samples")
        if result.near_duplicates:
            rec.append(f"{len(result.near_duplicates)} near-duplicate pairs: review them and consider removing them")
        if result.potential_leakage:
            rec.append(f"{len(result.potential_leakage)} potential leaks across splits: re-split the dataset")
        ts = result.distribution_stats.get("text_length")
        if ts and ts["std"] > ts["mean"]:
            rec.append("the text lengths are unevenly distributed: pre-process or filter the texts")
        if result.overall_score < 70:
            rec.append("low dataset quality: a full clean-up is advised")
        elif result.overall_score < 85:
            rec.append("medium dataset quality: targeted improvements are advised")
        else:
            rec.append("good dataset quality")
        result.recommendations = rec

    def _save_validation_report(self, result: ValidationResult) -> Path:
        """:700-746 -- ``validation_report_<unix time>.json`` under ``report_dir``."""
        report_dir = Path(self.config.report_dir)
        report_dir.mkdir(parents=True, exist_ok=True)
        stamp = int(time.time())
        path = report_dir / f"validation_report_{stamp}.json"
        data = {
            "timestamp": stamp,
            "config": dict(self.config.__dict__),
            "results": {
                "total_samples": result.total_samples, "valid_samples": result.valid_samples,
                "invalid_samples": result.invalid_samples, "exact_duplicates_count": len(result.exact_duplicates),
                "near_duplicates_count": len(result.near_duplicates), "potential_leakage_count": len(result.potential_leakage),
                "quality_issues_count": len(result.quality_issues), "overall_score": result.overall_score,
                "distribution_stats": result.distribution_stats, "recommendations": result.recommendations,
            },
            "details": {
                "exact_duplicates": result.exact_duplicates,
                "near_duplicates": [(i, j, float(s)) for i, j, s in result.near_duplicates],
                "potential_leakage": result.potential_leakage, "quality_issues": result.quality_issues,
            },
        }
        with open(path, "w", encoding="utf-8") as f:
            json.dump(data, f, indent=2, ensure_ascii=False, default=str)
        return path


def create_data_validator(config: Optional[DataValidationConfig] = None, **kwargs) -> DataValidator:
    """:797-810."""
    return DataValidator(config or DataValidationConfig(), **kwargs)
