"""PGD and Hubness attack inner loops on the GPU.

Mirror of ``src/attacks/pgd_attack.py`` (``PGDAttackConfig`` :19-58, ``PGDAttacker`` :60-640,
``create_pgd_attacker`` :643): same constructor, ``attack`` / ``batch_attack`` / stats / cache surface, same
result dictionaries.  What runs per step is different:

* forward + input gradient = ``tvc_encode_image_grad`` + ``tvc_encode_image_backward`` (hand-written HIP; only
  d/d pixels exists, no weight gradient is ever formed);
* the loss ``mean_b cos(f_b, t_b)`` (:472-476,486-492) has the closed-form embedding gradient ``+-t_b / B`` on
  unit rows, so no autograd graph is built at all -- the kernel's own L2-normalise backward projects it;
* momentum, sign step, eps projection and clamp (:500-521) are ONE kernel (``tvc_pgd_step``), in place.

``CLIPModel.encode_image_tensor(x, requires_grad=True)`` offers the same gradient behind ``torch.autograd`` for
callers that write the loop themselves (``src/attacks/hubness_attack.py:586``).

FSTA and SMA (``src/attacks/fsta_attack.py``, ``src/attacks/sma_attack.py``) are at the end of this file: their loss couples
the rows of a batch, so its embedding gradient is a kernel of its own (``tvc_attack_feature_grad``), and their step is
another recipe (``tvc_attack_step``); the tower forward and backward between the two are the ones PGD uses.

On purpose not carried over: nn.DataParallel (:131-133; one process per GPU instead -- shard the image list across
ranks), the GradScaler branch (:452-471; the tower is bf16-MFMA / fp32-accumulate already, there is nothing to
scale), ``gradient_clip_value`` (:497-498 clips a tensor whose ``.grad`` is then never read).  The random start
draws from a seeded CPU generator (the reference uses the global device RNG, :437-442), so a run is reproducible
and equals ``oracle/synth_pgd.py`` on the same seed.
"""
from __future__ import annotations

import logging
import time
from dataclasses import dataclass, field
import random
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import torch


@dataclass
class PGDAttackConfig:
    """src/attacks/pgd_attack.py:19-58 (same names and defaults; multi-GPU / AMP fields kept for compatibility)."""
    random_seed: int = 42
    device: str = "cuda"
    epsilon: float = 8.0 / 255.0
    alpha: float = 2.0 / 255.0
    num_steps: int = 10
    targeted: bool = False
    clip_min: float = 0.0
    clip_max: float = 1.0
    momentum: float = 0.9
    use_momentum: bool = True
    batch_size: int = 32
    enable_cache: bool = True
    cache_size: int = 1000
    enable_multi_gpu: bool = False
    gpu_ids: Optional[List[int]] = None
    batch_size_per_gpu: int = 8
    num_workers: int = 4
    gradient_accumulation_steps: int = 1
    mixed_precision: bool = False
    pin_memory: bool = True
    gradient_clip_value: float = 0.0
    # batches of `batch_size` in flight at once (not in the reference): each on its own HIP stream and its own engine handle
    # (same weights), so that the launches of one batch fill the compute units the other's leave idle -- a batch of 32 images
    # is 132 output tiles in half of its GEMMs, on 256 compute units.  Every batch's arithmetic is what it is alone.
    concurrent_batches: int = 2


class PGDAttacker:
    def __init__(self, clip_model, config: Optional[PGDAttackConfig] = None):
        self.config = config or PGDAttackConfig()
        self.clip_model = clip_model
        self.engine = clip_model.engine
        self.device = clip_model.device
        self.device_ids = [self.device.index or 0]
        self._gen = torch.Generator().manual_seed(self.config.random_seed)
        self.cache: Optional[Dict[str, Any]] = {} if self.config.enable_cache else None
        self.reset_stats()

    # ---- helpers ---------------------------------------------------------------------------------
    def _to_batch(self, images) -> torch.Tensor:
        if isinstance(images, torch.Tensor):
            x = images if images.dim() == 4 else images.unsqueeze(0)
        else:
            x = torch.stack([im if isinstance(im, torch.Tensor) else self.clip_model.preprocess(im) for im in images])
        return x.to(self.device, torch.float32).contiguous()

    def _text_unit(self, texts: Sequence[str]) -> torch.Tensor:
        toks = self.clip_model.tokenize(list(texts))
        return self.clip_model.encode_tokens(toks, True)               # unit rows, on the device (:424-425)

    def _random_start(self, clean: torch.Tensor) -> torch.Tensor:
        c = self.config
        adv = clean.clone()
        if c.num_steps > 1:                                                                         # :437-442
            noise = (torch.rand(clean.shape, generator=self._gen) * 2 - 1) * c.epsilon
            adv = torch.clamp(adv + noise.to(clean.device), c.clip_min, c.clip_max)
        return adv.contiguous()

    def _engine_pool(self, n: int):
        """`n` engines (the model's own first) and as many side streams; the extra handles reference the same tower
        weights (uploaded once more: 0.6 GB for ViT-L/14) and own their workspaces / kept activations."""
        if not hasattr(self, "_pool"):
            self._pool, self._streams = [self.engine], []
        while len(self._pool) < n:
            from .engine import TVCEngine
            self._pool.append(TVCEngine(self.engine.arch, self.engine._w_host[0], None, device=str(self.device),
                                        grad_precision=self.engine.grad_precision))
        while len(self._streams) < n:
            self._streams.append(torch.cuda.Stream(self.device))
        return self._pool[:n], self._streams[:n]

    def close(self) -> None:
        """Release the extra engine handles of `concurrent_batches` (the model's own engine is the model's to close)."""
        for e in getattr(self, "_pool", [])[1:]:
            e.close()
        if hasattr(self, "_pool"):
            self._pool = self._pool[:1]

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 -- interpreter shutdown
            pass

    def _steps_concurrent(self, jobs: Sequence[Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]]) -> List[torch.Tensor]:
        """`_steps` for several batches at once, batch j on stream j / engine j; the random starts are drawn in batch
        order, so the outputs equal the sequential ones bit for bit."""
        if len(jobs) == 1:
            return [self._steps(*jobs[0])]
        c = self.config
        engines, streams = self._engine_pool(len(jobs))
        state = []
        for clean, text_f, target_f in jobs:
            adv = self._random_start(clean)
            mom = torch.zeros_like(adv) if c.use_momentum else None
            targeted = bool(c.targeted and target_f is not None)
            g_out = ((-target_f if targeted else text_f) / clean.shape[0]).contiguous()
            state.append((clean, adv, mom, g_out))
        main = torch.cuda.current_stream()
        for st in streams:
            st.wait_stream(main)
        for _ in range(c.num_steps):
            for (clean, adv, mom, g_out), eng, st in zip(state, engines, streams):
                with torch.cuda.stream(st):
                    eng.encode_image_grad(adv, True)
                    grad = eng.encode_image_backward(g_out)
                    eng.pgd_step(adv, clean, grad, mom, c.epsilon, c.alpha, c.momentum, c.clip_min, c.clip_max, c.targeted)
        for st in streams:
            main.wait_stream(st)
        return [adv for _, adv, _, _ in state]

    def _steps(self, clean: torch.Tensor, text_f: torch.Tensor, target_f: Optional[torch.Tensor],
               history: Optional[Dict[str, list]] = None) -> torch.Tensor:
        """The iteration of :452-521 / :238-302 on a device batch."""
        c = self.config
        B = clean.shape[0]
        adv = self._random_start(clean)
        mom = torch.zeros_like(adv) if c.use_momentum else None
        targeted = bool(c.targeted and target_f is not None)
        # d(loss)/d(unit embedding): loss = mean_b cos(f_b, text_b)  or  -mean_b cos(f_b, target_b)
        g_out = ((-target_f if targeted else text_f) / B).contiguous()
        for _ in range(c.num_steps):
            f = self.engine.encode_image_grad(adv, True)
            grad = self.engine.encode_image_backward(g_out)
            if history is not None:
                history["loss_history"].append(float((f * g_out).sum()))
            self.engine.pgd_step(adv, clean, grad, mom, c.epsilon, c.alpha, c.momentum, c.clip_min, c.clip_max, c.targeted)
            if history is not None:                                                                  # :293-301
                cur = self.engine.encode_image(adv, True)
                history["similarity_history"].append(float((cur * text_f).sum(-1).mean()))
                history["iterations"] += 1
        return adv

    # ---- single image (:144-340) --------------------------------------------------------------------
    def attack(self, image, text: str, target_text: Optional[str] = None) -> Dict[str, Any]:
        key = self._get_cache_key(image, text, target_text)
        if self.cache and key in self.cache:
            return self.cache[key]
        clean = self._to_batch(image if isinstance(image, torch.Tensor) else [image])
        text_f = self._text_unit([text])
        target_f = self._text_unit([target_text]) if target_text else None
        info = {"iterations": 0, "loss_history": [], "similarity_history": [], "perturbation_norm": 0.0}
        adv = self._steps(clean, text_f, target_f, info)
        info["perturbation_norm"] = float(torch.norm(adv - clean))                                   # :307-308
        success = self._evaluate_attack_success(adv, text_f, target_f)
        self._update_stats(info, success)
        result = {"adversarial_image": adv, "original_image": clean, "perturbation": adv - clean, "success": success,
                  "attack_info": info, "config": self.config}
        if self.cache is not None and len(self.cache) < self.config.cache_size:
            self.cache[key] = result
        return result

    def _pgd_attack(self, image: torch.Tensor, text_features: torch.Tensor,
                    target_features: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Dict]:
        info = {"iterations": 0, "loss_history": [], "similarity_history": [], "perturbation_norm": 0.0}
        unit = lambda t: None if t is None else torch.nn.functional.normalize(t.to(self.device, torch.float32), dim=-1)
        clean = self._to_batch(image)
        adv = self._steps(clean, unit(text_features), unit(target_features), info)
        info["perturbation_norm"] = float(torch.norm(adv - clean))
        return adv, info

    def _evaluate_attack_success(self, adversarial_image: torch.Tensor, text_features: torch.Tensor,
                                 target_features: Optional[torch.Tensor] = None) -> bool:
        """:312-340."""
        f = self.engine.encode_image(adversarial_image, True)
        cos = lambda t: float(torch.nn.functional.cosine_similarity(f, t.to(f.device)).mean())
        if self.config.targeted and target_features is not None:
            return cos(target_features) > cos(text_features)
        return cos(text_features) < 0.5

    # ---- batches (:342-563) ----------------------------------------------------------------------------
    def batch_attack(self, images, texts: List[str], target_texts: Optional[List[str]] = None) -> List[Dict[str, Any]]:
        t0 = time.time()
        x = self._to_batch(images)
        out: List[Dict[str, Any]] = []
        bs = self.config.batch_size
        for i in range(0, x.shape[0], bs):
            out.extend(self._batch_pgd_attack(x[i:i + bs], texts[i:i + bs], target_texts[i:i + bs] if target_texts else None))
        ok = sum(1 for r in out if r["success"])
        self.attack_stats["total_attacks"] += len(out)
        self.attack_stats["successful_attacks"] += ok
        logging.info("batch PGD: %d/%d succeeded in %.2f s", ok, len(out), time.time() - t0)
        return out

    def perturb(self, images: torch.Tensor, texts: Sequence[str], target_texts: Optional[Sequence[str]] = None) -> torch.Tensor:
        """Device tensor in, adversarial device tensor out (no per-sample dictionaries): what an evaluation run
        feeds straight into ``pipeline.detect``."""
        x = self._to_batch(images)
        bs = self.config.batch_size
        nc = max(1, int(self.config.concurrent_batches))
        outs = []
        starts = list(range(0, x.shape[0], bs))
        for g0 in range(0, len(starts), nc):
            jobs = []
            for i in starts[g0:g0 + nc]:
                tf = self._text_unit(texts[i:i + bs])
                gf = self._text_unit(target_texts[i:i + bs]) if target_texts else None
                jobs.append((x[i:i + bs].contiguous(), tf, gf))
            outs.extend(self._steps_concurrent(jobs))
        return torch.cat(outs)

    def _batch_pgd_attack(self, batch_images: torch.Tensor, batch_texts: List[str],
                          batch_targets: Optional[List[str]] = None) -> List[Dict[str, Any]]:
        c = self.config
        clean = self._to_batch(batch_images)
        text_f = self._text_unit(batch_texts)
        target_f = self._text_unit(batch_targets) if batch_targets else None
        adv = self._steps(clean, text_f, target_f)
        final = self.engine.encode_image(adv, True)                                                   # :524-526
        targeted = bool(c.targeted and target_f is not None)
        sims = (final * (target_f if targeted else text_f)).sum(-1).cpu().tolist()
        pert = adv - clean
        linf = pert.abs().flatten(1).max(dim=1).values.cpu().tolist()
        adv_c, clean_c, pert_c = adv.cpu(), clean.cpu(), pert.cpu()
        results = []
        for i in range(clean.shape[0]):
            success = sims[i] > 0.5 if targeted else sims[i] < 0.3                                    # :530-540
            results.append({"adversarial_image": adv_c[i], "original_image": clean_c[i], "perturbation": pert_c[i],
                            "success": success,
                            "attack_info": {"iterations": c.num_steps, "final_similarity": sims[i],
                                            "perturbation_norm": linf[i], "targeted": c.targeted},
                            "config": c})
        return results

    # ---- cache / stats (:565-640) -----------------------------------------------------------------------
    def _get_cache_key(self, image, text: str, target_text: Optional[str] = None) -> str:
        if isinstance(image, torch.Tensor):
            ih = hash(f"{tuple(image.shape)}_{image.device}_{float(image.sum())}")
        else:
            ih = hash(str(image))
        return f"pgd_{ih}_{hash(text)}_{hash(target_text) if target_text else 0}_{self.config.epsilon}_{self.config.num_steps}"

    def _update_stats(self, attack_info: Dict, success: bool) -> None:
        s = self.attack_stats
        s["total_attacks"] += 1
        s["successful_attacks"] += int(bool(success))
        n = s["total_attacks"]
        s["average_perturbation"] = (s["average_perturbation"] * (n - 1) + attack_info["perturbation_norm"]) / n
        s["average_iterations"] = (s["average_iterations"] * (n - 1) + attack_info["iterations"]) / n

    def get_attack_stats(self) -> Dict[str, Any]:
        s = dict(self.attack_stats)
        s["success_rate"] = s["successful_attacks"] / s["total_attacks"] if s["total_attacks"] else 0.0
        return s

    def reset_stats(self) -> None:
        self.attack_stats = {"total_attacks": 0, "successful_attacks": 0, "average_perturbation": 0.0,
                             "average_iterations": 0.0}

    def clear_cache(self) -> None:
        if self.cache:
            self.cache.clear()


def create_pgd_attacker(clip_model, config: Optional[PGDAttackConfig] = None) -> PGDAttacker:
    return PGDAttacker(clip_model, config or PGDAttackConfig())


# ================================================================================================
# Hubness attack (src/attacks/hubness_attack.py): push ONE image towards many text queries at once.
#   loss = -mean_q cos(f(x), t_q) = -(f_hat . mean_q t_hat_q)            (:656-676)
# so the embedding gradient is the constant vector -mean_q t_hat_q (/ B in a batch): again no autograd
# graph, and the "bank" of 10-200 queries collapses to one row per image before the loop starts.
# ================================================================================================
@dataclass
class HubnessAttackConfig:
    """src/attacks/hubness_attack.py:40-99 (same names and defaults)."""
    clip_model: str = "openai/clip-vit-base-patch32"
    device: str = "cuda"
    epsilon: float = 16.0 / 255.0
    num_iterations: int = 500
    step_size: float = 0.02
    k_neighbors: int = 10
    num_target_queries: int = 100
    hubness_weight: float = 1.0
    success_threshold: float = 0.84
    learning_rate: float = 0.02
    momentum: float = 0.9
    weight_decay: float = 1e-4
    attack_mode: str = "universal"
    target_concepts: List[str] = field(default_factory=list)
    norm_constraint: str = "linf"
    clamp_min: float = 0.0
    clamp_max: float = 1.0
    random_start: bool = True
    random_seed: int = 42
    enable_multi_gpu: bool = True
    gpu_ids: Optional[List[int]] = None
    batch_size: int = 64
    batch_size_per_gpu: int = 16
    num_workers: int = 4
    gradient_accumulation_steps: int = 1
    mixed_precision: bool = True
    pin_memory: bool = True
    enable_cache: bool = True
    cache_size: int = 1000
    dataset_size: int = 25000
    query_pool_size: int = 1000

    def __post_init__(self):
        if self.target_concepts is None:
            self.target_concepts = []

    @classmethod
    def from_dict(cls, config_dict: Dict[str, Any]) -> "HubnessAttackConfig":
        """:100-128: reads ``config_dict['attacks']['hubness']``."""
        h = config_dict.get("attacks", {}).get("hubness", {})
        keys = ("clip_model", "epsilon", "num_iterations", "step_size", "k_neighbors", "num_target_queries",
                "hubness_weight", "success_threshold", "learning_rate", "momentum", "weight_decay", "attack_mode",
                "target_concepts", "norm_constraint", "clamp_min", "clamp_max", "random_start", "random_seed",
                "enable_cache", "cache_size", "dataset_size", "query_pool_size")
        return cls(**{k: h[k] for k in keys if k in h})


COMMON_QUERIES = ("a photo of a cat", "a dog playing", "a beautiful landscape", "a person walking", "a car on the road",
                  "a bird flying", "a flower in the garden", "a building in the city", "food on a plate",
                  "a sunset over the ocean")                                                              # :769-774


class HubnessAttack:
    """Mirror of ``HubnessAttack`` (:131-787).  ``clip_model`` may be injected (the reference builds its own from
    ``config.clip_model``, :435-462; done here too when none is given).  ``norm_constraint`` 'linf' (default) or 'l2'
    (the batch core's L2 step and projection, :378-386, as one fused kernel: ``tvc_l2_step``)."""

    def __init__(self, config: Optional[HubnessAttackConfig] = None, clip_model=None):
        self.config = config or HubnessAttackConfig()
        if self.config.norm_constraint not in ("linf", "l2"):
            raise ValueError(f"norm_constraint must be 'linf' or 'l2' (got {self.config.norm_constraint!r})")
        if clip_model is None:
            from .clip import CLIPConfig, CLIPModel
            clip_model = CLIPModel(CLIPConfig(model_name=self.config.clip_model, device=self.config.device))
        self.clip_model = clip_model
        self.engine = clip_model.engine
        self.device = clip_model.device
        self.device_ids = [self.device.index or 0]
        self.attack_stats = {"total_attacks": 0, "successful_attacks": 0, "average_iterations": 0,
                             "average_hubness_score": 0.0, "average_attack_time": 0.0}
        self.cache: Optional[Dict[str, Any]] = {} if self.config.enable_cache else None
        self._rng = random.Random(self.config.random_seed)
        self._gen = torch.Generator().manual_seed(self.config.random_seed)
        self.text_features = None
        self.image_features = None

    # ---- reference database (:189-204) ----------------------------------------------------------------
    def build_reference_database(self, reference_images, reference_texts: List[str]) -> None:
        self.image_features = self.clip_model.encode_image(reference_images)
        self.text_features = self.clip_model.encode_text(reference_texts)

    def _generate_random_queries(self, n: Optional[int] = None) -> List[str]:
        """:766-777 (the batch core passes a count, :289, which the reference's signature does not take)."""
        n = min(n or self.config.num_target_queries, len(COMMON_QUERIES))
        return self._rng.sample(list(COMMON_QUERIES), n)

    def compute_hubness(self, image_features: torch.Tensor, text_features: torch.Tensor, k: int = 10) -> float:
        """:464-498: share of the text queries whose top-1 image is image 0.  One all-pairs cosine launch."""
        from .metrics import SimilarityCalculator
        img = image_features.reshape(-1, image_features.shape[-1])
        C = SimilarityCalculator.batch_cosine_similarity(text_features.reshape(-1, img.shape[-1]), img, engine=self.engine)
        return float((C.argmax(axis=1) == 0).mean())

    # ---- the loop (:549-654) on a device batch -----------------------------------------------------------
    def _optimise(self, clean: torch.Tensor, q_mean: torch.Tensor):
        """clean [B,3,S,S], q_mean [B, D] = mean of each image's unit query rows -> (best image, best loss [B])."""
        c = self.config
        B = clean.shape[0]
        if c.random_start:                                       # :573-576: perturbation ~ U(-eps, eps)
            noise = (torch.rand(clean.shape, generator=self._gen) * 2 - 1) * c.epsilon
            adv = torch.clamp(clean + noise.to(clean.device), c.clamp_min, c.clamp_max).contiguous()
        else:
            adv = torch.clamp(clean, c.clamp_min, c.clamp_max).contiguous()
        g_out = (-q_mean / B).contiguous()                       # d(mean_b loss_b) / d(unit embedding)
        best_loss = torch.full((B,), float("inf"), device=clean.device)
        best = adv.clone()
        for _ in range(c.num_iterations):
            f = self.engine.encode_image_grad(adv, True)
            loss = -(f * q_mean).sum(-1)                         # per image, on the device: no host sync in the loop
            better = loss < best_loss                            # :626-628 (the image the loss was computed on)
            best_loss = torch.where(better, loss, best_loss)
            best = torch.where(better.view(-1, 1, 1, 1), adv, best)
            grad = self.engine.encode_image_backward(g_out)
            if c.norm_constraint == "l2":
                # :378-386: unit-L2 gradient step, projection onto the eps L2 ball, clamp (descent, as the L-inf form)
                self.engine.l2_step(adv, clean, grad, c.epsilon, c.step_size, c.clamp_min, c.clamp_max, True)
            else:
                # :617-637: p -= step * sign(grad); clamp to the eps ball; clamp the image  == one descent pgd_step
                self.engine.pgd_step(adv, clean, grad, None, c.epsilon, c.step_size, 0.0, c.clamp_min, c.clamp_max, True)
        return best, best_loss

    def _unit_queries(self, queries: Sequence[str]) -> torch.Tensor:
        return self.clip_model.encode_tokens(self.clip_model.tokenize(list(queries)), True)

    def _perform_attack(self, image_tensor: torch.Tensor, text_features: torch.Tensor, text_queries: List[str]) -> Dict[str, Any]:
        clean = image_tensor.to(self.device, torch.float32)
        clean = (clean if clean.dim() == 4 else clean.unsqueeze(0)).contiguous()
        tq = torch.nn.functional.normalize(text_features.to(self.device, torch.float32), dim=-1)
        best, best_loss = self._optimise(clean, tq.mean(0, keepdim=True))
        final = self.engine.encode_image(best, True)
        hub = self.compute_hubness(final.unsqueeze(0), tq, self.config.k_neighbors)        # :640-646 (one image: 1.0)
        pert = best - clean
        return {"adversarial_image": best.squeeze(0).cpu(), "original_image": clean.squeeze(0).cpu(),
                "perturbation": pert.squeeze(0).cpu(), "hubness_score": hub,
                "perturbation_norm": float(pert.abs().max()), "final_loss": float(best_loss[0]),
                "iterations": self.config.num_iterations, "success": hub > self.config.success_threshold,
                "text_queries": text_queries}

    def create_adversarial_hub(self, image, text_queries: List[str]) -> Dict[str, Any]:
        """:500-547."""
        t0 = time.time()
        key = self._generate_cache_key(image, text_queries)
        if self.cache is not None and key in self.cache:
            return self.cache[key]
        x = image if isinstance(image, torch.Tensor) else self.clip_model.preprocess(image)
        result = self._perform_attack(x, self._unit_queries(text_queries), text_queries)
        self._update_attack_stats(result, time.time() - t0)
        if self.cache is not None and len(self.cache) < self.config.cache_size:
            self.cache[key] = result
        return result

    def attack(self, image, text: Optional[str] = None) -> Dict[str, Any]:
        """:703-728."""
        return self.create_adversarial_hub(image, self._generate_random_queries() if text is None else [text])

    def attack_single(self, image, text: str) -> Dict[str, Any]:
        """:730-764 (the key names run_experiments.py expects; errors are reported, not raised, as there)."""
        try:
            r = self.attack(image, text)
            return {"success": r.get("success", False), "hubness": r.get("hubness_score", 0.0),
                    "similarity_change": r.get("perturbation_norm", 0.0), "iterations": r.get("iterations", 0),
                    "adversarial_image": r.get("adversarial_image"), "original_image": r.get("original_image"),
                    "perturbation": r.get("perturbation"), "final_loss": r.get("final_loss", float("inf"))}
        except Exception as e:                                   # noqa: BLE001 -- mirrors :757-764
            logging.error("hubness attack_single failed: %s", e)
            return {"success": False, "hubness": 0.0, "similarity_change": 0.0, "iterations": 0, "error": str(e)}

    def batch_attack(self, images, texts: List[str]) -> List[Dict[str, Any]]:
        """:206-267.  Every image gets its own random query set (:286-291)."""
        t0 = time.time()
        if isinstance(images, torch.Tensor):
            x = images
        else:
            x = torch.stack([im if isinstance(im, torch.Tensor) else self.clip_model.preprocess(im) for im in images])
        out: List[Dict[str, Any]] = []
        bs = self.config.batch_size
        for i in range(0, x.shape[0], bs):
            out.extend(self._batch_attack_core(x[i:i + bs].to(self.device, torch.float32).contiguous(), texts[i:i + bs]))
        n, ok = len(out), sum(1 for r in out if r["success"])
        s = self.attack_stats
        s["total_attacks"] += n
        s["successful_attacks"] += ok
        s["average_attack_time"] = (s["average_attack_time"] * (s["total_attacks"] - n) + (time.time() - t0)) / max(s["total_attacks"], 1)
        return out

    def _batch_attack_core(self, batch_images: torch.Tensor, batch_texts: List[str]) -> List[Dict[str, Any]]:
        """:269-424 with the single-image loop's DESCENT on the loss.  (The reference's batch core steps
        ``+ step_size * grad.sign()`` on the same negative-similarity loss, :357, i.e. away from the queries --
        against its own comment and its single-image loop, :617; and it cannot run at all: it calls
        ``_generate_random_queries`` with an argument the method does not take, :289.)"""
        B = batch_images.shape[0]
        queries = [self._generate_random_queries(self.config.num_target_queries) for _ in range(B)]
        qf = self._unit_queries([q for qs in queries for q in qs])
        nq = len(queries[0])
        q_mean = qf.view(B, nq, -1).mean(1)
        best, _ = self._optimise(batch_images, q_mean)
        final = self.engine.encode_image(best, True)
        scores = (final * q_mean).sum(-1).cpu().tolist()                                   # mean similarity (:392-393)
        linf = (best - batch_images).abs().flatten(1).max(dim=1).values.cpu().tolist()
        best_c, clean_c = best.cpu(), batch_images.cpu()
        return [{"success": scores[i] > self.config.success_threshold, "hubness_score": scores[i],
                 "perturbation_strength": linf[i], "adversarial_image": best_c[i], "original_image": clean_c[i],
                 "target_queries": queries[i], "iterations": self.config.num_iterations} for i in range(B)]

    # ---- cache / stats (:678-701, 779-786) ---------------------------------------------------------------
    def _generate_cache_key(self, image, text_queries: List[str]) -> str:
        import hashlib
        ih = f"{tuple(image.shape)}_{float(image.sum())}" if isinstance(image, torch.Tensor) else str(image)
        return hashlib.md5((ih + "|".join(text_queries) + f"{self.config.epsilon}_{self.config.num_iterations}").encode()).hexdigest()

    def _update_attack_stats(self, result: Dict[str, Any], attack_time: float) -> None:
        s = self.attack_stats
        s["total_attacks"] += 1
        s["successful_attacks"] += int(bool(result["success"]))
        n = s["total_attacks"]
        s["average_iterations"] = (s["average_iterations"] * (n - 1) + result["iterations"]) / n
        s["average_hubness_score"] = (s["average_hubness_score"] * (n - 1) + result["hubness_score"]) / n
        s["average_attack_time"] = (s["average_attack_time"] * (n - 1) + attack_time) / n

    def get_attack_stats(self) -> Dict[str, Any]:
        s = dict(self.attack_stats)
        s["success_rate"] = s["successful_attacks"] / s["total_attacks"] if s["total_attacks"] else 0.0
        return s


class HubnessAttackPresets:
    """:789-838."""
    @staticmethod
    def weak_attack() -> HubnessAttackConfig:
        return HubnessAttackConfig(epsilon=8.0 / 255.0, num_iterations=100, learning_rate=0.01, k_neighbors=5, num_target_queries=50)

    @staticmethod
    def strong_attack() -> HubnessAttackConfig:
        return HubnessAttackConfig(epsilon=32.0 / 255.0, num_iterations=1000, learning_rate=0.05, k_neighbors=20, num_target_queries=200)

    @staticmethod
    def targeted_attack(target_concepts: List[str]) -> HubnessAttackConfig:
        return HubnessAttackConfig(attack_mode="targeted", target_concepts=target_concepts, epsilon=16.0 / 255.0,
                                   num_iterations=500, learning_rate=0.02, k_neighbors=10, num_target_queries=100)

    @staticmethod
    def paper_standard() -> HubnessAttackConfig:
        return HubnessAttackConfig(epsilon=16.0 / 255.0, num_iterations=500, learning_rate=0.02, k_neighbors=10,
                                   num_target_queries=100, dataset_size=25000, query_pool_size=1000)


def create_hubness_attacker(config: Optional[HubnessAttackConfig] = None, clip_model=None) -> HubnessAttack:
    return HubnessAttack(config or HubnessAttackConfig(), clip_model=clip_model)


# ================================================================================================
# FSTA (src/attacks/fsta_attack.py) and SMA (src/attacks/sma_attack.py): ONE loop with different constants.
#   loss = a_tgt mean cos(f, target) + a_txt mean cos(f, text) + w_out mse(f, target) + w_div diversity(f)
#          [+ perceptual_weight mse(adv, clean), SMA]
# The loss couples the rows of a batch (diversity) and is not linear in f, so its embedding gradient is a kernel
# (tvc_attack_feature_grad); the pixel-space term never passes the tower and is added inside the step kernel
# (tvc_attack_step: gradient clamp, un-normalised momentum, sign step + L-inf ball or momentum step + L2 ball).
# Per iteration: encode_image_grad -> attack_feature_grad -> encode_image_backward -> attack_step, no host
# synchronisation unless a history is asked for.  On purpose not carried over: nn.DataParallel, GradScaler /
# autocast, tqdm, `feature_layer` (read by nothing in the reference).  Generated targets and the JPEG noise draw
# from a seeded CPU generator (the reference uses the global device RNG), so a run is reproducible.
# ================================================================================================
def attack_lr_schedule(learning_rate: float, num_iter: int, decay_factor: float, every: int = 1, enabled: bool = True) -> List[float]:
    """The learning rate of each iteration: ``lr *= decay_factor`` after every ``every``-th iteration when ``enabled``.
    FSTA (:249-250): every 1, enabled = adaptive_step_size.  SMA ``attack`` (:308): every gamma_epochs, always.  SMA batch
    core (:734): every gamma_epochs, enabled = adaptive_step_size.  Python floats, multiplied as the reference multiplies them."""
    out, lr = [], float(learning_rate)
    for k in range(int(num_iter)):
        out.append(lr)
        if enabled and (k + 1) % max(int(every), 1) == 0:
            lr *= decay_factor
    return out


def attack_targets(text_f: torch.Tensor, selection: str, gen: torch.Generator) -> torch.Tensor:
    """Target rows when the caller names none (fsta_attack.py:299-315, sma_attack.py:375-411), on the device of ``text_f``:
    'random' unit Gaussian rows; 'centroid' minus the unit mean text row, repeated; 'semantic' a Gaussian draw made
    orthogonal to its text row (row-wise Gram-Schmidt) and normalised; 'adversarial' minus the unit text row."""
    B, D = text_f.shape
    if selection == "random":
        out = torch.nn.functional.normalize(torch.randn((B, D), generator=gen), p=2, dim=1).to(text_f.device)
    elif selection == "centroid":
        out = -torch.nn.functional.normalize(text_f.mean(dim=0, keepdim=True), p=2, dim=1).repeat(B, 1)
    elif selection == "semantic":
        r = torch.randn((B, D), generator=gen).to(text_f.device)
        r = r - (r * text_f).sum(1, keepdim=True) / text_f.norm(dim=1, keepdim=True) ** 2 * text_f
        out = torch.nn.functional.normalize(r, p=2, dim=1)
    elif selection == "adversarial":
        out = -torch.nn.functional.normalize(text_f, p=2, dim=1)
    else:
        raise ValueError(f"target_selection must be 'random', 'centroid', 'semantic' or 'adversarial' (got {selection!r})")
    return out.contiguous()


def feature_attack_loop(engine, clean: torch.Tensor, text_f: torch.Tensor, target_f: torch.Tensor, *, lrs: Sequence[float],
                        a_tgt: float, a_txt: float, metric: str = "cosine", w_out: float = 0.0, w_div: float = 0.0,
                        eps: float, mu: float, clip: float, perceptual_weight: float = 0.0, lo: float = 0.0, hi: float = 1.0,
                        norm: str = "inf", noise_std: float = 0.0, gen: Optional[torch.Generator] = None,
                        history: Optional[Dict[str, list]] = None) -> torch.Tensor:
    """The loop of fsta_attack.py:169-252 / sma_attack.py:221-318,605-735 on a device batch: starts at adv = clean (no
    random start; the ball is around the unclamped clean image), one iteration per entry of ``lrs``.  ``noise_std`` > 0 is
    SMA's JPEG stand-in (:413-422): clamp(adv + noise, 0, 1) goes to the tower, with torch ops, and the tower's input
    gradient is zeroed where that clamp is active."""
    B = clean.shape[0]
    adv = clean.clone().contiguous()
    mom = torch.zeros_like(adv)
    p = 2.0 * perceptual_weight / max(adv.numel(), 1)
    for lr in lrs:
        if noise_std > 0.0:
            noisy = adv + (torch.randn(adv.shape, generator=gen) * noise_std).to(adv.device)
            x = torch.clamp(noisy, 0.0, 1.0).contiguous()
        else:
            x = adv
        f = engine.encode_image_grad(x, True)
        gf, rows = engine.attack_feature_grad(f, text_f, target_f, a_tgt=a_tgt, a_txt=a_txt, metric=metric, w_out=w_out, w_div=w_div)
        grad = engine.encode_image_backward(gf)
        if noise_std > 0.0:
            grad = (grad * ((noisy >= 0.0) & (noisy <= 1.0))).contiguous()
        if history is not None:                                  # the only host synchronisation of the loop
            m = rows.double().mean(0).tolist()
            sgn = -1.0 if metric == "euclidean" else 1.0
            div = m[3] / (B - 1) if B > 1 else 0.0
            pix = perceptual_weight * float(((adv - clean).double() ** 2).mean())
            history["loss_history"].append(sgn * (a_tgt * m[0] + a_txt * m[1]) + w_out * m[2] + w_div * div + pix)
            history["target_history"].append(m[0])
            history["text_history"].append(m[1])
            history["lr_history"].append(float(lr))
        engine.attack_step(adv, clean, grad, mom, eps, lr, mu, clip, p, lo, hi, norm)
    return adv


class _FeatureSpaceAttacker:
    """What FSTAAttacker and SMAAttacker share: the tensors in, the loop, the per-sample dictionaries, stats and cache.
    A subclass gives the loop's constants per path ('attack' / 'batch'), the success rule without targets and its stats keys."""
    _name = "feature"
    _untargeted_threshold = 0.5

    def __init__(self, clip_model, config):
        self.config = config
        self.clip_model = clip_model
        self.engine = clip_model.engine
        self.device = clip_model.device
        self.device_ids = [self.device.index or 0]
        self._gen = torch.Generator().manual_seed(self.config.random_seed)
        if self.config.enable_cache:
            self.cache: Dict[Any, Dict[str, Any]] = {}
            self.cache_keys: List[Any] = []
        self.reset_stats()

    # ---- helpers ---------------------------------------------------------------------------------
    def _to_batch(self, images) -> torch.Tensor:
        if isinstance(images, torch.Tensor):
            x = images if images.dim() == 4 else images.unsqueeze(0)
        else:
            x = torch.stack([im if isinstance(im, torch.Tensor) else self.clip_model.preprocess(im) for im in images])
        return x.to(self.device, torch.float32).contiguous()

    def _text_unit(self, texts: Sequence[str]) -> torch.Tensor:
        return self.clip_model.encode_tokens(self.clip_model.tokenize(list(texts)), True)

    def _norm(self) -> str:
        return "inf" if self.config.norm_type == "inf" else "l2"       # the reference's else branch is the L2 one

    def _loop_kwargs(self, path: str) -> Dict[str, Any]:
        raise NotImplementedError

    def _loop(self, clean: torch.Tensor, text_f: torch.Tensor, target_f: torch.Tensor, path: str,
              history: Optional[Dict[str, list]] = None) -> torch.Tensor:
        c = self.config
        return feature_attack_loop(self.engine, clean, text_f.contiguous(), target_f.contiguous(), eps=c.epsilon, mu=c.momentum,
                                   lo=c.clamp_min, hi=c.clamp_max, norm=self._norm(), gen=self._gen, history=history,
                                   **self._loop_kwargs(path))

    def _similarities(self, adv: torch.Tensor, text_f: torch.Tensor, target_f: Optional[torch.Tensor]):
        f = self.engine.encode_image(adv, True)
        cos = torch.nn.functional.cosine_similarity
        return cos(f, text_f, dim=1), (cos(f, target_f, dim=1) if target_f is not None else None)

    def _judge(self, adv: torch.Tensor, text_f: torch.Tensor, target_f: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        """Per image (success flag, semantic score).  With named targets: target similarity above text similarity, score
        their difference (fsta :334-341, sma :445-455,747-752); without: text similarity under the threshold, score minus
        the text similarity (fsta :342-344, sma :456-459,753-755)."""
        ts, gs = self._similarities(adv, text_f, target_f)
        if gs is not None:
            return gs > ts, gs - ts
        return ts < self._untargeted_threshold, -ts

    def _batches(self, images, texts: Sequence[str], targets: Optional[Sequence[str]]):
        """(clean, text rows, target rows, named-target rows or None, texts, targets) per `batch_size` images."""
        x = self._to_batch(images)
        bs = max(1, int(self.config.batch_size))
        for i in range(0, x.shape[0], bs):
            clean = x[i:i + bs].contiguous()
            tx = list(texts[i:i + bs])
            tg = list(targets[i:i + bs]) if targets else None
            text_f = self._text_unit(tx)
            named = self._text_unit(tg) if tg else None
            target_f = named if named is not None else attack_targets(text_f, self.config.target_selection, self._gen)
            yield clean, text_f, target_f, named, tx, tg

    # ---- the public surface ------------------------------------------------------------------------
    def perturb(self, images: torch.Tensor, texts: Sequence[str], targets: Optional[Sequence[str]] = None) -> torch.Tensor:
        """Device tensor in, adversarial device tensor out (the batch path, no per-sample dictionaries)."""
        return torch.cat([self._loop(clean, text_f, target_f, "batch") for clean, text_f, target_f, _, _, _ in
                          self._batches(images, texts, targets)])

    def _batch_results(self, images, texts: Sequence[str], targets: Optional[Sequence[str]]) -> List[Dict[str, Any]]:
        out: List[Dict[str, Any]] = []
        for clean, text_f, target_f, named, tx, tg in self._batches(images, texts, targets):
            adv = self._loop(clean, text_f, target_f, "batch")
            ok, score = self._judge(adv, text_f, named)
            linf = (adv - clean).abs().flatten(1).max(dim=1).values.cpu().tolist()
            ok, score, adv_c, clean_c = ok.cpu().tolist(), score.cpu().tolist(), adv.cpu(), clean.cpu()
            for i in range(clean.shape[0]):
                out.append({"adversarial_images": adv_c[i], "original_images": clean_c[i], "success_rate": float(ok[i]),
                            "semantic_misalignment_score": float(score[i]), "perturbation_norm": float(linf[i]),
                            "text": tx[i], "target_semantic": tg[i] if tg else None,
                            "success": bool(ok[i]), "adversarial_image": adv_c[i], "original_image": clean_c[i]})
        return out

    def batch_attack(self, images, texts: List[str], targets: Optional[List[str]] = None) -> List[Dict[str, Any]]:
        """Per-sample dictionaries (sma_attack.py:508-575,763-772; the experiment driver calls it on both attackers and reads
        'success' and 'adversarial_image', so both key sets are present)."""
        t0 = time.time()
        out = self._batch_results(images, texts, targets)
        n, good = len(out), sum(1 for r in out if r["success"])
        self.attack_stats["total_attacks"] += n
        self.attack_stats["successful_attacks"] += good
        logging.info("batch %s: %d/%d succeeded in %.2f s", self._name, good, n, time.time() - t0)
        return out

    def _attack(self, images, texts: List[str], targets: Optional[List[str]]):
        clean = self._to_batch(images)
        text_f = self._text_unit(texts)
        named = self._text_unit(targets) if targets else None
        target_f = named if named is not None else attack_targets(text_f, self.config.target_selection, self._gen)
        adv = self._loop(clean, text_f, target_f, "attack")
        ok, score = self._judge(adv, text_f, named)
        B = clean.shape[0]
        rate = float(ok.float().mean())
        self.attack_stats["total_attacks"] += B
        self.attack_stats["successful_attacks"] += int(rate * B)
        if self.config.enable_cache:
            self._cache_results(clean, adv, texts)
        linf = float((adv - clean).abs().flatten(1).max(dim=1).values.mean())
        return clean, adv, rate, float(score.mean()), linf

    def _cache_results(self, images: torch.Tensor, adv_images: torch.Tensor, texts: List[str]) -> None:
        """fsta :348-367 / sma :463-482: first in, first out.  (The key is the image batch's shape and sum and the texts,
        not a tuple of every pixel.)"""
        if len(self.cache_keys) >= self.config.cache_size:
            del self.cache[self.cache_keys.pop(0)]
        key = hash((tuple(images.shape), float(images.sum()), tuple(texts)))
        if key not in self.cache:
            self.cache_keys.append(key)
        self.cache[key] = {"adversarial_images": adv_images.clone(), "original_images": images.clone(), "texts": list(texts)}


@dataclass
class FSTAAttackConfig:
    """src/attacks/fsta_attack.py:20-69 (same names and defaults), plus what the experiment driver passes
    (run_experiments.py:599-609): ``num_iterations`` (an alias of ``num_iter``) and the multi-GPU fields, accepted and
    unused as in PGDAttackConfig.  ``feature_layer`` is kept for the constructor only (nothing reads it)."""
    random_seed: int = 42
    device: str = "cuda"
    epsilon: float = 0.031
    alpha: float = 0.008
    num_iter: int = 20
    feature_layer: str = "penultimate"
    target_feature_method: str = "centroid"
    feature_distance_metric: str = "cosine"
    targeted: bool = True
    target_selection: str = "random"
    num_targets: int = 10
    feature_weight: float = 1.0
    output_weight: float = 0.1
    diversity_weight: float = 0.05
    momentum: float = 0.9
    decay_factor: float = 0.99
    learning_rate: float = 0.01
    norm_type: str = "inf"
    clamp_min: float = 0.0
    clamp_max: float = 1.0
    adaptive_step_size: bool = True
    gradient_clipping: bool = True
    clip_value: float = 1.0
    batch_size: int = 32
    enable_cache: bool = True
    cache_size: int = 1000
    num_iterations: Optional[int] = None
    enable_multi_gpu: bool = False
    gpu_ids: Optional[List[int]] = None
    batch_size_per_gpu: int = 8
    num_workers: int = 4

    def __post_init__(self):
        if self.num_iterations is not None:
            self.num_iter = int(self.num_iterations)
        if self.feature_distance_metric not in ("cosine", "euclidean"):
            raise ValueError(f"feature_distance_metric must be 'cosine' or 'euclidean' (got {self.feature_distance_metric!r})")


class FSTAAttacker(_FeatureSpaceAttacker):
    """Mirror of ``FSTAAttacker`` (fsta_attack.py:72-389) plus the ``batch_attack`` the driver calls (:646) and ``perturb``."""
    _name = "FSTA"
    _untargeted_threshold = 0.5                                                                       # :344

    def _loop_kwargs(self, path: str) -> Dict[str, Any]:
        c = self.config
        return dict(lrs=attack_lr_schedule(c.learning_rate, c.num_iter, c.decay_factor, 1, c.adaptive_step_size),
                    a_tgt=-c.feature_weight, a_txt=c.feature_weight, metric=c.feature_distance_metric, w_out=c.output_weight,
                    w_div=c.diversity_weight, clip=c.clip_value if c.gradient_clipping else 0.0)

    def attack(self, images, texts: List[str], target_texts: Optional[List[str]] = None) -> Dict[str, Any]:
        """:105-154."""
        clean, adv, rate, _, linf = self._attack(images, texts, target_texts)
        return {"adversarial_images": adv, "original_images": clean, "success_rate": rate, "perturbation_norm": linf}

    def _fsta_attack(self, images: torch.Tensor, text_features: torch.Tensor, target_features: torch.Tensor) -> torch.Tensor:
        """:156-252 on rows the caller encoded."""
        dev = lambda t: t.to(self.device, torch.float32).contiguous()
        return self._loop(self._to_batch(images), dev(text_features), dev(target_features), "attack")

    def get_attack_stats(self) -> Dict[str, Any]:
        s = dict(self.attack_stats)
        s["success_rate"] = s["successful_attacks"] / s["total_attacks"] if s["total_attacks"] > 0 else 0.0
        return s

    def reset_stats(self) -> None:
        self.attack_stats = {"total_attacks": 0, "successful_attacks": 0, "avg_iterations": 0, "avg_perturbation_norm": 0.0}


def create_fsta_attacker(clip_model, config: Optional[FSTAAttackConfig] = None) -> FSTAAttacker:
    return FSTAAttacker(clip_model, config or FSTAAttackConfig())


class FSTAAttackPresets:
    """:409-451."""
    @staticmethod
    def weak_attack() -> FSTAAttackConfig:
        return FSTAAttackConfig(epsilon=0.016, num_iter=10, learning_rate=0.005)

    @staticmethod
    def strong_attack() -> FSTAAttackConfig:
        return FSTAAttackConfig(epsilon=0.047, num_iter=40, learning_rate=0.02)

    @staticmethod
    def targeted_attack() -> FSTAAttackConfig:
        return FSTAAttackConfig(targeted=True, target_selection="centroid", feature_weight=2.0, num_iter=30)

    @staticmethod
    def paper_config() -> FSTAAttackConfig:
        return FSTAAttackConfig(epsilon=0.031, alpha=0.008, num_iter=20, feature_layer="penultimate", feature_distance_metric="cosine")


@dataclass
class SMAAttackConfig:
    """src/attacks/sma_attack.py:21-82 (same names and defaults), plus the driver's ``num_iterations`` alias of
    ``num_iter`` (run_experiments.py:686)."""
    random_seed: int = 42
    device: str = "cuda"
    epsilon: float = 0.031
    alpha: float = 0.008
    num_iter: int = 15
    semantic_weight: float = 2.0
    perceptual_weight: float = 0.5
    diversity_weight: float = 0.1
    targeted: bool = True
    target_selection: str = "semantic"
    semantic_shift_strength: float = 1.5
    momentum: float = 0.9
    decay_factor: float = 0.95
    learning_rate: float = 0.01
    gamma_epochs: int = 5
    norm_type: str = "inf"
    clamp_min: float = 0.0
    clamp_max: float = 1.0
    jpeg_compression: bool = False
    jpeg_quality: int = 95
    adaptive_step_size: bool = True
    gradient_clipping: bool = True
    clip_value: float = 1.0
    batch_size: int = 32
    enable_multi_gpu: bool = False
    gpu_ids: Optional[List[int]] = None
    batch_size_per_gpu: int = 8
    num_workers: int = 4
    gradient_accumulation_steps: int = 1
    mixed_precision: bool = False
    pin_memory: bool = True
    gradient_clip_value: float = 1.0
    enable_cache: bool = True
    cache_size: int = 1000
    num_iterations: Optional[int] = None

    def __post_init__(self):
        if self.num_iterations is not None:
            self.num_iter = int(self.num_iterations)


class SMAAttacker(_FeatureSpaceAttacker):
    """Mirror of ``SMAAttacker`` (sma_attack.py:85-774).  ``attack`` runs the loop of :207-318 (``clip_value``, the
    learning rate decays every ``gamma_epochs`` iterations), ``batch_attack`` / ``perturb`` the batch core of :577-735
    (``gradient_clip_value``, the decay only with ``adaptive_step_size``)."""
    _name = "SMA"
    _untargeted_threshold = 0.3                                                                       # :459,755

    def _loop_kwargs(self, path: str) -> Dict[str, Any]:
        c = self.config
        k = c.semantic_weight * (1.0 + c.semantic_shift_strength)                                      # :335-342
        batch = path == "batch"
        clip = (c.gradient_clip_value if batch else c.clip_value) if c.gradient_clipping else 0.0
        return dict(lrs=attack_lr_schedule(c.learning_rate, c.num_iter, c.decay_factor, c.gamma_epochs,
                                           c.adaptive_step_size if batch else True),
                    a_tgt=-k, a_txt=k, metric="cosine", w_out=0.0, w_div=c.diversity_weight, clip=clip,
                    perceptual_weight=c.perceptual_weight,
                    noise_std=(100 - c.jpeg_quality) / 100.0 * 0.01 if c.jpeg_compression else 0.0)   # :420-421

    def attack(self, images, texts: List[str], target_semantics: Optional[List[str]] = None) -> Dict[str, Any]:
        """:154-205."""
        clean, adv, rate, score, linf = self._attack(images, texts, target_semantics)
        self.attack_stats["semantic_misalignment_score"] += score
        return {"adversarial_images": adv, "original_images": clean, "success_rate": rate,
                "semantic_misalignment_score": score, "perturbation_norm": linf}

    def _batch_sma_attack(self, batch_images: torch.Tensor, batch_texts: List[str],
                          batch_targets: Optional[List[str]] = None) -> List[Dict[str, Any]]:
        """:577-774 (no statistics; more than `batch_size` images are run `batch_size` at a time)."""
        return self._batch_results(batch_images, batch_texts, batch_targets)

    def get_attack_stats(self) -> Dict[str, Any]:
        s = dict(self.attack_stats)
        n = s["total_attacks"]
        s["success_rate"] = s["successful_attacks"] / n if n > 0 else 0.0
        s["avg_semantic_score"] = s["semantic_misalignment_score"] / n if n > 0 else 0.0
        return s

    def reset_stats(self) -> None:
        self.attack_stats = {"total_attacks": 0, "successful_attacks": 0, "semantic_misalignment_score": 0.0,
                             "avg_perturbation_norm": 0.0}


def create_sma_attacker(clip_model, config: Optional[SMAAttackConfig] = None) -> SMAAttacker:
    return SMAAttacker(clip_model, config or SMAAttackConfig())


class SMAAttackPresets:
    """:794-851."""
    @staticmethod
    def weak_attack() -> SMAAttackConfig:
        return SMAAttackConfig(epsilon=0.016, num_iter=10, semantic_weight=1.0, learning_rate=0.005)

    @staticmethod
    def strong_attack() -> SMAAttackConfig:
        return SMAAttackConfig(epsilon=0.047, num_iter=25, semantic_weight=3.0, learning_rate=0.02)

    @staticmethod
    def semantic_targeted_attack() -> SMAAttackConfig:
        return SMAAttackConfig(targeted=True, target_selection="semantic", semantic_weight=2.5, semantic_shift_strength=2.0,
                               num_iter=20)

    @staticmethod
    def paper_config() -> SMAAttackConfig:
        return SMAAttackConfig(epsilon=0.031, alpha=0.008, num_iter=15, semantic_weight=2.0, target_selection="semantic",
                               jpeg_compression=False)

    @staticmethod
    def jpeg_robust_attack() -> SMAAttackConfig:
        return SMAAttackConfig(epsilon=0.039, num_iter=20, semantic_weight=2.0, jpeg_compression=True, jpeg_quality=85)
