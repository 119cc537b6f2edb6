"""``TVCEngine``: one C-ABI handle on one GPU, plus the tensor plumbing around it.

PyTorch-ROCm is used for device memory and streams only: every computation on
the hot path is a HIP kernel launched through ``include/tvc.h``.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import threading
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from .arch import ClipArch


@dataclass
class ConsistencyConfig:
    """Fields of the reference configs the consistency stage reads."""
    reference_count: int = 5             # experiments/defenses/retrieval_ref.py:23
    similarity_threshold: float = 0.3    # retrieval_ref.py:24
    retrieval_top_k: int = 10            # experiments/defenses/detector.py:29
    dup_threshold: float = 0.95          # experiments/defenses/detector.py:318
    w_text_variants: float = 0.4         # src/detector.py:667
    w_consistency: float = 0.2           # src/detector.py:669
    w_exp: Tuple[float, float, float, float] = (0.25, 0.25, 0.25, 0.25)   # consistency_checker.py:61-66
    search_k: int = 5                    # rows searched per text; >= reference_count

    def to_c(self) -> _lib.ConsistencyParams:
        p = _lib.ConsistencyParams()
        p.reference_count = self.reference_count
        p.similarity_threshold = self.similarity_threshold
        p.retrieval_top_k = self.retrieval_top_k
        p.dup_threshold = self.dup_threshold
        p.w_text_variants = self.w_text_variants
        p.w_consistency = self.w_consistency
        for i, w in enumerate(self.w_exp):
            p.w_exp[i] = w
        return p


@dataclass
class IVFIndex:
    """An inverted-file index built by ``TVCEngine.ivf_build``: the centroids, the list layout and the bank slot ``name``
    of the engine, which holds the bank rows in list order and belongs to the index (``TVCEngine.ivf_release`` frees it).
    List l = the stored rows ``offsets[l]:offsets[l + 1]``; ``ids[p]`` = the original row index of stored row p, ascending
    inside a list."""
    name: str
    nlist: int
    centroids: torch.Tensor      # fp32 [nlist, D]
    offsets: torch.Tensor        # int32 [nlist + 1]
    ids: torch.Tensor            # int32 [rows]
    max_list_rows: int
    rows: int
    dim: int


@dataclass
class RetrievalRanks:
    """What ``TVCEngine.retrieval_ranks`` returns.  Query i's relevant rows (its targets) are the entries
    ``tgt_off[i]:tgt_off[i + 1]`` of ``tgt_row`` / ``tgt_sim`` / ``pos``, best first; ``pos`` is the 0-based position of the
    target in the query's ranking of the whole slot.  The per-query arrays follow ``tvc_rank_metrics`` (include/tvc.h); a
    query without targets has zeros."""
    k_values: Tuple[int, ...]
    tgt_off: torch.Tensor        # int64 [M + 1]
    tgt_row: torch.Tensor        # int32 [T]
    tgt_sim: torch.Tensor        # fp32 [T]
    pos: torch.Tensor            # int32 [T]
    hist: torch.Tensor           # int32 [T]: the irrelevant rows between the target before this one and this one
    ap: torch.Tensor             # fp64 [M]
    rr: torch.Tensor             # fp64 [M]
    hits: torch.Tensor           # int32 [M, len(k_values)]
    dcg: torch.Tensor            # fp64 [M, len(k_values)]
    idcg: torch.Tensor           # fp64 [M, len(k_values)]

    @property
    def n_targets(self) -> torch.Tensor:
        """int64 [M]: the number of relevant rows of every query."""
        return self.tgt_off[1:] - self.tgt_off[:-1]


@dataclass
class RocSweep:
    """What ``TVCEngine.roc_sweep`` returns: the sorted sample and the per-row results of ``tvc_roc_sweep`` (include/tvc.h).
    Row 0 is the full sample (every multiplicity 1), rows 1 .. are the resamples / weightings asked for.  An invalid row (no
    positive or no negative weight) has ``valid == 0`` and zeros everywhere else."""
    scores: torch.Tensor         # fp32 [N] sorted descending (stable); -0.0 became 0.0
    labels: torch.Tensor         # uint8 [N] in sorted order
    order: torch.Tensor          # int32 [N]: the original index of every sorted position
    target_tpr: float
    thresholds: Tuple[float, ...]
    n_pos: torch.Tensor          # int32 [R]
    n_neg: torch.Tensor          # int32 [R]
    valid: torch.Tensor          # int32 [R]
    n_points: torch.Tensor       # int32 [R]: tie groups of weight > 0
    n_kept: torch.Tensor         # int32 [R]: the points sklearn's drop_intermediate keeps
    auc2: torch.Tensor           # int64 [R]: auc = auc2 / (2 P N)
    auc: torch.Tensor            # fp64 [R]
    ap: torch.Tensor             # fp64 [R]
    youden_j: torch.Tensor       # fp64 [R]
    youden_pos: torch.Tensor     # int32 [R]: sorted position of the Youden point, -1 = the origin (threshold +inf)
    youden_tp: torch.Tensor      # int32 [R]
    youden_fp: torch.Tensor      # int32 [R]
    target_pos: torch.Tensor     # int32 [R]: as youden_pos, of the point nearest to target_tpr
    target_tp: torch.Tensor      # int32 [R]
    target_fp: torch.Tensor      # int32 [R]
    thr_tp: torch.Tensor         # int32 [R, len(thresholds)]: TP of score >= threshold
    thr_fp: torch.Tensor         # int32 [R, len(thresholds)]

    def threshold_at(self, pos: int) -> float:
        """The score threshold of a reported sorted position: +inf for the origin (-1)."""
        return float("inf") if pos < 0 else float(self.scores[pos])


@dataclass
class SimilarityRows:
    """What ``TVCEngine.similarity_rows`` / ``similarity_flat`` return: one row per pair (``tvc_sim_rows``, include/tvc.h)."""
    values: torch.Tensor         # fp64 [B, 5]: cosine, Euclidean, Manhattan, Pearson, Spearman (NaN where undefined)
    ints: torch.Tensor           # int64 [B, 4]: the sums of cx cy, cx cx, cy cy over the centred doubled ranks; the NaN elements

    COLUMNS = ("cosine_similarity", "euclidean_distance", "manhattan_distance", "pearson_correlation", "spearman_correlation")


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _require_cuda(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (got {t.device}); the TVC path has no CPU fallback")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _check_out(out: torch.Tensor, J: int, I: int, dtype, name: str = "out") -> int:
    """The row pitch of a GEMM output: ``out`` must be a [J, >= I] matrix of unit column stride and of the epilogue's
    dtype on the GPU (a column view of a wider buffer is fine: its row stride becomes ``ld_out``)."""
    if not out.is_cuda:
        raise ValueError(f"{name} must live on the GPU (got {out.device})")
    if out.dtype != dtype:
        raise ValueError(f"{name} must be {dtype} for this epilogue (got {out.dtype})")
    if out.dim() != 2 or out.shape[0] != J or out.shape[1] < I or out.stride(1) != 1 or (J > 1 and out.stride(0) < I):
        raise ValueError(f"{name} must be [{J}, >= {I}] with unit column stride (got shape {tuple(out.shape)}, "
                         f"strides {tuple(out.stride())})")
    return out.stride(0)


class TVCEngine:
    """Owns a ``tvc_handle`` and the device copies of the tower weights."""

    def __init__(self, arch: Optional[ClipArch] = None, vision_w: Optional[Dict] = None,
                 text_w: Optional[Dict] = None, device: str = "cuda:0", precision: str = "bf16",
                 grad_precision: str = "bf16"):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.TVCError(_lib.TVC_E_HIP, "no GPU visible to PyTorch-ROCm; the TVC path has no CPU fallback")
        self.device = torch.device(device)
        self.arch = arch
        self._lock = threading.Lock()
        self.dense_fallbacks = 0           # searches that overflowed the candidate lists and were redone brute force
        self._keep = []          # device tensors / ctypes objects referenced by the handle
        # named bank slots: every owner (retriever index, ReferenceBank, defense references ...) registers
        # its rows under its own name, so owners sharing one engine cannot replace each other's bank
        self._banks: Dict[str, Dict] = {}
        self.handle = C.c_void_p()
        with torch.cuda.device(self.device):
            desc = vis = txt = None
            if arch is not None:
                desc = _lib.ModelDesc(arch.image_size, arch.patch, arch.vocab, arch.ctx, arch.embed_dim,
                                      _lib.TowerArch(arch.vision.width, arch.vision.layers, arch.vision.heads, arch.vision.mlp,
                                                     int(arch.vision.act == "gelu")),
                                      _lib.TowerArch(arch.text.width, arch.text.layers, arch.text.heads, arch.text.mlp,
                                                     int(arch.text.act == "gelu")))
                if vision_w is not None:
                    vis = self._vision_struct(arch, vision_w)
                if text_w is not None:
                    txt = self._text_struct(arch, text_w)
            rc = self.lib.tvc_create(C.byref(desc) if desc is not None else None,
                                     C.byref(vis) if vis is not None else None,
                                     C.byref(txt) if txt is not None else None, C.byref(self.handle))
            _lib.check(None, rc)
        self._w_host = (vision_w, text_w)     # the caller's (fp32) weight dicts: the fp32-grade mode uploads them as they are
        self._has_f32 = False
        self._has_f16 = False
        self.precision = "bf16"
        self.sd_precision = "bf16"            # TVC_OPT_SD_PRECISION (set_sd_precision): the latent-diffusion model's 16-bit format
        self.grad_precision = "bf16"          # TVC_OPT_GRAD_PRECISION (set_grad_precision): the input-gradient entry points' mode
        self._grad_pair = None                # the option value the last encode_image_grad ran under, when it named one
        if precision != "bf16":
            self.set_precision(precision)
        if grad_precision != "bf16":
            self.set_grad_precision(grad_precision)

    # ---- weights -------------------------------------------------------
    def _layers_f32(self, layers) -> "C.Array":
        arr = (_lib.LayerWeights * len(layers))()
        for i, lw in enumerate(layers):
            for name in ("ln1_g", "ln1_b", "wqkv", "bqkv", "wo", "bo", "ln2_g", "ln2_b", "w1", "b1", "w2", "b2"):
                setattr(arr[i], name, self._dev(lw[name], torch.float32).data_ptr())
        self._keep.append(arr)
        return arr

    def _upload_f32_weights(self) -> None:
        """fp32 copies of every weight for ``TVC_OPT_TOWER_PRECISION = 1`` (nothing rounded to bf16)."""
        vw, tw = self._w_host
        vis = txt = None
        if vw is not None:
            vis = _lib.VisionWeights()
            for name in ("patch_w", "cls", "pos", "ln_pre_g", "ln_pre_b", "ln_post_g", "ln_post_b", "proj"):
                setattr(vis, name, self._dev(vw[name], torch.float32).data_ptr())
            vis.layers = C.cast(self._layers_f32(vw["layers"]), C.POINTER(_lib.LayerWeights))
            self._keep.append(vis)
        if tw is not None:
            txt = _lib.TextWeights()
            for name in ("tok_emb", "pos", "ln_final_g", "ln_final_b", "proj"):
                setattr(txt, name, self._dev(tw[name], torch.float32).data_ptr())
            txt.layers = C.cast(self._layers_f32(tw["layers"]), C.POINTER(_lib.LayerWeights))
            self._keep.append(txt)
        self._check(self.lib.tvc_set_weights_f32(self.handle, C.byref(vis) if vis is not None else None,
                                                 C.byref(txt) if txt is not None else None))
        self._has_f32 = True

    PRECISIONS = {"bf16": 0, "fp32": 1, "split": 2, "fp16": 3}

    def set_precision(self, precision: str) -> None:
        """Tower arithmetic (``TVC_OPT_TOWER_PRECISION``):

        * ``"bf16"`` (default, the benchmarked path): bf16 x bf16 products, fp32 accumulation; scores within ~1e-3 of the
          reference's fp32 CPU path;
        * ``"split"``: fp32-grade at about a third of the bf16 matrix rate -- every activation and weight travels as
          hi | lo bf16 planes, three MFMA products per element; scores within 1e-4 of the fp32 CPU path END TO END (the
          bar of BASELINE.json), EOT packing / prefix sharing kept;
        * ``"fp32"``: the exact reference -- every GEMM on the exact-f32 matrix instruction (1/16 of the bf16 rate),
          fp32 attention; embeddings within ~1e-6 of the fp32 CPU path;
        * ``"fp16"``: the bf16 path with IEEE fp16 weights and 16-bit activations (the reference runs its towers in fp16)
          at the bf16 rate; 3 more mantissa bits than bf16, but a value beyond 65504 becomes inf (never clamped).

        ``"split"`` and ``"fp32"`` upload fp32 copies of the caller's weights, ``"fp16"`` fp16 copies (rounded to nearest
        even on the host).  The input-gradient entry points
        (``encode_image_grad`` / ``encode_image_backward``: the attack loops) do not follow this: see
        ``set_grad_precision``."""
        if precision not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(self.PRECISIONS)} (got {precision!r})")
        with self._lock, torch.cuda.device(self.device):
            if precision in ("fp32", "split") and not self._has_f32:
                if self._w_host[0] is None and self._w_host[1] is None:
                    raise _lib.TVCError(_lib.TVC_E_STATE, "this engine has no towers to run in fp32")
                self._upload_f32_weights()
            if precision == "fp16" and not self._has_f16:
                if self._w_host[0] is None and self._w_host[1] is None:
                    raise _lib.TVCError(_lib.TVC_E_STATE, "this engine has no towers to run in fp16")
                self._upload_f16_weights()
            self._check(self.lib.tvc_set_option(self.handle, _lib.TVC_OPT_TOWER_PRECISION, self.PRECISIONS[precision]))
        self.precision = precision

    GRAD_PRECISIONS = {"bf16": 0, "split": 2}

    def _grad_option(self, value: int) -> None:
        """``TVC_OPT_GRAD_PRECISION`` under the held lock; mode 2 first uploads the fp32 weights it is built from, when the
        engine has host weights it has not uploaded yet (without them the C-ABI reports what is missing at the forward)."""
        if value == 2 and not self._has_f32 and self._w_host[0] is not None:
            self._upload_f32_weights()
        self._check(self.lib.tvc_set_option(self.handle, _lib.TVC_OPT_GRAD_PRECISION, value))

    def set_grad_precision(self, precision: str) -> None:
        """Arithmetic of ``encode_image_grad`` / ``encode_image_backward`` (``TVC_OPT_GRAD_PRECISION``), independent of
        ``set_precision``: ``"bf16"`` (default) or ``"split"`` -- the vision tower forward and backward at fp32 grade (three
        bf16 MFMA products per element on hi | lo planes, fp32 activations, kept state and gradients)."""
        if precision not in self.GRAD_PRECISIONS:
            raise ValueError(f"grad_precision must be one of {sorted(self.GRAD_PRECISIONS)} (got {precision!r})")
        with self._lock, torch.cuda.device(self.device):
            self._grad_option(self.GRAD_PRECISIONS[precision])
        self.grad_precision = precision

    def _upload_f16_weights(self) -> None:
        """IEEE fp16 copies of every GEMM weight for ``TVC_OPT_TOWER_PRECISION = 3`` (rounded on the host: ``.to(float16)``
        is round-to-nearest-even; the fp32 tensors are uploaded as for the bf16 set)."""
        vw, tw = self._w_host
        vis = self._vision_struct(self.arch, vw, torch.float16) if vw is not None else None
        txt = self._text_struct(self.arch, tw, torch.float16) if tw is not None else None
        self._check(self.lib.tvc_set_weights_f16(self.handle, C.byref(vis) if vis is not None else None,
                                                 C.byref(txt) if txt is not None else None))
        self._has_f16 = True

    def _dev(self, t: torch.Tensor, dtype) -> torch.Tensor:
        if dtype == torch.float16:
            t = t.detach().cpu().float().to(torch.float16)      # round on the host (round to nearest even, overflow -> inf)
        d = t.detach().to(device=self.device, dtype=dtype).contiguous()
        self._keep.append(d)
        return d

    def _layers(self, layers, wdtype=torch.bfloat16) -> "C.Array":
        arr = (_lib.LayerWeights * len(layers))()
        for i, lw in enumerate(layers):
            for name in ("ln1_g", "ln1_b", "bqkv", "bo", "ln2_g", "ln2_b", "b1", "b2"):
                setattr(arr[i], name, self._dev(lw[name], torch.float32).data_ptr())
            for name in ("wqkv", "wo", "w1", "w2"):
                setattr(arr[i], name, self._dev(lw[name], wdtype).data_ptr())
        self._keep.append(arr)
        return arr

    def _vision_struct(self, arch: ClipArch, w: Dict, wdtype=torch.bfloat16) -> _lib.VisionWeights:
        """wdtype: the 16-bit type of the GEMM weights (bf16: tvc_create; fp16: tvc_set_weights_f16)."""
        s = _lib.VisionWeights()
        pw = torch.zeros((arch.vision.width, arch.patch_k_padded), dtype=torch.float32)
        pw[:, :arch.patch_k] = w['patch_w'].float().cpu()
        s.patch_w = self._dev(pw, wdtype).data_ptr()
        for name in ("cls", "pos", "ln_pre_g", "ln_pre_b", "ln_post_g", "ln_post_b"):
            setattr(s, name, self._dev(w[name], torch.float32).data_ptr())
        s.proj = self._dev(w['proj'], wdtype).data_ptr()
        s.layers = C.cast(self._layers(w['layers'], wdtype), C.POINTER(_lib.LayerWeights))
        self._keep.append(s)
        return s

    def _text_struct(self, arch: ClipArch, w: Dict, wdtype=torch.bfloat16) -> _lib.TextWeights:
        s = _lib.TextWeights()
        for name in ("tok_emb", "pos", "ln_final_g", "ln_final_b"):
            setattr(s, name, self._dev(w[name], torch.float32).data_ptr())
        s.proj = self._dev(w['proj'], wdtype).data_ptr()
        s.layers = C.cast(self._layers(w['layers'], wdtype), C.POINTER(_lib.LayerWeights))
        self._keep.append(s)
        return s

    def close(self) -> None:
        if getattr(self, "handle", None) and self.handle.value:
            torch.cuda.synchronize(self.device)
            self.lib.tvc_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        _lib.check(self.handle, rc)

    # ---- encoders ------------------------------------------------------
    def encode_image(self, pixels: torch.Tensor, normalize: bool = True) -> torch.Tensor:
        """pixels [B, 3, S, S] (preprocessed, on the GPU) -> fp32 [B, D]."""
        a = self.arch
        if pixels.dim() == 3:
            pixels = pixels.unsqueeze(0)
        if pixels.dim() != 4 or pixels.shape[1:] != (3, a.image_size, a.image_size):
            raise ValueError(f"expected [B, 3, {a.image_size}, {a.image_size}], got {tuple(pixels.shape)}")
        pixels = _require_cuda(pixels, torch.float32, "pixels")
        out = torch.empty((pixels.shape[0], a.embed_dim), dtype=torch.float32, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_encode_image(self.handle, _ptr(pixels), pixels.shape[0], _ptr(out),
                                                  int(normalize), _stream()))
        return out

    def encode_text_hidden(self, tokens: torch.Tensor) -> torch.Tensor:
        """tokens int [T, ctx] (on the GPU) -> fp32 [T, ctx, width]: ln_final of the hidden state at every position
        (``CLIPTextModel.last_hidden_state``; the conditioning a latent-diffusion UNet takes)."""
        a = self.arch
        if tokens.dim() != 2 or tokens.shape[1] != a.ctx:
            raise ValueError(f"expected [T, {a.ctx}] tokens, got {tuple(tokens.shape)}")
        tokens = _require_cuda(tokens, torch.int32, "tokens")
        out = torch.empty((tokens.shape[0], a.ctx, a.text.width), dtype=torch.float32, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_encode_text_hidden(self.handle, _ptr(tokens), tokens.shape[0], _ptr(out), _stream()))
        return out

    # ---- input gradient of the vision tower (attacks: PGD / Hubness inner loop) ----------------
    def encode_image_grad(self, pixels: torch.Tensor, normalize: bool = True, precision: Optional[str] = None) -> torch.Tensor:
        """As ``encode_image`` but keeps what ``encode_image_backward`` needs inside the handle.  ``pixels`` must stay
        alive and unchanged until the backward (the engine holds a reference).  ``precision``: ``None`` = the engine's
        gradient precision (``set_grad_precision``); ``"bf16"`` / ``"split"`` = that mode for this forward and its backward(s),
        the option set and put back under the engine lock around each of the calls."""
        if precision is not None and precision not in self.GRAD_PRECISIONS:
            raise ValueError(f"precision must be None or one of {sorted(self.GRAD_PRECISIONS)} (got {precision!r})")
        a = self.arch
        if pixels.dim() != 4 or pixels.shape[1:] != (3, a.image_size, a.image_size):
            raise ValueError(f"expected [B, 3, {a.image_size}, {a.image_size}], got {tuple(pixels.shape)}")
        pixels = _require_cuda(pixels, torch.float32, "pixels")
        out = torch.empty((pixels.shape[0], a.embed_dim), dtype=torch.float32, device=self.device)
        pair = None if precision is None else self.GRAD_PRECISIONS[precision]
        with self._lock, torch.cuda.device(self.device):
            with self._grad_mode(pair):
                self._check(self.lib.tvc_encode_image_grad(self.handle, _ptr(pixels), pixels.shape[0], _ptr(out),
                                                           int(normalize), _stream()))
            self._grad_pair = pair
            self._grad_pixels = pixels
            self._grad_generation = getattr(self, "_grad_generation", 0) + 1
        return out

    def encode_image_backward(self, grad_out: torch.Tensor, generation: Optional[int] = None) -> torch.Tensor:
        """d(loss)/d(out of the last ``encode_image_grad``) [B, D] -> d(loss)/d(pixels) [B, 3, S, S]."""
        px = getattr(self, "_grad_pixels", None)
        if px is None:
            raise RuntimeError("encode_image_backward: no encode_image_grad call to differentiate")
        if generation is not None and generation != self._grad_generation:
            raise RuntimeError("encode_image_backward: a later encode_image_grad call replaced the saved activations "
                               "(one differentiable image batch at a time per engine)")
        grad_out = _require_cuda(grad_out, torch.float32, "grad_out")
        if tuple(grad_out.shape) != (px.shape[0], self.arch.embed_dim):
            raise ValueError(f"grad_out must be [{px.shape[0]}, {self.arch.embed_dim}], got {tuple(grad_out.shape)}")
        gp = torch.empty_like(px)
        with self._lock, torch.cuda.device(self.device), self._grad_mode(self._grad_pair):
            self._check(self.lib.tvc_encode_image_backward(self.handle, _ptr(grad_out), _ptr(gp), _stream()))
        return gp

    @contextlib.contextmanager
    def _grad_mode(self, value: Optional[int]):
        """Under the held lock: ``TVC_OPT_GRAD_PRECISION`` = value for the body, the engine's configured mode after it."""
        if value is None or value == self.GRAD_PRECISIONS[self.grad_precision]:
            yield
            return
        self._grad_option(value)
        try:
            yield
        finally:
            self._check(self.lib.tvc_set_option(self.handle, _lib.TVC_OPT_GRAD_PRECISION, self.GRAD_PRECISIONS[self.grad_precision]))

    def pgd_step(self, adv: torch.Tensor, clean: torch.Tensor, grad: torch.Tensor, momentum: Optional[torch.Tensor],
                 eps: float, alpha: float, mu: float = 0.9, clip_min: float = 0.0, clip_max: float = 1.0,
                 targeted: bool = False) -> None:
        """One projected sign-gradient step, in place on ``adv`` (and ``momentum``)."""
        for name, t in (("adv", adv), ("clean", clean), ("grad", grad), ("momentum", momentum)):
            if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == adv.shape):
                raise ValueError(f"{name}: contiguous fp32 device tensor shaped like adv expected")
        B = adv.shape[0]
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_pgd_step(self.handle, _ptr(adv), _ptr(clean), _ptr(grad), _ptr(momentum), B,
                                              adv.numel() // max(B, 1), eps, alpha, mu, clip_min, clip_max,
                                              int(targeted), _stream()))

    def l2_step(self, adv: torch.Tensor, clean: torch.Tensor, grad: torch.Tensor, eps: float, step: float,
                clip_min: float = 0.0, clip_max: float = 1.0, descent: bool = True) -> None:
        """One L2-normalised gradient step + projection onto the eps L2 ball + clamp, in place on ``adv``
        (src/attacks/hubness_attack.py:378-386)."""
        for name, t in (("adv", adv), ("clean", clean), ("grad", grad)):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == adv.shape):
                raise ValueError(f"{name}: contiguous fp32 device tensor shaped like adv expected")
        B = adv.shape[0]
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_l2_step(self.handle, _ptr(adv), _ptr(clean), _ptr(grad), B, adv.numel() // max(B, 1),
                                             eps, step, clip_min, clip_max, int(descent), _stream()))

    def attack_feature_grad(self, f: torch.Tensor, t: torch.Tensor, g: torch.Tensor, *, a_tgt: float, a_txt: float,
                            metric: str = "cosine", w_out: float = 0.0, w_div: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
        """Embedding gradient of the FSTA / SMA feature loss (``tvc_attack_feature_grad``, formulas in include/tvc.h):
        f, t, g fp32 [B, D] (image, text, target rows) -> (grad [B, D], loss_rows [B, 4]).  The gradient is what
        ``encode_image_backward`` takes; the loss terms are means of the columns of ``loss_rows``."""
        if metric not in ("cosine", "euclidean"):
            raise ValueError(f"metric must be 'cosine' or 'euclidean' (got {metric!r})")
        if f.dim() != 2:
            raise ValueError(f"f: [B, D] expected, got {tuple(f.shape)}")
        for name, x in (("f", f), ("t", t), ("g", g)):
            if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape == f.shape):
                raise ValueError(f"{name}: contiguous fp32 device tensor shaped like f expected")
        B, D = f.shape
        grad = torch.empty_like(f)
        loss_rows = torch.empty((B, 4), dtype=torch.float32, device=f.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_attack_feature_grad(self.handle, _ptr(f), _ptr(t), _ptr(g), B, D, a_tgt, a_txt,
                                                         int(metric == "euclidean"), w_out, w_div, _ptr(grad),
                                                         _ptr(loss_rows), _stream()))
        return grad, loss_rows

    def attack_step(self, adv: torch.Tensor, clean: torch.Tensor, grad: torch.Tensor, mom: torch.Tensor, eps: float,
                    lr: float, mu: float, clip: float, p: float, clip_min: float, clip_max: float, norm: str = "inf") -> None:
        """One FSTA / SMA step, in place on ``adv`` and ``mom`` (``tvc_attack_step``): gradient clamp (``clip`` > 0), the
        pixel-space term ``p * (adv - clean)``, un-normalised momentum, then the sign step and L-inf ball (``norm='inf'``) or
        the momentum step and L2 ball (``'l2'``), and the clamp to [clip_min, clip_max]."""
        if norm not in ("inf", "l2"):
            raise ValueError(f"norm must be 'inf' or 'l2' (got {norm!r})")
        for name, x in (("adv", adv), ("clean", clean), ("grad", grad), ("mom", mom)):
            if x is None or not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape == adv.shape):
                raise ValueError(f"{name}: contiguous fp32 device tensor shaped like adv expected")
        B = adv.shape[0]
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_attack_step(self.handle, _ptr(adv), _ptr(clean), _ptr(grad), _ptr(mom), B,
                                                 adv.numel() // max(B, 1), eps, lr, mu, clip, p, clip_min, clip_max,
                                                 int(norm == "l2"), _stream()))

    def encode_text(self, tokens: torch.Tensor, normalize: bool = True, group: int = 0) -> torch.Tensor:
        """tokens int [T, ctx] (on the GPU) -> fp32 [T, D].  ``group`` = N + 1 declares that the rows
        are consecutive (original, variant_1 .. variant_N) groups: variants then share the rows of
        the token prefix they have in common with their original (``TVC_OPT_TEXT_GROUP``; the
        embeddings are bit-identical, the text tower does less work)."""
        a = self.arch
        if tokens.dim() != 2 or tokens.shape[1] != a.ctx:
            raise ValueError(f"expected [T, {a.ctx}] token ids, got {tuple(tokens.shape)}")
        tokens = _require_cuda(tokens, torch.int32, "tokens")
        out = torch.empty((tokens.shape[0], a.embed_dim), dtype=torch.float32, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            if group >= 2:
                self._check(self.lib.tvc_set_option(self.handle, _lib.TVC_OPT_TEXT_GROUP, int(group)))
            try:
                self._check(self.lib.tvc_encode_text(self.handle, _ptr(tokens), tokens.shape[0], _ptr(out),
                                                     int(normalize), _stream()))
            finally:
                if group >= 2:
                    self._check(self.lib.tvc_set_option(self.handle, _lib.TVC_OPT_TEXT_GROUP, 0))
        return out

    # ---- bank ----------------------------------------------------------
    DEFAULT_BANK = "default"

    def _slot(self, name: str, create: bool = False) -> Dict:
        b = self._banks.get(name)
        if b is None:
            if not create:
                raise _lib.TVCError(_lib.TVC_E_STATE, f"no bank registered under the name {name!r}")
            used = {v["slot"] for v in self._banks.values()}
            free = [i for i in range(_lib.TVC_MAX_BANKS) if i not in used]
            if not free:
                raise _lib.TVCError(_lib.TVC_E_STATE, f"all {_lib.TVC_MAX_BANKS} bank slots of this engine are in use "
                                                      f"({sorted(self._banks)}); release_bank() one first")
            b = self._banks[name] = {"slot": free[0], "rows": 0, "dim": 0, "keep": None}
        return b

    def _select(self, name: str, create: bool = False) -> Dict:
        """(lock held) point the handle's bank calls at the slot of ``name``."""
        b = self._slot(name, create)
        self._check(self.lib.tvc_bank_select(self.handle, b["slot"]))
        return b

    @property
    def bank_rows(self) -> int:
        return self.bank_size(self.DEFAULT_BANK)

    @property
    def bank_dim(self) -> int:
        b = self._banks.get(self.DEFAULT_BANK)
        return b["dim"] if b else 0

    def bank_size(self, name: str = DEFAULT_BANK) -> int:
        b = self._banks.get(name)
        return b["rows"] if b else 0

    def has_bank(self, name: str = DEFAULT_BANK) -> bool:
        return name in self._banks

    def bank_is_bf16(self, name: str = DEFAULT_BANK) -> bool:
        """True when the bank of ``name`` was registered as bf16 (its rows are exact in bf16)."""
        b = self._banks.get(name)
        return bool(b and b.get("bf16"))

    def set_bank(self, bank: torch.Tensor, name: str = DEFAULT_BANK) -> None:
        """bank [R, D], rows L2-normalised; bf16 is used in place, fp32 is split
        into (hi, lo) bf16 planes inside the handle.  ``name`` = the owner's slot."""
        if bank.dim() != 2:
            raise ValueError("bank must be [R, D]")
        if bank.dtype not in (torch.bfloat16, torch.float32):
            bank = bank.float()
        bank = _require_cuda(bank, bank.dtype, "bank")
        dt = _lib.TVC_DTYPE_BF16 if bank.dtype == torch.bfloat16 else _lib.TVC_DTYPE_F32
        with self._lock, torch.cuda.device(self.device):
            b = self._select(name, create=True)
            self._check(self.lib.tvc_bank_set(self.handle, _ptr(bank), bank.shape[0], bank.shape[1], dt, _stream()))
            if dt == _lib.TVC_DTYPE_F32:
                torch.cuda.current_stream().synchronize()   # the split read `bank`; it may now be freed
            b["keep"] = bank if dt == _lib.TVC_DTYPE_BF16 else None
            b["bf16"] = dt == _lib.TVC_DTYPE_BF16
            b["rows"], b["dim"] = bank.shape

    def release_bank(self, name: str) -> None:
        """Forget the bank of ``name`` and free its slot (an fp32 bank's planes are freed too)."""
        with self._lock, torch.cuda.device(self.device):
            if name in self._banks:
                self._select(name)
                self._check(self.lib.tvc_bank_set(self.handle, None, 0, 64, _lib.TVC_DTYPE_BF16, _stream()))
                del self._banks[name]

    def bank_search(self, rows: torch.Tensor, k: int, count_thr: float = 0.3, idx_offset: int = 0,
                    want_moments: bool = True, bank: str = DEFAULT_BANK):
        """rows fp32 [M, D] -> (idx int32 [M, k], sim fp32 [M, k], moments fp32 [M, 4] | None)."""
        if not 1 <= k <= _lib.TVC_MAX_TOPK:
            raise ValueError(f"top-k must be in [1, {_lib.TVC_MAX_TOPK}] (got {k}): tvc_bank_search never truncates silently")
        rows = _require_cuda(rows, torch.float32, "rows")
        M = rows.shape[0]
        idx = torch.empty((M, k), dtype=torch.int32, device=self.device)
        sim = torch.empty((M, k), dtype=torch.float32, device=self.device)
        mom = torch.empty((M, 4), dtype=torch.float32, device=self.device) if want_moments else None
        with self._lock, torch.cuda.device(self.device):
            self._select(bank)
            self._check(self.lib.tvc_bank_search(self.handle, _ptr(rows), M, k, count_thr, idx_offset,
                                                 _ptr(idx), _ptr(sim), _ptr(mom), _stream()))
        return idx, sim, mom

    def bank_search_robust(self, rows: torch.Tensor, k: int, count_thr: float = 0.3, idx_offset: int = 0,
                           want_moments: bool = True, bank: str = DEFAULT_BANK):
        """``bank_search`` + status check; on candidate overflow (degenerate bank) the same
        contract is recomputed by the brute-force kernel.  Synchronises the stream."""
        out = self.bank_search(rows, k, count_thr, idx_offset, want_moments, bank)
        try:
            self.bank_status()
            return out
        except _lib.TVCError as e:
            if e.code != _lib.TVC_E_OVERFLOW:
                raise
        out = self.bank_search_dense(rows, k, count_thr, idx_offset, want_moments, bank, out=out)
        self.dense_fallbacks += 1
        return out

    def bank_search_dense(self, rows: torch.Tensor, k: int, count_thr: float = 0.3, idx_offset: int = 0,
                          want_moments: bool = True, bank: str = DEFAULT_BANK, out=None):
        """``bank_search``'s contract by the brute-force kernels (``tvc_bank_search_dense``): every similarity is
        materialised, nothing can overflow.  ``out``: the (idx, sim, moments) tensors of a ``bank_search`` call to fill."""
        if not 1 <= k <= _lib.TVC_MAX_TOPK:
            raise ValueError(f"top-k must be in [1, {_lib.TVC_MAX_TOPK}] (got {k})")
        rows = _require_cuda(rows, torch.float32, "rows")
        M = rows.shape[0]
        if out is None:
            out = (torch.empty((M, k), dtype=torch.int32, device=self.device),
                   torch.empty((M, k), dtype=torch.float32, device=self.device),
                   torch.empty((M, 4), dtype=torch.float32, device=self.device) if want_moments else None)
        idx, sim, mom = out
        with self._lock, torch.cuda.device(self.device):
            self._select(bank)
            self._check(self.lib.tvc_bank_search_dense(self.handle, _ptr(rows), M, k, count_thr, idx_offset,
                                                       _ptr(idx), _ptr(sim), _ptr(mom), _stream()))
        return idx, sim, mom

    def bank_status(self) -> None:
        """Synchronise and raise ``TVCError(TVC_E_OVERFLOW)`` if the last search dropped candidates."""
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_bank_status(self.handle, _stream()))

    def bank_gather(self, idx: torch.Tensor, idx_offset: int = 0, bank: str = DEFAULT_BANK) -> torch.Tensor:
        idx = _require_cuda(idx, torch.int32, "idx")
        n = idx.numel()
        with self._lock, torch.cuda.device(self.device):
            b = self._select(bank)
            out = torch.empty((n, b["dim"]), dtype=torch.float32, device=self.device)
            self._check(self.lib.tvc_bank_gather(self.handle, _ptr(idx), n, idx_offset, _ptr(out), _stream()))
        return out.view(*idx.shape, b["dim"])

    # ---- k-means over a bank slot ----------------------------------------
    def kmeans_assign(self, centroids: torch.Tensor, bank: str = DEFAULT_BANK):
        """centroids fp32 [K, D] -> (labels int32 [R], score fp32 [R], dist2 fp32 [R]) over the rows of ``bank``:
        the Euclidean nearest centre of every row (ties: lowest centre index; -1 when every score is NaN), its score
        x.c - |c|^2 / 2 and the squared distance max(0, |x|^2 - 2 score)."""
        centroids = _require_cuda(centroids, torch.float32, "centroids")
        with self._lock, torch.cuda.device(self.device):
            b = self._select(bank)
            if centroids.dim() != 2 or centroids.shape[1] != b["dim"]:
                raise ValueError(f"centroids must be [K, {b['dim']}] (got {tuple(centroids.shape)})")
            R = b["rows"]
            labels = torch.empty(R, dtype=torch.int32, device=self.device)
            score = torch.empty(R, dtype=torch.float32, device=self.device)
            dist2 = torch.empty(R, dtype=torch.float32, device=self.device)
            self._check(self.lib.tvc_kmeans_assign(self.handle, _ptr(centroids), centroids.shape[0], _ptr(labels), _ptr(score),
                                                   _ptr(dist2), _stream()))
        return labels, score, dist2

    def kmeans_update(self, labels: torch.Tensor, centroids: torch.Tensor, bank: str = DEFAULT_BANK, want_lists: bool = False):
        """labels int32 [R], centroids fp32 [K, D] -> (centres fp32 [K, D], counts int32 [K], offsets int32 [K + 1] | None,
        order int32 [R] | None): the mean of every cluster's rows (an empty cluster keeps its row of ``centroids``),
        bit-reproducible.  ``want_lists``: also the member lists -- ``order[offsets[j]:offsets[j + 1]]`` are cluster j's
        rows in ascending order; entries of ``order`` from ``offsets[K]`` on are -1 (rows labelled -1 are in no list)."""
        labels = _require_cuda(labels, torch.int32, "labels")
        centroids = _require_cuda(centroids, torch.float32, "centroids")
        with self._lock, torch.cuda.device(self.device):
            b = self._select(bank)
            if labels.shape != (b["rows"],):
                raise ValueError(f"labels must be [{b['rows']}] (got {tuple(labels.shape)})")
            if centroids.dim() != 2 or centroids.shape[1] != b["dim"]:
                raise ValueError(f"centroids must be [K, {b['dim']}] (got {tuple(centroids.shape)})")
            K = centroids.shape[0]
            out = torch.empty_like(centroids)
            counts = torch.empty(K, dtype=torch.int32, device=self.device)
            offsets = torch.empty(K + 1, dtype=torch.int32, device=self.device) if want_lists else None
            order = torch.full((b["rows"],), -1, dtype=torch.int32, device=self.device) if want_lists else None
            self._check(self.lib.tvc_kmeans_update(self.handle, _ptr(labels), _ptr(centroids), K, _ptr(out), _ptr(counts),
                                                   _ptr(offsets), _ptr(order), _stream()))
        return out, counts, offsets, order

    def _kmeans_init(self, K: int, bank: str, init, rng) -> torch.Tensor:
        """The K starting centres of one restart; every random number comes from ``rng`` (a seeded CPU generator), drawn
        before the first kernel runs."""
        import numpy as np
        R = self.bank_size(bank)
        if init == "random":
            rows = rng.choice(R, K, replace=False)
            return self.bank_gather(torch.from_numpy(rows.astype(np.int32)).to(self.device), bank=bank)
        if init != "k-means++":
            raise ValueError(f"init must be 'k-means++', 'random' or a [K, D] tensor (got {init!r})")
        # D^2 sampling (Arthur & Vassilvitskii): centre j is row searchsorted(cumsum(d2), u[j] * sum(d2)), d2 = the squared
        # distance to the nearest centre chosen so far -- one K = 1 assign per centre
        u = rng.random(K)
        first = min(int(u[0] * R), R - 1)
        centres = [self.bank_gather(torch.tensor([first], dtype=torch.int32, device=self.device), bank=bank)]
        d2 = None
        for j in range(1, K):
            _, _, d = self.kmeans_assign(centres[-1], bank=bank)
            d2 = d if d2 is None else torch.minimum(d2, d)
            cum = torch.cumsum(d2.double(), 0)
            target = (cum[-1] * float(u[j])).reshape(1)
            row = torch.searchsorted(cum, target, right=True).clamp_(max=R - 1).to(torch.int32)
            centres.append(self.bank_gather(row, bank=bank))
        return torch.cat(centres, 0)

    def kmeans(self, K: int, bank: str = DEFAULT_BANK, init="k-means++", n_init: int = 10, max_iter: int = 300,
               tol: float = 1e-4, seed=42, n_features: Optional[int] = None):
        """Lloyd's k-means over the rows of ``bank`` -> (centres fp32 [K, D], labels int32 [R], inertia float, n_iter int,
        order int32 [R], offsets int32 [K + 1]) of the best of ``n_init`` restarts (lowest inertia, the earliest restart
        on equality).  ``KMeans(n_clusters=K, n_init=n_init, max_iter=max_iter, tol=tol)`` of src/ref_bank.py:298 with the
        arithmetic in ``tvc_kmeans_assign`` / ``tvc_kmeans_update``; this loop is Python, as the PGD loop is.

        * init: ``"k-means++"`` (D^2 sampling), ``"random"`` (K distinct rows) or a tensor [K, D] (one restart).  Restart
          i draws from ``numpy.random.default_rng(seed + i)`` (``seed`` may also be a sequence of ``n_init`` seeds), so a
          run is reproducible; the starting centres of the returned restart are kept in ``self.kmeans_last_init``.
        * stop rule (sklearn's): the labels did not change, or sum |c_new - c_old|^2 <= tol * the mean over the
          ``n_features`` features (default: the bank's D) of the data's variance; then one final assign, so the returned
          labels, inertia (``dist2.double().sum()``), ``order`` and ``offsets`` belong to the returned centres.
        * empty clusters: after an update the e empty clusters take the e rows with the largest ``dist2`` (ties: the lower
          row index), handed out in that order to the empty clusters in ascending id, and the loop goes on.  This is
          sklearn's ``_relocate_empty_clusters`` WITHOUT the subtraction: the donor clusters' centres are not adjusted
          for the row they gave away (the next update recomputes them anyway)."""
        import numpy as np
        R = self.bank_size(bank)
        if not 1 <= K <= R:
            raise ValueError(f"need 1 <= K <= R = {R} (got K = {K})")
        fixed = isinstance(init, torch.Tensor)
        if fixed:
            init = _require_cuda(init, torch.float32, "init")
            n_init = 1
        seeds = [int(s) for s in seed] if isinstance(seed, (list, tuple)) else [int(seed) + i for i in range(n_init)]
        if len(seeds) != n_init:
            raise ValueError(f"seed must be an int or a sequence of n_init = {n_init} ints")
        # the data's variance from the kernels themselves: the K = 1 update is the mean row, its assign the squared deviations
        zero = torch.zeros(R, dtype=torch.int32, device=self.device)
        mean, _, _, _ = self.kmeans_update(zero, torch.zeros((1, self._banks[bank]["dim"]), device=self.device), bank=bank)
        _, _, dev2 = self.kmeans_assign(mean, bank=bank)
        tol_abs = tol * dev2.double().sum().item() / (R * (n_features or self._banks[bank]["dim"]))
        best = None
        for s in seeds:
            C0 = init if fixed else self._kmeans_init(K, bank, init, np.random.default_rng(s))
            Cc, prev, n_iter = C0, None, 0
            for it in range(max_iter):
                labels, _, d2 = self.kmeans_assign(Cc, bank=bank)
                Cn, counts, _, _ = self.kmeans_update(labels, Cc, bank=bank)
                empty = (counts == 0).nonzero().flatten()
                if empty.numel():
                    far = torch.sort(d2, descending=True, stable=True).indices[:empty.numel()].to(torch.int32)
                    Cn[empty] = self.bank_gather(far, bank=bank)
                n_iter = it + 1
                shift = (Cn - Cc).double().pow(2).sum().item()
                Cc = Cn
                if prev is not None and torch.equal(labels, prev):
                    break
                if shift <= tol_abs:
                    break
                prev = labels
            labels, _, d2 = self.kmeans_assign(Cc, bank=bank)
            inertia = d2.double().sum().item()
            if best is None or inertia < best[2]:
                best = (Cc, labels, inertia, n_iter, C0)
        Cc, labels, inertia, n_iter, C0 = best
        self.kmeans_last_init = C0
        _, _, offsets, order = self.kmeans_update(labels, Cc, bank=bank, want_lists=True)
        return Cc, labels, inertia, n_iter, order, offsets

    # ---- retrieval evaluation over a bank slot -----------------------------
    RANK_MAX_K = 8

    def _rank_inputs(self, b: Dict, rows, qlabel, glabel, tgt_off):
        rows = _require_cuda(rows, torch.float32, "rows")
        if rows.dim() != 2 or rows.shape[1] != b["dim"]:
            raise ValueError(f"rows must be [M, {b['dim']}] (got {tuple(rows.shape)})")
        M = rows.shape[0]
        qlabel = _require_cuda(qlabel, torch.int32, "qlabel")
        glabel = _require_cuda(glabel, torch.int32, "glabel")
        tgt_off = _require_cuda(tgt_off, torch.int64, "tgt_off")
        if qlabel.shape != (M,) or glabel.shape != (b["rows"],) or tgt_off.shape != (M + 1,):
            raise ValueError(f"need qlabel [{M}], glabel [{b['rows']}] and tgt_off [{M + 1}] (got {tuple(qlabel.shape)}, "
                             f"{tuple(glabel.shape)}, {tuple(tgt_off.shape)})")
        return rows, M, qlabel, glabel, tgt_off

    def rank_targets(self, rows: torch.Tensor, qlabel: torch.Tensor, glabel: torch.Tensor, gpos: torch.Tensor,
                     tgt_off: torch.Tensor, T: int, bank: str = DEFAULT_BANK):
        """``tvc_rank_targets``: rows fp32 [M, D], qlabel int32 [M], glabel / gpos int32 [R], tgt_off int64 [M + 1], T =
        ``tgt_off[M]`` -> (tgt_sim fp32 [T], tgt_row int32 [T]), every query's relevant rows in ascending row order."""
        with self._lock, torch.cuda.device(self.device):
            b = self._select(bank)
            rows, M, qlabel, glabel, tgt_off = self._rank_inputs(b, rows, qlabel, glabel, tgt_off)
            gpos = _require_cuda(gpos, torch.int32, "gpos")
            if gpos.shape != glabel.shape:
                raise ValueError(f"gpos must be [{b['rows']}] (got {tuple(gpos.shape)})")
            tgt_sim = torch.empty(T, dtype=torch.float32, device=self.device)
            tgt_row = torch.empty(T, dtype=torch.int32, device=self.device)
            self._check(self.lib.tvc_rank_targets(self.handle, _ptr(rows), M, _ptr(qlabel), _ptr(glabel), _ptr(gpos), _ptr(tgt_off),
                                                  T, _ptr(tgt_sim), _ptr(tgt_row), _stream()))
        return tgt_sim, tgt_row

    def rank_count(self, rows: torch.Tensor, qlabel: torch.Tensor, glabel: torch.Tensor, tgt_off: torch.Tensor,
                   tgt_sim: torch.Tensor, tgt_row: torch.Tensor, bank: str = DEFAULT_BANK) -> torch.Tensor:
        """``tvc_rank_count``: the lists of ``rank_targets`` with every query's in rank order -> hist int32 [T]."""
        with self._lock, torch.cuda.device(self.device):
            b = self._select(bank)
            rows, M, qlabel, glabel, tgt_off = self._rank_inputs(b, rows, qlabel, glabel, tgt_off)
            tgt_sim = _require_cuda(tgt_sim, torch.float32, "tgt_sim")
            tgt_row = _require_cuda(tgt_row, torch.int32, "tgt_row")
            T = tgt_sim.numel()
            if tgt_sim.dim() != 1 or tgt_row.shape != tgt_sim.shape:
                raise ValueError(f"tgt_sim and tgt_row must be [T] (got {tuple(tgt_sim.shape)}, {tuple(tgt_row.shape)})")
            hist = torch.zeros(T, dtype=torch.int32, device=self.device)
            self._check(self.lib.tvc_rank_count(self.handle, _ptr(rows), M, _ptr(qlabel), _ptr(glabel), _ptr(tgt_off), _ptr(tgt_sim),
                                                _ptr(tgt_row), T, _ptr(hist), _stream()))
        return hist

    def rank_metrics(self, tgt_off: torch.Tensor, hist: torch.Tensor, k_values=(1, 5, 10), bank: str = DEFAULT_BANK):
        """``tvc_rank_metrics``: tgt_off int64 [M + 1], hist int32 [T] -> (pos int32 [T], ap fp64 [M], rr fp64 [M], hits int32
        [M, n_k], dcg fp64 [M, n_k], idcg fp64 [M, n_k])."""
        tgt_off = _require_cuda(tgt_off, torch.int64, "tgt_off")
        hist = _require_cuda(hist, torch.int32, "hist")
        ks = [int(k) for k in k_values]
        M, T, n_k = tgt_off.numel() - 1, hist.numel(), len(ks)
        karr = (C.c_int32 * max(n_k, 1))(*ks)
        with self._lock, torch.cuda.device(self.device):
            self._select(bank)
            pos = torch.empty(T, dtype=torch.int32, device=self.device)
            ap = torch.empty(max(M, 0), dtype=torch.float64, device=self.device)
            rr = torch.empty_like(ap)
            hits = torch.empty((max(M, 0), n_k), dtype=torch.int32, device=self.device)
            dcg = torch.empty((max(M, 0), n_k), dtype=torch.float64, device=self.device)
            idcg = torch.empty_like(dcg)
            self._check(self.lib.tvc_rank_metrics(self.handle, M, _ptr(tgt_off), _ptr(hist), T, karr, n_k, _ptr(pos), _ptr(ap),
                                                  _ptr(rr), _ptr(hits), _ptr(dcg), _ptr(idcg), _stream()))
        return pos, ap, rr, hits, dcg, idcg

    def rank_layout(self, qlabels: torch.Tensor, glabels: torch.Tensor):
        """Labels of any integer type -> (qlabel int32 [M], glabel int32 [R], gpos int32 [R], tgt_off int64 [M + 1]) for the rank
        calls: the non-negative gallery labels renumbered 0 .. G - 1 (negative ones stay -1), a query label no gallery row
        carries becomes -1, ``gpos[j]`` = the place of row j among the rows of its label in ascending row order, ``tgt_off``
        = the exclusive scan of the queries' group sizes.  Integer torch ops on the engine's device."""
        ql = torch.as_tensor(qlabels).to(self.device).long().reshape(-1)
        gl = torch.as_tensor(glabels).to(self.device).long().reshape(-1)
        R = gl.numel()
        valid = gl >= 0
        uniq, inv = torch.unique(gl[valid], return_inverse=True)
        G = uniq.numel()
        gc = torch.full((R,), -1, dtype=torch.int64, device=self.device)
        gc[valid] = inv
        counts = torch.bincount(inv, minlength=max(G, 1))
        # a stable sort by label puts every group in ascending row order behind the distractors
        order = torch.sort(gc, stable=True).indices
        start = torch.cumsum(counts, 0) - counts + (R - int(valid.sum()))
        gpos = torch.zeros(R, dtype=torch.int64, device=self.device)
        gpos[order] = torch.arange(R, device=self.device) - start[gc[order].clamp(min=0)]
        gpos[~valid] = 0
        if G:
            at = torch.searchsorted(uniq, ql.clamp(min=0)).clamp(max=G - 1)
            qc = torch.where((uniq[at] == ql) & (ql >= 0), at, torch.full_like(at, -1))
        else:
            qc = torch.full_like(ql, -1)
        sizes = torch.where(qc >= 0, counts[qc.clamp(min=0)], torch.zeros_like(qc))
        tgt_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), torch.cumsum(sizes, 0)])
        return qc.int(), gc.int(), gpos.int(), tgt_off

    def retrieval_ranks(self, rows: torch.Tensor, qlabels, glabels, bank: str = DEFAULT_BANK, k_values=(1, 5, 10)) -> RetrievalRanks:
        """The position of every relevant row of every query in its ranking of the rows of ``bank``, and the per-query metric
        terms (``RetrievalRanks``).  rows fp32 [M, D]; (i, j) is relevant iff ``qlabels[i] == glabels[j] >= 0``; the order is
        (score descending, row ascending), ``tvc_bank_search``'s.  Two tile passes over the slot (``tvc_rank_targets``,
        ``tvc_rank_count``) with two stable sorts of the T targets between them; no [M, R] matrix exists.  Synchronises (it
        reads T, and checks the target scores): an evaluation call.  ``ValueError`` for a non-finite target score."""
        ks = tuple(int(k) for k in k_values)
        if len(ks) > self.RANK_MAX_K or any(k < 1 for k in ks):
            raise ValueError(f"need at most {self.RANK_MAX_K} values of k, each >= 1 (got {ks})")
        rows = _require_cuda(rows, torch.float32, "rows")
        if rows.dim() != 2 or rows.shape[0] < 1:
            raise ValueError(f"rows must be [M >= 1, D] (got {tuple(rows.shape)})")
        M = rows.shape[0]
        with torch.cuda.device(self.device):
            qlabel, glabel, gpos, tgt_off = self.rank_layout(qlabels, glabels)
            if qlabel.numel() != M or glabel.numel() != self.bank_size(bank):
                raise ValueError(f"need {M} query labels and {self.bank_size(bank)} gallery labels "
                                 f"(got {qlabel.numel()}, {glabel.numel()})")
            T = int(tgt_off[-1])
            tgt_sim, tgt_row = self.rank_targets(rows, qlabel, glabel, gpos, tgt_off, T, bank=bank)
            if not bool(torch.isfinite(tgt_sim).all()):
                raise ValueError("retrieval_ranks: a relevant row has a non-finite score")
            # rank order inside every query: by score over the row-ascending lists, then by query, both stable
            qid = torch.repeat_interleave(torch.arange(M, device=self.device), tgt_off[1:] - tgt_off[:-1])
            by_score = torch.sort(tgt_sim, descending=True, stable=True).indices
            perm = by_score[torch.sort(qid[by_score], stable=True).indices]
            tgt_sim, tgt_row = tgt_sim[perm].contiguous(), tgt_row[perm].contiguous()
            hist = self.rank_count(rows, qlabel, glabel, tgt_off, tgt_sim, tgt_row, bank=bank)
            pos, ap, rr, hits, dcg, idcg = self.rank_metrics(tgt_off, hist, ks, bank=bank)
        return RetrievalRanks(ks, tgt_off, tgt_row, tgt_sim, pos, hist, ap, rr, hits, dcg, idcg)

    # ---- detection evaluation: ROC sweep under integer weightings -----------
    ROC_LDS_ROWS = 36864          # TVC_ROC_LDS_ROWS: up to this many samples a row's multiplicities live in LDS
    ROC_MAX_THR = 8               # TVC_ROC_MAX_THR
    ROC_MAX_N = 1 << 24           # TVC_ROC_MAX_N

    def roc_prepare(self, scores, labels, pos_label=1):
        """scores [N] (finite; taken as fp32), labels [N] -> (scores fp32 [N] sorted descending and stably, labels uint8 [N] =
        ``labels == pos_label`` in sorted order, order int32 [N]) on the engine's device: the three arrays every ``tvc_roc_*``
        call takes.  ``-0.0`` becomes ``0.0`` first (one tie group).  ``ValueError`` for N < 1, N > ``ROC_MAX_N``, a length
        mismatch or a non-finite score (as sklearn raises), before anything is sorted."""
        s = torch.as_tensor(scores).reshape(-1)
        lab = torch.as_tensor(labels).reshape(-1)
        N = s.numel()
        if N < 1 or N > self.ROC_MAX_N:
            raise ValueError(f"need 1 <= N <= {self.ROC_MAX_N} scores (got {N})")
        if lab.numel() != N:
            raise ValueError(f"need {N} labels (got {lab.numel()})")
        with torch.cuda.device(self.device):
            s = s.to(self.device, torch.float32)
            if not bool(torch.isfinite(s).all()):
                raise ValueError("scores must be finite (NaN or infinity found)")
            s = s + 0.0
            lab = (lab.to(self.device) == pos_label).to(torch.uint8)
            ss, order = torch.sort(s, descending=True, stable=True)
            return ss.contiguous(), lab[order].contiguous(), order.to(torch.int32).contiguous()

    def _roc_rows(self, prepared, n_resamples, weights, indices, seed, first):
        """-> (``_lib.RocRows``, B, what must stay alive): the source of a call's rows.  ``weights`` / ``indices`` int [B, N] over
        the original indices; neither and ``n_resamples`` > 0: Philox draws; neither and 0: one row of ones."""
        ss, sl, order = prepared
        N = ss.numel()
        if weights is not None and indices is not None:
            raise ValueError("give weights or indices, not both")
        src, source, B = None, _lib.TVC_ROC_SRC_WEIGHTS, 1
        if weights is not None or indices is not None:
            src = torch.as_tensor(weights if weights is not None else indices).to(self.device, torch.int32)
            src = (src.reshape(1, -1) if src.dim() == 1 else src).contiguous()
            if src.dim() != 2 or src.shape[1] != N or src.shape[0] < 1:
                raise ValueError(f"weights / indices must be [B >= 1, {N}] (got {tuple(src.shape)})")
            B = src.shape[0]
            if indices is not None:
                source = _lib.TVC_ROC_SRC_INDICES
            elif int(src.to(torch.int64).clamp(min=0).sum(1).max()) >= 1 << 31:
                raise ValueError("the total weight of a row must be < 2^31")
        elif n_resamples > 0:
            source, B = _lib.TVC_ROC_SRC_PHILOX, int(n_resamples)
        rows = _lib.RocRows(ss.data_ptr(), sl.data_ptr(), order.data_ptr(), N, source, 0 if src is None else src.data_ptr(), B,
                            int(first), int(seed) & 0xFFFFFFFFFFFFFFFF)
        return rows, B, (ss, sl, order, src)

    def roc_weights(self, scores, labels, *, n_resamples: int = 0, weights=None, indices=None, seed: int = 0, first: int = 0,
                    pos_label=1) -> torch.Tensor:
        """``tvc_roc_weights``: int32 [B, N], the multiplicities of every row of the source over the SORTED positions (column
        ``pos`` weighs the sample ``order[pos]`` of ``roc_prepare``)."""
        prepared = self.roc_prepare(scores, labels, pos_label)
        with self._lock, torch.cuda.device(self.device):
            rows, B, keep = self._roc_rows(prepared, n_resamples, weights, indices, seed, first)
            w = torch.empty((B, rows.N), dtype=torch.int32, device=self.device)
            self._check(self.lib.tvc_roc_weights(self.handle, C.byref(rows), _ptr(w), _stream()))
        return w

    def roc_sweep(self, scores, labels, *, n_resamples: int = 0, weights=None, indices=None, seed: int = 0,
                  target_tpr: float = 0.95, thresholds=(), pos_label=1, first: int = 0) -> RocSweep:
        """The ROC sweep of the full sample (row 0) and of B further rows: ``weights`` / ``indices`` int [B, N] over the original
        indices, or ``n_resamples`` Philox resamples numbered ``first`` .. (``seed``).  ``ValueError``, before any launch, for
        non-finite scores, N over ``ROC_MAX_N``, a full sample of one class, more than ``ROC_MAX_THR`` thresholds, a NaN
        threshold or a target outside [0, 1]."""
        thr = tuple(float(t) for t in thresholds)
        if len(thr) > self.ROC_MAX_THR or any(t != t for t in thr):
            raise ValueError(f"need at most {self.ROC_MAX_THR} thresholds, none NaN (got {thr})")
        if not 0.0 <= float(target_tpr) <= 1.0:
            raise ValueError(f"target_tpr must lie in [0, 1] (got {target_tpr})")
        prepared = self.roc_prepare(scores, labels, pos_label)
        n_pos = int(prepared[1].sum())
        if n_pos == 0 or n_pos == prepared[1].numel():
            raise ValueError("only one class present in labels: the ROC sweep is not defined")
        extra = weights is not None or indices is not None or n_resamples > 0
        with self._lock, torch.cuda.device(self.device):
            rows, B, keep = self._roc_rows(prepared, n_resamples, weights, indices, seed, first)
            R = 1 + (B if extra else 0)
            n_thr = len(thr)
            dt = {"auc2": torch.int64, "auc": torch.float64, "ap": torch.float64, "youden_j": torch.float64}
            out = {n: torch.empty((R, n_thr) if n.startswith("thr_") else (R,), dtype=dt.get(n, torch.int32), device=self.device)
                   for n in _lib.ROC_OUT_FIELDS}
            tarr = (C.c_float * max(n_thr, 1))(*thr)
            full = _lib.RocRows(rows.scores, rows.labels, rows.order, rows.N, _lib.TVC_ROC_SRC_WEIGHTS, 0, 1, 0, 0)
            calls = [(full, 0)] + ([(rows, 1)] if extra else [])
            for r, at in calls:
                o = _lib.RocOut(*[out[n][at:].data_ptr() if out[n][at:].numel() else 0 for n in _lib.ROC_OUT_FIELDS])
                self._check(self.lib.tvc_roc_sweep(self.handle, C.byref(r), float(target_tpr), tarr, n_thr, C.byref(o), _stream()))
        return RocSweep(prepared[0], prepared[1], prepared[2], float(target_tpr), thr, **out)

    def roc_curve(self, scores, labels, *, weights=None, pos_label=1):
        """``tvc_roc_curve`` of one row (``weights`` int [N] over the original indices; None: the full sample) -> (tp, fp, pos,
        kept int32 [points], sorted scores fp32 [N], P, N): every tie group of weight > 0 with its cumulative counts, the sorted
        position of its end and sklearn's drop_intermediate verdict.  Synchronises (it reads the count).  ``ValueError`` when the
        row has no positive or no negative weight."""
        prepared = self.roc_prepare(scores, labels, pos_label)
        with self._lock, torch.cuda.device(self.device):
            rows, B, keep = self._roc_rows(prepared, 0, weights, None, 0, 0)
            if B != 1:
                raise ValueError("roc_curve takes one row of weights")
            N = rows.N
            pts = torch.empty((4, N), dtype=torch.int32, device=self.device)
            count = torch.zeros(2, dtype=torch.int32, device=self.device)
            self._check(self.lib.tvc_roc_curve(self.handle, C.byref(rows), _ptr(pts[0]), _ptr(pts[1]), _ptr(pts[2]), _ptr(pts[3]),
                                               _ptr(count), _stream()))
            n = int(count[0])
        if n == 0:
            raise ValueError("only one class present in labels: the ROC curve is not defined")
        tp, fp, pos, kept = (pts[i, :n] for i in range(4))
        return tp, fp, pos, kept, prepared[0], int(tp[-1]), int(fp[-1])

    # ---- radius graph of a bank slot, DBSCAN on a radius graph -------------
    DBSCAN_SWEEP_BATCH = 4

    @staticmethod
    def radius_words(R: int) -> int:
        """uint32 words per row of a radius graph over R rows: round_up(R, 64) / 32."""
        return (R + 63) // 64 * 2

    def radius_graph(self, eps: float, bank: str = DEFAULT_BANK):
        """-> (adj int32 [R, W], degree int32 [R]) over the rows of ``bank``: bit ``j & 31`` of ``adj[i, j // 32]`` is
        ``|x_i - x_j|^2 <= eps^2`` (the words are uint32 bit patterns held in int32, W = ``radius_words(R)``).  Symmetric bit
        for bit, zero padding bits, the diagonal set for every row of finite norm; ``degree`` is the popcount of the row,
        self included.  ``eps`` is taken as an fp32 value."""
        eps = float(eps)
        if not (eps > 0.0 and eps != float("inf")):
            raise ValueError(f"eps must be finite and positive (got {eps})")
        with self._lock, torch.cuda.device(self.device):
            b = self._select(bank)
            R = b["rows"]
            adj = torch.empty((R, self.radius_words(R)), dtype=torch.int32, device=self.device)
            degree = torch.empty(R, dtype=torch.int32, device=self.device)
            self._check(self.lib.tvc_radius_graph(self.handle, eps, _ptr(adj), _ptr(degree), _stream()))
        return adj, degree

    def dbscan_labels(self, adj: torch.Tensor, degree: torch.Tensor, min_samples: int):
        """adj int32 [R, radius_words(R)] (any symmetric bitmask graph, ``radius_graph``'s or the caller's), degree int32
        [R] -> (labels int32 [R], core bool [R], n_clusters int, sweeps int).  Core rows have ``degree >= min_samples``;
        clusters are the components of the core-core graph, numbered by their lowest core row; a border row takes the
        lowest id among its core neighbours; noise is -1.  The labels are exact and deterministic; ``sweeps`` (label
        propagation sweeps up to and including the first that lowered nothing) is not.  The loop is Python, as the k-means
        loop is: sweeps run in batches of ``DBSCAN_SWEEP_BATCH``, each sweep of a batch flags its own ``changed`` word and
        the words are read once per batch, so up to ``DBSCAN_SWEEP_BATCH - 1`` idle sweeps run after the confirming one.
        R sweeps always suffice: a graph still changing after them raises ``RuntimeError``."""
        adj = _require_cuda(adj, torch.int32, "adj")
        degree = _require_cuda(degree, torch.int32, "degree")
        if adj.dim() != 2 or adj.shape[0] < 1 or adj.shape[1] != self.radius_words(adj.shape[0]):
            raise ValueError(f"adj must be [R, round_up(R, 64) / 32] with R >= 1 (got {tuple(adj.shape)})")
        R = adj.shape[0]
        if degree.shape != (R,):
            raise ValueError(f"degree must be [{R}] (got {tuple(degree.shape)})")
        min_samples = int(min_samples)
        if min_samples < 1:
            raise ValueError(f"min_samples must be >= 1 (got {min_samples})")
        comp = torch.empty(R, dtype=torch.int32, device=self.device)
        changed = torch.zeros(self.DBSCAN_SWEEP_BATCH, dtype=torch.int32, device=self.device)    # one word per sweep of a batch
        labels = torch.empty(R, dtype=torch.int32, device=self.device)
        core = torch.empty(R, dtype=torch.uint8, device=self.device)
        n_clusters = torch.zeros(1, dtype=torch.int32, device=self.device)
        done = 0
        with self._lock, torch.cuda.device(self.device):
            while True:
                if done >= R:
                    raise RuntimeError(f"dbscan_labels: the labels still change after {done} sweeps over {R} rows")
                changed.zero_()
                n = min(self.DBSCAN_SWEEP_BATCH, R - done)
                for k in range(n):
                    self._check(self.lib.tvc_dbscan_sweep(self.handle, _ptr(adj), _ptr(degree), R, min_samples, _ptr(comp),
                                                          C.c_void_p(changed.data_ptr() + 4 * k), 1 if done + k == 0 else 0,
                                                          _stream()))
                flags = changed[:n].tolist()
                if 0 in flags:                    # the first sweep that lowered nothing: the sweeps after it were idle
                    sweeps = done + flags.index(0) + 1
                    break
                done += n
            self._check(self.lib.tvc_dbscan_finish(self.handle, _ptr(adj), _ptr(degree), R, min_samples, _ptr(comp), _ptr(labels),
                                                   _ptr(core), _ptr(n_clusters), _stream()))
        return labels, core.bool(), int(n_clusters.item()), sweeps

    def dbscan(self, eps: float = 0.5, min_samples: int = 5, bank: str = DEFAULT_BANK):
        """``DBSCAN(eps, min_samples).fit_predict`` over the rows of ``bank`` (src/ref_bank.py:302-315) -> (labels int32 [R],
        core bool [R], centres fp32 [C, D] | None, order int32 [R], offsets int32 [C + 1]): ``radius_graph``, ``dbscan_labels``
        and the mean of every cluster's rows, core and border, through ``kmeans_update`` (bit-reproducible).
        ``order[offsets[c]:offsets[c + 1]]`` are cluster c's rows in ascending order, the rest of ``order`` is -1.  Without
        a cluster the centres are ``None`` and nothing is launched for them.  More than 65 536 clusters are refused by
        ``tvc_kmeans_update``."""
        adj, degree = self.radius_graph(eps, bank=bank)
        labels, core, n_clusters, _ = self.dbscan_labels(adj, degree, min_samples)
        if n_clusters == 0:
            return (labels, core, None, torch.full_like(labels, -1), torch.zeros(1, dtype=torch.int32, device=self.device))
        zeros = torch.zeros((n_clusters, self._banks[bank]["dim"]), dtype=torch.float32, device=self.device)
        centres, _, offsets, order = self.kmeans_update(labels, zeros, bank=bank, want_lists=True)
        return labels, core, centres, order, offsets

    # ---- pair lists of a bitmask graph, cosine of listed pairs, similar pairs of a slot of unit rows ----
    SIMILAR_TAU = 1.1e-5       # DESIGN.md 4.13's tau_ij for rows of norm <= 1 + 2^-8: (8e-6 + 2^-19) (1 + 2^-8)^2 < 1.1e-5

    def graph_pairs(self, adj: torch.Tensor, groups: Optional[torch.Tensor] = None, max_pairs: int = 1 << 27):
        """adj int32 [R, radius_words(R)] (any bitmask graph, symmetric or not), groups int32 [R] | None -> (pairs int32
        [P, 2], offsets int64 [R + 1]): the set bits ``i < j < R`` of the upper triangle in lexicographic (i, j) order, the
        order of a double loop ``for i: for j > i``; row i's pairs are ``pairs[offsets[i]:offsets[i + 1]]``.  With ``groups``
        a pair also needs both groups ``>= 0`` and different.  One host read (the total) sits between the count and the
        fill; a total above ``max_pairs`` raises ``ValueError`` naming it -- the list is never truncated."""
        adj = _require_cuda(adj, torch.int32, "adj")
        if adj.dim() != 2 or adj.shape[0] < 1 or adj.shape[1] != self.radius_words(adj.shape[0]):
            raise ValueError(f"adj must be [R, round_up(R, 64) / 32] with R >= 1 (got {tuple(adj.shape)})")
        R = adj.shape[0]
        if groups is not None:
            groups = _require_cuda(groups, torch.int32, "groups")
            if groups.shape != (R,):
                raise ValueError(f"groups must be [{R}] (got {tuple(groups.shape)})")
        with self._lock, torch.cuda.device(self.device):
            offsets = torch.empty(R + 1, dtype=torch.int64, device=self.device)
            self._check(self.lib.tvc_graph_pair_count(self.handle, _ptr(adj), R, _ptr(groups), _ptr(offsets), _stream()))
            total = int(offsets[R].item())
            if total > int(max_pairs):
                raise ValueError(f"the graph holds {total} pairs, more than max_pairs = {int(max_pairs)}: raise the threshold "
                                 f"or max_pairs (the list is never truncated)")
            pairs = torch.empty((total, 2), dtype=torch.int32, device=self.device)
            self._check(self.lib.tvc_graph_pair_fill(self.handle, _ptr(adj), R, _ptr(groups), _ptr(offsets), _ptr(pairs), total,
                                                     _stream()))
        return pairs, offsets

    def pair_cosine(self, pairs: torch.Tensor, bank: str = DEFAULT_BANK) -> torch.Tensor:
        """pairs int32 [P, 2] -> fp32 [P]: the cosine of the stored rows of every pair of ``bank`` (a bf16 slot: the stored
        values; an fp32 slot: hi + lo), within ``cosine_bound(D)`` of fp64 on those rows, bit-identical between runs and for
        (i, j) and (j, i).  0 for an all-zero row, NaN for a NaN row and for an index outside [0, R)."""
        pairs = _require_cuda(pairs, torch.int32, "pairs")
        if pairs.dim() != 2 or pairs.shape[1] != 2:
            raise ValueError(f"pairs must be [P, 2] (got {tuple(pairs.shape)})")
        P = pairs.shape[0]
        with self._lock, torch.cuda.device(self.device):
            self._select(bank)
            sims = torch.empty(P, dtype=torch.float32, device=self.device)
            self._check(self.lib.tvc_pair_cosine(self.handle, _ptr(pairs), P, _ptr(sims), _stream()))
        return sims

    @staticmethod
    def cosine_bound(D: int) -> float:
        """B(D) = 2^-24 (2 D + 16): the bound on ``|pair_cosine - cos64(stored rows)|`` for any summation order of the D fp32
        FMA terms of the dot product and of the two norms, plus the sqrt, the multiply and the divide."""
        return 2.0 ** -24 * (2 * D + 16)

    @classmethod
    def similar_margin(cls, D: int, t: float, bf16: bool) -> float:
        """m: ``similar_pairs`` asks the radius graph for ``eps^2 = 2 - 2 t + m`` (the one place m is
        computed).  Stored rows of norm ``1 + d``, ``|d| <= nu``, with cosine ``c >= t - B(D)`` lie at
        ``|x - y|^2 = (|x| - |y|)^2 + 2 |x| |y| (1 - c) <= 4 nu^2 + 2 (1 + nu)^2 (1 - t + B)``; adding 4.13's tau for such rows
        and 2^-19 for the fp32 rounding of eps and of its square makes every such pair a DECIDED in-graph pair.
        nu = 2^-24 (D + 8) for the fp32 normalisation, plus 2^-16 for the hi | lo planes of an fp32 slot or 2^-9 for the
        rounding of the elements to a bf16 slot."""
        nu = 2.0 ** -24 * (D + 8) + (2.0 ** -9 if bf16 else 2.0 ** -16)
        eps2 = 4 * nu * nu + 2 * (1 + nu) ** 2 * (1 - t + cls.cosine_bound(D)) + cls.SIMILAR_TAU + 2.0 ** -19
        return eps2 - (2 - 2 * t)

    def similar_pairs(self, t: float, bank: str = DEFAULT_BANK, groups: Optional[torch.Tensor] = None, max_pairs: int = 1 << 27):
        """The pairs ``i < j`` of a slot of UNIT rows with cosine ``>= float32(t)`` -> (pairs int32 [P, 2], sims fp32 [P]) in
        lexicographic (i, j) order: ``radius_graph`` at the widened radius ``eps^2 = 2 - 2 t + similar_margin(D, t, bf16)``,
        ``graph_pairs`` (``groups``: only pairs of two different groups ``>= 0``), ``pair_cosine``, and the filter
        ``sims >= float32(t)`` -- the fp32-grade cosine decides a pair, the graph only nominates it: a pair differs from
        fp64 on the stored rows only inside ``|cos64 - t| <= cosine_bound(D)``.  ``t > 1`` gives empty lists without a
        launch; a non-finite ``t`` raises; more than ``max_pairs`` nominated pairs raise ``ValueError``."""
        import math
        t = float(t)
        if not math.isfinite(t):
            raise ValueError(f"t must be finite (got {t})")
        if t > 1.0:
            return (torch.empty((0, 2), dtype=torch.int32, device=self.device), torch.empty(0, dtype=torch.float32, device=self.device))
        b = self._slot(bank)
        eps2 = 2 - 2 * t + self.similar_margin(b["dim"], t, bool(b.get("bf16")))
        adj, _ = self.radius_graph(math.sqrt(eps2), bank=bank)
        pairs, _ = self.graph_pairs(adj, groups=groups, max_pairs=max_pairs)
        del adj
        sims = self.pair_cosine(pairs, bank=bank)
        keep = sims >= torch.tensor(t, dtype=torch.float32, device=self.device)
        return pairs[keep], sims[keep]

    # ---- closest pair of a bank slot ----------------------------------------
    CLOSEST_PAIR_TAU = 1e-6    # the contract's tau in cosine units: the bank search's bound

    def closest_pair(self, bank: str = DEFAULT_BANK):
        """-> (pair int32 [2], pair_sim fp32 [1], partner int32 [R], sim fp32 [R]) over the rows of ``bank``, all device
        tensors on the current stream; the call does no host synchronisation.  ``partner[i]`` is the arg-max over the LATER
        rows ``j > i`` of ``cos(x_i, x_j)`` (value descending, ``j`` ascending), ``sim[i]`` that cosine; ``pair`` is
        ``(i, partner[i])`` of the best row under (sim descending, ``i`` ascending) -- the first maximal pair in lexicographic
        ``(i, j)`` order, the pair a strict ``>`` over a double loop ``for i: for j > i`` keeps -- and ``pair_sim`` its cosine.
        A row with no admissible later row (the last row, a row whose norm is not finite, a row all of whose later rows have
        a non-finite norm) has ``partner = -1, sim = -inf``; without any pair ``pair = (-1, -1), pair_sim = -inf`` (R = 1 is
        valid).  An all-zero row has cosine 0 with every row; a row of non-finite norm is never a partner.

        Contract.  With ``c64(i, j)`` the fp64 cosine of the STORED rows (a bf16 slot: the bf16 values; an fp32 slot: hi + lo)
        and ``tau = CLOSEST_PAIR_TAU = 1e-6``: ``|sim[i] - c64(i, partner[i])| <= tau`` and ``c64(i, partner[i]) >=
        max_{j > i} c64(i, j) - 2 tau``; both hold for ``pair`` / ``pair_sim`` over all ``i < j``.  Where the arithmetic is
        exact -- rows of one common norm whose ``1 / norm`` is a power of two and whose dot products are small integers --
        ``partner`` and ``pair`` are exactly the above, including every tie.  The outputs are a pure function of the slot,
        bit-identical between runs (no atomics, no floating-point reduction across workgroups)."""
        with self._lock, torch.cuda.device(self.device):
            b = self._select(bank)
            R = b["rows"]
            partner = torch.empty(R, dtype=torch.int32, device=self.device)
            sim = torch.empty(R, dtype=torch.float32, device=self.device)
            pair = torch.empty(2, dtype=torch.int32, device=self.device)
            pair_sim = torch.empty(1, dtype=torch.float32, device=self.device)
            self._check(self.lib.tvc_closest_pair(self.handle, _ptr(partner), _ptr(sim), _ptr(pair), _ptr(pair_sim), _stream()))
        return pair, pair_sim, partner, sim

    # ---- similarity metrics of row pairs; top-k overlap ----------------------
    SIM_MAX_D = 4096              # TVC_SIM_MAX_D: the row form's widest row
    SIM_MAX_N = 1 << 20           # TVC_SIM_MAX_N: the long form's cap
    TOPK_OVERLAP_MAX_K = 1024     # TVC_TOPK_OVERLAP_MAX_K

    def _sim_operand(self, t, dtype, name: str) -> torch.Tensor:
        """[B, D] on the device with unit column stride (a column view of a wider buffer keeps its row pitch); 1-D = one row"""
        t = torch.as_tensor(t)
        if dtype == torch.int32 and t.dtype != torch.int32:
            if t.is_floating_point() or t.dtype == torch.bool:
                raise ValueError(f"{name}: key='i32' takes integer elements (got {t.dtype})")
            if t.numel() and (int(t.min()) < -(1 << 31) or int(t.max()) >= 1 << 31):
                raise ValueError(f"{name}: an element does not fit int32")
        t = t.to(self.device, dtype)
        if t.dim() == 1:
            t = t.reshape(1, -1)
        if t.dim() != 2:
            raise ValueError(f"{name} must be [B, D] or [D] (got shape {tuple(t.shape)})")
        if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            t = t.contiguous()
        return t

    def similarity_rows(self, x, y, key: str = "f32") -> SimilarityRows:
        """x, y [B, D] (or [D]: one pair), 1 <= D <= ``SIM_MAX_D`` -> ``SimilarityRows`` of the B pairs (x[b], y[b]) from one launch
        of ``tvc_sim_rows``: device tensors on the current stream, no host synchronisation.  ``key="f32"``: the elements are
        taken as fp32 (values that fp32 cannot hold are rounded first, which can create ties); ``key="i32"``: integer index
        lists, taken exactly.  Formulas, specials and error bounds: include/tvc.h.  B == 0 is valid."""
        if key not in ("f32", "i32"):
            raise ValueError(f"key must be 'f32' or 'i32' (got {key!r})")
        dt = torch.int32 if key == "i32" else torch.float32
        with self._lock, torch.cuda.device(self.device):
            xd, yd = self._sim_operand(x, dt, "x"), self._sim_operand(y, dt, "y")
            if xd.shape != yd.shape:
                raise ValueError(f"x and y must have one shape (got {tuple(xd.shape)}, {tuple(yd.shape)})")
            B, D = xd.shape
            if D < 1 or D > self.SIM_MAX_D:
                raise ValueError(f"need 1 <= D <= {self.SIM_MAX_D} (got {D}); similarity_flat takes one longer pair")
            out = torch.empty((B, 8), dtype=torch.float64, device=self.device)
            ints = torch.empty((B, 4), dtype=torch.int64, device=self.device)
            self._check(self.lib.tvc_sim_rows(self.handle, _ptr(xd), _ptr(yd), B, D, xd.stride(0) if B > 1 else D,
                                              yd.stride(0) if B > 1 else D, _lib.TVC_SIM_KEY_I32 if key == "i32" else _lib.TVC_SIM_KEY_F32,
                                              _ptr(out), _ptr(ints), _stream()))
        return SimilarityRows(out[:, :5], ints)

    def similarity_flat(self, x, y, force_long: bool = False) -> SimilarityRows:
        """The ``SimilarityRows`` (one row) of ONE pair: x and y of any shape with equally many elements n, flattened and taken
        as fp32.  n <= ``SIM_MAX_D`` runs the row form; a longer pair (or ``force_long``) the long form: ``torch.sort`` of the
        values (plumbing: the kernels need only the sorted values), ``tvc_sim_flat_rank`` twice and ``tvc_sim_flat``.
        ``ValueError`` for n < 1 or n > ``SIM_MAX_N``."""
        with torch.cuda.device(self.device):
            xd = torch.as_tensor(x).to(self.device, torch.float32).reshape(-1).contiguous()
            yd = torch.as_tensor(y).to(self.device, torch.float32).reshape(-1).contiguous()
        n = xd.numel()
        if yd.numel() != n:
            raise ValueError(f"x and y must have equally many elements (got {n}, {yd.numel()})")
        if n < 1 or n > self.SIM_MAX_N:
            raise ValueError(f"need 1 <= n <= {self.SIM_MAX_N} elements (got {n})")
        if n <= self.SIM_MAX_D and not force_long:
            return self.similarity_rows(xd, yd)
        with self._lock, torch.cuda.device(self.device):
            out = torch.empty((1, 8), dtype=torch.float64, device=self.device)
            ints = torch.empty((1, 4), dtype=torch.int64, device=self.device)
            ws = torch.empty(int(self.lib.tvc_sim_flat_workspace(n)) // 8, dtype=torch.int64, device=self.device)
            cranks = []
            for v in (xd, yd):
                sv = torch.sort(v).values                  # ascending, NaN last
                c = torch.empty(n, dtype=torch.int32, device=self.device)
                self._check(self.lib.tvc_sim_flat_rank(self.handle, _ptr(v), _ptr(sv), n, _ptr(c), None, _stream()))
                cranks.append(c)
            self._check(self.lib.tvc_sim_flat(self.handle, _ptr(xd), _ptr(yd), _ptr(cranks[0]), _ptr(cranks[1]), n, _ptr(out),
                                              _ptr(ints), _ptr(ws), ws.numel() * 8, _stream()))
        return SimilarityRows(out[:, :5], ints)

    def topk_overlap(self, a, b, k: int) -> torch.Tensor:
        """a int [M, La], b int [M, Lb] (or 1-D: one query) -> int32 [M] on the device: ``len(set(a[i, :k]) & set(b[i, :k]))``,
        one wave per query (``tvc_topk_overlap``); 1 <= k <= ``TOPK_OVERLAP_MAX_K``.  Ids must fit int32; none is special."""
        k = int(k)
        if k < 1 or k > self.TOPK_OVERLAP_MAX_K:
            raise ValueError(f"need 1 <= k <= {self.TOPK_OVERLAP_MAX_K} (got {k})")
        with self._lock, torch.cuda.device(self.device):
            ad, bd = self._sim_operand(a, torch.int32, "a").contiguous(), self._sim_operand(b, torch.int32, "b").contiguous()
            if ad.shape[0] != bd.shape[0]:
                raise ValueError(f"a and b must have equally many rows (got {ad.shape[0]}, {bd.shape[0]})")
            M = ad.shape[0]
            if ad.shape[1] == 0 or bd.shape[1] == 0:          # an empty list shares nothing (and has no buffer to pass)
                return torch.zeros(M, dtype=torch.int32, device=self.device)
            count = torch.empty(M, dtype=torch.int32, device=self.device)
            self._check(self.lib.tvc_topk_overlap(self.handle, _ptr(ad), _ptr(bd), M, ad.shape[1], bd.shape[1], k, _ptr(count), _stream()))
        return count

    # ---- IVF search over a bank slot in list order -------------------------
    def ivf_probe(self, rows: torch.Tensor, centroids: torch.Tensor, nprobe: int):
        """rows fp32 [M, D], centroids fp32 [nlist, D] -> (lists int32 [M, nprobe], score fp32 [M, nprobe]): the nprobe
        lists with the largest q.c - |c|^2 / 2, best first, ties to the lower list id (``kmeans_assign``'s rule).  Ranks
        beyond nlist, or that only NaN scores could fill, are -1 / -inf."""
        if not 1 <= nprobe <= _lib.TVC_MAX_TOPK:
            raise ValueError(f"nprobe must be in [1, {_lib.TVC_MAX_TOPK}] (got {nprobe})")
        rows = _require_cuda(rows, torch.float32, "rows")
        centroids = _require_cuda(centroids, torch.float32, "centroids")
        if rows.dim() != 2 or centroids.dim() != 2 or rows.shape[1] != centroids.shape[1]:
            raise ValueError(f"rows [M, D] and centroids [nlist, D] must share D (got {tuple(rows.shape)}, {tuple(centroids.shape)})")
        M, D = rows.shape
        lists = torch.empty((M, nprobe), dtype=torch.int32, device=self.device)
        score = torch.empty((M, nprobe), dtype=torch.float32, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_ivf_probe(self.handle, _ptr(rows), M, D, _ptr(centroids), centroids.shape[0], nprobe,
                                               _ptr(lists), _ptr(score), _stream()))
        return lists, score

    def ivf_scan(self, rows: torch.Tensor, k: int, probes: torch.Tensor, index: "IVFIndex", idx_offset: int = 0):
        """rows fp32 [M, D], probes int32 [M, nprobe] (-1 = skip) -> (idx int32 [M, k], sim fp32 [M, k], pos int32 [M, k]):
        the exact top-k of every query over the rows of its probed lists, in ``bank_search``'s contract (idx = the original
        row index + idx_offset, (sim desc, idx asc), -1 / -inf padded); ``pos`` is the stored position, what
        ``bank_gather(pos, bank=index.name)`` takes.  A probed list longer than ``index.max_list_rows`` shows in
        ``bank_status()`` as TVC_E_OVERFLOW."""
        if not 1 <= k <= _lib.TVC_MAX_TOPK:
            raise ValueError(f"top-k must be in [1, {_lib.TVC_MAX_TOPK}] (got {k}): tvc_ivf_scan never truncates silently")
        rows = _require_cuda(rows, torch.float32, "rows")
        probes = _require_cuda(probes, torch.int32, "probes")
        M = rows.shape[0]
        if probes.dim() != 2 or probes.shape[0] != M:
            raise ValueError(f"probes must be [{M}, nprobe] (got {tuple(probes.shape)})")
        idx = torch.empty((M, k), dtype=torch.int32, device=self.device)
        sim = torch.empty((M, k), dtype=torch.float32, device=self.device)
        pos = torch.empty((M, k), dtype=torch.int32, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            b = self._select(index.name)
            if rows.dim() != 2 or rows.shape[1] != b["dim"]:
                raise ValueError(f"rows must be [M, {b['dim']}] (got {tuple(rows.shape)})")
            self._check(self.lib.tvc_ivf_scan(self.handle, _ptr(rows), M, k, _ptr(probes), probes.shape[1], _ptr(index.offsets),
                                              index.nlist, index.max_list_rows, _ptr(index.ids), idx_offset, _ptr(idx), _ptr(sim),
                                              _ptr(pos), _stream()))
        return idx, sim, pos

    def ivf_search(self, rows: torch.Tensor, k: int, nprobe: int, index: "IVFIndex", idx_offset: int = 0):
        """``ivf_probe`` (nprobe clamped to nlist, as faiss does) + ``ivf_scan`` -> (idx, sim, pos); no host synchronisation."""
        lists, _ = self.ivf_probe(rows, index.centroids, max(1, min(int(nprobe), index.nlist)))
        return self.ivf_scan(rows, k, lists, index, idx_offset)

    def ivf_build(self, bank: torch.Tensor, nlist: int, name: str, train_rows: Optional[int] = None, max_iter: int = 10,
                  seed: int = 1234) -> "IVFIndex":
        """Train ``nlist`` centroids on ``bank`` [R, D] (bf16 or fp32), store the rows in list order under the bank slot
        ``name`` (which the index then owns) and return the ``IVFIndex``.

        faiss's level-1 training (``IndexIVFFlat.train`` -> ``Clustering``: niter = 10, seed 1234, at most 256 points
        per centroid, random distinct rows as the start) as far as ``TVCEngine.kmeans`` allows: k-means with
        ``init="random"``, ``n_init=1``, ``max_iter`` iterations on at most ``train_rows`` (default 256 * nlist) rows.
        Where it differs: the subsample and the start are drawn with the seeded numpy generator
        (``default_rng(seed)``), not faiss's own; the loop may stop early by sklearn's rule; an empty cluster takes the
        farthest row instead of splitting a big cluster.  One assign + update over ALL rows then gives the lists.  Two
        builds with the same arguments are bit-identical."""
        import numpy as np
        if bank.dim() != 2:
            raise ValueError("bank must be [R, D]")
        if bank.dtype not in (torch.bfloat16, torch.float32):
            bank = bank.float()
        bank = _require_cuda(bank, bank.dtype, "bank")
        R = bank.shape[0]
        if not 1 <= nlist <= min(R, 65536):
            raise ValueError(f"need 1 <= nlist <= min(R, 65536) (got nlist = {nlist}, R = {R})")
        n_train = min(R, int(train_rows) if train_rows else 256 * nlist)
        if n_train < nlist:
            raise ValueError(f"train_rows = {n_train} is fewer than nlist = {nlist}")
        tmp = name + ":ivf-train"
        try:
            if n_train < R:
                sel = np.sort(np.random.default_rng(seed).choice(R, n_train, replace=False))
                self.set_bank(bank[torch.from_numpy(sel).to(self.device)], name=tmp)
            else:
                self.set_bank(bank, name=tmp)
            centroids = self.kmeans(nlist, bank=tmp, init="random", n_init=1, max_iter=max_iter, seed=seed)[0]
        finally:
            self.release_bank(tmp)
        try:
            self.set_bank(bank, name=name)
            labels, _, _ = self.kmeans_assign(centroids, bank=name)
            _, counts, offsets, order = self.kmeans_update(labels, centroids, bank=name, want_lists=True)
            n_in = int(offsets[-1].item())             # rows whose scores are all NaN are in no list
            ids = order[:n_in].contiguous()
            self.set_bank(bank[ids.long()], name=name)
        except Exception:
            self.release_bank(name)
            raise
        return IVFIndex(name=name, nlist=nlist, centroids=centroids.contiguous(), offsets=offsets, ids=ids,
                        max_list_rows=max(1, int(counts.max().item())), rows=n_in, dim=bank.shape[1])

    def ivf_release(self, index: "IVFIndex") -> None:
        """Free the bank slot the index owns."""
        self.release_bank(index.name)

    def topk_merge(self, idx_parts, sim_parts, feat_parts=None, mom_parts=None):
        """parts [W, M, k] (+ feat [W, M, kf, D], mom [W, M, 4]) -> merged (idx, sim, feat, mom)."""
        idx_parts = _require_cuda(idx_parts, torch.int32, "idx_parts")
        sim_parts = _require_cuda(sim_parts, torch.float32, "sim_parts")
        W, M, k = idx_parts.shape
        kf, D = (feat_parts.shape[2], feat_parts.shape[3]) if feat_parts is not None else (0, 0)
        idx = torch.empty((M, k), dtype=torch.int32, device=self.device)
        sim = torch.empty((M, k), dtype=torch.float32, device=self.device)
        feat = torch.empty((M, kf, D), dtype=torch.float32, device=self.device) if feat_parts is not None else None
        mom = torch.empty((M, 4), dtype=torch.float32, device=self.device) if mom_parts is not None else None
        if feat_parts is not None:
            feat_parts = _require_cuda(feat_parts, torch.float32, "feat_parts")
        if mom_parts is not None:
            mom_parts = _require_cuda(mom_parts, torch.float32, "mom_parts")
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_topk_merge(self.handle, _ptr(idx_parts), _ptr(sim_parts), _ptr(feat_parts),
                                                _ptr(mom_parts), W, M, k, kf, D, _ptr(idx), _ptr(sim), _ptr(feat),
                                                _ptr(mom), _stream()))
        return idx, sim, feat, mom

    # ---- consistency ---------------------------------------------------
    def consistency(self, img: torch.Tensor, txt: torch.Tensor, cfg: ConsistencyConfig,
                    ref_idx: Optional[torch.Tensor] = None, ref_sim: Optional[torch.Tensor] = None,
                    ref_feat: Optional[torch.Tensor] = None) -> torch.Tensor:
        """img [B, D], txt [B, N+1, D]; optional refs for the text rows:
        ref_idx / ref_sim [B*(N+1), ks], ref_feat [B*(N+1), kf, D].  Returns the
        record tensor fp32 [B, rec_stride(N)] (layout: include/tvc.h)."""
        img = _require_cuda(img, torch.float32, "img")
        txt = _require_cuda(txt, torch.float32, "txt")
        B, N1, D = txt.shape
        N = N1 - 1
        ks = kf = 0
        if ref_idx is not None:
            ref_idx = _require_cuda(ref_idx, torch.int32, "ref_idx")
            ref_sim = _require_cuda(ref_sim, torch.float32, "ref_sim")
            ref_feat = _require_cuda(ref_feat, torch.float32, "ref_feat")
            ks, kf = ref_idx.shape[-1], ref_feat.shape[-2]
        rec = torch.empty((B, _lib.rec_stride(N)), dtype=torch.float32, device=self.device)
        p = cfg.to_c()
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_consistency(self.handle, _ptr(img), _ptr(txt), B, N, D, _ptr(ref_idx),
                                                 _ptr(ref_sim), _ptr(ref_feat), ks, kf, C.byref(p), _ptr(rec), _stream()))
        return rec

    def detect_embeddings(self, img: torch.Tensor, txt: torch.Tensor, cfg: ConsistencyConfig,
                          use_bank: bool = True, robust: bool = False, bank: str = DEFAULT_BANK,
                          ivf: Optional["IVFIndex"] = None, nprobe: int = 1) -> torch.Tensor:
        """Bank search of the text rows -> gather -> consistency; all on the current stream.
        ``robust=False``: no host synchronisation, the caller checks ``bank_status()`` later;
        ``robust=True``: synchronises once and falls back to the brute-force search on overflow.
        ``ivf``: search the ``nprobe`` nearest lists of that index instead of the whole bank (``ivf_search``; the rows
        are gathered from the index's slot by stored position); ``bank`` / ``robust`` are then not used."""
        B, N1, D = txt.shape
        if use_bank and ivf is not None and ivf.rows > 0:
            k = max(cfg.search_k, cfg.reference_count)
            idx, sim, pos = self.ivf_search(txt.reshape(B * N1, D), k, nprobe, ivf)
            feat = self.bank_gather(pos[:, :cfg.reference_count].contiguous(), bank=ivf.name)
            return self.consistency(img, txt, cfg, idx, sim, feat)
        if use_bank and self.bank_size(bank) > 0:
            k = max(cfg.search_k, cfg.reference_count)
            search = self.bank_search_robust if robust else self.bank_search
            idx, sim, _ = search(txt.reshape(B * N1, D), k, cfg.similarity_threshold, want_moments=False, bank=bank)
            kf = cfg.reference_count
            feat = self.bank_gather(idx[:, :kf].contiguous(), bank=bank)
            return self.consistency(img, txt, cfg, idx, sim, feat)
        return self.consistency(img, txt, cfg)

    # ---- building blocks (parity tests / profiling) ----------------------
    def _gemm16(self, dt: torch.dtype, fn, a, b, bias, epilogue, out, k) -> torch.Tensor:
        a = _require_cuda(a, dt, "a")
        b = _require_cuda(b, dt, "b")
        I, lda = a.shape
        J, ldb = b.shape
        K = k if k is not None else lda
        if k is None and lda != ldb:
            raise ValueError("a and b must have the same number of columns (or pass k)")
        odt = torch.float32 if epilogue in (0, 3) else dt
        if out is None:
            out = torch.empty((J, I), dtype=odt, device=self.device)
            if epilogue == 3:
                out.zero_()
        ld_out = _check_out(out, J, I, odt)
        if bias is not None:
            bias = _require_cuda(bias, torch.float32, "bias")
        with self._lock, torch.cuda.device(self.device):
            self._check(fn(self.handle, _ptr(a), _ptr(b), _ptr(bias), _ptr(out), I, J, K, lda, ldb, ld_out, epilogue, _stream()))
        return out

    def gemm(self, a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = 0,
             out: Optional[torch.Tensor] = None, k: Optional[int] = None) -> torch.Tensor:
        """out[j, i] = sum_k a[i, k] b[j, k] (+ bias[i]); a, b bf16.  ``k``: multiply only the first k columns
        (the operands' row strides stay their full widths: padded leading dimensions)."""
        return self._gemm16(torch.bfloat16, self.lib.tvc_gemm_bf16, a, b, bias, epilogue, out, k)

    def gemm_f16(self, a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = 0,
                 out: Optional[torch.Tensor] = None, k: Optional[int] = None) -> torch.Tensor:
        """fp16 twin of :meth:`gemm` (tower mode 3): a, b fp16 on the f16 MFMA; epilogues 1 / 2 store fp16."""
        return self._gemm16(torch.float16, self.lib.tvc_gemm_f16, a, b, bias, epilogue, out, k)

    def _attention16(self, dt: torch.dtype, fn, qkv, n_seq, seq_len, heads, causal, *starts) -> torch.Tensor:
        # starts: given (a tensor or None) only for an entry point that takes the argument
        qkv = _require_cuda(qkv, dt, "qkv")
        out = torch.empty((qkv.shape[0], heads * 64), dtype=dt, device=self.device)
        starts = [s if s is None else _require_cuda(s, torch.int32, "starts") for s in starts]
        with self._lock, torch.cuda.device(self.device):
            self._check(fn(self.handle, _ptr(qkv), _ptr(out), *map(_ptr, starts), n_seq, seq_len, heads, int(causal), _stream()))
        return out

    def attention(self, qkv: torch.Tensor, n_seq: int, seq_len: int, heads: int, causal: bool) -> torch.Tensor:
        return self._attention16(torch.bfloat16, self.lib.tvc_attention, qkv, n_seq, seq_len, heads, causal)

    def attention_f16(self, qkv: torch.Tensor, n_seq: int, seq_len: int, heads: int, causal: bool,
                      starts: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp16 twin of :meth:`attention`; ``starts`` (int32 [n_seq + 1]): packed sequences of at most seq_len rows."""
        return self._attention16(torch.float16, self.lib.tvc_attention_f16, qkv, n_seq, seq_len, heads, causal, starts)

    def attention_ex(self, qkv: torch.Tensor, n_seq: int, seq_len: int, heads: int, causal: bool,
                     starts: Optional[torch.Tensor] = None, pfx: Optional[torch.Tensor] = None, pool_mode: int = 0,
                     pool_row: Optional[torch.Tensor] = None, f16: bool = False,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The tower attention kernel with every launch option (``tvc_attention_ex``, include/tvc.h): qkv bf16 (fp16 with
        ``f16``); ``starts`` int32 [n_seq + 1], ``pfx`` int32 [2 * n_seq], ``pool_row`` int32 [n_seq].  Returns
        [rows, width], or the compact [n_seq, width] when ``pool_mode`` is 1 / 2; ``out`` (optional) is written in place."""
        dt = torch.float16 if f16 else torch.bfloat16
        qkv = _require_cuda(qkv, dt, "qkv")
        shape = (n_seq if pool_mode else qkv.shape[0], heads * 64)
        if out is None:
            out = torch.empty(shape, dtype=dt, device=self.device)
        elif not out.is_cuda or out.dtype != dt or out.shape != shape or not out.is_contiguous():
            raise ValueError(f"attention_ex: out must be a contiguous {dt} tensor of shape {shape} on the GPU")
        starts, pfx, pool_row = (t if t is None else _require_cuda(t, torch.int32, name)
                                 for t, name in ((starts, "starts"), (pfx, "pfx"), (pool_row, "pool_row")))
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_attention_ex(self.handle, _ptr(qkv), _ptr(out), _ptr(starts), _ptr(pfx), n_seq, seq_len,
                                                  heads, int(causal), pool_mode, _ptr(pool_row), int(f16), _stream()))
        return out

    def attention_backward(self, qkv: torch.Tensor, dout: torch.Tensor, n_seq: int, seq_len: int, heads: int,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dQ | dK | dV bf16 [rows, 3 * width] of the dense non-causal tower attention (``tvc_attention_backward``); ``out``
        (optional) is written in place: a buffer with more rows is handed in as its first ``rows`` rows."""
        qkv = _require_cuda(qkv, torch.bfloat16, "qkv")
        dout = _require_cuda(dout, torch.bfloat16, "dout")
        if qkv.shape != (n_seq * seq_len, 3 * heads * 64) or dout.shape != (n_seq * seq_len, heads * 64):
            raise ValueError("attention_backward: qkv [rows, 3*heads*64] and dout [rows, heads*64] expected")
        if out is None:
            dqkv = torch.empty_like(qkv)
        elif not out.is_cuda or out.dtype != torch.bfloat16 or out.shape != qkv.shape or not out.is_contiguous():
            raise ValueError(f"attention_backward: out must be a contiguous {torch.bfloat16} tensor of shape "
                             f"{tuple(qkv.shape)} on the GPU")
        else:
            dqkv = out
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_attention_backward(self.handle, _ptr(qkv), _ptr(dout), _ptr(dqkv), n_seq, seq_len,
                                                        heads, _stream()))
        return dqkv

    def attention_split_backward(self, qkv: torch.Tensor, dout: torch.Tensor, n_seq: int, seq_len: int, heads: int) -> torch.Tensor:
        """dQ | dK | dV fp32 [rows, 3 * width] of the dense non-causal tower attention on fp32 operands, every product on
        hi | lo planes (``tvc_attention_split_backward``: the split-bf16 input gradient's attention backward)."""
        qkv = _require_cuda(qkv, torch.float32, "qkv")
        dout = _require_cuda(dout, torch.float32, "dout")
        if qkv.shape != (n_seq * seq_len, 3 * heads * 64) or dout.shape != (n_seq * seq_len, heads * 64):
            raise ValueError("attention_split_backward: qkv [rows, 3*heads*64] and dout [rows, heads*64] expected")
        dqkv = torch.empty_like(qkv)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_attention_split_backward(self.handle, _ptr(qkv), _ptr(dout), _ptr(dqkv), n_seq, seq_len,
                                                              heads, _stream()))
        return dqkv

    def layernorm_backward(self, x: torch.Tensor, dy: torch.Tensor, g: torch.Tensor,
                           dres: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _require_cuda(x, torch.float32, "x")
        dy = _require_cuda(dy, torch.bfloat16, "dy")
        g = _require_cuda(g, torch.float32, "g")
        if dres is not None:
            dres = _require_cuda(dres, torch.float32, "dres")
        dx = torch.empty_like(x)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_layernorm_backward(self.handle, _ptr(x), _ptr(dy), _ptr(g), _ptr(dres), _ptr(dx),
                                                        x.shape[0], x.shape[1], _stream()))
        return dx

    def preprocess_images(self, images: torch.Tensor, size: int, mean, std, bicubic: bool = True,
                          keep_aspect: bool = True) -> torch.Tensor:
        """images fp32 [n, 3, H, W] in [0, 1] (on the GPU) -> fp32 [n, 3, size, size]: antialiased resize (+ centre crop)
        and (x - mean) / std in one kernel (``tvc_preprocess_images``)."""
        images = _require_cuda(images, torch.float32, "images")
        n, _, H, W = images.shape
        out = torch.empty((n, 3, size, size), dtype=torch.float32, device=self.device)
        m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_preprocess_images(self.handle, _ptr(images), n, H, W, size, int(bicubic), int(keep_aspect),
                                                       m3, s3, _ptr(out), _stream()))
        return out

    def gemm_f32(self, w: torch.Tensor, x: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = 0,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """out[j, i] (op)= sum_k x[j, k] w[i, k] + bias[i] on the exact-f32 matrix instruction (fp32-grade mode)."""
        w = _require_cuda(w, torch.float32, "w")
        x = _require_cuda(x, torch.float32, "x")
        if w.shape[1] != x.shape[1]:
            raise ValueError("w [I, K] and x [J, K] expected")
        if out is None:
            out = torch.zeros((x.shape[0], w.shape[0]), dtype=torch.float32, device=self.device)
        ld_out = _check_out(out, x.shape[0], w.shape[0], torch.float32)
        if bias is not None:
            bias = _require_cuda(bias, torch.float32, "bias")
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_gemm_f32(self.handle, _ptr(w), _ptr(x), _ptr(bias), _ptr(out), w.shape[0], x.shape[0],
                                              w.shape[1], ld_out, epilogue, _stream()))
        return out

    def attention_f32(self, qkv: torch.Tensor, n_seq: int, seq_len: int, heads: int, causal: bool) -> torch.Tensor:
        qkv = _require_cuda(qkv, torch.float32, "qkv")
        out = torch.empty((qkv.shape[0], heads * 64), dtype=torch.float32, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_attention_f32(self.handle, _ptr(qkv), _ptr(out), n_seq, seq_len, heads, int(causal),
                                                   _stream()))
        return out

    def gemm_split(self, w: torch.Tensor, x: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
        """out [J, I] = x [J, K] w [I, K]^T + bias on hi | lo bf16 planes, three MFMA products per element (split-bf16 mode)."""
        w = _require_cuda(w, torch.float32, "w")
        x = _require_cuda(x, torch.float32, "x")
        if w.shape[1] != x.shape[1]:
            raise ValueError("w [I, K] and x [J, K] expected")
        ld = (w.shape[0] + 3) // 4 * 4
        out = torch.zeros((x.shape[0], ld), dtype=torch.float32, device=self.device)
        if bias is not None:
            bias = _require_cuda(bias, torch.float32, "bias")
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_gemm_split(self.handle, _ptr(w), _ptr(x), _ptr(bias), _ptr(out), w.shape[0], x.shape[0],
                                                w.shape[1], ld, _stream()))
        return out[:, :w.shape[0]]

    def attention_split(self, qkv: torch.Tensor, n_seq: int, seq_len: int, heads: int, causal: bool,
                        starts: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 qkv rows -> fp32 attention output (hi + lo of the planes the split-bf16 tower's out-projection reads)."""
        qkv = _require_cuda(qkv, torch.float32, "qkv")
        w = heads * 64
        planes = torch.zeros((qkv.shape[0], 2 * w), dtype=torch.bfloat16, device=self.device)
        if starts is not None:
            starts = _require_cuda(starts, torch.int32, "starts")
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_attention_split(self.handle, _ptr(qkv), _ptr(planes), _ptr(starts), n_seq, seq_len, heads,
                                                     int(causal), _stream()))
        return planes[:, :w].float() + planes[:, w:].float()

    def attention_split_ex(self, qkv: torch.Tensor, n_seq: int, seq_len: int, heads: int, causal: bool,
                           starts: Optional[torch.Tensor] = None, pfx: Optional[torch.Tensor] = None) -> torch.Tensor:
        """:meth:`attention_split` plus prefix sharing (``tvc_attention_split_ex``): ``pfx`` int32 [2 * n_seq] as in
        :meth:`attention_ex`.  Rows the kernel does not write come back as zeros."""
        qkv = _require_cuda(qkv, torch.float32, "qkv")
        w = heads * 64
        planes = torch.zeros((qkv.shape[0], 2 * w), dtype=torch.bfloat16, device=self.device)
        starts, pfx = (t if t is None else _require_cuda(t, torch.int32, name) for t, name in ((starts, "starts"), (pfx, "pfx")))
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_attention_split_ex(self.handle, _ptr(qkv), _ptr(planes), _ptr(starts), _ptr(pfx), n_seq,
                                                        seq_len, heads, int(causal), _stream()))
        return planes[:, :w].float() + planes[:, w:].float()

    def _layernorm16(self, dt: torch.dtype, fn, x, g, b) -> torch.Tensor:
        x = _require_cuda(x, torch.float32, "x")
        g = _require_cuda(g, torch.float32, "g")
        b = _require_cuda(b, torch.float32, "b")
        out = torch.empty(x.shape, dtype=dt, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(fn(self.handle, _ptr(x), _ptr(g), _ptr(b), _ptr(out), x.shape[0], x.shape[1], _stream()))
        return out

    def layernorm(self, x: torch.Tensor, g: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        return self._layernorm16(torch.bfloat16, self.lib.tvc_layernorm, x, g, b)

    def layernorm_f16(self, x: torch.Tensor, g: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        return self._layernorm16(torch.float16, self.lib.tvc_layernorm_f16, x, g, b)

    def tower_op(self, op: str, ins=(), outs=(), i=()) -> None:
        """One row kernel of the towers on the caller's tensors (``tvc_tower_op``; needs no weights).  ``op`` is a key of
        ``_lib.TOWER_OPS``; ``ins`` / ``outs`` / ``i`` fill the slots include/tvc.h lists for it (``None`` = NULL).  Nothing is
        converted, copied or checked here: the tensors' data pointers are passed as they are, a view inside a larger buffer
        included.  Raises ``TVCError`` where the C-ABI refuses the call."""
        a = _lib.TowerOpArgs()
        for k, t in enumerate(ins):
            a.inp[k] = None if t is None else t.data_ptr()
        for k, t in enumerate(outs):
            a.out[k] = None if t is None else t.data_ptr()
        for k, v in enumerate(i):
            a.i[k] = int(v)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_tower_op(self.handle, _lib.TOWER_OPS[op], C.byref(a), _stream()))

    def grad_split_op(self, op: str, ins=(), outs=(), i=()) -> None:
        """One fp32 row kernel of the split-bf16 input gradient on the caller's tensors (``tvc_grad_split_op``): ``tower_op``'s
        conventions, ``op`` a key of ``_lib.GRAD_SPLIT_OPS``."""
        a = _lib.TowerOpArgs()
        for k, t in enumerate(ins):
            a.inp[k] = None if t is None else t.data_ptr()
        for k, t in enumerate(outs):
            a.out[k] = None if t is None else t.data_ptr()
        for k, v in enumerate(i):
            a.i[k] = int(v)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.tvc_grad_split_op(self.handle, _lib.GRAD_SPLIT_OPS[op], C.byref(a), _stream()))

    PROF_CATEGORIES = ("gemm", "attention", "bank", "rowops")

    def profile_begin(self) -> None:
        self._check(self.lib.tvc_profile_begin(self.handle))

    def profile_end(self) -> Dict[str, Dict[str, float]]:
        """Per kernel category: summed kernel ms (HIP events on the launch stream),
        summed algorithmic work (FLOPs; bytes for row ops) and launch count."""
        ms = (C.c_double * 4)()
        work = (C.c_double * 4)()
        n = (C.c_int64 * 4)()
        big = (C.c_double * 3)()
        self._check(self.lib.tvc_profile_end(self.handle, ms, work, n, big))
        out = {c: {"ms": ms[i], "work": work[i], "launches": int(n[i])} for i, c in enumerate(self.PROF_CATEGORIES)}
        # the GEMM launches of >= 64 tiles (the ring kernels): compulsory HBM bytes, count, ms
        out["gemm"].update({"big_bytes": big[0], "big_launches": int(big[1]), "big_ms": big[2]})
        return out

    def set_option(self, option: int, value: int) -> None:
        """``_lib.TVC_OPT_*`` (e.g. text packing on / off)."""
        self._check(self.lib.tvc_set_option(self.handle, option, value))
        if option == _lib.TVC_OPT_SD_PRECISION:
            self.sd_precision = "fp16" if value else "bf16"

    SD_PRECISIONS = {"bf16": 0, "fp16": 1}

    def set_sd_precision(self, precision: str) -> None:
        """The 16-bit format of the latent-diffusion model on this handle (``TVC_OPT_SD_PRECISION``): ``"bf16"`` (default) or
        ``"fp16"`` -- the tensors given to ``tvc_sd_load`` and the operands of ``tvc_sd_attention`` are then IEEE fp16.
        Independent of the towers' ``set_precision``.  Changing it while a model is loaded raises ``TVCError`` (TVC_E_STATE)."""
        if precision not in self.SD_PRECISIONS:
            raise ValueError(f"SD precision must be one of {sorted(self.SD_PRECISIONS)} (got {precision!r})")
        with self._lock:
            self.set_option(_lib.TVC_OPT_SD_PRECISION, self.SD_PRECISIONS[precision])

    def workspace_bytes(self) -> int:
        return int(self.lib.tvc_workspace_bytes(self.handle))
