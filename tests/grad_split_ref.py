"""fp64 references of the split-bf16 input gradient (TVC_OPT_GRAD_PRECISION = 2): the attention backward in closed form, the
whole tower gradient through ``oracle/clip_oracle.vision_forward`` in double (no step of the oracle hard-codes float32: it
runs on whatever dtype its weights and input have), the cosine loss the tests differentiate, and the operand view of the
hi | lo planes.  tests/test_grad_split_ref.py checks these against torch autograd; tests/test_gpu_grad_split.py judges the
kernels with them."""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import clip_oracle


def operands(x: torch.Tensor) -> torch.Tensor:
    """fp64 values of fp32 ``x`` as the split kernels see them: hi + lo of its bf16 planes (tests/test_gpu_kmeans.py::operands)."""
    hi = x.bfloat16().float()
    lo = (x - hi).bfloat16().float()
    return hi.double() + lo.double()


def to_double(w):
    """The weight dict of ``synth.make_clip_weights`` (one tower) in fp64."""
    if isinstance(w, dict):
        return {k: to_double(v) for k, v in w.items()}
    if isinstance(w, (list, tuple)):
        return [to_double(v) for v in w]
    return w.double() if torch.is_tensor(w) and w.is_floating_point() else w


def attention_parts64(qkv: torch.Tensor, heads: int, n_seq: int, T: int):
    """qkv [n_seq * T, 3 * heads * 64] fp64 -> q, k, v [n_seq, heads, T, 64], P [n_seq, heads, T, T]."""
    W = heads * 64
    q, k, v = (qkv[:, i * W:(i + 1) * W].reshape(n_seq, T, heads, 64).transpose(1, 2) for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    return q, k, v, p


def attention_backward64(qkv: torch.Tensor, dout: torch.Tensor, heads: int, n_seq: int, T: int) -> torch.Tensor:
    """The closed form the kernel follows, in fp64: dV = P^T dO, dP = dO V^T, dS = P (dP - rowsum(dO * O)),
    dQ = dS K / 8, dK = dS^T Q / 8.  -> dqkv [n_seq * T, 3 * heads * 64]."""
    W = heads * 64
    q, k, v, p = attention_parts64(qkv, heads, n_seq, T)
    do = dout.reshape(n_seq, T, heads, 64).transpose(1, 2)
    o = p @ v
    dv = p.transpose(-1, -2) @ do
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (do * o).sum(-1, keepdim=True))
    dq = ds @ k / 8.0
    dk = ds.transpose(-1, -2) @ q / 8.0
    back = lambda x: x.transpose(1, 2).reshape(n_seq * T, W)
    return torch.cat([back(dq), back(dk), back(dv)], dim=1)


def attention_autograd64(qkv: torch.Tensor, dout: torch.Tensor, heads: int, n_seq: int, T: int) -> torch.Tensor:
    x = qkv.clone().requires_grad_(True)
    _, _, v, p = attention_parts64(x, heads, n_seq, T)
    o = (p @ v).transpose(1, 2).reshape(n_seq * T, heads * 64)
    o.backward(dout)
    return x.grad


def cos_grad64(f: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """d cos(f_b, t) / d f_b for rows f [B, D] of any norm and one text row t [D], fp64."""
    fn, tn = f.norm(dim=-1, keepdim=True), t.norm()
    c = (f @ t).unsqueeze(-1) / (fn * tn)
    return t / (fn * tn) - c * f / (fn * fn)


def tower_grad64(vw, pixels: torch.Tensor, text_row: torch.Tensor, heads: int, patch: int, normalize: bool):
    """The double oracle tower on fp32 ``vw`` / ``pixels`` cast to fp64 -> (f [B, D], grad_out [B, D], grad_pix [B, 3, S, S]):
    grad_out = d(sum_b cos(f_b, t)) / df in closed form (``cos_grad64``), grad_pix its pull-back through the tower."""
    x = pixels.double().clone().requires_grad_(True)
    f = clip_oracle.vision_forward(to_double(vw), x, heads, patch, normalize=normalize)
    g = cos_grad64(f.detach(), text_row.double())
    (gp,) = torch.autograd.grad(f, x, g)
    return f.detach(), g, gp


def tower_grad64_autograd(vw, pixels: torch.Tensor, text_row: torch.Tensor, heads: int, patch: int, normalize: bool) -> torch.Tensor:
    """The same gradient with the loss differentiated by autograd end to end."""
    x = pixels.double().clone().requires_grad_(True)
    f = clip_oracle.vision_forward(to_double(vw), x, heads, patch, normalize=normalize)
    torch.nn.functional.cosine_similarity(f, text_row.double().unsqueeze(0), dim=-1, eps=0.0).sum().backward()
    return x.grad


def rel_l2(a, ref) -> float:
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-300))


def max_max(a, ref) -> float:
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def sign_flips(a, ref) -> float:
    """Share of elements whose sign differs from the reference's."""
    return float((np.sign(np.asarray(a, dtype=np.float64)) != np.sign(np.asarray(ref, dtype=np.float64))).mean())


@functools.lru_cache(maxsize=None)
def attention_case(T: int, heads: int, n_seq: int):
    """-> (qkv fp32, dout fp32, fp64 dqkv of the operands the kernel sees); computed once, shared, never modified."""
    g0 = torch.Generator().manual_seed(1000 * T + 10 * heads + n_seq)
    W = heads * 64
    qkv = torch.randn(n_seq * T, 3 * W, generator=g0) * 0.7
    dout = torch.randn(n_seq * T, W, generator=g0) * 0.7
    return qkv, dout, attention_backward64(operands(qkv), operands(dout), heads, n_seq, T)
