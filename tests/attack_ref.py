"""Torch restatement of the FSTA / SMA attacks (src/attacks/fsta_attack.py:156-297, src/attacks/sma_attack.py:207-373,577-735):
the feature loss as plain torch ops (for autograd), its closed-form gradient with the error scale of an fp32 evaluation, the
step, and the loop both attacks share.  Works in the dtype of its inputs; the tests evaluate it in fp64.  What the kernels
(csrc/attack.hip) are compared with, and what reproduces the committed fixture (tests/golden/fsta_sma_t16.npz)."""
from typing import Callable, Dict, Sequence, Tuple

import torch

F = torch.nn.functional


# the shapes the gradient is tested at, on the CPU and on the GPU: one row, two, an odd D under one pass of 256 threads, more
# than one pass, more rows than a wave and D = 3 passes
SHAPES = [(1, 128), (2, 128), (3, 100), (5, 512), (33, 768)]
WEIGHTS = dict(a_tgt=-1.3, a_txt=0.7, w_out=0.1, w_div=0.05)


def make_rows(B: int, D: int, dtype=torch.float64):
    """f, t, g [B, D] with rows of different lengths and the degenerate rows: row 0 of g equals row 0 of f (distance 0 under
    the Euclidean metric), and with B >= 3 rows 1 and 2 of f are identical.  Drawn in fp32, so every dtype sees the same values."""
    gen = torch.Generator().manual_seed(1000 * B + D)
    f = torch.randn((B, D), generator=gen) * (0.5 + torch.rand((B, 1), generator=gen))
    t = torch.randn((B, D), generator=gen) * (0.5 + torch.rand((B, 1), generator=gen))
    g = torch.randn((B, D), generator=gen) * (0.5 + torch.rand((B, 1), generator=gen))
    g[0] = f[0]
    if B >= 3:
        f[2] = f[1]
    return f.to(dtype), t.to(dtype), g.to(dtype)


def feature_loss(f, t, g, *, a_tgt: float, a_txt: float, metric: str = "cosine", w_out: float = 0.0, w_div: float = 0.0):
    """L = a_tgt mean cos(f, g) + a_txt mean cos(f, t) + w_out mse(f, g) + w_div div(f) with torch's own ops, written the
    way the two attack files write it (the [B, B] cosine matrix included)."""
    B = f.shape[0]
    if metric == "cosine":
        loss = a_tgt * F.cosine_similarity(f, g, dim=1).mean() + a_txt * F.cosine_similarity(f, t, dim=1).mean()
    elif metric == "euclidean":
        loss = -a_tgt * torch.norm(f - g, p=2, dim=1).mean() - a_txt * torch.norm(f - t, p=2, dim=1).mean()
    else:
        raise ValueError(metric)
    loss = loss + w_out * F.mse_loss(f, g)
    if B > 1:
        sim = F.cosine_similarity(f.unsqueeze(1), f.unsqueeze(0), dim=2)
        sim = sim.masked_fill(torch.eye(B, dtype=torch.bool), 0)
        loss = loss + w_div * sim.sum() / (B * (B - 1))
    return loss


def feature_grad_autograd(f, t, g, **kw) -> torch.Tensor:
    x = f.clone().requires_grad_(True)
    grad, = torch.autograd.grad(feature_loss(x, t, g, **kw), x)
    return grad


def feature_grad(f, t, g, *, a_tgt: float, a_txt: float, metric: str = "cosine", w_out: float = 0.0, w_div: float = 0.0
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The closed forms -> (grad [B, D], loss_rows [B, 4], A_grad [B, D], A_rows [B, 4]).

    A is the scale an fp32 evaluation's error is measured against: per output element the sum of the absolute values of its
    addends, every dot-product coefficient c = sum_c x_c y_c replaced by sum_c |x_c y_c| (and S - fh_i by sum_j |fh_j| + |fh_i|:
    it is formed by that subtraction).  A term whose weight is 0 adds nothing to either."""
    B, D = f.shape
    n = f.norm(dim=1, keepdim=True)
    fh = f / n
    grad = torch.zeros_like(f)
    A = torch.zeros_like(f)
    rows = torch.zeros((B, 4), dtype=f.dtype)
    A_rows = torch.zeros((B, 4), dtype=f.dtype)
    for col, (a, v) in enumerate(((a_tgt, g), (a_txt, t))):
        if metric == "cosine":
            vh = v / v.norm(dim=1, keepdim=True)
            c = (fh * vh).sum(1, keepdim=True)
            cabs = (fh * vh).abs().sum(1, keepdim=True)
            rows[:, col], A_rows[:, col] = c[:, 0], cabs[:, 0]
            if a != 0:
                grad = grad + a * (vh - c * fh) / (n * B)
                A = A + abs(a) * (vh.abs() + cabs * fh.abs()) / (n * B)
        else:
            d = f - v
            dist = d.norm(dim=1, keepdim=True)
            rows[:, col], A_rows[:, col] = dist[:, 0], dist[:, 0]
            if a != 0:
                unit = torch.where(dist > 0, d / torch.where(dist > 0, dist, torch.ones_like(dist)), torch.zeros_like(d))
                grad = grad - a * unit / B
                A = A + abs(a) * unit.abs() / B
    rows[:, 2] = ((f - g) ** 2).sum(1) / D
    A_rows[:, 2] = rows[:, 2]
    if w_out != 0:
        grad = grad + 2 * w_out * (f - g) / (B * D)
        A = A + 2 * abs(w_out) * (f - g).abs() / (B * D)
    if B > 1:
        S = fh.sum(0, keepdim=True)
        Sabs = fh.abs().sum(0, keepdim=True)
        q = (fh * S).sum(1, keepdim=True)
        qabs = (fh.abs() * Sabs).sum(1, keepdim=True)
        rows[:, 3], A_rows[:, 3] = q[:, 0] - 1, qabs[:, 0] + 1
        if w_div != 0:
            k = 2 * w_div / (n * B * (B - 1))
            grad = grad + k * ((S - fh) - (q - 1) * fh)
            A = A + k.abs() * ((Sabs + fh.abs()) + (qabs + 1) * fh.abs())
    return grad, rows, A, A_rows


def step(adv, clean, grad, mom, *, eps: float, lr: float, mu: float, clip: float, p: float, lo: float, hi: float, norm: str = "inf"
         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One step -> (adv, mom), the operations in the order the attack files apply them."""
    g = grad if p == 0 else grad + p * (adv - clean)
    if clip > 0:
        g = torch.clamp(g, -clip, clip)
    m = mu * mom + g
    if norm == "inf":
        a = adv - lr * m.sign()
        a = clean + torch.clamp(a - clean, -eps, eps)
    elif norm == "l2":
        a = adv - lr * m
        d = a - clean
        dn = torch.norm(d.reshape(d.shape[0], -1), p=2, dim=1)
        factor = torch.min(torch.ones_like(dn), eps / (dn + 1e-8))
        a = clean + d * factor.view(-1, *([1] * (d.dim() - 1)))
    else:
        raise ValueError(norm)
    return torch.clamp(a, lo, hi), m


def run_loop(forward: Callable[[torch.Tensor], torch.Tensor], clean: torch.Tensor, t: torch.Tensor, g: torch.Tensor, *,
             lrs: Sequence[float], a_tgt: float, a_txt: float, metric: str = "cosine", w_out: float = 0.0, w_div: float = 0.0,
             eps: float, mu: float, clip: float, perceptual_weight: float = 0.0, lo: float = 0.0, hi: float = 1.0,
             norm: str = "inf") -> torch.Tensor:
    """The loop both attacks run: forward(adv) -> unit image rows; the closed-form embedding gradient (evaluated in fp64,
    handed back in the tower's dtype); autograd through the tower; the step.  Starts at adv = clean, no random start."""
    adv = clean.clone()
    mom = torch.zeros_like(clean)
    p = 2.0 * perceptual_weight / clean.numel()
    for lr in lrs:
        x = adv.clone().requires_grad_(True)
        f = forward(x)
        gf = feature_grad(f.detach().double(), t.double(), g.double(), a_tgt=a_tgt, a_txt=a_txt, metric=metric, w_out=w_out,
                          w_div=w_div)[0].to(f.dtype)
        gx, = torch.autograd.grad(f, x, gf)
        adv, mom = step(adv, clean, gx, mom, eps=eps, lr=lr, mu=mu, clip=clip, p=p, lo=lo, hi=hi, norm=norm)
    return adv


def loop_constants(kind: str, cfg: Dict) -> Dict:
    """The constants of ``run_loop`` / of the kernels from a config's values (a dict of the fixture's recorded fields):
    kind 'fsta', or 'sma_batch' (the batch core: gradient_clip_value)."""
    if kind == "fsta":
        fw = float(cfg["feature_weight"])
        return dict(a_tgt=-fw, a_txt=fw, metric=str(cfg["feature_distance_metric"]), w_out=float(cfg["output_weight"]),
                    w_div=float(cfg["diversity_weight"]), eps=float(cfg["epsilon"]), mu=float(cfg["momentum"]),
                    clip=float(cfg["clip_value"]) if cfg["gradient_clipping"] else 0.0, perceptual_weight=0.0,
                    lo=float(cfg["clamp_min"]), hi=float(cfg["clamp_max"]), norm=str(cfg["norm_type"]))
    k = float(cfg["semantic_weight"]) * (1.0 + float(cfg["semantic_shift_strength"]))
    return dict(a_tgt=-k, a_txt=k, metric="cosine", w_out=0.0, w_div=float(cfg["diversity_weight"]), eps=float(cfg["epsilon"]),
                mu=float(cfg["momentum"]), clip=float(cfg["gradient_clip_value"]) if cfg["gradient_clipping"] else 0.0,
                perceptual_weight=float(cfg["perceptual_weight"]), lo=float(cfg["clamp_min"]), hi=float(cfg["clamp_max"]),
                norm=str(cfg["norm_type"]))


FIXTURE_RUNS = ("fsta", "sma", "fsta_l2")
# the config fields the fixture records per run (arrays of one element each, named <run>_cfg_<field>)
FIXTURE_FIELDS = {
    "fsta": ("epsilon", "num_iter", "feature_distance_metric", "feature_weight", "output_weight", "diversity_weight", "momentum",
             "decay_factor", "learning_rate", "norm_type", "clamp_min", "clamp_max", "adaptive_step_size", "gradient_clipping",
             "clip_value"),
    "sma": ("epsilon", "num_iter", "semantic_weight", "perceptual_weight", "diversity_weight", "semantic_shift_strength", "momentum",
            "decay_factor", "learning_rate", "gamma_epochs", "norm_type", "clamp_min", "clamp_max", "adaptive_step_size",
            "gradient_clipping", "gradient_clip_value"),
}
FIXTURE_FIELDS["fsta_l2"] = FIXTURE_FIELDS["fsta"]


def fixture_config(z, run: str) -> Dict:
    """The recorded config values of one run of the fixture as Python scalars."""
    out = {}
    for k in FIXTURE_FIELDS[run]:
        v = z[f"{run}_cfg_{k}"]
        out[k] = v.item() if v.dtype.kind != "U" else str(v.item())
    return out
