"""fp64 references of the latent-diffusion generator's row kernels (csrc/sd_ops.hip), written from each operation's
definition, plus the layout helpers and the 16-bit rounding the GPU tests judge a kernel's output with
(tests/test_gpu_sd_ops.py).  tests/test_sd_ops_ref.py checks every function here against torch's own fp64 op on the CPU.

Activations are channels-last: [n, H, W, C] here, the kernels' "tokens" [n * H * W, C] after ``.reshape(-1, C)``.
All functions take and return CPU float64 tensors unless they say otherwise."""
import math

import torch

FORMATS = {                       # significand bits (hidden one included), exponent range of the normal numbers, torch dtype
    "bf16": dict(p=8, emin=-126, emax=127, dtype=torch.bfloat16),
    "fp16": dict(p=11, emin=-14, emax=15, dtype=torch.float16),
}


# ------------------------------------------------------------------------------------------------- 16-bit formats
def max_finite(fmt):
    f = FORMATS[fmt]
    return (2.0 - 2.0 ** (1 - f["p"])) * 2.0 ** f["emax"]


def _spacing(x64, fmt, clamp_top):
    """Distance between neighbouring numbers of the format in the binade of |x| (the subnormal spacing below the
    smallest normal number; ``clamp_top``: the top binade's spacing beyond it too)."""
    f = FORMATS[fmt]
    a = x64.abs()
    fin = torch.isfinite(a)
    _, e = torch.frexp(torch.where(fin, a, torch.ones_like(a)))          # a = m * 2^e, m in [0.5, 1)
    E = (e.to(torch.int64) - 1).clamp(min=f["emin"])
    E = torch.where(a == 0, torch.full_like(E, f["emin"]), E)
    if clamp_top:
        E = torch.where(fin, E.clamp(max=f["emax"]), torch.full_like(E, f["emax"]))
    return torch.ldexp(torch.ones_like(a), E - (f["p"] - 1))


def round16(x64, fmt):
    """x rounded to the format, round to nearest even, as float64: overflow goes to +-inf (never clamped), the sign of a
    zero result is kept, inf / nan pass through."""
    x64 = x64.double()
    q = _spacing(x64, fmt, False)
    r = torch.round(x64 / q) * q                                          # torch.round: half to even; x / q is exact
    r = torch.where(r.abs() > max_finite(fmt), torch.copysign(torch.full_like(r, math.inf), x64), r)
    return torch.where(torch.isfinite(x64), r, x64)


def ulp16(x64, fmt):
    """The format's spacing at |x| (one unit in the last place of a result near x); the top binade's beyond the range."""
    return _spacing(x64.double(), fmt, True)


def bits16(x64, fmt):
    """The int16 bit patterns of round16(x)."""
    return round16(x64, fmt).to(FORMATS[fmt]["dtype"]).view(torch.int16)


# ------------------------------------------------------------------------------------------------------- layouts
def tok_row(img, t, H, W, pad):
    """Row of pixel t = y * W + x of image img among the token rows: dense, or in the padded layout where every image is
    an (H + 2) x (W + 2) grid and pixel (y, x) sits at (y + 1, x + 1)."""
    if not pad:
        return img * H * W + t
    y, x = divmod(t, W)
    return img * (H + 2) * (W + 2) + (y + 1) * (W + 2) + (x + 1)


def to_padded(x, fill=0.0):
    """[n, H, W, C] -> [n, H + 2, W + 2, C] with ``fill`` in every border element."""
    n, H, W, C = x.shape
    out = torch.full((n, H + 2, W + 2, C), fill, dtype=x.dtype)
    out[:, 1:-1, 1:-1] = x
    return out


def interior(xp):
    return xp[:, 1:-1, 1:-1]


def border_mask(n, H, W):
    """bool [n, H + 2, W + 2]: True on the border rows / columns of the padded layout."""
    m = torch.ones((n, H + 2, W + 2), dtype=torch.bool)
    m[:, 1:-1, 1:-1] = False
    return m


def im2col_column(ky, kx, c, C):
    """Column of tap (ky, kx), channel c in a row of the 3x3 gather: tap-major."""
    return (ky * 3 + kx) * C + c


# ----------------------------------------------------------------------------------------------------- the ops
def silu(v):
    return v / (1.0 + torch.exp(-v))


def groupnorm(x, tadd, gamma, beta, groups, eps, act=False, parts=False):
    """GroupNorm of x + tadd[img, c] over (pixels, channels of a group), biased variance, then gamma / beta, then SiLU.
    x [n, H, W, C], tadd [n, C] or None.  ``parts``: also the pre-activation value and the magnitude sum of its terms
    |x' rstd gamma| + |mean rstd gamma| + |beta|."""
    n, H, W, C = x.shape
    xs = x if tadd is None else x + tadd[:, None, None, :]
    g = xs.reshape(n, H * W, groups, C // groups)
    mean = g.mean(dim=(1, 3), keepdim=True)
    var = ((g - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    pre = ((g - mean) * rstd).reshape(n, H, W, C) * gamma + beta
    y = silu(pre) if act else pre
    if not parts:
        return y
    mag = ((g.abs() + mean.abs()) * rstd).reshape(n, H, W, C) * gamma.abs() + beta.abs()
    return y, pre, mag


def layernorm(x, g, b, eps, parts=False):
    """LayerNorm over the last axis, biased variance.  ``parts``: also |x - mean| rstd |g| + |b|."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean) * rstd * g + b
    if not parts:
        return y
    return y, (x.abs() + mean.abs()) * rstd * g.abs() + b.abs()


def gelu_erf(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def geglu(x):
    """[rows, 2 * Ch] (value | gate) -> value * gelu(gate)."""
    ch = x.shape[1] // 2
    return x[:, :ch] * gelu_erf(x[:, ch:])


def softmax_rows(s, scale):
    z = s * scale
    z = z - z.max(-1, keepdim=True).values
    e = torch.exp(z)
    return e / e.sum(-1, keepdim=True)


def upsample2(x):
    """Nearest-neighbour 2x: [n, H, W, C] -> [n, 2H, 2W, C]."""
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def relayout(x, in_pad, out_pad, up, fill=0.0):
    """Dense / padded copy ([n, H(+2), W(+2), C] in and out), optionally through the nearest-2x upsampling; the borders
    of a padded input are dropped, those of a padded output hold ``fill`` (the kernels': zero)."""
    d = interior(x) if in_pad else x
    if up:
        d = upsample2(d)
    return to_padded(d, fill) if out_pad else d


def im2col3x3(x, stride=1, up=False):
    """[n, Hi, Wi, C] -> [n * Ho * Wo, 9 * C]: row (img, y, x), column im2col_column(ky, kx, c) holds the source pixel
    (y * stride + ky - 1, x * stride + kx - 1) of the (upsampled) input, zero outside it."""
    if up:
        x = upsample2(x)
    n, Hs, Ws, C = x.shape
    Ho, Wo = (Hs - 1) // stride + 1, (Ws - 1) // stride + 1
    xp = to_padded(x)
    out = torch.zeros((n, Ho, Wo, 9 * C), dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            c0 = im2col_column(ky, kx, 0, C)
            out[..., c0:c0 + C] = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
    return out.reshape(n * Ho * Wo, 9 * C)


def im2col_in(x_nchw, Kp, scale):
    """fp32-style NCHW [n, Cin, H, W] -> [n * H * W, Kp]: column tap * Cin + ci of x * scale, zeros from 9 * Cin on."""
    n, Cin, H, W = x_nchw.shape
    cols = im2col3x3((x_nchw * scale).permute(0, 2, 3, 1))
    out = torch.zeros((n * H * W, Kp), dtype=x_nchw.dtype)
    out[:, :9 * Cin] = cols
    return out


def concat(a, b):
    return torch.cat([a, b], dim=1)


def tokens_to_nchw(rows, n, C, H, W, mul, add, clamp, in_pad):
    """rows [*, ld] (dense, or padded with in_pad): the first C columns -> NCHW, * mul + add, optionally clamped to
    [0, 1].  Returns (value, magnitude sum |x mul| + |add|)."""
    ld = rows.shape[1]
    g = rows.reshape(n, H + 2, W + 2, ld) if in_pad else rows.reshape(n, H, W, ld)
    g = (interior(g) if in_pad else g)[..., :C].permute(0, 3, 1, 2)
    v = g * mul + add
    return (v.clamp(0.0, 1.0) if clamp else v), (g * mul).abs() + abs(add)


def nchw_to_tokens(x):
    n, C = x.shape[:2]
    return x.reshape(n, C, -1).permute(0, 2, 1).reshape(-1, C)


def tokens_to_nchw16(rows, n):
    C = rows.shape[1]
    return rows.reshape(n, -1, C).permute(0, 2, 1)


def pointwise_small(x, w, bias, in_scale):
    """x [n, C, HW]: bias[c] + sum_ci w[c, ci] * (x[n, ci, p] * in_scale).  Returns (value, magnitude sum)."""
    xs = x * in_scale
    v = torch.einsum("oc,ncp->nop", w, xs) + bias[None, :, None]
    return v, torch.einsum("oc,ncp->nop", w.abs(), xs.abs()) + bias.abs()[None, :, None]


def cfg(e, g):
    """e = [unconditional | conditional] halves: eu + g * (ec - eu).  Returns (value, magnitude sum)."""
    n = e.numel() // 2
    eu, ec = e[:n], e[n:]
    return eu + g * (ec - eu), eu.abs() + abs(g) * (ec.abs() + eu.abs())


def lincomb(sample, cs, ce, es, cs_e):
    """cs * sample - ce * sum_i c_i e_i.  Returns (value, magnitude sum)."""
    m = sum(c * e for c, e in zip(cs_e, es))
    mag = sum(abs(c) * e.abs() for c, e in zip(cs_e, es))
    return cs * sample - ce * m, abs(cs) * sample.abs() + abs(ce) * mag


def timestep_embed(t, dim):
    """[cos | sin](t * 10000^(-j / half)), j < half = dim / 2.  Returns (row [dim], the angles [dim])."""
    half = dim // 2
    ang = t * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    return torch.cat([torch.cos(ang), torch.sin(ang)]), torch.cat([ang, ang])


# ------------------------------------------------------------------------- GroupNorm in the kernel's summation order
def _f32(x):
    return x.to(torch.float32)


def gn_emulated(x, tadd, gamma, beta, groups, eps, slab_tokens=64):
    """GroupNorm (no activation) with the statistics summed the way gn_partial_kernel / gn_apply_kernel sum them: fp32
    sums of x' and x'^2 per (token lane, channel) inside slabs of ``slab_tokens`` tokens (a lane takes every lanes-th
    token, two at a time), fp32 over lanes and a group's channels inside a slab, fp64 across slabs, variance as
    E[x'^2] - mean^2, mean and rstd kept in fp32, one fp32 fma per element.  x [n, H, W, C] of 16-bit-representable
    values, tadd [n, C] fp32-representable or None.  Only there to SIZE a conditioning slack: the deviation of this from
    ``groupnorm`` is what fp32 statistics of this order cost on a given input.  Returns float64 [n, H, W, C]."""
    n, H, W, C = x.shape
    HW, cpg = H * W, C // groups
    cv = C // 8
    lanes = 256 // min(cv, 256)
    xf = _f32(x).reshape(n, HW, C)
    ta = torch.zeros((n, C), dtype=torch.float32) if tadd is None else _f32(tadd)
    S = torch.zeros((n, groups), dtype=torch.float64)
    Q = torch.zeros((n, groups), dtype=torch.float64)
    for t0 in range(0, HW, slab_tokens):
        t1 = min(HW, t0 + slab_tokens)
        ls = torch.zeros((lanes, n, C), dtype=torch.float32)
        lq = torch.zeros((lanes, n, C), dtype=torch.float32)
        for tl in range(lanes):
            s = torch.zeros((n, C), dtype=torch.float32)
            q = torch.zeros((n, C), dtype=torch.float32)
            t = t0 + tl
            while t + lanes < t1:
                a, b = xf[:, t] + ta, xf[:, t + lanes] + ta
                s = s + (a + b)
                q = q + (a * a + b * b)
                t += 2 * lanes
            while t < t1:
                a = xf[:, t] + ta
                s = s + a
                q = q + a * a
                t += lanes
            ls[tl], lq[tl] = s, q
        ss = torch.zeros((n, groups), dtype=torch.float32)
        qq = torch.zeros((n, groups), dtype=torch.float32)
        for l in range(lanes):
            for c in range(cpg):
                ss = ss + ls[l].reshape(n, groups, cpg)[:, :, c]
                qq = qq + lq[l].reshape(n, groups, cpg)[:, :, c]
        S += ss.double()
        Q += qq.double()
    count = float(HW * cpg)
    mean = S / count
    var = (Q / count - mean * mean).clamp(min=0.0)
    mean32 = _f32(mean)
    rstd32 = _f32(1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32))))
    mean_c = mean32.repeat_interleave(cpg, 1)                     # [n, C]
    rstd_c = rstd32.repeat_interleave(cpg, 1)
    sc = rstd_c * _f32(gamma)
    sh = _f32(beta) + (ta - mean_c) * sc
    y = _f32(xf.double() * sc.double()[:, None, :] + sh.double()[:, None, :])       # one rounding: the fma
    return y.double().reshape(n, H, W, C)
