"""fp64 references of the CLIP towers' row kernels (csrc/elementwise.hip, backward.hip, and the row kernels of split.hip and
precise.hip), written from each operation's definition, for tests/test_gpu_tower_ops.py.  tests/test_tower_ops_ref.py checks
every function here against torch's own fp64 op or autograd on the CPU.  The text length / embedding references are plain
integer Python.  The 16-bit rounding comes from sd_ops_ref.

All functions take and return CPU float64 tensors unless they say otherwise."""
import torch

from sd_ops_ref import FORMATS, bits16, gelu_erf, max_finite, round16, ulp16  # noqa: F401  (re-exported for the GPU tests)

LN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))      # csrc/rows.hpp: the fp32 constant


def f32(x64):
    """x rounded to fp32, as float64 (what an fp32 addition of exact operands stores)."""
    return x64.to(torch.float32).double()


def fold_deltas(x, d1=None, d2=None):
    """The LayerNorm kernels' folded residual adds: fp32 (x + d1) + d2, in that order (x, d1, d2 hold fp32 / 16-bit values)."""
    s = x
    if d1 is not None:
        s = f32(s + d1)
    if d2 is not None:
        s = f32(s + d2)
    return s


# ------------------------------------------------------------------------------------------------ LayerNorm family
def _stats(x, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + eps)


def layernorm(x, g, b, eps=LN_EPS, parts=False):
    """LayerNorm over the last axis, biased variance.  ``parts``: also M = |y| + |xhat g| + |mean rstd g| + |b|."""
    mean, rstd = _stats(x, eps)
    xhat = (x - mean) * rstd
    y = xhat * g + b
    if not parts:
        return y
    return y, y.abs() + (xhat * g).abs() + (mean * rstd * g).abs() + b.abs()


def layernorm_bwd(x, dy, gamma, dres=None, eps=LN_EPS, parts=False):
    """Gradient of LayerNorm(x) * gamma + beta w.r.t. x for the output gradient dy, plus dres:
    dx = rstd (g - mean(g) - xhat mean(g xhat)) + dres, g = dy gamma.
    ``parts``: also M = |dx| + rstd (|g| + mean|g| + |xhat| mean|g xhat|) + |dres| (the two row means are sums of d terms)."""
    mean, rstd = _stats(x, eps)
    xhat = (x - mean) * rstd
    g = dy * gamma
    c1 = g.mean(-1, keepdim=True)
    c2 = (g * xhat).mean(-1, keepdim=True)
    dx = rstd * (g - c1 - xhat * c2)
    if dres is not None:
        dx = dx + dres
    if not parts:
        return dx
    mag = dx.abs() + rstd * (g.abs() + g.abs().mean(-1, keepdim=True) + xhat.abs() * (g * xhat).abs().mean(-1, keepdim=True))
    if dres is not None:
        mag = mag + dres.abs()
    return dx, mag


def lnpre_input(patch_out, cls, pos):
    """The rows ln_pre normalises: [B, T, d] = (t == 0 ? cls : patch_out[b, t - 1]) + pos[t], one fp32 addition.
    patch_out [B, T - 1, d], cls [d], pos [T, d]."""
    B = patch_out.shape[0]
    rows = torch.cat([cls.expand(B, 1, -1), patch_out], dim=1)
    return f32(rows + pos)


def assemble_lnpre(patch_out, cls, pos, g, b, parts=False):
    return layernorm(lnpre_input(patch_out, cls, pos), g, b, parts=parts)


def lnpre_bwd(patch_out, cls, pos, gamma, dy, parts=False):
    """dy [B, T, d] -> the gradient w.r.t. patch_out [B, T - 1, d] (the class row's goes to a parameter and is dropped)."""
    v = lnpre_input(patch_out, cls, pos)[:, 1:]
    return layernorm_bwd(v, dy[:, 1:], gamma, parts=parts)


# ------------------------------------------------------------------------------------------------ the stem's gathers
def im2col(pix, patch, Kp=None):
    """[B, 3, S, S] -> [B * P, Kp]: row (b, py, px), column (c * patch + ky) * patch + kx holds pix[b, c, py * patch + ky,
    px * patch + kx]; zeros from column 3 * patch^2 on."""
    B, Cc, S, _ = pix.shape
    g = S // patch
    K = Cc * patch * patch
    cols = pix.reshape(B, Cc, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, K)
    if Kp is None or Kp == K:
        return cols.contiguous()
    out = torch.zeros((B * g * g, Kp), dtype=pix.dtype)
    out[:, :K] = cols
    return out


def col2im(dcols, B, S, patch):
    """The inverse move: dcols [B * P, >= K] -> [B, 3, S, S] (patches do not overlap; columns from K on are ignored)."""
    g = S // patch
    K = 3 * patch * patch
    return dcols[:, :K].reshape(B, g, g, 3, patch, patch).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, S, S).contiguous()


# ------------------------------------------------------------------------------------------------------ activations
def quick_gelu(u):
    """u sigmoid(1.702 u)."""
    return u * torch.sigmoid(1.702 * u)


def quick_gelu_grad(u, parts=False):
    """d quick_gelu / du = s + 1.702 u s (1 - s).  ``parts``: also s + |1.702 u s (1 - s)| (the two terms cancel near u = -0.75)."""
    s = torch.sigmoid(1.702 * u)
    t = 1.702 * u * s * (1.0 - s)
    return (s + t, s + t.abs()) if parts else s + t


# ------------------------------------------------------------------------------------------------------------ L2
def l2norm(x):
    return x / torch.sqrt((x * x).sum(-1, keepdim=True))


def l2norm_bwd(x, dy, parts=False):
    """Gradient of y = x / |x|: (dy - y (y . dy)) / |x|.  ``parts``: also (|dy| + |y| sum|y dy|) / |x|."""
    n = torch.sqrt((x * x).sum(-1, keepdim=True))
    y = x / n
    dx = (dy - y * (y * dy).sum(-1, keepdim=True)) / n
    if not parts:
        return dx
    return dx, (dy.abs() + y.abs() * (y * dy).abs().sum(-1, keepdim=True)) / n


# -------------------------------------------------------------------------------------------------- split planes
def split_planes(x):
    """fp32 values -> (hi, lo) = (bf16(x), bf16(x - hi)) as float64."""
    hi = round16(x, "bf16")
    return hi, round16(x - hi, "bf16")


# ------------------------------------------------------------------------------------------------------- gathers
def gather_rows(bank, planes, D, idx, idx_offset):
    """bank: bf16 values [R, ld]; out[n] = fp32(bank[idx - offset, :D] (+ [D:2D])), zeros where the index is negative or the row
    outside the bank.  Returns a float32 tensor (the sum of two bf16 numbers is one fp32 addition)."""
    R = bank.shape[0]
    out = torch.zeros((len(idx), D), dtype=torch.float32)
    for n, ix in enumerate(int(v) for v in idx):
        src = ix - idx_offset
        if ix < 0 or src < 0 or src >= R:
            continue
        v = bank[src, :D].to(torch.float32)
        if planes > 1:
            v = v + bank[src, D:2 * D].to(torch.float32)
        out[n] = v
    return out


def gather_f32_rows(x, idx, idx_mul, n, d):
    """x [*, ld]; out[r] = x[idx[r], :d], or x[r * idx_mul, :d] without idx."""
    src = idx.long() if idx is not None else torch.arange(n) * idx_mul
    return x[src, :d].contiguous()


# ---------------------------------------------------------------------------------------------------- text kernels
def first_max(row):
    """Position of the first maximum (ties -> lowest position, as torch.argmax)."""
    return row.index(max(row))


def text_lens_scan(tok, G=0):
    """tok: list of n_text lists of ctx ints.  Returns (starts [n_text + 2], pfx [2 * n_text] or None, lens).
    len = first maximum + 1; with G (groups of G consecutive texts, the first is the base) prefix = min(first mismatch with
    the base, own length, base length), 0 for a base; starts = exclusive scan of len - prefix, then the total, then the
    maximum length; pfx[n_text + n] = starts[base of n]."""
    n_text = len(tok)
    lens = [first_max(r) + 1 for r in tok]
    pref = [0] * n_text
    if G:
        for n in range(n_text):
            bn = n // G * G
            if bn == n:
                continue
            a, b = tok[n], tok[bn]
            mis = next((t for t in range(len(a)) if a[t] != b[t]), len(a))
            pref[n] = min(mis, lens[n], lens[bn])
    starts, acc = [], 0
    for n in range(n_text):
        starts.append(acc)
        acc += lens[n] - pref[n]
    starts += [acc, max(lens)]
    pfx = pref + [starts[n // G * G] for n in range(n_text)] if G else None
    return starts, pfx, lens


def text_embed(tok, emb, pos, vocab, starts=None, pfx=None):
    """x rows = emb[clamp(id)] + pos[t] (one fp32 addition; emb, pos float32 tensors).  Dense (starts None): every (n, t) at row
    n * ctx + t.  Packed: text n's positions pfx[n] <= t < pfx[n] + own(n) at rows starts[n] + t - pfx[n].  Returns
    (dict row -> float32 [d], eot_row list): the EOT row is the row of the first maximum; a text with no own rows takes its
    base's: pfx[n_text + n] + pfx[n] - 1."""
    n_text, ctx = len(tok), len(tok[0])
    rows, eot = {}, []
    for n in range(n_text):
        if starts is None:
            p, own, s0 = 0, ctx, n * ctx
            eot.append(n * ctx + first_max(tok[n]))
        else:
            s0, own = starts[n], starts[n + 1] - starts[n]
            p = pfx[n] if pfx is not None else 0
            eot.append(s0 + own - 1 if own > 0 else pfx[n_text + n] + p - 1)
        for t in range(p, p + own):
            ident = min(max(tok[n][t], 0), vocab - 1)
            rows[s0 + t - p] = emb[ident] + pos[t]
    return rows, eot


# ------------------------------------------------------------------------------ the kernels' summation order, on the CPU
def _wave_sum(v):
    """The 64-lane butterfly (xor 32, 16, .. 1) in fp32: every lane ends with the same sum."""
    v = v.clone()
    o = 32
    while o:
        v = v + v[..., torch.arange(64) ^ o]
        o >>= 1
    return v[..., 0]


def ln_stats_emulated(x32):
    """(mean, rstd with an IEEE square root and division) of fp32 rows [rows, d] in the order of csrc/rows.hpp: lane l holds
    the 4-vectors l, l + 64, ..; per piece (v0 + v1) + (v2 + v3), pieces in order, then the butterfly; squared deviations one
    multiply and one add per element.  fp32 throughout."""
    rows, d = x32.shape
    nv = d // 4
    pad = torch.zeros((rows, 256 * 4), dtype=torch.float32)
    pad[:, :d] = x32
    p = pad.reshape(rows, 4, 64, 4)                       # [row, piece, lane, t]
    live = (torch.arange(4)[:, None] * 64 + torch.arange(64)[None, :]) < nv
    s = torch.zeros((rows, 64), dtype=torch.float32)
    for i in range(4):
        ps = (p[:, i, :, 0] + p[:, i, :, 1]) + (p[:, i, :, 2] + p[:, i, :, 3])
        s = torch.where(live[i], s + ps, s)
    mean = _wave_sum(s) / torch.tensor(float(d), dtype=torch.float32)
    q = torch.zeros((rows, 64), dtype=torch.float32)
    for i in range(4):
        for t in range(4):
            dl = p[:, i, :, t] - mean[:, None]
            q = torch.where(live[i], q + dl * dl, q)
    var = _wave_sum(q) / torch.tensor(float(d), dtype=torch.float32) + torch.tensor(1e-5, dtype=torch.float32)
    return mean, 1.0 / torch.sqrt(var)


def layernorm_emulated(x32, g32, b32):
    """The forward kernels' arithmetic in fp32 on the CPU (ln_stats_emulated, then fma((x - mean) rstd, g, b) -- the fma as
    an fp64 product and sum rounded once)."""
    mean, rstd = ln_stats_emulated(x32)
    t = (x32 - mean[:, None]) * rstd[:, None]
    return (t.double() * g32.double() + b32.double()).to(torch.float32)


# --------------------------------------------------- inputs and slack coefficients shared by the GPU tests and the CPU checks
NS = [8, 8 * 1000 + 8]                 # element counts of the elementwise tests
L2_D = [8, 64, 100, 768]
VOCAB, EOT, LATER = 64, 60, 61         # ids of the text tests: EOT ends a text, LATER / LATER + 1 are larger ids planted beyond it
TEXT_CTX, TEXT_N, TEXT_G = (1, 63, 64, 65, 77), (1, 5, 1024, 1025, 2500), (0, 2, 8)
TEXT_SHAPES = [(ctx, n) for ctx in TEXT_CTX for n in TEXT_N]
# Slack coefficients of the erff / expf / IEEE-division forms ("Tower row kernels alone"): per family twice the
# worst deviation of the same formula in fp32 torch on the CPU from fp64, on the GPU tests' inputs (cpu_fp32_deviation), in units
# of the magnitude sum M, rounded up to a power of two.  quick_gelu_exact stands out because the argument of expf carries the
# rounding of 1.702 x (|x| up to 13: 2^-21 absolute on the argument, which is relative on the exponential) and of 1.702f.
C_EXACT = {"gelu_erf": 2.0 ** -21, "quick_gelu_exact": 2.0 ** -19, "l2norm": 2.0 ** -21, "l2norm_bwd": 2.0 ** -21}
SUB32 = 2.0 ** -149                    # one fp32 subnormal spacing: below 2^-126 an fp32 result rounds absolutely


def rnd(seed, *shape):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def f32v(x64):
    return x64.to(torch.float32).double()


def rows_of(seed, rows, d):
    """fp32 values [rows, d], every row with another mean and scale (a wrong row shows)."""
    r = torch.arange(rows, dtype=torch.float64)[:, None]
    return f32v(rnd(seed, rows, d) * (0.5 + 0.4 * r) + (0.9 * r - 1.3))


def plant(x, vals):
    x.reshape(-1)[:len(vals)] = torch.tensor(vals, dtype=torch.float64)[:x.numel()]
    return x


def specials(fmt):
    """+-0, +-largest finite, a subnormal, +-8."""
    if fmt == "fp32":
        return [0.0, -0.0, 3.4028234663852886e38, -3.4028234663852886e38, 2.0 ** -130, 8.0, -8.0]
    return [0.0, -0.0, max_finite(fmt), -max_finite(fmt), {"bf16": 2.0 ** -130, "fp16": 2.0 ** -20}[fmt], 8.0, -8.0]


def _rows_by(n):
    """n elements as [rows, width]: 1 x 8, or 143 x 56."""
    return (1, 8) if n == 8 else (n // 56, 56)


def _u16(seed, n, fmt):
    return plant(round16(rnd(seed, n) * 3.0, fmt), specials(fmt))


def gelu_erf_mag(x):
    return 0.5 * x.abs() * (1.0 + torch.erf(x / 2.0 ** 0.5).abs())


def _rs_x(n):
    return f32v(plant(rnd(1500 + n, *_rows_by(n)) * 3.0, specials("fp32")))


def _l2_x(seed, rows, D):
    # +-0, a subnormal and +-8; not +-the largest finite number: the squared norm of such a row is not an fp32 number
    return f32v(plant(rows_of(seed, rows, D), [0.0, -0.0, 2.0 ** -130, 8.0, -8.0]))


def make_texts(n_text, ctx, G, seed):
    """n_text token rows of ctx ids.  Every text: random ids below 50, EOT at a random position, zeros after.  Planted (where
    ctx has room): the maximum twice; the maximum at position 0; at ctx - 1; an all-zero row.  With G every group holds, in turn,
    a copy of its base (no own rows), a text that differs at position 0, one longer than the base and equal on all of it, one
    shorter than the base; every third group's base carries a larger id beyond its EOT and its first member is that base without
    it, so that its first mismatch lies beyond its own length (the own-length cap of the prefix binds)."""
    g = torch.Generator().manual_seed(seed)
    body = torch.randint(1, 50, (n_text, ctx), generator=g).tolist()
    lens = torch.randint(1, ctx + 1, (n_text,), generator=g).tolist()
    where = torch.randint(0, 1 << 30, (n_text,), generator=g).tolist()
    tok = []
    for n in range(n_text):
        L = lens[n]
        tok.append(body[n][:L - 1] + [EOT] + [0] * (ctx - L))
    if n_text > 4:
        tok[1], tok[2], tok[3], tok[4] = [0] * ctx, [EOT] + [5] * (ctx - 1), [5] * (ctx - 1) + [EOT], [7] * ctx
        tok[4][ctx // 3], tok[4][ctx - 1] = EOT, EOT
        lens[1:5] = [1, 1, ctx, ctx // 3 + 1]
    if G:
        kind = 0
        for bn in range(0, n_text, G):
            gi, bl = bn // G, lens[bn]
            late = gi % 3 == 0 and bl <= ctx - 2 and bn + 1 < n_text
            if late:                                           # a larger id after the base's EOT, with a gap: the base grows to q + 1
                q = bl + 1 + where[bn] % (ctx - bl - 1)
                tok[bn][q] = LATER
                bl = q + 1
            base = tok[bn]
            for n in range(bn + 1, min(bn + G, n_text)):
                m = list(base)
                if late and n == bn + 1:                       # kind 4: the base without that id -- equal to it on all of its own
                    m[q] = 0                                   # length and one position beyond: first mismatch q > own length
                else:
                    k = kind % 4
                    kind += 1
                    if k == 1:
                        m[0] = base[0] % 40 + 1
                    elif k == 2 and bl < ctx:
                        m[bl + where[n] % (ctx - bl)] = LATER + 1
                    elif k == 3 and bl >= 3:
                        cut = 1 + where[n] % (bl - 2)
                        m = base[:cut] + [EOT] + [0] * (ctx - cut - 1)
                tok[n] = m
    return tok


def cpu_fp32_deviation():
    """Worst (|fp32 formula - fp64| - SUB32) / M per family over the inputs of the GPU tests, the formulas written as the
    kernels write them, in fp32 torch on the CPU: {family: ratio}."""
    out = {k: 0.0 for k in C_EXACT}

    def note(k, got, ref, M):
        ok = M > 0
        out[k] = max(out[k], (((got.double() - ref).abs() - SUB32).clamp(min=0)[ok] / M[ok]).max().item())

    for n in NS:
        for fmt in ("bf16", "fp16"):
            x = _u16(1300 + n, n, fmt)
            x32 = x.to(torch.float32)
            note("gelu_erf", 0.5 * x32 * (1.0 + torch.erf(x32 * 0.70710678118654752)), gelu_erf(x), gelu_erf_mag(x))
        x = f32v(plant(rnd(1200 + n, n) * 3.0, specials("fp32")))
        x32 = x.to(torch.float32)
        note("gelu_erf", 0.5 * x32 * (1.0 + torch.erf(x32 * 0.70710678118654752)), gelu_erf(x), gelu_erf_mag(x))
        x = _rs_x(n)
        x32 = x.to(torch.float32)
        note("gelu_erf", 0.5 * x32 * (1.0 + torch.erf(x32 * 0.70710678118654752)), gelu_erf(x), gelu_erf_mag(x))
        note("quick_gelu_exact", x32 / (1.0 + torch.exp(-1.702 * x32)), quick_gelu(x), quick_gelu(x).abs())
    for D in L2_D:
        for rows in (1, 5):
            x = _l2_x(1600 + D, rows, D)
            x32 = x.to(torch.float32)
            note("l2norm", x32 * (1.0 / torch.sqrt((x32 * x32).sum(-1, keepdim=True))), l2norm(x), l2norm(x).abs())
            x = _l2_x(1700 + D, rows, D)
            dy = f32v(plant(rnd(1800 + D, rows, D), [0.0, -0.0, 8.0, -8.0]))
            x32, d32 = x.to(torch.float32), dy.to(torch.float32)
            inv = 1.0 / torch.sqrt((x32 * x32).sum(-1, keepdim=True))
            ref, M = l2norm_bwd(x, dy, parts=True)
            note("l2norm_bwd", (d32 - x32 * ((x32 * d32).sum(-1, keepdim=True) * inv * inv)) * inv, ref, M)
    return out
