"""CPU-only witness of the latent-diffusion convolutions (csrc/tvc_sd.cpp: Run::conv3x3_planes, Run::conv3x3,
Run::upsample_conv behind tvc_sd_block kinds 3 / 4 / 5): numpy and torch on the CPU, never the package's GPU side.

* ``CASES`` / ``LABELS``: the shapes tests/test_gpu_sd_conv_witness.py runs and the GEMM form each reaches in each
  process (tests/test_gemm_form.py checks the labels against csrc/host_plan.hpp on the CPU).
* ``make_case``: EXACT data.  Inputs are integers in [-3, 3], weights are zero except for a few entries of {+-1, +-2} per
  output channel, the bias holds integers in [-8, 8]: every product is exact in bf16 and in fp16, every fp32 partial sum
  is an integer far below 2^24 in any order, every output is an integer of |v| <= 256 and so survives the 16-bit store.
  Every launch form and every K split must then return the bits of the fp64 ``conv2d``.
* ``planes_model``: the address arithmetic of tvc_sd.cpp restated in numpy -- padded token layout, the nine plane
  offsets and the W + 3 output shift, sd_relayout's upsampling map, sd_im2col3x3's rows, the tap-major weight columns,
  a K loop cut into S slices of whole K-tiles -- with single-line ``defect``s.  tests/test_sd_conv_witness.py proves
  that the model equals the reference and that every defect changes an output integer of the witness data.
* ``make_resnet_case`` / ``resnet_ref``: the small non-square resnet blocks and their fp64 restatement, with the defect
  "GroupNorm statistics over the padded grid".

Entries per output channel: the issue that asked for this module capped them at 12 and also asked that each of the
9 * Cin weight columns be nonzero in some channel.  Where 12 * Cout < 9 * Cin + the K-tile edge columns (cases B, G, I)
both cannot hold; the count is then the smallest that covers every column, and never above 41, the largest for which
41 * 2 * 3 + 8 <= 256 still follows by construction.  The exactness itself is asserted on the data, not on the count.
"""
import numpy as np
import torch

F = torch.nn.functional

# id -> (kind, n, Cin, Cout, H, W)
CASES = {
    "A": (3, 3, 64, 64, 5, 7),        # one-tile kernel, 9 planes, non-square, three samples
    "B": (3, 2, 128, 64, 4, 4),       # fixed split S = 3 in the ring-split kernel
    "C": (3, 2, 256, 320, 8, 8),      # fixed split S = 9, slices 4 K-tiles deep (the minimum), ragged I
    "D": (3, 3, 64, 320, 16, 20),     # ring form 4 on 10 tiles, ragged I through a_rows_padded, ragged J
    "E": (4, 2, 64, 64, 6, 10),       # im2col stride 2, one tile
    "F": (4, 2, 64, 64, 5, 7),        # odd H and W: Ho, Wo = 3, 4
    "G": (4, 2, 256, 64, 8, 8),       # fixed split S = 9 on the one-plane K = 2304
    "H": (5, 2, 64, 64, 3, 5),        # upsample and planes, one tile
    "I": (5, 2, 128, 72, 2, 2),       # upsample with fixed split S = 3, Cout not a multiple of 16
    "J": (5, 3, 64, 320, 8, 10),      # upsample with ring form 4
}
SEEDS = {cid: 100 + i for i, cid in enumerate(CASES)}
ENVS = ("", "TVC_GEMM_RING_SPLIT=0", "TVC_GEMM_RING_FORM=1")
# id -> env -> (form, S, slices in the ring kernel); a case runs in the default process and in every child it is labelled for
LABELS = {
    "A": {"": ("ONE_TILE", 0, 0)},
    "B": {"": ("SPLITK_FIXED", 3, 1), "TVC_GEMM_RING_SPLIT=0": ("SPLITK_FIXED", 3, 0)},
    "C": {"": ("SPLITK_FIXED", 9, 1), "TVC_GEMM_RING_SPLIT=0": ("SPLITK_FIXED", 9, 0)},
    "D": {"": ("RING4", 0, 0), "TVC_GEMM_RING_FORM=1": ("RING1", 0, 0)},
    "E": {"": ("ONE_TILE", 0, 0)},
    "F": {"": ("ONE_TILE", 0, 0)},
    "G": {"": ("SPLITK_FIXED", 9, 1), "TVC_GEMM_RING_SPLIT=0": ("SPLITK_FIXED", 9, 0)},
    "H": {"": ("ONE_TILE", 0, 0)},
    "I": {"": ("SPLITK_FIXED", 3, 1), "TVC_GEMM_RING_SPLIT=0": ("SPLITK_FIXED", 3, 0)},
    "J": {"": ("RING4", 0, 0), "TVC_GEMM_RING_FORM=1": ("RING1", 0, 0)},
}
# the resnet blocks: (n, Cin, Cout, H, W); conv1 of the second one splits K three ways
RESNET_SHAPES = ((3, 64, 64, 3, 5), (2, 128, 64, 5, 7))
GROUPS = 32
RESNET_EPS = 1e-5                     # SDArch().norm_eps (the GPU test asserts it); the VAE's blocks use 1e-6
# (rel L2, max |d| / std) bounds of the resnet blocks against resnet_ref, per 16-bit format: 2x the largest deviation measured on
# the GPU over both shapes and both eps (EXPERIMENTS.md: bf16 3.02e-3 / 1.93e-2, fp16 3.81e-4 / 2.04e-3) -- the project's margin
# for 16-bit activations against a high-precision reference --, and never above the 8e-3 / 6e-2 of tests/test_gpu_sd.py
RESNET_BOUND = {"bf16": (6.1e-3, 3.9e-2), "fp16": (7.7e-4, 4.1e-3)}
MAX_ENTRIES = 41                      # 41 entries * |w| 2 * |x| 3 + |bias| 8 = 254 <= 256


def gemm_shape(kind, n, Cin, Cout, H, W):
    """The GEMM tvc_sd.cpp launches for a case: I, J, K per plane, planes, lda, ldb, B rows of one sample."""
    if kind == 4:
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        return dict(I=Cout, J=n * Ho * Wo, K=9 * Cin, planes=1, lda=9 * Cin, ldb=9 * Cin, rows_per_sample=Ho * Wo)
    if kind == 5:
        H, W = 2 * H, 2 * W
    Wp = W + 2
    rows = n * (H + 2) * Wp
    return dict(I=Cout, J=rows - 2 * (Wp + 1), K=Cin, planes=9, lda=9 * Cin, ldb=Cin, rows_per_sample=(H + 2) * Wp)


def conv3x3_rows(w):
    """[Co, Ci, 3, 3] -> [Co, 9 * Ci], column (ky * 3 + kx) * Ci + ci (sd_model._conv3x3_rows, restated)."""
    w = np.asarray(w)
    return np.ascontiguousarray(w.transpose(0, 2, 3, 1)).reshape(w.shape[0], -1)


def reference(x, w, bias, kind):
    """fp64 conv2d: kind 3 padding 1, kind 4 stride 2 + padding 1, kind 5 on the nearest-2x upsampling."""
    xs = x.double()
    if kind == 5:
        xs = F.interpolate(xs, scale_factor=2.0, mode="nearest")
    return F.conv2d(xs, w.double(), bias.double(), stride=2 if kind == 4 else 1, padding=1)


def entries_per_channel(Cin, Cout):
    need = 9 * Cin + 2 * (9 * Cin // 64)          # every column once, the K-tile edge columns twice
    return max(12, -(-need // Cout))


def make_case(kind, n, Cin, Cout, H, W, seed):
    """-> dict(x fp32 [n, Cin, H, W], w fp32 [Cout, Cin, 3, 3], bias fp32 [Cout], ref fp64 NCHW); asserts both rules."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, size=(n, Cin, H, W))
    for s in range(n - 1):
        if np.array_equal(x[s], x[s + 1]):
            x[s + 1, 0, 0, 0] = -x[s + 1, 0, 0, 0] if x[s + 1, 0, 0, 0] else 1
    ncol = 9 * Cin
    rows = np.zeros((Cout, ncol), dtype=np.int64)
    val = lambda: int(rng.choice((-2, -1, 1, 2)))
    first = np.empty(ncol, dtype=np.int64)
    for i, col in enumerate(rng.permutation(ncol)):              # every column, round-robin over the output channels
        o = i % Cout
        rows[o, col] = val()
        first[col] = o
    ngroups = Cout // 16                                         # whole 16-row groups
    for col in range(ncol):                                      # K-tile edges: a second channel in another 16-row group
        if col % 64 in (0, 63):
            g1 = first[col] // 16
            cand = [o for o in range(16 * ngroups) if o // 16 != g1]
            load = (rows[cand] != 0).sum(1)
            o2 = cand[int(rng.choice(np.nonzero(load == load.min())[0]))]      # the emptiest channel of another group
            assert rows[o2, col] == 0 and o2 // 16 != g1
            rows[o2, col] = val()
    bias = rng.integers(-8, 9, size=Cout)
    if Cout > 256:                                               # the two row tiles' bias values differ, element by element
        lo, hi = bias[:Cout - 256], bias[256:]
        hi[hi == lo] += np.where(lo[hi == lo] < 8, 1, -1)
    w = rows.reshape(Cout, 3, 3, Cin).transpose(0, 3, 1, 2)      # column (ky * 3 + kx) * Cin + ci
    case = dict(kind=kind, x=torch.from_numpy(x.astype(np.float32)), w=torch.from_numpy(np.ascontiguousarray(w).astype(np.float32)),
                bias=torch.from_numpy(bias.astype(np.float32)))
    case["ref"] = reference(case["x"], case["w"], case["bias"], kind)
    check_rules(case)
    return case


def check_rules(case):
    """The exactness rule and the coverage rule of the module docstring, asserted on the data."""
    x, w, bias, ref = case["x"].numpy(), case["w"].numpy(), case["bias"].numpy(), case["ref"]
    Cout, Cin = w.shape[:2]
    rows = conv3x3_rows(w)
    # ---- exactness
    assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 3
    assert set(np.unique(rows)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    per = (rows != 0).sum(1)
    assert per.max() <= entries_per_channel(Cin, Cout) + 1 and per.max() <= MAX_ENTRIES, per.max()
    assert np.array_equal(bias, np.round(bias)) and np.abs(bias).max() <= 8
    assert 3.0 * np.abs(rows).sum(1).max() + 8 < 2 ** 24          # any partial sum, in any order
    assert torch.equal(ref, ref.round()) and ref.abs().max().item() <= 256
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(ref.to(dt).double(), ref)
        assert torch.equal(case["x"].to(dt).float(), case["x"]) and torch.equal(case["w"].to(dt).float(), case["w"])
    # ---- coverage
    assert ((rows != 0).sum(0) >= 1).all()                       # every one of the 9 * Cin columns
    for col in range(9 * Cin):
        if col % 64 in (0, 63):                                  # K-tile edges: two channels in different 16-row groups
            assert len({int(o) // 16 for o in np.nonzero(rows[:, col])[0]}) >= 2, col
    if Cout > 256:
        assert (rows[:256] != 0).any() and (rows[256:] != 0).any()
        assert (bias[256:] != bias[:Cout - 256]).all()
    for s in range(x.shape[0] - 1):
        assert not np.array_equal(x[s], x[s + 1])


# ---------------------------------------------------------------------------------------------------- the model
# defect -> the kinds whose code holds the faulted line
DEFECTS = {
    "tap_shift_w": (3, 5),                 # tap (ky, kx) shifts by ky * W + kx
    "tap_shift_w1": (3, 5),                # ... by ky * (W + 1) + kx
    "tap_ky_kx_swapped": (3, 4, 5),
    "out_shift_w2": (3, 5),                # the output lands W + 2 rows on, not W + 3
    "hw_swapped_conv": (3,),               # conv3x3_planes takes the padded width from H
    "hw_swapped_up": (5,),                 # ... behind upsample_conv
    "hw_swapped_im2col": (4,),             # sd_im2col3x3 addresses pixel (y, x) as y * H + x
    "border_reads_neighbour": (3, 4, 5),   # a border row / an out-of-image tap holds the nearest pixel, not zero
    "last_ktile_dropped": (3, 4, 5),       # the K loop of a plane ends one K-tile early
    "slice_boundary_off_by_one": (3, 4, 5),
    "slice_summed_twice": (3, 4, 5),
    "plane_not_advanced": (3, 5),          # B keeps plane 0's offset and runs on along the row
    "stride2_phase_1": (4,),
    "upsample_round_up": (5,),             # source pixel (y + 1) // 2
    "bias_second_row_tile": (3, 4, 5),     # row tile r > 0 reads the bias of row tile 0
    "weight_cols_ci_major": (3, 4, 5),     # weight column ci * 9 + tap
}
SLICE_DEFECTS = ("slice_boundary_off_by_one", "slice_summed_twice")


def _gemm(B, ldb, A, J, K, planes, a_off, b_off, bias, S, row_tile, defect):
    """out[j, i] = sum over the planes' K-tiles of B[j, b_off[t] + k] * A[i, a_off[t] + k] + bias[i]: flat addresses into B
    (a tap that runs off a row reads what lies there), virtual K-tiles v = t * (K / 64) + kt cut into S slices, partial
    sums per slice, then the finish."""
    I = A.shape[0]
    kpp = K // 64
    nk = kpp * planes
    assert K % 64 == 0 and nk % S == 0
    depth = nk // S
    Bf = B.reshape(-1)
    j0 = np.arange(J)[:, None] * ldb + np.arange(64)[None, :]
    part = np.zeros((S, J, I))
    for s in range(S):
        lo, hi = s * depth, (s + 1) * depth
        if defect == "slice_boundary_off_by_one" and s > 0:
            lo += 1
        for v in range(lo, hi):
            t, kt = divmod(v, kpp)
            if defect == "last_ktile_dropped" and kt == kpp - 1:
                continue
            bcol = b_off[0] + v * 64 if defect == "plane_not_advanced" else b_off[t] + kt * 64
            part[s] += Bf[j0 + bcol] @ A[:, a_off[t] + kt * 64: a_off[t] + kt * 64 + 64].T
    acc = part.sum(0)
    if defect == "slice_summed_twice":
        acc += part[S - 1]
    i = np.arange(I)
    return acc + bias[i % row_tile if defect == "bias_second_row_tile" else i][None, :]


def planes_model(x, w_rows, bias, kind, defect=None, S=1, row_tile=256):
    """tvc_sd_block kinds 3 / 4 / 5 on x [n, Cin, H, W], the tap-major weight rows [Cout, 9 * Cin] and the bias -> fp64 NCHW."""
    x, A, bias = np.asarray(x, dtype=np.float64), np.asarray(w_rows, dtype=np.float64), np.asarray(bias, dtype=np.float64)
    n, Cin, H, W = x.shape
    Cout = A.shape[0]
    assert defect is None or kind in DEFECTS[defect], (defect, kind)
    if defect == "weight_cols_ci_major":
        A = A.reshape(Cout, 9, Cin).transpose(0, 2, 1).reshape(Cout, 9 * Cin)
    tok = x.transpose(0, 2, 3, 1).reshape(n * H * W, Cin)                       # sd_nchw_to_tokens: dense rows, pixel y * W + x
    tokf = np.concatenate([tok, np.zeros((4 * (H + W) + 8, Cin))])              # (what a faulted address finds past the end)
    clamp = defect == "border_reads_neighbour"
    if kind == 4:
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        col = np.zeros((n * Ho * Wo, 9 * Cin))
        pitch = H if defect == "hw_swapped_im2col" else W
        for img in range(n):
            for yo in range(Ho):
                for xo in range(Wo):
                    for tap in range(9):
                        ky, kx = (tap % 3, tap // 3) if defect == "tap_ky_kx_swapped" else (tap // 3, tap % 3)
                        p = 1 if defect == "stride2_phase_1" else 0
                        yy, xx = 2 * yo + p + ky - 1, 2 * xo + p + kx - 1
                        if clamp:
                            yy, xx = min(max(yy, 0), H - 1), min(max(xx, 0), W - 1)
                        if 0 <= yy < H and 0 <= xx < W:
                            col[(img * Ho + yo) * Wo + xo, tap * Cin:(tap + 1) * Cin] = tokf[img * H * W + yy * pitch + xx]
        out = _gemm(col, 9 * Cin, A, n * Ho * Wo, 9 * Cin, 1, [0], [0], bias, S, row_tile, defect)
        return out.reshape(n, Ho, Wo, Cout).transpose(0, 3, 1, 2)
    # kinds 3 and 5: the padded layout, (Hs + 2) x (Ws + 2) rows per image with zero borders (sd_relayout)
    up = kind == 5
    Hs, Ws = (2 * H, 2 * W) if up else (H, W)
    Wp = Ws + 2
    P = n * (Hs + 2) * Wp
    pad = np.zeros((P + 4 * (Hs + Ws) + 16, Cin))
    for img in range(n):
        for yp in range(Hs + 2):
            for xp in range(Wp):
                yy, xx = yp - 1, xp - 1
                if clamp:
                    yy, xx = min(max(yy, 0), Hs - 1), min(max(xx, 0), Ws - 1)
                if 0 <= yy < Hs and 0 <= xx < Ws:
                    if up:
                        ys, xs = ((yy + 1) // 2, (xx + 1) // 2) if defect == "upsample_round_up" else (yy >> 1, xx >> 1)
                    else:
                        ys, xs = yy, xx
                    pad[(img * (Hs + 2) + yp) * Wp + xp] = tokf[img * H * W + ys * W + xs]
    Wg = Hs + 2 if defect in ("hw_swapped_conv", "hw_swapped_up") else Wp       # the padded width as the GEMM's caller sees it
    Wt = {"tap_shift_w": Wg - 2, "tap_shift_w1": Wg - 1}.get(defect, Wg)
    b_off = []
    for t in range(9):
        ky, kx = (t % 3, t // 3) if defect == "tap_ky_kx_swapped" else (t // 3, t % 3)
        b_off.append((ky * Wt + kx) * Cin)
    J = P - 2 * (Wg + 1)
    out = _gemm(pad, Cin, A, J, Cin, 9, [t * Cin for t in range(9)], b_off, bias, S, row_tile, defect)
    shift = Wg if defect == "out_shift_w2" else Wg + 1
    outp = np.zeros((pad.shape[0], Cout))
    outp[shift:shift + J] = out
    y = outp[:P].reshape(n, Hs + 2, Wp, Cout)[:, 1:Hs + 1, 1:Ws + 1]           # sd_relayout back to dense rows
    return y.transpose(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ resnet blocks
def make_resnet_case(n, Cin, Cout, H, W, seed):
    """Hand-made tensors of one ResnetBlock2D (state-dict names without the prefix) and its input.  The GEMM weights are
    exactly representable in bf16 and in fp16, so the only 16-bit roundings are the activations'."""
    g = torch.Generator().manual_seed(seed)
    def r16(t):          # bf16-rounded, and zero below fp16's normal range: exact in both formats
        t = t.to(torch.bfloat16).float()
        return torch.where(t.abs() < 2.0 ** -12, torch.zeros_like(t), t)
    t = {"norm1.weight": 1 + 0.2 * torch.randn(Cin, generator=g), "norm1.bias": 0.2 * torch.randn(Cin, generator=g),
         "conv1.weight": r16(torch.randn((Cout, Cin, 3, 3), generator=g) * (9 * Cin) ** -0.5),
         "conv1.bias": 0.5 + 0.2 * torch.randn(Cout, generator=g),
         "norm2.weight": 1 + 0.2 * torch.randn(Cout, generator=g), "norm2.bias": 0.2 * torch.randn(Cout, generator=g),
         "conv2.weight": r16(torch.randn((Cout, Cout, 3, 3), generator=g) * (9 * Cout) ** -0.5),
         "conv2.bias": 0.2 * torch.randn(Cout, generator=g)}
    if Cin != Cout:
        t["conv_shortcut.weight"] = r16(torch.randn((Cout, Cin, 1, 1), generator=g) * Cin ** -0.5)
        t["conv_shortcut.bias"] = 0.2 * torch.randn(Cout, generator=g)
    for k in [k for k in t if k.endswith("weight") and t[k].dim() == 4]:
        assert torch.equal(t[k].to(torch.float16).float(), t[k])
    x = torch.randn((n, Cin, H, W), generator=g)
    return t, x


def resnet_ref(t, x16, eps, padded_stats=False):
    """fp64 ResnetBlock2D without a time embedding on the 16-bit-rounded input ``x16`` and the fp32 tensors ``t``:
    x + conv2(silu(gn2(conv1(silu(gn1(x)))))), 1x1 shortcut where the widths differ.  ``padded_stats``: the defect
    "norm2 takes its statistics over the (H + 2) x (W + 2) padded grid", whose border rows hold what conv1's GEMM wrote
    there -- its windows centred outside the image."""
    d = {k: v.double() for k, v in t.items()}
    x = x16.double()
    h = F.silu(F.group_norm(x, GROUPS, d["norm1.weight"], d["norm1.bias"], eps))
    c1 = F.conv2d(h, d["conv1.weight"], d["conv1.bias"], padding=1)
    if padded_stats:
        n, C = c1.shape[:2]
        grid = F.conv2d(h, d["conv1.weight"], d["conv1.bias"], padding=2).reshape(n, GROUPS, -1)
        mean, var = grid.mean(-1), grid.var(-1, unbiased=False)
        hn = (c1.reshape(n, GROUPS, -1) - mean[..., None]) / (var[..., None] + eps).sqrt()
        h2 = hn.reshape(c1.shape) * d["norm2.weight"].view(1, C, 1, 1) + d["norm2.bias"].view(1, C, 1, 1)
    else:
        h2 = F.group_norm(c1, GROUPS, d["norm2.weight"], d["norm2.bias"], eps)
    c2 = F.conv2d(F.silu(h2), d["conv2.weight"], d["conv2.bias"], padding=1)
    sc = F.conv2d(x, d["conv_shortcut.weight"], d["conv_shortcut.bias"]) if "conv_shortcut.weight" in d else x
    return sc + c2


def rel(got, ref):
    """(relative L2 error, max |d| / std(ref)), as tests/test_gpu_sd.py measures."""
    d = got.double().cpu() - ref.double()
    return (d.norm() / ref.double().norm()).item(), (d.abs().max() / ref.double().std()).item()
