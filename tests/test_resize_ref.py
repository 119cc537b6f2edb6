"""CPU: everything tests/resize_ref.py states, before tests/test_gpu_preprocess_values.py relies on it.

* The reference is pinned twice from outside: Pillow's float (mode "F") resize and torch's antialiased interpolate, for the
  same size, crop and filter, on every GPU case.  Allowed 5e-7 and 3e-5 (about four times what the rule's author measured,
  1.2e-7 and 1.2e-5).  Measured here over all cases: Pillow <= 1.14e-7 on pixels in [0, 1] (2.9e-7 on the 0 .. 7 integers of
  shrink2); torch on fp64 pixels <= 1.8e-15.  torch on fp32 pixels -- printed, not asserted -- is <= 1.46e-5 on every case with
  sides up to 512 and 4.3e-5 .. 8.5e-5 on the four 2000 x 37 crop cases (2000 -> 3459 rows): its centres and taps are fp32
  there, one ulp of a coordinate near 2000 is 1.2e-4, and Pillow and torch's own fp64 path agree with the reference on the
  same cases.  So the 3e-5 is asserted against the fp64 path, which holds it on every case.
* ``resized_size`` against values computed by hand.
* ``emulate`` (the kernel's fp32 arithmetic) stays inside ``bound`` on every GPU case and meets every witness equality;
  measured worst |emulate - ref| / bound 0.48 (values-128x128-S224-linear-full, values-2000x37-S64-linear-crop).
* Every entry of ``DEFECTS`` leaves the bound on the GPU case ``DEFECT_CASE`` names for it.
* ``long_side_rounded_half_to_even`` passes the old criterion (max error < 2e-4 against torch on 512 x 512, 300 x 420,
  224 x 224 and 150 x 100 at S = 224, tests/test_gpu_sd.py): none of those four long sides ends in .5, so the defective size
  rule gives the very same bits there.  ``long_side_truncated`` does not pass it (300 x 420: 313.6 -> 313); it would pass only
  a test that copies the kernel's own formula, as the old one does.
"""
import numpy as np
import pytest
import torch
from PIL import Image

import resize_ref as R

CASES = {c.id: c for c in R.gpu_cases()}


def _resampled(c):
    """The reference before the mean / std step, fp64 [n, 3, S, S]."""
    ref, _ = c.reference()
    m, s = (np.asarray(v, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1) for v in c.mean_std)
    return ref * s + m


def test_cases_are_the_issue_s_list():
    ids = set(CASES)
    assert len(ids) == len(R.gpu_cases()) == 8 + 1 + 2 * 26 + 1
    for want in ("values-512x512-S224-cubic-crop", "values-512x512-S224-linear-full", "values-128x128-S224-cubic-crop",
                 "values-32x32-S64-linear-full", "values-300x420-S224-cubic-crop", "values-420x300-S224-linear-crop",
                 "values-449x448-S224-cubic-crop", "values-2000x37-S64-cubic-full", "values-2000x37-S64-linear-crop",
                 "values-7x5-S32-cubic-crop", "values-2x3-S8-linear-full", "values-1x1-S8-cubic-crop", "values-1x9-S8-cubic-crop",
                 "values-100x150-S7-linear-full", "grid-2x2-S224-linear-full", "shrink2-16x16-S8-linear-full",
                 "identity-33x33-S33-cubic-full"):
        assert want in ids, want
    assert all(c.S == 224 for c in R.gpu_cases() if (c.H, c.W) in ((512, 512), (2, 2)))
    g = R.GRID
    assert g.n * 3 * g.S * g.S == 16859136 > 65536 * 256 and len(g.images) == g.n
    for c in R.gpu_cases():                                           # finite, in [0, 1] unless stated, and not trivial
        x = c.inputs()
        assert x.dtype == np.float32 and x.shape == (len(c.images), 3, c.H, c.W) and np.isfinite(x).all()
        assert x.min() >= 0 and x.max() <= (7 if c.kind == "shrink2" else 1), c.id
    # every witness image the issue lists, and three channels with distinct means and spreads in the value images
    assert R.WITNESS_IMAGES == ("constant", "impulse_first", "impulse_last", "impulse_centre", "ramp_x", "ramp_y")
    smooth = CASES["values-512x512-S224-cubic-crop"].inputs()[0]
    assert len({round(float(v), 2) for v in smooth.mean((1, 2))}) == 3 and len({round(float(v), 2) for v in smooth.std((1, 2))}) == 3


def test_resized_size_by_hand():
    rs = R.resized_size
    assert rs(449, 448, 224, True) == (225, 224, 0, 0)               # 449 * 224 / 448 = 224.5 -> 225 (half up), offset 1 // 2
    assert rs(448, 449, 224, True) == (224, 225, 0, 0)
    assert rs(300, 420, 224, True) == (224, 314, 0, 45)              # 313.6 -> 314
    assert rs(420, 300, 224, True) == (314, 224, 45, 0)
    assert rs(150, 100, 224, True) == (336, 224, 56, 0)              # exact
    assert rs(224, 224, 224, True) == (224, 224, 0, 0)               # the long side is S already
    assert rs(100, 224, 100, True) == (100, 224, 0, 62)
    assert rs(2000, 37, 64, True) == (3459, 64, 1697, 0)             # 128000 / 37 = 3459.46
    assert rs(1, 9, 8, True) == (8, 72, 0, 32)
    assert rs(3, 5, 2, True) == (2, 3, 0, 0)                         # 10 / 3 = 3.33
    assert rs(5, 3, 2, True) == (3, 2, 0, 0)
    assert rs(2, 3, 1, True) == (1, 2, 0, 0)                         # 1.5 -> 2 (half up; half to even would give 2 as well)
    assert rs(2, 5, 1, True) == (1, 3, 0, 1)                         # 2.5 -> 3 (half to even: 2)
    assert rs(2000, 37, 64, False) == rs(1, 1, 64, False) == (64, 64, 0, 0)
    assert rs(2, 5, 1, True, "long_side_rounded_half_to_even")[:2] == (1, 2) and rs(2, 3, 1, True, "long_side_rounded_half_to_even")[:2] == (1, 2)
    assert rs(449, 448, 224, True, "long_side_rounded_half_to_even")[:2] == (224, 224)
    assert rs(300, 420, 224, True, "long_side_truncated")[:2] == (224, 313)
    # (resized - S) even: rounding the offset up changes nothing; odd: one pixel
    assert rs(300, 420, 224, True, "crop_offset_rounded_up")[2:] == (0, 45) and rs(449, 448, 224, True, "crop_offset_rounded_up")[2:] == (1, 0)


def test_weights_by_hand():
    w = R.weights(16, 8, 0, 8, False)                                 # the 2x bilinear shrink
    assert np.array_equal(w[3, 5:9], [0.125, 0.375, 0.375, 0.125]) and w[3].sum() == 1 and np.count_nonzero(w[3]) == 4
    assert np.allclose(w[0, :3], np.array([3, 3, 1]) / 7, rtol=0, atol=1e-16) and np.count_nonzero(w[0]) == 3
    for cubic in (False, True):                                       # identity: (.., 0, 1, 0, ..)
        assert np.array_equal(R.weights(33, 33, 0, 33, cubic), np.eye(33))
    w = R.weights(4, 8, 0, 8, True)                                   # 2x bicubic upscale, a = -0.5: the taps at +-0.25, +-0.75, ..
    k = lambda t: 1.5 * t ** 3 - 2.5 * t ** 2 + 1 if t < 1 else -0.5 * (t ** 3 - 5 * t ** 2 + 8 * t - 4)
    assert np.allclose(w[3], [k(1.25), k(0.25), k(0.75), k(1.75)], rtol=0, atol=1e-15)
    assert k(1.25) == -0.0703125 and abs(sum(k(t) for t in (1.25, 0.25, 0.75, 1.75)) - 1) < 1e-15
    w = R.weights(9, 72, 32, 8, True)                                 # offset: output 32 of 72 sits at 32.5 / 8 = 4.0625
    assert np.count_nonzero(w[0]) == 4 and w[0, 4] > w[0, 3] > 0 > w[0, 2] and w[0, 5] < 0
    assert np.allclose(R.weights(2000, 64, 0, 64, True).sum(1), 1, rtol=0, atol=1e-14)
    assert np.count_nonzero(R.weights(2000, 64, 0, 64, True)[30]) == 125


@pytest.mark.parametrize("case", list(CASES))
def test_reference_against_pillow_and_torch(case):
    c = CASES[case]
    x, r = c.inputs(), _resampled(c)
    Hr, Wr, oy, ox = R.resized_size(c.H, c.W, c.S, c.keep_aspect)
    n = min(len(x), 6)                                                # grid: the 112 images differ only in their noise
    flt = Image.BICUBIC if c.cubic else Image.BILINEAR
    pil = np.stack([[np.asarray(Image.fromarray(x[i, ch]).resize((Wr, Hr), flt))[oy:oy + c.S, ox:ox + c.S]
                     for ch in range(3)] for i in range(n)])
    tor64, tor32 = (torch.nn.functional.interpolate(torch.from_numpy(x[:n].copy()).to(dt), size=(Hr, Wr), mode="bicubic" if c.cubic else "bilinear",
                                                    antialias=True, align_corners=False)[:, :, oy:oy + c.S, ox:ox + c.S].numpy()
                    for dt in (torch.float64, torch.float32))
    dp, dt, d32 = np.abs(pil - r[:n]).max(), np.abs(tor64 - r[:n]).max(), np.abs(tor32 - r[:n]).max()
    print(f"[measured] {c.id}: reference vs Pillow F {dp:.2e}, vs torch antialias on fp64 pixels {dt:.2e} (on fp32 pixels {d32:.2e})")
    assert dp <= 5e-7 and dt <= 3e-5, (c.id, dp, dt)


@pytest.mark.parametrize("case", list(CASES))
def test_emulation_stays_inside_the_bound(case):
    c = CASES[case]
    x = c.inputs()
    ref, bound = c.reference()
    assert np.isfinite(ref).all() and np.isfinite(bound).all() and (bound >= 0).all()
    got = R.emulate(x, c.S, c.cubic, c.keep_aspect, *c.mean_std)
    assert np.isfinite(got).all()
    ratio, at, over = R.worst(got, ref, bound)
    print(f"[measured] {c.id}: worst |emulate - ref| / bound {ratio:.3f} at {at}, largest bound {bound.max():.2e}")
    assert over == 0 and ratio <= 1, (c.id, ratio, at, over)
    R.check_witnesses(c, x, got, ref, bound)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_defect_leaves_the_bound(defect):
    c = CASES[R.DEFECT_CASE[defect]]
    ref, bound = c.reference()
    got = R.emulate(c.inputs(), c.S, c.cubic, c.keep_aspect, *c.mean_std, defect=defect)
    ratio, at, over = R.worst(got, ref, bound)
    print(f"[measured] {defect} on {c.id}: worst |emulate - ref| / bound {ratio:.1f}, {over} of {got.size} elements over")
    assert ratio > 2 and over > 0, (defect, c.id, ratio)


def test_size_defects_are_invisible_where_no_long_side_ends_in_half():
    """The old criterion on the old shapes: the half-to-even size rule passes it, bit for bit."""
    g = torch.Generator().manual_seed(8)
    for H, W in ((512, 512), (300, 420), (224, 224), (150, 100)):
        x = torch.rand((2, 3, H, W), generator=g)
        Hr, Wr = (224, max(224, int(W * 224 / H + 0.5))) if H <= W else (max(224, int(H * 224 / W + 0.5)), 224)
        assert R.resized_size(H, W, 224, True)[:2] == (Hr, Wr)
        r = torch.nn.functional.interpolate(x, size=(Hr, Wr), mode="bicubic", antialias=True, align_corners=False)
        oy, ox = (Hr - 224) // 2, (Wr - 224) // 2
        ref = (r[:, :, oy:oy + 224, ox:ox + 224] - torch.tensor(R.CLIP_MEAN).view(1, 3, 1, 1)) / torch.tensor(R.CLIP_STD).view(1, 3, 1, 1)
        good = R.emulate(x.numpy(), 224, True, True, R.CLIP_MEAN, R.CLIP_STD)
        bad = R.emulate(x.numpy(), 224, True, True, R.CLIP_MEAN, R.CLIP_STD, defect="long_side_rounded_half_to_even")
        err = np.abs(bad - ref.numpy()).max()
        print(f"[measured] old criterion, half-to-even size rule, {H}x{W}: max error vs torch {err:.2e} (allowed 2e-4)")
        assert err < 2e-4 and np.array_equal(bad, good)
    # while on 449 x 448 it is a different image
    c = CASES["values-449x448-S224-cubic-crop"]
    bad = R.emulate(c.inputs(), c.S, True, True, *c.mean_std, defect="long_side_rounded_half_to_even")
    assert R.worst(bad, *c.reference())[0] > 100
