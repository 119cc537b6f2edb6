"""GPU: the VALUES of the image preprocessing (``tvc_preprocess_images``: resize_norm_kernel of csrc/sd_ops.hip -- antialiased
bilinear / bicubic resize, centre crop, (x - mean) / std) element by element against fp64, on the cases of tests/resize_ref.py.

Every output element must be finite and within the bound of ``resize_ref.reference`` (derived from the kernel's arithmetic;
DESIGN.md, "Image preprocessing: values"); no element is left out.  The witnesses add equalities: identity resizes return the
input's bits, the 2x bilinear shrink of small integers is exact, a constant image stays constant to one rounding per tap, an
impulse appears nowhere outside its taps.  tests/test_resize_ref.py shows on the CPU that the reference agrees with Pillow and
torch, that a correct fp32 kernel meets the bound on exactly these cases and that each of ten one-line defects does not.

The kernel is called through ctypes on buffers with guards: the images lie inside a NaN-filled allocation (a read outside
them makes the output non-finite), the output inside a sentinel-filled one (every sentinel outside [n, 3, S, S] must survive);
both start at an odd multiple of four bytes.  Every test prints ``[measured]`` lines: the worst |got - ref| / bound (allowed 1)."""
import ctypes as C

import numpy as np
import pytest
import torch

import resize_ref as R

pytestmark = pytest.mark.gpu

CASES = {c.id: c for c in R.gpu_cases()}
GUARD = 1021                            # floats before and after each buffer
SENT32 = 0x7FA5A5A5                     # a NaN bit pattern
TVC_E_INVALID = 1


def _floats(v):
    return None if v is None else (C.c_float * 3)(*v)


def _call(eng, x, S, filt, keep_aspect, mean, std, n=None, H=None, W=None, images=True):
    """One call on guarded buffers: x fp32 numpy [n, 3, H, W] -> (rc, the output [n, 3, S, S] on the CPU, sentinels intact?).
    ``n`` / ``H`` / ``W`` override what is passed (the refusals); the buffers keep the sizes of ``x`` and ``S`` (at least 1)."""
    dev = eng.device
    xin = torch.full((GUARD + x.size + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    xin[GUARD:GUARD + x.size] = torch.from_numpy(x.reshape(-1).copy()).to(dev)
    numel = x.shape[0] * 3 * max(S, 1) ** 2
    buf = torch.full((GUARD + numel + GUARD,), SENT32, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = eng.lib.tvc_preprocess_images(eng.handle, C.c_void_p(xin.data_ptr() + 4 * GUARD if images else None),
                                           x.shape[0] if n is None else n, x.shape[2] if H is None else H,
                                           x.shape[3] if W is None else W, S, filt, int(keep_aspect), _floats(mean), _floats(std),
                                           C.c_void_p(buf.data_ptr() + 4 * GUARD), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    host = buf.cpu()
    written = numel if (rc == 0 and (n is None or n > 0)) else 0
    intact = bool((host[:GUARD] == SENT32).all() and (host[GUARD + written:] == SENT32).all())
    out = host[GUARD:GUARD + numel].view(torch.float32).numpy().reshape(x.shape[0], 3, max(S, 1), max(S, 1))
    return rc, out, intact


def _run(eng, c):
    x = c.inputs()
    rc, got, intact = _call(eng, x, c.S, int(c.cubic), c.keep_aspect, *c.mean_std)
    assert rc == 0, (c.id, rc)
    assert intact, f"{c.id}: a write outside the output [n, 3, S, S]"
    return x, got


def _check(c, x, got):
    ref, bound = c.reference()
    assert got.shape == ref.shape and got.dtype == np.float32
    bad = ~np.isfinite(got)
    assert not bad.any(), f"{c.id}: {int(bad.sum())} non-finite outputs (a read outside the images?), first at {tuple(np.argwhere(bad)[0])}"
    ratio, (i, ch, y, xx), over = R.worst(got, ref, bound)
    assert over == 0, (f"{c.id}: |got - ref| / bound = {ratio:.3f} at image {i} ({c.images[i]}) channel {ch} y {y} x {xx}: got "
                       f"{got[i, ch, y, xx]!r}, ref {ref[i, ch, y, xx]!r}, bound {bound[i, ch, y, xx]:.3e}; {over} of {got.size} elements over")
    R.check_witnesses(c, x, got, ref, bound)
    return ratio


@pytest.mark.parametrize("case", list(CASES))
def test_preprocess_values(gpu_engine, case):
    c = CASES[case]
    x, got = _run(gpu_engine, c)
    ratio = _check(c, x, got)
    Hr, Wr, oy, ox = R.resized_size(c.H, c.W, c.S, c.keep_aspect)
    print(f"[measured] preprocess values {c.id} n={len(x)} resized {Hr}x{Wr} crop ({oy}, {ox}): worst |got - ref| / bound {ratio:.3f}")


def test_preprocess_is_deterministic(gpu_engine):
    c = CASES["values-300x420-S224-cubic-crop"]
    x, one = _run(gpu_engine, c)
    _, two = _run(gpu_engine, c)
    ratio = _check(c, x, one)
    assert np.array_equal(one.view(np.int32), two.view(np.int32)), f"{c.id}: two runs differ"
    print(f"[measured] preprocess values determinism: worst |got - ref| / bound {ratio:.3f} ({c.id})")


def test_preprocess_of_no_images_writes_nothing(gpu_engine):
    x = CASES["values-7x5-S32-cubic-crop"].inputs()
    for images in (True, False):                                      # n = 0 needs no image pointer
        rc, out, intact = _call(gpu_engine, x, 32, 1, True, R.CLIP_MEAN, R.CLIP_STD, n=0, images=images)
        assert rc == 0 and intact and (out.view(np.int32) == SENT32).all()


@pytest.mark.parametrize("what,kw", [("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("S = 0", dict(S=0)), ("filter = 2", dict(filt=2)),
                                     ("filter = -1", dict(filt=-1)), ("n = -1", dict(n=-1)), ("NULL mean", dict(mean=None)),
                                     ("NULL std", dict(std=None)), ("NULL images", dict(images=False))])
def test_preprocess_refusals_touch_nothing(gpu_engine, what, kw):
    x = CASES["values-7x5-S32-cubic-crop"].inputs()
    args = dict(S=32, filt=1, keep_aspect=True, mean=R.CLIP_MEAN, std=R.CLIP_STD)
    args.update(kw)
    rc, out, intact = _call(gpu_engine, x, **args)
    assert rc == TVC_E_INVALID, (what, rc)
    assert intact and (out.view(np.int32) == SENT32).all(), f"{what}: refused, yet the output was written"
    # the engine still works after a refusal
    rc, out, intact = _call(gpu_engine, x, 32, 1, True, R.CLIP_MEAN, R.CLIP_STD)
    assert rc == 0 and intact and np.isfinite(out).all()


def test_sd_resize_norm_refusals_are_unreachable_through_the_entry_point(gpu_engine):
    """sd_resize_norm refuses a resized side below S and a crop outside the resized image; tvc_preprocess_images derives both
    from (H, W, S) by the size rule, so every accepted call meets them: the shapes where the rule is tightest run clean."""
    for H, W, S, keep in ((1, 1000, 3, True), (1000, 1, 3, True), (3, 2, 2, True), (2, 5, 1, True), (5, 4, 7, False)):
        assert min(R.resized_size(H, W, S, keep)[:2]) >= S
        x = np.full((1, 3, H, W), 0.25, dtype=np.float32)
        for filt in (0, 1):
            rc, out, intact = _call(gpu_engine, x, S, filt, keep, R.UNIT_MEAN, R.UNIT_STD)
            ref, bound = R.reference(x, S, bool(filt), keep, R.UNIT_MEAN, R.UNIT_STD)
            assert rc == 0 and intact and R.worst(out, ref, bound)[2] == 0, (H, W, S, keep, filt, rc)


def test_clip_preprocess_tensor_is_the_bicubic_crop_form(pkg, gpu_engine):
    """``CLIPModel.preprocess_tensor`` = bicubic, short side to image_size, centre crop, CLIP constants."""
    clip = pkg.CLIPModel.__new__(pkg.CLIPModel)                       # the method reads the engine, the device and the size only
    clip.engine, clip.device, clip.arch = gpu_engine, gpu_engine.device, pkg.get_arch("ViT-L/14")
    S = clip.arch.image_size
    x = np.stack([R.image(name, 150, 100, np.random.default_rng(5)) for name in ("smooth", "noise")])
    got = clip.preprocess_tensor(torch.from_numpy(x)).cpu().numpy()
    ref, bound = R.reference(x, S, True, True, pkg.clip.CLIP_MEAN, pkg.clip.CLIP_STD)
    ratio, at, over = R.worst(got, ref, bound)
    print(f"[measured] CLIPModel.preprocess_tensor 150x100 -> {S}: worst |got - ref| / bound {ratio:.3f}")
    assert got.shape == ref.shape and np.isfinite(got).all() and over == 0, (ratio, at, over)
    assert (pkg.clip.CLIP_MEAN, pkg.clip.CLIP_STD) == (R.CLIP_MEAN, R.CLIP_STD)


def test_generative_reference_transform_is_the_bilinear_full_form(pkg, gpu_engine):
    """The transform of sd_ref.py's ``GenerativeReferenceGenerator`` = bilinear, both sides to 224, ImageNet constants
    (``SDReferenceGenerator`` itself goes through ``CLIPModel.preprocess_tensor``, the test above)."""
    class _Clip:
        engine = gpu_engine
    gen = pkg.GenerativeReferenceGenerator(None, _Clip())
    x = np.stack([R.image(name, 96, 160, np.random.default_rng(6)) for name in ("smooth", "noise")])
    got = gen._to_clip_tensor(torch.from_numpy(x).to(gpu_engine.device)).cpu().numpy()
    ref, bound = R.reference(x, 224, False, False, R.IMAGENET_MEAN, R.IMAGENET_STD)
    ratio, at, over = R.worst(got, ref, bound)
    print(f"[measured] GenerativeReferenceGenerator transform 96x160 -> 224: worst |got - ref| / bound {ratio:.3f}")
    assert got.shape == ref.shape and np.isfinite(got).all() and over == 0, (ratio, at, over)
    assert (gen.IMAGENET_MEAN, gen.IMAGENET_STD) == (R.IMAGENET_MEAN, R.IMAGENET_STD)
