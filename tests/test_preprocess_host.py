"""CPU: the host path ``CLIPModel.preprocess`` (Pillow, 8-bit pixels, two passes) against the fp64 reference of the device
path (tests/resize_ref.py) applied to the same 8-bit values -- same size rule (include/tvc.h), same taps, same crop.

On smooth images whose fp64 resample stays inside [0, 255] (so that Pillow's clipping never acts) the two differ by Pillow's
two roundings only: half an LSB after the horizontal pass, carried through the vertical pass's sum of |weights| <= 1.25, and
half an LSB after the vertical pass: <= 1.125 LSB; allowed 2 LSB = 2 / 255 / std.  Measured: 0.97 .. 1.07 LSB on the four shapes.
449 x 448 is the shape where Python's ``round`` (half to even: 224 rows) and the rule (half up: 225 rows) part; with ``round``
the host path was 5.7 LSB away there on this gentle image."""
import numpy as np
import pytest
from PIL import Image

import resize_ref as R


def _smooth_u8(H, W):
    """uint8 [H, W, 3]: low-frequency sinusoids with 40 levels of head room for the bicubic's overshoot."""
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    v = np.stack([128 + a * np.sin(2 * np.pi * (fx * i / W + fy * j / H) + ph)
                  for a, fx, fy, ph in ((85.0, 1.0, 2.0, 0.3), (60.0, 3.0, 1.0, 1.1), (30.0, 2.0, 4.0, 2.0))], axis=-1)
    return np.rint(v).astype(np.uint8)


@pytest.mark.parametrize("H,W", [(512, 512), (300, 420), (150, 100), (449, 448)])
def test_host_preprocess_matches_the_reference_on_8_bit_pixels(pkg, H, W):
    clip = pkg.CLIPModel.__new__(pkg.CLIPModel)                       # ``preprocess`` reads the image size only
    clip.arch = pkg.get_arch("ViT-L/14")
    S = clip.arch.image_size
    u8 = _smooth_u8(H, W)
    x = np.ascontiguousarray(u8.transpose(2, 0, 1)[None], dtype=np.float32)                    # 0 .. 255, exact
    r255, _ = R.reference(x, S, True, True, R.UNIT_MEAN, R.UNIT_STD)
    assert r255.min() >= 0 and r255.max() <= 255, (r255.min(), r255.max())
    m, s = (np.asarray(v, dtype=np.float64).reshape(1, 3, 1, 1) for v in (pkg.clip.CLIP_MEAN, pkg.clip.CLIP_STD))
    ref = (r255 / 255 - m) / s
    got = clip.preprocess(Image.fromarray(u8)).numpy()[None].astype(np.float64)
    assert got.shape == ref.shape == (1, 3, S, S)
    lsb = (np.abs(got - ref) * s * 255).max()
    print(f"[measured] CLIPModel.preprocess {H}x{W} -> {S} (resized {R.resized_size(H, W, S, True)[:2]}): {lsb:.3f} LSB from the fp64 rule")
    assert (np.abs(got - ref) <= 2 / 255 / s).all(), (H, W, lsb)
