"""CPU: the fp64 references of tests/grad_split_ref.py against torch autograd in double -- the closed-form attention backward
that the split-bf16 kernel follows, and the tower gradient helper (closed-form cosine gradient pulled back through the double
oracle) against the loss differentiated end to end.  tests/test_gpu_grad_split.py judges the kernels with these."""
import pytest
import torch

import grad_split_ref as R


@pytest.mark.parametrize("T,heads,n_seq", [(17, 3, 2), (1, 2, 3)])
def test_attention_backward_formula_equals_autograd(T, heads, n_seq):
    g0 = torch.Generator().manual_seed(T)
    qkv = torch.randn(n_seq * T, 3 * heads * 64, generator=g0, dtype=torch.float64) * 0.7
    dout = torch.randn(n_seq * T, heads * 64, generator=g0, dtype=torch.float64)
    got, want = R.attention_backward64(qkv, dout, heads, n_seq, T), R.attention_autograd64(qkv, dout, heads, n_seq, T)
    assert got.shape == want.shape == qkv.shape
    assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    if T == 1:                                      # one key: P = 1, dS = dP - dO . O = 0 up to the dot product's rounding, dV = dO
        W = heads * 64
        assert got[:, :2 * W].abs().max().item() <= 1e-14 and torch.equal(got[:, 2 * W:], dout)


def test_operands_are_hi_plus_lo():
    x = torch.randn(1000, generator=torch.Generator().manual_seed(0)) * 3
    o = R.operands(x)
    assert o.dtype == torch.float64 and ((o - x.double()).abs() <= x.double().abs() * 2.0 ** -16).all()
    assert torch.equal(R.operands(x.bfloat16().float()), x.bfloat16().double())


@pytest.mark.parametrize("normalize", [False, True])
def test_tower_gradient_helper_equals_autograd_through_the_double_oracle(pkg, normalize):
    arch = pkg.get_arch("ViT-T/16-test")
    vw, _ = pkg.synth.make_clip_weights(arch, seed=0)
    x = pkg.synth.make_images(2, arch.image_size, seed=1)
    t = torch.randn(arch.embed_dim, generator=torch.Generator().manual_seed(2))
    f, g, gp = R.tower_grad64(vw, x, t, arch.vision.heads, arch.patch, normalize)
    want = R.tower_grad64_autograd(vw, x, t, arch.vision.heads, arch.patch, normalize)
    assert f.dtype == g.dtype == gp.dtype == torch.float64 and gp.shape == x.shape and g.shape == (2, arch.embed_dim)
    assert want.abs().max().item() > 0
    assert (gp - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    if normalize:                                   # unit rows: the cosine gradient is tangent to the sphere
        assert (g * f).sum(-1).abs().max().item() < 1e-12
