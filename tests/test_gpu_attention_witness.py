"""GPU: which keys a query sees, read back exactly from every forward attention kernel and every launch option.

Both witnesses of tests/attn_witness.py (visibility read-back: q = 0 and an indicator V, output exactly 0.0 where the
spec says invisible and 1 / n_i where visible; needle: +-1 codes, q = 8 k_target, the output decodes to the target or --
for a forbidden target -- equals the fp64 model that never sees it) run on every case:

* tower kernel (csrc/attention.hip), bf16 and fp16, through ``attention_ex``: every template of the launcher from both
  sides of its limit (causal NT <= 2 / <= 6 / 18; non-causal EXACT 17 / EXACT 4 dense and the general forms packed and
  dense), packed length mixes, heads = 3 with a spare item in the last workgroup, prefix groups, pool_mode 1 / 2;
* split kernel (csrc/split.hip) through ``attention_split_ex``: the same packed, causal and prefix cases up to 272 tokens;
* fp32 kernel (csrc/precise.hip): dense, causal and not;
* streaming kernel (csrc/sd_attention.hip): all twelve head dims, ragged query blocks and key tiles, the three workgroup
  shapes as the dispatcher chooses them by item count, separate row strides with guard columns.

Value bounds come from the storage formats (attn_witness.PRECISION / SD_REL), invisible entries are exactly zero.
tests/test_attention_witness.py proves on the CPU that these checks flag every defect of attn_witness.DEFECTS.
"""
import pytest
import torch

import attn_witness as W

pytestmark = pytest.mark.gpu

TOWER = {c.name: c for c in W.tower_configs()}
SPLIT = {c.name: c for c in W.split_configs()}
F32 = {c.name: c for c in W.f32_configs()}
GUARD = 2           # output rows after the last one, which no launch may touch


def _dev(t):
    return None if t is None else t.cuda()


def _tower_kernel(eng, cfg, f16):
    dt = torch.float16 if f16 else torch.bfloat16
    starts, pfx, pool_row = _dev(cfg.starts_tensor()), _dev(cfg.pfx_tensor()), _dev(cfg.pool_row_tensor())

    def kernel(qkv):
        buf = torch.full((cfg.n_out + GUARD, cfg.width), float("nan"), dtype=dt, device="cuda")      # an unwritten row stays NaN
        eng.attention_ex(qkv.to(dt).cuda(), cfg.n_seq, cfg.seq_len, cfg.heads, cfg.causal, starts=starts, pfx=pfx,
                         pool_mode=cfg.pool_mode, pool_row=pool_row, f16=f16, out=buf[:cfg.n_out])
        assert torch.isnan(buf[cfg.n_out:]).all(), f"{cfg.name}: rows past the output were written"
        return buf[:cfg.n_out].float().cpu()
    return kernel


@pytest.mark.parametrize("name", list(TOWER))
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_tower_attention_masks(gpu_engine, precision, name):
    cfg = TOWER[name]
    fails = W.check_both(_tower_kernel(gpu_engine, cfg, precision == "fp16"), cfg, precision)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", list(SPLIT))
def test_split_attention_masks(gpu_engine, name):
    cfg = SPLIT[name]
    starts, pfx = _dev(cfg.starts_tensor()), _dev(cfg.pfx_tensor())

    def kernel(qkv):           # rows the kernel does not write come back as zeros: no row of a valid config is all zero
        return gpu_engine.attention_split_ex(qkv.cuda(), cfg.n_seq, cfg.seq_len, cfg.heads, cfg.causal, starts=starts, pfx=pfx).cpu()
    fails = W.check_both(kernel, cfg, "split")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", list(F32))
def test_f32_attention_masks(gpu_engine, name):
    cfg = F32[name]
    fails = W.check_both(lambda qkv: gpu_engine.attention_f32(qkv.cuda(), cfg.n_seq, cfg.seq_len, cfg.heads, cfg.causal).cpu(),
                         cfg, "fp32")
    assert not fails, "\n".join(fails)


def test_ex_entry_points_refuse_what_the_launchers_refuse(pkg, gpu_engine):
    eng, E = gpu_engine, pkg.TVCError
    heads, T, n = 2, 20, 2
    st = torch.tensor([0, T, 2 * T], dtype=torch.int32).cuda()
    pf = torch.tensor([0, 0, 0, 0], dtype=torch.int32).cuda()
    for f16 in (False, True):
        dt = torch.float16 if f16 else torch.bfloat16
        qkv = torch.zeros((n * T, 3 * heads * 64), dtype=dt, device="cuda")
        out = torch.full((n * T, heads * 64), 5.0, dtype=dt, device="cuda")
        for kw in (dict(causal=True, pfx=pf), dict(causal=False, starts=st, pfx=pf)):       # pfx without starts / without causal
            with pytest.raises(E) as e:
                eng.attention_ex(qkv, n, T, heads, f16=f16, out=out, **kw)
            assert e.value.code == pkg._lib.TVC_E_INVALID
        for mode in (2, 3):                                                                  # dense EOT pooling without pool_row; no such mode
            with pytest.raises(E) as e:
                eng.attention_ex(qkv, n, T, heads, True, pool_mode=mode, f16=f16, out=out[:n])
            assert e.value.code == pkg._lib.TVC_E_INVALID
        for bad_T in (0, 289):
            with pytest.raises(E) as e:
                eng.attention_ex(qkv, n, bad_T, heads, True, f16=f16, out=out)
            assert e.value.code == pkg._lib.TVC_E_INVALID
        torch.cuda.synchronize()
        assert (out == 5.0).all()                                            # nothing was launched
    q32 = torch.zeros((n * T, 3 * heads * 64), device="cuda")
    for args, kw in (((n, T, heads, True), dict(pfx=pf)), ((n, T, heads, False), dict(starts=st, pfx=pf)),
                     ((n, 273, heads, True), dict(starts=st)), ((n, 0, heads, True), {})):
        with pytest.raises(E) as e:
            eng.attention_split_ex(q32, *args, **kw)
        assert e.value.code == pkg._lib.TVC_E_INVALID
    sa = pkg.sd_model.streaming_attention
    mk = lambda rows, ld: torch.zeros((rows, ld), dtype=torch.bfloat16, device="cuda")
    for ld in ((52, 64, 72, 52), (56, 68, 72, 52), (56, 64, 76, 52), (56, 64, 72, 50), (40, 64, 72, 52), (56, 64, 72, 44)):
        out = torch.full((2 * 5, ld[3]), 5.0, dtype=torch.bfloat16, device="cuda")
        with pytest.raises(E) as e:
            sa(eng, mk(2 * 5, ld[0]), mk(2 * 7, ld[1]), mk(2 * 7, ld[2]), 2, 2, ld=ld, dh=24, out=out)
        assert e.value.code == pkg._lib.TVC_E_INVALID
        torch.cuda.synchronize()
        assert (out == 5.0).all()


# ------------------------------------------------------------------------------------------- streaming kernel
TQ = (1, 63, 64, 65, 129, 257)
TK = (1, 63, 64, 65, 77, 130)


def _sd_kernel(pkg, eng, n, heads, dh, pad=None):
    """pad = None: the one-stride entry point.  pad = (pq, pk, pv, po): rows padded by that many columns, q / k / v pads
    filled with NaN (never read), the output's with a sentinel that must survive."""
    sa = pkg.sd_model.streaming_attention
    C = heads * dh
    if pad is None:
        return lambda q, k, v: sa(eng, q.to(torch.bfloat16).cuda(), k.to(torch.bfloat16).cuda(), v.to(torch.bfloat16).cuda(), n, heads).float().cpu()

    def kernel(q, k, v):
        wide = []
        for t, p in zip((q, k, v), pad):
            w = torch.full((t.shape[0], C + p), float("nan"), dtype=torch.bfloat16, device="cuda")
            w[:, :C] = t.to(torch.bfloat16).cuda()
            wide.append(w)
        out = torch.full((q.shape[0] + GUARD, C + pad[3]), 7.0, dtype=torch.bfloat16, device="cuda")
        sa(eng, *wide, n, heads, ld=tuple(C + p for p in pad), dh=dh, out=out[:q.shape[0]])
        assert (out[:q.shape[0], C:] == 7.0).all() and (out[q.shape[0]:] == 7.0).all(), "guard columns / rows were written"
        return out[:q.shape[0], :C].float().cpu()
    return kernel


@pytest.mark.parametrize("dh", W.SD_HEAD_DIMS)
def test_streaming_attention_masks_every_head_dim(pkg, gpu_engine, dh):
    """Shape 1 (4 waves x 1 block; n * heads = 6): every Tq against a Tk, rotated by the head dim so that the twelve head
    dims between them meet all 36 (Tq, Tk) pairs twice."""
    n, heads = 2, 3
    kernel = _sd_kernel(pkg, gpu_engine, n, heads, dh)
    fails = []
    for j, Tq in enumerate(TQ):
        Tk = TK[(j + W.SD_HEAD_DIMS.index(dh)) % len(TK)]
        fails += W.sd_check_readback(kernel, n, heads, dh, Tq, Tk) + W.sd_check_needle(kernel, n, heads, dh, Tq, Tk)
    assert not fails, "\n".join(fails)


def _shape(items, Tq, dh):
    """The dispatcher's rule (csrc/sd_attention.hip, sd_flash_attention), restated to name the shape a case reaches."""
    shape = 1
    if items * ((Tq + 127) // 128) >= 512:
        shape = 2
    if items * ((Tq + 255) // 256) >= 512:
        shape = 3
    return min(shape, 3 if dh <= 80 else 1)


@pytest.mark.parametrize("Tq,shape", [(130, 2), (257, 3)])
@pytest.mark.parametrize("dh", [d for d in W.SD_HEAD_DIMS if d <= 80])
def test_streaming_attention_masks_wide_workgroups(pkg, gpu_engine, dh, Tq, shape):
    """n * heads = 256 items: 4 waves x 2 blocks at Tq = 130, 8 waves x 2 blocks at Tq = 257, with a ragged last query
    block and a ragged second key tile (Tk = 77) in both."""
    n, heads, Tk = 32, 8, 77
    assert _shape(n * heads, Tq, dh) == shape
    kernel = _sd_kernel(pkg, gpu_engine, n, heads, dh)
    fails = W.sd_check_readback(kernel, n, heads, dh, Tq, Tk) + W.sd_check_needle(kernel, n, heads, dh, Tq, Tk)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n,heads,Tq,shape", [(2, 3, 65, 1), (32, 8, 130, 2), (32, 8, 257, 3)])
def test_streaming_attention_masks_with_separate_strides(pkg, gpu_engine, n, heads, Tq, shape):
    """ldq != ldk != ldv != ldo (rows padded by 8 / 16 / 24 / 4 columns: 16-byte-aligned q / k / v rows, 8-byte-aligned
    output rows), as the model's fused projections pass them; guard columns and rows checked untouched."""
    dh, Tk = 40, 130
    assert _shape(n * heads, Tq, dh) == shape
    kernel = _sd_kernel(pkg, gpu_engine, n, heads, dh, pad=(8, 16, 24, 4))
    fails = W.sd_check_readback(kernel, n, heads, dh, Tq, Tk) + W.sd_check_needle(kernel, n, heads, dh, Tq, Tk)
    assert not fails, "\n".join(fails)
