"""CPU: the latent-diffusion model's fp16 mode (TVC_OPT_SD_PRECISION = 1) without a GPU -- the option is declared in
include/tvc.h and bound in _lib with no new exported symbol and no ABI bump; ``prepare_sd_tensors`` prepares either 16-bit
dtype and its default output is unchanged; and the host code that drives the mode runs clean under AddressSanitizer / UBSan
with every GEMM range checked (tests/host_san_sd_f16/driver.cpp on tests/host_san's HIP stand-in, built and run by
tests/host_san_build.py)."""
import importlib
import re
import subprocess
from pathlib import Path

import pytest
import torch

import host_san_build

ROOT = Path(__file__).resolve().parents[1]


def test_sd_precision_option_declared_and_bound_without_a_new_symbol(pkg):
    text = (ROOT / "include" / "tvc.h").read_text()
    assert re.search(r"\bTVC_OPT_SD_PRECISION\s*=\s*10\b", text)
    assert pkg._lib.TVC_OPT_SD_PRECISION == 10
    assert re.search(r"#define\s+TVC_ABI_VERSION\s+4\b", text) and pkg._lib.TVC_ABI_VERSION == 4
    lib = pkg._lib.load()
    assert lib.tvc_abi_version() == 4
    # the exported symbol set is what the header declares and _lib binds: the mode adds an option value, not an entry point
    h = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tvc_[a-z0-9_]+)\s*\(", h)) - {"tvc_rec_stride"}          # a static inline of the header
    out = subprocess.run(["nm", "-D", "--defined-only", str(pkg._lib.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (tvc_[a-z0-9_]+)", out))
    assert exported == set(pkg._lib.SIGNATURES) == declared
    assert not any("sd_precision" in n or n.endswith("_sd_f16") for n in exported)


def _tiny_state_dicts():
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(s, generator=g)
    p = "down_blocks.0.attentions.0.transformer_blocks.0."
    unet = {
        "conv_in.weight": r(24, 4, 3, 3), "conv_in.bias": r(24),                       # 36 columns -> zero padded to 64
        "down_blocks.0.resnets.0.conv1.weight": r(24, 16, 3, 3), "down_blocks.0.resnets.0.conv1.bias": r(24),
        "down_blocks.0.resnets.0.norm1.weight": r(16), "down_blocks.0.resnets.0.norm1.bias": r(16),
        "down_blocks.0.resnets.0.conv_shortcut.weight": r(24, 16, 1, 1), "down_blocks.0.resnets.0.conv_shortcut.bias": r(24),
        p + "attn1.to_q.weight": r(24, 24), p + "attn1.to_k.weight": r(24, 24), p + "attn1.to_v.weight": r(24, 24),
        p + "attn2.to_q.weight": r(24, 24), p + "attn2.to_k.weight": r(24, 40), p + "attn2.to_v.weight": r(24, 40),
        p + "ff.net.2.weight": r(24, 96), p + "ff.net.2.bias": r(24),
        "big.weight": r(512, 8),                                                         # already whole tiles: no padding
    }
    v = "decoder.mid_block.attentions.0."
    vae = {
        v + "query.weight": r(16, 16), v + "key.weight": r(16, 16), v + "value.weight": r(16, 16),
        v + "query.bias": r(16), v + "key.bias": r(16), v + "value.bias": r(16),
        v + "group_norm.weight": r(16), v + "group_norm.bias": r(16),
        "post_quant_conv.weight": r(4, 4, 1, 1), "post_quant_conv.bias": r(4),
    }
    return unet, vae


def test_prepare_sd_tensors_in_either_16_bit_dtype(pkg):
    sdm = importlib.import_module(pkg.__name__ + ".sd_model")
    unet, vae = _tiny_state_dicts()
    cpu = torch.device("cpu")
    t16 = sdm.prepare_sd_tensors(unet, vae, cpu, dtype=torch.float16)
    tbf = sdm.prepare_sd_tensors(unet, vae, cpu, dtype=torch.bfloat16)
    dflt = sdm.prepare_sd_tensors(unet, vae, cpu)
    # the default is today's output: same names, dtypes, shapes and bits (bf16 GEMM operands)
    assert sorted(dflt) == sorted(tbf) == sorted(t16)
    for n in dflt:
        assert dflt[n].dtype == tbf[n].dtype and torch.equal(dflt[n], tbf[n]), n
    p = "down_blocks.0.attentions.0.transformer_blocks.0."
    v = "decoder.mid_block.attentions.0."
    gemm = {"conv_in.weight": (24, 64), "down_blocks.0.resnets.0.conv1.weight": (24, 144),
            "down_blocks.0.resnets.0.conv_shortcut.weight": (24, 16), p + "attn1.to_qkv.weight": (72, 24),
            p + "attn2.to_q.weight": (24, 24), p + "attn2.to_kv.weight": (48, 40), p + "ff.net.2.weight": (24, 96),
            "big.weight": (512, 8), v + "to_qkv.weight": (48, 16)}
    for n, (rows, cols) in gemm.items():
        for t, dt in ((t16, torch.float16), (tbf, torch.bfloat16)):
            x = t[n]
            assert x.dtype == dt and x.is_contiguous(), n
            assert x.shape == ((rows + 255) // 256 * 256, cols), (n, x.shape)          # readable to whole 256-row tiles
            assert not x[rows:].any(), n                                                  # ... of zeros (0x0000 in both formats)
    assert {n for n in t16 if t16[n].dtype == torch.float16} == set(gemm)
    # the layout does not depend on the dtype: each fp16 tensor is the fp32 source, rearranged, rounded once
    w = unet["down_blocks.0.resnets.0.conv1.weight"]
    assert torch.equal(t16["down_blocks.0.resnets.0.conv1.weight"][:24], w.permute(0, 2, 3, 1).reshape(24, 144).to(torch.float16))  # tap-major
    ci = t16["conv_in.weight"]
    assert torch.equal(ci[:24, :36], unet["conv_in.weight"].permute(0, 2, 3, 1).reshape(24, 36).to(torch.float16)) and not ci[:, 36:].any()
    assert torch.equal(t16[p + "attn1.to_qkv.weight"][:72],
                       torch.cat([unet[p + "attn1.to_q.weight"], unet[p + "attn1.to_k.weight"], unet[p + "attn1.to_v.weight"]]).to(torch.float16))
    assert torch.equal(t16[p + "attn2.to_kv.weight"][:48], torch.cat([unet[p + "attn2.to_k.weight"], unet[p + "attn2.to_v.weight"]]).to(torch.float16))
    assert torch.equal(t16[v + "to_qkv.weight"][:48], torch.cat([vae[v + "query.weight"], vae[v + "key.weight"], vae[v + "value.weight"]]).to(torch.float16))
    assert torch.equal(t16["down_blocks.0.resnets.0.conv_shortcut.weight"][:24], unet["down_blocks.0.resnets.0.conv_shortcut.weight"].reshape(24, 16).to(torch.float16))
    # biases, norms and post_quant_conv stay fp32 and unpadded, bit for bit the source
    for n in ("conv_in.bias", "down_blocks.0.resnets.0.norm1.weight", p + "ff.net.2.bias", v + "group_norm.bias"):
        assert t16[n].dtype == torch.float32 and torch.equal(t16[n], (unet if n in unet else vae)[n])
    assert torch.equal(t16[v + "to_qkv.bias"], torch.cat([vae[v + "query.bias"], vae[v + "key.bias"], vae[v + "value.bias"]]))
    assert t16["post_quant_conv.weight"].dtype == torch.float32 and t16["post_quant_conv.weight"].shape == (4, 4)
    # fp16 rounds closer than bf16 (10 mantissa bits to 7) on the same source
    big = unet["big.weight"]
    assert (t16["big.weight"].float() - big).abs().max() < (tbf["big.weight"].float() - big).abs().max()
    with pytest.raises(ValueError):
        sdm.prepare_sd_tensors(unet, vae, cpu, dtype=torch.float32)


def test_precision_fields_and_defaults(pkg):
    """The defaults stay bf16 everywhere; ``torch_dtype`` keeps the reference's name and default and selects nothing."""
    assert pkg.SDModelConfig().precision == "bf16" and pkg.SDReferenceConfig().precision == "bf16"
    assert pkg.SDReferenceConfig().torch_dtype == "float16"
    assert pkg.SDReferenceConfig(precision="fp16").precision == "fp16"
    assert pkg.TVCEngine.SD_PRECISIONS == {"bf16": 0, "fp16": 1}


def test_sd_fp16_host_code_under_address_and_ub_sanitizers(pkg, tmp_path, tmp_path_factory):
    # the toy geometry of the driver, tensors as the product's own host code prepares them for the fp16 mode
    names = host_san_build.write_sd_names(pkg, tmp_path / "names.txt", dtype=torch.float16)
    host_san_build.run_driver("host_san_sd_f16", "HOST_SAN_SD_F16_OK", tmp_path_factory, args=[names])
