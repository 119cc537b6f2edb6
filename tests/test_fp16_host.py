"""CPU: the fp16 tower mode's C-ABI surface (TVC_OPT_TOWER_PRECISION = 3) -- the new entry points are declared in
include/tvc.h, bound in _lib.SIGNATURES and exported by the built library, and the host code that drives the mode runs
clean under AddressSanitizer / UBSan with every GEMM range checked (tests/host_san_f16/driver.cpp on tests/host_san's HIP
stand-in, built and run by tests/host_san_build.py)."""
import re
import subprocess
from pathlib import Path

import host_san_build

ROOT = Path(__file__).resolve().parents[1]
NEW = {"tvc_set_weights_f16", "tvc_gemm_f16", "tvc_attention_f16", "tvc_layernorm_f16"}


def test_fp16_entry_points_declared_bound_and_exported(pkg):
    h = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tvc.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(tvc_[a-z0-9_]+)\s*\(", h))
    assert NEW <= declared
    assert NEW <= set(pkg._lib.SIGNATURES)
    lib = pkg._lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    out = subprocess.run(["nm", "-D", "--defined-only", str(pkg._lib.LIB_PATH)], capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\bT (tvc_[a-z0-9_]+)", out))
    assert lib.tvc_abi_version() == 4                        # additive: no ABI version bump
    assert pkg.TVCEngine.PRECISIONS["fp16"] == 3


def test_fp16_mode_host_code_under_address_and_ub_sanitizers(tmp_path_factory):
    host_san_build.run_driver("host_san_f16", "HOST_SAN_F16_OK", tmp_path_factory)
