"""CPU: the closest-pair C-ABI surface -- tvc_closest_pair is declared in include/tvc.h, bound in _lib.SIGNATURES and exported by
the built library without an ABI version bump, no other source references its unit, and its host code (tvc_nearest.cpp: every
refusal, the workspace, the plan of host_plan.hpp) runs clean under AddressSanitizer / UBSan with leak detection
(tests/host_san_nearest/driver.cpp, a stand-alone program on tests/host_san's HIP stand-in, built and run by
tests/host_san_build.py)."""
import re
import subprocess
from pathlib import Path

import host_san_build

ROOT = Path(__file__).resolve().parents[1]
NEW = {"tvc_closest_pair"}


def test_closest_pair_entry_point_declared_bound_and_exported(pkg):
    h = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tvc.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(tvc_[a-z0-9_]+)\s*\(", h))
    assert NEW <= declared
    assert NEW <= set(pkg._lib.SIGNATURES)
    assert len(pkg._lib.SIGNATURES["tvc_closest_pair"][1]) == 6
    lib = pkg._lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    out = subprocess.run(["nm", "-D", "--defined-only", str(pkg._lib.LIB_PATH)], capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\bT (tvc_[a-z0-9_]+)", out))
    assert lib.tvc_abi_version() == 4                        # additive: no ABI version bump
    assert callable(pkg.TVCEngine.closest_pair)
    assert callable(pkg.ref_bank.similarity_victim) and callable(pkg.ReferenceBank._remove_most_similar)
    assert pkg.ReferenceBankConfig().update_strategy == "fifo"            # the default does not change


def test_no_existing_source_references_the_nearest_unit():
    """The other host-sanitizer tests compile fixed source lists without tvc_nearest.cpp: nothing outside it may need its symbols."""
    csrc = ROOT / "multimodal-detection-consistency_amd" / "csrc"
    for p in sorted(csrc.glob("*.cpp")):
        if p.name != "tvc_nearest.cpp":
            text = p.read_text()
            for name in ("tvc_closest_pair", "launch_closest_pair", "nearest_plan", "WS_NN_"):
                assert name not in text, (p.name, name)


def test_nearest_host_code_under_address_and_ub_sanitizers(tmp_path_factory):
    assert "launch_closest_pair" in host_san_build.stubs_text(tmp_path_factory)
    host_san_build.run_driver("host_san_nearest", "HOST_SAN_NEAREST_OK", tmp_path_factory)      # run directly: nothing is preloaded
