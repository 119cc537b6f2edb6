"""CPU: the closest-pair C-ABI surface -- tvc_closest_pair is declared in include/tvc.h, bound in _lib.SIGNATURES and exported by
the built library without an ABI version bump, no other source references its unit, and its host code (tvc_nearest.cpp: every
refusal, the workspace, the plan of host_plan.hpp) runs clean under AddressSanitizer / UBSan with leak detection
(tests/host_san_nearest/driver.cpp, a stand-alone program on tests/host_san's HIP stand-in: the build of test_dbscan_host.py
plus tvc_nearest.cpp)."""
import os
import re
import subprocess
import sys
from pathlib import Path

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


def test_nearest_host_code_under_address_and_ub_sanitizers(tmp_path):
    csrc = ROOT / "multimodal-detection-consistency_amd" / "csrc"
    san = ROOT / "tests" / "host_san"
    stubs = tmp_path / "stubs.cpp"
    subprocess.run([sys.executable, str(san / "gen_stubs.py"), str(csrc / "kernels.hpp"), str(stubs)], check=True)
    assert "launch_closest_pair" in stubs.read_text()
    exe = tmp_path / "driver_nearest"
    srcs = ("tvc_abi.cpp", "tvc_precise.cpp", "tvc_split.cpp", "tvc_sd.cpp", "tvc_sd_op.cpp", "tvc_tower_op.cpp", "tvc_kmeans.cpp",
            "tvc_ivf.cpp", "tvc_attack.cpp", "tvc_dbscan.cpp", "tvc_nearest.cpp")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{san}", f"-I{csrc}", "-x", "c++"] + [str(csrc / f) for f in srcs] + \
          [str(stubs), str(ROOT / "tests" / "host_san_nearest" / "driver.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)       # run directly: nothing is preloaded
    assert r.returncode == 0 and "HOST_SAN_NEAREST_OK" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
