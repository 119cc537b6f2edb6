"""CPU: the host code of the retrieval-evaluation entry points (tvc_rank.cpp: slot checks, refusals, workspaces; the plan of
host_plan.hpp) runs clean under AddressSanitizer / UBSan with leak detection, as a stand-alone program
(tests/host_san_rank/driver.cpp on tests/host_san's HIP stand-in, the build of test_kmeans_host.py with tvc_rank.cpp)."""
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_rank_host_code_under_address_and_ub_sanitizers(tmp_path):
    csrc = ROOT / "multimodal-detection-consistency_amd" / "csrc"
    san = ROOT / "tests" / "host_san"
    stubs = tmp_path / "stubs.cpp"
    subprocess.run([sys.executable, str(san / "gen_stubs.py"), str(csrc / "kernels.hpp"), str(stubs)], check=True)
    exe = tmp_path / "driver_rank"
    srcs = ("tvc_abi.cpp", "tvc_precise.cpp", "tvc_split.cpp", "tvc_sd.cpp", "tvc_sd_op.cpp", "tvc_tower_op.cpp", "tvc_rank.cpp")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{san}", f"-I{csrc}", "-x", "c++"] + [str(csrc / f) for f in srcs] + \
          [str(stubs), str(ROOT / "tests" / "host_san_rank" / "driver.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "HOST_SAN_RANK_OK" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
