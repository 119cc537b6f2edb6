"""CPU: the k-means C-ABI surface -- tvc_kmeans_assign / tvc_kmeans_update are declared in include/tvc.h, bound in
_lib.SIGNATURES and exported by the built library without an ABI version bump, and their host code (tvc_kmeans.cpp: slot
checks, refusals, workspaces) runs clean under AddressSanitizer / UBSan with leak detection
(tests/host_san_kmeans/driver.cpp on tests/host_san's HIP stand-in, built and run by tests/host_san_build.py)."""
import re
import subprocess
from pathlib import Path

import host_san_build

ROOT = Path(__file__).resolve().parents[1]
NEW = {"tvc_kmeans_assign", "tvc_kmeans_update"}


def test_kmeans_entry_points_declared_bound_and_exported(pkg):
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
    for name in ("kmeans_assign", "kmeans_update", "kmeans"):
        assert callable(getattr(pkg.TVCEngine, name))


PLAN_CHECK = r"""
#include "host_plan.hpp"
#include <stdio.h>
int main() {
    const int64_t Rs[] = {1, 2, 255, 256, 257, 1000, 4096, 65536, 1000000, 10000019, 0x7fffffffLL};
    const int Ks[] = {1, 3, 100, 1024, 4097, 65536};
    for (int64_t R : Rs) for (int K : Ks) {
        if (K > R) continue;
        int nb = -1, rpb = -1;
        kmeans_update_plan(R, K, &nb, &rpb);
        const bool ok = nb >= 1 && nb <= 1024 && rpb >= 256 && rpb % 256 == 0 && (int64_t)nb * rpb >= R &&
                        (int64_t)(nb - 1) * rpb < R && (int64_t)nb * K <= ((int64_t)4 << 20);
        if (!ok) { printf("bad plan R=%lld K=%d: nblocks=%d rows_per_block=%d\n", (long long)R, K, nb, rpb); return 1; }
    }
    printf("PLAN_OK\n");
    return 0;
}
"""


def test_kmeans_update_plan_covers_every_row(tmp_path):
    """host_plan.hpp's kmeans_update_plan, the arithmetic the product and the sanitizer build share: the blocks cover R with
    none left empty, a block is a whole number of 256-row chunks, the counter matrix stays under 16 MiB."""
    csrc = ROOT / "multimodal-detection-consistency_amd" / "csrc"
    src = tmp_path / "plan.cpp"
    src.write_text(PLAN_CHECK)
    exe = tmp_path / "plan"
    b = subprocess.run(["g++", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", f"-I{csrc}", str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "PLAN_OK" in r.stdout, (r.stdout, r.stderr)


def test_kmeans_host_code_under_address_and_ub_sanitizers(tmp_path_factory):
    host_san_build.run_driver("host_san_kmeans", "HOST_SAN_KMEANS_OK", tmp_path_factory)
