"""CPU: the launch sequence of the latent-diffusion host code (csrc/tvc_sd.cpp) is pinned without a GPU.

tests/host_san_sd_trace/driver.cpp runs every SD entry point on the toy geometry against tests/host_san's HIP stand-in with
the stubs of ``gen_stubs.py --trace``, under AddressSanitizer / UBSan with leak detection (built and run by
tests/host_san_build.py, which every host-sanitizer test shares): every launcher with all its
arguments (floats as %a, streams as ordinals, pointers as block + offset: the arena's walk), every GemmLaunch field, every
hipMalloc / copy / event call lands in one trace.  The full trace is about 2 MB, more than a committed file may have, so tests/golden/sd_host_trace.txt holds
one line per call of the driver: the SHA-256 of the call's trace lines, their count, the call.  It was recorded from the
csrc/tvc_sd.cpp of commit 2b4a924 ("One arg-max select core and one bank-row view for bank, k-means, IVF"), the last one before
that file's host code was reorganised; a refactor of tvc_sd.cpp leaves it byte-identical.

As a script, to find the line behind a digest that differs, in two steps with the same DIR:
  1. in a checkout of the recorded commit (with this test, tests/host_san_build.py, the driver and tests/host_san from here;
     the sources come from that checkout's own csrc/Makefile):
         python tests/test_sd_trace_host.py --keep DIR       writes the full trace to DIR/sd_host_trace.full.txt
  2. in the checkout under test, the same command: DIR already holds a trace, so the new one is compared with it and the first
     differing line is printed with the call it belongs to (the new trace goes to DIR/sd_host_trace.full.new.txt).
``--record`` rewrites the golden file from the sources of the checkout it runs in."""
import hashlib
import importlib
import sys
from pathlib import Path

import host_san_build

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "sd_host_trace.txt"


def run_driver(pkg, tmp_path: Path, tmp_path_factory=None) -> Path:
    import torch
    names = host_san_build.write_sd_names(pkg, tmp_path / "names.txt", dtype=torch.float16)
    trace = tmp_path / "trace.txt"
    host_san_build.run_driver("host_san_sd_trace", "HOST_SAN_SD_TRACE_OK", tmp_path_factory, args=[names], trace=trace)
    return trace


def digests(trace: Path) -> list:
    """One '<sha256> <lines> <marker>' per call: a call's lines run from its '# ...' marker to the next one."""
    out, marker, sha, n = [], "# start", hashlib.sha256(), 0
    with open(trace) as f:
        for line in f:
            if line.startswith("#"):
                out.append(f"{sha.hexdigest()} {n} {marker}")
                marker, sha, n = line.rstrip("\n"), hashlib.sha256(), 0
            else:
                sha.update(line.encode())
                n += 1
    out.append(f"{sha.hexdigest()} {n} {marker}")
    return out


def test_sd_host_trace_matches_the_recorded_one(pkg, tmp_path, tmp_path_factory):
    got = digests(run_driver(pkg, tmp_path, tmp_path_factory))
    want = GOLDEN.read_text().splitlines()
    print(f"{len(got)} calls, {sum(int(g.split()[1]) for g in got)} trace lines")
    assert len(want) > 60 and sum(int(w.split()[1]) for w in want) > 10000            # the recorded trace is a real one
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff and len(got) == len(want), \
        f"{len(diff)} of {len(want)} calls differ; the first (recorded, got): {diff[:1]} -- python {Path(__file__).name} --keep DIR shows the line"


def first_difference(a: Path, b: Path):
    marker = ""
    with open(a) as fa, open(b) as fb:
        for i, (x, y) in enumerate(zip(fa, fb), 1):
            if x.startswith("#"):
                marker = x.strip()
            if x != y:
                return i, marker, x.rstrip("\n"), y.rstrip("\n")
        x, y = fa.readline(), fb.readline()
        if x or y:
            return i + 1, marker, x.rstrip("\n") or "<end>", y.rstrip("\n") or "<end>"
    return None


if __name__ == "__main__":
    import argparse
    import shutil
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None, help="directory that keeps the full trace")
    ap.add_argument("--record", action="store_true", help="rewrite tests/golden/sd_host_trace.txt")
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    pkg_ = importlib.import_module("multimodal-detection-consistency_amd")
    with tempfile.TemporaryDirectory() as tmp:
        t = run_driver(pkg_, Path(tmp))
        d = digests(t)
        print(f"{len(d)} calls, {sum(int(x.split()[1]) for x in d)} trace lines, {t.stat().st_size} bytes")
        if a.record:
            GOLDEN.write_text("\n".join(d) + "\n")
        if a.keep:
            kept = Path(a.keep) / "sd_host_trace.full.txt"
            kept.parent.mkdir(parents=True, exist_ok=True)
            if kept.exists():
                fd = first_difference(kept, t)
                print("identical to the kept trace" if fd is None else
                      f"first difference at line {fd[0]} in [{fd[1]}]:\n  kept: {fd[2]}\n  new:  {fd[3]}")
                shutil.copy(t, kept.with_suffix(".new.txt"))
            else:
                shutil.copy(t, kept)
        same = d == GOLDEN.read_text().splitlines()
        print("golden:", "identical" if same else "DIFFERENT")
        sys.exit(0 if same else 1)
