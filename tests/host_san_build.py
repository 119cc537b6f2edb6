"""The host-sanitizer build, shared by every test that runs a tests/host_san*/driver.cpp (imported like similarity_ref.py; no
fixture, no plugin).

The C-ABI's host code -- every source on the ``CPP_SRCS`` line of csrc/Makefile -- and the kernel-launcher stubs of
``tests/host_san/gen_stubs.py --trace`` are compiled once per Python process, one ``g++ -fsanitize=address,undefined`` per file
against the HIP stand-in of tests/host_san, into object files; ``run_driver`` then compiles one driver, links it with those
objects and runs it as a stand-alone program (nothing is preloaded).  The stubs trace only when HIP_STUB_TRACE is set
(tests/host_san/hip/hip_runtime.h: hip_trace), so one stub object serves every driver.  Nothing outlives the process: the
objects live in a directory of the caller's ``tmp_path_factory``, or without one in a temporary directory removed at exit."""
import atexit
import importlib
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "multimodal-detection-consistency_amd" / "csrc"
SAN = ROOT / "tests" / "host_san"
CXX = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{SAN}", f"-I{CSRC}"]
TIMEOUT = 600

_build = None            # (object files, stubs.cpp) once built; the error text if the build failed


def sources() -> list:
    """The host sources of the product: the CPP_SRCS line of csrc/Makefile."""
    m = re.search(r"^CPP_SRCS[ \t]*=[ \t]*(.*)$", (CSRC / "Makefile").read_text(), flags=re.M)
    assert m and m.group(1).split(), "csrc/Makefile: no CPP_SRCS line, or an empty one"
    srcs = [CSRC / name for name in m.group(1).split()]
    missing = [p.name for p in srcs if not p.is_file()]
    assert not missing, f"csrc/Makefile: CPP_SRCS names {', '.join(missing)}, which csrc/ does not hold"
    return srcs


def _tmp_dir(tmp_path_factory, name: str) -> Path:
    if tmp_path_factory is not None:
        return tmp_path_factory.mktemp(name)
    d = Path(tempfile.mkdtemp(prefix=name + "_"))
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


def _compile_all(out: Path):
    stubs = out / "stubs.cpp"
    subprocess.run([sys.executable, str(SAN / "gen_stubs.py"), str(CSRC / "kernels.hpp"), str(stubs), "--trace"], check=True,
                   capture_output=True, timeout=TIMEOUT)
    units = sources() + [stubs]
    objs = [out / (p.stem + ".o") for p in units]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        done = list(pool.map(lambda po: subprocess.run(CXX + ["-c", str(po[0]), "-o", str(po[1])], capture_output=True, text=True,
                                                       timeout=TIMEOUT), zip(units, objs)))
    failed = [f"{p.name}:\n{b.stderr[-3000:]}" for p, b in zip(units, done) if b.returncode != 0]
    assert not failed, "\n".join(failed)
    return objs, stubs


def build(tmp_path_factory=None):
    """(object files, stubs.cpp) of the sanitizer build; compiled by the first call of the process."""
    global _build
    if _build is None:
        try:
            _build = _compile_all(_tmp_dir(tmp_path_factory, "host_san_objs"))
        except Exception as e:                      # a later test shows the same failure without compiling again
            _build = f"the host-sanitizer build failed: {e}"
    assert not isinstance(_build, str), _build
    return _build


def stubs_text(tmp_path_factory=None) -> str:
    """The generated stubs.cpp: a test asserts the launchers its driver needs are in it."""
    return build(tmp_path_factory)[1].read_text()


def run_driver(name: str, marker: str, tmp_path_factory=None, args=(), trace=None) -> None:
    """Compiles tests/<name>/driver.cpp, links it with the shared objects and runs it under ASan (leaks on) and UBSan; it must
    end with status 0 and print `marker`.  `trace`: the file HIP_STUB_TRACE names (unset without it)."""
    objs, _ = build(tmp_path_factory)
    exe = _tmp_dir(tmp_path_factory, name) / "driver"
    driver = Path("tests") / name / "driver.cpp"    # relative to ROOT: a CHECK reports it as __FILE__
    b = subprocess.run(CXX + [str(driver)] + [str(o) for o in objs] + ["-o", str(exe)], capture_output=True, text=True,
                       timeout=TIMEOUT, cwd=ROOT)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("HIP_STUB_TRACE", None)
    if trace is not None:
        env["HIP_STUB_TRACE"] = str(trace)
    r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=TIMEOUT, env=env)
    assert r.returncode == 0 and marker in r.stdout, (r.stdout[-500:], r.stderr[-3000:])


def write_sd_names(pkg, path: Path, dtype=None) -> Path:
    """names.txt of the toy latent-diffusion geometry the SD drivers load: one "name rows cols element_size" per tensor, as the
    product's own host code prepares them (`dtype`: the 16-bit format of the GEMM operands; None = the default)."""
    import torch
    sdm = importlib.import_module(pkg.__name__ + ".sd_model")
    arch = pkg.SDArch(block_out_channels=(64, 128), down_block_attn=(True, False), layers_per_block=1, heads=8,
                      cross_attention_dim=128, vae_block_out_channels=(64, 128), vae_layers_per_block=1, sample_size=16)
    uw, vw = pkg.make_sd_weights(arch, seed=3)
    kw = {} if dtype is None else {"dtype": dtype}
    with open(path, "w") as f:
        for n, x in sorted(sdm.prepare_sd_tensors(uw, vw, torch.device("cpu"), **kw).items()):
            f.write(f"{n} {x.shape[0]} {x.numel() // x.shape[0]} {x.element_size()}\n")
    return path
