"""GPU: the C-ABI contract of the GEMMs (include/tvc.h) on every launch form -- operand row pitches beyond K (the padding
is filled with NaN, so a read past K shows), output pitches beyond I (I + 4 with I % 8 == 0 reaches the 8-byte 16-bit
store, I + 1 the scalar one), ragged I (I % 4 = 1, 3), and guard bands: the output is a [J, I] view at row G of a
(G + J + G) x ld_out buffer of sentinel bits, and every bit outside the view must survive the launch.

tvc_gemm_bf16 / tvc_gemm_f16 run in one child process per env switch (read once per process), each over the cases
labelled for it; a case's label is the form csrc/host_plan.hpp's gemm_form gives it in that process, which
tests/test_gemm_form.py asserts on the CPU.  References: fp64 on the same rounded operands.  Epilogue 1 must equal the
round-to-nearest-even of the same form's epilogue-0 output, epilogue 2 one 16-bit rounding of QuickGELU of it,
epilogue 3 base + epilogue 0 within two fp32 roundings.  Across children: ring forms 1 and 4 return the same bits, and
a split-K form really runs (its fp32 sums differ from the one-pass kernel's in at least one element).

Run as ``python tests/test_gpu_gemm_contract.py --child ENV`` it is that child."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import pytest
import torch

G = 16                                  # guard rows on each side (16 rows keep the view 16-byte aligned at any pitch)
SENT16, SENT32 = 0x7FA5, 0x7FA5A5A5     # NaN bit patterns in bf16, fp16 and fp32
ENVS = ("", "TVC_GEMM_RING_FORM=1", "TVC_GEMM_VARIANT=0", "TVC_GEMM_SPLITK_SMALL=1", "TVC_GEMM_SPLITK_TAIL=1")
LDO_OFF = (0, 4, 1, 64)                 # ld_out - I
LD_OFF = (0, 8, 64)                     # lda - K, ldb - K


def _pairwise(space):
    """Greedy all-pairs selection over the dict of value lists ``space`` (deterministic)."""
    names = list(space)
    vals = [space[n] for n in names]
    combos = list(itertools.product(*[range(len(v)) for v in vals]))
    pairs = lambda c: {(i, c[i], j, c[j]) for i in range(len(c)) for j in range(i + 1, len(c))}
    todo = set().union(*(pairs(c) for c in combos))
    rows = []
    while todo:
        best = max(combos, key=lambda c: len(pairs(c) & todo))
        todo -= pairs(best)
        rows.append({n: vals[i][best[i]] for i, n in enumerate(names)})
    return rows


def _family(name, I_of, J, K, labels, epis=(0, 1, 2, 3), lds=LD_OFF, imods=(0, 1, 3)):
    space = dict(epi=epis, ldo=LDO_OFF, lda=lds, ldb=lds, imod=imods, bias=(True, False))
    out = []
    for n, r in enumerate(_pairwise(space)):
        I = I_of[r["imod"]]
        out.append(dict(id=f"{name}{n}", I=I, J=J, K=K, lda=K + r["lda"], ldb=K + r["ldb"], ldo=I + r["ldo"],
                        epi=r["epi"], bias=r["bias"], labels=labels))
    return out


# label: env -> the form gemm_form gives the case in that process (a case runs only in the children it is labelled for)
CASES = (
    # K = 128 < 256: no ring stages to speak of, the one-tile kernel whatever the tile count
    _family("one", {0: 512, 1: 257, 3: 299}, 300, 128, {"": "ONE_TILE"})
    # 8 tiles of K = 256 with ragged token rows (J % 256 != 0): ring form 1; TVC_GEMM_VARIANT=0: one tile per workgroup
    + _family("ring1_", {0: 512, 1: 257, 3: 299}, 1000, 256, {"": "RING1", "TVC_GEMM_VARIANT=0": "ONE_TILE"})
    # 8 whole tiles, pitches of whole 128-byte lines: ring form 4 by default, form 1 when forced
    + _family("ring4_", {0: 512}, 1024, 256, {"": "RING4", "TVC_GEMM_RING_FORM=1": "RING1"}, epis=(0, 1, 2), lds=(0, 64),
              imods=(0,))
    # the same shape where form 4's preconditions fail (a pitch of K + 8, the residual epilogue): form 1 in both processes
    + [dict(id=f"ring4to1_{n}", I=512, J=1024, K=256, lda=256 + da, ldb=256 + db, ldo=512 + do, epi=epi, bias=True,
            labels={"": "RING1", "TVC_GEMM_RING_FORM=1": "RING1"})
       for n, (da, db, do, epi) in enumerate(((8, 0, 0, 1), (0, 8, 4, 0), (64, 64, 4, 3), (8, 64, 1, 2)))]
    # 4 tiles of a deep K: TVC_GEMM_SPLITK_SMALL=1 splits K 8 ways; by default the one-tile kernel
    + _family("small", {0: 512, 1: 257, 3: 299}, 300, 1024, {"TVC_GEMM_SPLITK_SMALL=1": "SPLITK_SMALL", "": "ONE_TILE"})
    # 258 tiles of K = 512: TVC_GEMM_SPLITK_TAIL=1 runs one whole ring round and splits the 2 left-over tiles 2 ways;
    # by default ring form 1 (J % 256 != 0)
    + _family("tail", {0: 256, 1: 253, 3: 255}, 65836, 512, {"TVC_GEMM_SPLITK_TAIL=1": "SPLITK_TAIL", "": "RING1"})
)
RING = ("RING1", "RING4")
SPLIT = ("SPLITK_SMALL", "SPLITK_TAIL")


# ------------------------------------------------------------------------------------------------------------ helpers
def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _checksum(t):
    b = _bits(t).to(torch.int64)
    return int((b * (torch.arange(b.numel(), device=b.device).view(b.shape) % 1000003 + 1)).sum().item())


def _guarded(J, I, ldo, dtype, dev, base=None):
    """(buffer, out view): out = rows [G, G + J) x columns [0, I) of a sentinel-filled (G + J + G) x ldo buffer."""
    sent, idt = (SENT32, torch.int32) if dtype == torch.float32 else (SENT16, torch.int16)
    buf = torch.full((G + J + G, ldo), sent, dtype=idt, device=dev).view(dtype)
    out = buf[G:G + J, :I]
    if base is not None:
        out.copy_(base)
    return buf, out


def _check_guards(buf, J, I, what):
    b = _bits(buf)
    sent = SENT32 if b.dtype == torch.int32 else SENT16
    assert bool((b[:G] == sent).all()), f"{what}: a write into the {G} rows before the output"
    assert bool((b[G + J:] == sent).all()), f"{what}: a write into the {G} rows after the output"
    assert bool((b[G:G + J, I:] == sent).all()), f"{what}: a write into columns [I, ld_out)"


def _operand(rows, K, ld, dtype, gen, scale, dev):
    """[rows, ld] of which the first K columns are random (rounded to dtype) and the padding is NaN."""
    x = (torch.randn((rows, ld), device=dev, generator=gen) * scale).to(dtype)
    x[:, K:] = float("nan")
    return x


def _run_case(eng, c, dtype, dev="cuda:0"):
    """Every check of one case in one dtype; returns {epilogue: checksum of the output bits}."""
    I, J, K = c["I"], c["J"], c["K"]
    gen = torch.Generator(device=dev).manual_seed(1000 + CASES.index(c))
    a = _operand(I, K, c["lda"], dtype, gen, K ** -0.5, dev)
    b = _operand(J, K, c["ldb"], dtype, gen, 1.0, dev)
    bias = torch.randn(I, device=dev, generator=gen) if c["bias"] else None
    gemm = eng.gemm if dtype == torch.bfloat16 else eng.gemm_f16
    ref = b[:, :K].double() @ a[:, :K].double().t()
    if bias is not None:
        ref += bias.double()
    what = f"{c['id']} {dtype} I={I} J={J} K={K} lda={c['lda']} ldb={c['ldb']} ldo={c['ldo']}"

    def run(epi, base=None):
        buf, out = _guarded(J, I, c["ldo"], torch.float32 if epi in (0, 3) else dtype, dev, base)
        r = gemm(a, b, bias, epi, out=out, k=K)
        assert r.data_ptr() == out.data_ptr()
        _check_guards(buf, J, I, f"{what} epi={epi}")
        return out

    sums = {}
    e0 = run(0)
    sums[0] = _checksum(e0)
    e0d = e0.double()
    assert bool(torch.isfinite(e0d).all()), f"{what}: non-finite output (padding read?)"
    err = (e0d - ref).abs().max().item()
    assert err < 2e-6 * (1 + ref.abs().max().item()), f"{what}: epi 0 max|err| {err:.3e}"
    epi = c["epi"]
    if epi == 1:
        e1 = run(1)
        assert torch.equal(_bits(e1), _bits(e0.to(dtype))), f"{what}: epi 1 is not RNE of the epi-0 output"
        sums[1] = _checksum(e1)
    elif epi == 2:
        e2 = run(2).double()
        q = e0d * torch.sigmoid(1.702 * e0d)
        ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10        # one rounding, an ulp where the fp32 value is near a tie
        assert bool(((e2 - q).abs() <= q.abs() * ulp + 1e-5).all()), f"{what}: epi 2 off QuickGELU(epi 0)"
        sums[2] = _checksum(e2.to(dtype))
    elif epi == 3:
        base = torch.randn((J, I), device=dev, generator=gen)
        e3 = run(3, base).double()
        bd = base.double()
        bound = 2.0 ** -23 * (bd.abs() + e0d.abs() + (bias.double().abs() if bias is not None else 0) + (bd + e0d).abs())
        assert bool(((e3 - (bd + e0d)).abs() <= bound).all()), f"{what}: epi 3 != base + epi 0"
        sums[3] = _checksum(e3.float())
    return sums


def _child_main(env_key):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import importlib
    pkg = importlib.import_module("multimodal-detection-consistency_amd")
    eng = pkg.TVCEngine(device="cuda:0")
    fails = 0
    for c in CASES:
        if env_key not in c["labels"]:
            continue
        for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            try:
                sums = _run_case(eng, c, dt)
            except AssertionError as ex:
                fails += 1
                print("FAIL", ex, flush=True)
                continue
            print("SUMS", json.dumps({"id": c["id"], "dt": name, "sums": sums}), flush=True)
    eng.close()
    print("CHILD_DONE fails", fails, flush=True)
    return 1 if fails else 0


# -------------------------------------------------------------------------------------------------- the GPU tests
_CHILDREN = {}


def _child(env_key):
    """Run (once per session) the child of one env switch; returns {(case id, dtype): {epilogue: checksum}}."""
    if env_key in _CHILDREN:
        return _CHILDREN[env_key]
    if any(r is None for r in _CHILDREN.values()):
        pytest.fail("an earlier child process crashed: no further GPU children are started")
    _CHILDREN[env_key] = None
    env = dict(os.environ)
    for k in ("TVC_GEMM_RING_FORM", "TVC_GEMM_VARIANT", "TVC_GEMM_SPLITK_SMALL", "TVC_GEMM_SPLITK_TAIL"):
        env.pop(k, None)
    if env_key:
        k, v = env_key.split("=")
        env[k] = v
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", env_key], cwd=root, env=env,
                       capture_output=True, text=True, timeout=300)
    fails = [ln for ln in r.stdout.splitlines() if ln.startswith("FAIL")]
    assert r.returncode in (0, 1) and "CHILD_DONE" in r.stdout, f"child {env_key!r} rc {r.returncode}: " + r.stdout[-2000:] + r.stderr[-3000:]
    sums = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("SUMS "):
            d = json.loads(ln[5:])
            sums[(d["id"], d["dt"])] = {int(k): v for k, v in d["sums"].items()}
    _CHILDREN[env_key] = (sums, fails)
    return _CHILDREN[env_key]


@pytest.mark.gpu
@pytest.mark.parametrize("env_key", ENVS)
def test_gemm16_contract_in_child(env_key):
    sums, fails = _child(env_key)
    assert not fails, "\n".join(fails[:20])
    n = sum(env_key in c["labels"] for c in CASES)
    assert len(sums) == 2 * n


@pytest.mark.gpu
def test_ring_forms_return_the_same_bits():
    """DESIGN.md 4.1 on the contract's shapes: every case that is a ring launch both by default and under
    TVC_GEMM_RING_FORM=1 (form 4 vs form 1, or form 1 vs form 1 where form 4's preconditions fail) returns the same
    bits in every epilogue, in both 16-bit types -- padded pitches (K + 64) and ld_out % 8 == 4 included."""
    d, _ = _child("")
    f1, _ = _child("TVC_GEMM_RING_FORM=1")
    keys = [c for c in CASES if c["labels"].get("") in RING and c["labels"].get("TVC_GEMM_RING_FORM=1") in RING]
    assert any(c["labels"][""] == "RING4" and c["lda"] == c["ldb"] == c["K"] + 64 for c in keys)
    assert any(c["labels"][""] == "RING4" and c["ldo"] % 8 == 4 for c in keys)
    compared = 0
    for c in keys:
        for dt in ("bf16", "fp16"):
            k = (c["id"], dt)
            assert k in d and k in f1, k
            assert d[k] == f1[k], (k, d[k], f1[k])
            compared += 1
    assert compared >= 2 * 10


@pytest.mark.gpu
@pytest.mark.parametrize("env_key", ["TVC_GEMM_SPLITK_SMALL=1", "TVC_GEMM_SPLITK_TAIL=1"])
def test_splitk_forms_really_split(env_key):
    """A split-K case is correct in its child (test_gemm16_contract_in_child), and its fp32 output bits differ in at
    least one element from the same case in the default child, which runs a one-pass kernel: the K sums were taken in
    another order, i.e. the split-K kernels ran."""
    s, _ = _child(env_key)
    d, _ = _child("")
    n = 0
    for c in CASES:
        if c["labels"].get(env_key) in SPLIT:
            assert c["labels"][""] not in SPLIT
            for dt in ("bf16", "fp16"):
                k = (c["id"], dt)
                print(f"[checksum] {k} epi 0: {env_key} {s[k][0]}  default {d[k][0]}")
                assert s[k][0] != d[k][0], k
                n += 1
    assert n >= 8


@pytest.fixture(scope="module")
def eng(pkg):
    e = pkg.TVCEngine(device="cuda:0")
    yield e
    e.close()


@pytest.mark.gpu
def test_wrappers_refuse_an_out_they_cannot_describe(eng):
    """An out of the wrong dtype, a transposed view or too few rows / columns raise instead of being written at a wrong
    pitch; a column view of a wider buffer is written at its own row stride."""
    a = torch.randn(64, 128, device="cuda:0")
    b = torch.randn(40, 128, device="cuda:0")
    for gemm, dt in ((eng.gemm, torch.bfloat16), (eng.gemm_f16, torch.float16)):
        a16, b16 = a.to(dt), b.to(dt)
        with pytest.raises(ValueError):
            gemm(a16, b16, None, 1, out=torch.empty(40, 64, device="cuda:0"))          # fp32 out, 16-bit epilogue
        with pytest.raises(ValueError):
            gemm(a16, b16, None, 0, out=torch.empty(40, 64, device="cuda:0", dtype=dt))   # 16-bit out, fp32 epilogue
        with pytest.raises(ValueError):
            gemm(a16, b16, None, 0, out=torch.empty(64, 40, device="cuda:0").t())        # column stride != 1
        with pytest.raises(ValueError):
            gemm(a16, b16, None, 0, out=torch.empty(39, 64, device="cuda:0"))
        with pytest.raises(ValueError):
            gemm(a16, b16, None, 0, out=torch.empty(40, 63, device="cuda:0"))
        buf, out = _guarded(40, 64, 100, torch.float32, "cuda:0")
        gemm(a16, b16, None, 0, out=out)
        _check_guards(buf, 40, 64, "column view")
        ref = b16.double() @ a16.double().t()
        assert (out.double() - ref).abs().max().item() < 2e-6 * (1 + ref.abs().max().item())
    with pytest.raises(ValueError):
        eng.gemm_f32(a, b, None, 0, out=torch.empty(40, 64, device="cuda:0", dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        eng.gemm_f32(a, b, None, 0, out=torch.empty(64, 40, device="cuda:0").t())


@pytest.mark.gpu
def test_gemm16_refuses_misaligned_and_overpitched_operands(eng, pkg):
    """tvc.h: a_dev, b_dev, out_dev and a non-NULL bias_dev 16-byte aligned, lda / ldb below 2^23 -- refused with
    TVC_E_INVALID before any launch (the over-pitched calls are one-row launches, in bounds even if they ran)."""
    lib = eng.lib
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = torch.zeros(64 * 64 + 64, dtype=torch.bfloat16, device="cuda:0")
    b = torch.zeros(64 * 64 + 64, dtype=torch.bfloat16, device="cuda:0")
    bias = torch.zeros(128, device="cuda:0")
    out = torch.zeros(64 * 64 + 64, device="cuda:0")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    invalid = pkg._lib.TVC_E_INVALID
    for fn in (lib.tvc_gemm_bf16, lib.tvc_gemm_f16):
        for args in ((p(a, 2), p(b), p(bias), p(out), 64, 64, 64, 64, 64, 64, 0),
                     (p(a), p(b, 8), p(bias), p(out), 64, 64, 64, 64, 64, 64, 0),
                     (p(a), p(b), p(bias, 4), p(out), 64, 64, 64, 64, 64, 64, 0),
                     (p(a), p(b), p(bias), p(out, 8), 64, 64, 64, 64, 64, 64, 1),
                     (p(a), p(b), None, p(out), 1, 1, 64, 1 << 23, 64, 64, 0),
                     (p(a), p(b), None, p(out), 1, 1, 64, 64, (1 << 23) + 8, 64, 0)):
            assert fn(eng.handle, *args, st) == invalid, args
    torch.cuda.synchronize()
    assert bool((out == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("I,J,K", [(300, 77, 132), (257, 300, 64), (256, 513, 256)])
def test_gemm_f32_guard_bands_and_pitch(eng, I, J, K):
    """tvc_gemm_f32 (epilogues 0 / 1 / 2) into [J, I] views of sentinel buffers at ld_out = I, I + 1, I + 4, I + 64, I % 4
    in {0, 1, 3}: nothing outside the view changes; fp64 references and bounds of test_gpu_fp32_mode.py."""
    g = torch.Generator(device="cuda:0").manual_seed(I + J + K)
    w = torch.randn((I, K), device="cuda:0", generator=g)
    x = torch.randn((J, K), device="cuda:0", generator=g)
    bias = torch.randn(I, device="cuda:0", generator=g)
    ref = x.double() @ w.double().t() + bias.double()
    tol = 2e-6 * 0.2 * K
    for n, off in enumerate(LDO_OFF):
        for epi in (0, 1, 2):
            base = torch.randn((J, I), device="cuda:0", generator=g) if epi == 2 else None
            buf, out = _guarded(J, I, I + off, torch.float32, "cuda:0", base)
            eng.gemm_f32(w, x, bias if (n + epi) % 2 == 0 else None, epi, out=out)
            _check_guards(buf, J, I, f"f32 I={I} J={J} K={K} ldo=I+{off} epi={epi}")
            r = ref if (n + epi) % 2 == 0 else ref - bias.double()
            if epi == 1:
                r = r * torch.sigmoid(1.702 * r)
            if epi == 2:
                r = base.double() + r
            assert (out.double() - r).abs().max().item() < tol, (I, J, K, off, epi)


@pytest.mark.gpu
@pytest.mark.parametrize("I,J,K", [(300, 77, 132), (257, 300, 64), (255, 600, 256)])
def test_gemm_split_guard_bands_and_pitch(eng, I, J, K):
    """tvc_gemm_split (through ctypes: the wrapper picks its own pitch) into [J, I] views of sentinel buffers at ld_out =
    round_up(I, 4) + 0 / 4 / 64 with I % 4 in {0, 1, 3}; fp64 reference and bound of test_gpu_fp32_mode.py."""
    g = torch.Generator(device="cuda:0").manual_seed(I * J + K)
    w = torch.randn((I, K), device="cuda:0", generator=g)
    x = torch.randn((J, K), device="cuda:0", generator=g)
    bias = torch.randn(I, device="cuda:0", generator=g)
    ref = x.double() @ w.double().t() + bias.double()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for off in (0, 4, 64):
        ldo = (I + 3) // 4 * 4 + off
        buf, out = _guarded(J, I, ldo, torch.float32, "cuda:0")
        rc = eng.lib.tvc_gemm_split(eng.handle, C.c_void_p(w.data_ptr()), C.c_void_p(x.data_ptr()),
                                    C.c_void_p(bias.data_ptr()), C.c_void_p(out.data_ptr()), I, J, K, ldo, st)
        assert rc == 0
        _check_guards(buf, J, I, f"split I={I} J={J} K={K} ldo={ldo}")
        assert (out.double() - ref).abs().max().item() < 6e-5 * K ** 0.5, (I, J, K, ldo)


if __name__ == "__main__" and len(sys.argv) >= 2 and sys.argv[1] == "--child":
    sys.exit(_child_main(sys.argv[2] if len(sys.argv) > 2 else ""))
