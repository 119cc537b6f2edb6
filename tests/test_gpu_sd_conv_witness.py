"""GPU: the convolutions of the latent-diffusion generator (csrc/tvc_sd.cpp: Run::conv3x3_planes, Run::conv3x3,
Run::upsample_conv behind tvc_sd_block kinds 3 / 4 / 5) on EXACT data -- tests/sd_conv_witness.py: small integers, so
every launch form and every K split must return the bits of the fp64 conv2d.  The cases reach the three launch shapes
only these callers have: nine K-planes over the padded token layout, the caller-fixed K split (in the ring-split kernel,
and in the partial and finish kernels under TVC_GEMM_RING_SPLIT=0), and ring form 4 with a ragged last row tile (ring
form 1 with nine planes under TVC_GEMM_RING_FORM=1).  tests/test_gemm_form.py proves the labels on the CPU,
tests/test_sd_conv_witness.py that the data sees a wrong tap, border, K-tile, slice, phase or column order.

One engine per 16-bit format; the handle holds ONLY the hand-made tensors (tvc_sd_load gathers no time projections without
conv_in.weight, and the block kinds used here need nothing else).  The switches are read once per process, so each runs in
one child (``python tests/test_gpu_sd_conv_witness.py --child ENV``), which asserts equality itself and prints checksums;
no further child is started after one that crashed.

Resnet blocks (kind 0) at 3 x 5 and 5 x 7, where the border rows are 20 of 35 and 28 of 63 rows of the padded grid: against
the fp64 restatement ``sd_conv_witness.resnet_ref`` within ``RESNET_BOUND``, and bit-identical whatever the arena held."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import sd_conv_witness as wit

PRECISIONS = {"bf16": torch.bfloat16, "fp16": torch.float16}


@functools.lru_cache(maxsize=None)
def _cases():
    return {cid: wit.make_case(*c, wit.SEEDS[cid]) for cid, c in wit.CASES.items()}


@functools.lru_cache(maxsize=None)
def _resnets():
    return [wit.make_resnet_case(*shape, seed=7 + shape[1]) for shape in wit.RESNET_SHAPES]


def _weights():
    """state-dict style names under made-up prefixes: "wit<id>." for the convolutions, "res<i>." for the resnet blocks"""
    w = {}
    for cid, case in _cases().items():
        w[f"wit{cid}.weight"], w[f"wit{cid}.bias"] = case["w"], case["bias"]
    for i, (t, _) in enumerate(_resnets()):
        w.update({f"res{i}.{k}": v for k, v in t.items()})
    return w


def _kernels(pkg, precision):
    eng = pkg.TVCEngine()
    return pkg.SDKernels(eng, pkg.SDArch(), _weights(), None, precision=precision)


def _run_case(k, cid, x=None):
    kind, n, Cin, Cout, H, W = wit.CASES[cid]
    return k.block(kind, f"wit{cid}.", _cases()[cid]["x"] if x is None else x, Cout).cpu()


def _checksum(t):
    b = t.contiguous().view(torch.int32).to(torch.int64).reshape(-1)
    return int((b * (torch.arange(b.numel()) % 1000003 + 1)).sum().item())


# ------------------------------------------------------------------------------------------------------ the child
def _child_main(env_key):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import importlib
    pkg = importlib.import_module("multimodal-detection-consistency_amd")
    fails = 0
    for precision in PRECISIONS:
        k = _kernels(pkg, precision)
        for cid in wit.CASES:
            if env_key not in wit.LABELS[cid]:
                continue
            got = _run_case(k, cid)
            ref = _cases()[cid]["ref"]
            if got.shape != ref.shape or not torch.equal(got.double(), ref):
                fails += 1
                bad = int((got.double() != ref).sum()) if got.shape == ref.shape else -1
                print("FAIL", cid, precision, env_key, f"{bad} of {ref.numel()} outputs differ from the fp64 conv2d", flush=True)
                continue
            print("SUMS", json.dumps({"id": cid, "dt": precision, "sum": _checksum(got)}), flush=True)
        k.engine.close()
    print("CHILD_DONE fails", fails, flush=True)
    return 1 if fails else 0


_CHILDREN = {}
_SWITCHES = ("TVC_GEMM_RING_FORM", "TVC_GEMM_VARIANT", "TVC_GEMM_SPLITK_SMALL", "TVC_GEMM_SPLITK_TAIL", "TVC_GEMM_RING_SPLIT",
             "TVC_GEMM_RING_MIN_TILES")


def _child(env_key):
    """Run (once per session) the child of one env switch; returns ({(case id, dtype): checksum}, FAIL lines)."""
    if env_key in _CHILDREN:
        if _CHILDREN[env_key] is None:
            pytest.fail(f"the child of {env_key!r} crashed")
        return _CHILDREN[env_key]
    if any(r is None for r in _CHILDREN.values()):
        pytest.fail("an earlier child process crashed: no further GPU children are started")
    _CHILDREN[env_key] = None
    env = dict(os.environ)
    for name in _SWITCHES:
        env.pop(name, None)
    name, v = env_key.split("=")
    env[name] = v
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", env_key], cwd=root, env=env,
                       capture_output=True, text=True, timeout=300)
    fails = [ln for ln in r.stdout.splitlines() if ln.startswith("FAIL")]
    assert r.returncode in (0, 1) and "CHILD_DONE" in r.stdout, f"child {env_key!r} rc {r.returncode}: " + r.stdout[-2000:] + r.stderr[-3000:]
    sums = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("SUMS "):
            d = json.loads(ln[5:])
            sums[(d["id"], d["dt"])] = d["sum"]
    _CHILDREN[env_key] = (sums, fails)
    return _CHILDREN[env_key]


# -------------------------------------------------------------------------------------------------- the GPU tests
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=list(PRECISIONS))
def k(pkg, request):
    assert not any(name in os.environ for name in _SWITCHES), "the default process runs without GEMM switches"
    kern = _kernels(pkg, request.param)
    assert kern.arch.norm_eps == wit.RESNET_EPS and kern.arch.norm_groups == wit.GROUPS
    yield kern
    kern.engine.close()


def test_block_refuses_a_cin_that_is_no_multiple_of_64(pkg, k):
    """Every GEMM behind tvc_sd_block reads whole 64-column K-tiles per plane: Cin = 8 (no K-tile at all) and Cin = 72 (eight
    columns beyond the last one) are TVC_E_INVALID for every kind before anything is launched, and the handle goes on working."""
    for kind in range(6):
        for cin in (8, 72):
            x = torch.ones((1, cin, 4, 4))
            with pytest.raises(pkg.TVCError) as e:
                k.block(kind, "witA.", x, 64, ctx=torch.zeros((1, k.arch.ctx, k.arch.cross_attention_dim)) if kind == 1 else None)
            assert e.value.code == pkg._lib.TVC_E_INVALID, (kind, cin)
    torch.cuda.synchronize()
    assert torch.equal(_run_case(k, "A").double(), _cases()["A"]["ref"])


@pytest.mark.parametrize("cid", list(wit.CASES))
def test_conv_case_equals_the_fp64_conv2d(k, cid):
    got, ref = _run_case(k, cid), _cases()[cid]["ref"]
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert torch.equal(got.cpu().double(), ref), f"{cid} {k.precision}: {int((got.double() != ref).sum())} of {ref.numel()} outputs differ"


@pytest.mark.parametrize("cid", ["A", "B"])
def test_a_sample_does_not_depend_on_its_batch(k, cid):
    """Sample 1 alone and inside its batch: the same bits (B: the K split is chosen from the per-sample shape)."""
    x = _cases()[cid]["x"]
    whole, alone = _run_case(k, cid), _run_case(k, cid, x[1:2])
    assert torch.equal(whole[1:2], alone)
    assert torch.equal(alone.double(), _cases()[cid]["ref"][1:2])


@pytest.mark.parametrize("env_key", [e for e in wit.ENVS if e])
def test_conv_cases_in_the_child_of_a_switch(k, env_key):
    """The cases labelled for a switch equal the reference in its child, and print the checksums of the default process."""
    sums, fails = _child(env_key)
    assert not fails, "\n".join(fails[:20])
    ids = [cid for cid in wit.CASES if env_key in wit.LABELS[cid]]
    assert len(ids) >= 2 and set(sums) == {(cid, p) for cid in ids for p in PRECISIONS}
    for cid in ids:
        assert sums[(cid, k.precision)] == _checksum(_run_case(k, cid)), (cid, k.precision, env_key)


@pytest.mark.parametrize("vae", [0, 1])
@pytest.mark.parametrize("i", range(len(wit.RESNET_SHAPES)))
def test_resnet_block_at_small_non_square_sizes(k, i, vae):
    """Measured on the GPU against the fp64 restatement (EXPERIMENTS.md, "Exact test of the latent-diffusion convolutions"):
    rel L2 2.68e-3 .. 3.02e-3 in bf16 and 3.35e-4 .. 3.81e-4 in fp16, max |d| / std 1.28e-2 .. 1.93e-2 and 1.91e-3 .. 2.04e-3;
    the bounds are 2x the largest of each.  Statistics over the padded grid would be off by 1.1e-1 / 4.7e-1 (the CPU test)."""
    t, x = _resnets()[i]
    n, Cin, Cout, H, W = wit.RESNET_SHAPES[i]
    got = k.block(0, f"res{i}.", x, Cout, vae=bool(vae)).cpu()
    ref = wit.resnet_ref(t, x.to(PRECISIONS[k.precision]).float(), 1e-6 if vae else wit.RESNET_EPS)
    r2, rm = wit.rel(got, ref)
    print(f"[measured] resnet {wit.RESNET_SHAPES[i]} vae={vae} {k.precision}: rel L2 {r2:.3e} max|d|/std {rm:.3e}")
    assert got.shape == ref.shape and torch.isfinite(got).all()
    b2, bm = wit.RESNET_BOUND[k.precision]
    assert b2 <= 8e-3 and bm <= 6e-2
    assert r2 < b2 and rm < bm


@pytest.mark.parametrize("what", ["res0", "res1", "A", "C"])
def test_result_does_not_depend_on_what_the_arena_held(k, what):
    """The same call after the same block on zeros and after it on 1e3 * random data: the same bits.  Border rows, split-K
    partial tiles and the rows beyond the last tile are stale memory of the call before."""
    if what.startswith("res"):
        i = int(what[3:])
        x = _resnets()[i][1]
        run = lambda v: k.block(0, f"res{i}.", v, wit.RESNET_SHAPES[i][2]).cpu()
    else:
        x = _cases()[what]["x"]
        run = lambda v: _run_case(k, what, v)
    run(torch.zeros_like(x))
    after_zeros = run(x)
    run(1e3 * torch.randn(x.shape, generator=torch.Generator().manual_seed(5)))
    after_noise = run(x)
    assert torch.isfinite(after_zeros).all() and torch.equal(after_zeros, after_noise)


if __name__ == "__main__" and len(sys.argv) >= 2 and sys.argv[1] == "--child":
    sys.exit(_child_main(sys.argv[2] if len(sys.argv) > 2 else ""))
