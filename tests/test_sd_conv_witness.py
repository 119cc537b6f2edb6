"""CPU: the witness data of tests/test_gpu_sd_conv_witness.py can see the faults it is there for.  On every case of the GPU
file the builder's exactness and coverage rules hold, tests/sd_conv_witness.py's restatement of tvc_sd.cpp's address
arithmetic equals the fp64 conv2d bit for bit, and every single-line defect of that restatement changes at least one
output integer -- so a GPU result equal to the reference rules each of them out.

Two defects are vacuous at a case's own launch geometry: the slice defects where the GEMM does not split K (S = 1), and
the second-row-tile bias where Cout <= 256 leaves one row tile.  The model takes S and the row tile as parameters, so
these are evaluated at the nearest geometry where they are not (the smallest S >= 2 that divides the K-tile count; a
32-row tile): the DATA would show them.  ``test_every_defect_is_red_at_a_gpu_geometry`` then asserts that each defect is
red on at least one case at exactly the S and the 256-row tile the GPU runs.  What is left is listed in ``EXEMPT``."""
import numpy as np
import pytest
import torch

import sd_conv_witness as wit

# (defect, case) pairs a defect cannot touch, with the reason; at most two per defect
EXEMPT = {
    ("hw_swapped_conv", "B"): "H = W = 4: swapping H and W changes no address",
    ("hw_swapped_conv", "C"): "H = W = 8: swapping H and W changes no address",
    ("hw_swapped_up", "I"): "H = W = 2: swapping H and W changes no address",
    ("hw_swapped_im2col", "G"): "H = W = 8: swapping H and W changes no address",
}


@pytest.fixture(scope="module")
def cases():
    out = {}
    for cid, c in wit.CASES.items():
        case = wit.make_case(*c, wit.SEEDS[cid])
        case["rows"] = wit.conv3x3_rows(case["w"].numpy())
        out[cid] = case
    return out


def _model(case, defect=None, S=1, row_tile=256):
    return wit.planes_model(case["x"].numpy(), case["rows"], case["bias"].numpy(), case["kind"], defect, S, row_tile)


def _gpu_S(cid):
    return max(1, wit.LABELS[cid][""][1])


def _nk64(cid):
    g = wit.gemm_shape(*wit.CASES[cid])
    return g["K"] * g["planes"] // 64


def _defect_geometry(defect, cid):
    """(S, row tile) a defect is evaluated at on a case: the GPU's own where the defect can act there."""
    S, tile = _gpu_S(cid), 256
    if defect in wit.SLICE_DEFECTS and S == 1:
        S = next(s for s in range(2, _nk64(cid) + 1) if _nk64(cid) % s == 0)
    if defect == "bias_second_row_tile" and wit.CASES[cid][3] <= 256:
        tile = 32
    return S, tile


def test_builder_rules_hold_on_every_gpu_case(cases):
    for cid, case in cases.items():
        wit.check_rules(case)                                        # (make_case asserted them already)
        kind, n, Cin, Cout, H, W = wit.CASES[cid]
        Ho, Wo = {3: (H, W), 4: ((H + 1) // 2, (W + 1) // 2), 5: (2 * H, 2 * W)}[kind]
        assert tuple(case["ref"].shape) == (n, Cout, Ho, Wo)
        assert case["ref"].dtype == torch.float64
    # case A keeps the 12 entries per channel: its outputs stay below 12 * 2 * 3 + 8
    assert (cases["A"]["rows"] != 0).sum(1).max() <= 12 and cases["A"]["ref"].abs().max().item() <= 80


def test_model_equals_the_reference_bit_for_bit(cases):
    for cid, case in cases.items():
        ref = case["ref"].numpy()
        for S in sorted({1, _gpu_S(cid)}):
            assert np.array_equal(_model(case, None, S), ref), (cid, S)
        assert np.array_equal(_model(case, None, 1, 32), ref), cid


def test_every_defect_changes_an_output_integer(cases):
    assert set(wit.DEFECTS) >= {"tap_shift_w", "tap_shift_w1", "tap_ky_kx_swapped", "out_shift_w2", "border_reads_neighbour",
                                "last_ktile_dropped", "slice_boundary_off_by_one", "slice_summed_twice", "plane_not_advanced",
                                "stride2_phase_1", "upsample_round_up", "bias_second_row_tile", "weight_cols_ci_major"}
    red = {d: 0 for d in wit.DEFECTS}
    for defect, kinds in wit.DEFECTS.items():
        for cid, case in cases.items():
            if case["kind"] not in kinds:
                continue
            S, tile = _defect_geometry(defect, cid)
            got, ref = _model(case, defect, S, tile), case["ref"].numpy()
            assert got.shape == ref.shape
            changed = int((got != ref).sum())
            if (defect, cid) in EXEMPT:
                assert changed == 0, f"{defect} on {cid} is listed as exempt but changes {changed} outputs"
                continue
            assert changed >= 1, f"{defect} leaves case {cid} unchanged"
            assert np.array_equal(got, np.round(got))                 # ... by whole integers
            red[defect] += 1
    assert all(v >= 1 for v in red.values()), red
    for defect in wit.DEFECTS:
        listed = [k for k in EXEMPT if k[0] == defect]
        assert len(listed) <= 2 and all(EXEMPT[k] for k in listed), defect
    assert all(d in wit.DEFECTS and c in wit.CASES and wit.CASES[c][0] in wit.DEFECTS[d] for d, c in EXEMPT)


def test_every_defect_is_red_at_a_gpu_geometry(cases):
    """At the S the GPU really splits a case by and at the 256-row tile: each defect is red on at least one case, so each is
    ruled out by a GPU run and not only by the data."""
    for defect, kinds in wit.DEFECTS.items():
        hit = []
        for cid, case in cases.items():
            if case["kind"] in kinds and (defect, cid) not in EXEMPT and _defect_geometry(defect, cid) == (_gpu_S(cid), 256):
                if not np.array_equal(_model(case, defect, _gpu_S(cid), 256), case["ref"].numpy()):
                    hit.append(cid)
        assert hit, defect
    # the slice defects are live on every split case, the bias defect on every two-row-tile case
    assert {c for c in wit.CASES if _gpu_S(c) >= 2} == {"B", "C", "G", "I"}
    assert {c for c, v in wit.CASES.items() if v[3] > 256} == {"C", "D", "J"}


def test_a_tap_across_a_sample_border_changes_an_integer(cases):
    """Sample s differs from sample s + 1 and the border rows between them are what keeps a tap of one out of the other:
    with borders that are not zero the first and the last image rows of the inner samples change."""
    case = cases["A"]
    got, ref = _model(case, "border_reads_neighbour"), case["ref"].numpy()
    assert (got[1, :, 0] != ref[1, :, 0]).any() and (got[1, :, -1] != ref[1, :, -1]).any()
    assert np.array_equal(got[:, :, 1:-1, 1:-1], ref[:, :, 1:-1, 1:-1])


@pytest.mark.parametrize("shape", wit.RESNET_SHAPES)
@pytest.mark.parametrize("vae", [0, 1])
def test_resnet_reference_sees_statistics_over_the_padded_grid(shape, vae):
    """The fp64 resnet reference with norm2's statistics taken over the padded grid deviates from the correct one by at least
    5x the GPU test's bounds, on both shapes: a GroupNorm that read the border rows cannot pass."""
    n, Cin, Cout, H, W = shape
    t, x = wit.make_resnet_case(*shape, seed=7 + Cin)
    eps = 1e-6 if vae else wit.RESNET_EPS
    x16 = x.to(torch.bfloat16).float()
    good, bad = wit.resnet_ref(t, x16, eps), wit.resnet_ref(t, x16, eps, padded_stats=True)
    r2, rm = wit.rel(bad, good)
    print(f"[measured] resnet {shape} vae={vae}: padded-grid statistics move the fp64 reference by rel L2 {r2:.2e} max|d|/std {rm:.2e}")
    for b2, bm in wit.RESNET_BOUND.values():
        assert b2 <= 8e-3 and bm <= 6e-2 and r2 >= 5 * b2 and rm >= 5 * bm
    assert (H + 2) * (W + 2) - H * W >= 0.5 * H * W                    # the border rows are no small part of the grid
