"""GPU tests of compute_mode="bf16x3" (fp32-accurate products on the bf16 matrix cores: hi/lo split operand, three bf16 MFMAs per
product; include/crossclr.h ABI 8) on the MI355X: every float32 reference golden at the fp32 mode's bars (full arrays for B <= 256,
sampled rows + norms beyond), determinism, and the double backward behind a bf16x3 step."""
import os

import numpy as np
import pytest
import torch

import crossclr_amd
from conftest import golden_arrays, golden_index, golden_inputs
from crossclr_amd import _native as nat
from test_bf16x3_cpu import bars
from test_second_order_cpu import CASES, GOLDEN, second_order_through_the_module

pytestmark = pytest.mark.gpu
IDX = golden_index()
F32 = [n for n, m in IDX.items() if m["dtype"] == "float32"]


@pytest.fixture(autouse=True)
def _hip_only():
    nat.use_library_for_testing(None)
    assert nat.backend() == "hip-gfx950", "GPU tests must run the HIP library"
    yield


def run(v, t, m):
    crit = crossclr_amd.CrossCLR_onlyIntraModality(m["temperature"], m["negative_weight"], compute_mode="bf16x3").cuda()
    vd, td = v.cuda().requires_grad_(True), t.cuda().requires_grad_(True)
    loss = crit(vd, td)
    loss.backward()
    torch.cuda.synchronize()
    return loss, vd.grad, td.grad


@pytest.mark.parametrize("name", F32)
def test_goldens_at_the_fp32_bars(name):
    m = IDX[name]
    v, t = golden_inputs(m)
    loss, gv, gt = run(v, t, m)
    lib = nat.library()
    assert lib.crossclr_last_kernel(0).startswith(b"fwd_sums_kernel<x3_t>")
    assert lib.crossclr_last_kernel(1).startswith((b"bwd_saved_x3_kernel", b"bwd_kernel<x3_t>"))
    ltol, gtol = bars(m)
    assert abs(loss.item() - m["loss"]) <= ltol, (loss.item(), m["loss"])
    arr = golden_arrays(name)
    if m["B"] <= 256:
        assert np.abs(gv.double().cpu().numpy() - arr["grad_v"].astype(np.float64)).max() <= gtol
        assert np.abs(gt.double().cpu().numpy() - arr["grad_t"].astype(np.float64)).max() <= gtol
    elif m["loss"] > 1e-3:
        rows = arr["rows"]
        assert np.abs(gv[rows].double().cpu().numpy() - arr["grad_v_rows"]).max() <= gtol
        assert np.abs(gt[rows].double().cpu().numpy() - arr["grad_t_rows"]).max() <= gtol
        assert abs(gv.double().norm().item() - m["grad_v_norm"]) <= 1e-3 * m["grad_v_norm"]
        assert abs(gt.double().norm().item() - m["grad_t_norm"]) <= 1e-3 * m["grad_t_norm"]


@pytest.mark.parametrize("name", ["g3_b256_d512_s2", "g6_tau0005_b2048_d512"])
def test_two_identical_steps_are_bit_identical(name):
    m = IDX[name]
    v, t = golden_inputs(m)
    a, b = run(v, t, m), run(v, t, m)
    assert a[0].item() == b[0].item() and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("name", sorted(CASES))
def test_gradient_penalty_step_behind_bf16x3(name):
    m = CASES[name]
    want = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    got = second_order_through_the_module(m, dev="cuda", mode="bf16x3")
    assert abs(got["loss"].item() - m["loss"]) <= 2e-5 * max(1.0, abs(m["loss"])) + 2e-8 / m["temperature"]
    two_pass = max(1.0, abs(m["negative_weight"])) / m["temperature"] > 128      # (twice the bar there, as for the first-order gradients)
    for key, tol in (("gv", 2e-4), ("gt", 2e-4), ("hv", 2e-4), ("ht", 2e-4), ("pv", 2e-4), ("pt", 2e-4)):
        tol *= 2 if two_pass else 1
        scale = max(np.abs(want[key[0] + "v"]).max(), np.abs(want[key[0] + "t"]).max())
        assert np.abs(got[key].double().numpy() - want[key]).max() <= tol * scale + 1e-7 / (m["B"] * m["temperature"]), key
