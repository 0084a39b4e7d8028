"""The fused projection head on the MI355X, on exact operands (tests/exact_inputs.py: `projection_inputs` and the runners; the emulated side
and the teeth are in tests/test_projection_exact_cpu.py).  X, W and bias are such that X W^T + bias is a set of planted sign rows Y EXACTLY
in bf16-operand / fp32-accumulate arithmetic in any summation order, so every output of crossclr_project_pack has a closed form without
rounding and is held to EQUALITY, on outputs prefilled with garbage:
* crossclr_project_pack / crossclr_project_pack_wf, the cases of the emulated file (every padded width, ragged / odd / unequal Din, Din < D,
  fp32 / bf16 / fp16 / fp64 inputs, strided and misaligned rows, partial bias, an all-zero row) AND the 64-rows-per-block instantiations,
  which only start at bpad >= 16384 (project_pack_t: bpad / 64 >= 256, Dpad <= 512): b = 16300 and 16385 at every Dpad of 128 .. 512
  with fp32 and bf16 inputs, fp16 and fp64 at one width each, both weight layouts.  The yardstick is O(b D) on the host;
* crossclr_project_dw: dW and db equal the float64 products (every partial sum is exact) over the split geometries of exact_inputs.DW_CASES;
* g_y of the prenormalized = 2 finish, per element: |got - want| <= 2^-8 |want| + GRAD_BAR["bf16"] rowmax + the row's tie allowance,
  want = the two-rounding weight model at (Y_v, Y_t);
* projected_crossclr_loss end to end (loss against the exact closed form; dx, dW, db against the chain from the model's g_y; neither crossclr_normalize, crossclr_pack nor crossclr_project_backward_prep may run);
* crossclr_project_backward_prep against float64 from the same packed rows.

MEASURED on the MI355X, unmodified kernels of commit 98909ec, 2026-10-19:
  crossclr_project_pack / _wf, crossclr_project_dw   every case equal, the twenty 64-rows-per-block launches included
  g_y, worst (err - 2^-8 |want| - slack) / rowmax    2.5e-10 (b = 300, D = 600; the other cases <= 1.6e-11), against the bar 1.7e-05; the
                                                     whole element-wise bound is reached to 0.98 .. 0.99 of its value: an element whose
                                                     significand is just above a power of two, rounded to bf16 half a unit off
  crossclr_project_backward_prep, worst row          6.04e-08, 4.23e-08, 3.98e-08 (the host emulation gives the same figures): PREP_BAR = 2.4e-07
  end to end                                         loss <= 2.1e-08; worst err / bound over the five cases: dx 0.76, dW 0.37, db 0.24
                                                     (the same gradients against the chain from the exact closed form's g_y, which lacks
                                                     the bf16 roundings of the saved backward's weights: dx up to 3.77 of that bound)
"""
import pytest
import torch

import exact_inputs as xi
from crossclr_amd import _native as nat

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _hip_only():
    nat.use_library_for_testing(None)
    assert nat.backend() == "hip-gfx950", "GPU tests must run the HIP library"
    yield


@pytest.mark.parametrize("c", xi.PACK_CASES, ids=xi.pack_id)
def test_project_pack_bit_for_bit(c):
    plan = xi.run_pack_case(c, "cuda")
    assert plan.bpad in (128, 256) and plan.bpad // 64 < 256        # 32 rows per block


@pytest.mark.parametrize("c", xi.PACK_CASES_64, ids=xi.pack_id)
def test_project_pack_64_rows_per_block_bit_for_bit(c):
    """project_pack_kernel<TIN, DKP, RF = 2>: no other test reaches these instantiations (bench.py runs b = 8192: 32 rows per block)"""
    plan = nat.make_plan(c[0], c[1], 1, 0, nat.MODE_BF16)
    # (a change of the threshold must not silently turn this into a 32-row test)
    assert plan.bpad // 64 >= 256 and plan.Dpad <= 512 and plan.bpad == {16300: 16384, 16385: 16512}[c[0]]
    xi.run_pack_case(c, "cuda")


@pytest.mark.parametrize("c", xi.DW_CASES, ids=xi.dw_id)
def test_project_dw_equals_the_float64_products(c):
    xi.run_dw_case(c, "cuda")


@pytest.mark.parametrize("b,D,din_v,din_t,tau,w", xi.GY_CASES)
def test_gy_of_the_fused_finish_element_by_element(b, D, din_v, din_t, tau, w):
    case = xi.gy_case(b, D, din_v, din_t)
    want, bar, m = xi.gy_yardstick(case, tau, w)
    loss, gyv, gyt, kernels = xi.projected_gy_via_impl(case, tau, w, "cuda")
    assert gyv.dtype == torch.bfloat16 and gyt.dtype == torch.bfloat16 and gyv.shape == (b, D) and gyt.shape == (b, D)
    xi.check_gy(torch.cat([gyv, gyt]), want, bar, m, f"b={b} D={D} Din={din_v}x{din_t} tau={tau} {kernels[1]}")
    assert xi.slack_fraction(m, xi.GRAD_BAR["bf16", False, True]) <= xi.SLACK_ROWS_MAX


@pytest.mark.parametrize("b,D,din_v,din_t,tau,w", xi.GY_CASES)
def test_projected_loss_end_to_end(b, D, din_v, din_t, tau, w, monkeypatch):
    lib = nat.library()

    def boom(*a):
        raise AssertionError("a separate normalisation / normalise-backward pass was launched on the fused-projection path")
    monkeypatch.setattr(lib, "crossclr_normalize", boom, raising=False)
    monkeypatch.setattr(lib, "crossclr_pack", boom, raising=False)
    monkeypatch.setattr(lib, "crossclr_project_backward_prep", boom, raising=False)     # the finish kernel writes g_y itself (prenormalized = 2)
    xi.check_projected_end_to_end(xi.gy_case(b, D, din_v, din_t), tau, w, "cuda", f"b={b} D={D} Din={din_v}x{din_t} tau={tau}")


@pytest.mark.parametrize("b,D,din_v,din_t", xi.PREP_CASES)
def test_backward_prep_against_float64(b, D, din_v, din_t):
    xi.check_backward_prep(xi.pack_case(b, D, din_v, din_t, xi.BOTH if b == 70 else (False, True), None), "cuda", f"b={b} D={D}")
