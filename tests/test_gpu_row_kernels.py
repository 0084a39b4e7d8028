"""The row kernels alone on the MI355X (case tables, synthetic inputs, float64 closed forms, C-ABI runners and checkers are in
tests/row_kernel_cases.py; the emulated subset and the teeth are in tests/test_row_kernels_cpu.py).  Eleven C-ABI entry points read or write
the caller's own tensors through (pointer, row stride, in_dtype); each is run ALONE on a hand-made gbuf / inv_norm / best_index / hinge /
active, in the four input dtypes, on contiguous, strided (ld+1, ld+3) and offset rows with NaN between them, into NaN-prefilled outputs
with a row stride of their own, and every element is held to the derived bar
    |got - want| <= 1/2 ulp_T(max(|want|, |got|)) + 2^-24 |want| + 1e-12 A
against a float64 closed form of the values after their conversion to the dtype (row_kernel_cases.py has the derivation).  Reached here
and nowhere else on the device: misaligned fp32 rows (row_load4<float> / row_store4<float> choose per row between a 16-byte access and
the element-wise loop), 16-bit and fp64 rows with a row stride, 16-bit and fp64 rows beyond 1024 columns, each KC of
bwd_finish_pair_kernel against bwd_finish_kernel (crossclr_last_kernel(2)), the stage loop (b > 2048) and the slab loop (D > 1024) of
hardneg_backward_kernel, and crossclr_maxmargin_backward_finish at all.

MEASURED on the MI355X, worst err / bar per family (the bars are the derived ones, not re-tuned):
(211 cases; a ratio of 1.000 is a value a hair under the bar: a correctly rounded 16-bit element whose float64 value lies next to a
  rounding tie uses all of its half unit)
  family                                   fp32     fp16     bf16     fp64
  pairloss_backward_finish_kernel          0.500    1.000    1.000    0.000   (dscale within 1e-12 of the sum of its absolute terms)
  crossclr_backward_finish_w / _p          0.500    1.000    1.000    0.000
  crossclr_maxmargin_backward_finish       0.499    0.999    1.000    0.000
  crossclr_hardneg_backward                0.480    0.998    0.993    0.000   (fp64: every element equal)
  lay-out kernels, sign rows               bit for bit in every case (packed rows, padding, inv_norm, diag_cos; _xf halves; crossclr_topk_pack)
  lay-out kernels, random rows             1.000 in all four input dtypes (the packed element's bf16 / split-operand rounding)
Two cases that no other test holds: an entry of best_index = -1 with a positive hinge adds nothing to any row of
crossclr_hardneg_backward (test_hardneg_backward, row 4 of grad_im), and crossclr_maxmargin_backward_finish divides by B * B in full
precision (test_maxmargin_backward_finish, the float64 cases: a float reciprocal of B / 2 is 2^-24 off).
crossclr_last_kernel(2) reports the template's name without KC: the assertion tells bwd_finish_pair_kernel from bwd_finish_kernel; which
KC ran follows from the shape table (row_kernel_cases.STRETCHES) and the host's switch on D.
"""
import pytest

import row_kernel_cases as rk
from crossclr_amd import _native as nat

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _hip_only():
    nat.use_library_for_testing(None)
    assert nat.backend() == "hip-gfx950", "GPU tests must run the HIP library"
    yield


@pytest.mark.parametrize("c", rk.FINISH_CASES, ids=rk.case_id)
def test_pairloss_backward_finish(c):
    assert rk.check_pairloss_case(*c, "cuda") <= 1.0


@pytest.mark.parametrize("c", rk.FINISH_CASES + [rk.WORLD3_CASE + (3,)], ids=rk.case_id)
def test_backward_finish(c):
    assert rk.check_finish_case(*c[:5], "cuda", world=c[5] if len(c) > 5 else 1) <= 1.0


@pytest.mark.parametrize("c", rk.MAXMARGIN_CASES, ids=rk.case_id)
def test_maxmargin_backward_finish(c):
    assert rk.check_maxmargin_case(*c, "cuda") <= 1.0


@pytest.mark.parametrize("c", rk.HARDNEG_CASES, ids=rk.case_id)
def test_hardneg_backward(c):
    assert rk.check_hardneg_case(*c, "cuda") <= 1.0


@pytest.mark.parametrize("c", rk.LAYOUT_CASES, ids=rk.case_id)
def test_layout_kernels(c):
    assert rk.check_layout_case(*c, "cuda") <= 1.0
