"""The fused projection head on exact operands, host-emulated kernels (the MI355X side is tests/test_gpu_projection_exact.py; inputs,
runners and case tables are in tests/exact_inputs.py).

`exact_inputs.projection_inputs` builds X, W and bias whose projection X W^T + bias is a set of planted sign rows Y EXACTLY in bf16-operand /
fp32-accumulate arithmetic, whatever the summation order.  Every output of crossclr_project_pack then has a closed form that fp32 holds
without rounding -- the packed operand is bfloat16(F.normalize(Y)), inv_norm is 2^-j, diag_cos the float64 cosine -- and the tests assert
EQUALITY, on outputs prefilled with garbage so that anything the kernel leaves unwritten shows:
* crossclr_project_pack / crossclr_project_pack_wf (row-major and fragment-major weights: the same bytes) at every padded width, Din below
  one chunk / no multiple of 16 / odd / different per modality / below D, four input dtypes, strided and misaligned rows, bias on both, one
  or no modality, an all-zero row; ONE launch of the 64-rows-per-block instantiation (b = 16300, Dpad 128; `slow`: the others run on the
  MI355X only);
* crossclr_project_dw on inputs whose every partial sum is exact: dW and db equal the float64 products for one to eight splits, a last
  split of one row, empty splits, the narrower modality's early return, every stride above its width, NULL bias gradients, four dtypes;
* g_y from the prenormalized = 2 finish (the way projection.py obtains it), element by element against the two-rounding weight model at
  (Y_v, Y_t): |got - want| <= 2^-8 |want| (the output's one bf16 rounding) + GRAD_BAR["bf16"] x the row's largest entry + the row's tie
  allowance;
* projected_crossclr_loss end to end: loss at LOSS_BAR against the exact closed form; dx / dW / db per element against the chain from the
  model's g_y (not rounded to bf16), within what the element-wise bound on g_y allows their sums;
* crossclr_project_backward_prep (the two-step normalise-backward of the C-ABI, which the module no longer calls) against float64 from the
  same packed rows, per row, strides of its own per tensor, columns beyond D untouched;
* TEETH (float64 only, no kernel): in every g_y case a dropped 32 x 32 tile of weights and the neighbouring column's statistic move some
  ELEMENT by at least 10 x its bar (no sample weights on this path: the third mutation of tests/test_exact_operands_cpu.py does not
  apply); one zeroed 16-column k-step of W -- any of them, either modality -- and a bias shifted by one column change the bit-exact
  outputs of every crossclr_project_pack case.

MEASURED on the host emulation, unmodified kernels of commit 98909ec (the MI355X figures are in the other file):
  g_y, worst (err - 2^-8 |want| - slack) / rowmax    <= 2.5e-10 in every case (the bar: 1.7e-05); the element-wise bound itself is reached
                                                     to 0.98 .. 0.99 -- an element whose significand is just above a power of two, half a unit off
  crossclr_project_backward_prep, worst row          6.04e-08 in the three cases (PREP_BAR = 4 x that)
  end to end, worst err / bound                      dx 0.76, dW 0.34, db 0.17 (three cases)
  teeth                                              a dropped tile moves an element by 480 .. 7700 of its bars, the neighbouring column's
                                                     statistic by > 1e12
"""
import pytest
import torch
import torch.nn.functional as F

import exact_inputs as xi
from crossclr_amd import _native as nat
from oracle import crossclr_oracle as orc


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    from emu import build_emu
    nat.use_library_for_testing(build_emu.build())
    yield
    nat.use_library_for_testing(None)


@pytest.mark.parametrize("b,D,din_v,din_t", [(70, 100, 100, 104), (70, 16, 24, 24), (130, 100, 101, 101), (70, 128, 32, 32), (130, 600, 640, 700)])
def test_projection_inputs_are_exact(b, D, din_v, din_t):
    case = xi.projection_inputs(b, D, din_v, din_t)      # (asserts its own conditions)
    for x, w, bias, y, din in zip(case["x"], case["w"], case["bias"], case["y"], (din_v, din_t)):
        assert x.shape == (b, din) and w.shape == (D, din) and bias.shape == (D,)
        assert torch.equal(x, x.round()) and x.abs().max() <= 128 and set(bias.unique().tolist()) <= {-1.0, 0.0, 1.0}
        nz = w[w != 0].abs()
        assert torch.equal(torch.exp2(torch.log2(nz).round()), nz), "weights are +-2^-k"
        assert int((w != 0).sum(1).max()) == xi.hadamard_blocks(din)[0], "a weight row has as many non-zeros as its block has columns"
        assert torch.equal(F.linear(x, w, bias), y)
    assert xi.hadamard_blocks(101) == [64, 32, 4, 1] and xi.hadamard_blocks(24) == [16, 8]


@pytest.mark.parametrize("c", xi.PACK_CASES, ids=xi.pack_id)
def test_project_pack_bit_for_bit(c):
    plan = xi.run_pack_case(c, "cpu")
    assert plan.bpad in (128, 256) and plan.bpad // 64 < 256        # 32 rows per block


@pytest.mark.slow
def test_project_pack_64_rows_per_block_bit_for_bit():
    plan = xi.run_pack_case(xi.PACK_CASES_64[0], "cpu")
    assert plan.bpad // 64 >= 256 and plan.Dpad <= 512 and plan.Dpad == 128 and plan.b == 16300


@pytest.mark.parametrize("c", xi.DW_CASES, ids=xi.dw_id)
def test_project_dw_equals_the_float64_products(c):
    xi.run_dw_case(c, "cpu")


# (the two large cases take the emulated saved backward 20 s: `slow`; end to end the emulated crossclr_project_dw takes them minutes
#  -- 512 thread blocks at D = Din = 1024 --: those two run end to end on the MI355X only)
EMULATED_GY_CASES = [pytest.param(*c, marks=pytest.mark.slow) if c[0] * c[1] > 100000 else c for c in xi.GY_CASES]
EMULATED_END_TO_END = [c for c in xi.GY_CASES if c[0] * c[1] <= 100000]


@pytest.mark.parametrize("b,D,din_v,din_t,tau,w", EMULATED_GY_CASES)
def test_gy_of_the_fused_finish_element_by_element(b, D, din_v, din_t, tau, w):
    case = xi.gy_case(b, D, din_v, din_t)
    want, bar, m = xi.gy_yardstick(case, tau, w)
    loss, gyv, gyt, kernels = xi.projected_gy_via_impl(case, tau, w, "cpu")
    assert gyv.dtype == torch.bfloat16 and gyt.dtype == torch.bfloat16 and gyv.shape == (b, D) and gyt.shape == (b, D)
    xi.check_gy(torch.cat([gyv, gyt]), want, bar, m, f"b={b} D={D} Din={din_v}x{din_t} tau={tau} {kernels[1]}")
    assert xi.slack_fraction(m, xi.GRAD_BAR["bf16", False, True]) <= xi.SLACK_ROWS_MAX


@pytest.mark.parametrize("b,D,din_v,din_t,tau,w", EMULATED_END_TO_END)
def test_projected_loss_end_to_end(b, D, din_v, din_t, tau, w):
    xi.check_projected_end_to_end(xi.gy_case(b, D, din_v, din_t), tau, w, "cpu", f"b={b} D={D} Din={din_v}x{din_t} tau={tau}")


@pytest.mark.parametrize("b,D,din_v,din_t", xi.PREP_CASES)
def test_backward_prep_against_float64(b, D, din_v, din_t):
    xi.check_backward_prep(xi.pack_case(b, D, din_v, din_t, xi.BOTH if b == 70 else (False, True), None), "cpu", f"b={b} D={D}")


# ----------------------------------------------------------------------------------------------------------------------------------
# teeth
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,D,din_v,din_t,tau,w", xi.GY_CASES)
def test_teeth_every_gy_case_shows_every_defect_at_ten_element_bars(b, D, din_v, din_t, tau, w):
    case = xi.gy_case(b, D, din_v, din_t)
    want2, bar, _ = xi.gy_yardstick(case, tau, w)
    clean = orc.stacked_weight_model(case["y"][0], case["y"][1], tau, w)
    assert torch.equal(xi.defective_weights(clean), clean["W"])
    want = torch.cat(orc.grads_from_stacked_weights(clean))
    defects = {}
    for name, (rows, cols) in xi.tiles(b).items():
        Wd = clean["W"].clone()
        Wd[rows, cols] = 0.0
        defects["tile dropped: " + name] = Wd
    defects["column statistics of the neighbouring column"] = xi.defective_weights(clean, col_stat_shift=1)
    for name, Wd in defects.items():
        moved = (torch.cat(orc.grads_from_stacked_weights(clean, Wd)) - want).abs() / bar      # (the bar of the element, from the rounded model)
        print(f"{name}: an element moves by {float(moved.max()):.0f} of its bars")
        assert float(moved.max()) >= 10.0, name


@pytest.mark.parametrize("c", [c for c in xi.PACK_CASES if c[6] == xi.F32 and c[7] == "contiguous"], ids=xi.pack_id)
def test_teeth_projection_defects_change_the_bit_exact_outputs(c):
    """one 16-column k-step of W zeroed (every k-step of either modality in turn), the bias shifted by one column: some packed element,
    inv_norm or cosine of the yardstick changes -- the equalities of test_project_pack_bit_for_bit cannot hold for such a kernel"""
    b, D, din_v, din_t, _Dpad, bias, _dtype, _layout, zero_row = c
    case = xi.pack_case(b, D, din_v, din_t, bias, zero_row)
    clean = xi.projection_expected(*case["y"])
    same = lambda yv, yt: all(torch.equal(p, q) for p, q in zip(xi.projection_outputs(yv, yt), clean))
    assert same(*case["y"])
    for mod in range(2):
        x, w, y = case["x"][mod].double(), case["w"][mod].double(), case["y"][mod].double()
        for k0 in range(0, case["live"][mod], 16):      # (input columns from `live` on are zero: no block of theirs holds a column of Y)
            yd = y - x[:, k0:k0 + 16] @ w[:, k0:k0 + 16].t()
            ys = [case["y"][0].double(), case["y"][1].double()]
            ys[mod] = yd
            assert not same(*ys), f"modality {mod}: k-step at column {k0} zeroed, outputs unchanged"
        if case["bias"][mod] is not None:
            bvec = case["bias"][mod].double()
            ys = [case["y"][0].double(), case["y"][1].double()]
            ys[mod] = y - bvec + torch.roll(bvec, 1)
            assert not same(*ys), f"modality {mod}: bias of the neighbouring column, outputs unchanged"
