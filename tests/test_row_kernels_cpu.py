"""The row kernels alone on the host emulation (the MI355X side is tests/test_gpu_row_kernels.py; case tables, synthetic inputs, float64 closed
forms, runners and checkers are in tests/row_kernel_cases.py): the same checkers at the emulated subset -- every family at (70, 101), the
hardest-negative gather at (70, 48) and (2049, 48) (two stages, the second of ONE entry), {fp32, bf16} x {contiguous, ld+3, offset} -- and the
TEETH: each defect is applied to a copy of the float64 reference (rounded once into the output dtype, as a kernel with that defect would
write it) or to an output buffer on the host, never to a kernel, and the checker must reject it while it accepts the same data without the
defect:
  a bf16 output truncated instead of rounded; the gradient of row i formed with row i + 1's inv_norm; the positive-pair term taken from the
  row's own modality; one element written at column D; a gbuf slice skipped; the selectors of the hardest-negative gather's second stage dropped.

MEASURED on the host emulation, worst err / bar per family (the bar is the derived one of row_kernel_cases.py, never re-tuned):
  family                                   fp32     bf16
  pairloss_backward_finish_kernel          0.499    1.000
  crossclr_backward_finish_w / _p          0.499    1.000   (world = 3 included)
  crossclr_maxmargin_backward_finish       0.497    0.999
  crossclr_hardneg_backward                0.447    0.993   (after the fix of the index check; before it every case failed at row 4 of grad_im)
  lay-out kernels                          sign rows bit for bit; random rows 1.000 (a packed bf16 element next to a rounding tie)
  teeth                                    every defect rejected, the same data without it accepted
"""
import pytest
import torch

import row_kernel_cases as rk
from crossclr_amd import _native as nat


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    from emu import build_emu
    nat.use_library_for_testing(build_emu.build())
    yield
    nat.use_library_for_testing(None)


@pytest.mark.parametrize("c", rk.CPU_FINISH_CASES, ids=rk.case_id)
def test_pairloss_backward_finish(c):
    assert rk.check_pairloss_case(*c, "cpu") <= 1.0


@pytest.mark.parametrize("c", rk.CPU_FINISH_CASES + [rk.WORLD3_CASE + (3,)], ids=rk.case_id)
def test_backward_finish(c):
    assert rk.check_finish_case(*c[:5], "cpu", world=c[5] if len(c) > 5 else 1) <= 1.0


@pytest.mark.parametrize("c", rk.CPU_MAXMARGIN_CASES, ids=rk.case_id)
def test_maxmargin_backward_finish(c):
    assert rk.check_maxmargin_case(*c, "cpu") <= 1.0


# (b = 2049: 513 x 2 thread blocks of barriers, three launches: 10 s a case on an idle host, several times that on a busy one: `slow`)
@pytest.mark.parametrize("c", [pytest.param(c, marks=pytest.mark.slow) if c[0] > 1000 else c for c in rk.CPU_HARDNEG_CASES], ids=rk.case_id)
def test_hardneg_backward(c):
    assert rk.check_hardneg_case(*c, "cpu") <= 1.0


@pytest.mark.parametrize("c", rk.CPU_LAYOUT_CASES, ids=rk.case_id)
def test_layout_kernels(c):
    assert rk.check_layout_case(*c, "cpu") <= 1.0


# ----------------------------------------------------------------------------------------------------------------------------------
# teeth
# ----------------------------------------------------------------------------------------------------------------------------------
B, D = 70, 101


def accepted_and_rejected(clean, defective, A, dtype, what):
    """the checker accepts the clean reference rounded once into `dtype` and rejects the defective one"""
    rk.check_elements(clean.to(dtype), clean, A, dtype, what)
    with pytest.raises(AssertionError, match="beyond their bar"):
        rk.check_elements(defective.to(dtype), clean, A, dtype, what)


def pairloss_setup():
    plan = nat.make_plan(B, D, 1, 0, nat.MODE_FP32)
    gbuf = rk.synthetic_gbuf(plan, B + D)
    x, inv = rk.raw_rows(B, D, rk.F32)
    return plan, gbuf, x, inv


def test_teeth_a_bf16_output_truncated_instead_of_rounded():
    plan, gbuf, x, inv = pairloss_setup()
    ref = rk.pairloss_reference(x, rk.slice_sum(gbuf, plan), inv, 1, 1.0 / 0.07, 2.0, 0.25)
    want = ref["grads"][1]
    truncated = (want.float().view(torch.int32) & -65536).view(torch.float32)          # the upper 16 bits of the fp32 value
    assert torch.equal(truncated.bfloat16().float(), truncated) and not torch.equal(truncated.bfloat16(), want.bfloat16())
    rk.check_elements(want.bfloat16(), want, ref["A"][1], rk.BF16, "rounded")
    with pytest.raises(AssertionError, match="beyond their bar"):
        rk.check_elements(truncated.bfloat16(), want, ref["A"][1], rk.BF16, "truncated")


@pytest.mark.parametrize("dtype", [rk.F32, rk.BF16], ids=rk.dtype_name)
def test_teeth_the_neighbouring_rows_inv_norm(dtype):
    plan, gbuf, x, inv = pairloss_setup()
    M = rk.slice_sum(gbuf, plan)
    clean = rk.pairloss_reference(x, M, inv, 1, 1.0 / 0.07, 2.0, 0.25)
    wrong = rk.pairloss_reference(x, M, inv, 1, 1.0 / 0.07, 2.0, 0.25, neighbour_inv=True)
    for m in range(2):
        accepted_and_rejected(clean["grads"][m], wrong["grads"][m], clean["A"][m], dtype, f"pairloss modality {m}")
    with pytest.raises(AssertionError):
        rk.check_scalar(wrong["dscale"][1], clean["dscale"][1], clean["dscale_abs"][1], "dscale[1]")
    for pre in (0, 2):
        rows, iv = (x, inv) if pre == 0 else rk.unit_rows(B, D, rk.F32)
        clean = rk.finish_reference(rows, M, iv, rk.float32_reciprocal(rk.TAU), B, None, pre)
        wrong = rk.finish_reference(rows, M, iv, rk.float32_reciprocal(rk.TAU), B, None, pre, neighbour_inv=True)
        for m in range(2):
            accepted_and_rejected(clean["grads"][m], wrong["grads"][m], clean["A"][m], dtype, f"finish prenormalized={pre} modality {m}")


@pytest.mark.parametrize("dtype", [rk.F32, rk.BF16], ids=rk.dtype_name)
def test_teeth_the_positive_pair_from_the_rows_own_modality(dtype):
    plan, gbuf, x, inv = pairloss_setup()
    M = rk.slice_sum(gbuf, plan)
    lw = torch.stack(rk.xi.sample_weights(B, seed=B + D)[1])
    for pre in (0, 1, 2):
        rows, iv = (x, inv) if pre == 0 else rk.unit_rows(B, D, rk.F32)
        clean = rk.finish_reference(rows, M, iv, rk.float32_reciprocal(rk.TAU), B, lw, pre)
        wrong = rk.finish_reference(rows, M, iv, rk.float32_reciprocal(rk.TAU), B, lw, pre, own_modality_pair=True)
        for m in range(2):
            accepted_and_rejected(clean["grads"][m], wrong["grads"][m], clean["A"][m], dtype, f"finish prenormalized={pre} modality {m}")
    u, _ = rk.unit_rows(B, D, rk.F32)
    active = torch.randint(0, B + 1, (2, B), generator=torch.Generator().manual_seed(1)).float()
    clean, wrong = rk.maxmargin_reference(u, M, active), rk.maxmargin_reference(u, M, active, own_modality_pair=True)
    for m in range(2):
        accepted_and_rejected(clean["grads"][m], wrong["grads"][m], clean["A"][m], dtype, f"maxmargin modality {m}")


def test_the_closed_forms_are_autograd_of_the_documented_losses():
    """no kernel: the float64 references of families (1) and (2) against autograd through F.normalize of the scalar whose gradient
    include/crossclr.h says the finish kernels return -- sum <M, x^> s / (per_b B) for the pair losses, sum <M, x^> / (2 B tau) -
    sum_i (omega_v,i + omega_t,i) / (2 B tau) <v^_i, t^_i> for the loss -- with the exact 1 / ||x|| as inv_norm"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, B, D, generator=g, dtype=torch.float64)
    M = torch.randn(2, B, D, generator=g, dtype=torch.float64)
    lw = torch.stack(rk.xi.sample_weights(B, seed=3)[1])
    inv, go, inv_tau = 1.0 / x.norm(dim=2), rk.GRAD_OUT, 1.0 / 0.07
    close = lambda got, want: torch.allclose(got, want, rtol=1e-11, atol=1e-13 * float(want.abs().max()))
    leaf = x.clone().requires_grad_(True)
    (go * 2.5 / (2.0 * B) * (M * F.normalize(leaf, dim=2)).sum()).backward()
    assert close(rk.pairloss_reference(x, M, inv, 1, 2.5, 2.0, 0.25)["grads"], leaf.grad)
    for weights in (None, lw):
        omega = 0.5 * (weights[0] + weights[1]).double() if weights is not None else torch.ones(B, dtype=torch.float64)
        loss = lambda u: go * inv_tau / (2.0 * B) * (M * u).sum() - go * inv_tau / B * (omega * (u[0] * u[1]).sum(1)).sum()
        leaf = x.clone().requires_grad_(True)
        loss(F.normalize(leaf, dim=2)).backward()
        assert close(rk.finish_reference(x, M, inv, inv_tau, B, weights, 0)["grads"], leaf.grad)
        # prenormalized = 2: the kernel is handed the unit rows and 1 / ||y||, and returns the gradient w.r.t. y; = 1: w.r.t. the unit rows
        unit = F.normalize(x, dim=2)
        assert close(rk.finish_reference(unit, M, inv, inv_tau, B, weights, 2)["grads"], leaf.grad)
        leaf = unit.clone().requires_grad_(True)
        loss(leaf).backward()
        assert close(rk.finish_reference(unit, M, torch.ones(2, B), inv_tau, B, weights, 1)["grads"], leaf.grad)


@pytest.mark.parametrize("layout", ["ld+1", "ld+3", "offset"])
def test_teeth_one_element_written_at_column_D(layout):
    out = rk.Out(B, D, rk.F32, layout, "cpu")
    out.view.copy_(torch.zeros(B, D))
    assert torch.equal(out.read("clean"), torch.zeros(B, D))
    flat, off = out.buf.view(-1), (out.view.data_ptr() - out.buf.data_ptr()) // 4
    flat[off + 2 * out.ld + D] = 1.0                                                    # row 2, column D
    with pytest.raises(AssertionError, match="written outside"):
        out.read("one element at column D")


def test_teeth_a_gbuf_slice_skipped():
    plan, gbuf, x, inv = pairloss_setup()
    assert plan.bwd_slices > 1
    for skip in range(plan.bwd_slices):
        M, Ms = rk.slice_sum(gbuf, plan), rk.slice_sum(gbuf, plan, skip=skip)
        clean, wrong = rk.pairloss_reference(x, M, inv, 1, -5.0, 1.0, 0.5), rk.pairloss_reference(x, Ms, inv, 1, -5.0, 1.0, 0.5)
        for m in range(2):
            accepted_and_rejected(clean["grads"][m], wrong["grads"][m], clean["A"][m], rk.F32, f"pairloss slice {skip} modality {m}")
        clean = rk.finish_reference(x, M, inv, rk.float32_reciprocal(rk.TAU), B, None, 0)
        wrong = rk.finish_reference(x, Ms, inv, rk.float32_reciprocal(rk.TAU), B, None, 0)
        for m in range(2):
            accepted_and_rejected(clean["grads"][m], wrong["grads"][m], clean["A"][m], rk.F32, f"finish slice {skip} modality {m}")


@pytest.mark.parametrize("b", [2049, 4100])
def test_teeth_the_second_stage_of_the_hardest_negative_gather_dropped(b):
    x, idx, hinge = rk.hardneg_inputs(b, 48)
    clean = rk.hardneg_reference(x, idx, hinge)
    wrong = rk.hardneg_reference(x, idx, hinge, stages=[0] + ([2] if b > 4096 else []))
    for m in range(2):
        accepted_and_rejected(clean["grads"][m], wrong["grads"][m], clean["A"][m], rk.F32, f"hardneg b={b} modality {m}")
