"""CPU tests of the pairwise sigmoid loss with a device-resident logit scale and bias: the REAL kernel sources (lane-level emulation)
against the dense float64 definition and the bars written out in tests/sigmoid_cases.py.  grad_out = 3 throughout.

  1  exact operands (tests/exact_inputs.planted, normalize=True, (s, beta) = (16, -8)): loss, row_loss and pair are the same bits in all
     three compute modes, equal float64 at the fp32 bars; gradients at each mode's bar
  2  random unit rows over (s, beta) in {(10, -10), (1 / 0.07, -3), (100, -10), (100, 0)}: fp32 and bf16x3 against the exact definition;
     bf16 on F.normalize(x).bfloat16().float() fed with normalize=False, against the definition on those tensors.  cluster and
     t = v + 2 n in fp32 and bf16x3 at (10, -10) and (100, -10) (the device tests run them over the whole set)
  3  bf16 with normalize=True against the exact definition (randn, SigLIP's initial values): loss 1e-3, gradients 1e-2
  4  the anti-diagonal input, t[B - 1 - i] = v[i] + 0.05 n, at s = 100: every row's positive-looking score sits in another tile than
     the diagonal
  5  edges: B = 1, a zero row, s = 0, negative s, beta = 0, strided rows, input dtypes
  6  the interface and the module;  7  the split count"""
import math

import pytest
import torch
import torch.nn.functional as F

import crossclr_amd
import exact_inputs as xi
import sigmoid_cases as sg
from crossclr_amd import _native as nat
from crossclr_amd import sigmoid as G

DEV = torch.device("cpu")
S0, B0 = sg.SCALE_BIAS[0]
# The emulation runs one OS thread per lane: the random inputs take one block with ragged rows and columns and 3 x 3 ragged blocks
# here (the exact-operand cases walk all five shapes in all three modes); tests/test_gpu_sigmoid.py runs every shape of RANDOM_CASES.
RANDOM_CASES = [c for c in sg.RANDOM_CASES if c[0] in (70, 300)]


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    from emu import build_emu
    nat.use_library_for_testing(build_emu.build())
    yield
    nat.use_library_for_testing(None)


@pytest.mark.parametrize("kind,B,D,nnz", sg.EXACT_CASES)
def test_exact_operands_same_bits_in_every_mode(kind, B, D, nnz):
    sg.check_exact_case(kind, B, D, nnz, DEV)


@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("s,beta", sg.SCALE_BIAS)
@pytest.mark.parametrize("B,D,seed", RANDOM_CASES)
def test_random_unit_rows(B, D, seed, s, beta, mode):
    sg.check_case("randn", B, D, seed, s, beta, mode, DEV)


@pytest.mark.parametrize("mode", ("fp32", "bf16x3"))
@pytest.mark.parametrize("s,beta", (sg.SCALE_BIAS[0], sg.SCALE_BIAS[2]))
@pytest.mark.parametrize("kind", ("cluster", "noisy"))
@pytest.mark.parametrize("B,D,seed", RANDOM_CASES)
def test_cluster_and_noisy_pairs(B, D, seed, kind, s, beta, mode):
    sg.check_case(kind, B, D, seed, s, beta, mode, DEV)


@pytest.mark.parametrize("B,D,seed", RANDOM_CASES)
def test_bf16_normalized_against_the_exact_definition(B, D, seed):
    sg.check_bf16_normalized(B, D, seed, DEV)


@pytest.mark.parametrize("B,D", sg.SHAPES)
def test_anti_diagonal_pairs(B, D):
    for mode in ("fp32", "bf16x3"):
        out, ref = sg.check_case("anti", B, D, B + D, 100.0, -10.0, mode, DEV)
    sg.check_rows(out, ref, f"anti B={B} D={D}")


def test_a_single_pair_is_not_trivial():
    v, t = torch.randn(1, 24, generator=torch.Generator().manual_seed(0)), torch.randn(1, 24, generator=torch.Generator().manual_seed(1))
    for normalize in (True, False):
        s, beta = (S0, B0) if normalize else (0.25, -1.0)
        ref = sg.definition(v, t, s, beta, normalize)
        out = sg.run(v, t, s, beta, "fp32", normalize, DEV)
        assert ref["loss"] > 1e-3 and abs(ref["gs"]) > 1e-6 and abs(ref["gb"]) > 1e-3 and float(ref["gv"].abs().max()) > 1e-6
        assert float(out["loss"]) != 0.0 and out["gv"].any() and out["gt"].any() and float(out["gs"]) != 0.0 and float(out["gb"]) != 0.0
        sg.check(out, ref, "fp32", f"B=1 normalize={normalize}")
        sg.check_rows(out, ref, "B=1")


def test_a_zero_row_is_finite_and_follows_f_normalize():
    v, t = sg.inputs("randn", 70, 48, 1)
    v, t = v.clone(), t.clone()
    v[37] = 0.0
    ref = sg.definition(v, t, S0, B0, True)
    out = sg.run(v, t, S0, B0, "fp32", True, DEV)
    # F.normalize divides a zero row by eps = 1e-12: that row's gradient is 1e12 times the others'.  It is checked relative to itself.
    sg.check(out, ref, "fp32", "zero row", skip_rows=(37,))
    got, want = out["gv"][37].double(), ref["gv"][37]
    assert torch.isfinite(got).all() and float((got - want).abs().max()) <= 2e-4 * float(want.abs().max())
    gt_err = float((out["gt"].double() - ref["gt"]).abs().max())
    assert gt_err <= 2e-4 * float(ref["gt"].abs().max()) + 1e-7 * ref["s"] / 70


@pytest.mark.parametrize("s,beta", [(0.0, -2.0), (0.0, 1.5), (-5.0, -3.0), (10.0, 0.0), (-5.0, 0.0)])
def test_zero_and_negative_scales_and_a_zero_bias(s, beta):
    v, t, ref = sg.reference_case("randn", 70, 48, 1, s, beta, True)
    out = sg.run(v, t, s, beta, "fp32", True, DEV)
    sg.check(out, ref, "fp32", "scale")
    sg.check_rows(out, ref, "scale")
    if s == 0.0:      # closed form: every logit is beta
        want = F.softplus(torch.tensor(-beta, dtype=torch.float64)) + 69 * F.softplus(torch.tensor(beta, dtype=torch.float64))
        assert abs(float(out["loss"]) - float(want)) <= 2e-5 * float(want)


def test_row_strided_inputs_give_the_same_bits():
    v, t = sg.inputs("randn", 70, 48, 1)
    base = sg.run(v, t, S0, B0, "fp32", True, DEV)
    sv, st = xi.lay_out(v, torch.float32, "ld+3", DEV), xi.lay_out(t, torch.float32, "ld+3", DEV)
    assert sv.stride(0) == 51
    a, b = sv.detach().requires_grad_(), st.detach().requires_grad_()      # (sg.run clones: the views themselves)
    sc = torch.tensor(S0, dtype=torch.float32, requires_grad=True)
    bc = torch.tensor(B0, dtype=torch.float32, requires_grad=True)
    loss = crossclr_amd.sigmoid_loss(a, b, sc, bc)
    (sg.GRAD_OUT * loss).backward()
    assert a.stride(0) == 51
    got = dict(loss=loss.detach(), gv=a.grad, gt=b.grad, gs=sc.grad, gb=bc.grad)
    for key in got:
        assert torch.equal(got[key], base[key]), key


@pytest.mark.parametrize("dtype,eps", [(torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8), (torch.float64, 0.0)])
def test_output_dtypes(dtype, eps):
    """Sign rows are exact in every dtype, so the loss is the fp32 run's and each gradient entry is the fp32 accumulation rounded ONCE
    into the input dtype: half a unit of its significand (eps) on top of the fp32 bar."""
    v, t, ref = sg.exact_case("inter", 70, 48, 16)
    out = sg.run(v.to(dtype), t.to(dtype), *sg.EXACT_SB, "fp32", True, DEV)
    assert out["loss"].dtype == (torch.float64 if dtype == torch.float64 else torch.float32)
    assert out["gv"].dtype == dtype and out["gt"].dtype == dtype and out["gs"].dtype == torch.float32 and out["gb"].dtype == torch.float32
    assert abs(float(out["loss"]) - ref["loss"]) <= sg.loss_bar(ref)
    for key in ("gv", "gt"):
        gmax = float(ref[key].abs().max())
        err = float((out[key].double() - ref[key]).abs().max())
        assert err <= (2e-4 + eps) * gmax + 1e-7 * ref["s"] / 70, (key, err)
    assert abs(float(out["gs"]) - ref["gs"]) <= 2e-4 * ref["A_s"] and abs(float(out["gb"]) - ref["gb"]) <= 2e-4 * ref["A_b"]


def test_requires_grad_on_one_argument_only():
    v, t, ref = sg.reference_case("randn", 70, 48, 1, S0, B0, True)
    full = sg.run(v, t, S0, B0, "fp32", True, DEV)
    a = v.clone().requires_grad_()
    (sg.GRAD_OUT * crossclr_amd.sigmoid_loss(a, t)).backward()
    assert torch.equal(a.grad, full["gv"])
    b = t.clone().requires_grad_()
    (sg.GRAD_OUT * crossclr_amd.sigmoid_loss(v, b, S0, B0)).backward()
    assert torch.equal(b.grad, full["gt"])
    sc = torch.tensor(S0, dtype=torch.float64, requires_grad=True)      # (another float dtype: the gradient comes back in it)
    (sg.GRAD_OUT * crossclr_amd.sigmoid_loss(v, t, sc, B0)).backward()
    assert sc.grad.dtype == torch.float64 and sc.grad.shape == sc.shape and float(sc.grad.float()) == float(full["gs"])
    bc = torch.tensor(B0, dtype=torch.float64, requires_grad=True)
    (sg.GRAD_OUT * crossclr_amd.sigmoid_loss(v, t, S0, bc)).backward()
    assert bc.grad.dtype == torch.float64 and bc.grad.shape == bc.shape and float(bc.grad.float()) == float(full["gb"])
    one_s, one_b = torch.full((1, 1), S0, requires_grad=True), torch.full((1, 1), B0, requires_grad=True)
    (sg.GRAD_OUT * crossclr_amd.sigmoid_loss(v, t, one_s, one_b)).backward()
    assert one_s.grad.shape == (1, 1) and float(one_s.grad) == float(full["gs"])
    assert one_b.grad.shape == (1, 1) and float(one_b.grad) == float(full["gb"])
    assert not crossclr_amd.sigmoid_loss(v, t).requires_grad


def test_float_arguments_give_the_bits_of_tensor_arguments():
    v, t = sg.inputs("randn", 70, 48, 1)
    x = crossclr_amd.sigmoid_loss(v, t, 10.0, -10.0)
    y = crossclr_amd.sigmoid_loss(v, t, torch.tensor(10.0), torch.tensor(-10.0))
    assert torch.equal(x, y) and x.dim() == 0 and torch.equal(x, crossclr_amd.sigmoid_loss(v, t))
    assert not torch.equal(x, crossclr_amd.sigmoid_loss(v, t, 10.0, -9.0))


def test_arguments_that_are_refused():
    v, t = sg.inputs("randn", 8, 16, 0)
    with pytest.raises(RuntimeError, match="logit_scale is on"):
        crossclr_amd.sigmoid_loss(v, t, torch.empty(1, device="meta"))
    with pytest.raises(RuntimeError, match="logit_bias is on"):
        crossclr_amd.sigmoid_loss(v, t, 10.0, torch.empty(1, device="meta"))
    with pytest.raises(RuntimeError, match="one-element"):
        crossclr_amd.sigmoid_loss(v, t, torch.ones(2))
    with pytest.raises(RuntimeError, match="one-element"):
        crossclr_amd.sigmoid_loss(v, t, 10.0, torch.ones(1, dtype=torch.int32))
    for mode in ("auto", "fp8"):
        with pytest.raises(ValueError):
            crossclr_amd.sigmoid_loss(v, t, compute_mode=mode)
    with pytest.raises(RuntimeError):
        crossclr_amd.sigmoid_loss(v, t[:7])
    a = v.clone().requires_grad_()
    loss = crossclr_amd.sigmoid_loss(a, t)
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(loss, a, create_graph=True)


def test_new_symbols_are_bound_and_the_abi_version_is_unchanged():
    lib = nat.library()
    for sym in ("crossclr_sigmoid_splits", "crossclr_sigmoid_workspace_bytes", "crossclr_sigmoid_stats", "crossclr_sigmoid_finish",
                "crossclr_sigmoid_backward", "crossclr_sigmoid_backward_finish"):
        assert sym in nat.EXPORTED_SYMBOLS and getattr(lib, sym).argtypes is not None
    assert lib.crossclr_abi_version() == 8 == nat.ABI_VERSION
    assert crossclr_amd.sigmoid_loss is G.sigmoid_loss and crossclr_amd.SigmoidLoss is G.SigmoidLoss
    assert "sigmoid_loss" in crossclr_amd.__all__ and "SigmoidLoss" in crossclr_amd.__all__
    plan = nat.make_plan(130, 200, 1, 0, nat.MODE_FP32)
    need = lib.crossclr_sigmoid_workspace_bytes(plan, 0)
    assert need == (2 * 2 + 1) * 256 * 4 and lib.crossclr_sigmoid_workspace_bytes(plan, 1) == (2 * 1 + 1) * 256 * 4
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    p = buf.data_ptr()
    assert lib.crossclr_sigmoid_stats(plan, p, p, p, 0, p, need - 1, 0) == -4      # CROSSCLR_E_WORKSPACE
    assert lib.crossclr_sigmoid_stats(plan, p, 0, p, 0, p, need, 0) == -1          # CROSSCLR_E_ARG
    assert lib.crossclr_sigmoid_stats(plan, p, p, 0, 0, p, need, 0) == -1
    assert lib.crossclr_sigmoid_finish(plan, p, 0, p, p, p, p, p, 0, 0) == -1
    sharded = nat.make_plan(130, 200, 2, 0, nat.MODE_FP32)
    assert lib.crossclr_sigmoid_workspace_bytes(sharded, 0) == 0
    assert lib.crossclr_sigmoid_splits(sharded, 0) == -1 and b"single-device" in lib.crossclr_last_error()
    assert lib.crossclr_sigmoid_backward(sharded, p, p, p, p, 0) == -1
    assert b"single-device" in lib.crossclr_last_error()


def test_the_module():
    m = crossclr_amd.SigmoidLoss(init_logit_scale=20.0, init_logit_bias=-5.0)
    assert list(m.state_dict()) == ["logit_scale", "logit_bias"]
    assert isinstance(m.logit_scale, torch.nn.Parameter) and isinstance(m.logit_bias, torch.nn.Parameter)
    assert abs(float(m.logit_scale.detach()) - math.log(20.0)) < 1e-6 and float(m.logit_bias.detach()) == -5.0
    assert "learnable=True" in repr(m) and "max_logit_scale=100.0" in repr(m) and "compute_mode='fp32'" in repr(m)
    default = crossclr_amd.SigmoidLoss()
    assert abs(float(default.logit_scale.detach()) - math.log(10.0)) < 1e-6 and float(default.logit_bias.detach()) == -10.0
    frozen = crossclr_amd.SigmoidLoss(learnable=False)
    assert list(frozen.parameters()) == [] and list(frozen.state_dict()) == ["logit_scale", "logit_bias"]
    v, t = sg.inputs("randn", 70, 48, 1)
    assert torch.equal(frozen(v, t), crossclr_amd.sigmoid_loss(v, t, frozen.logit_scale.exp(), -10.0))
    # the clamp is active: log(1000) is far above log(100); the loss is the one at s = 100 and no gradient reaches logit_scale
    hot = crossclr_amd.SigmoidLoss(init_logit_scale=1000.0)
    loss = hot(v, t)
    assert torch.equal(loss.detach(), crossclr_amd.sigmoid_loss(v, t, 100.0, -10.0))
    loss.backward()
    assert float(hot.logit_scale.grad) == 0.0 and float(hot.logit_bias.grad) != 0.0
    # one optimiser step moves logit_scale by lr * dL/ds * s (the chain through exp) and logit_bias by lr * dL/dbeta
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    before_s, before_b = float(m.logit_scale.detach()), float(m.logit_bias.detach())
    m(v, t).backward()
    ref = sg.definition(v, t, 20.0, -5.0, True, grad_out=1.0)
    want_s, want_b = ref["gs"] * 20.0, ref["gb"]
    assert abs(float(m.logit_scale.grad) - want_s) <= 2e-4 * ref["A_s"] * 20.0 + 1e-6 * abs(want_s)
    assert abs(float(m.logit_bias.grad) - want_b) <= 2e-4 * ref["A_b"]
    opt.step()
    after_s, after_b = float(m.logit_scale.detach()), float(m.logit_bias.detach())
    assert abs(after_s - (before_s - 0.1 * want_s)) <= 1e-5 and after_s != before_s
    assert abs(after_b - (before_b - 0.1 * want_b)) <= 1e-5 and after_b != before_b


@pytest.mark.parametrize("B,D", [(130, 200), (300, 40)])
def test_split_counts(B, D):
    lib = nat.library()
    plan = nat.make_plan(B, D, 1, 0, nat.MODE_FP32)
    tiles = plan.bpad // 128
    assert lib.crossclr_sigmoid_splits(plan, 0) == tiles and lib.crossclr_sigmoid_splits(plan, 1) == 1
    assert lib.crossclr_sigmoid_splits(plan, 3) == min(3, tiles)
    sg.check_splits(B, D, DEV)
