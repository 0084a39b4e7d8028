"""CPU tests of the symmetric InfoNCE loss with a device-resident logit scale: the REAL kernel sources (lane-level emulation) against the
dense float64 definition and the bars written out in tests/infonce_cases.py.  grad_out = 3 throughout.

  1  exact operands (tests/exact_inputs.planted, normalize=True, s = 16): lse, pair and loss are the same bits in all three compute modes,
     equal float64 at the fp32 bars; gradients at each mode's bar
  2  random unit rows, s in {1 / 0.07, 100}: fp32 and bf16x3 against the exact definition (randn, cluster, t = v + 2 n); bf16 on
     F.normalize(x).bfloat16().float() fed with normalize=False, against the definition on those tensors
  3  bf16 with normalize=True against the exact definition (randn, s = 1 / 0.07): loss 1e-3, gradients 1e-2
  4  online-max stress, t[B - 1 - i] = v[i] + 0.05 n: s = 100 normalised (fp32, bf16x3) and s = 4 on the rows as given (logits span
     +-800: no fixed shift survives; fp32 only -- the split operand's products are fp32-grade relative to |v| |t|, which at logits of
     800 is not an fp32-grade logit)
  5  edges: B = 1, a zero row, s = 0, negative s, strided rows, input dtypes
  6  the interface;  7  the split count"""
import math

import pytest
import torch
import torch.nn.functional as F

import crossclr_amd
import exact_inputs as xi
import infonce_cases as ic
from crossclr_amd import _native as nat
from crossclr_amd import infonce as N

DEV = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    from emu import build_emu
    nat.use_library_for_testing(build_emu.build())
    yield
    nat.use_library_for_testing(None)


@pytest.mark.parametrize("kind,B,D,nnz", ic.EXACT_CASES)
def test_exact_operands_same_bits_in_every_mode(kind, B, D, nnz):
    ic.check_exact_case(kind, B, D, nnz, DEV)


@pytest.mark.parametrize("mode", ic.MODES)
@pytest.mark.parametrize("s", ic.SCALES)
@pytest.mark.parametrize("B,D,seed", ic.RANDOM_CASES)
def test_random_unit_rows(B, D, seed, s, mode):
    ic.check_case("randn", B, D, seed, s, mode, DEV)


@pytest.mark.parametrize("mode", ("fp32", "bf16x3"))
@pytest.mark.parametrize("s", ic.SCALES)
@pytest.mark.parametrize("kind", ("cluster", "noisy"))
@pytest.mark.parametrize("B,D,seed", ic.RANDOM_CASES)
def test_cluster_and_noisy_pairs(B, D, seed, kind, s, mode):
    ic.check_case(kind, B, D, seed, s, mode, DEV)


@pytest.mark.parametrize("B,D,seed", ic.RANDOM_CASES)
def test_bf16_normalized_against_the_exact_definition(B, D, seed):
    ic.check_bf16_normalized(B, D, seed, DEV)


@pytest.mark.parametrize("B,D", ic.SHAPES)
def test_online_max_stress(B, D):
    for mode in ("fp32", "bf16x3"):
        ic.check_case("anti", B, D, B + D, 100.0, mode, DEV)
    out, ref = ic.check_case("anti", B, D, B + D, 4.0, "fp32", DEV, normalize=False)
    if D >= 40:
        top = float(ref["lr"].max())      # (>= the row's largest logit, 4 |v|^2 on the anti-diagonal)
        assert top > 128 * math.log(2), top      # beyond exp's range in fp32: the shift has to be the slot's own maximum


def test_a_single_pair():
    v, t = torch.randn(1, 24, generator=torch.Generator().manual_seed(0)), torch.randn(1, 24, generator=torch.Generator().manual_seed(1))
    for normalize in (True, False):
        out = ic.run(v, t, 1 / 0.07, "fp32", normalize, DEV)
        ref = ic.definition(v, t, 1 / 0.07, normalize)
        assert abs(ref["loss"]) < 1e-12 and ref["A"] < 1e-12
        assert float(out["loss"]) == 0.0 and not out["gv"].any() and not out["gt"].any() and float(out["gs"]) == 0.0


def test_a_zero_row_is_finite_and_follows_f_normalize():
    v, t = ic.inputs("randn", 70, 48, 1)
    v, t = v.clone(), t.clone()
    v[37] = 0.0
    ref = ic.definition(v, t, 1 / 0.07, True)
    out = ic.run(v, t, 1 / 0.07, "fp32", True, DEV)
    # F.normalize divides a zero row by eps = 1e-12: that row's gradient is 1e12 times the others'.  It is checked relative to itself.
    ic.check(out, ref, "fp32", "zero row", skip_rows=(37,))
    got, want = out["gv"][37].double(), ref["gv"][37]
    assert torch.isfinite(got).all() and float((got - want).abs().max()) <= 2e-4 * float(want.abs().max())
    gt_err = float((out["gt"].double() - ref["gt"]).abs().max())
    assert gt_err <= 2e-4 * float(ref["gt"].abs().max()) + 1e-7 * ref["s"] / 70


@pytest.mark.parametrize("s", (0.0, -5.0))
def test_zero_and_negative_scales(s):
    v, t, ref = ic.reference_case("randn", 70, 48, 1, s, True)
    out = ic.run(v, t, s, "fp32", True, DEV)
    ic.check(out, ref, "fp32", "scale")
    if s == 0.0:
        assert abs(float(out["loss"]) - math.log(70)) <= 2e-5 * math.log(70)


def test_row_strided_inputs_give_the_same_bits():
    v, t = ic.inputs("randn", 70, 48, 1)
    base = ic.run(v, t, 1 / 0.07, "fp32", True, DEV)
    sv, st = xi.lay_out(v, torch.float32, "ld+3", DEV), xi.lay_out(t, torch.float32, "ld+3", DEV)
    assert sv.stride(0) == 51
    a, b = sv.detach().requires_grad_(), st.detach().requires_grad_()      # (ic.run clones: the views themselves)
    sc = torch.tensor(1 / 0.07, dtype=torch.float32, requires_grad=True)
    loss = crossclr_amd.info_nce_loss(a, b, sc)
    (ic.GRAD_OUT * loss).backward()
    assert a.stride(0) == 51
    got = dict(loss=loss.detach(), gv=a.grad, gt=b.grad, gs=sc.grad)
    for key in got:
        assert torch.equal(got[key], base[key]), key


@pytest.mark.parametrize("dtype,eps", [(torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8), (torch.float64, 0.0)])
def test_output_dtypes(dtype, eps):
    """Sign rows are exact in every dtype, so the loss is the fp32 run's and each gradient entry is the fp32 accumulation rounded ONCE
    into the input dtype: half a unit of its significand (eps) on top of the fp32 bar."""
    v, t, ref = ic.exact_case("inter", 70, 48, 16)
    out = ic.run(v.to(dtype), t.to(dtype), ic.EXACT_SCALE, "fp32", True, DEV)
    assert out["loss"].dtype == (torch.float64 if dtype == torch.float64 else torch.float32)
    assert out["gv"].dtype == dtype and out["gt"].dtype == dtype and out["gs"].dtype == torch.float32
    assert abs(float(out["loss"]) - ref["loss"]) <= ic.loss_bar(ref)
    for key in ("gv", "gt"):
        gmax = float(ref[key].abs().max())
        err = float((out[key].double() - ref[key]).abs().max())
        assert err <= (2e-4 + eps) * gmax + 1e-7 * ref["s"] / 70, (key, err)
    assert abs(float(out["gs"]) - ref["gs"]) <= 2e-4 * ref["A"]


def test_requires_grad_on_one_argument_only():
    v, t, ref = ic.reference_case("randn", 70, 48, 1, ic.SCALES[0], True)
    full = ic.run(v, t, ic.SCALES[0], "fp32", True, DEV)
    a = v.clone().requires_grad_()
    (ic.GRAD_OUT * crossclr_amd.info_nce_loss(a, t)).backward()
    assert torch.equal(a.grad, full["gv"])
    b = t.clone().requires_grad_()
    (ic.GRAD_OUT * crossclr_amd.info_nce_loss(v, b, ic.SCALES[0])).backward()
    assert torch.equal(b.grad, full["gt"])
    sc = torch.tensor(ic.SCALES[0], dtype=torch.float64, requires_grad=True)      # (another float dtype: the gradient comes back in it)
    (ic.GRAD_OUT * crossclr_amd.info_nce_loss(v, t, sc)).backward()
    assert sc.grad.dtype == torch.float64 and sc.grad.shape == sc.shape and float(sc.grad.float()) == float(full["gs"])
    one = torch.full((1, 1), ic.SCALES[0], requires_grad=True)
    (ic.GRAD_OUT * crossclr_amd.info_nce_loss(v, t, one)).backward()
    assert one.grad.shape == (1, 1) and float(one.grad) == float(full["gs"])
    assert not crossclr_amd.info_nce_loss(v, t).requires_grad


def test_a_float_scale_gives_the_bits_of_a_tensor_scale():
    v, t = ic.inputs("randn", 70, 48, 1)
    x = crossclr_amd.info_nce_loss(v, t, 1 / 0.07)
    y = crossclr_amd.info_nce_loss(v, t, torch.tensor(1 / 0.07, dtype=torch.float32))
    assert torch.equal(x, y) and x.dim() == 0 and torch.equal(x, crossclr_amd.info_nce_loss(v, t))


def test_arguments_that_are_refused():
    v, t = ic.inputs("randn", 8, 16, 0)
    with pytest.raises(RuntimeError, match="logit_scale is on"):
        crossclr_amd.info_nce_loss(v, t, torch.empty(1, device="meta"))
    with pytest.raises(RuntimeError, match="one-element"):
        crossclr_amd.info_nce_loss(v, t, torch.ones(2))
    for mode in ("auto", "fp8"):
        with pytest.raises(ValueError):
            crossclr_amd.info_nce_loss(v, t, compute_mode=mode)
    with pytest.raises(RuntimeError):
        crossclr_amd.info_nce_loss(v, t[:7])
    a = v.clone().requires_grad_()
    loss = crossclr_amd.info_nce_loss(a, t)
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(loss, a, create_graph=True)


def test_new_symbols_are_bound_and_the_abi_version_is_unchanged():
    lib = nat.library()
    for sym in ("crossclr_infonce_splits", "crossclr_infonce_workspace_bytes", "crossclr_infonce_stats", "crossclr_infonce_finish",
                "crossclr_infonce_backward", "crossclr_infonce_backward_finish"):
        assert sym in nat.EXPORTED_SYMBOLS and getattr(lib, sym).argtypes is not None
    assert lib.crossclr_abi_version() == 8 == nat.ABI_VERSION
    assert crossclr_amd.info_nce_loss is N.info_nce_loss and crossclr_amd.InfoNCE is N.InfoNCE
    assert "info_nce_loss" in crossclr_amd.__all__ and "InfoNCE" in crossclr_amd.__all__
    plan = nat.make_plan(130, 200, 1, 0, nat.MODE_FP32)
    need = lib.crossclr_infonce_workspace_bytes(plan, 0)
    assert need == (2 * 2 + 2 * 2 + 1) * 256 * 4
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    assert lib.crossclr_infonce_stats(plan, buf.data_ptr(), buf.data_ptr(), 0, buf.data_ptr(), need - 1, 0) == -4      # CROSSCLR_E_WORKSPACE
    assert lib.crossclr_infonce_stats(plan, buf.data_ptr(), 0, 0, buf.data_ptr(), need, 0) == -1                      # CROSSCLR_E_ARG
    sharded = nat.make_plan(130, 200, 2, 0, nat.MODE_FP32)
    assert lib.crossclr_infonce_workspace_bytes(sharded, 0) == 0
    assert lib.crossclr_infonce_splits(sharded, 0) == -1 and b"single-device" in lib.crossclr_last_error()
    assert lib.crossclr_infonce_backward(sharded, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 0) == -1
    assert b"single-device" in lib.crossclr_last_error()


def test_the_module():
    m = crossclr_amd.InfoNCE(temperature=0.05)
    assert list(m.state_dict()) == ["logit_scale"] and isinstance(m.logit_scale, torch.nn.Parameter)
    assert abs(float(m.logit_scale.detach()) - math.log(20.0)) < 1e-6
    assert "learnable=True" in repr(m) and "max_logit_scale=100.0" in repr(m) and "compute_mode='fp32'" in repr(m)
    frozen = crossclr_amd.InfoNCE(learnable=False)
    assert list(frozen.parameters()) == [] and list(frozen.state_dict()) == ["logit_scale"]
    v, t = ic.inputs("randn", 70, 48, 1)
    assert torch.equal(frozen(v, t), crossclr_amd.info_nce_loss(v, t, frozen.logit_scale.exp()))
    # the clamp is active: log(1 / 0.001) is far above log(100); the loss is the one at s = 100 and no gradient reaches the parameter
    hot = crossclr_amd.InfoNCE(temperature=0.001)
    loss = hot(v, t)
    assert torch.equal(loss.detach(), crossclr_amd.info_nce_loss(v, t, 100.0))
    loss.backward()
    assert float(hot.logit_scale.grad) == 0.0
    # one optimiser step moves logit_scale, by lr * dL/ds * s (the chain through exp)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    before = float(m.logit_scale.detach())
    m(v, t).backward()
    ref = ic.definition(v, t, 20.0, True, grad_out=1.0)
    want = ref["gs"] * 20.0
    assert abs(float(m.logit_scale.grad) - want) <= 2e-4 * ref["A"] * 20.0 + 1e-6 * abs(want)
    opt.step()
    after = float(m.logit_scale.detach())
    assert abs(after - (before - 0.1 * want)) <= 1e-5 and after != before


@pytest.mark.parametrize("B,D", [(130, 200), (300, 40)])
def test_split_counts(B, D):
    lib = nat.library()
    plan = nat.make_plan(B, D, 1, 0, nat.MODE_FP32)
    tiles = plan.bpad // 128
    assert lib.crossclr_infonce_splits(plan, 0) == tiles and lib.crossclr_infonce_splits(plan, 1) == 1
    assert lib.crossclr_infonce_splits(plan, 3) == min(3, tiles)
    ic.check_splits(B, D, DEV)
