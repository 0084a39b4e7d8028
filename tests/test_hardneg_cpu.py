"""CPU tests of the hardest-negative (max_violation=True) ranking loss and `hardest_negatives`: the REAL kernel sources (lane-level
emulation) against the dense float64 definition written out in tests/hardneg_cases.py.

  1  exact operands (tests/exact_inputs.planted, used as given: integer scores in every compute mode): selections equal the definition's
     with first-index ties, scores bit-equal, loss 1e-6, gradient rows 1e-6 -- sums of small-integer rows, the only roundings are the
     1 / B^2 and grad_out scalings
  2  unit-row random inputs against autograd of the definition (bf16: the definition on bf16-rounded operands): loss 1e-5, rows 1e-5
  3  the split count changes no bit
  4  the interface: dtypes, strides, B = 1, one-sided requires_grad, double backward, max_violation=False, retrieval_topk agreement"""
import pytest
import torch

import crossclr_amd
import exact_inputs as xi
import hardneg_cases as hc
from crossclr_amd import _native as nat
from crossclr_amd import ranking as R

DEV = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    from emu import build_emu
    nat.use_library_for_testing(build_emu.build())
    yield
    nat.use_library_for_testing(None)


@pytest.mark.parametrize("mode", hc.MODES)
@pytest.mark.parametrize("kind,B,D,nnz", hc.EXACT_CASES)
def test_exact_operands_select_bit_for_bit(kind, B, D, nnz, mode):
    hc.check_exact_case(kind, B, D, nnz, mode, DEV)


@pytest.mark.parametrize("mode", hc.MODES)
@pytest.mark.parametrize("B,D,seed", hc.RANDOM_CASES)
def test_unit_rows_match_autograd_of_the_dense_definition(B, D, seed, mode):
    hc.check_random_case(B, D, seed, mode, DEV)


@pytest.mark.parametrize("B,D", hc.SPLIT_CASES)
def test_every_split_count_gives_the_same_bits(B, D):
    lib = nat.library()
    plan = nat.make_plan(B, D, 1, 0, nat.MODE_FP32)
    tiles = plan.bpad // 128
    assert lib.crossclr_hardneg_splits(plan, 0) == tiles           # small batches: one split per column tile
    assert lib.crossclr_hardneg_splits(plan, 1) == 1 and lib.crossclr_hardneg_splits(plan, 2) == 2
    assert lib.crossclr_hardneg_splits(plan, 3) == min(3, tiles)
    hc.check_split_independence(B, D, DEV)


@pytest.mark.parametrize("dtype,bar", [(torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8), (torch.float64, 1e-6)])
def test_outputs_come_in_the_input_dtype(dtype, bar):
    """+-1 rows are exact in every dtype, so loss and accumulated gradients are the definition's; what is left is ONE rounding of each
    gradient entry into the output dtype (half a unit: 2^-11 for fp16, 2^-8 for bf16 relative to the entry, at most that of the row's
    largest) and the 1 / B^2 scaling for fp64 (fp64 accumulation: 1e-6 is the common bar of the exact cases)."""
    v, t, ref = hc.exact_case("inter", 70, 48, 16)
    loss, g_im, g_s = hc.run(v.to(dtype), t.to(dtype), hc.EXACT_MARGIN, "fp32", DEV)
    assert loss.dtype == dtype and g_im.dtype == dtype and g_s.dtype == dtype
    assert abs(float(loss) - ref["loss"]) <= bar * max(1.0, abs(ref["loss"]))
    xi.check_rows(g_im, ref["grads"][0], bar=bar)
    xi.check_rows(g_s, ref["grads"][1], bar=bar)


def test_row_strided_inputs_give_the_same_bits():
    v, t, _ = hc.exact_case("inter", 70, 48, 16)
    base = hc.run(v, t, hc.EXACT_MARGIN, "fp32", DEV)
    sv, st = xi.lay_out(v, torch.float32, "ld+3", DEV), xi.lay_out(t, torch.float32, "ld+3", DEV)
    assert sv.stride(0) == 51
    for x, y in zip(base, hc.run(sv, st, hc.EXACT_MARGIN, "fp32", DEV)):
        assert torch.equal(x, y)
    a, b = crossclr_amd.hardest_negatives(v, t), crossclr_amd.hardest_negatives(sv, st)
    for key in a:
        assert torch.equal(a[key], b[key]), key


def test_a_single_pair_has_no_negative():
    v, t = torch.randn(1, 24, generator=torch.Generator().manual_seed(0)), torch.ones(1, 24)
    loss, g_im, g_s = hc.run(v, t, 0.1, "fp32", DEV)
    assert float(loss) == 0.0 and not g_im.any() and not g_s.any()
    hn = crossclr_amd.hardest_negatives(v, t)
    assert hn["v2t_index"].tolist() == [-1] and hn["t2v_index"].tolist() == [-1]


def test_an_inactive_hinge_reports_its_index_and_contributes_nothing():
    """margin far below every S[i, i] - S[i, j]: no hinge is active, the selections are still the definition's"""
    v, t, ref = hc.random_case(70, 48, 1, False)
    big = 4.0 * torch.eye(70)
    a, b = torch.cat([v, big], 1), torch.cat([t, big], 1)          # every positive pair scores 16 more; the negatives stay v . t
    loss, g_im, g_s = hc.run(a, b, 0.1, "fp32", DEV)
    assert float(loss) == 0.0 and not g_im.any() and not g_s.any()
    hn, want = crossclr_amd.hardest_negatives(a, b), hc.definition(a, b, 0.1)
    assert torch.equal(hn["v2t_index"], want["jr"]) and torch.equal(hn["t2v_index"], want["ic"])


def test_requires_grad_on_one_input_only():
    v, t, ref = hc.exact_case("inter", 70, 48, 16)
    a = v.clone().requires_grad_()
    (3.0 * crossclr_amd.max_margin_loss(a, t, hc.EXACT_MARGIN, max_violation=True)).backward()
    xi.check_rows(a.grad, ref["grads"][0], bar=1e-6)
    b = t.clone().requires_grad_()
    (3.0 * crossclr_amd.MaxMargin_coot(margin=hc.EXACT_MARGIN, max_violation=True)(v, b)).backward()
    xi.check_rows(b.grad, ref["grads"][1], bar=1e-6)


def test_double_backward_raises():
    v, t, _ = hc.exact_case("inter", 8, 16, 4)
    a = v.clone().requires_grad_()
    loss = crossclr_amd.max_margin_loss(a, t, hc.EXACT_MARGIN, max_violation=True)
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(loss, a, create_graph=True)


def test_the_default_is_the_sum_form_unchanged():
    v, t, _ = hc.random_case(70, 48, 1, False)
    outs = []
    for kw in ({}, {"max_violation": False}):
        a, b = v.clone().requires_grad_(), t.clone().requires_grad_()
        loss = crossclr_amd.max_margin_loss(a, b, 0.1, **kw)
        loss.backward()
        outs.append((loss.detach(), a.grad, b.grad))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    m = crossclr_amd.MaxMargin_coot(margin=0.1)
    assert m.max_violation is False and "max_violation=False" in repr(m)
    assert torch.equal(m(v, t), outs[0][0])
    assert "max_violation=True" in repr(crossclr_amd.MaxMargin_coot(max_violation=True))
    hard = crossclr_amd.max_margin_loss(v, t, 0.1, max_violation=True)
    assert float(hard) < float(outs[0][0])      # a maximum per row instead of the row's sum


def test_hardest_negatives_agree_with_retrieval_topk():
    """the best two of every row with the partner removed: the same scores from the same tiled product, under the same total order"""
    v, t, _ = hc.random_case(130, 200, 11, False)
    hn = crossclr_amd.hardest_negatives(v, t, normalize=True)
    partner = torch.arange(130)
    for q, g, key in ((v, t, "v2t"), (t, v, "t2v")):
        scores, indices = crossclr_amd.retrieval_topk(q, g, 2, normalize=True)
        first = indices[:, 0] != partner
        assert torch.equal(hn[key + "_index"], torch.where(first, indices[:, 0], indices[:, 1]))
        assert torch.equal(hn[key + "_score"], torch.where(first, scores[:, 0], scores[:, 1]))


def test_new_symbols_are_bound_and_the_abi_version_is_unchanged():
    lib = nat.library()
    for sym in ("crossclr_hardneg_splits", "crossclr_hardneg_workspace_bytes", "crossclr_hardneg_select", "crossclr_hardneg_finish",
                "crossclr_hardneg_backward"):
        assert sym in nat.EXPORTED_SYMBOLS and getattr(lib, sym).argtypes is not None
    assert lib.crossclr_abi_version() == 8 == nat.ABI_VERSION
    assert crossclr_amd.hardest_negatives is R.hardest_negatives and "hardest_negatives" in crossclr_amd.__all__
    plan = nat.make_plan(130, 200, 1, 0, nat.MODE_FP32)
    need = lib.crossclr_hardneg_workspace_bytes(plan, 0)
    assert need == (2 * 2 + 2 * 2 + 1) * 256 * 4
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    assert lib.crossclr_hardneg_select(plan, buf.data_ptr(), 0, buf.data_ptr(), need - 1, 0) == -4      # CROSSCLR_E_WORKSPACE
    assert lib.crossclr_hardneg_select(plan, 0, 0, buf.data_ptr(), need, 0) == -1                      # CROSSCLR_E_ARG
    sharded = nat.make_plan(130, 200, 2, 0, nat.MODE_FP32)
    assert lib.crossclr_hardneg_workspace_bytes(sharded, 0) == 0
    assert lib.crossclr_hardneg_splits(sharded, 0) == -1 and b"single-device" in lib.crossclr_last_error()
