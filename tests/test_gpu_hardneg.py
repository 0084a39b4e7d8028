"""The hardest-negative (max_violation=True) ranking loss and `hardest_negatives` on the MI355X: the checks of tests/test_hardneg_cpu.py
(tests/hardneg_cases.py: exact operands bit for bit, unit rows against autograd of the dense float64 definition, split independence) on
the device, and shapes with several row blocks, column splits and a real merge.

LARGER SHAPES, (B, D) = (1000, 300) and (2048, 512), `make_inputs("cluster", B, D, seed = B + D)` L2-normalised, margin 0.1, fp32 and
bf16.  Cluster inputs have near-ties, so the selections are checked by conditions (tol = 1e-5 max|S| for fp32, 2e-2 max|S| for bf16: the
project's score bars):
  (a) the index is in [0, B) and is not the partner
  (b) the returned score is within tol of S64[i, index]
  (c) S64[i, index] >= max_{j != i} S64[i, j] - 2 tol
The loss is within 2 tol (2 B) / B^2 of the float64 loss (2 B hinges, each off by at most 2 tol: the selected score and the pair's).
Gradients: the closed form (tests/hardneg_cases.closed_form_grads) rebuilt in float64 from the kernels' OWN returned selections and
active flags, rows within 1e-5.  Separately, an active flag may differ from float64 only where |m + S - d| <= 2 tol, and at most 2 % of
the float64 hinges lie in that band (seeds B + D satisfy this in float64: no hinge of either shape is within 4e-2 of zero).
One exact-operand case at B = 2048, D = 256 (integer scores, 16 row blocks): selections bit-equal in all three modes."""
import pytest
import torch

import crossclr_amd
import exact_inputs as xi
import hardneg_cases as hc
from crossclr_amd import _native as nat
from crossclr_amd import ranking as R
from oracle import crossclr_oracle as orc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.fixture(autouse=True)
def _hip_only():
    nat.use_library_for_testing(None)
    assert nat.backend() == "hip-gfx950", "GPU tests must run the HIP library"
    yield


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
    hc.check_split_independence(B, D, DEV)


MARGIN = 0.1
_large = {}


def large_case(B, D):
    """inputs and the float64 definition, once per shape"""
    if (B, D) not in _large:
        v, t = orc.make_inputs("cluster", B, D, B + D)
        v, t = torch.nn.functional.normalize(v, dim=1), torch.nn.functional.normalize(t, dim=1)
        _large[(B, D)] = (v, t, hc.definition(v, t, MARGIN))
    return _large[(B, D)]


@pytest.mark.parametrize("mode,rel_tol", [("fp32", 1e-5), ("bf16", 2e-2)])
@pytest.mark.parametrize("B,D", [(1000, 300), (2048, 512)])
def test_larger_shapes_by_conditions(B, D, mode, rel_tol):
    v, t, ref = large_case(B, D)
    S, d = ref["S"], ref["d"]
    tol = rel_tol * float(S.abs().max())
    lib, plan = nat.library(), nat.make_plan(B, D, 1, 0, R._resolve_mode(mode, B, torch.float32))
    assert lib.crossclr_hardneg_splits(plan, 0) > 1 and plan.bpad // 128 > 1      # several row blocks and column splits: a real merge
    a, b = v.to(DEV).requires_grad_(), t.to(DEV).requires_grad_()
    hn = R._hardneg(a.detach(), b.detach(), MARGIN, mode, normalize=False)
    bpad = hn.plan.bpad
    index, score, hinge = hn.index.cpu().long(), hn.score.cpu().double(), hn.hinge.cpu().double()
    partner = torch.arange(B)
    active = []
    for side, off, Sd, best in (("v2t", 0, S, ref["sr"]), ("t2v", bpad, S.t(), ref["sc"])):
        idx, sc, h = index[off:off + B], score[off:off + B], hinge[off:off + B]
        assert ((idx >= 0) & (idx < B) & (idx != partner)).all(), f"(a) {side}"
        at = Sd.gather(1, idx.view(-1, 1)).flatten()
        err_b, short_c = float((sc - at).abs().max()), float((best - at).max())
        print(f"{side} B={B} D={D} {mode}: tol {tol:.3e}  (b) {err_b:.3e}  (c) best - chosen {short_c:.3e}  selections equal to float64: "
              f"{float((idx == (ref['jr'] if off == 0 else ref['ic'])).double().mean()):.4f}")
        assert err_b <= tol, f"(b) {side}"
        assert short_c <= 2 * tol, f"(c) {side}"
        # active flags: free only where the float64 hinge argument of the CHOSEN pair is within 2 tol of zero
        arg = MARGIN + at - d
        band = arg.abs() <= 2 * tol
        assert float(((MARGIN + best - d).abs() <= 2 * tol).double().mean()) <= 0.02, "the reference has too many hinges near zero"
        act = h > 0
        assert ((act == (arg > 0)) | band).all(), f"active flags {side}"
        active.append(act)
    loss = crossclr_amd.max_margin_loss(a, b, MARGIN, compute_mode=mode, max_violation=True)
    (3.0 * loss).backward()
    err = abs(float(loss.detach()) - ref["loss"])
    print(f"loss {float(loss.detach()):.9g} ref {ref['loss']:.9g} |delta| {err:.3e} bound {2 * tol * 2 * B / (B * B):.3e}")
    assert err <= 2 * tol * (2 * B) / (B * B)
    want_im, want_s = hc.closed_form_grads(v, t, index[:B], index[bpad:bpad + B], active[0], active[1], 3.0)
    for got, want, what in ((a.grad, want_im, "grad_im"), (b.grad, want_s, "grad_s")):
        worst, row = xi.check_rows(got, want)
        print(f"  {what}: worst row {row} at {worst:.3e}")
        xi.check_rows(got, want, bar=1e-5)


_big_exact = {}


@pytest.mark.parametrize("mode", hc.MODES)
def test_exact_operands_at_2048_rows(mode):
    if not _big_exact:
        v, t = xi.planted("inter", 2048, 256, seed=2048 + 256, gram=False)
        _big_exact["case"] = (v, t, hc.definition(v, t, hc.EXACT_MARGIN))
    v, t, ref = _big_exact["case"]
    hn = crossclr_amd.hardest_negatives(v.to(DEV), t.to(DEV), compute_mode=mode)
    assert torch.equal(hn["v2t_index"].cpu(), ref["jr"]) and torch.equal(hn["t2v_index"].cpu(), ref["ic"])
    assert torch.equal(hn["v2t_score"].cpu().double(), ref["sr"]) and torch.equal(hn["t2v_score"].cpu().double(), ref["sc"])
