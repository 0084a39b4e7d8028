"""The pairwise sigmoid loss with a device-resident logit scale and bias on the MI355X: the checks of tests/test_sigmoid_cpu.py
(tests/sigmoid_cases.py: the float64 definition and the bars) on the device, and shapes with several row blocks, column splits, gradient
slices and D slices.  grad_out = 3 throughout.

LARGER SHAPES, (B, D) = (1000, 300), (2048, 512) and (130, 1100), SigLIP's initial values (s, beta) = (10, -10), against the float64
definition computed once per input: fp32 on `make_inputs("cluster" / "randn", B, D, seed = B + D)` with normalize=True; bf16 on the randn
rows as F.normalize(x).bfloat16().float() fed with normalize=False (the bf16 bars are stated for the same bf16-exact operands).
One exact-operand case at B = 2048, D = 256 (16 row blocks): loss, row_loss and pair are the same bits in all three modes.

GRAPH CAPTURE: forward + backward with a tensor scale AND a tensor bias captured into a HIP graph; the inputs, the scale and the bias are
overwritten in place and the graph replayed: loss and all four gradients equal an eager run with the new values bit for bit -- nothing
reads either scalar on the host.

MEASURED on the MI355X, worst error / bar over all cases of this file (every test prints each figure beside its bar): fp32 loss 0.04,
gradients 0.05, dL/ds 0.001, dL/dbeta 0.005; bf16x3 loss 0.06, gradients 0.11 (cluster, B = 130, D = 200), dL/ds 0.02, dL/dbeta 0.02;
bf16 loss 0.44 and gradients 0.35 (normalize=True against the exact definition, bars 1e-3 / 1e-2), dL/ds 0.27, dL/dbeta 0.001.  The bars
are the project's, not tightened."""
import pytest
import torch

import crossclr_amd
import exact_inputs as xi
import sigmoid_cases as sg
from crossclr_amd import _native as nat

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
S0, B0 = sg.SCALE_BIAS[0]


@pytest.fixture(autouse=True)
def _hip_only():
    nat.use_library_for_testing(None)
    assert nat.backend() == "hip-gfx950", "GPU tests must run the HIP library"
    yield


@pytest.mark.parametrize("kind,B,D,nnz", sg.EXACT_CASES)
def test_exact_operands_same_bits_in_every_mode(kind, B, D, nnz):
    sg.check_exact_case(kind, B, D, nnz, DEV)


@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("s,beta", sg.SCALE_BIAS)
@pytest.mark.parametrize("B,D,seed", sg.RANDOM_CASES)
def test_random_unit_rows(B, D, seed, s, beta, mode):
    sg.check_case("randn", B, D, seed, s, beta, mode, DEV)


@pytest.mark.parametrize("mode", ("fp32", "bf16x3"))
@pytest.mark.parametrize("s,beta", sg.SCALE_BIAS)
@pytest.mark.parametrize("kind", ("cluster", "noisy"))
@pytest.mark.parametrize("B,D,seed", sg.RANDOM_CASES)
def test_cluster_and_noisy_pairs(B, D, seed, kind, s, beta, mode):
    sg.check_case(kind, B, D, seed, s, beta, mode, DEV)


@pytest.mark.parametrize("B,D,seed", sg.RANDOM_CASES)
def test_bf16_normalized_against_the_exact_definition(B, D, seed):
    sg.check_bf16_normalized(B, D, seed, DEV)


@pytest.mark.parametrize("B,D", sg.SHAPES)
def test_anti_diagonal_pairs(B, D):
    for mode in ("fp32", "bf16x3"):
        out, ref = sg.check_case("anti", B, D, B + D, 100.0, -10.0, mode, DEV)
    sg.check_rows(out, ref, f"anti B={B} D={D}")


@pytest.mark.parametrize("B,D", [(130, 200), (300, 40)])
def test_split_counts(B, D):
    sg.check_splits(B, D, DEV)


def test_edges_on_the_device():
    v, t = torch.randn(1, 24, generator=torch.Generator().manual_seed(0)), torch.randn(1, 24, generator=torch.Generator().manual_seed(1))
    ref = sg.definition(v, t, S0, B0, True)
    out = sg.run(v, t, S0, B0, "fp32", True, DEV)
    assert float(out["loss"]) != 0.0 and out["gv"].any() and out["gt"].any() and float(out["gs"]) != 0.0 and float(out["gb"]) != 0.0
    sg.check(out, ref, "fp32", "B=1")
    for s, beta in ((0.0, -2.0), (-5.0, -3.0), (10.0, 0.0)):
        a, b, ref = sg.reference_case("randn", 70, 48, 1, s, beta, True)
        out = sg.run(a, b, s, beta, "fp32", True, DEV)
        sg.check(out, ref, "fp32", "scale")
        sg.check_rows(out, ref, "scale")
    a, b, ref = sg.exact_case("inter", 70, 48, 16)
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        out = sg.run(a.to(dtype), b.to(dtype), *sg.EXACT_SB, "fp32", True, DEV)
        assert out["loss"].dtype == (torch.float64 if dtype == torch.float64 else torch.float32) and out["gv"].dtype == dtype
        assert abs(float(out["loss"]) - ref["loss"]) <= sg.loss_bar(ref)
    with pytest.raises(RuntimeError, match="logit_scale is on"):
        crossclr_amd.sigmoid_loss(a.to(DEV), b.to(DEV), torch.tensor(2.0))
    with pytest.raises(RuntimeError, match="logit_bias is on"):
        crossclr_amd.sigmoid_loss(a.to(DEV), b.to(DEV), 2.0, torch.tensor(2.0))


LARGE = [(1000, 300), (2048, 512), (130, 1100)]


@pytest.mark.parametrize("kind,mode", [("cluster", "fp32"), ("randn", "fp32"), ("randn", "bf16")])
@pytest.mark.parametrize("B,D", LARGE)
def test_larger_shapes(B, D, kind, mode):
    lib, plan = nat.library(), nat.make_plan(B, D, 1, 0, nat.MODE_BF16 if mode == "bf16" else nat.MODE_FP32)
    if B >= 1000:
        assert lib.crossclr_sigmoid_splits(plan, 0) > 1 and plan.bpad // 128 > 1 and plan.bwd_slices > 1      # several splits, blocks, slices
    else:
        assert plan.Dpad // 256 > 1      # several D slices
    out, ref = sg.check_case(kind, B, D, B + D, S0, B0, mode, DEV)
    sg.check_rows(out, ref, f"{kind} B={B} D={D} {mode}")


def test_exact_operands_at_2048_rows():
    v, t = xi.planted("inter", 2048, 256, seed=2048 + 256, gram=False)
    ref = sg.definition(v, t, *sg.EXACT_SB, True)
    sg.check_exact_outputs(v, t, ref, DEV, "exact B=2048 D=256")


def test_forward_and_backward_are_graph_capturable_with_a_device_scale_and_bias():
    B, D = 512, 256
    v0, t0 = sg.inputs("randn", B, D, 1)
    v1, t1 = sg.inputs("randn", B, D, 2)
    (s0, b0), (s1, b1) = (S0, B0), (31.5, -4.25)
    sv, st = v0.to(DEV).requires_grad_(True), t0.to(DEV).requires_grad_(True)
    ss = torch.tensor(s0, dtype=torch.float32, device=DEV, requires_grad=True)
    sb = torch.tensor(b0, dtype=torch.float32, device=DEV, requires_grad=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # warm-up off the default stream, as torch's capture rules ask
        for _ in range(2):
            sv.grad = st.grad = ss.grad = sb.grad = None
            crossclr_amd.sigmoid_loss(sv, st, ss, sb).backward()
    torch.cuda.current_stream().wait_stream(side)
    sv.grad = st.grad = ss.grad = sb.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = crossclr_amd.sigmoid_loss(sv, st, ss, sb)
        static_loss.backward()
    with torch.no_grad():
        sv.copy_(v1.to(DEV))
        st.copy_(t1.to(DEV))
        ss.fill_(s1)
        sb.fill_(b1)
    graph.replay()
    torch.cuda.synchronize()
    ev, et = v1.to(DEV).requires_grad_(True), t1.to(DEV).requires_grad_(True)
    es = torch.tensor(s1, dtype=torch.float32, device=DEV, requires_grad=True)
    eb = torch.tensor(b1, dtype=torch.float32, device=DEV, requires_grad=True)
    eager = crossclr_amd.sigmoid_loss(ev, et, es, eb)
    eager.backward()
    torch.cuda.synchronize()
    assert static_loss.item() == eager.item()
    assert torch.equal(sv.grad, ev.grad) and torch.equal(st.grad, et.grad) and torch.equal(ss.grad, es.grad) and torch.equal(sb.grad, eb.grad)
    # and the values are those of the NEW scale and bias
    ref = sg.definition(v1, t1, s1, b1, True, grad_out=1.0)
    sg.check(dict(loss=eager.detach(), gv=ev.grad, gt=et.grad, gs=es.grad, gb=eb.grad), ref, "fp32", "replayed")


def test_the_module_on_the_device():
    m = crossclr_amd.SigmoidLoss(init_logit_scale=20.0, init_logit_bias=-5.0, compute_mode="bf16x3").to(DEV)
    v, t = sg.inputs("randn", 257, 72, 2)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    before_s, before_b = m.logit_scale.detach().clone(), m.logit_bias.detach().clone()
    m(v.to(DEV), t.to(DEV)).backward()
    ref = sg.definition(v, t, 20.0, -5.0, True, grad_out=1.0)
    assert abs(float(m.logit_scale.grad) - ref["gs"] * 20.0) <= 2e-4 * ref["A_s"] * 20.0 + 1e-6 * abs(ref["gs"] * 20.0)
    assert abs(float(m.logit_bias.grad) - ref["gb"]) <= 2e-4 * ref["A_b"]
    opt.step()
    assert not torch.equal(m.logit_scale.detach(), before_s) and not torch.equal(m.logit_bias.detach(), before_b)
