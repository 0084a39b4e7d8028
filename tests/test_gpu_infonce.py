"""The symmetric InfoNCE loss with a device-resident logit scale on the MI355X: the checks of tests/test_infonce_cpu.py
(tests/infonce_cases.py: the float64 definition and the bars) on the device, and shapes with several row blocks, column splits, gradient
slices and D slices.  grad_out = 3 throughout.

LARGER SHAPES, (B, D) = (1000, 300), (2048, 512) and (130, 1100), s = 1 / 0.07, against the float64 definition computed once per input:
fp32 on `make_inputs("cluster" / "randn", B, D, seed = B + D)` with normalize=True; bf16 on the randn rows as
F.normalize(x).bfloat16().float() fed with normalize=False (the bf16 bars are stated for the same bf16-exact operands, and a float64
model with bf16 weights puts the 16-cluster kind at 1.1e-2 of max|grad|, beyond the 1e-2 bar: cluster inputs are checked in fp32 only).
One exact-operand case at B = 2048, D = 256 (16 row blocks): lse, pair and loss are the same bits in all three modes.

GRAPH CAPTURE: forward + backward with a tensor scale captured into a HIP graph; the inputs AND the scale are overwritten in place and the
graph replayed: loss and all three gradients equal an eager run with the new values bit for bit -- nothing reads the scale on the host.

MEASURED on the MI355X, worst error / bar over all cases of this file (every test prints each figure beside its bar): fp32 loss 0.05,
gradients 0.08, dL/ds 0.01; bf16x3 loss 0.20, gradients 0.59 (cluster, B = 300, D = 40, s = 100), dL/ds 0.07; bf16 loss 0.49, gradients
0.48 (normalize=True against the exact definition, bar 1e-2), dL/ds 0.10.  The bars are the project's, not tightened."""
import pytest
import torch

import crossclr_amd
import exact_inputs as xi
import infonce_cases as ic
from crossclr_amd import _native as nat
from crossclr_amd import infonce as N

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.fixture(autouse=True)
def _hip_only():
    nat.use_library_for_testing(None)
    assert nat.backend() == "hip-gfx950", "GPU tests must run the HIP library"
    yield


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
    ic.check_case("anti", B, D, B + D, 4.0, "fp32", DEV, normalize=False)


@pytest.mark.parametrize("B,D", [(130, 200), (300, 40)])
def test_split_counts(B, D):
    ic.check_splits(B, D, DEV)


def test_edges_on_the_device():
    v, t = torch.randn(1, 24, generator=torch.Generator().manual_seed(0)), torch.randn(1, 24, generator=torch.Generator().manual_seed(1))
    out = ic.run(v, t, 1 / 0.07, "fp32", True, DEV)
    assert float(out["loss"]) == 0.0 and not out["gv"].any() and not out["gt"].any() and float(out["gs"]) == 0.0
    for s in (0.0, -5.0):
        a, b, ref = ic.reference_case("randn", 70, 48, 1, s, True)
        ic.check(ic.run(a, b, s, "fp32", True, DEV), ref, "fp32", "scale")
    a, b, ref = ic.exact_case("inter", 70, 48, 16)
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        out = ic.run(a.to(dtype), b.to(dtype), ic.EXACT_SCALE, "fp32", True, DEV)
        assert out["loss"].dtype == (torch.float64 if dtype == torch.float64 else torch.float32) and out["gv"].dtype == dtype
        assert abs(float(out["loss"]) - ref["loss"]) <= ic.loss_bar(ref)
    with pytest.raises(RuntimeError, match="logit_scale is on"):
        crossclr_amd.info_nce_loss(a.to(DEV), b.to(DEV), torch.tensor(2.0))


LARGE = [(1000, 300), (2048, 512), (130, 1100)]


@pytest.mark.parametrize("kind,mode", [("cluster", "fp32"), ("randn", "fp32"), ("randn", "bf16")])
@pytest.mark.parametrize("B,D", LARGE)
def test_larger_shapes(B, D, kind, mode):
    lib, plan = nat.library(), nat.make_plan(B, D, 1, 0, nat.MODE_BF16 if mode == "bf16" else nat.MODE_FP32)
    if B >= 1000:
        assert lib.crossclr_infonce_splits(plan, 0) > 1 and plan.bpad // 128 > 1 and plan.bwd_slices > 1      # a real merge, several slices
    else:
        assert plan.Dpad // 256 > 1      # several D slices
    out, ref = ic.check_case(kind, B, D, B + D, ic.SCALES[0], mode, DEV)
    ic.check_lse(out, ref, f"{kind} B={B} D={D} {mode}")


def test_exact_operands_at_2048_rows():
    v, t = xi.planted("inter", 2048, 256, seed=2048 + 256, gram=False)
    ref = ic.definition(v, t, ic.EXACT_SCALE, True)
    outs = {mode: ic.run(v, t, ic.EXACT_SCALE, mode, True, DEV) for mode in ic.MODES}
    for mode in ic.MODES[1:]:
        for key in ("lse", "pair", "loss"):
            assert torch.equal(outs[mode][key], outs["fp32"][key]), f"{key} differs between fp32 and {mode}"
    ic.check_lse(outs["fp32"], ref, "exact B=2048 D=256")
    for mode in ic.MODES:
        ic.check(outs[mode], ref, mode, "exact B=2048 D=256")


def test_forward_and_backward_are_graph_capturable_with_a_device_scale():
    B, D = 512, 256
    v0, t0 = ic.inputs("randn", B, D, 1)
    v1, t1 = ic.inputs("randn", B, D, 2)
    s0, s1 = 1 / 0.07, 31.5
    sv, st = v0.to(DEV).requires_grad_(True), t0.to(DEV).requires_grad_(True)
    ss = torch.tensor(s0, dtype=torch.float32, device=DEV, requires_grad=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # warm-up off the default stream, as torch's capture rules ask
        for _ in range(2):
            sv.grad = st.grad = ss.grad = None
            crossclr_amd.info_nce_loss(sv, st, ss).backward()
    torch.cuda.current_stream().wait_stream(side)
    sv.grad = st.grad = ss.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = crossclr_amd.info_nce_loss(sv, st, ss)
        static_loss.backward()
    with torch.no_grad():
        sv.copy_(v1.to(DEV))
        st.copy_(t1.to(DEV))
        ss.fill_(s1)
    graph.replay()
    torch.cuda.synchronize()
    ev, et = v1.to(DEV).requires_grad_(True), t1.to(DEV).requires_grad_(True)
    es = torch.tensor(s1, dtype=torch.float32, device=DEV, requires_grad=True)
    eager = crossclr_amd.info_nce_loss(ev, et, es)
    eager.backward()
    torch.cuda.synchronize()
    assert static_loss.item() == eager.item()
    assert torch.equal(sv.grad, ev.grad) and torch.equal(st.grad, et.grad) and torch.equal(ss.grad, es.grad)
    # and the values are those of the NEW scale
    ref = ic.definition(v1, t1, s1, True, grad_out=1.0)
    ic.check(dict(loss=eager.detach(), gv=ev.grad, gt=et.grad, gs=es.grad), ref, "fp32", "replayed")


def test_the_module_on_the_device():
    m = crossclr_amd.InfoNCE(temperature=0.05, compute_mode="bf16x3").to(DEV)
    v, t = ic.inputs("randn", 257, 72, 2)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    before = m.logit_scale.detach().clone()
    m(v.to(DEV), t.to(DEV)).backward()
    ref = ic.definition(v, t, 20.0, True, grad_out=1.0)
    assert abs(float(m.logit_scale.grad) - ref["gs"] * 20.0) <= 2e-4 * ref["A"] * 20.0 + 1e-6 * abs(ref["gs"] * 20.0)
    opt.step()
    assert not torch.equal(m.logit_scale.detach(), before)
