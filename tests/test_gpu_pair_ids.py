"""pair_ids on the InfoNCE and the sigmoid loss on the MI355X (same-item pairs are excluded from the negatives): the checks of
tests/test_pair_ids_cpu.py (tests/pair_ids_cases.py: the float64 definitions, the id patterns) on the device, and

LARGER SHAPES, (B, D) = (1000, 300) and (2048, 512), runs3 and stride7, both losses, against one float64 definition per input: fp32 on
`make_inputs("randn", B, D, seed = B + D)`; bf16 on those rows as F.normalize(x).bfloat16().float() fed with normalize=False.  The plans
have several column splits, row blocks and gradient slices.

GRAPH CAPTURE at B = 512, D = 256: forward + backward with a device ids tensor captured into a HIP graph; the inputs, the scale AND THE
IDS are overwritten in place (runs3 -> stride7) and the graph replayed: loss and gradients equal an eager run with the new values bit for
bit -- nothing reads the ids on the host -- and meet the definition at the fp32 bars.  grad_out = 3 in the other tests."""
import pytest
import torch

import crossclr_amd
import infonce_cases as ic
import pair_ids_cases as pc
import sigmoid_cases as sc
from crossclr_amd import _native as nat

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.fixture(autouse=True)
def _hip_only():
    nat.use_library_for_testing(None)
    assert nat.backend() == "hip-gfx950", "GPU tests must run the HIP library"
    yield


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("pattern", ("runs3", "stride7"))
@pytest.mark.parametrize("B,D,seed", pc.RANDOM_CASES)
def test_infonce_against_the_definition(B, D, seed, pattern, mode):
    pc.check_infonce_case(B, D, seed, ic.SCALES[0], mode, pattern, DEV)


@pytest.mark.parametrize("mode", ("fp32", "bf16x3"))
@pytest.mark.parametrize("pattern", ("runs3", "stride7"))
@pytest.mark.parametrize("B,D,seed", [(257, 72, 2), (300, 40, 5)])
def test_infonce_against_the_definition_at_scale_100(B, D, seed, pattern, mode):
    pc.check_infonce_case(B, D, seed, 100.0, mode, pattern, DEV)


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("s,beta", [(10.0, -10.0), (100.0, -10.0)])
@pytest.mark.parametrize("pattern", ("runs3", "stride7"))
@pytest.mark.parametrize("B,D,seed", pc.RANDOM_CASES)
def test_sigmoid_against_the_definition(B, D, seed, pattern, s, beta, mode):
    pc.check_sigmoid_case(B, D, seed, s, beta, mode, pattern, DEV)


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("B,D", [(70, 48), (257, 72)])
def test_distinct_ids_give_the_bits_of_none(B, D, mode):
    pc.check_distinct_ids_give_the_bits_of_none(B, D, mode, DEV)


@pytest.mark.parametrize("pattern", ("runs3", "stride7"))
def test_labelling_does_not_matter(pattern):
    pc.check_labelling_does_not_matter(pattern, DEV)


def test_the_ids_matter():
    pc.check_the_ids_matter(DEV)


@pytest.mark.parametrize("mode", ("fp32", "bf16x3"))
@pytest.mark.parametrize("B,D", [(8, 16), (300, 40)])
def test_all_ids_equal(B, D, mode):
    pc.check_equal_ids(B, D, mode, DEV)


@pytest.mark.parametrize("B,D", pc.SHAPES)
def test_dominant_excluded_entries(B, D):
    pc.check_dominant_excluded_entries(B, D, DEV)


def test_split_counts():
    pc.check_splits(DEV)


def test_the_interface():
    pc.check_interface(DEV)
    v, t = (x.to(DEV) for x in ic.inputs("randn", 8, 16, 0))
    with pytest.raises(RuntimeError, match="pair_ids is on"):
        crossclr_amd.info_nce_loss(v, t, pair_ids=torch.arange(8))
    with pytest.raises(RuntimeError, match="pair_ids is on"):
        crossclr_amd.sigmoid_loss(v, t, pair_ids=torch.arange(8))


def test_a_module_step_on_the_device():
    pc.check_module_step(DEV, mode="bf16x3")


LARGE = [(1000, 300), (2048, 512)]


@pytest.mark.parametrize("mode", ("fp32", "bf16"))
@pytest.mark.parametrize("pattern", ("runs3", "stride7"))
@pytest.mark.parametrize("B,D", LARGE)
def test_larger_shapes(B, D, pattern, mode):
    lib, plan = nat.library(), nat.make_plan(B, D, 1, 0, nat.MODE_BF16 if mode == "bf16" else nat.MODE_FP32)
    assert lib.crossclr_infonce_splits(plan, 0) > 1 and lib.crossclr_sigmoid_splits(plan, 0) > 1      # a real merge,
    assert plan.bpad // 128 > 1 and plan.bwd_slices > 1                                                 # several row blocks and slices
    pc.check_infonce_case(B, D, B + D, ic.SCALES[0], mode, pattern, DEV)
    pc.check_sigmoid_case(B, D, B + D, 10.0, -10.0, mode, pattern, DEV)


def _capture_and_replay(loss_fn, params0, params1, B=512, D=256):
    """Capture loss_fn(v, t, *params, ids) + backward with static tensors (inputs 1, params0, runs3), overwrite everything in place
    (inputs 2, params1, stride7), replay; an eager run on the new values.  Returns (static loss, static grads, eager loss, eager grads)."""
    v0, t0 = ic.inputs("randn", B, D, 1)
    v1, t1 = ic.inputs("randn", B, D, 2)
    ids0, ids1 = pc.ids_of("runs3", B), pc.ids_of("stride7", B)
    leaves = [v0.to(DEV).requires_grad_(True), t0.to(DEV).requires_grad_(True)]
    leaves += [torch.tensor(p, dtype=torch.float32, device=DEV, requires_grad=True) for p in params0]
    sid = ids0.to(DEV)

    def clear():
        for x in leaves:
            x.grad = None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # warm-up off the default stream, as torch's capture rules ask
        for _ in range(2):
            clear()
            loss_fn(*leaves, sid).backward()
    torch.cuda.current_stream().wait_stream(side)
    clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = loss_fn(*leaves, sid)
        static_loss.backward()
    with torch.no_grad():
        leaves[0].copy_(v1.to(DEV))
        leaves[1].copy_(t1.to(DEV))
        for x, p in zip(leaves[2:], params1):
            x.fill_(p)
        sid.copy_(ids1.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager = [v1.to(DEV).requires_grad_(True), t1.to(DEV).requires_grad_(True)]
    eager += [torch.tensor(p, dtype=torch.float32, device=DEV, requires_grad=True) for p in params1]
    eager_loss = loss_fn(*eager, ids1.to(DEV))
    eager_loss.backward()
    torch.cuda.synchronize()
    assert static_loss.item() == eager_loss.item()
    for x, y in zip(leaves, eager):
        assert torch.equal(x.grad, y.grad)
    return v1, t1, ids1, eager_loss.detach(), [x.grad for x in eager]


def test_infonce_is_graph_capturable_with_device_ids():
    s0, s1 = 1 / 0.07, 31.5
    v1, t1, ids1, loss, grads = _capture_and_replay(lambda v, t, s, ids: crossclr_amd.info_nce_loss(v, t, s, pair_ids=ids), (s0,), (s1,))
    ref = pc.infonce_definition(v1, t1, s1, True, ids1, grad_out=1.0)      # the values are those of the NEW scale and the NEW ids
    ic.check(dict(loss=loss, gv=grads[0], gt=grads[1], gs=grads[2]), ref, "fp32", "replayed")


def test_sigmoid_is_graph_capturable_with_device_ids():
    p0, p1 = (10.0, -10.0), (31.5, -4.0)
    v1, t1, ids1, loss, grads = _capture_and_replay(lambda v, t, s, b, ids: crossclr_amd.sigmoid_loss(v, t, s, b, pair_ids=ids), p0, p1)
    ref = pc.sigmoid_definition(v1, t1, *p1, True, ids1, grad_out=1.0)
    sc.check(dict(loss=loss, gv=grads[0], gt=grads[1], gs=grads[2], gb=grads[3]), ref, "fp32", "replayed")
