"""Parity of the HIP path (through the nn.Module and the C-ABI) with the reference on the MI355X.

Bars (BASELINE.json north_star): |loss - reference| <= 1e-3, gradients within 1e-2 of max|grad|.
compute_mode="fp32" is held to much tighter bounds (it is an exact-fp32 MFMA path); "bf16" is held
to the stated bars on the configurations the bars are stated for, and on toy shapes to the
bf16-operand numerical model in the oracle (what a correct bf16 kernel must produce)."""
import ctypes

import numpy as np
import pytest
import torch

import crossclr_amd
import fwd_sums_table as fst
from conftest import golden_arrays, golden_index, golden_inputs
from crossclr_amd import _native as nat
from crossclr_amd import loss as L
from oracle import crossclr_oracle as orc

pytestmark = pytest.mark.gpu
IDX = golden_index()
FULL = [n for n, m in IDX.items() if m["B"] <= 256]
SAMPLED = [n for n, m in IDX.items() if m["B"] > 256]


@pytest.fixture(autouse=True)
def _hip_only():
    nat.use_library_for_testing(None)
    assert nat.backend() == "hip-gfx950", "GPU tests must run the HIP library"
    yield


def run_module(v, t, m, mode, grad_scale=1.0):
    crit = crossclr_amd.CrossCLR_onlyIntraModality(m["temperature"], m["negative_weight"], compute_mode=mode).cuda()
    vd = v.cuda().requires_grad_(True)
    td = t.cuda().requires_grad_(True)
    loss = crit(vd, td)
    (loss * grad_scale).backward()
    torch.cuda.synchronize()
    return loss, vd.grad, td.grad


@pytest.mark.parametrize("name", FULL)
def test_fp32_mode_matches_golden_loss_and_grads(name):
    m = IDX[name]
    v, t = golden_inputs(m)
    loss, gv, gt = run_module(v, t, m, "fp32")
    assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.is_cuda
    assert gv.dtype == v.dtype and gt.dtype == t.dtype
    half_in = m["dtype"] in ("float16", "bfloat16")
    # for fp16/bf16 inputs the reference itself computes in that precision (its own rounding noise is ~1e-3)
    ltol = 5e-3 if half_in else 2e-5 * max(1.0, abs(m["loss"]))
    assert abs(loss.item() - m["loss"]) <= ltol
    arr = golden_arrays(name)
    scale = max(m["grad_v_absmax"], m["grad_t_absmax"])
    # + fp32 cancellation floor: the positive-pair term (p_ii - 1)/(B tau) is formed in fp32 here and in
    # fp64 by the reference's softmax; it matters only where the gradient itself is ~1e-14 (aligned regime)
    # the reference forms its logits from an fp32 GEMM (loss.py:83-93): a 6e-8 rounding of a cosine is a 6e-8/tau error of
    # the logit, i.e. of the relative size of a soft-max weight -- at tau = 0.002 the reference's own noise is ~1e-4
    gtol = (2e-2 if half_in else max(2e-4, 4e-7 / m["temperature"])) * scale + 1e-7 / (m["B"] * m["temperature"])
    assert np.abs(gv.double().cpu().numpy() - arr["grad_v"].astype(np.float64)).max() <= gtol
    assert np.abs(gt.double().cpu().numpy() - arr["grad_t"].astype(np.float64)).max() <= gtol


@pytest.mark.parametrize("name", [n for n in FULL if IDX[n]["dtype"] == "float32"])
def test_bf16_mode_matches_bf16_operand_model(name):
    m = IDX[name]
    v, t = golden_inputs(m)
    loss, gv, gt = run_module(v, t, m, "bf16")
    model = float(orc.bf16_operand_model_loss(v, t, m["temperature"], m["negative_weight"]))
    assert abs(loss.item() - model) <= 5e-5 * max(1.0, abs(model))
    arr = golden_arrays(name)
    scale = max(m["grad_v_absmax"], m["grad_t_absmax"])
    # (the aligned regime has gradients ~1e-11: below what bf16 operands resolve; and a bf16 cosine (2^-9) times 1/tau is a
    # logit error of 0.1-1 at tau <= 0.005: the gradient bar is stated, and held, at the reference's default temperature range)
    if m["loss"] > 1e-3 and m["temperature"] >= 0.02:
        assert np.abs(gv.double().cpu().numpy() - arr["grad_v"].astype(np.float64)).max() <= 2e-2 * scale
        assert np.abs(gt.double().cpu().numpy() - arr["grad_t"].astype(np.float64)).max() <= 2e-2 * scale


@pytest.mark.parametrize("name", ["g1_b64_d256_s0", "g1_b64_d256_s7", "g1_b64_d256_s1234", "g3_b256_d512_s2"])
def test_bf16_mode_meets_the_stated_bars_on_baseline_config1(name):
    m = IDX[name]
    v, t = golden_inputs(m)
    loss, gv, gt = run_module(v, t, m, "bf16")
    assert abs(loss.item() - m["loss"]) <= 1e-3
    arr = golden_arrays(name)
    scale = max(m["grad_v_absmax"], m["grad_t_absmax"])
    assert np.abs(gv.cpu().numpy() - arr["grad_v"]).max() <= 1e-2 * scale
    assert np.abs(gt.cpu().numpy() - arr["grad_t"]).max() <= 1e-2 * scale


@pytest.mark.parametrize("name", SAMPLED)
@pytest.mark.parametrize("mode", ["fp32", "bf16", "auto"])
def test_large_cases_sampled_rows(name, mode):
    m = IDX[name]
    v, t = golden_inputs(m)
    loss, gv, gt = run_module(v, t, m, mode)
    if name == "g7_b8192_d512_s1234" and mode == "bf16":
        # this case is what pins the fragment-major saved backwards to the REFERENCE's goldens (tests/test_gpu_xf.py compares them with
        # the LDS-staged kernel only): make sure it really ran one of them -- the pair kernel unless the self-test rejected it
        took = [k[3] for k, ok in L._xf_verified.items() if ok and k[1] == 512 and not k[2]]
        assert "crossclr_backward_saved_xfp" in took or "crossclr_backward_saved_xf" in took, L._xf_verified
    small_tau = max(1.0, abs(m["negative_weight"])) / m["temperature"] > 128      # two-pass regime: "auto" computes in fp32 there
    exact = mode == "fp32" or (mode == "auto" and small_tau)
    # explicit bf16 at small temperatures: a bf16 cosine (2^-9) times 1/tau -- the bars are stated at tau = 0.03
    coarse = (0.03 / m["temperature"]) ** 2 if (small_tau and not exact) else 1.0
    ltol = 2e-5 * max(1.0, abs(m["loss"])) if exact else 1e-3 * coarse
    assert abs(loss.item() - m["loss"]) <= ltol, (loss.item(), m["loss"])
    arr = golden_arrays(name)
    rows = arr["rows"]
    scale = max(m["grad_v_absmax"], m["grad_t_absmax"])
    if m["loss"] > 1e-3 and coarse == 1.0:
        mode = "fp32" if exact else mode
        gtol = (max(2e-4, 4e-7 / m["temperature"]) if mode == "fp32" else 1e-2) * scale
        assert np.abs(gv[rows].cpu().numpy() - arr["grad_v_rows"]).max() <= gtol
        assert np.abs(gt[rows].cpu().numpy() - arr["grad_t_rows"]).max() <= gtol
        # norms of the whole gradient (catches errors outside the sampled rows)
        assert abs(gv.double().norm().item() - m["grad_v_norm"]) <= (1e-3 if mode == "fp32" else 1e-2) * m["grad_v_norm"]
        assert abs(gt.double().norm().item() - m["grad_t_norm"]) <= (1e-3 if mode == "fp32" else 1e-2) * m["grad_t_norm"]


def test_config2_forward_only_fp32_b4096():
    # BASELINE.json configs[1]: fused forward-only kernel, B=4096 D=512 fp32, parity <= 1e-3 vs CPU
    m = IDX["g7_b4096_d512_s1234"]
    v, t = golden_inputs(m)
    with torch.no_grad():
        loss = crossclr_amd.crossclr_loss(v.cuda(), t.cuda(), 0.03, 0.8, compute_mode="fp32")
    assert not loss.requires_grad
    assert abs(loss.item() - m["loss"]) <= 1e-3
    assert abs(loss.item() - m["loss"]) <= 5e-5  # what exact-fp32 MFMA actually achieves


def test_per_row_statistics_match_oracle():
    m = IDX["g3_b256_d512_s2"]
    v, t = golden_inputs(m)
    arr = golden_arrays("g3_b256_d512_s2")
    _, ws = L._forward_impl(v.cuda(), t.cuda(), 0.03, 0.8, "fp32", None)
    torch.cuda.synchronize()
    bp = ws.plan.bpad
    logz = ws.logz.cpu().double().numpy()
    assert np.abs(logz[:256] - arr["logZv"]).max() <= 2e-5
    assert np.abs(logz[bp:bp + 256] - arr["logZt"]).max() <= 2e-5
    assert np.abs(ws.diag.cpu().double().numpy()[:256] / 0.03 - arr["diag"]).max() <= 2e-5
    assert (ws.rz.cpu()[256:bp] == 0).all(), "padding rows must carry zero weight"


# ----------------------------------------------------------------------------------------------
# size-independent properties at the BASELINE size (B=8192, D=512, bf16)
# ----------------------------------------------------------------------------------------------
def test_properties_at_full_size():
    B, D = 8192, 512
    v, t = orc.make_inputs("randn", B, D, 99)
    vd, td = v.cuda(), t.cuda()
    base = crossclr_amd.crossclr_loss(vd, td, 0.03, 0.8, compute_mode="bf16").item()
    # (1) the loss is invariant under a common permutation of the batch (a sum over rows)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).cuda()
    assert abs(crossclr_amd.crossclr_loss(vd[perm], td[perm], 0.03, 0.8, compute_mode="bf16").item() - base) <= 1e-6
    # (2) positive row scaling leaves it unchanged (rows are L2-normalised first) -- power-of-two scale is exact
    assert abs(crossclr_amd.crossclr_loss(vd * 4.0, td * 0.5, 0.03, 0.8, compute_mode="bf16").item() - base) <= 1e-9
    # (3) swapping the modalities leaves it unchanged (the loss is symmetric in video/text)
    assert abs(crossclr_amd.crossclr_loss(td, vd, 0.03, 0.8, compute_mode="bf16").item() - base) <= 1e-6
    # (4) gradients are linear in grad_output and orthogonal to their own rows (normalise backward)
    m = dict(temperature=0.03, negative_weight=0.8)
    _, gv1, gt1 = run_module(v, t, m, "bf16", 1.0)
    _, gv3, gt3 = run_module(v, t, m, "bf16", -3.0)
    assert torch.allclose(gv3, -3.0 * gv1, rtol=1e-5, atol=1e-12) and torch.allclose(gt3, -3.0 * gt1, rtol=1e-5, atol=1e-12)
    radial = (gv1.double() * vd.double()).sum(1).abs().max().item()
    assert radial <= 1e-3 * gv1.double().norm(dim=1).max().item() * vd.double().norm(dim=1).max().item()
    # (5) fp32 and bf16 modes agree within the stated bar
    f32 = crossclr_amd.crossclr_loss(vd, td, 0.03, 0.8, compute_mode="fp32").item()
    assert abs(f32 - base) <= 1e-3
    # (6) deterministic: same inputs, same bits
    assert crossclr_amd.crossclr_loss(vd, td, 0.03, 0.8, compute_mode="bf16").item() == base


def _shard_via_cabi(v, t, world, mode, saved=False):
    """Drive the C-ABI exactly like `world` ranks would, on one GPU: every rank normalises its rows
    into its slice of the gathered operand, then forward/backward run against all column ranks.
    saved (exact-fp32 plans): the local block and the block against the other ranks save their fp32 exponentials
    (crossclr_forward_save / crossclr_forward_rect_save) and the backward is the gradient product alone (crossclr_backward_saved /
    crossclr_backward_rect_saved on bwd_saved32_kernel)."""
    lib = nat.library()
    p = L._ptr
    B, D = v.shape
    b = B // world
    dev = v.device
    stream = L._stream_for(v)
    plans = [nat.make_plan(b, D, world, r, mode) for r in range(world)]
    pl = plans[0]
    xall = torch.empty(world * pl.operand_bytes, dtype=torch.uint8, device=dev)
    inv = [torch.empty(2 * pl.bpad, device=dev) for _ in range(world)]
    diag = [torch.empty(pl.bpad, device=dev) for _ in range(world)]
    f32 = dict(dtype=torch.float32, device=dev)
    for r in range(world):
        xr = xall[r * pl.operand_bytes:(r + 1) * pl.operand_bytes]
        nat.check(lib.crossclr_normalize(ctypes.byref(plans[r]), p(v[r * b:]), p(t[r * b:]), v.stride(0), t.stride(0),
                                         nat.IN_F32, p(xr), p(inv[r]), p(diag[r]), stream))
    rz = torch.empty(world, 2 * pl.bpad, **f32)
    wrz = torch.empty(world, 2 * pl.bpad, **f32)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    stashes = []
    for r in range(world):
        pp = ctypes.byref(plans[r])
        xr = xall[r * pl.operand_bytes:(r + 1) * pl.operand_bytes]
        part = torch.empty(pl.fwd_ws_floats, **f32)
        # local block first, then every other rank's columns (skip_rank = r): the overlap schedule
        if saved:
            stashes.append((torch.empty(pl.stash_bytes, dtype=torch.uint8, device=dev),
                            torch.empty(lib.crossclr_rect_stash_bytes(pp, world - 1), dtype=torch.uint8, device=dev)))
            assert stashes[-1][1].numel() > 0
            nat.check(lib.crossclr_forward_save(pp, p(xr), 0.03, 0.8, None, p(part), 0, p(stashes[-1][0]), stream))
            nat.check(lib.crossclr_forward_rect_save(pp, p(xr), p(xall), (r + 1) % world, world - 1, 0, 0.03, 0.8, None, p(part), pl.fwd_slots,
                                                     None, p(stashes[-1][1]), stream))
        else:
            nat.check(lib.crossclr_forward(pp, p(xr), p(xr), 1, r, -1, 0.03, 0.8, p(part), 0, stream))
            nat.check(lib.crossclr_forward(pp, p(xr), p(xall), world, 0, r, 0.03, 0.8, p(part), pl.fwd_slots, stream))
        logz = torch.empty(2 * pl.bpad, **f32)
        ls = torch.empty(pl.loss_ws_doubles, dtype=torch.float64, device=dev)
        nat.check(lib.crossclr_forward_finish(pp, p(part), 2 * pl.fwd_slots, p(diag[r]), 0.03, 0.8, p(logz), p(rz[r]),
                                              p(wrz[r]), p(ls), stream))
        total += ls[:1]
    loss = total / (2.0 * B)
    gv = torch.empty_like(v)
    gt = torch.empty_like(t)
    go = torch.ones(1, dtype=torch.float64, device=dev)
    for r in range(world):
        pp = ctypes.byref(plans[r])
        xr = xall[r * pl.operand_bytes:(r + 1) * pl.operand_bytes]
        gbuf = torch.empty(pl.gbuf_bytes // 4, **f32)
        if saved:
            nat.check(lib.crossclr_backward_saved(pp, p(xr), p(stashes[r][0]), 0.03, 0.8, p(rz[r]), p(wrz[r]), None, p(gbuf), 0, stream))
            nat.check(lib.crossclr_backward_rect_saved(pp, p(xall), p(stashes[r][1]), (r + 1) % world, world - 1, 0.03, 0.8, p(rz[r]), p(wrz[r]),
                                                       p(rz), p(wrz), None, p(gbuf), 1, stream))
        else:
            nat.check(lib.crossclr_backward(pp, p(xr), p(xr), 1, r, -1, 0.03, 0.8, p(rz[r]), p(wrz[r]), p(rz[r]), p(wrz[r]),
                                            p(gbuf), 0, stream))
            nat.check(lib.crossclr_backward(pp, p(xr), p(xall), world, 0, r, 0.03, 0.8, p(rz[r]), p(wrz[r]), p(rz), p(wrz),
                                            p(gbuf), 1, stream))
        nat.check(lib.crossclr_backward_finish(pp, p(gbuf), p(v[r * b:]), p(t[r * b:]), v.stride(0), t.stride(0),
                                               nat.IN_F32, p(inv[r]), 0.03, p(go), p(gv[r * b:]), p(gt[r * b:]),
                                               gv.stride(0), gt.stride(0), stream))
    torch.cuda.synchronize()
    return loss.item(), gv, gt


@pytest.mark.parametrize("world,B,D", [(2, 512, 128), (3, 300, 96), (4, 2048, 512), (8, 1024, 200)])
def test_fp32_sharded_blocks_from_saved_exponentials_equal_single_device(world, B, D):
    """Exact-fp32 sharded runs (round 4): the remote blocks save their fp32 exponentials too (rectangular stash of the generic forward) and the
    backward of those blocks is bwd_saved32_kernel<..., RECT>; one GPU plays every rank through the C-ABI; against the single-device module
    and the streaming float64 oracle."""
    v, t = orc.make_inputs("randn", B, D, 37)
    loss1, gv1, gt1 = run_module(v, t, dict(temperature=0.03, negative_weight=0.8), "fp32")
    lossN, gvN, gtN = _shard_via_cabi(v.cuda(), t.cuda(), world, nat.MODE_FP32, saved=True)
    assert abs(lossN - loss1.item()) <= 1e-6 * max(1.0, abs(lossN))
    scale = gv1.abs().max().item()
    assert (gvN - gv1).abs().max().item() <= 1e-5 * scale and (gtN - gt1).abs().max().item() <= 1e-5 * scale
    ref = orc.streaming_loss_and_grads(v, t, 0.03, 0.8)
    assert abs(lossN - float(ref["loss"])) <= 1e-5
    assert (gvN.double().cpu() - ref["grad_v"]).abs().max().item() <= 2e-4 * scale


@pytest.mark.parametrize("world,B,D", [(2, 512, 1100), (3, 768, 1536), (4, 2048, 2048), (8, 1024, 1300)])
def test_wide_bf16_sharded_blocks_from_saved_exponentials(world, B, D):
    """Wide bf16 plans (D > 1024) in a sharded run: the block against the other ranks saves bf16 records too (generic forward, rectangular
    layout) and its backward is the D-slice kernel in column parts (MODE 1); one GPU plays every rank through the C-ABI; against the
    recomputing pair of the same run and the streaming float64 oracle."""
    v, t = orc.make_inputs("randn", B, D, 43)
    lossS, gvS, gtS = _shard_via_cabi(v.cuda(), t.cuda(), world, nat.MODE_BF16, saved=True)
    lossR, gvR, gtR = _shard_via_cabi(v.cuda(), t.cuda(), world, nat.MODE_BF16, saved=False)
    ref = orc.streaming_loss_and_grads(v, t, 0.03, 0.8)
    scale = ref["grad_v"].abs().max().item()
    assert abs(lossS - lossR) <= 1e-5 * max(1.0, abs(lossR))            # the same exponentials, summed in another order
    assert abs(lossS - float(ref["loss"])) <= 1e-3
    # saved weights are rounded to bf16 before the product, recomputed ones are not: both within the bf16 bar of the oracle
    assert (gvS.double().cpu() - ref["grad_v"]).abs().max().item() <= 1e-2 * scale
    assert (gtS.double().cpu() - ref["grad_t"]).abs().max().item() <= 1e-2 * scale
    assert (gvS - gvR).abs().max().item() <= 1e-2 * scale


def _shard_two_pass_via_cabi(v, t, world, tau, w, saved, mode=nat.MODE_FP32):
    """The two-pass regime (tau < 0.0078) of an exact-fp32 sharded run through the C-ABI, one GPU playing every rank: row maxima over the
    local and the remote columns, the ranks' maxima "gathered", sums relative to them; saved: the local block and the block against the other
    ranks leave U and Ut behind (crossclr_forward_save_s / crossclr_forward_rect_save_s) and the backward recomputes nothing
    (crossclr_backward_saved_s / crossclr_backward_rect_saved_s); otherwise the recomputing pair (crossclr_forward_s / crossclr_backward_s)."""
    lib, p = nat.library(), L._ptr
    B, D = v.shape
    b, dev, stream = B // world, v.device, L._stream_for(v)
    plans = [nat.make_plan(b, D, world, r, mode) for r in range(world)]
    pl = plans[0]
    f32 = dict(dtype=torch.float32, device=dev)
    xall = torch.empty(world * pl.operand_bytes, dtype=torch.uint8, device=dev)
    inv = [torch.empty(2 * pl.bpad, **f32) for _ in range(world)]
    diag = [torch.empty(pl.bpad, **f32) for _ in range(world)]
    xs = [xall[r * pl.operand_bytes:(r + 1) * pl.operand_bytes] for r in range(world)]
    for r in range(world):
        nat.check(lib.crossclr_normalize(ctypes.byref(plans[r]), p(v[r * b:]), p(t[r * b:]), v.stride(0), t.stride(0), nat.IN_F32, p(xs[r]),
                                         p(inv[r]), p(diag[r]), stream))
    shift = torch.empty(world, 2 * pl.bpad, **f32)      # the "gathered" row maxima
    parts = [torch.empty(pl.fwd_ws_floats, **f32) for _ in range(world)]
    for r in range(world):
        pp = ctypes.byref(plans[r])
        nat.check(lib.crossclr_forward_rowmax(pp, p(xs[r]), p(xs[r]), 1, r, -1, tau, w, None, p(parts[r]), p(shift[r]), 0, stream))
        nat.check(lib.crossclr_forward_rowmax(pp, p(xs[r]), p(xall), world, 0, r, tau, w, None, p(parts[r]), p(shift[r]), 1, stream))
    rz, wrz = torch.empty(world, 2 * pl.bpad, **f32), torch.empty(world, 2 * pl.bpad, **f32)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    stashes = []
    for r in range(world):
        pp = ctypes.byref(plans[r])
        if saved:
            nb = lib.crossclr_rect_stash_bytes_s(pp, world - 1)
            assert nb >= 2 * lib.crossclr_rect_stash_bytes(pp, world - 1) > 0
            stashes.append((torch.empty(lib.crossclr_stash_bytes_s(pp), dtype=torch.uint8, device=dev), torch.empty(nb, dtype=torch.uint8, device=dev)))
            nat.check(lib.crossclr_forward_save_s(pp, p(xs[r]), tau, w, None, p(shift[r]), p(parts[r]), 0, p(stashes[r][0]), stream))
            nat.check(lib.crossclr_forward_rect_save_s(pp, p(xs[r]), p(xall), (r + 1) % world, world - 1, tau, w, None, p(shift[r]), p(shift),
                                                       p(parts[r]), pl.fwd_slots, p(stashes[r][1]), stream))
        else:
            nat.check(lib.crossclr_forward_s(pp, p(xs[r]), p(xs[r]), 1, r, -1, tau, w, None, p(shift[r]), p(parts[r]), 0, stream))
            nat.check(lib.crossclr_forward_s(pp, p(xs[r]), p(xall), world, 0, r, tau, w, None, p(shift[r]), p(parts[r]), pl.fwd_slots, stream))
        logz = torch.empty(2 * pl.bpad, **f32)
        ls = torch.empty(pl.loss_ws_doubles, dtype=torch.float64, device=dev)
        nat.check(lib.crossclr_forward_finish_s(pp, p(parts[r]), 2 * pl.fwd_slots, p(diag[r]), tau, w, None, p(shift[r]), p(logz), p(rz[r]),
                                                p(wrz[r]), p(ls), stream))
        total += ls[:1]
    loss = total / (2.0 * B)
    gv, gt = torch.empty_like(v), torch.empty_like(t)
    go = torch.ones(1, dtype=torch.float64, device=dev)
    for r in range(world):
        pp = ctypes.byref(plans[r])
        gbuf = torch.empty(pl.gbuf_bytes // 4, **f32)
        if saved:
            nat.check(lib.crossclr_backward_saved_s(pp, p(xs[r]), p(stashes[r][0]), tau, w, p(rz[r]), p(wrz[r]), None, p(gbuf), 0, stream))
            nat.check(lib.crossclr_backward_rect_saved_s(pp, p(xall), p(stashes[r][1]), (r + 1) % world, world - 1, tau, w, p(rz[r]), p(wrz[r]),
                                                         p(rz), p(wrz), None, p(gbuf), 1, stream))
        else:
            nat.check(lib.crossclr_backward_s(pp, p(xs[r]), p(xs[r]), 1, r, -1, tau, w, p(rz[r]), p(wrz[r]), p(rz[r]), p(wrz[r]), None,
                                              p(shift[r]), p(shift[r]), p(gbuf), 0, stream))
            nat.check(lib.crossclr_backward_s(pp, p(xs[r]), p(xall), world, 0, r, tau, w, p(rz[r]), p(wrz[r]), p(rz), p(wrz), None,
                                              p(shift[r]), p(shift), p(gbuf), 1, stream))
        nat.check(lib.crossclr_backward_finish(pp, p(gbuf), p(v[r * b:]), p(t[r * b:]), v.stride(0), t.stride(0), nat.IN_F32, p(inv[r]), tau,
                                               p(go), p(gv[r * b:]), p(gt[r * b:]), gv.stride(0), gt.stride(0), stream))
    torch.cuda.synchronize()
    return loss.item(), gv, gt


@pytest.mark.parametrize("world,B,D,tau", [(2, 512, 128, 0.005), (3, 300, 96, 0.004), (4, 2048, 512, 0.005), (8, 1024, 200, 0.002)])
def test_fp32_sharded_two_pass_blocks_from_saved_exponentials(world, B, D, tau):
    """Exact-fp32 sharded runs in the two-pass regime: the block against the other ranks saves U and Ut (the latter relative to the REMOTE rows'
    maxima) and its backward is bwd_saved32_kernel<..., RM, RECT>; against the recomputing pair of the same run, the single-device module and
    the streaming float64 oracle."""
    v, t = orc.make_inputs("randn", B, D, 41)
    lossS, gvS, gtS = _shard_two_pass_via_cabi(v.cuda(), t.cuda(), world, tau, 0.8, saved=True)
    lossR, gvR, gtR = _shard_two_pass_via_cabi(v.cuda(), t.cuda(), world, tau, 0.8, saved=False)
    loss1, gv1, gt1 = run_module(v, t, dict(temperature=tau, negative_weight=0.8), "fp32")
    scale = gv1.abs().max().item()
    assert abs(lossS - lossR) <= 1e-6 * max(1.0, abs(lossR)) and abs(lossS - loss1.item()) <= 1e-6 * max(1.0, abs(lossS))
    assert (gvS - gvR).abs().max().item() <= 1e-5 * scale and (gtS - gtR).abs().max().item() <= 1e-5 * scale
    assert (gvS - gv1).abs().max().item() <= 1e-5 * scale and (gtS - gt1).abs().max().item() <= 1e-5 * scale
    ref = orc.streaming_loss_and_grads(v, t, tau, 0.8)
    assert abs(lossS - float(ref["loss"])) <= 1e-4 * max(1.0, abs(float(ref["loss"])))
    assert (gvS.double().cpu() - ref["grad_v"]).abs().max().item() <= 1e-3 * scale


@pytest.mark.parametrize("world,B,D,tau", [(2, 512, 128, 0.005), (3, 300, 96, 0.004), (4, 2048, 512, 0.005), (8, 1024, 1000, 0.003),
                                           (2, 512, 1100, 0.005), (4, 1024, 1536, 0.004)])       # (the last two: wide plans, U and Ut for the local block too)
def test_bf16_sharded_two_pass_blocks_from_saved_exponentials(world, B, D, tau):
    """bf16 register-resident plans in the two-pass regime of a sharded run: the block against the other ranks saves bf16 records of U and of Ut
    and its backward is two rectangular launches of the saved D-slice kernel (rows' side, columns' side); against the recomputing pair of the
    same run and the streaming float64 oracle."""
    v, t = orc.make_inputs("randn", B, D, 47)
    lossS, gvS, gtS = _shard_two_pass_via_cabi(v.cuda(), t.cuda(), world, tau, 0.8, saved=True, mode=nat.MODE_BF16)
    lossR, gvR, gtR = _shard_two_pass_via_cabi(v.cuda(), t.cuda(), world, tau, 0.8, saved=False, mode=nat.MODE_BF16)
    ref = orc.streaming_loss_and_grads(v, t, tau, 0.8)
    scale = ref["grad_v"].abs().max().item()
    assert abs(lossS - lossR) <= 1e-5 * max(1.0, abs(lossR))
    assert abs(lossS - float(ref["loss"])) <= 2e-2 * max(1.0, abs(float(ref["loss"])))      # (the bars of the local block's test at these temperatures)
    assert (gvS - gvR).abs().max().item() <= 1e-2 * scale and (gtS - gtR).abs().max().item() <= 1e-2 * scale
    assert (gvS.double().cpu() - ref["grad_v"]).abs().max().item() <= 3e-2 * scale
    assert (gtS.double().cpu() - ref["grad_t"]).abs().max().item() <= 3e-2 * scale


@pytest.mark.parametrize("world,B,D,mode", [(2, 512, 128, nat.MODE_FP32), (4, 1024, 512, nat.MODE_BF16),
                                            (8, 2048, 512, nat.MODE_BF16), (3, 300, 96, nat.MODE_FP32)])
def test_sharded_kernel_path_equals_single_device(world, B, D, mode):
    """N-rank result == single-process result on the concatenated batch.  One GPU
    plays every rank through the same entry points a multi-GPU run uses (row_rank / col_ranks /
    skip_rank / accumulate)."""
    v, t = orc.make_inputs("randn", B, D, 31)
    vd, td = v.cuda(), t.cuda()
    mname = "fp32" if mode == nat.MODE_FP32 else "bf16"
    loss1, gv1, gt1 = run_module(v, t, dict(temperature=0.03, negative_weight=0.8), mname)
    lossN, gvN, gtN = _shard_via_cabi(vd, td, world, mode)
    assert abs(lossN - loss1.item()) <= 1e-6 * max(1.0, abs(lossN))
    scale = gv1.abs().max().item()
    tol = 1e-5 if mode == nat.MODE_FP32 else 2e-3  # bf16: W is rounded per 64-wide column tile in both
    assert (gvN - gv1).abs().max().item() <= tol * scale
    assert (gtN - gt1).abs().max().item() <= tol * scale
    ref = orc.streaming_loss_and_grads(v, t, 0.03, 0.8)
    assert abs(lossN - float(ref["loss"])) <= (1e-5 if mode == nat.MODE_FP32 else 1e-3)


# ----------------------------------------------------------------------------------------------
# drop-in behaviour on the device
# ----------------------------------------------------------------------------------------------
def test_module_device_behaviour():
    crit = crossclr_amd.CrossCLR_onlyIntraModality().cuda()
    v, t = orc.make_inputs("randn", 16, 32, 3)
    vd, td = v.cuda(), t.cuda()
    keep_v = vd.clone()
    loss = crit(vd, td)
    assert torch.equal(vd, keep_v), "inputs must not be modified"
    assert not loss.requires_grad
    # temperature / negative_w are read at call time
    crit.temperature = 0.1
    crit.negative_w = 0.0
    assert abs(crit(vd, td).item() - IDX["g5_w0_tau01_b16_d32"]["loss"]) <= 2e-5
    # non-leaf inputs, non-contiguous rows
    base = torch.randn(16, 64, device="cuda", requires_grad=True)
    vn = (base * 2.0)[:, ::2]
    out = crossclr_amd.crossclr_loss(vn, td.requires_grad_(True), compute_mode="fp32")
    out.backward()
    assert base.grad is not None and base.grad.shape == (16, 64) and crit.logit_scale.grad is None
    with pytest.raises(RuntimeError):
        crit(vd, td[:8])
    with pytest.raises(RuntimeError):
        crit(vd[None], td[None])
    with pytest.raises(RuntimeError):
        crit(v, t)  # CPU tensors: no CPU fallback
    # outside the fixed-shift range the module takes the two-pass soft-max (like the reference's float64 one): finite, right
    tiny = crossclr_amd.crossclr_loss(vd, td, temperature=0.001)
    ref = orc.streaming_stats(v, t, 0.001, 0.8)
    assert torch.isfinite(tiny) and abs(tiny.item() - float(ref["loss"])) <= 1e-4 * float(ref["loss"])


def test_sharded_host_path_with_real_collectives_on_one_gpu(monkeypatch):
    """The multi-rank code path end to end on the device: RCCL all_gather_into_tensor of the packed operand
    (async, overlapped with the local launch), the skip_rank launch, the statistics all-gather and the loss
    all-reduce -- with a 1-rank NCCL group (CROSSCLR_FORCE_SHARDED_PATH), which is all a 1-GPU box allows.
    Must reproduce the plain single-GPU result."""
    import os
    import torch.distributed as dist
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 300))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        for mode, B, D in (("bf16", 1024, 512), ("fp32", 200, 96)):
            v, t = orc.make_inputs("randn", B, D, 41)
            m = dict(temperature=0.03, negative_weight=0.8)
            loss1, gv1, gt1 = run_module(v, t, m, mode)
            monkeypatch.setenv("CROSSCLR_FORCE_SHARDED_PATH", "1")
            crit = crossclr_amd.CrossCLR_onlyIntraModality(0.03, 0.8, compute_mode=mode, process_group=dist.group.WORLD).cuda()
            vd = v.cuda().requires_grad_(True)
            td = t.cuda().requires_grad_(True)
            loss = crit(vd, td)
            loss.backward()
            torch.cuda.synchronize()
            monkeypatch.delenv("CROSSCLR_FORCE_SHARDED_PATH")
            assert abs(loss.item() - loss1.item()) <= 1e-9 * max(1.0, abs(loss1.item()))
            assert torch.equal(vd.grad, gv1) and torch.equal(td.grad, gt1)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("B,D,mode", [
    (1000, 100, "bf16"),    # D padded 100 -> 128 (DK=8), ragged batch
    (1536, 256, "bf16"),    # DK=16; bpad = 1536 (6 row blocks of 256)
    (1300, 384, "bf16"),    # DK=24 (48 KiB tiles), ragged, row block straddling the modality boundary
    (2048, 512, "bf16"),    # DK=32
    (640, 600, "bf16"),     # 512 < D <= 768: 4-wave persistent forward + 16-row-wave backward, Dpad = 768
    (512, 1024, "bf16"),    # BASELINE config 5's embedding width: 4-wave persistent forward + 16-row-wave backward
    (2048, 768, "bf16"),    # the common ViT-L / BERT width
    (300, 1100, "bf16"),    # D > 1024: generic tiled forward that saves bf16 records + the D-slice backward in 3 parts of 384 (Dpad = 1152)
    (1500, 1536, "bf16"),   # 3 parts of 512, ragged batch, several 128-row blocks (mirrored and direct tiles)
    (640, 2000, "bf16"),    # 4 parts of 512
    (384, 2300, "bf16"),    # 5 parts (Dpad = 2560)
    (256, 4096, "bf16"),    # 8 parts
    (200, 4500, "bf16"),    # 10 parts (Dpad = 5120; round 6: the saved D-slice backward up to D = 8192)
    (300, 6000, "bf16"),    # 12 parts
    (130, 8192, "bf16"),    # 16 parts
    (100, 8300, "bf16"),    # beyond 8192: the recomputing generic backward
    (777, 200, "fp32"),     # generic fp32, Dpad = 256
    (1024, 768, "fp32"),    # generic fp32, three backward slices
    (3000, 512, "auto"),    # auto -> bf16 (global batch >= 1024)
    (500, 512, "auto"),     # auto -> fp32
])
def test_shape_sweep_against_streaming_oracle(B, D, mode):
    v, t = orc.make_inputs("randn", B, D, 1000 + B + D)
    ref = orc.streaming_loss_and_grads(v, t, 0.03, 0.8, block=512)
    loss, gv, gt = run_module(v, t, dict(temperature=0.03, negative_weight=0.8), mode)
    exact = mode == "fp32" or (mode == "auto" and B < crossclr_amd.AUTO_BF16_MIN_GLOBAL_BATCH)
    assert abs(loss.item() - float(ref["loss"])) <= (2e-5 if exact else 1e-3)
    scale = max(ref["grad_v"].abs().max().item(), ref["grad_t"].abs().max().item())
    tol = (2e-4 if exact else 1e-2) * scale
    assert (gv.double().cpu() - ref["grad_v"]).abs().max().item() <= tol
    assert (gt.double().cpu() - ref["grad_t"]).abs().max().item() <= tol


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_input_dtypes_on_the_fast_path(dtype):
    # inputs in any float dtype; gradients come back in that dtype; loss stays float64
    v, t = orc.make_inputs("randn", 1280, 256, 9)
    v, t = v.to(dtype), t.to(dtype)
    ref = orc.streaming_loss_and_grads(v.double(), t.double(), 0.03, 0.8, block=512)
    loss, gv, gt = run_module(v, t, dict(temperature=0.03, negative_weight=0.8), "bf16")
    assert loss.dtype == torch.float64 and gv.dtype == dtype and gt.dtype == dtype
    assert abs(loss.item() - float(ref["loss"])) <= 1e-3
    scale = ref["grad_v"].abs().max().item()
    out_eps = {torch.float16: 1e-3, torch.bfloat16: 8e-3, torch.float64: 0.0}[dtype]  # rounding of the stored gradient
    assert (gv.double().cpu() - ref["grad_v"]).abs().max().item() <= (1e-2 + out_eps) * scale


def test_global_batch_scale_on_one_gpu():
    """B = 32768 (half of BASELINE's 8-GPU global batch) on one GPU: index arithmetic, workspace sizes and
    finiteness at scale.  The CPU oracle would take minutes here, so the checker is an independent blocked
    evaluation with stock torch ops on the device (fp32 GEMMs, fp64 logsumexp) -- the closed form of
    SURVEY.md 3.4, not the kernels under test."""
    B, D = 32768, 512
    gen = torch.Generator(device="cuda").manual_seed(5)
    v = torch.randn(B, D, device="cuda", generator=gen).requires_grad_(True)
    t = torch.randn(B, D, device="cuda", generator=gen).requires_grad_(True)
    loss = crossclr_amd.crossclr_loss(v, t, 0.03, 0.8, compute_mode="bf16")
    loss.backward()
    assert torch.isfinite(v.grad).all() and torch.isfinite(t.grad).all()
    with torch.no_grad():
        vh = torch.nn.functional.normalize(v.detach(), dim=1)
        th = torch.nn.functional.normalize(t.detach(), dim=1)
        tot = torch.zeros((), dtype=torch.float64, device="cuda")
        blk = 2048
        rr = torch.arange(blk, device="cuda")
        for r0 in range(0, B, blk):
            idx = torch.arange(r0, r0 + blk, device="cuda")
            for own, oth in ((vh, th), (th, vh)):
                a = (own[r0:r0 + blk] @ oth.t()).double() / 0.03
                c = (own[r0:r0 + blk] @ own.t()).double() * (0.8 / 0.03)
                c[rr, idx] = 0.0
                tot += torch.logsumexp(torch.cat([a, c], 1), 1).sum()
        ref = (tot - 2 * (vh * th).sum(1).double().sum() / 0.03) / (2 * B)
    assert abs(loss.item() - ref.item()) <= 1e-4
    # the normalise-backward leaves every gradient row orthogonal to its input row
    radial = (v.grad.double() * v.detach().double()).sum(1).abs().max().item()
    assert radial <= 1e-3 * v.grad.double().norm(dim=1).max().item() * v.detach().double().norm(dim=1).max().item()


@pytest.mark.parametrize("B,D,tau", [(512, 256, 0.03), (512, 1536, 0.03), (512, 256, 0.004)])
def test_step_is_hip_graph_capturable(B, D, tau):
    """No entry point synchronises the host or allocates device memory itself, so a whole fwd+bwd step can be
    captured into a HIP graph (torch.cuda.CUDAGraph) and replayed on new data -- also a wide plan (generic forward that saves + the
    D-slice backward in column parts) and a bf16 plan in the two-pass regime (whose forward zero-fills the statistics behind its stash)."""
    crit = crossclr_amd.CrossCLR_onlyIntraModality(tau, 0.8, compute_mode="bf16").cuda()
    v0, t0 = orc.make_inputs("randn", B, D, 1)
    v1, t1 = orc.make_inputs("randn", B, D, 2)
    sv = v0.cuda().requires_grad_(True)
    st = t0.cuda().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # warm-up off the default stream, as torch's capture rules ask
        for _ in range(2):
            sv.grad = st.grad = None
            crit(sv, st).backward()
    torch.cuda.current_stream().wait_stream(side)
    sv.grad = st.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = crit(sv, st)
        static_loss.backward()
    with torch.no_grad():
        sv.copy_(v1.cuda())
        st.copy_(t1.cuda())
    graph.replay()
    torch.cuda.synchronize()
    ev = v1.cuda().requires_grad_(True)
    et = t1.cuda().requires_grad_(True)
    eager = crit(ev, et)
    eager.backward()
    torch.cuda.synchronize()
    assert static_loss.item() == eager.item()
    assert torch.equal(sv.grad, ev.grad) and torch.equal(st.grad, et.grad)


@pytest.mark.parametrize("world,B,D,weighted", [(3, 768, 128, False), (4, 1024, 256, False), (5, 640, 512, False),
                                                (8, 2048, 512, False), (5, 1280, 256, True), (8, 2048, 512, True),
                                                (4, 1024, 1024, True), (3, 900, 700, False)])   # 4-wave forward (D > 512), ragged
def test_pair_forward_scheme_equals_single_device(world, B, D, weighted):
    """crossclr_forward_pairs: every (r, s) block of the symmetric matrix is evaluated by ONE rank, whose column sums
    become the other rank's partial row sums (crossclr_forward_add).  One GPU plays all ranks; logZ / loss / rz must
    equal what the plain scheme (every rank evaluates every block) and the single-device run give."""
    v, t = orc.make_inputs("randn", B, D, 77)
    vd, td = v.cuda(), t.cuda()
    lib, p = nat.library(), L._ptr
    b = B // world
    stream = L._stream_for(vd)
    f32 = dict(dtype=torch.float32, device="cuda")
    plans = [nat.make_plan(b, D, world, r, nat.MODE_BF16) for r in range(world)]
    pl = plans[0]
    assert pl.fast_path == 1
    n2, K = 2 * pl.bpad, (world - 1) // 2
    xall = torch.empty(world * pl.operand_bytes, dtype=torch.uint8, device="cuda")
    inv = [torch.empty(n2, **f32) for _ in range(world)]
    diag = [torch.empty(pl.bpad, **f32) for _ in range(world)]
    for r in range(world):
        nat.check(lib.crossclr_normalize(ctypes.byref(plans[r]), p(vd[r * b:]), p(td[r * b:]), vd.stride(0), td.stride(0),
                                         nat.IN_F32, p(xall[r * pl.operand_bytes:]), p(inv[r]), p(diag[r]), stream))
    parts = [torch.empty(pl.fwd_ws_floats, **f32) for _ in range(world)]
    colsums = [torch.empty(K, n2, **f32) for _ in range(world)]
    kall = None
    if weighted:   # negative scales in the statistics layout [world][2][bpad]; columns pruned / re-weighted at random
        gen = torch.Generator().manual_seed(3)
        kv, kt = (torch.rand(B, generator=gen) > 0.4).float(), 2 * torch.rand(B, generator=gen)
        kall = torch.zeros(world, 2, pl.bpad, **f32)
        for r in range(world):
            kall[r, 0, :b], kall[r, 1, :b] = kv[r * b:(r + 1) * b].cuda(), kt[r * b:(r + 1) * b].cuda()
    sw = (lambda rows, cols: L._sw(rows, cols, None)) if weighted else (lambda rows, cols: None)
    for r in range(world):
        pp = ctypes.byref(plans[r])
        xr = xall[r * pl.operand_bytes:(r + 1) * pl.operand_bytes]
        kr = kall[r] if weighted else None
        nat.check(lib.crossclr_forward_w(pp, p(xr), p(xr), 1, r, -1, 0.03, 0.8, sw(kr, kr), p(parts[r]), 0, stream))
        nat.check(lib.crossclr_forward_pairs(pp, p(xr), p(xall), (r + 1) % world, K, 0.03, 0.8, sw(kr, kall), p(parts[r]),
                                             pl.fwd_slots, p(colsums[r]), stream))
        if world % 2 == 0:
            opp = (r + world // 2) % world
            nat.check(lib.crossclr_forward_w(pp, p(xr), p(xall[opp * pl.operand_bytes:]), 1, opp, -1, 0.03, 0.8,
                                             sw(kr, kall[opp] if weighted else None), p(parts[r]), 2 * pl.fwd_slots, stream))
        else:
            nat.check(lib.crossclr_forward_add(pp, p(parts[r]), 2 * pl.fwd_slots, None, stream))
    logz_pairs, loss_pairs = [], torch.zeros(1, dtype=torch.float64, device="cuda")
    for r in range(world):
        pp = ctypes.byref(plans[r])
        received = torch.zeros(n2, **f32)
        for k in range(K):                     # rank (r-1-k) evaluated the pair and computed my sums as its colsum[k]
            received += colsums[(r - 1 - k) % world][k]
        nat.check(lib.crossclr_forward_add(pp, p(parts[r]), 3 * pl.fwd_slots, p(received), stream))
        logz, rz, wrz = (torch.empty(n2, **f32) for _ in range(3))
        ls = torch.empty(pl.loss_ws_doubles, dtype=torch.float64, device="cuda")
        nat.check(lib.crossclr_forward_finish_w(pp, p(parts[r]), 4 * pl.fwd_slots, p(diag[r]), 0.03, 0.8,
                                                sw(kall[r] if weighted else None, None), p(logz), p(rz), p(wrz), p(ls), stream))
        logz_pairs.append(logz)
        loss_pairs += ls[:1]
    torch.cuda.synchronize()
    loss_pairs = (loss_pairs / (2.0 * B)).item()
    ref = orc.streaming_stats(v, t, 0.03, 0.8)
    if not weighted:
        assert abs(loss_pairs - float(ref["loss"])) <= 1e-3
    # per-row: against the single-device run of the same bf16 kernels (same operands, different summation order only)
    _, ws1 = L._forward_impl(vd, td, 0.03, 0.8, "bf16", None, (kv.cuda(), kt.cuda()) if weighted else None, None)
    torch.cuda.synchronize()
    p1 = ws1.plan
    for r in range(world):
        lz = logz_pairs[r].cpu().double()
        assert (lz[:b] - ws1.logz[r * b:(r + 1) * b].cpu().double()).abs().max().item() <= 2e-5
        assert (lz[pl.bpad:pl.bpad + b] - ws1.logz[p1.bpad + r * b:p1.bpad + (r + 1) * b].cpu().double()).abs().max().item() <= 2e-5
        if not weighted:
            assert (lz[:b] - ref["logZv"][r * b:(r + 1) * b]).abs().max().item() <= 3e-2     # bf16 operands vs float64
    loss1 = crossclr_amd.crossclr_loss(vd, td, 0.03, 0.8, compute_mode="bf16",
                                       negative_scale=(kv.cuda(), kt.cuda()) if weighted else None).item()
    assert abs(loss_pairs - loss1) <= 2e-6 * max(1.0, abs(loss1))


# (the caller-side entry points -- prenormalized=True, the fused projection -- are checked against the reference's goldens and the
#  float64 oracle in tests/test_gpu_projection.py)


@pytest.mark.parametrize("world,B,D,weighted", [(2, 512, 128, False), (3, 768, 256, False), (4, 2048, 512, False), (5, 1280, 256, True),
                                                (8, 2048, 512, False), (2, 512, 1024, False), (3, 768, 700, True), (8, 2048, 1024, True),
                                                # BASELINE config 4 at full size: 8 ranks x 8192 rows, every rank played on this GPU
                                                (8, 65536, 512, False)])
@pytest.mark.parametrize("partner", [False, True])
def test_remote_blocks_with_saved_exponentials_equal_single_device(world, B, D, weighted, partner):
    """The sharded step with a backward to follow: pair partners' and the antipodal rank's blocks save their exponentials in the
    forward (crossclr_forward_rect_save) and feed the backward from them (crossclr_backward_rect_saved); the blocks the OTHER
    side of a pair evaluated are recomputed (crossclr_backward_ranks).  One GPU plays every rank through the C-ABI; loss and
    gradients must equal the single-device run on the concatenated batch."""
    lib, p = nat.library(), L._ptr
    b = B // world
    v, t = orc.make_inputs("randn", B, D, 71)
    vd, td = v.cuda(), t.cuda()
    g = torch.Generator().manual_seed(3)
    kv = (torch.rand(B, generator=g) > 0.2).float()
    kt = (torch.rand(B, generator=g) > 0.2).float()
    ov = 0.5 + torch.rand(B, generator=g)
    ot = 0.5 + torch.rand(B, generator=g)
    stream = L._stream_for(vd)
    f32 = dict(dtype=torch.float32, device="cuda")
    plans = [nat.make_plan(b, D, world, r, nat.MODE_BF16) for r in range(world)]
    pl = plans[0]
    assert pl.stash_bytes > 0
    n2 = 2 * pl.bpad
    xall = torch.empty(world * pl.operand_bytes, dtype=torch.uint8, device="cuda")
    inv = [torch.empty(n2, **f32) for _ in range(world)]
    diag = [torch.empty(pl.bpad, **f32) for _ in range(world)]
    kall = torch.zeros(world, 2, pl.bpad, **f32)
    lwall = torch.zeros(world, 2, pl.bpad, **f32)
    kall[:, 0, :b], kall[:, 1, :b] = kv.view(world, b).cuda(), kt.view(world, b).cuda()
    lwall[:, 0, :b], lwall[:, 1, :b] = ov.view(world, b).cuda(), ot.view(world, b).cuda()

    def sw(r, cols_all, lw):
        if not weighted:
            return None
        return ctypes.pointer(nat.SampleWeights(kall[r].data_ptr(), kall.data_ptr() if cols_all else kall[r].data_ptr(),
                                                lwall[r].data_ptr() if lw else 0))
    for r in range(world):
        xr = xall[r * pl.operand_bytes:(r + 1) * pl.operand_bytes]
        nat.check(lib.crossclr_normalize(ctypes.byref(plans[r]), p(vd[r * b:]), p(td[r * b:]), vd.stride(0), td.stride(0), nat.IN_F32,
                                         p(xr), p(inv[r]), p(diag[r]), stream))
    K = (world - 1) // 2
    parts = [torch.empty(pl.fwd_ws_floats, **f32) for _ in range(world)]
    colsums = [torch.zeros(max(K, 1), n2, **f32) for _ in range(world)]
    stashes, blocks = [], []
    for r in range(world):
        pp = ctypes.byref(plans[r])
        xr = xall[r * pl.operand_bytes:(r + 1) * pl.operand_bytes]
        st_loc = torch.empty(pl.stash_bytes, dtype=torch.uint8, device="cuda")
        nat.check(lib.crossclr_forward_save(pp, p(xr), 0.03, 0.8, sw(r, False, False), p(parts[r]), 0, p(st_loc), stream))
        saved = []
        if K:
            st = torch.empty(lib.crossclr_rect_stash_bytes(pp, K), dtype=torch.uint8, device="cuda")
            nat.check(lib.crossclr_forward_rect_save(pp, p(xr), p(xall), (r + 1) % world, K, 1, 0.03, 0.8, sw(r, True, False), p(parts[r]),
                                                     pl.fwd_slots, p(colsums[r]), p(st), stream))
            saved.append(((r + 1) % world, K, st))
        if world % 2 == 0:
            opp = (r + world // 2) % world
            st = torch.empty(lib.crossclr_rect_stash_bytes(pp, 1), dtype=torch.uint8, device="cuda")
            nat.check(lib.crossclr_forward_rect_save(pp, p(xr), p(xall), opp, 1, 0, 0.03, 0.8, sw(r, True, False), p(parts[r]),
                                                     (2 if K else 1) * pl.fwd_slots, None, p(st), stream))
            saved.append((opp, 1, st))
        elif K:
            nat.check(lib.crossclr_forward_add(pp, p(parts[r]), 2 * pl.fwd_slots, None, stream))
        stashes.append(st_loc)
        blocks.append(saved)
    rz = torch.empty(world, n2, **f32)
    wrz = torch.empty(world, n2, **f32)
    total = torch.zeros(1, dtype=torch.float64, device="cuda")
    for r in range(world):
        pp = ctypes.byref(plans[r])
        nl = 2
        if K:
            received = torch.zeros(n2, **f32)
            for k in range(K):
                received += colsums[(r - 1 - k) % world][k]
            nat.check(lib.crossclr_forward_add(pp, p(parts[r]), 3 * pl.fwd_slots, p(received), stream))
            nl = 4
        logz = torch.empty(n2, **f32)
        ls = torch.empty(pl.loss_ws_doubles, dtype=torch.float64, device="cuda")
        nat.check(lib.crossclr_forward_finish_w(pp, p(parts[r]), nl * pl.fwd_slots, p(diag[r]), 0.03, 0.8, sw(r, False, True), p(logz),
                                                p(rz[r]), p(wrz[r]), p(ls), stream))
        total += ls[:1]
    lossN = (total / (2.0 * B)).item()
    gv, gt = torch.empty_like(vd), torch.empty_like(td)
    go = torch.ones(1, dtype=torch.float64, device="cuda")
    # the same blocks through the pair kernel on fragment-major operands (crossclr_backward_rect_saved_xfp / _t_xfp): the copy is made from
    # the PACKED slices (crossclr_pack_xf_from_packed -- what a rank does with the slices it received) and every launch must reproduce
    # the LDS-staged kernel's gradient buffer BIT FOR BIT (same slices, same MFMA sequence per accumulator)
    xfall = None
    if pl.xf_bytes and world * pl.operand_bytes < (1 << 32):
        xfall = torch.empty(world * pl.operand_bytes, dtype=torch.uint8, device="cuda")
        nat.check(lib.crossclr_pack_xf_from_packed(ctypes.byref(pl), p(xall), world, p(xfall), stream))
    for r in range(world):
        pp = ctypes.byref(plans[r])
        xr = xall[r * pl.operand_bytes:(r + 1) * pl.operand_bytes]
        gbuf = torch.empty(pl.gbuf_bytes // 4, **f32)
        nat.check(lib.crossclr_backward_saved(pp, p(xr), p(stashes[r]), 0.03, 0.8, p(rz[r]), p(wrz[r]), sw(r, False, False), p(gbuf), 0, stream))
        for first, n, st in blocks[r]:
            twin = gbuf.clone() if xfall is not None else None
            nat.check(lib.crossclr_backward_rect_saved(pp, p(xall), p(st), first, n, 0.03, 0.8, p(rz[r]), p(wrz[r]), p(rz), p(wrz),
                                                       sw(r, True, False), p(gbuf), 1, stream))
            if twin is not None and (r < 2 or B <= 8192):        # (every rank at the small shapes, two ranks of the big ones)
                nat.check(lib.crossclr_backward_rect_saved_xfp(pp, p(xfall), p(st), first, n, 0.03, 0.8, p(rz[r]), p(wrz[r]), p(rz), p(wrz),
                                                               sw(r, True, False), p(twin), 1, stream))
                assert torch.equal(twin, gbuf), (r, first, n)
        if K and partner:
            # partner gradients: rank s = r-1-k evaluated block (s, r) and forms its transposed contribution to r's buffer
            # (crossclr_backward_rect_saved_t, played here by the same GPU); r adds the column slices' sum
            nel = n2 * pl.Dpad
            for k in range(K):
                src = (r - 1 - k) % world
                xs = xall[src * pl.operand_bytes:(src + 1) * pl.operand_bytes]
                first, n, st = blocks[src][0]
                tmp = torch.empty(pl.gbuf_bytes // 4, **f32)
                nat.check(lib.crossclr_backward_rect_saved_t(ctypes.byref(plans[src]), p(xs), p(st), first, n, k, 0.03, 0.8, p(rz[src]),
                                                             p(wrz[src]), p(rz), p(wrz), sw(src, True, False), p(tmp), stream))
                if xfall is not None and (r < 2 or B <= 8192):
                    tmp2 = torch.full_like(tmp, float("nan"))
                    xfs = xfall[src * pl.operand_bytes:(src + 1) * pl.operand_bytes]
                    nat.check(lib.crossclr_backward_rect_saved_t_xfp(ctypes.byref(plans[src]), p(xfs), p(st), first, n, k, 0.03, 0.8, p(rz[src]),
                                                                     p(wrz[src]), p(rz), p(wrz), sw(src, True, False), p(tmp2), stream))
                    assert torch.equal(tmp2, tmp), (r, src, k)
                gbuf[:nel] += tmp.view(-1, nel).sum(0)
        elif K:
            nat.check(lib.crossclr_backward_ranks(pp, p(xr), p(xall), (r - K) % world, K, 0.03, 0.8, p(rz[r]), p(wrz[r]), p(rz), p(wrz),
                                                  sw(r, True, False), p(gbuf), 1, stream))
        nat.check(lib.crossclr_backward_finish_w(pp, p(gbuf), p(vd[r * b:]), p(td[r * b:]), vd.stride(0), td.stride(0), nat.IN_F32,
                                                 p(inv[r]), 0.03, sw(r, False, True), p(go), p(gv[r * b:]), p(gt[r * b:]),
                                                 gv.stride(0), gt.stride(0), stream))
    torch.cuda.synchronize()
    vg, tg = vd.clone().requires_grad_(True), td.clone().requires_grad_(True)
    loss1 = crossclr_amd.crossclr_loss(vg, tg, 0.03, 0.8, compute_mode="bf16",
                                       negative_scale=(kv.cuda(), kt.cuda()) if weighted else None,
                                       loss_weight=(ov.cuda(), ot.cuda()) if weighted else None)
    loss1.backward()
    torch.cuda.synchronize()
    assert abs(lossN - loss1.item()) <= 2e-6 * max(1.0, abs(loss1.item()))
    scale = vg.grad.abs().max().item()
    assert (gv - vg.grad).abs().max().item() <= 3e-3 * scale      # bf16 weights rounded in different tile groupings
    assert (gt - tg.grad).abs().max().item() <= 3e-3 * scale


def test_second_order_terms_on_the_device():
    """create_graph=True through the criterion (the reference's eager ops, trainer/loss.py:79-114, are twice differentiable): the first
    gradient equals the HIP backward's, and a gradient penalty differentiates to the op-for-op oracle's values."""
    v, t = orc.make_inputs("randn", 64, 48, 5)
    vd, td = v.cuda().requires_grad_(True), t.cuda().requires_grad_(True)
    crit = crossclr_amd.CrossCLR_onlyIntraModality(0.05, 0.8, compute_mode="fp32").cuda()
    loss = crit(vd, td)
    gv, gt = torch.autograd.grad(loss, (vd, td), create_graph=True)
    ((gv.double() ** 2).sum() + (gt.double() ** 2).sum()).backward()
    _, gv1, gt1 = run_module(v, t, {"temperature": 0.05, "negative_weight": 0.8}, "fp32")
    assert (gv.detach() - gv1).abs().max().item() <= 1e-5 * gv1.abs().max().item()
    vc, tc = v.clone().requires_grad_(True), t.clone().requires_grad_(True)
    rv, rt = torch.autograd.grad(orc.eager_loss(vc, tc, 0.05, 0.8), (vc, tc), create_graph=True)
    ((rv.double() ** 2).sum() + (rt.double() ** 2).sum()).backward()
    assert (vd.grad.cpu() - vc.grad).abs().max().item() <= 1e-4 * vc.grad.abs().max().item()
    assert (td.grad.cpu() - tc.grad).abs().max().item() <= 1e-4 * tc.grad.abs().max().item()


@pytest.mark.parametrize("B,D", fst.SHAPES)
@pytest.mark.parametrize("row", [r for r in fst.ROWS if r.knob is None], ids=fst.row_id)
def test_fwd_sums_launches_through_the_c_abi(row, B, D):
    """The table of tests/test_kernels_emulated.py::test_fwd_sums_launches_through_the_c_abi on the hipcc build (the rows no environment
    knob is needed for: this library reads its knobs once per process): the launcher's template choice, seen as the launch's name and
    the loss it leads to."""
    fst.check_row(row, B, D, torch.device("cuda"))
