"""Every kernel family on the MI355X, per row, on operands all three compute modes hold exactly (tests/exact_inputs.py): +-1 sign rows
whose unit rows are powers of two, so every cosine is a multiple of 1 / nnz in bf16, bf16x3 and fp32 alike and the kernels' operand
rounding -- what the 1e-2 bars of tests/test_gpu_parity.py have to absorb -- does not exist.  Yardsticks are float64 only, never
another kernel: the exact closed form (oracle.stacked_weight_model(roundings=0)) for the forward statistics of every mode and for the
fp32 / bf16x3 gradients; for the bf16 gradients the weight model with the kernels' own bf16 roundings of the weights (two for the
saved backwards, one for the recomputing ones: oracle.bf16_weight_model_grads).  Gradients are compared row by row
(max_d |delta| / max_d |want_i|, exact_inputs.check_rows), the score kernels (top-k, ranks) bit for bit under their documented order.

BARS (exact_inputs.GRAD_BAR / LOGZ_BAR / LOSS_BAR) = 4 x the worst error measured below, under the ceilings 1e-4 (gradient rows) and
2e-5 (logZ, loss); the teeth test of tests/test_exact_operands_cpu.py shows that a dropped 32 x 32 tile, a column statistic from the
neighbouring column or ignored column sample weights move a row of EVERY case here by at least 10 x its bar.

MEASURED on the MI355X, unmodified kernels of commit 17a4a32, 2026-10-19 (worst over all cases of the group, video and text rows):
  gradient rows, fp32 vs float64        1.003e-06 single pass (saved = recomputing)    2.146e-05 two-pass (recomputing; saved 3.3e-07)
  gradient rows, bf16x3 vs float64      1.011e-05 single pass                          2.030e-05 two-pass (recomputing; saved 5.2e-06)
  gradient rows, bf16 vs weight model   4.146e-06 (most cases 1.3e-07 .. 5e-07; the same rows against plain float64: 1.9e-03 .. 1.0e-01)
  gradient rows, two-pass bf16          1.322e-03 against plain float64 (not modelled: bar 4 x this, as the forward keeps the common bars)
  logZ                                  5.986e-06 at tau = 0.01 (logZ ~ 100, fp32 unit 7.6e-06), 2.9e-06 at tau = 0.03: 4 x is above the
                                        ceiling, the bar IS the ceiling 2e-5;  two-pass (tau = 0.004): 7.2e-07 in the form below
  loss (relative to max(1, |loss|))     6.570e-08
  max-margin (bars of the golden test)  loss 3.0e-08, gradients 5.4e-08 of the largest entry, fp32 and bf16 alike
WHAT THE YARDSTICKS LACKED, found while measuring (no kernel was changed):
  * bf16 weights at a rounding tie.  The device's exp2 is accurate to a unit of fp32, not correctly rounded: a weight (or saved exponential)
    whose fp32 value lies within 8 units of the midpoint of two bf16 values can round the other way than in the model -- one row of
    (intra, B = 130, D = 512) was off by 3.0e-05, 4 x that is above the ceiling.  The model returns the rows' allowance for exactly those
    weights (`slack_rows`: two bf16 steps of about one weight in 4000; zero for most rows), subtracted before the bar applies.
  * the two-pass forward.  logZ ~ 1 / tau = 250 there: fp32, the type of `logz`, has a unit of 3.05e-05 (stored values were 1.7e-05 and
    3.05e-05 off the exact closed form), and the C-ABI's float temperature moves a logit of 235 by 1.1e-05 (float(0.004) = 0.004 (1 +
    4.7e-08)).  The bar is held by ln 2 * shift - log(rz) -- the statistics as the backward reads them -- against the closed form on the
    kernels' own scaled logits (oracle.stacked_weight_model(fp32_logits=...)); the stored logz must be that value within one fp32 unit.
"""
import ctypes
import math

import pytest
import torch

import crossclr_amd
import exact_inputs as xi
from crossclr_amd import _native as nat
from crossclr_amd import loss as L
from crossclr_amd import ranking as R
from oracle import crossclr_oracle as orc
from oracle import ranking_oracle as rk

pytestmark = pytest.mark.gpu
TAU, W, MODES = xi.TAU, xi.W, xi.MODES
LDS, WIDE = xi.LDS, xi.WIDE


@pytest.fixture(autouse=True)
def _hip_only():
    nat.use_library_for_testing(None)
    assert nat.backend() == "hip-gfx950", "GPU tests must run the HIP library"
    yield


_inputs = {}


def inputs(kind, B, D):
    """(video, text) on the CPU, generated (and checked for exactness) once per case"""
    key = (kind, B, D)
    if key not in _inputs:
        _inputs[key] = xi.planted(kind, B, D, seed=B + D)
    return _inputs[key]


_models = {}


def model(kind, B, D, tau, w, weighted, rounds):
    key = (kind, B, D, tau, w, weighted, rounds)
    if key not in _models:
        v, t = inputs(kind, B, D)
        k, om = xi.sample_weights(B, B + D) if weighted else (None, None)
        m = orc.stacked_weight_model(v, t, tau, w, k, om, roundings=rounds)
        m["grads"] = orc.grads_from_stacked_weights(m)
        _models[key] = m
    return _models[key]


def last_kernels():
    lib = nat.library()
    return lib.crossclr_last_kernel(0).decode(), lib.crossclr_last_kernel(1).decode()


def check_forward(ws, loss, m, B, what, m32=None):
    """logZ per row, the positive pair's logit and the loss against float64.  Two-pass regime (m32: the closed form on the kernels' fp32 logits):
    logZ is ~ 1 / tau = 250 there, where fp32 -- the type of `logz` -- has a unit in the last place of 3.05e-5, above the bar, and where a logit's
    own fp32 rounding is 1.5e-5: the exact closed form lacks both.  The bar is held there by the row statistics in the form the backward
    reads them, which fp32 does hold: ln 2 * shift - log(rz) against m32; the stored logz must be that value within one fp32 unit."""
    bp = ws.plan.bpad
    rows = torch.cat([torch.arange(B), bp + torch.arange(B)])
    logz = ws.logz.cpu().double()[rows]
    tau = float(m["tau"])
    want = torch.cat([m["logZv"], m["logZt"]])
    if m32 is not None:
        want = torch.cat([m32["logZv"], m32["logZt"]])
        stored = logz
        logz = ws.shift.cpu().double()[rows] * math.log(2.0) - torch.log(ws.rz.cpu().double()[rows])
        ulp = torch.exp2(torch.floor(torch.log2(want.abs())) - 23)
        assert ((stored - logz).abs() <= ulp).all(), what
        print(f"        two-pass: stored logz within {((stored - logz).abs() / ulp).max().item():.2f} fp32 units of ln 2 * shift - log(rz); "
              f"against the exact closed form {(stored - torch.cat([m['logZv'], m['logZt']])).abs().max().item():.3e}")
    e_lz = (logz - want).abs().max().item()
    e_diag = (ws.diag.cpu().double()[:B] / tau - m["diag"]).abs().max().item()
    e_loss = abs(float(loss) - float(m["loss"])) / max(1.0, abs(float(m["loss"])))
    print(f"MEASURE forward {what}: logZ {e_lz:.3e} diag {e_diag:.3e} loss {e_loss:.3e}")
    assert e_lz <= (xi.LOGZ_BAR if m32 is None else xi.LOGZ_BAR_TWO_PASS) and e_diag <= xi.LOGZ_BAR and e_loss <= xi.LOSS_BAR, what
    assert (ws.rz.cpu()[B:bp] == 0).all() and (ws.rz.cpu()[bp + B:] == 0).all(), "padding rows must carry zero weight"


# ------------------------------------------------------------------------------------------------------------------------------
# forward: per-row logZ, the positive pair's logit, the loss -- every forward family at its smallest shape
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B,D,tau,w,kernel", xi.FORWARD)
def test_forward_statistics_per_row(mode, B, D, tau, w, kernel):
    v, t = inputs("mixed", B, D)
    m = model("mixed", B, D, tau, w, False, 0)
    vd, td = v.cuda(), t.cuda()
    for save in (True, False):
        # (two-pass regime: the saving pass subtracts the row shift inside the scaling's fused multiply-add, the plain pass rounds the scaled logit first)
        m32 = orc.stacked_weight_model(v, t, tau, w, fp32_logits="scale" if save else "product") if orc.needs_row_shift(tau, w) else None
        loss, ws = L._forward_impl(vd, td, tau, w, mode, None, save_for_backward=save)
        torch.cuda.synchronize()
        k0 = last_kernels()[0]
        print(f"forward {mode} B={B} D={D} tau={tau} save={save}: {k0}")
        assert k0.startswith(kernel if save else kernel.split(" (")[0]) and ("x3_t" in k0) == (mode == "bf16x3"), k0
        check_forward(ws, loss, m, B, f"{mode} B={B} D={D} tau={tau} save={save}", m32)


# ------------------------------------------------------------------------------------------------------------------------------
# backward through the module
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("mode,kind,B,D,tau,w,recompute,kernel", xi.BACKWARD)
def test_backward_per_row(mode, kind, B, D, tau, w, recompute, kernel, weighted, monkeypatch):
    if recompute:
        # (CROSSCLR_DISABLE_SAVE is read once per process by the HIP build; crossclr_step_plan reads CROSSCLR_MAX_STASH_GB per call: with 0
        #  nothing is saved and the backward recomputes -- the kernel name and `_last_step_saved` below say that it did)
        monkeypatch.setenv("CROSSCLR_MAX_STASH_GB", "0")
    v, t = inputs(kind, B, D)
    k, om = xi.sample_weights(B, B + D) if weighted else (None, None)
    loss, gv, gt = xi.run_loss(v.cuda(), t.cuda(), tau, w, mode, k, om)
    torch.cuda.synchronize()
    k0, k1 = last_kernels()
    assert k1.startswith(kernel) and ("x3_t" in k1 or "_x3_" in k1) == (mode == "bf16x3"), (k0, k1)
    assert L._last_step_saved == (not recompute)
    exact = model(kind, B, D, tau, w, weighted, 0)
    want = model(kind, B, D, tau, w, weighted, 0 if mode != "bf16" else (1 if recompute else 2))
    e_loss = abs(loss - float(exact["loss"])) / max(1.0, abs(float(exact["loss"])))
    ev, et = xi.check_rows(gv, want["grads"][0], slack=want["slack_rows"][:B]), xi.check_rows(gt, want["grads"][1], slack=want["slack_rows"][B:])
    group = "bf16 vs weight model" if mode == "bf16" else f"{mode} vs float64"
    print(f"MEASURE backward [{group}] {kind} B={B} D={D} tau={tau} weighted={weighted} {k1}: video {ev[0]:.3e} @ row {ev[1]}  text {et[0]:.3e} @ row {et[1]}  loss {e_loss:.3e}")
    if mode == "bf16":
        f64 = xi.check_rows(gv, exact["grads"][0])[0]
        print(f"        (the same rows against plain float64: {f64:.3e})")
    assert e_loss <= xi.LOSS_BAR
    assert max(ev[0], et[0]) <= xi.GRAD_BAR[mode, orc.needs_row_shift(tau, w), not recompute], (ev, et)
    if mode == "bf16":
        assert xi.slack_fraction(want, xi.GRAD_BAR[mode, False, not recompute]) <= xi.SLACK_ROWS_MAX


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_two_pass_bf16_backward_against_the_weight_model(weighted):
    """The saved bf16 backward of the two-pass regime (crossclr_backward_saved_s: bf16 records U[p][q] = exp2(x - shift_p) with per-row
    shifts, a direct and a transposed launch, each rounding its own weight) against the weight model of that scheme."""
    B, D, tau, w = xi.TWO_PASS_BF16
    v, t = inputs("mixed", B, D)
    k, om = xi.sample_weights(B, B + D) if weighted else (None, None)
    loss, gv, gt = xi.run_loss(v.cuda(), t.cuda(), tau, w, "bf16", k, om)
    assert last_kernels() == ("fwd_sums_kernel (save, bf16 records)", LDS) and L._last_step_saved
    exact = model("mixed", B, D, tau, w, weighted, 0)
    want = model("mixed", B, D, tau, w, weighted, 2)
    ev, et = xi.check_rows(gv, want["grads"][0], slack=want["slack_rows"][:B]), xi.check_rows(gt, want["grads"][1], slack=want["slack_rows"][B:])
    print(f"MEASURE backward [bf16 two-pass vs weight model] weighted={weighted}: video {ev[0]:.3e} @ {ev[1]} text {et[0]:.3e} @ {et[1]}"
          f"  (against plain float64: {xi.check_rows(gv, exact['grads'][0])[0]:.3e})")
    assert abs(loss - float(exact["loss"])) <= xi.LOSS_BAR * max(1.0, abs(float(exact["loss"])))
    assert max(ev[0], et[0]) <= xi.GRAD_BAR["bf16", True, True]


# ------------------------------------------------------------------------------------------------------------------------------
# backward through the C-ABI entry points: the LDS-staged, the fragment-major and the pair kernel, each against the weight model
# ------------------------------------------------------------------------------------------------------------------------------
CABI_KERNEL = {"crossclr_backward_saved": LDS, "crossclr_backward_saved_xf": "fast_bwd_dsl_kernel (fragment-major, one tile)",
               "crossclr_backward_saved_xfp": "fast_bwd_xfp_kernel"}


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("B,D", xi.CABI_SHAPES)
def test_saved_backward_entry_points_against_the_weight_model(B, D, weighted):
    v, t = inputs("mixed", B, D)
    k, om = xi.sample_weights(B, B + D) if weighted else (None, None)
    want = model("mixed", B, D, TAU, W, weighted, 2)
    exact = model("mixed", B, D, TAU, W, weighted, 0)
    vd, td = v.cuda(), t.cuda()
    for entry, kernel in CABI_KERNEL.items():
        loss, gv, gt = xi.saved_backward_via_cabi(vd, td, TAU, W, k, om, entry)
        assert last_kernels()[1] == kernel
        ev, et = xi.check_rows(gv, want["grads"][0], slack=want["slack_rows"][:B]), xi.check_rows(gt, want["grads"][1], slack=want["slack_rows"][B:])
        print(f"MEASURE backward [bf16 vs weight model] C-ABI {entry} B={B} D={D} weighted={weighted}: video {ev[0]:.3e} @ {ev[1]} text {et[0]:.3e} @ {et[1]}")
        assert abs(loss - float(exact["loss"])) <= xi.LOSS_BAR * max(1.0, abs(float(exact["loss"])))
        assert max(ev[0], et[0]) <= xi.GRAD_BAR["bf16", False, True], (entry, ev, et)


def _shard_via_cabi(v, t, world, mode, tau, w):
    """(after tests/test_gpu_parity.py::_shard_via_cabi, saved form) one GPU plays `world` ranks through the C-ABI: every rank normalises its
    rows into its slice of the gathered operand, its local block and the rectangular block against the other ranks save their exponentials,
    and the backward is the gradient product of the two stashes alone."""
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
    rz, wrz = torch.empty(world, 2 * pl.bpad, **f32), torch.empty(world, 2 * pl.bpad, **f32)
    logz = torch.empty(world, 2 * pl.bpad, **f32)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    stashes = []
    for r in range(world):
        pp = ctypes.byref(plans[r])
        part = torch.empty(pl.fwd_ws_floats, **f32)
        stashes.append((torch.empty(pl.stash_bytes, dtype=torch.uint8, device=dev),
                        torch.empty(lib.crossclr_rect_stash_bytes(pp, world - 1), dtype=torch.uint8, device=dev)))
        assert stashes[-1][0].numel() > 0 and stashes[-1][1].numel() > 0
        nat.check(lib.crossclr_forward_save(pp, p(xs[r]), tau, w, None, p(part), 0, p(stashes[-1][0]), stream))
        nat.check(lib.crossclr_forward_rect_save(pp, p(xs[r]), p(xall), (r + 1) % world, world - 1, 0, tau, w, None, p(part), pl.fwd_slots,
                                                 None, p(stashes[-1][1]), stream))
        ls = torch.empty(pl.loss_ws_doubles, dtype=torch.float64, device=dev)
        nat.check(lib.crossclr_forward_finish(pp, p(part), 2 * pl.fwd_slots, p(diag[r]), tau, w, p(logz[r]), p(rz[r]), p(wrz[r]), p(ls), stream))
        total += ls[:1]
    gv, gt = torch.empty_like(v), torch.empty_like(t)
    go = torch.ones(1, dtype=torch.float64, device=dev)
    kernels = set()
    for r in range(world):
        pp = ctypes.byref(plans[r])
        gbuf = torch.empty(pl.gbuf_bytes // 4, **f32)
        nat.check(lib.crossclr_backward_saved(pp, p(xs[r]), p(stashes[r][0]), tau, w, p(rz[r]), p(wrz[r]), None, p(gbuf), 0, stream))
        kernels.add(last_kernels()[1])
        nat.check(lib.crossclr_backward_rect_saved(pp, p(xall), p(stashes[r][1]), (r + 1) % world, world - 1, tau, w, p(rz[r]), p(wrz[r]),
                                                   p(rz), p(wrz), None, p(gbuf), 1, stream))
        kernels.add(last_kernels()[1])
        nat.check(lib.crossclr_backward_finish(pp, p(gbuf), p(v[r * b:]), p(t[r * b:]), v.stride(0), t.stride(0), nat.IN_F32, p(inv[r]), tau, p(go),
                                               p(gv[r * b:]), p(gt[r * b:]), gv.stride(0), gt.stride(0), stream))
    torch.cuda.synchronize()
    return (total / (2.0 * B)).item(), gv, gt, logz, pl.bpad, kernels


@pytest.mark.parametrize("mode,D", xi.THREE_RANKS)
def test_three_ranks_through_rectangular_saved_blocks(mode, D):
    """world = 3 on one GPU (100 ragged rows per rank): the local block and the rectangular block against the two other ranks, both from saved
    exponentials, against the single-batch yardstick -- the bf16 rectangular saved backward (fast_bwd_dsl_kernel in column parts, MODE 1) per
    row against the weight model, bwd_saved32_kernel<RECT> against float64."""
    world, B = 3, 300
    v, t = inputs("mixed", B, D)
    loss, gv, gt, logz, bpad, kernels = _shard_via_cabi(v.cuda(), t.cuda(), world, nat.MODE_BF16 if mode == "bf16" else nat.MODE_FP32, TAU, W)
    assert kernels == ({WIDE} if mode == "bf16" else {"bwd_saved32_kernel", "bwd_saved32_kernel (rect)"}), kernels
    exact = model("mixed", B, D, TAU, W, False, 0)
    want = model("mixed", B, D, TAU, W, False, 2 if mode == "bf16" else 0)
    b = B // world
    lz = logz.cpu().double()
    e_lz = max((torch.cat([lz[r, :b] for r in range(world)]) - exact["logZv"]).abs().max().item(),
               (torch.cat([lz[r, bpad:bpad + b] for r in range(world)]) - exact["logZt"]).abs().max().item())
    ev, et = xi.check_rows(gv, want["grads"][0], slack=want["slack_rows"][:B]), xi.check_rows(gt, want["grads"][1], slack=want["slack_rows"][B:])
    print(f"MEASURE backward [{'bf16 vs weight model' if mode == 'bf16' else 'fp32 vs float64'}] world=3 rect: video {ev[0]:.3e} @ {ev[1]} "
          f"text {et[0]:.3e} @ {et[1]}  logZ {e_lz:.3e}")
    assert e_lz <= xi.LOGZ_BAR and abs(loss - float(exact["loss"])) <= xi.LOSS_BAR * max(1.0, abs(float(exact["loss"])))
    assert max(ev[0], et[0]) <= xi.GRAD_BAR[mode, False, True]


def _pair_scheme_via_cabi(v, t, world, tau, w, k, om, xfp):
    """(after tests/test_gpu_parity.py::test_remote_blocks_with_saved_exponentials_equal_single_device, partner gradients) one GPU plays
    `world` = 3 ranks of the bf16 pair scheme through the C-ABI: rank r evaluates and saves its local block and the block against rank
    r + 1 (crossclr_forward_rect_save, whose column sums travel to r + 1); its backward is the local saved block, the rectangular block
    (crossclr_backward_rect_saved) and the TRANSPOSE of the block rank r - 1 saved (crossclr_backward_rect_saved_t, formed by r - 1).
    xfp: the rectangular and the transposed block through the pair kernel on fragment-major operands (_xfp / _t_xfp)."""
    lib, p = nat.library(), L._ptr
    B, D = v.shape
    b, dev, stream = B // world, v.device, L._stream_for(v)
    f32 = dict(dtype=torch.float32, device=dev)
    plans = [nat.make_plan(b, D, world, r, nat.MODE_BF16) for r in range(world)]
    pl = plans[0]
    assert pl.stash_bytes > 0 and (world - 1) // 2 == 1
    n2 = 2 * pl.bpad
    xall = torch.empty(world * pl.operand_bytes, dtype=torch.uint8, device=dev)
    xs = [xall[r * pl.operand_bytes:(r + 1) * pl.operand_bytes] for r in range(world)]
    inv = [torch.empty(n2, **f32) for _ in range(world)]
    diag = [torch.empty(pl.bpad, **f32) for _ in range(world)]
    weighted = k is not None
    kall, lwall = torch.zeros(world, 2, pl.bpad, **f32), torch.zeros(world, 2, pl.bpad, **f32)
    if weighted:
        kall[:, 0, :b], kall[:, 1, :b] = k[0].view(world, b).to(dev), k[1].view(world, b).to(dev)
        lwall[:, 0, :b], lwall[:, 1, :b] = om[0].view(world, b).to(dev), om[1].view(world, b).to(dev)

    def sw(r, cols_all, lw):
        if not weighted:
            return None
        return ctypes.pointer(nat.SampleWeights(kall[r].data_ptr(), kall.data_ptr() if cols_all else kall[r].data_ptr(), lwall[r].data_ptr() if lw else 0))
    for r in range(world):
        nat.check(lib.crossclr_normalize(ctypes.byref(plans[r]), p(v[r * b:]), p(t[r * b:]), v.stride(0), t.stride(0), nat.IN_F32, p(xs[r]),
                                         p(inv[r]), p(diag[r]), stream))
    parts = [torch.empty(pl.fwd_ws_floats, **f32) for _ in range(world)]
    colsums = [torch.zeros(1, n2, **f32) for _ in range(world)]
    local, rect = [], []
    for r in range(world):
        pp = ctypes.byref(plans[r])
        local.append(torch.empty(pl.stash_bytes, dtype=torch.uint8, device=dev))
        nat.check(lib.crossclr_forward_save(pp, p(xs[r]), tau, w, sw(r, False, False), p(parts[r]), 0, p(local[r]), stream))
        rect.append(torch.empty(lib.crossclr_rect_stash_bytes(pp, 1), dtype=torch.uint8, device=dev))
        nat.check(lib.crossclr_forward_rect_save(pp, p(xs[r]), p(xall), (r + 1) % world, 1, 1, tau, w, sw(r, True, False), p(parts[r]), pl.fwd_slots,
                                                 p(colsums[r]), p(rect[r]), stream))
        nat.check(lib.crossclr_forward_add(pp, p(parts[r]), 2 * pl.fwd_slots, None, stream))
    rz, wrz, logz = torch.empty(world, n2, **f32), torch.empty(world, n2, **f32), torch.empty(world, n2, **f32)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    for r in range(world):
        pp = ctypes.byref(plans[r])
        nat.check(lib.crossclr_forward_add(pp, p(parts[r]), 3 * pl.fwd_slots, p(colsums[(r - 1) % world][0]), stream))
        ls = torch.empty(pl.loss_ws_doubles, dtype=torch.float64, device=dev)
        nat.check(lib.crossclr_forward_finish_w(pp, p(parts[r]), 4 * pl.fwd_slots, p(diag[r]), tau, w, sw(r, False, True), p(logz[r]), p(rz[r]), p(wrz[r]),
                                                p(ls), stream))
        total += ls[:1]
    xfall = None
    if xfp:
        assert pl.xf_bytes and world * pl.operand_bytes < (1 << 32)
        xfall = torch.empty(world * pl.operand_bytes, dtype=torch.uint8, device=dev)
        nat.check(lib.crossclr_pack_xf_from_packed(ctypes.byref(pl), p(xall), world, p(xfall), stream))
    gv, gt = torch.empty_like(v), torch.empty_like(t)
    go = torch.ones(1, dtype=torch.float64, device=dev)
    kernels = []
    nel = n2 * pl.Dpad
    for r in range(world):
        pp = ctypes.byref(plans[r])
        gbuf = torch.empty(pl.gbuf_bytes // 4, **f32)
        nat.check(lib.crossclr_backward_saved(pp, p(xs[r]), p(local[r]), tau, w, p(rz[r]), p(wrz[r]), sw(r, False, False), p(gbuf), 0, stream))
        kernels.append(last_kernels()[1])
        first = (r + 1) % world
        if xfp:
            nat.check(lib.crossclr_backward_rect_saved_xfp(pp, p(xfall), p(rect[r]), first, 1, tau, w, p(rz[r]), p(wrz[r]), p(rz), p(wrz), sw(r, True, False),
                                                           p(gbuf), 1, stream))
        else:
            nat.check(lib.crossclr_backward_rect_saved(pp, p(xall), p(rect[r]), first, 1, tau, w, p(rz[r]), p(wrz[r]), p(rz), p(wrz), sw(r, True, False),
                                                       p(gbuf), 1, stream))
        kernels.append(last_kernels()[1])
        # the partner's gradient: rank src = r - 1 evaluated block (src, r) and forms its transposed contribution to r's buffer
        src = (r - 1) % world
        tmp = torch.full((pl.gbuf_bytes // 4,), float("nan"), **f32)
        if xfp:
            xfs = xfall[src * pl.operand_bytes:(src + 1) * pl.operand_bytes]
            nat.check(lib.crossclr_backward_rect_saved_t_xfp(ctypes.byref(plans[src]), p(xfs), p(rect[src]), r, 1, 0, tau, w, p(rz[src]), p(wrz[src]), p(rz), p(wrz),
                                                             sw(src, True, False), p(tmp), stream))
        else:
            nat.check(lib.crossclr_backward_rect_saved_t(ctypes.byref(plans[src]), p(xs[src]), p(rect[src]), r, 1, 0, tau, w, p(rz[src]), p(wrz[src]), p(rz), p(wrz),
                                                         sw(src, True, False), p(tmp), stream))
        kernels.append(last_kernels()[1])
        gbuf[:nel] += tmp.view(-1, nel).sum(0)
        nat.check(lib.crossclr_backward_finish_w(pp, p(gbuf), p(v[r * b:]), p(t[r * b:]), v.stride(0), t.stride(0), nat.IN_F32, p(inv[r]), tau,
                                                 sw(r, False, True), p(go), p(gv[r * b:]), p(gt[r * b:]), gv.stride(0), gt.stride(0), stream))
    torch.cuda.synchronize()
    return (total / (2.0 * B)).item(), gv, gt, logz, pl.bpad, kernels


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("xfp", [False, True], ids=["lds-staged", "pair-kernel"])
def test_three_ranks_through_rectangular_and_transposed_saved_blocks(xfp, weighted):
    """The bf16 pair scheme at world = 3: every rank's gradient is its local block, the rectangular block it saved (fast_bwd_dsl_kernel MODE 1
    / fast_bwd_xfp_kernel) and the TRANSPOSE of the block its predecessor saved (MODE 2) -- per row against the weight model of the
    whole batch, logZ and the loss against float64: these kernels were tied to other kernels only."""
    world, B, D = xi.PAIR_SCHEME
    v, t = inputs("mixed", B, D)
    k, om = xi.sample_weights(B, B + D) if weighted else (None, None)
    loss, gv, gt, logz, bpad, kernels = _pair_scheme_via_cabi(v.cuda(), t.cuda(), world, TAU, W, k, om, xfp)
    other = "fast_bwd_xfp_kernel" if xfp else LDS
    assert kernels == [LDS, other, other] * world, kernels
    exact = model("mixed", B, D, TAU, W, weighted, 0)
    want = model("mixed", B, D, TAU, W, weighted, 2)
    b = B // world
    lz = logz.cpu().double()
    e_lz = max((torch.cat([lz[r, :b] for r in range(world)]) - exact["logZv"]).abs().max().item(),
               (torch.cat([lz[r, bpad:bpad + b] for r in range(world)]) - exact["logZt"]).abs().max().item())
    ev, et = xi.check_rows(gv, want["grads"][0], slack=want["slack_rows"][:B]), xi.check_rows(gt, want["grads"][1], slack=want["slack_rows"][B:])
    print(f"MEASURE backward [bf16 vs weight model] world=3 pair scheme xfp={xfp} weighted={weighted}: video {ev[0]:.3e} @ {ev[1]} text {et[0]:.3e} @ {et[1]}  logZ {e_lz:.3e}")
    assert e_lz <= xi.LOGZ_BAR and abs(loss - float(exact["loss"])) <= xi.LOSS_BAR * max(1.0, abs(float(exact["loss"])))
    assert max(ev[0], et[0]) <= xi.GRAD_BAR["bf16", False, True]


# ------------------------------------------------------------------------------------------------------------------------------
# input dtypes: +-1 is exact in all of them; the gradient is the model's, rounded to the output dtype
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,mode", xi.DTYPES)
def test_input_dtypes(dtype, mode):
    dtype = getattr(torch, dtype)
    B, D = 200, 192
    v, t = inputs("mixed", B, D)
    loss, gv, gt = xi.run_loss(v.to(dtype).cuda(), t.to(dtype).cuda(), TAU, W, mode)
    assert gv.dtype == dtype and gt.dtype == dtype
    assert last_kernels()[1].startswith({"bf16": LDS, "fp32": "bwd_saved32_kernel", "bf16x3": "bwd_saved_x3_kernel"}[mode])
    exact = model("mixed", B, D, TAU, W, False, 0)
    want = model("mixed", B, D, TAU, W, False, 2 if mode == "bf16" else 0)
    assert abs(loss - float(exact["loss"])) <= xi.LOSS_BAR * max(1.0, abs(float(exact["loss"])))
    for got, w64, slack in ((gv, want["grads"][0], want["slack_rows"][:B]), (gt, want["grads"][1], want["slack_rows"][B:])):
        got = got.cpu().double()
        # a correct rounding to the output dtype of a value within the mode's bar of the model: half a unit in the last place of the
        # dtype on top of the bar (fp16: 10 mantissa bits, subnormal below 2^-14; bf16: 7)
        if dtype == torch.float64:
            half_ulp = torch.zeros_like(w64)
        else:
            bits, emin = (10, -14) if dtype == torch.float16 else (7, -126)
            expo = torch.floor(torch.log2(torch.maximum(w64.abs(), got.abs()).clamp_min(2.0 ** emin))).clamp_min(emin)
            half_ulp = 0.5 * torch.exp2(expo - bits)
        room = xi.GRAD_BAR[mode, False, True] * w64.abs().amax(1, keepdim=True) + slack[:, None] + half_ulp
        excess = ((got - w64).abs() / room).max().item()
        print(f"MEASURE dtype {dtype} {mode}: worst |delta| / (bar x row max + half ulp) = {excess:.3f}; vs the rounded model "
              f"{xi.check_rows(got, w64.to(dtype).double())[0]:.3e}")
        assert excess <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# score kernels: every score is a multiple of 1 / nnz and the same bits in every mode -- exact comparisons
# ------------------------------------------------------------------------------------------------------------------------------
_topk_ref = {}


def topk_reference(nq, ng, D):
    """queries, gallery and the float64 definition under the documented total order: score descending, index ascending"""
    key = (nq, ng, D)
    if key not in _topk_ref:
        g = torch.Generator().manual_seed(nq + ng + D)
        q, gal = xi._sign_rows(nq, D, xi.default_nnz(D), g), xi._sign_rows(ng, D, xi.default_nnz(D), g)
        for i in range(0, min(nq, ng), 3):      # planted duplicates and near-duplicates: ties at the top as well
            gal[(7 * i + 5) % ng] = q[i % nq]
            gal[(11 * i + 3) % ng] = xi._near_duplicate(q[i % nq], 2, g)
        xi.assert_exact(q, gal)
        S = torch.nn.functional.normalize(q.double(), dim=1) @ torch.nn.functional.normalize(gal.double(), dim=1).t()
        order = torch.sort(S, dim=1, descending=True, stable=True).indices
        _topk_ref[key] = (q, gal, S, order)
    return _topk_ref[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nq,ng,D", [(130, 4099, 72), (300, 3000, 200), (1, 128, 64), (37, 100, 64)])
def test_topk_exact_under_the_total_order(nq, ng, D, mode):
    q, gal, S, order = topk_reference(nq, ng, D)
    qd, gd = q.cuda(), gal.cuda()
    ties = 0
    for k in (1, 8, 9, 16, 17, 64):
        idx = order[:, :k]
        want = S.gather(1, idx)
        if k < ng:
            ties += int((S.gather(1, order[:, k:k + 1]) == want[:, -1:]).sum())      # the k-th and the (k+1)-th best score alike
        for splits in (0, 1, 3):
            scores, indices = R._topk(qd, gd, k, True, mode, splits)
            assert torch.equal(indices.cpu(), idx), (k, splits)
            assert torch.equal(scores.cpu(), want.float()), (k, splits)
    assert nq < 30 or ties > 0, "the cases are meant to have ties at the k-th place"


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("B,D,normalize", [(1000, 300, False), (384, 192, True)])
def test_retrieval_ranks_equal_the_dense_count(B, D, normalize, mode):
    v, t = inputs("inter", B, D)
    got = crossclr_amd.retrieval_ranks(v.cuda(), t.cuda(), normalize=normalize, compute_mode=mode)
    ref = rk.retrieval_ranks_dense(v, t, normalize=normalize)
    S, d = ref["scores"], ref["scores"].diag()
    assert int((S == d[:, None]).sum()) > B, "ties with the partner's score are the point"
    assert torch.equal(got["v2t_ranks"].cpu(), ref["v2t_ranks"]) and torch.equal(got["t2v_ranks"].cpu(), ref["t2v_ranks"])


@pytest.mark.parametrize("save", [True, False], ids=["saved-mask", "recomputing"])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("B,D", [(300, 200), (130, 1100)])
def test_max_margin_on_exact_scores(B, D, mode, save, monkeypatch):
    """0.1 is no multiple of 1 / nnz: no hinge argument margin + S - d sits at its kink (asserted in float64), so the bf16 mode gets
    the fp32 mode's bars of tests/test_gpu_ranking.py (2e-6) on the loss and on both gradients, with no row allowance."""
    if not save:
        monkeypatch.setenv("CROSSCLR_MAXMARGIN_SAVE", "0")
    v, t = inputs("inter", B, D)
    im, s = torch.nn.functional.normalize(v, dim=1), torch.nn.functional.normalize(t, dim=1)
    S = im.double() @ s.double().t()
    d = S.diag()
    off = ~torch.eye(B, dtype=torch.bool)
    assert min((0.1 + S - d[:, None]).abs()[off].min().item(), (0.1 + S - d[None, :]).abs()[off].min().item()) > 1e-3
    st = rk.max_margin_streaming(im, s, 0.1)
    a, b = im.cuda().requires_grad_(True), s.cuda().requires_grad_(True)
    loss = crossclr_amd.max_margin_loss(a, b, 0.1, compute_mode=mode)
    assert (loss.grad_fn.sc.mask is not None) == save
    loss.backward()
    e_loss = abs(loss.item() - float(st["loss"])) / max(1.0, abs(float(st["loss"])))
    scale = max(float(st["grad_im"].abs().max()), float(st["grad_s"].abs().max()))
    e_im = (a.grad.double().cpu() - st["grad_im"]).abs().max().item() / scale
    e_s = (b.grad.double().cpu() - st["grad_s"]).abs().max().item() / scale
    print(f"MEASURE max-margin {mode} B={B} D={D} save={save}: loss {e_loss:.3e} grad_im {e_im:.3e} grad_s {e_s:.3e}")
    assert e_loss <= 2e-6 and e_im <= 2e-6 and e_s <= 2e-6
