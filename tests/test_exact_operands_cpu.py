"""CPU side of the exact-operand tests (tests/exact_inputs.py; the MI355X side is tests/test_gpu_exact_operands.py):
* the generators are exact (unit rows are bf16 values, float32 Gram matrix = float64 Gram matrix) and planted pairs spread logZ over units;
* the dense weight model of the oracle is the streaming closed form when nothing is rounded, with and without sample weights;
* the emulated kernels meet the GPU file's assertions on small shapes: three modes, saved and recomputing, plain / planted / weighted
  inputs, the kernel family that was meant (crossclr_last_kernel), per row, at the GPU file's bars;
* TEETH (float64 only, no kernel): at every case of the GPU file, a dropped 32 x 32 tile of weights (first, last ragged, across the
  video / text boundary, mirrored), column statistics from the neighbouring column and ignored column sample weights each move some
  row by at least 10 x the bar that case is held to -- a case that could not show a defect would not be in the GPU file."""
import pytest
import torch

import exact_inputs as xi
from crossclr_amd import _native as nat
from crossclr_amd import loss as L
from oracle import crossclr_oracle as orc
from oracle import influence_oracle as inf

TAU, W = xi.TAU, xi.W


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    from emu import build_emu
    nat.use_library_for_testing(build_emu.build())
    yield
    nat.use_library_for_testing(None)


@pytest.mark.parametrize("kind", ["plain", "inter", "intra", "mixed"])
@pytest.mark.parametrize("B,D,nnz", [(200, 64, 64), (130, 192, 64), (77, 40, 16), (50, 1100, 256), (33, 20, 4)])
def test_generators_are_exact_and_planted_pairs_spread_logz(kind, B, D, nnz):
    v, t = xi.planted(kind, B, D, nnz, seed=3)        # (asserts the exactness condition itself)
    for x in (v, t):
        assert torch.equal(x.abs().sum(1), torch.full((B,), float(nnz))) and set(x.unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert torch.equal(x.half().float(), x) and torch.equal(x.bfloat16().float(), x)
    S = (torch.nn.functional.normalize(v, dim=1) @ torch.nn.functional.normalize(t, dim=1).t()) * nnz
    assert torch.equal(S, S.round()), "every cosine is a multiple of 1 / nnz"
    if kind != "plain" and nnz >= 16:
        st = orc.streaming_stats(v, t, TAU, W)
        assert float(st["logZv"].max() - st["logZv"].min()) > 4.0 and float(st["logZt"].max() - st["logZt"].min()) > 4.0


@pytest.mark.parametrize("tau,w", [(0.03, 0.8), (0.01, 1.0), (0.004, 1.0)])
def test_unrounded_weight_model_is_the_streaming_closed_form(tau, w):
    v, t = xi.planted("mixed", 130, 192, seed=5)
    m = orc.stacked_weight_model(v, t, tau, w)
    gv, gt = orc.grads_from_stacked_weights(m)
    ref = orc.streaming_loss_and_grads(v, t, tau, w)
    assert abs(float(m["loss"] - ref["loss"])) <= 1e-12 * abs(float(ref["loss"]))
    assert (m["logZv"] - ref["logZv"]).abs().max() <= 1e-11 and (m["logZt"] - ref["logZt"]).abs().max() <= 1e-11
    assert xi.check_rows(gv, ref["grad_v"])[0] <= 1e-11 and xi.check_rows(gt, ref["grad_t"])[0] <= 1e-11
    k, om = xi.sample_weights(130, 2)
    m = orc.stacked_weight_model(v, t, tau, w, k, om)
    gv, gt = orc.grads_from_stacked_weights(m)
    ref = inf.streaming_weighted_loss_and_grads(v, t, tau, w, k[0], k[1], om[0], om[1])
    assert abs(float(m["loss"] - ref["loss"])) <= 1e-12 * abs(float(ref["loss"]))
    assert xi.check_rows(gv, ref["grad_v"])[0] <= 1e-11 and xi.check_rows(gt, ref["grad_t"])[0] <= 1e-11


def test_rounded_weight_models_differ_from_float64_by_the_bf16_roundings():
    """two roundings, one rounding and none are three different yardsticks: 1e-3 apart per row, a thousand bars"""
    v, t = xi.planted("mixed", 130, 192, seed=5)
    g0 = orc.grads_from_stacked_weights(orc.stacked_weight_model(v, t, TAU, W))[0]
    g1 = orc.bf16_weight_model_grads(v, t, TAU, W, saved=False)["grad_v"]
    g2 = orc.bf16_weight_model_grads(v, t, TAU, W)["grad_v"]
    for a, b in ((g0, g1), (g0, g2), (g1, g2)):
        assert 3e-4 <= xi.check_rows(a, b)[0] <= 2e-2
    with pytest.raises(NotImplementedError):
        orc.bf16_weight_model_grads(v, t, 0.004, 1.0, saved=False)


EMULATED = [  # B, D, kind, weighted
    (200, 64, "plain", False), (200, 64, "mixed", True), (130, 192, "inter", False), (130, 192, "intra", True),
]
KERNELS = {  # (mode, saved) -> forward, backward
    ("fp32", True): ("fwd_sums_kernel (symmetric, save)", "bwd_saved32_kernel"), ("fp32", False): ("fwd_sums_kernel (symmetric)", "bwd_kernel"),
    ("bf16x3", True): ("fwd_sums_kernel<x3_t> (symmetric, save)", "bwd_saved_x3_kernel"),
    ("bf16x3", False): ("fwd_sums_kernel<x3_t> (symmetric)", "bwd_kernel<x3_t>"),
    ("bf16", True): ("fast_fwd_pipe_kernel", "fast_bwd_dsl_kernel (LDS-staged)"), ("bf16", False): ("fast_fwd_pipe_kernel", "fast_bwd_kernel (recomputing)"),
}


@pytest.mark.parametrize("saved", [True, False], ids=["saved", "recomputing"])
@pytest.mark.parametrize("mode", xi.MODES)
@pytest.mark.parametrize("B,D,kind,weighted", EMULATED)
def test_emulated_kernels_per_row(B, D, kind, weighted, mode, saved, monkeypatch):
    if not saved:
        monkeypatch.setenv("CROSSCLR_DISABLE_SAVE", "1")
    v, t = xi.planted(kind, B, D, seed=B + D)
    k, om = xi.sample_weights(B, B + D) if weighted else (None, None)
    loss, gv, gt = xi.run_loss(v, t, TAU, W, mode, k, om)
    lib = nat.library()
    assert (lib.crossclr_last_kernel(0).decode(), lib.crossclr_last_kernel(1).decode()) == KERNELS[mode, saved]
    m, wv, wt, sv, st = xi.yardstick(v, t, TAU, W, mode, saved, k, om)
    exact = orc.stacked_weight_model(v, t, TAU, W, k, om)
    e_loss = abs(loss - float(exact["loss"])) / max(1.0, abs(float(exact["loss"])))
    ev, et = xi.check_rows(gv, wv, slack=sv), xi.check_rows(gt, wt, slack=st)
    print(f"{mode} saved={saved} {kind} B={B} D={D} weighted={weighted}: video {ev[0]:.3e} @ row {ev[1]}  text {et[0]:.3e} @ row {et[1]}  loss {e_loss:.3e}")
    assert e_loss <= xi.LOSS_BAR
    assert max(ev[0], et[0]) <= xi.GRAD_BAR[mode, False, saved]


@pytest.mark.parametrize("mode", xi.MODES)
@pytest.mark.parametrize("B,D,tau,w", [(130, 192, TAU, W), (100, 64, 0.01, 1.0), (100, 64, 0.004, 1.0)])
def test_emulated_forward_statistics_per_row(B, D, tau, w, mode):
    """logZ per row, the positive pair's logit and the loss of the saving forward, as tests/test_gpu_exact_operands.py asserts them"""
    v, t = xi.planted("mixed", B, D, seed=B + D)
    m = orc.stacked_weight_model(v, t, tau, w)
    loss, ws = L._forward_impl(v, t, tau, w, mode, None, save_for_backward=True)
    bp = ws.plan.bpad
    rows = torch.cat([torch.arange(B), bp + torch.arange(B)])
    want, bar = torch.cat([m["logZv"], m["logZt"]]), xi.LOGZ_BAR
    logz = ws.logz.double()[rows]
    if orc.needs_row_shift(tau, w):      # (the form the fp32 statistics hold: see check_forward of the GPU file; the host build does not
        m32 = orc.stacked_weight_model(v, t, tau, w, fp32_logits="product")      # contract scale and shift into one fma: the product is rounded)
        want, bar = torch.cat([m32["logZv"], m32["logZt"]]), xi.LOGZ_BAR_TWO_PASS
        logz = ws.shift.double()[rows] * 0.6931471805599453 - torch.log(ws.rz.double()[rows])
    assert (logz - want).abs().max().item() <= bar
    assert (ws.diag.double()[:B] / tau - m["diag"]).abs().max().item() <= xi.LOGZ_BAR
    assert abs(float(loss) - float(m["loss"])) <= xi.LOSS_BAR * max(1.0, abs(float(m["loss"])))


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_emulated_two_pass_bf16_backward_against_the_weight_model(weighted):
    B, D, tau, w = 130, 192, 0.004, 1.0
    v, t = xi.planted("mixed", B, D, seed=B + D)
    k, om = xi.sample_weights(B, B + D) if weighted else (None, None)
    loss, gv, gt = xi.run_loss(v, t, tau, w, "bf16", k, om)
    assert nat.library().crossclr_last_kernel(1) == b"fast_bwd_dsl_kernel (LDS-staged)"
    m, wv, wt, sv, st = xi.yardstick(v, t, tau, w, "bf16", True, k, om)
    ev, et = xi.check_rows(gv, wv, slack=sv), xi.check_rows(gt, wt, slack=st)
    f64 = xi.check_rows(gv, orc.grads_from_stacked_weights(orc.stacked_weight_model(v, t, tau, w, k, om))[0])[0]
    print(f"two-pass bf16 weighted={weighted}: video {ev[0]:.3e} text {et[0]:.3e}; against plain float64 {f64:.3e}")
    assert max(ev[0], et[0]) <= xi.GRAD_BAR["bf16", True, True] and f64 >= 10 * xi.GRAD_BAR["bf16", True, True]


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("entry", ["crossclr_backward_saved", "crossclr_backward_saved_xf", "crossclr_backward_saved_xfp"])
def test_emulated_saved_backward_entry_points(entry, weighted):
    B, D = 130, 192
    v, t = xi.planted("mixed", B, D, seed=B + D)
    k, om = xi.sample_weights(B, B + D) if weighted else (None, None)
    loss, gv, gt = xi.saved_backward_via_cabi(v, t, TAU, W, k, om, entry)
    m, wv, wt, sv, st = xi.yardstick(v, t, TAU, W, "bf16", True, k, om)
    assert max(xi.check_rows(gv, wv, slack=sv)[0], xi.check_rows(gt, wt, slack=st)[0]) <= xi.GRAD_BAR["bf16", False, True]


# ----------------------------------------------------------------------------------------------------------------------------------
# teeth
# ----------------------------------------------------------------------------------------------------------------------------------
def _gpu_cases():
    """(kind, B, D, tau, w, weighted, mode, bar) of every gradient case of the GPU file"""
    out = []
    for mode, kind, B, D, tau, w, recompute, _kernel in xi.BACKWARD:
        for weighted in (False, True):
            out.append((kind, B, D, tau, w, weighted, mode, xi.GRAD_BAR[mode, orc.needs_row_shift(tau, w), not recompute]))
    B, D, tau, w = xi.TWO_PASS_BF16
    for weighted in (False, True):
        out.append(("mixed", B, D, tau, w, weighted, "bf16", xi.GRAD_BAR["bf16", True, True]))
        out.append(("mixed", xi.PAIR_SCHEME[1], xi.PAIR_SCHEME[2], TAU, W, weighted, "bf16", xi.GRAD_BAR["bf16", False, True]))
        for B2, D2 in xi.CABI_SHAPES:
            out.append(("mixed", B2, D2, TAU, W, weighted, "bf16", xi.GRAD_BAR["bf16", False, True]))
    for mode, D in xi.THREE_RANKS:
        out.append(("mixed", 300, D, TAU, W, False, mode, xi.GRAD_BAR[mode, False, True]))
    for _dtype, mode in xi.DTYPES:
        out.append(("mixed", 200, 192, TAU, W, False, mode, xi.GRAD_BAR[mode, False, True]))
    return sorted(set(out))


_tiles, _defective_weights = xi.tiles, xi.defective_weights      # (shared with tests/test_projection_exact_cpu.py)


_TEETH_GROUPS = {}
for _c in _gpu_cases():
    _TEETH_GROUPS.setdefault(_c[:6], []).append(_c[6:])


@pytest.mark.parametrize("kind,B,D,tau,w,weighted", sorted(_TEETH_GROUPS), ids=lambda x: str(x))
def test_teeth_every_gpu_case_shows_every_defect_at_ten_bars(kind, B, D, tau, w, weighted):
    v, t = xi.planted(kind, B, D, seed=B + D)
    k, om = xi.sample_weights(B, B + D) if weighted else (None, None)
    clean = orc.stacked_weight_model(v, t, tau, w, k, om)
    assert torch.equal(_defective_weights(clean), clean["W"])
    want = torch.cat(orc.grads_from_stacked_weights(clean))
    slack = None
    if any(mode == "bf16" for mode, _ in _TEETH_GROUPS[kind, B, D, tau, w, weighted]):
        slack = orc.stacked_weight_model(v, t, tau, w, k, om, roundings=2)["slack_rows"]      # what the bf16 yardstick forgives a row
    bar = max(b for _, b in _TEETH_GROUPS[kind, B, D, tau, w, weighted])
    defects = {}
    for name, (rows, cols) in _tiles(B).items():
        Wd = clean["W"].clone()
        Wd[rows, cols] = 0.0
        defects["tile dropped: " + name] = Wd
    defects["column statistics of the neighbouring column"] = _defective_weights(clean, col_stat_shift=1)
    if weighted:
        defects["column sample weights ignored"] = _defective_weights(clean, ignore_col_k=True)
    for name, Wd in defects.items():
        worst, row = xi.check_rows(torch.cat(orc.grads_from_stacked_weights(clean, Wd)), want, slack=slack)
        print(f"{name}: row {row} moves by {worst:.3e} of its gradient = {worst / bar:.0f} bars")
        assert worst >= 10 * bar, (name, worst, bar)


@pytest.mark.parametrize("B,D,tau,w", sorted({(B, D, tau, w) for _m, B, D, tau, w, _k in xi.FORWARD}), ids=lambda x: str(x))
def test_teeth_every_forward_shape_shows_a_dropped_tile_in_logz(B, D, tau, w):
    """a 32 x 32 tile of exponentials missing from the row sums moves logZ of one of its rows by at least 10 x the bar it is held to"""
    v, t = xi.planted("mixed", B, D, seed=B + D)
    m = orc.stacked_weight_model(v, t, tau, w)
    logz = torch.cat([m["logZv"], m["logZt"]])
    share = torch.exp(m["logits"] - logz[:, None])       # every term's share of its row's Z (no sample weights here)
    bar = xi.LOGZ_BAR_TWO_PASS if orc.needs_row_shift(tau, w) else xi.LOGZ_BAR
    for name, (rows, cols) in _tiles(B).items():
        moved = -torch.log1p(-share[rows, cols].sum(1).clamp_max(1 - 1e-15))
        print(f"tile dropped: {name}: logZ moves by {moved.max().item():.3e} = {moved.max().item() / bar:.0f} bars")
        assert moved.max().item() >= 10 * bar, name
