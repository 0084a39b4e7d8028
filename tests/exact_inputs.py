"""Inputs every compute mode holds EXACTLY, and the per-row checker of the exact-operand tests (tests/test_exact_operands_cpu.py,
tests/test_gpu_exact_operands.py).  A helper module like tests/fwd_sums_table.py: pytest collects nothing here.

Rows with `nnz` entries of +-1 (nnz a power of four) and zeros elsewhere have the norm sqrt(nnz) = 2^j: their unit rows are +-2^-j,
which bf16 holds, every cosine is a multiple of 1 / nnz, and every partial sum of a similarity product is exact in fp32.  The bf16,
bf16x3 and fp32 modes then see the same operands and the same cosines as the float64 oracle: what is left between a kernel and its
yardstick is the arithmetic AFTER the products (exponentials, sums, the weights' roundings), 1e-6 and not 1e-2.  Planted near-duplicate
pairs make the soft-max denominators differ from row to row by many units (on random rows they differ by a few per cent), so a statistic
read from the wrong row or column is visible.

Yardsticks: oracle/crossclr_oracle.py -- `streaming_loss_and_grads` / `stacked_weight_model(roundings=0)` for fp32 and bf16x3,
`bf16_weight_model_grads` (the weights' two bf16 roundings) for the bf16 backward."""
import math

import torch
import torch.nn.functional as F

NNZ = (4, 16, 64, 256)


def default_nnz(D):
    return 16 if D < 64 else (64 if D < 1024 else 256)


def assert_exact(*sets):
    """The exactness condition: the unit rows survive a round trip through bf16 unchanged, and the float32 and float64 Gram matrices of
    all rows agree exactly."""
    x32 = torch.cat([F.normalize(x.float(), dim=1) for x in sets])
    assert torch.equal(x32.bfloat16().float(), x32), "unit rows are not bf16 values"
    x64 = torch.cat([F.normalize(x.double(), dim=1) for x in sets])
    assert torch.equal(x64, x32.double())
    assert torch.equal((x32 @ x32.t()).double(), x64 @ x64.t()), "the float32 Gram matrix is not exact"


def _sign_rows(B, D, nnz, g):
    assert nnz in NNZ and nnz <= D, (nnz, D)
    support = torch.rand(B, D, generator=g).argsort(1)[:, :nnz]
    signs = torch.randint(0, 2, (B, nnz), generator=g).float() * 2 - 1
    return torch.zeros(B, D).scatter_(1, support, signs)


def sign_rows(B, D, nnz=None, seed=0):
    """[B, D] float32: +-1 on a random support of `nnz` columns per row (norm sqrt(nnz))."""
    x = _sign_rows(B, D, nnz or default_nnz(D), torch.Generator().manual_seed(seed))
    assert_exact(x)
    return x


def _near_duplicate(row, flips, g):
    """`row` with `flips` of its non-zero entries negated: cosine (nnz - 2 flips) / nnz with the original"""
    idx = row.nonzero().flatten()
    out = row.clone()
    out[idx[torch.randperm(idx.numel(), generator=g)[:flips]]] *= -1
    return out


def _coprime_near(x, n):
    a = max(1, int(x))
    while math.gcd(a, n) != 1:
        a += 1
    return a


def planted(kind, B, D, nnz=None, seed=0):
    """(video, text) sign rows with planted near-duplicate pairs (2 .. 10 sign flips, at most nnz / 4) on every other row; the rows in
    between stay random, so that every tile of the weight matrix keeps rows whose weights are spread over all columns.

    "plain"  nothing planted
    "inter"  t[pi(i)] = v[i] + flips, pi(i) = (a i + B - 1) mod B with a ~ 0.618 B coprime to B: partners scattered over the 32-, 128- and
             256-row boundaries, pi(0) = B - 1 in the last (ragged) tile; never the positive pair itself; and t[B - 2] = v[B - 1] + 2 flips,
             the pair that loads the tile (last ragged rows) x (last ragged columns), and t[1] = v[B - 3] + 3 flips across the modality boundary
    "intra"  near-duplicate pairs (row 4 m, an odd row) inside each modality, scattered the same way, another pairing per modality
    "mixed"  both"""
    assert kind in ("plain", "inter", "intra", "mixed"), kind
    nnz = nnz or default_nnz(D)
    g = torch.Generator().manual_seed(seed)
    v, t = _sign_rows(B, D, nnz, g), _sign_rows(B, D, nnz, g)
    nflip = lambda i: 2 + i % max(1, min(9, nnz // 4 - 1))
    if kind in ("intra", "mixed"):
        h = B // 2
        for x, frac in ((v, 0.618), (t, 0.382)):
            a = _coprime_near(frac * h, h)
            for m in range(0, h, 2):
                x[2 * ((a * m + h - 1) % h) + 1] = _near_duplicate(x[2 * m], nflip(m // 2), g)
    if kind in ("inter", "mixed"):
        a = _coprime_near(0.618 * B, B)
        for i in range(0, B, 2):
            j = (a * i + B - 1) % B
            if j != i:
                t[j] = _near_duplicate(v[i], nflip(i // 2), g)
        if B >= 5:
            t[B - 2] = _near_duplicate(v[B - 1], 2, g)      # a pair inside the last (ragged) tile of both modalities
            t[1] = _near_duplicate(v[B - 3], 3, g)          # and one in (last video tile) x (first text tile), across the modality boundary
    assert_exact(v, t)
    return v, t


def sample_weights(B, seed=0):
    """negative_scale with zeros (and 2s), loss_weight in powers of two: products with them are exact in fp32"""
    g = torch.Generator().manual_seed(1000 + seed)
    pick = lambda values: torch.tensor(values)[torch.randint(0, len(values), (B,), generator=g)]
    k = (pick([0.0, 1.0, 1.0, 2.0]), pick([0.0, 1.0, 1.0, 0.5]))
    omega = (pick([0.5, 1.0, 2.0]), pick([0.25, 1.0, 2.0, 0.0]))
    return k, omega


def check_rows(got, want, bar=None, slack=None):
    """Per row i: max_d |got - want| / max_d |want_i|.  Returns (worst ratio, its row); with `bar` asserts worst <= bar.
    slack [rows]: what a row may be off by before anything counts (oracle.stacked_weight_model's `slack_rows`: weights at a bf16 tie)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got - want).abs().amax(1)
    if slack is not None:
        err = (err - slack.double()).clamp_min(0.0)
    den = want.abs().amax(1)
    ratio = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst, idx = ratio.max(0)
    worst, idx = float(worst), int(idx)
    if bar is not None:
        assert worst <= bar, f"row {idx}: max|delta| / max|want| = {worst:.3e} > {bar:.1e}"
    return worst, idx


def run_loss(v, t, tau, w, mode, k=None, omega=None):
    """loss and input gradients through crossclr_amd.crossclr_loss on the tensors' device"""
    import crossclr_amd
    vv, tt = v.clone().requires_grad_(True), t.clone().requires_grad_(True)
    kw = {}
    if k is not None:
        kw = dict(negative_scale=tuple(x.to(v.device) for x in k), loss_weight=tuple(x.to(v.device) for x in omega))
    loss = crossclr_amd.crossclr_loss(vv, tt, tau, w, compute_mode=mode, **kw)
    loss.backward()
    return float(loss.detach()), vv.grad, tt.grad


def saved_backward_via_cabi(v, t, tau, w, k, om, entry_name):
    """forward (saving) and one of the saved backwards of the local block through the fine-grained C-ABI entry points, on the tensors' device:
    crossclr_normalize_xf, crossclr_forward_save, crossclr_forward_finish_w, `entry_name`, crossclr_backward_finish_w.  (loss, grad_v, grad_t)"""
    import ctypes
    from crossclr_amd import _native as nat
    from crossclr_amd import loss as L
    lib, p = nat.library(), L._ptr
    B, D = v.shape
    dev, stream = v.device, L._stream_for(v)
    plan = nat.make_plan(B, D, 1, 0, nat.MODE_BF16)
    assert plan.stash_bytes > 0 and plan.xf_bytes == plan.operand_bytes
    pp = ctypes.byref(plan)
    n2 = 2 * plan.bpad
    f32 = dict(dtype=torch.float32, device=dev)
    xhat = torch.empty(plan.operand_bytes, dtype=torch.uint8, device=dev)
    xf = torch.empty(plan.xf_bytes, dtype=torch.uint8, device=dev)
    inv_norm, diag = torch.empty(n2, **f32), torch.empty(plan.bpad, **f32)
    logz, rz, wrz = torch.empty(n2, **f32), torch.empty(n2, **f32), torch.empty(n2, **f32)
    part = torch.empty(plan.fwd_ws_floats, **f32)
    loss_sum = torch.empty(max(2, plan.loss_ws_doubles), dtype=torch.float64, device=dev)
    stash = torch.empty(plan.stash_bytes, dtype=torch.uint8, device=dev)
    ks = L._pack_pair(k, B, plan.bpad, dev, "negative_scale")
    lw = L._pack_pair(om, B, plan.bpad, dev, "loss_weight")
    sw = L._sw(ks, ks, lw)
    nat.check(lib.crossclr_normalize_xf(pp, p(v), p(t), v.stride(0), t.stride(0), nat.IN_F32, p(xhat), p(xf), p(inv_norm), p(diag), stream))
    nat.check(lib.crossclr_forward_save(pp, p(xhat), tau, w, sw, p(part), 0, p(stash), stream))
    nat.check(lib.crossclr_forward_finish_w(pp, p(part), plan.fwd_slots, p(diag), tau, w, sw, p(logz), p(rz), p(wrz), p(loss_sum), stream))
    gbuf = torch.full((plan.gbuf_bytes // 4,), float("nan"), **f32)
    operand = xhat if entry_name == "crossclr_backward_saved" else xf
    nat.check(getattr(lib, entry_name)(pp, p(operand), p(stash), tau, w, p(rz), p(wrz), sw, p(gbuf), 0, stream))
    gv, gt = torch.empty_like(v), torch.empty_like(t)
    go = torch.ones(1, dtype=torch.float64, device=dev)
    nat.check(lib.crossclr_backward_finish_w(pp, p(gbuf), p(v), p(t), v.stride(0), t.stride(0), nat.IN_F32, p(inv_norm), tau, sw, p(go), p(gv), p(gt),
                                             gv.stride(0), gt.stride(0), stream))
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return float(loss_sum[0]) / (2.0 * B), gv, gt


def yardstick(v, t, tau, w, mode, saved, k=None, omega=None):
    """The float64 yardstick of a mode's gradients: the exact closed form for fp32 and bf16x3, the weight model for bf16 (with the rows'
    slack for weights at a bf16 tie).  Returns (model, grad_video, grad_text, slack_video, slack_text)."""
    from oracle import crossclr_oracle as orc
    rounds = 0 if mode != "bf16" else (2 if saved else 1)
    m = orc.stacked_weight_model(v.cpu(), t.cpu(), tau, w, k, omega, roundings=rounds)
    gv, gt = orc.grads_from_stacked_weights(m)
    B = v.shape[0]
    return m, gv, gt, m["slack_rows"][:B], m["slack_rows"][B:]


# ----------------------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_exact_operands.py (shared with the teeth test of tests/test_exact_operands_cpu.py)
# ----------------------------------------------------------------------------------------------------------------------------------
TAU, W = 0.03, 0.8
MODES = ("fp32", "bf16x3", "bf16")
# (the wide 4-wave forward at Dpad 768 / 1024 reports the same name as the 8-wave one: the shape selects the instantiation, the name
#  assertion only says that the register-resident family ran)
FORWARD = [  # mode, B, D, tau, w, kernel of the saving forward
    ("bf16", 300, 100, TAU, W, "fast_fwd_pipe_kernel"), ("bf16", 300, 256, TAU, W, "fast_fwd_pipe_kernel"),
    ("bf16", 300, 384, TAU, W, "fast_fwd_pipe_kernel"), ("bf16", 300, 512, TAU, W, "fast_fwd_pipe_kernel"),
    ("bf16", 256, 128, TAU, W, "fast_fwd_pair_kernel"), ("bf16", 256, 1024, TAU, W, "fast_fwd_pair_kernel"),
    ("bf16", 300, 768, TAU, W, "fast_fwd_pipe_kernel"), ("bf16", 300, 1024, TAU, W, "fast_fwd_pipe_kernel"),      # the wide 4-wave forward
    ("fp32", 300, 200, TAU, W, "fwd_sums_kernel (symmetric, save)"), ("bf16x3", 300, 200, TAU, W, "fwd_sums_kernel<x3_t> (symmetric, save)"),
    ("bf16", 150, 1100, TAU, W, "fwd_sums_kernel (symmetric, save, bf16 records)"),
    ("bf16", 150, 1536, TAU, W, "fwd_sums_kernel (symmetric, save, bf16 records)"),
    ("bf16", 150, 2300, TAU, W, "fwd_sums_kernel (symmetric, save, bf16 records)"),
    ("bf16", 200, 64, 0.01, 1.0, "fast_fwd_pipe_kernel"),                                                             # the common shift (64 < 1 / tau <= 128)
    ("fp32", 200, 192, 0.004, 1.0, "fwd_sums_kernel"), ("bf16x3", 200, 192, 0.004, 1.0, "fwd_sums_kernel<x3_t>"),     # the two-pass regime
    ("bf16", 200, 192, 0.004, 1.0, "fwd_sums_kernel"),
]
SAVED32, SAVEDX3 = "bwd_saved32_kernel", "bwd_saved_x3_kernel"
LDS, WIDE = "fast_bwd_dsl_kernel (LDS-staged)", "fast_bwd_dsl_kernel (wide, column parts)"
BACKWARD = [  # mode, kind, B, D, tau, w, recompute, backward kernel
    ("fp32", "mixed", 300, 40, TAU, W, False, SAVED32), ("fp32", "inter", 130, 200, TAU, W, False, SAVED32),
    ("fp32", "mixed", 200, 192, 0.004, 1.0, False, SAVED32),
    ("bf16x3", "mixed", 300, 40, TAU, W, False, SAVEDX3), ("bf16x3", "mixed", 130, 200, TAU, W, False, SAVEDX3),
    ("bf16x3", "mixed", 200, 192, 0.004, 1.0, False, SAVEDX3),
    ("fp32", "mixed", 300, 40, TAU, W, True, "bwd_kernel"), ("fp32", "mixed", 130, 300, TAU, W, True, "bwd_kernel"),
    ("bf16x3", "mixed", 300, 40, TAU, W, True, "bwd_kernel<x3_t>"), ("bf16x3", "mixed", 130, 300, TAU, W, True, "bwd_kernel<x3_t>"),
    ("fp32", "mixed", 200, 192, 0.004, 1.0, True, "bwd_kernel"), ("bf16x3", "mixed", 200, 192, 0.004, 1.0, True, "bwd_kernel<x3_t>"),
    # bf16, LDS-staged saved backward at every padded width of its table
    ("bf16", "mixed", 300, 40, TAU, W, False, LDS), ("bf16", "inter", 130, 200, TAU, W, False, LDS), ("bf16", "mixed", 200, 384, TAU, W, False, LDS),
    ("bf16", "mixed", 130, 512, TAU, W, False, LDS), ("bf16", "mixed", 300, 768, TAU, W, False, LDS), ("bf16", "mixed", 256, 1024, TAU, W, False, LDS),
    ("bf16", "mixed", 200, 64, 0.01, 1.0, False, LDS),
    # the D-slice column parts of the wide plans
    ("bf16", "mixed", 150, 1100, TAU, W, False, WIDE), ("bf16", "mixed", 150, 1536, TAU, W, False, WIDE), ("bf16", "mixed", 150, 2300, TAU, W, False, WIDE),
    # the recomputing 32- and 16-row kernels
    ("bf16", "mixed", 200, 384, TAU, W, True, "fast_bwd_kernel (recomputing)"), ("bf16", "mixed", 300, 768, TAU, W, True, "fast_bwd16_kernel (recomputing)"),
]
CABI_SHAPES = [(300, 40), (130, 512), (256, 1024), (384, 384)]
THREE_RANKS = [("bf16", 1100), ("fp32", 96)]            # rectangular saved blocks: the wide bf16 plan's column parts, bwd_saved32_kernel (rect)
PAIR_SCHEME = (3, 384, 256)                             # world, B, D of the bf16 pair scheme (rectangular + transposed blocks)
DTYPES = [("float16", "bf16"), ("bfloat16", "fp32"), ("float64", "bf16x3")]


TWO_PASS_BF16 = (200, 192, 0.004, 1.0)                  # B, D, tau, w of the two-pass bf16 backward

# Bars of the exact-operand tests: 4 x the worst error of the unmodified kernels against the float64 yardstick on the MI355X (the figures
# are in the docstring of tests/test_gpu_exact_operands.py), under the ceilings 1e-4 (gradient rows) and 2e-5 (logZ, loss).
# Keys of GRAD_BAR: (compute mode, two-pass regime, saved exponentials).
GRAD_BAR = {("fp32", False, True): 3.7e-6, ("fp32", False, False): 3.7e-6, ("fp32", True, True): 1.4e-6, ("fp32", True, False): 4.4e-5,
            ("bf16x3", False, True): 7.2e-5, ("bf16x3", False, False): 7.2e-5, ("bf16x3", True, True): 1.8e-5, ("bf16x3", True, False): 4.4e-5,
            ("bf16", False, True): 1.7e-5, ("bf16", False, False): 1.7e-5, ("bf16", True, True): 1.7e-5}
LOGZ_BAR = 2e-5                      # (the ceiling: 3.3 x the worst measured)
LOGZ_BAR_TWO_PASS = 2.9e-6           # ln 2 * shift - log(rz) against the closed form on the kernels' own scaled logits
LOSS_BAR = 2.7e-7                    # relative to max(1, |loss|)
SLACK_ROWS_MAX = 0.10                # at most this fraction of a case's rows may carry a tie allowance above the bar (measured: 1 .. 7 %)


def slack_fraction(model, bar):
    """fraction of the rows of a rounded weight model whose tie allowance (`slack_rows`) exceeds bar x the row's largest gradient entry"""
    g = torch.cat(model["grads"]) if "grads" in model else None
    assert g is not None
    return float((model["slack_rows"] > bar * g.abs().amax(1)).double().mean())
