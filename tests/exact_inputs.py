"""Inputs every compute mode holds EXACTLY, and the per-row checker of the exact-operand tests (tests/test_exact_operands_cpu.py,
tests/test_gpu_exact_operands.py).  A helper module like tests/fwd_sums_table.py: pytest collects nothing here.  The second half holds the same for the fused projection head
(tests/test_projection_exact_cpu.py, tests/test_gpu_projection_exact.py): `projection_inputs` and the C-ABI runners.

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


def assert_exact(*sets, gram=True):
    """The exactness condition: the unit rows survive a round trip through bf16 unchanged, and the float32 and float64 Gram matrices of
    all rows agree exactly (gram=False: the rows' condition only, O(B D) -- for batches whose Gram matrix does not fit)."""
    x32 = torch.cat([F.normalize(x.float(), dim=1) for x in sets])
    assert torch.equal(x32.bfloat16().float(), x32), "unit rows are not bf16 values"
    x64 = torch.cat([F.normalize(x.double(), dim=1) for x in sets])
    assert torch.equal(x64, x32.double())
    if gram:
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


def planted(kind, B, D, nnz=None, seed=0, gram=True):
    """(video, text) sign rows with planted near-duplicate pairs (2 .. 10 sign flips, at most nnz / 4) on every other row; the rows in
    between stay random, so that every tile of the weight matrix keeps rows whose weights are spread over all columns.

    "plain"  nothing planted
    "inter"  t[pi(i)] = v[i] + flips, pi(i) = (a i + B - 1) mod B with a ~ 0.618 B coprime to B: partners scattered over the 32-, 128- and
             256-row boundaries, pi(0) = B - 1 in the last (ragged) tile; never the positive pair itself; and t[B - 2] = v[B - 1] + 2 flips,
             the pair that loads the tile (last ragged rows) x (last ragged columns), and t[1] = v[B - 3] + 3 flips across the modality boundary
    "intra"  near-duplicate pairs (row 4 m, an odd row) inside each modality, scattered the same way, another pairing per modality
    "mixed"  both
    gram=False: skip the Gram-matrix half of the exactness condition (`assert_exact`), for batches of many thousand rows"""
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
    assert_exact(v, t, gram=gram)
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


# ----------------------------------------------------------------------------------------------------------------------------------
# Defects of the weight matrix, for the teeth tests (they live here, not in the oracle)
# ----------------------------------------------------------------------------------------------------------------------------------
def tiles(B):
    """(rows, columns) of the dropped tiles in stacked coordinates (video rows 0 .. B-1, text rows B .. 2B-1; the kernels' tiles start at each
    modality's first row): first, last ragged, across the video / text boundary, mirrored (left of the diagonal)"""
    last = 32 * ((B - 1) // 32)
    second = 32 if B > 32 else 0
    return {"first": (slice(0, 32), slice(0, 32)),
            "last ragged": (slice(B + last, 2 * B), slice(last, B)),
            "across the modality boundary": (slice(last, B), slice(B, B + 32)),
            "mirrored": (slice(B + second, B + second + 32), slice(0, 32))}


def defective_weights(m, col_stat_shift=0, ignore_col_k=False):
    """W of an exact model (oracle.exact_weights) with the COLUMN statistics read `col_stat_shift` columns further on, or the columns'
    sample weights ignored"""
    from oracle import crossclr_oracle as orc
    logz, om = torch.cat([m["logZv"], m["logZt"]]), m["omega"]
    k_cols = torch.ones_like(m["k_cols"]) if ignore_col_k else m["k_cols"]
    W = orc.exact_weights(m["logits"], logz, torch.roll(logz, -col_stat_shift), om, torch.roll(om, -col_stat_shift), k_cols, m["k_rows"], m["intra"], m["w"])
    return W.masked_fill(torch.eye(W.shape[0], dtype=torch.bool), 0.0)


# ----------------------------------------------------------------------------------------------------------------------------------
# The fused projection head on exact operands
# ----------------------------------------------------------------------------------------------------------------------------------
def _sylvester(n):
    H = torch.ones(1, 1, dtype=torch.float64)
    while H.shape[0] < n:
        H = torch.cat([torch.cat([H, H], 1), torch.cat([H, -H], 1)], 0)
    assert H.shape[0] == n
    return H


def hadamard_blocks(Din):
    """the greedy power-of-two split of Din starting at 64: 101 -> 64, 32, 4, 1"""
    out, size = [], 64
    while Din > 0:
        while size > Din:
            size //= 2
        out.append(size)
        Din -= size
    return out


def hadamard_mix(Din):
    """(H, s): H [Din, Din] block-diagonal from Sylvester-Hadamard blocks (symmetric, H H = diag(block size)), s [Din] = 1 / block size"""
    blocks = hadamard_blocks(Din)
    H = torch.block_diag(*[_sylvester(n) for n in blocks])
    s = torch.cat([torch.full((n,), 1.0 / n, dtype=torch.float64) for n in blocks])
    assert torch.equal(H @ (H * s[None, :]), torch.eye(Din, dtype=torch.float64))
    return H, s


def projection_inputs(b, D, din_v, din_t, bias=(True, True), seed=None, zero_row=None, gram=True):
    """Inputs of the fused projection head whose projected features are the planted sign rows (Y_v, Y_t) = planted("mixed", b, D) EXACTLY,
    in bf16-operand / fp32-accumulate arithmetic and in any summation order:
        bias_d in {-1, 0, 1} (or none),   X = [Y - bias | 0] H   (small integers: at most 64 terms of size <= 2),
        W = (H^T diag(1 / block size))[:D]   (entries +-2^-k, 64 non-zeros per row in full blocks)
    with H = `hadamard_mix(Din)`: X W^T = [Y - bias | 0] H diag(1 / n) H [:, :D] = Y - bias.  Every input column feeds every output column
    of its block, so a lost k-step or a mis-addressed weight fragment changes Y.
    Din < D (both modalities alike, D / Din a power of four): the same mix for sign rows Z of width Din, the weight block and the bias
    repeated D / Din times: Y = [Z | Z | ...], again sign rows with a power of four of non-zeros.
    zero_row = i (no bias): row i of both inputs is zero, and so is row i of Y.
    Returns {"x": (xv, xt), "w": (wv, wt), "bias": (bv | None, bt | None), "y": (Yv, Yt)}, all float32 on the CPU; asserts its own
    conditions: X and W are bf16 values (X fp16 values too), the float32 product plus bias equals the float64 one bit for bit and is Y,
    and `assert_exact(Y_v, Y_t)`."""
    seed = b + D if seed is None else seed
    g = torch.Generator().manual_seed(5000 + seed)
    rep = 1
    if min(din_v, din_t) < D:
        assert din_v == din_t and D % din_v == 0 and D // din_v in (4, 16, 64), (D, din_v, din_t)
        rep = D // din_v
        nnz = default_nnz(D) // rep
        zv, zt = planted("mixed", b, din_v, nnz, seed=seed, gram=False)
        yv, yt = zv.repeat(1, rep), zt.repeat(1, rep)
        assert_exact(yv, yt, gram=gram)
    else:
        yv, yt = planted("mixed", b, D, seed=seed, gram=gram)
    if zero_row is not None:
        assert bias == (False, False)
        yv[zero_row] = 0.0
        yt[zero_row] = 0.0
    xs, ws, bs = [], [], []
    for y, din, has_bias in ((yv, din_v, bias[0]), (yt, din_t, bias[1])):
        d0 = D // rep                                       # width of the block that is mixed
        b0 = (torch.randint(0, 3, (d0,), generator=g).double() - 1.0) if has_bias else torch.zeros(d0, dtype=torch.float64)
        H, s = hadamard_mix(din)
        z = torch.zeros(b, din, dtype=torch.float64)
        z[:, :d0] = y[:, :d0].double() - b0
        x = z @ H
        w = (H.t() * s[None, :])[:d0].repeat(rep, 1)          # [D, Din]
        bvec = b0.repeat(rep)
        x32, w32, b32 = x.float(), w.float(), bvec.float()
        assert torch.equal(x32.double(), x) and torch.equal(x32.bfloat16().float(), x32) and torch.equal(x32.half().float(), x32)
        assert torch.equal(w32.double(), w) and torch.equal(w32.bfloat16().float(), w32)
        y32, y64 = x32 @ w32.t() + b32, x @ w.t() + bvec
        assert torch.equal(y32.double(), y64), "the float32 projection is not exact"
        assert torch.equal(y32, y), "the projection is not the planted rows"
        xs.append(x32)
        ws.append(w32)
        bs.append(b32 if has_bias else None)
    # (input columns past the last block that holds a column of Y are zero, with zero weights: k-steps from `live` on carry nothing)
    live = tuple(sum(n for i, n in enumerate(hadamard_blocks(din)) if sum(hadamard_blocks(din)[:i]) < D // rep) for din in (din_v, din_t))
    return {"x": tuple(xs), "w": tuple(ws), "bias": tuple(bs), "y": (yv, yt), "b": b, "D": D, "live": live}


def projection_outputs(yv, yt):
    """(unit_v, unit_t, inv_v, inv_t, cos) of projected features in float64, rounded once to the kernel's output types: the unit rows to
    bf16, 1 / max(||y||, 1e-12) and the positive pair's cosine to fp32"""
    units, invs = [], []
    for y in (yv, yt):
        n = y.double().norm(dim=1)
        units.append(F.normalize(y.double(), dim=1))
        invs.append(torch.where(n > 1e-12, 1.0 / n.clamp_min(1e-300), torch.tensor(1e12, dtype=torch.float64)).float())
    return units[0].bfloat16(), units[1].bfloat16(), invs[0], invs[1], (units[0] * units[1]).sum(1).float()


def projection_expected(yv, yt):
    """`projection_outputs` of projected features that fp32 holds exactly with norms 2^j (or 0): what crossclr_project_pack must write,
    each a value of its type WITHOUT rounding (asserted)."""
    out = projection_outputs(yv, yt)
    for y, u, inv in zip((yv, yt), out[:2], out[2:4]):
        n = y.double().norm(dim=1)
        assert torch.equal(torch.where(n > 0, torch.exp2(torch.log2(n.clamp_min(1e-300)).round()), n), n), "norms are not powers of two"
        assert torch.equal(u.double(), F.normalize(y.double(), dim=1)) and torch.equal(u.float(), F.normalize(y.float(), dim=1))
        assert torch.equal(torch.where(n > 0, inv.double() * n, torch.ones_like(n)), torch.ones_like(n))
    assert torch.equal(out[4].double(), (F.normalize(yv.double(), dim=1) * F.normalize(yt.double(), dim=1)).sum(1))
    return out


LAYOUTS = ("contiguous", "ld+1", "ld+3", "offset")


def lay_out(x, dtype, layout, device):
    """x [b, n] as a view of the given dtype on `device`: "contiguous"; "ld+1" / "ld+3": row stride n + 1 / n + 3 (the rows' alignment
    changes from row to row); "offset": a column-sliced view whose every row starts ONE element past a 16-byte boundary.  What lies
    between the rows is NaN: a read past a row's end shows."""
    b, n = x.shape
    if layout == "contiguous":
        return x.to(dtype).to(device).contiguous()
    per16 = 16 // torch.empty(0, dtype=dtype).element_size()
    ld, off = {"ld+1": (n + 1, 0), "ld+3": (n + 3, 0), "offset": ((n + 1 + per16 - 1) // per16 * per16, 1)}[layout]
    buf = torch.full((b, ld), float("nan"), dtype=dtype, device=device)
    view = buf[:, off:off + n]
    view.copy_(x.to(dtype))
    assert view.stride() == (ld, 1) and view.data_ptr() % 16 == off * buf.element_size()
    return view


def project_pack_via_cabi(case, device, dtype=torch.float32, layout="contiguous", fragment_major=False, w=None, bias=None):
    """crossclr_project_pack (row-major weights) or crossclr_project_pack_wf (fragment-major, as the module passes them) on a case of
    `projection_inputs`, outputs prefilled with garbage (0x55 bytes / NaN).  `w` / `bias`: replacements (the teeth tests).
    Returns (plan, packed [2, bpad, Dpad] bf16, inv_norm [2 bpad], diag_cos [bpad]) on the CPU."""
    import ctypes
    from crossclr_amd import _native as nat
    from crossclr_amd import loss as L
    from crossclr_amd.projection import _weights_bf16
    lib = nat.library()
    b, D = case["b"], case["D"]
    plan = nat.make_plan(b, D, 1, 0, nat.MODE_BF16)
    xv, xt = (lay_out(x, dtype, layout, device) for x in case["x"])
    wv, wt = (x.to(device) for x in (w or case["w"]))
    bv, bt = (None if x is None else x.to(device).contiguous() for x in (bias or case["bias"]))
    wvb, ldw_v = _weights_bf16(wv, plan.Dpad if fragment_major else 0)
    wtb, ldw_t = _weights_bf16(wt, plan.Dpad if fragment_major else 0)
    assert plan.operand_bytes == 2 * plan.bpad * plan.Dpad * 2 and plan.b == b and plan.D == D
    xhat = torch.full((plan.operand_bytes,), 0x55, dtype=torch.uint8, device=device)
    inv = torch.full((2 * plan.bpad,), float("nan"), dtype=torch.float32, device=device)
    diag = torch.full((plan.bpad,), float("nan"), dtype=torch.float32, device=device)
    entry = lib.crossclr_project_pack_wf if fragment_major else lib.crossclr_project_pack
    nat.check(entry(ctypes.byref(plan), L._ptr(xv), L._ptr(xt), xv.stride(0), xt.stride(0), xv.shape[1], xt.shape[1], L._IN_DTYPE[dtype],
                    L._ptr(wvb), L._ptr(wtb), ldw_v, ldw_t, L._ptr(bv), L._ptr(bt), L._ptr(xhat), L._ptr(inv), L._ptr(diag), L._stream_for(xv)))
    if device != "cpu" and torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    return plan, xhat.cpu().view(torch.bfloat16).view(2, plan.bpad, plan.Dpad), inv.cpu(), diag.cpu()


def check_project_pack(case, plan, packed, inv, diag):
    """every output of crossclr_project_pack, bit for bit against the closed forms, the padding included"""
    b, D, bp = case["b"], case["D"], plan.bpad
    if "expected" not in case:
        case["expected"] = projection_expected(*case["y"])
    uv, ut, iv, it, cos = case["expected"]
    assert torch.equal(packed[0, :b, :D], uv), "packed video rows"
    assert torch.equal(packed[1, :b, :D], ut), "packed text rows"
    assert torch.equal(inv[:b], iv) and torch.equal(inv[bp:bp + b], it), "inv_norm"
    assert torch.equal(diag[:b], cos), "diag_cos"
    assert (packed[:, b:, :].float() == 0).all() and (packed[:, :, D:].float() == 0).all(), "padding of the packed operand"
    assert (inv[b:bp] == 0).all() and (inv[bp + b:] == 0).all(), "inv_norm of the padding rows"
    assert (diag[b:] == 0).all(), "diag_cos of the padding rows"


def dw_splits(b, D, din_v, din_t):
    """(nsplit, rows per split) of crossclr_project_dw (project_dw_splits, crossclr_api.cpp; rows per split: whole 32-row chunks)"""
    up = lambda x: (x + 127) // 128 * 128
    tiles_ = 2 * (up(D) // 128) * (up(max(din_v, din_t)) // 128)
    ns = max(1, min((512 + tiles_ - 1) // tiles_, max(1, b // 64), 32))
    return ns, ((b + ns - 1) // ns + 31) // 32 * 32


def dw_inputs(b, D, din_v, din_t, seed=None):
    """g_y in {-3 .. 3} 2^-7 (bf16 values, zeros included) and integer x with |x| <= 8: for b <= 520 every partial sum of g_y^T x is an
    integer multiple of 2^-7 below 2^24 of them -- exact in fp32 for every split count and summation order.  ((gyv, gyt), (xv, xt)) float32"""
    assert b * 24 < 2 ** 24
    g = torch.Generator().manual_seed(7000 + (b + D if seed is None else seed))
    gy = tuple(torch.randint(-3, 4, (b, D), generator=g).float() * 2.0 ** -7 for _ in range(2))
    x = tuple(torch.randint(-8, 9, (b, n), generator=g).float() for n in (din_v, din_t))
    return gy, x


def project_dw_via_cabi(gy, x, device, dtype=torch.float32, ld_gy=0, x_layout="contiguous", ld_dw=(0, 0), db=(True, True)):
    """crossclr_project_dw with outputs and workspace prefilled with NaN.  ld_gy / ld_dw: row strides (0 = dense); db: which bias
    gradients are asked for (False = NULL).  Returns ((dWv, dWt) as the full [D, ld_dw] buffers, (dbv | None, dbt | None)) on the CPU."""
    from crossclr_amd import _native as nat
    from crossclr_amd import loss as L
    lib = nat.library()
    b, D = gy[0].shape
    dins = (x[0].shape[1], x[1].shape[1])
    ld_gy = ld_gy or D
    gyd = []
    for t in gy:
        buf = torch.full((b, ld_gy), float("nan"), dtype=torch.bfloat16, device=device)
        buf[:, :D].copy_(t.bfloat16())
        gyd.append(buf)
    xd = [lay_out(t, dtype, x_layout, device) for t in x]
    nan32 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=device)
    ws = nan32(lib.crossclr_project_dw_ws_floats(b, D, dins[0], dins[1]))
    lds = [ld or n for ld, n in zip(ld_dw, dins)]
    dws = [nan32(D, ld) for ld in lds]
    dbs = [nan32(D) if want else None for want in db]
    nat.check(lib.crossclr_project_dw(b, D, L._ptr(gyd[0]), L._ptr(gyd[1]), ld_gy, L._ptr(xd[0]), L._ptr(xd[1]), xd[0].stride(0), xd[1].stride(0),
                                      dins[0], dins[1], L._IN_DTYPE[dtype], L._ptr(ws), L._ptr(dws[0]), L._ptr(dws[1]), lds[0], lds[1],
                                      L._ptr(dbs[0]), L._ptr(dbs[1]), L._stream_for(xd[0])))
    if xd[0].is_cuda:
        torch.cuda.synchronize()
    return tuple(t.cpu() for t in dws), tuple(None if t is None else t.cpu() for t in dbs)


def check_project_dw(gy, x, dws, dbs):
    """dW = g_y^T x and db = column sums, equal to the float64 products; the columns of dW beyond Din are untouched (NaN)"""
    for g, xx, dw, db in zip(gy, x, dws, dbs):
        din = xx.shape[1]
        assert torch.equal(dw[:, :din].double(), g.double().t() @ xx.double()), "dW"
        assert torch.isnan(dw[:, din:]).all(), "columns of dW beyond Din were written"
        if db is not None:
            assert torch.equal(db.double(), g.double().sum(0)), "db"


def projected_gy_via_impl(case, tau, w, device):
    """g_y = d loss / d (projected features) of both modalities the way projection.py obtains it: `_forward_impl(project=...)` (the fused
    crossclr_project_pack_wf), then `_backward_impl` with prenormalized = 2 on the packed bf16 unit rows.  (loss, gyv, gyt, last kernels)"""
    from crossclr_amd import _native as nat
    from crossclr_amd import loss as L
    from crossclr_amd.projection import _weights_bf16
    b, D = case["b"], case["D"]
    xv, xt = (x.to(device) for x in case["x"])
    wv, wt = (x.to(device) for x in case["w"])
    bv, bt = (None if x is None else x.to(device) for x in case["bias"])
    Dpad = L._plan_for(b, D, 1, 0, nat.MODE_BF16).Dpad
    wvb, ldw_v = _weights_bf16(wv, Dpad)
    wtb, ldw_t = _weights_bf16(wt, Dpad)
    loss, ws = L._forward_impl(xv, xt, tau, w, "bf16", None, None, None, save_for_backward=True, project=(wvb, wtb, (ldw_v, ldw_t), bv, bt, D))
    plan = ws.plan
    packed = ws.xhat.view(torch.bfloat16).view(2, plan.bpad, plan.Dpad)
    ws.in_dtype = nat.IN_BF16
    ws.prenormalized = 2
    gyv, gyt = L._backward_impl(ws, packed[0, :b, :D], packed[1, :b, :D], torch.ones((), dtype=torch.float64, device=device))
    if xv.is_cuda:
        torch.cuda.synchronize()
    lib = nat.library()
    return float(loss), gyv, gyt, (lib.crossclr_last_kernel(0).decode(), lib.crossclr_last_kernel(1).decode())


GY_CASES = [  # b, D, Din_video, Din_text, tau, w
    (70, 100, 100, 104, TAU, W), (130, 200, 256, 300, TAU, W),
    (200, 64, 64, 64, 0.01, 1.0),                               # the common shift (64 < 1 / tau <= 128)
    (300, 600, 640, 700, TAU, W), (256, 1024, 1024, 1024, TAU, W),
]
GY_BIAS = {70: (True, True), 130: (True, False), 200: (False, False), 300: (False, True), 256: (True, True)}      # by batch size

_gy_cases = {}


def gy_case(b, D, din_v, din_t):
    """the inputs of a case of GY_CASES, generated once"""
    key = (b, D, din_v, din_t)
    if key not in _gy_cases:
        _gy_cases[key] = projection_inputs(b, D, din_v, din_t, bias=GY_BIAS[b])
    return _gy_cases[key]
GY_ROUNDING = 2.0 ** -8          # the one bf16 rounding of g_y on its way out: half a unit of an 8-bit significand, relative to the element


def gy_yardstick(case, tau, w):
    """(want [2b, D] float64, bar [2b, D]) of g_y: the two-rounding weight model at (Y_v, Y_t) -- Y are sign rows, so d loss / d y is the
    input gradient of the plain loss there -- and per element 2^-8 |want| (the output's bf16 rounding) + GRAD_BAR x the row's largest
    entry (the arithmetic in front of it, the bar of the plain bf16 saved backward) + the row's tie allowance.  Also the model."""
    from oracle import crossclr_oracle as orc
    m = orc.stacked_weight_model(case["y"][0], case["y"][1], tau, w, roundings=2)
    m["grads"] = orc.grads_from_stacked_weights(m)
    want = torch.cat(m["grads"])
    bar = GY_ROUNDING * want.abs() + (GRAD_BAR["bf16", False, True] * want.abs().amax(1) + m["slack_rows"])[:, None]
    return want, bar, m


def check_gy(got, want, bar, m, what):
    """per element |got - want| <= bar; prints the worst (err - 2^-8 |want| - slack) / rowmax as a MEASURE line and returns it"""
    got = got.detach().double().cpu()
    err = (got - want).abs()
    assert not torch.isnan(err).any(), what
    rest = (err - GY_ROUNDING * want.abs() - m["slack_rows"][:, None]) / want.abs().amax(1, keepdim=True)
    worst, at = rest.flatten().max(0)
    print(f"MEASURE g_y {what}: worst (err - 2^-8 |want| - slack) / rowmax = {float(worst):.3e} @ row {int(at) // want.shape[1]} "
          f"(bar {GRAD_BAR['bf16', False, True]:.1e}); worst err / bar = {float((err / bar).max()):.3f}")
    assert (err <= bar).all(), (what, float(worst))
    return float(worst)


def check_projected_end_to_end(case, tau, w, device, what):
    """projected_crossclr_loss on a case of `projection_inputs`: the loss against the exact closed form (roundings = 0) at LOSS_BAR; dx, dW,
    db per element against the float64 chain from the model's g_y -- the yardstick of `gy_yardstick`, the two-rounding weight model at
    (Y_v, Y_t), NOT rounded to bf16 as the kernels' g_y is.  Per element of g_y the kernels may then be off by a_id = 2^-8 |g_id| (that bf16
    rounding) + GRAD_BAR rowmax_i + slack_i; a product sum_i g_id x_in is within sum_i a_id |x_in|, plus b 2^-23 sum_i |g_id| |x_in| for its
    fp32 accumulation (|W| in place of |x| for dx, 1 for db) -- all of it from the reference alone; an element whose bound is zero must be
    exact.  (The exact closed form's g_y is no yardstick here: it lacks the two bf16 roundings of the saved backward's weights, 3.4e-3 of a
    row's largest entry, which a sum over the b rows averages out and an element of dx -- one row of g_y times 8 .. 64 weights -- does not.)
    What this pins is the wiring: which W the dx GEMM multiplies with, strides, shapes, dtypes and devices of the returned gradients."""
    import crossclr_amd
    from oracle import crossclr_oracle as orc
    b, D = case["b"], case["D"]
    names = ("x_video", "x_text", "w_video", "b_video", "w_text", "b_text")
    values = (case["x"][0], case["x"][1], case["w"][0], case["bias"][0], case["w"][1], case["bias"][1])
    leaves = [None if a is None else a.clone().to(device).requires_grad_(True) for a in values]      # (a copy: the case's own tensors stay plain data)
    loss = crossclr_amd.projected_crossclr_loss(*leaves, tau, w)
    loss.backward()
    if leaves[0].is_cuda:
        torch.cuda.synchronize()
    assert loss.dtype == torch.float64 and loss.dim() == 0
    exact = orc.stacked_weight_model(case["y"][0], case["y"][1], tau, w)
    e_loss = abs(float(loss.detach()) - float(exact["loss"])) / max(1.0, abs(float(exact["loss"])))
    _, _, m = gy_yardstick(case, tau, w)
    acc = b * 2.0 ** -23
    worst = {}
    for mod, g in enumerate(m["grads"]):
        a = GY_ROUNDING * g.abs() + (GRAD_BAR["bf16", False, True] * g.abs().amax(1) + m["slack_rows"][mod * b:(mod + 1) * b])[:, None]
        x, wt = case["x"][mod].double(), case["w"][mod].double()
        want = {names[mod]: (g @ wt, a @ wt.abs() + acc * (g.abs() @ wt.abs())),
                names[2 + 2 * mod]: (g.t() @ x, a.t() @ x.abs() + acc * (g.abs().t() @ x.abs())),
                names[3 + 2 * mod]: (g.sum(0), a.sum(0) + acc * g.abs().sum(0))}
        for name, (ref, bound) in want.items():
            leaf = leaves[names.index(name)]
            if leaf is None:
                continue
            got = leaf.grad
            assert got is not None and got.dtype == leaf.dtype and got.shape == leaf.shape and got.device == leaf.device, name
            err = (got.detach().double().cpu() - ref).abs()
            assert not torch.isnan(err).any(), name
            ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
            worst[name] = float(ratio.max())
    print(f"MEASURE end to end {what}: loss {e_loss:.3e}; worst err / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert e_loss <= LOSS_BAR, what
    assert max(worst.values()) <= 1.0, (what, worst)


# crossclr_project_backward_prep against float64, per row (check_rows): 4 x the worst value measured on the unmodified kernel (host emulation
# and MI355X, the same figure: 6.04e-08), under the ceiling 1e-5
PREP_BAR = 2.4e-7
PREP_CASES = [(70, 100, 100, 104), (130, 500, 512, 500), (70, 600, 640, 700)]      # b, D, Din_video, Din_text: cases of PACK_CASES


def check_backward_prep(case, device, what):
    """crossclr_project_backward_prep on the unit rows crossclr_project_pack packed from `case`: random fp32 G with strides of its own per
    tensor, outputs prefilled with NaN, against float64 inv_norm (G - y^ (y^ . G)) from the same packed rows"""
    import ctypes
    from crossclr_amd import _native as nat
    from crossclr_amd import loss as L
    lib = nat.library()
    b, D = case["b"], case["D"]
    plan, packed, inv, _ = project_pack_via_cabi(case, device)
    g = torch.Generator().manual_seed(9000 + b + D)
    lds = (D + 3, D + 5, D + 7)                                  # ld_gv, ld_gt, ld_out
    G = [torch.randn(b, ld, generator=g) for ld in lds[:2]]
    Gd = [x.to(device) for x in G]
    outs = [torch.full((b, lds[2]), float("nan"), dtype=torch.float32, device=device) for _ in range(2)]
    xhat, invd = packed.contiguous().to(device), inv.to(device)
    nat.check(lib.crossclr_project_backward_prep(ctypes.byref(plan), L._ptr(Gd[0]), L._ptr(Gd[1]), lds[0], lds[1], L._ptr(xhat), L._ptr(invd),
                                                 L._ptr(outs[0]), L._ptr(outs[1]), lds[2], L._stream_for(xhat)))
    if xhat.is_cuda:
        torch.cuda.synchronize()
    worst = 0.0
    for mod in range(2):
        y = packed[mod, :b, :D].double()
        Gm = G[mod][:, :D].double()
        want = inv[mod * plan.bpad:mod * plan.bpad + b].double()[:, None] * (Gm - y * (y * Gm).sum(1, keepdim=True))
        out = outs[mod].cpu()
        worst = max(worst, check_rows(out[:, :D], want)[0])
        assert torch.isnan(out[:, D:]).all(), "columns beyond D were written"
    print(f"MEASURE backward_prep {what}: worst row {worst:.3e} (bar {PREP_BAR:.1e})")
    assert worst <= PREP_BAR, what
    return worst


# ----------------------------------------------------------------------------------------------------------------------------------
# The cases of crossclr_project_pack and crossclr_project_dw (tests/test_projection_exact_cpu.py, tests/test_gpu_projection_exact.py)
# ----------------------------------------------------------------------------------------------------------------------------------
F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
BOTH, NONE = (True, True), (False, False)
PACK_CASES = [  # b, D, Din_video, Din_text, Dpad, bias, dtype, layout, zero row
    # every padded width of the dispatch table (32 rows per block at these batches: bpad 128 = one ragged + one padded block, 256 alike)
    (70, 100, 100, 104, 128, BOTH, F32, "contiguous", None), (130, 200, 256, 300, 256, BOTH, F32, "contiguous", None),
    (70, 384, 384, 400, 384, (True, False), F32, "contiguous", None), (130, 500, 512, 500, 512, (False, True), F32, "contiguous", None),
    (70, 600, 640, 700, 768, BOTH, F32, "contiguous", None),                # 640 vs 700: 10 and 11 chunks
    (130, 1024, 1024, 1024, 1024, NONE, F32, "contiguous", None),
    (70, 16, 24, 24, 128, BOTH, F32, "contiguous", None),                   # Din below one 64-column chunk
    (70, 100, 104, 108, 128, BOTH, F32, "contiguous", None),                # Din no multiple of 16
    (130, 100, 101, 101, 128, BOTH, F32, "contiguous", None),               # odd Din: every other fp32 row of a block takes the element-wise loads
    (70, 64, 64, 300, 128, BOTH, F32, "contiguous", None),                  # 1 and 5 chunks
    (70, 128, 32, 32, 128, BOTH, F32, "contiguous", None),                  # Din < D
    (70, 100, 100, 104, 128, NONE, F32, "contiguous", 37),                  # an all-zero input row, no bias: the eps rule of F.normalize
    # input dtypes (Raw16Half for bf16 / fp16: 16-byte loads or element-wise, chosen per row by pointer alignment; Raw16<double>)
    (130, 200, 256, 300, 256, BOTH, BF16, "contiguous", None), (130, 200, 256, 300, 256, BOTH, F16, "contiguous", None),
    (130, 200, 256, 300, 256, BOTH, F64, "contiguous", None),
    (130, 100, 101, 101, 128, BOTH, BF16, "contiguous", None), (130, 100, 101, 101, 128, BOTH, F16, "contiguous", None),
    (70, 100, 104, 108, 128, BOTH, F64, "contiguous", None),
    # strided rows and a base pointer one element past a 16-byte boundary
    (130, 200, 256, 300, 256, BOTH, F32, "ld+1", None), (130, 200, 256, 300, 256, BOTH, F32, "ld+3", None),
    (130, 200, 256, 300, 256, BOTH, F32, "offset", None),
    (130, 200, 256, 300, 256, BOTH, BF16, "ld+1", None), (130, 200, 256, 300, 256, BOTH, BF16, "ld+3", None),
    (130, 200, 256, 300, 256, BOTH, BF16, "offset", None),
]
# 64 rows per block: bpad / 64 >= 256 and Dpad <= 512 (project_pack_t, crossclr_api.cpp).  b = 16300: bpad 16384, the last block has 44 valid
# rows; b = 16385: bpad 16512, the last block but one holds ONE valid row, the last none.
PACK_CASES_64 = [(b, D, dv, dt, Dpad, BOTH, dtype, "contiguous", None)
                 for b in (16300, 16385)
                 for D, dv, dt, Dpad in ((100, 104, 128, 128), (200, 200, 256, 256), (384, 384, 400, 384), (500, 512, 500, 512))
                 for dtype in (F32, BF16)] + \
                [(b, 200, 200, 256, 256, BOTH, F16, "contiguous", None) for b in (16300, 16385)] + \
                [(b, 100, 104, 128, 128, BOTH, F64, "contiguous", None) for b in (16300, 16385)]

_pack_inputs = {}


def pack_case(b, D, din_v, din_t, bias, zero_row):
    """the inputs of a case of PACK_CASES / PACK_CASES_64, generated once (the Gram-matrix condition only where the matrix fits)"""
    key = (b, D, din_v, din_t, bias, zero_row)
    if key not in _pack_inputs:
        _pack_inputs[key] = projection_inputs(b, D, din_v, din_t, bias=bias, zero_row=zero_row, gram=b <= 1024)
    return _pack_inputs[key]


def pack_id(c):
    return f"b{c[0]}-D{c[1]}-Din{c[2]}x{c[3]}-bias{int(c[5][0])}{int(c[5][1])}-{str(c[6]).split('.')[1]}-{c[7]}" + ("-zero-row" if c[8] is not None else "")


def run_pack_case(c, device):
    """both entry points on one case: every output bit for bit against the closed forms, and the two weight layouts give the same bytes"""
    b, D, din_v, din_t, Dpad, bias, dtype, layout, zero_row = c
    case = pack_case(b, D, din_v, din_t, bias, zero_row)
    outs = []
    for fragment_major in (False, True):
        plan, packed, inv, diag = project_pack_via_cabi(case, device, dtype, layout, fragment_major)
        assert plan.Dpad == Dpad, plan.Dpad
        check_project_pack(case, plan, packed, inv, diag)
        outs.append((packed.view(torch.int16), inv.view(torch.int32), diag[:b].view(torch.int32)))
    assert all(torch.equal(x, y) for x, y in zip(*outs)), "row-major and fragment-major weights give different bytes"
    return plan


DW_CASES = [  # b, D, Din_video, Din_text, dtype, ld_gy, x layout, ld_dw, db, (splits, rows of the last split) -- rows per split are 96 throughout
    (70, 48, 40, 100, F32, 0, "contiguous", (0, 0), BOTH, (1, 70)),                       # one split
    (130, 130, 100, 300, F32, 0, "contiguous", (0, 0), BOTH, (2, 34)),                    # a short last split; Din 100 against 300: the video
                                                                                          # blocks of the 2nd and 3rd column tile return early
    (193, 200, 64, 24, BF16, 0, "contiguous", (0, 0), BOTH, (3, 1)),                      # a last split of ONE row
    (260, 128, 128, 100, F32, 0, "contiguous", (0, 0), BOTH, (4, -28)),                   # one 128 x 128 tile per modality: the 4th split is EMPTY
    (520, 48, 100, 128, F32, 0, "contiguous", (0, 0), BOTH, (8, -152)),                   # 8 splits, the last two empty, the 6th has 40 rows
    (130, 130, 100, 300, F32, 131, "ld+3", (105, 308), NONE, (2, 34)),                    # every stride above its width, no bias gradients
    (193, 200, 100, 300, BF16, 208, "offset", (104, 0), (True, False), (3, 1)),           # one bias gradient
    (130, 130, 100, 300, F16, 0, "contiguous", (0, 0), BOTH, (2, 34)), (130, 130, 100, 300, F64, 0, "ld+1", (0, 0), BOTH, (2, 34)),
    (520, 48, 100, 300, BF16, 49, "ld+1", (0, 301), (False, True), (8, -152)),
]


def dw_id(c):
    return f"b{c[0]}-D{c[1]}-Din{c[2]}x{c[3]}-{str(c[4]).split('.')[1]}-ldgy{c[5]}-{c[6]}-lddw{c[7][0]}x{c[7][1]}-db{int(c[8][0])}{int(c[8][1])}"


def run_dw_case(c, device):
    from crossclr_amd import _native as nat
    b, D, din_v, din_t, dtype, ld_gy, layout, ld_dw, db, (ns, last) = c
    up = lambda x: (x + 127) // 128 * 128
    ws = nat.library().crossclr_project_dw_ws_floats(b, D, din_v, din_t)
    got_ns = ws // (2 * up(D) * (up(max(din_v, din_t)) + 1))
    assert (got_ns, 96) == dw_splits(b, D, din_v, din_t) and (got_ns, b - (got_ns - 1) * 96) == (ns, last), "the split geometry this case was chosen for"
    gy, x = dw_inputs(b, D, din_v, din_t)
    dws, dbs = project_dw_via_cabi(gy, x, device, dtype, ld_gy, layout, ld_dw, db)
    assert [t is None for t in dbs] == [not want for want in db]
    check_project_dw(gy, x, dws, dbs)
