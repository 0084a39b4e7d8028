"""CPU oracle for the CrossCLR "only intra-modality" contrastive loss hot path.

TEST INFRASTRUCTURE ONLY.  Nothing in the product package
(`crossmodal-contrastive-learning_amd/`) imports this file.  Only `tests/`,
`__graft_entry__.smoke()` and `bench.py`'s `cpu_baseline` leg use it, and only as
the checker / the timed CPU baseline -- never as the thing shipped.

What it restates: `/root/reference/trainer/loss.py:44-114`
(`CrossCLR_onlyIntraModality.forward`) plus the autograd backward that PyTorch
derives from it.  The reference has no tests of its own, so
parity is pinned by golden vectors generated in the build container by importing
the reference itself (`tests/golden/make_golden.py`); `tests/test_oracle.py`
checks every function here against those vectors.

Three forms:

* `eager_loss`      -- op-for-op: the same ATen op sequence as the reference,
                       including the NumPy float64 identity masks that promote
                       everything after the masking step to float64.  Verified
                       bit-identical (loss and both gradients) to the reference
                       import in the build container.  This is the function
                       `bench.py` times as the CPU baseline ("port").
* `streaming_stats` / `streaming_loss_and_grads`
                    -- closed form in float64, blocked over rows so nothing
                       O(B^2) is ever resident; usable at B=65536.  Also returns
                       the per-row intermediates (logZ, diagonal logit) that the
                       HIP kernels expose, so a failing parity test can say
                       which stage is off.
* `sharded_loss_and_grads`
                    -- the multi-GPU semantics: rank r owns rows [r*b,(r+1)*b);
                       result must equal the single-process value on the
                       concatenated batch.  Used by the gloo tests.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

NORM_EPS = 1e-12  # F.normalize default eps, reference loss.py:79-80


# --------------------------------------------------------------------------- #
# (a) op-for-op eager form                                                      #
# --------------------------------------------------------------------------- #
def _off_diagonal_mask(n: int) -> torch.Tensor:
    """float64 (1 - I_n), built through NumPy exactly like loss.py:62-66."""
    return 1 - torch.from_numpy(np.eye(n))


def _neg_log_masked_softmax(logits: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """loss.py:59-60: -log(sum_j softmax(logits)[i, j] * mask[i, j])."""
    return -torch.log((F.softmax(logits, dim=1) * mask).sum(1))


def eager_loss(video: torch.Tensor, text: torch.Tensor, temperature: float = 0.03,
               negative_weight: float = 0.8) -> torch.Tensor:
    """Same op sequence as loss.py:76-114 (device placement calls dropped).

    Returns the 0-dim float64 loss with an autograd graph attached when the
    inputs require grad, exactly like the reference on a CPU tensor.
    """
    n = video.shape[0]                                            # :76
    vhat = F.normalize(video, dim=1)                              # :79
    that = F.normalize(text, dim=1)                               # :80
    inter_v = vhat @ that.t()                                     # :83
    inter_t = that @ vhat.t()                                     # :84
    intra_v = vhat @ vhat.t()                                     # :87
    intra_t = that @ that.t()                                     # :88
    inter_v /= temperature                                        # :90
    inter_t /= temperature                                        # :91
    intra_v /= temperature                                        # :92
    intra_t /= temperature                                        # :93
    keep = _off_diagonal_mask(vhat.shape[0])                      # :95
    neg_v = intra_v * keep                                        # :96  (-> float64, diag := 0.0)
    neg_t = intra_t * keep                                        # :97
    rows_v = torch.cat([inter_v, negative_weight * neg_v], dim=1)  # :99
    rows_t = torch.cat([inter_t, negative_weight * neg_t], dim=1)  # :100
    eye_v = torch.from_numpy(np.eye(n))                           # :102-103
    eye_t = torch.from_numpy(np.eye(n))                           # :104
    tgt_v = torch.cat([eye_v, torch.zeros_like(neg_v)], dim=1)    # :106,108
    tgt_t = torch.cat([eye_t, torch.zeros_like(neg_t)], dim=1)    # :107,109
    per_v = _neg_log_masked_softmax(rows_v, tgt_v)                # :111
    per_t = _neg_log_masked_softmax(rows_t, tgt_t)                # :112
    return (per_v.mean() + per_t.mean()) / 2                      # :114


def eager_loss_and_grads(video: torch.Tensor, text: torch.Tensor, temperature: float = 0.03,
                         negative_weight: float = 0.8
                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    v = video.detach().clone().requires_grad_(True)
    t = text.detach().clone().requires_grad_(True)
    loss = eager_loss(v, t, temperature, negative_weight)
    loss.backward()
    return loss.detach(), v.grad, t.grad


# --------------------------------------------------------------------------- #
# (b) streaming float64 closed form                       #
# --------------------------------------------------------------------------- #
def _unit_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Row L2-normalisation the way loss.py:79 does it, carried out in the
    input dtype and then widened: returns (xhat float64, clamped norm float64)."""
    nrm = x.norm(dim=1, keepdim=True).clamp_min(NORM_EPS)
    return (x / nrm).double(), nrm.double().squeeze(1)


def streaming_stats(video: torch.Tensor, text: torch.Tensor, temperature: float = 0.03,
                    negative_weight: float = 0.8, block: int = 1024,
                    row_range: Optional[Tuple[int, int]] = None) -> Dict[str, torch.Tensor]:
    """Per-row statistics of the loss for rows in `row_range` against ALL columns.

        A[i,j]  = vhat_i . that_j / tau          Cv = vhat vhat^T / tau,  Ct likewise
        Zv[i]   = sum_j exp(A[i,j]) + sum_{j!=i} exp(w Cv[i,j]) + 1       (loss.py:96-100:
        Zt[i]   = sum_j exp(A[j,i]) + sum_{j!=i} exp(w Ct[i,j]) + 1        diag logit is 0, not -inf)
        loss    = mean_i(log Zv - A_ii)/2 + mean_i(log Zt - A_ii)/2       (loss.py:111-114)

    Returns float64 tensors: logZv, logZt, diag (A_ii) for the requested rows,
    `loss_sum` = sum over those rows of (logZv + logZt - 2*diag) and `loss` =
    loss_sum / (2*B) (only meaningful when row_range covers everything).
    """
    B = video.shape[0]
    lo, hi = (0, B) if row_range is None else row_range
    vhat, _ = _unit_rows(video)
    that, _ = _unit_rows(text)
    it = 1.0 / float(temperature)
    w = float(negative_weight)
    logZv = torch.empty(hi - lo, dtype=torch.float64)
    logZt = torch.empty(hi - lo, dtype=torch.float64)
    for r0 in range(lo, hi, block):
        r1 = min(hi, r0 + block)
        idx = torch.arange(r0, r1)
        rows = torch.arange(r1 - r0)
        for own, other, out in ((vhat, that, logZv), (that, vhat, logZt)):
            inter = (own[r0:r1] @ other.t()) * it               # [blk, B]
            intra = (own[r0:r1] @ own.t()) * (it * w)           # [blk, B]
            intra[rows, idx] = 0.0                               # masked diagonal -> logit 0
            out[r0 - lo:r1 - lo] = torch.logsumexp(torch.cat([inter, intra], dim=1), dim=1)
    diag = (vhat[lo:hi] * that[lo:hi]).sum(1) * it
    loss_sum = (logZv + logZt - 2.0 * diag).sum()
    return {"logZv": logZv, "logZt": logZt, "diag": diag, "loss_sum": loss_sum,
            "loss": loss_sum / (2.0 * B)}


def streaming_loss_and_grads(video: torch.Tensor, text: torch.Tensor, temperature: float = 0.03,
                             negative_weight: float = 0.8, block: int = 1024,
                             row_range: Optional[Tuple[int, int]] = None,
                             stats_all: Optional[Dict[str, torch.Tensor]] = None
                             ) -> Dict[str, torch.Tensor]:
    """Loss and d(loss)/d(inputs) in float64 from the closed form of SURVEY.md 3.5.

        GA[i,j] = (exp(A[i,j]) (1/Zv[i] + 1/Zt[j]) - 2 delta_ij) / (2B)
        Sv[i,j] = w exp(w Cv[i,j]) (1/Zv[i] + 1/Zv[j]) / (2B)   (diag 0), St likewise
        dL/dvhat = (GA that + Sv vhat)/tau      dL/dthat = (GA^T vhat + St that)/tau
        dL/dx_i  = (g_i - xhat_i (xhat_i . g_i)) / max(||x_i||, eps)

    Gradients are returned for rows in `row_range` only (exact derivative of the
    GLOBAL loss w.r.t. those rows) -- this is what each rank produces in the
    sharded scheme.  `stats_all` (full-batch logZv/logZt) may be passed in.
    """
    B = video.shape[0]
    lo, hi = (0, B) if row_range is None else row_range
    if stats_all is None:
        stats_all = streaming_stats(video, text, temperature, negative_weight, block)
    vhat, vnorm = _unit_rows(video)
    that, tnorm = _unit_rows(text)
    it = 1.0 / float(temperature)
    w = float(negative_weight)
    lzv, lzt = stats_all["logZv"], stats_all["logZt"]
    gv = torch.zeros(hi - lo, video.shape[1], dtype=torch.float64)
    gt = torch.zeros_like(gv)
    for r0 in range(lo, hi, block):
        r1 = min(hi, r0 + block)
        idx = torch.arange(r0, r1)
        rows = torch.arange(r1 - r0)
        # video rows: inter block A[r,:], intra block Cv[r,:]
        a = (vhat[r0:r1] @ that.t()) * it
        ga = torch.exp(a - lzv[r0:r1, None]) + torch.exp(a - lzt[None, :])
        cv = (vhat[r0:r1] @ vhat.t()) * (it * w)
        sv = torch.exp(cv - lzv[r0:r1, None]) + torch.exp(cv - lzv[None, :])
        sv[rows, idx] = 0.0
        gv[r0 - lo:r1 - lo] = ga @ that + w * (sv @ vhat)
        # text rows: inter block A[:,r]^T, intra block Ct[r,:]
        at = (that[r0:r1] @ vhat.t()) * it
        gat = torch.exp(at - lzt[r0:r1, None]) + torch.exp(at - lzv[None, :])
        ct = (that[r0:r1] @ that.t()) * (it * w)
        st = torch.exp(ct - lzt[r0:r1, None]) + torch.exp(ct - lzt[None, :])
        st[rows, idx] = 0.0
        gt[r0 - lo:r1 - lo] = gat @ vhat + w * (st @ that)
    scale = it / (2.0 * B)
    gv = gv * scale - that[lo:hi] * (it / B)       # analytic -2 delta_ij term
    gt = gt * scale - vhat[lo:hi] * (it / B)

    def _through_normalize(g, xhat, x, nrm):
        # normalize backward; rows with ||x|| < eps were divided by eps (no projection)
        proj = g - xhat * (xhat * g).sum(1, keepdim=True)
        tiny = (x.double().norm(dim=1) < NORM_EPS)[:, None]
        return torch.where(tiny, g, proj) / nrm[:, None]

    grad_v = _through_normalize(gv, vhat[lo:hi], video[lo:hi], vnorm[lo:hi])
    grad_t = _through_normalize(gt, that[lo:hi], text[lo:hi], tnorm[lo:hi])
    return {"loss": stats_all["loss"], "grad_v": grad_v, "grad_t": grad_t,
            "grad_vhat": gv, "grad_that": gt,
            "logZv": lzv[lo:hi], "logZt": lzt[lo:hi], "diag": stats_all["diag"][lo:hi]}


# --------------------------------------------------------------------------- #
# (c) sharded semantics                                        #
# --------------------------------------------------------------------------- #
def sharded_loss_and_grads(video: torch.Tensor, text: torch.Tensor, world: int, rank: int,
                           temperature: float = 0.03, negative_weight: float = 0.8,
                           block: int = 1024) -> Dict[str, torch.Tensor]:
    """What rank `rank` of `world` must return when the global batch (video,
    text) is row-sharded evenly: the GLOBAL loss and the exact gradient of the
    global loss w.r.t. its own rows."""
    B = video.shape[0]
    assert B % world == 0
    b = B // world
    return streaming_loss_and_grads(video, text, temperature, negative_weight, block,
                                    row_range=(rank * b, (rank + 1) * b))


# --------------------------------------------------------------------------- #
# bf16-operand model (what the bf16 MFMA path is expected to compute)          #
# --------------------------------------------------------------------------- #
def bf16_operand_model_loss(video: torch.Tensor, text: torch.Tensor, temperature: float = 0.03,
                            negative_weight: float = 0.8) -> torch.Tensor:
    """Closed-form loss with the normalised rows rounded to bf16 before the
    similarity products (products/accumulation exact in float64) and the
    diagonal logit kept in fp32 -- a numerical model of the bf16-compute /
    fp32-accumulate kernel, used to set honest tolerances for small cases."""
    vhat32 = F.normalize(video.float(), dim=1)
    that32 = F.normalize(text.float(), dim=1)
    vb = vhat32.bfloat16().double()
    tb = that32.bfloat16().double()
    it, w = 1.0 / temperature, negative_weight
    B = video.shape[0]
    a = vb @ tb.t() * it
    cv = vb @ vb.t() * (it * w)
    ct = tb @ tb.t() * (it * w)
    eye = torch.eye(B, dtype=torch.bool)
    cv[eye] = 0.0
    ct[eye] = 0.0
    lzv = torch.logsumexp(torch.cat([a, cv], 1), 1)
    lzt = torch.logsumexp(torch.cat([a.t(), ct], 1), 1)
    diag = (vhat32.double() * that32.double()).sum(1) * it
    return (lzv + lzt - 2 * diag).sum() / (2 * B)


def bf16_operand_model_loss_and_grads(video: torch.Tensor, text: torch.Tensor, temperature: float = 0.03,
                                      negative_weight: float = 0.8):
    """Loss AND input gradients of the bf16-operand model: the similarity products see the unit rows rounded to bf16, the
    gradient treats that rounding as the identity (straight-through) -- exactly what the kernels do: the backward's weights and
    its second operand are the rounded rows, the normalise-backward is exact.  The yardstick for bf16 gradients where the loss
    (and with it the float64 reference gradient) is nearly zero: aligned pairs."""
    v = video.double().clone().requires_grad_(True)
    t = text.double().clone().requires_grad_(True)
    vh, th = F.normalize(v, dim=1), F.normalize(t, dim=1)
    vb = vh + (vh.detach().float().bfloat16().double() - vh.detach())
    tb = th + (th.detach().float().bfloat16().double() - th.detach())
    it, w = 1.0 / temperature, negative_weight
    B = video.shape[0]
    a = vb @ tb.t() * it
    off = 1.0 - torch.eye(B, dtype=torch.float64)
    cv = (vb @ vb.t()) * (it * w) * off          # the masked self pair keeps logit 0 (trainer/loss.py:96-97)
    ct = (tb @ tb.t()) * (it * w) * off
    lzv = torch.logsumexp(torch.cat([a, cv], 1), 1)
    lzt = torch.logsumexp(torch.cat([a.t(), ct], 1), 1)
    diag = (vh * th).sum(1) * it                  # the positive pair's logit comes from the fp32 rows
    loss = (lzv + lzt - 2 * diag).sum() / (2 * B)
    loss.backward()
    return loss.detach(), v.grad, t.grad


def make_inputs(kind: str, B: int, D: int, seed: int, dtype: torch.dtype = torch.float32
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Deterministic synthetic inputs shared by goldens, tests and bench.

    randn   : v, t ~ N(0,1), v drawn first then t from one generator
    aligned : t = v + 0.3 n  (near-zero-loss regime; stress for bf16)
    cluster : 16 cluster centres + 0.1 noise per modality
    """
    g = torch.Generator().manual_seed(seed)
    if kind == "randn":
        v = torch.randn(B, D, generator=g)
        t = torch.randn(B, D, generator=g)
    elif kind == "aligned":
        v = torch.randn(B, D, generator=g)
        t = v + 0.3 * torch.randn(B, D, generator=g)
    elif kind == "cluster":
        c = torch.randn(16, D, generator=g)
        lab = torch.randint(0, 16, (B,), generator=g)
        v = c[lab] + 0.1 * torch.randn(B, D, generator=g)
        t = c[lab] + 0.1 * torch.randn(B, D, generator=g)
    else:
        raise ValueError(kind)
    return v.to(dtype), t.to(dtype)


# --------------------------------------------------------------------------- #
# (d) dense stacked weight model: the gradient product G = W X of the kernels  #
# --------------------------------------------------------------------------- #
LOG2E = 1.4426950408889634


def _f32(x: torch.Tensor) -> torch.Tensor:
    """round a float64 tensor to float32 and widen it again"""
    return x.float().double()


def _bf16(x: torch.Tensor) -> torch.Tensor:
    """float64 -> float32 -> bf16 (round to nearest even, as the kernels' conversion does) -> float64"""
    return x.float().bfloat16().double()


def _near_bf16_tie(x: torch.Tensor, ulps: int = 8) -> torch.Tensor:
    """where the fp32 value of x lies within `ulps` fp32 units of the midpoint of two neighbouring bf16 values"""
    low = x.float().contiguous().view(torch.int32) & 0xFFFF
    return (low - 0x8000).abs() <= ulps


_F32_LOG2E = float(torch.tensor(LOG2E).float())            # kLog2e, kLn2 of crossclr_device.h: float constants
_F32_LN2 = float(torch.tensor(0.6931471805599453).float())


def _kernel_scales(temperature: float, negative_weight: float) -> Tuple[float, float, float]:
    """(c_inter, c_intra, ln 2) as make_geo (crossclr_api.cpp) forms them: logit in log2 units = cos * c, from the float temperature and
    negative weight of the C-ABI and the float constant log2(e), rounded to fp32; back to natural units with the float constant ln 2"""
    it = 1.0 / float(torch.tensor(float(temperature)).float())
    w32 = float(torch.tensor(float(negative_weight)).float())
    return float(torch.tensor(it * _F32_LOG2E).float()), float(torch.tensor(it * w32 * _F32_LOG2E).float()), _F32_LN2


def _kernel_common_shift(temperature: float, negative_weight: float) -> float:
    """m2 of make_geo: the common soft-max shift max(0, max(1, |w|) / tau - 64) in log2 units, as a float (single-pass regime)"""
    bound = max(1.0, abs(float(torch.tensor(float(negative_weight)).float()))) / float(torch.tensor(float(temperature)).float())
    return float(torch.tensor((bound - 64.0 if bound > 64.0 else 0.0) * _F32_LOG2E).float())


def needs_row_shift(temperature: float, negative_weight: float) -> bool:
    """the two-pass soft-max regime of the kernels: max |logit| = max(1, |w|) / tau above 128"""
    return max(1.0, abs(float(negative_weight))) / float(temperature) > 128.0


def stacked_weight_model(video, text, temperature=0.03, negative_weight=0.8, k=None, omega=None, roundings: int = 0,
                         fp32_logits=False) -> Dict[str, torch.Tensor]:
    """Dense float64 form of what every backward kernel multiplies: the stacked unit rows X = [vhat; that] ([2B, D]) and the
    weight matrix W ([2B, 2B]) with

        inter-modal blocks   W_pq = E_pq (o_p / Z_p + o_q / Z_q)
        intra-modal blocks   W_pq = w E_pq (o_p k_q / Z_p + o_q k_p / Z_q),   W_pp = 0

    (k = (k_video, k_text) negative scales, omega = (o_video, o_text) loss weights; None = ones), so that
    d loss / d xhat = (W X) / (2 B tau) - the positive-pair term (`grads_from_stacked_weights`).

    roundings = 0  the exact closed form (the yardstick of the fp32 and bf16x3 modes).  fp32_logits = "scale" evaluates it with the scales
                   the kernels hold (`_kernel_scales`: the C-ABI takes the temperature as a float -- float(0.004) is 4.7e-8 above
                   0.004, 1.1e-5 of a logit of 235 --, log2(e) and ln 2 are float constants, the scale is rounded to fp32), "product"
                   also rounds every scaled logit to fp32: the two-pass regime's forward yardstick, where logZ ~ 1 / tau = 250.
    roundings = 2  the bf16 SAVED backward (crossclr_kernels_dsl.h:3, crossclr_kernels_dslp.h): the forward leaves
                   E = bf16(exp2(x - m2)) behind, x = fp32(cos * fp32(log2(e) / tau [* w])) and m2 the common shift
                   max(0, max(1, |w|) / tau - 64) log2(e); the backward forms bf16(fp32(E * fp32(rz_p + rz_q))) with rz = fp32(o / Z),
                   wrz = fp32(fp32(w) rz) on the intra-modal blocks (sample weights: fp32(fma(rz_p, k_q, rz_q k_p))), Z from the
                   UNROUNDED exponentials.  Two bf16 roundings per weight; the product with X and the normalise-backward are exact.
    roundings = 1  the bf16 RECOMPUTING backward (fast_bwd_kernel / fast_bwd16_kernel, crossclr_kernels_fast.h): the same
                   expression from the fp32 exponential: one bf16 rounding per weight.
    The rounded forms mirror the kernels' fp32 operations, so a weight falls on the other side of a bf16 tie only where the
    hardware's exp2 does (`slack_rows`: what that may move a row's gradient by).
    Two-pass regime (max(1, |w|) / tau > 128), roundings = 2 (crossclr_backward_saved_s, crossclr_api.cpp): the second pass of the
    forward leaves U[p][q] = bf16(exp2(fma(cos, c, -shift_p))) behind, shift_p = the row maximum of fp32(cos c) over the unmasked
    columns; the backward is two launches of the saved kernel, direct and transposed, each rounding its own weight:
    W_pq = bf16(fp32(U[p][q] fp32(rz_p k_q))) + bf16(fp32(U[q][p] fp32(rz_q k_p))), rz = fp32(o / sum_q exp2(x - shift_p)).
    The dict also carries the pieces (`logits`, `k_cols`, `k_rows`, `intra`, `w`) from which `exact_weights` forms W, for tests that
    perturb a statistic."""
    B = video.shape[0]
    vhat, vnorm = _unit_rows(video)
    that, tnorm = _unit_rows(text)
    X = torch.cat([vhat, that], 0)
    n = 2 * B
    it, w = 1.0 / float(temperature), float(negative_weight)
    two_pass = needs_row_shift(temperature, negative_weight)
    if roundings == 1 and two_pass:
        raise NotImplementedError("the one-rounding model covers the single-pass regime (the two-pass bf16 step saves)")
    ones = torch.ones(B, dtype=torch.float64)
    kk = torch.cat([x.double() for x in (k if k is not None else (ones, ones))])
    om = torch.cat([x.double() for x in (omega if omega is not None else (ones, ones))])
    mod = torch.arange(n) >= B
    intra = mod[:, None] == mod[None, :]
    eye = torch.eye(n, dtype=torch.bool)
    f64 = lambda a, b: torch.where(intra, torch.tensor(a, dtype=torch.float64), torch.tensor(b, dtype=torch.float64))
    S = X @ X.t()
    c_inter, c_intra, ln2 = _kernel_scales(temperature, negative_weight)
    kq = torch.where(intra, kk[None, :], torch.ones(n, n, dtype=torch.float64))      # the column's negative scale (intra-modal blocks)
    kr = torch.where(intra, kk[:, None], torch.ones(n, n, dtype=torch.float64))      # the row's
    slack = torch.zeros(n, dtype=torch.float64)
    logits = None
    if not roundings:
        logits = S * f64(it * w, it)
        if fp32_logits:
            x2 = S * f64(c_intra, c_inter)
            logits = (_f32(x2) if fp32_logits == "product" else x2) * ln2
        logits[eye] = 0.0
        lk = torch.where(kk > 0, torch.log(kk.clamp_min(1e-300)), torch.full_like(kk, float("-inf")))
        logZ = torch.logsumexp(logits + torch.where(intra, lk[None, :], torch.zeros_like(logits)), 1)
        W = exact_weights(logits, logZ, logZ, om, om, kq, kr, intra, w)
    else:
        if two_pass:
            # pass 1: the row maximum of the rounded scaled logits over the unmasked columns; pass 2: exp2(fma(cos, c, -shift_p))
            xs = _f32(_f32(S) * f64(c_intra, c_inter))
            live = ~eye & (~intra | (kk[None, :] > 0))
            shift = torch.where(live, xs, torch.full_like(xs, float("-inf"))).amax(1)
        else:
            shift = torch.full((n,), _kernel_common_shift(temperature, negative_weight), dtype=torch.float64)
        x2 = _f32(_f32(S) * f64(c_intra, c_inter) - shift[:, None])
        x2[eye] = -shift                                # the masked self pair: logit 0
        E = _f32(torch.exp2(x2))
        Zs = (E * kq).sum(1)
        logZ = shift * ln2 + torch.log(Zs)
        rz = _f32(om / Zs)
        wrz = _f32(float(torch.tensor(w).float()) * rz)
        U = _bf16(E) if roundings == 2 else E
        rs = torch.where(intra, wrz[:, None], rz[:, None]).expand(n, n)
        cs = torch.where(intra, wrz[None, :], rz[None, :]).expand(n, n)
        # What this model lacks: the last place of the hardware's exp2 (accurate to a unit of fp32, not correctly rounded).  A weight whose
        # fp32 value -- or whose saved exponential's -- lies within 8 fp32 units of a bf16 rounding boundary may fall on either side of it on
        # the device: such a weight (about one in 4000) is allowed two bf16 steps, and its row the resulting `slack_rows`.
        tie_e = _near_bf16_tie(E) if roundings == 2 else torch.zeros_like(eye)
        if two_pass:
            # two launches, each weight rounded on its own: bf16(U[p][q] rz_p k_q) + bf16(U[q][p] rz_q k_p)
            pre1, pre2 = _f32(U * _f32(rs * kq)), _f32(U.t() * _f32(cs * kr))
            W = _bf16(pre1) + _bf16(pre2)
            allow = (torch.where(_near_bf16_tie(pre1) | tie_e, _bf16(pre1).abs(), torch.zeros_like(W)) +
                     torch.where(_near_bf16_tie(pre2) | tie_e.t(), _bf16(pre2).abs(), torch.zeros_like(W))) * 2.0 ** -6
        else:
            pre = _f32(U * _f32(rs * kq + cs * kr))
            W = _bf16(pre)
            allow = torch.where(_near_bf16_tie(pre) | tie_e, W.abs() * 2.0 ** -6, torch.zeros_like(W))
        slack = 2.0 * (allow.masked_fill(eye, 0.0) @ X.abs().amax(1)) / (float(temperature) * n) / torch.cat([vnorm, tnorm])
    W = W.masked_fill(eye, 0.0)
    diag = (vhat * that).sum(1) * it
    loss = (om[:B] * (logZ[:B] - diag) + om[B:] * (logZ[B:] - diag)).sum() / n
    return {"W": W, "X": X, "slack_rows": slack, "logZv": logZ[:B], "logZt": logZ[B:], "diag": diag, "loss": loss, "omega": om,
            "logits": logits, "k_cols": kq, "k_rows": kr, "intra": intra, "w": w,
            "norms": torch.cat([vnorm, tnorm]), "tau": torch.tensor(float(temperature), dtype=torch.float64),
            "tiny": torch.cat([video.double().norm(dim=1), text.double().norm(dim=1)]) < NORM_EPS}


def exact_weights(logits, logz_rows, logz_cols, om_rows, om_cols, k_cols, k_rows, intra, w) -> torch.Tensor:
    """W_pq = c (exp(l_pq - logZ_p) o_p k_q + exp(l_pq - logZ_q) o_q k_p), c = w on the intra-modal blocks and 1 elsewhere, from the row
    statistics (logz_rows, om_rows: indexed by p) and the column statistics (logz_cols, om_cols: by q).  Every exponential is relative to
    a denominator of its own: nothing overflows at any temperature."""
    c = torch.where(intra, torch.tensor(float(w), dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64))
    return c * (torch.exp(logits - logz_rows[:, None]) * om_rows[:, None] * k_cols + torch.exp(logits - logz_cols[None, :]) * om_cols[None, :] * k_rows)


def grads_from_stacked_weights(model: Dict[str, torch.Tensor], W: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(grad_video, grad_text) in float64 from a `stacked_weight_model` (optionally with a modified W): the product W X, the
    positive-pair term and the normalise-backward, all exact."""
    X, om = model["X"], model["omega"]
    W = model["W"] if W is None else W
    B = X.shape[0] // 2
    scale = 1.0 / (float(model["tau"]) * 2.0 * B)
    G = (W @ X) * scale
    pos = ((om[:B] + om[B:]) * scale)[:, None]
    G[:B] -= X[B:] * pos
    G[B:] -= X[:B] * pos
    proj = G - X * (X * G).sum(1, keepdim=True)
    g = torch.where(model["tiny"][:, None], G, proj) / model["norms"][:, None]
    return g[:B], g[B:]


def bf16_weight_model_grads(video, text, temperature=0.03, negative_weight=0.8, k=None, omega=None, saved: bool = True
                            ) -> Dict[str, torch.Tensor]:
    """What a correct bf16 backward returns for operands bf16 holds exactly: the two-rounding weight model of the saved backward
    (saved=False: the one-rounding model of the recomputing kernels); see `stacked_weight_model`."""
    m = stacked_weight_model(video, text, temperature, negative_weight, k, omega, roundings=2 if saved else 1)
    gv, gt = grads_from_stacked_weights(m)
    return {"loss": m["loss"], "grad_v": gv, "grad_t": gt, "logZv": m["logZv"], "logZt": m["logZt"], "diag": m["diag"]}
