"""Pairwise sigmoid loss (SigLIP) with a learnable logit scale and logit bias.

    z = s S + beta,  S = v^ . t^T,   L = 1/B [ sum_i softplus(-z_ii) + sum_{i != j} softplus(z_ij) ]

Every (video, text) pair is a binary problem of its own, positive on the diagonal and negative elsewhere.  On the tiled-similarity
skeleton: one pass with a softplus / sigmoid epilogue (`crossclr_sigmoid_stats`, `crossclr_sigmoid_finish`), the three-phase gradient
product with W = sigma(z) - I (`crossclr_sigmoid_backward`) and a row finish that also yields dL/ds (`crossclr_sigmoid_backward_finish`);
dL/dbeta = 1/B sum_ij W_ij comes out of the forward.  Neither z, sigma(z) nor their gradients are materialised (eager PyTorch holds five
B x B tensors), and the loss is available in compute_mode="bf16x3".

The scale and the bias live in DEVICE memory from end to end: the kernels read one fp32 each, nothing here calls `.item()` or
`float(tensor)`, so a captured graph replays with whatever the two tensors hold then, and an optimiser can step them without a host
round trip.

`pair_ids` (optional, [B] int32 / int64 on the inputs' device): the item each pair belongs to.  An entry (i, j), i != j, with
pair_ids[i] == pair_ids[j] is EXCLUDED from the negatives: its softplus(z_ij) leaves the loss and row_loss[i], its weight is 0 (so it is
in neither dL/ds nor dL/dbeta); it is not an additional positive, and the divisor stays B.  The B x B mask is never formed and the ids'
values stay on the device (`crossclr_pair_groups`, see crossclr_amd/infonce.py).
"""
from __future__ import annotations

import ctypes
import math

import torch
from torch import nn

from . import _native as nat
from .infonce import _checked_pair_ids, _gradient_finish, _lay_out, _pair_groups, _refuse_auto, _scalar
from .loss import _device_of, _plan_for, _ptr, _refuse_double_backward, _resolve_mode, _row_major, _stream_for
from .ranking import _check


class _SigmoidFunction(torch.autograd.Function):
    """Saved for backward: the caller's tensors, the packed operand, inv_norm, the one-element fp32 scale and bias, dL/dbeta (one
    double) and, with pair_ids, group [bpad].  Outputs: the loss and, not differentiable, row_loss [bpad] and the positive pairs' scores
    [bpad]."""

    @staticmethod
    def forward(ctx, video, text, scale, bias, normalize, mode, splits, pair_ids=None):
        v_c, t_c = _row_major(video.detach()), _row_major(text.detach())
        lib = nat.library()
        b, D = v_c.shape
        dev = v_c.device
        plan = _plan_for(b, D, 1, 0, mode)
        pp = ctypes.byref(plan)
        f32 = dict(dtype=torch.float32, device=dev)
        with _device_of(v_c):
            stream = _stream_for(v_c)
            scale32 = scale.detach().reshape(1).to(torch.float32)      # (device ops: the values stay where they are)
            bias32 = bias.detach().reshape(1).to(torch.float32)
            in_dtype, xhat, inv_norm = _lay_out(plan, v_c, t_c, normalize, stream)
            ws = torch.empty(lib.crossclr_sigmoid_workspace_bytes(pp, splits), dtype=torch.uint8, device=dev)
            group = None if pair_ids is None else _pair_groups(pair_ids, plan, stream)      # once: the backward reads the same array
            if group is None:
                nat.check(lib.crossclr_sigmoid_stats(pp, _ptr(xhat), _ptr(scale32), _ptr(bias32), splits, _ptr(ws), ws.numel(), stream))
            else:
                nat.check(lib.crossclr_sigmoid_stats_ids(pp, _ptr(xhat), _ptr(scale32), _ptr(bias32), _ptr(group), splits, _ptr(ws),
                                                         ws.numel(), stream))
            row_loss, pair = torch.empty(plan.bpad, **f32), torch.empty(plan.bpad, **f32)
            loss_sum = torch.empty(plan.loss_ws_doubles, dtype=torch.float64, device=dev)
            sig_sum = torch.empty(plan.loss_ws_doubles, dtype=torch.float64, device=dev)
            nat.check(lib.crossclr_sigmoid_finish(pp, _ptr(ws), splits, _ptr(scale32), _ptr(bias32), _ptr(row_loss), _ptr(pair),
                                                  _ptr(loss_sum), _ptr(sig_sum), stream))
            loss = loss_sum[1].to(torch.float64 if video.dtype == torch.float64 else torch.float32)
            dbias = sig_sum[1].clone()
        ctx.plan, ctx.in_dtype, ctx.normalize = plan, in_dtype, normalize
        ctx.scale_meta, ctx.bias_meta = (scale.shape, scale.dtype), (bias.shape, bias.dtype)
        ctx.save_for_backward(v_c, t_c, xhat, inv_norm, scale32, bias32, dbias, group)
        ctx.mark_non_differentiable(row_loss, pair)
        return loss, row_loss, pair

    @staticmethod
    def backward(ctx, grad_out, _grad_row_loss, _grad_pair):
        _refuse_double_backward("sigmoid_loss")
        v_c, t_c, xhat, inv_norm, scale32, bias32, dbias, group = ctx.saved_tensors
        lib, plan, dev = nat.library(), ctx.plan, v_c.device
        pp = ctypes.byref(plan)
        need = ctx.needs_input_grad
        g_v = g_t = g_s = g_b = None
        with _device_of(v_c):
            go = grad_out.detach().to(device=dev, dtype=torch.float64).reshape(1).contiguous()
            if need[0] or need[1] or need[2]:
                stream = _stream_for(v_c)
                gbuf = torch.empty(plan.gbuf_bytes // 4, dtype=torch.float32, device=dev)
                if group is None:
                    nat.check(lib.crossclr_sigmoid_backward(pp, _ptr(xhat), _ptr(scale32), _ptr(bias32), _ptr(gbuf), stream))
                else:
                    nat.check(lib.crossclr_sigmoid_backward_ids(pp, _ptr(xhat), _ptr(scale32), _ptr(bias32), _ptr(group), _ptr(gbuf), stream))
                g_v, g_t, dscale = _gradient_finish(lib.crossclr_sigmoid_backward_finish, ctx, gbuf, v_c, t_c, inv_norm, scale32, go, stream)
                if need[2]:
                    shape, dtype = ctx.scale_meta
                    g_s = dscale[1].reshape(shape).to(dtype)
            if need[3]:
                shape, dtype = ctx.bias_meta
                g_b = (go[0] * dbias).reshape(shape).to(dtype)
        return g_v, g_t, g_s, g_b, None, None, None, None


def _sigmoid(video: torch.Tensor, text: torch.Tensor, logit_scale, logit_bias, normalize: bool, compute_mode: str, splits: int = 0,
             pair_ids=None):
    """`sigmoid_loss` with the number of column splits exposed (0 = the library's choice); returns (loss, row_loss [bpad] in nats -- row
    i's share of B L, 0 for padding entries --, pair_score [bpad])."""
    _check(video, text)
    pair_ids = _checked_pair_ids(pair_ids, video)
    _refuse_auto("sigmoid_loss", compute_mode)
    mode = _resolve_mode(compute_mode, video.shape[0], video.dtype)
    scale, bias = _scalar(logit_scale, "logit_scale", video), _scalar(logit_bias, "logit_bias", video)
    return _SigmoidFunction.apply(video, text, scale, bias, bool(normalize), mode, int(splits), pair_ids)


def sigmoid_loss(video_features: torch.Tensor, text_features: torch.Tensor, logit_scale=10.0, logit_bias=-10.0, *, normalize: bool = True,
                 compute_mode: str = "fp32", pair_ids=None) -> torch.Tensor:
    """Pairwise sigmoid loss: 1/B [sum_i softplus(-z_ii) + sum_{i != j} softplus(z_ij)], z = s S + beta over S = v^ . t^T
    (normalize=True: cosines, rows L2-normalised like `F.normalize`; normalize=False: rows as given), 0-dim, float32 (float64 for
    float64 inputs).

    logit_scale `s` and logit_bias `beta`: each a Python float (a constant) or a one-element float tensor on the inputs' device, which
    may require grad -- its gradient comes back in its dtype and shape.  Neither value is ever brought to the host.  Any finite values
    are valid, 0 and negative ones included.  Gradients of the inputs come in their dtype; only those `requires_grad` asks for are formed.
    compute_mode: "fp32" (default: exact-fp32 products), "bf16x3" (fp32-grade products on the bf16 matrix cores) or "bf16" (opt-in:
    a bf16 cosine error of 2^-9 is multiplied by s in the logit); "auto" raises ValueError.  Single device; double backward raises.
    pair_ids: None (every off-diagonal pair is a negative) or a [B] int32 / int64 tensor on the inputs' device, the item pair i belongs
    to (any int64 value, all 64 bits compared).  An entry (i, j), i != j, with equal ids is EXCLUDED from the negatives -- out of the
    loss, weight 0; it is not treated as a positive, and the divisor stays B.  The ids are not differentiated and never brought to the
    host; a wrong shape, dtype or device raises RuntimeError."""
    return _sigmoid(video_features, text_features, logit_scale, logit_bias, normalize, compute_mode, 0, pair_ids)[0]


class SigmoidLoss(nn.Module):
    """`sigmoid_loss` with SigLIP's parameterisation: `logit_scale` holds log(init_logit_scale) and `logit_bias` holds init_logit_bias --
    `nn.Parameter`s when `learnable`, buffers otherwise, the `state_dict` keys either way -- and the forward uses exp(logit_scale)
    clamped at `max_logit_scale` and logit_bias, as torch ops on the 0-dim device tensors, so autograd chains through them.  `forward`
    takes the optional `pair_ids` of `sigmoid_loss` (same-item pairs are excluded from the negatives)."""

    def __init__(self, init_logit_scale: float = 10.0, init_logit_bias: float = -10.0, *, learnable: bool = True,
                 max_logit_scale: float = 100.0, normalize: bool = True, compute_mode: str = "fp32"):
        super().__init__()
        if not init_logit_scale > 0:
            raise ValueError(f"init_logit_scale must be positive, got {init_logit_scale}")
        scale = torch.tensor(math.log(init_logit_scale), dtype=torch.float32)
        bias = torch.tensor(float(init_logit_bias), dtype=torch.float32)
        if learnable:
            self.logit_scale = nn.Parameter(scale)
            self.logit_bias = nn.Parameter(bias)
        else:
            self.register_buffer("logit_scale", scale)
            self.register_buffer("logit_bias", bias)
        self.learnable = learnable
        self.max_logit_scale = max_logit_scale
        self.normalize = normalize
        self.compute_mode = compute_mode

    def forward(self, video_features, text_features, pair_ids=None):
        scale = self.logit_scale.exp().clamp(max=self.max_logit_scale)
        return sigmoid_loss(video_features, text_features, scale, self.logit_bias, normalize=self.normalize,
                            compute_mode=self.compute_mode, pair_ids=pair_ids)

    def extra_repr(self):
        return (f"learnable={self.learnable}, max_logit_scale={self.max_logit_scale}, normalize={self.normalize}, "
                f"compute_mode={self.compute_mode!r}")
