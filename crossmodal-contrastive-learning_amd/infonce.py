"""Symmetric InfoNCE (CLIP) loss with a learnable logit scale.

    L = 1/2 [ CE(s S, diag) + CE(s S^T, diag) ],   S = v^ . t^T

The reference class carries the leftovers of this loss -- `logit_scale = nn.Parameter(torch.ones([]))` and a
`CrossEntropyLoss(reduction='none')` child that its forward never reads; here it is a loss of its own, on the
tiled-similarity skeleton: one pass with an online soft-max in both directions (`crossclr_infonce_stats`, `crossclr_infonce_finish`), the
three-phase gradient product (`crossclr_infonce_backward`) and a row finish that also yields dL/ds (`crossclr_infonce_backward_finish`).
Neither s S, the two soft-max outputs nor their gradients are materialised (eager PyTorch holds five B x B tensors), and the loss is
available in compute_mode="bf16x3": fp32-grade logits on the bf16 matrix cores, which matters at s = 100, where a bf16 cosine error of 2^-9
is 0.2 in the logit.

The scale lives in DEVICE memory from end to end: the kernels read one fp32, nothing here calls `.item()` or `float(tensor)`, so a
captured graph replays with whatever value the scale tensor holds then, and an optimiser can step it without a host round trip.

`pair_ids` (optional, [B] int32 / int64 on the inputs' device): the item each pair belongs to.  Video-text sets hold several pairs of one
item (20 captions per MSR-VTT video), and a batch that draws two of them scores a caption against the video it describes as a negative.
An entry (i, j), i != j, with pair_ids[i] == pair_ids[j] is EXCLUDED: it leaves row i's and column j's soft-max and carries weight 0; it
is not an additional positive, and the divisor stays 2 B.  The B x B mask is never formed -- `crossclr_pair_groups` turns the ids into one
int32 per pair and the tiled epilogues compare those -- and the ids' values stay on the device like the scale's.
"""
from __future__ import annotations

import ctypes
import math

import torch
from torch import nn

from . import _native as nat
from .loss import _IN_DTYPE, _device_of, _plan_for, _ptr, _refuse_double_backward, _resolve_mode, _row_major, _stream_for
from .ranking import _check


def _checked_pair_ids(pair_ids, like: torch.Tensor):
    """None, or the ids as handed in after the argument checks (shape [B], int32 / int64, the inputs' device, no grad)"""
    if pair_ids is None:
        return None
    if not isinstance(pair_ids, torch.Tensor):
        raise RuntimeError(f"pair_ids must be None or an integer tensor of shape [{like.shape[0]}], got {type(pair_ids).__name__}")
    if pair_ids.requires_grad:
        raise RuntimeError("pair_ids requires_grad: ids are labels, nothing is differentiated with respect to them")
    if pair_ids.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f"pair_ids must be an integer tensor (int32 or int64), got dtype {pair_ids.dtype}")
    if pair_ids.dim() != 1 or pair_ids.shape[0] != like.shape[0]:
        raise RuntimeError(f"pair_ids must have shape [{like.shape[0]}] (one id per pair), got shape {tuple(pair_ids.shape)}")
    if pair_ids.device != like.device:
        raise RuntimeError(f"pair_ids is on {pair_ids.device}, the inputs are on {like.device}")
    return pair_ids


def _pair_groups(pair_ids: torch.Tensor, plan, stream) -> torch.Tensor:
    """ids [B] -> group [bpad] int32 (crossclr_pair_groups): what the _ids kernels compare.  Device ops only: the values stay where they are."""
    ids64 = pair_ids.detach().to(torch.int64).contiguous()
    group = torch.empty(plan.bpad, dtype=torch.int32, device=ids64.device)
    nat.check(nat.library().crossclr_pair_groups(ctypes.byref(plan), _ptr(ids64), _ptr(group), stream))
    return group


def _lay_out(plan, video: torch.Tensor, text: torch.Tensor, normalize: bool, stream):
    """The packed operand of both rows (crossclr_normalize, or crossclr_pack for rows taken as given) -> in_dtype, xhat, inv_norm [2 bpad]"""
    lib = nat.library()
    f32 = dict(dtype=torch.float32, device=video.device)
    in_dtype = _IN_DTYPE[video.dtype]
    xhat = torch.empty(plan.operand_bytes, dtype=torch.uint8, device=video.device)
    inv_norm, pair_cos = torch.empty(2 * plan.bpad, **f32), torch.empty(plan.bpad, **f32)
    lay_out = lib.crossclr_normalize if normalize else lib.crossclr_pack
    nat.check(lay_out(ctypes.byref(plan), _ptr(video), _ptr(text), video.stride(0), text.stride(0), in_dtype, _ptr(xhat), _ptr(inv_norm),
                      _ptr(pair_cos), stream))
    return in_dtype, xhat, inv_norm


def _scalar(value, name: str, like: torch.Tensor) -> torch.Tensor:
    """a float -> a one-element fp32 tensor on the inputs' device; a tensor is checked and handed on"""
    if isinstance(value, torch.Tensor):
        if value.numel() != 1 or not value.is_floating_point():
            raise RuntimeError(f"{name} must be a float or a one-element float tensor, got shape {tuple(value.shape)} "
                               f"and dtype {value.dtype}")
        if value.device != like.device:
            raise RuntimeError(f"{name} is on {value.device}, the inputs are on {like.device}")
        return value
    return torch.full((1,), float(value), dtype=torch.float32, device=like.device)


def _refuse_auto(what: str, compute_mode: str) -> None:
    if compute_mode == "auto":
        raise ValueError(f"{what}: compute_mode='auto' is not offered (at a logit scale of 100 bf16 operands have no a-priori error "
                         "bar); pass 'fp32', 'bf16x3' or 'bf16'")


def _gradient_finish(finish, ctx, gbuf, v_c, t_c, inv_norm, scale32, go, stream):
    """The row finish of a gradient product (`finish`: crossclr_infonce_backward_finish or crossclr_sigmoid_backward_finish) ->
    (g_v, g_t, dscale): the input gradients ctx.needs_input_grad asks for (else None) and dscale [loss_ws_doubles], [1] = grad_out dL/ds"""
    need, plan = ctx.needs_input_grad, ctx.plan
    g_v = torch.empty_like(v_c) if need[0] else None
    g_t = torch.empty_like(t_c) if need[1] else None
    dscale = torch.empty(plan.loss_ws_doubles, dtype=torch.float64, device=v_c.device)
    nat.check(finish(ctypes.byref(plan), _ptr(gbuf), _ptr(v_c), _ptr(t_c), v_c.stride(0), t_c.stride(0), ctx.in_dtype, _ptr(inv_norm),
                     int(ctx.normalize), _ptr(scale32), _ptr(go), _ptr(g_v), _ptr(g_t), 0 if g_v is None else g_v.stride(0),
                     0 if g_t is None else g_t.stride(0), _ptr(dscale), stream))
    return g_v, g_t, dscale


class _Stats:
    __slots__ = ("plan", "in_dtype", "xhat", "inv_norm", "lse", "pair", "loss_sum", "group")


def _stats(video: torch.Tensor, text: torch.Tensor, scale32: torch.Tensor, mode: int, normalize: bool, splits: int = 0,
           pair_ids=None) -> _Stats:
    """Lay out + statistics + finish: lse [2, 2 bpad] (log2 domain, an fp32 value and its rounding's remainder; video rows, then text
    columns), pair [bpad] = S[i][i] and the loss.
    `splits` (0 = the library's choice) cuts the launch.  pair_ids: group [bpad] is made here, once, and kept for the backward."""
    lib = nat.library()
    b, D = video.shape
    dev = video.device
    plan = _plan_for(b, D, 1, 0, mode)
    pp = ctypes.byref(plan)
    stream = _stream_for(video)
    f32 = dict(dtype=torch.float32, device=dev)
    st = _Stats()
    st.plan = plan
    st.in_dtype, st.xhat, st.inv_norm = _lay_out(plan, video, text, normalize, stream)
    ws = torch.empty(lib.crossclr_infonce_workspace_bytes(pp, splits), dtype=torch.uint8, device=dev)
    st.group = None if pair_ids is None else _pair_groups(pair_ids, plan, stream)
    if st.group is None:
        nat.check(lib.crossclr_infonce_stats(pp, _ptr(st.xhat), _ptr(scale32), splits, _ptr(ws), ws.numel(), stream))
    else:
        nat.check(lib.crossclr_infonce_stats_ids(pp, _ptr(st.xhat), _ptr(scale32), _ptr(st.group), splits, _ptr(ws), ws.numel(), stream))
    st.lse, st.pair = torch.empty(4 * plan.bpad, **f32), torch.empty(plan.bpad, **f32)
    st.loss_sum = torch.empty(plan.loss_ws_doubles, dtype=torch.float64, device=dev)
    nat.check(lib.crossclr_infonce_finish(pp, _ptr(ws), splits, _ptr(scale32), _ptr(st.lse), _ptr(st.pair), _ptr(st.loss_sum), stream))
    return st


class _InfoNCEFunction(torch.autograd.Function):
    """Saved for backward: the caller's tensors, the packed operand, inv_norm, lse [4 bpad], pair [bpad], the one-element fp32 scale and,
    with pair_ids, group [bpad].  Outputs: the loss and, not differentiable, lse and the positive pairs' scores."""

    @staticmethod
    def forward(ctx, video, text, scale, normalize, mode, splits, pair_ids=None):
        v_c, t_c = _row_major(video.detach()), _row_major(text.detach())
        with _device_of(v_c):
            scale32 = scale.detach().reshape(1).to(torch.float32)      # (a device op: the value stays where it is)
            st = _stats(v_c, t_c, scale32, mode, normalize, splits, pair_ids)
        ctx.plan, ctx.in_dtype, ctx.normalize = st.plan, st.in_dtype, normalize
        ctx.scale_meta = (scale.shape, scale.dtype)
        ctx.save_for_backward(v_c, t_c, st.xhat, st.inv_norm, st.lse, st.pair, scale32, st.group)
        ctx.mark_non_differentiable(st.lse, st.pair)
        return st.loss_sum[1].to(torch.float64 if video.dtype == torch.float64 else torch.float32), st.lse, st.pair

    @staticmethod
    def backward(ctx, grad_out, _grad_lse, _grad_pair):
        _refuse_double_backward("InfoNCE")
        v_c, t_c, xhat, inv_norm, lse, pair, scale32, group = ctx.saved_tensors
        lib, plan, dev = nat.library(), ctx.plan, v_c.device
        pp = ctypes.byref(plan)
        with _device_of(v_c):
            stream = _stream_for(v_c)
            gbuf = torch.empty(plan.gbuf_bytes // 4, dtype=torch.float32, device=dev)
            if group is None:
                nat.check(lib.crossclr_infonce_backward(pp, _ptr(xhat), _ptr(scale32), _ptr(lse), _ptr(pair), _ptr(gbuf), stream))
            else:
                nat.check(lib.crossclr_infonce_backward_ids(pp, _ptr(xhat), _ptr(scale32), _ptr(lse), _ptr(pair), _ptr(group), _ptr(gbuf),
                                                            stream))
            go = grad_out.detach().to(device=dev, dtype=torch.float64).reshape(1).contiguous()
            g_v, g_t, dscale = _gradient_finish(lib.crossclr_infonce_backward_finish, ctx, gbuf, v_c, t_c, inv_norm, scale32, go, stream)
            g_s = None
            if ctx.needs_input_grad[2]:
                shape, dtype = ctx.scale_meta
                g_s = dscale[1].reshape(shape).to(dtype)
        return g_v, g_t, g_s, None, None, None, None


def _info_nce(video: torch.Tensor, text: torch.Tensor, logit_scale, normalize: bool, compute_mode: str, splits: int = 0, pair_ids=None):
    """`info_nce_loss` with the number of column splits exposed (0 = the library's choice); returns (loss, lse [2, 2 bpad] in the log2
    domain (value, remainder), pair_score [bpad])."""
    _check(video, text)
    pair_ids = _checked_pair_ids(pair_ids, video)
    _refuse_auto("info_nce_loss", compute_mode)
    mode = _resolve_mode(compute_mode, video.shape[0], video.dtype)
    scale = _scalar(logit_scale, "logit_scale", video)
    return _InfoNCEFunction.apply(video, text, scale, bool(normalize), mode, int(splits), pair_ids)


def info_nce_loss(video_features: torch.Tensor, text_features: torch.Tensor, logit_scale=1 / 0.07, *, normalize: bool = True,
                  compute_mode: str = "fp32", pair_ids=None) -> torch.Tensor:
    """Symmetric InfoNCE: 1/2 [CE(s S, diag) + CE(s S^T, diag)] over S = v^ . t^T (normalize=True: cosines, rows L2-normalised like
    `F.normalize`; normalize=False: rows as given), 0-dim, float32 (float64 for float64 inputs).

    logit_scale `s`: a Python float (a constant) or a one-element float tensor on the inputs' device, which may require grad -- its
    gradient comes back in its dtype and shape.  The value is never brought to the host.  Any finite scale is valid, 0 and negative
    values included.  Gradients of the inputs come in their dtype; only those `requires_grad` asks for are formed.
    compute_mode: "fp32" (default: exact-fp32 products), "bf16x3" (fp32-grade products on the bf16 matrix cores) or "bf16" (opt-in:
    a bf16 cosine error of 2^-9 is multiplied by s in the logit); "auto" raises ValueError.  Single device; double backward raises.
    pair_ids: None (every off-diagonal pair is a negative) or a [B] int32 / int64 tensor on the inputs' device, the item pair i belongs
    to (any int64 value, all 64 bits compared).  An entry (i, j), i != j, with equal ids is EXCLUDED -- out of row i's and column j's
    soft-max, weight 0; it is not treated as a positive, and the divisor stays 2 B.  The ids are not differentiated and never brought
    to the host; a wrong shape, dtype or device raises RuntimeError."""
    return _info_nce(video_features, text_features, logit_scale, normalize, compute_mode, 0, pair_ids)[0]


class InfoNCE(nn.Module):
    """`info_nce_loss` with CLIP's parameterisation of the scale: `logit_scale` holds log(1 / temperature) -- an `nn.Parameter` when
    `learnable`, a buffer otherwise, the `state_dict` key either way -- and the forward uses exp(logit_scale) clamped at
    `max_logit_scale`, as torch ops on the 0-dim device tensor, so autograd chains dL/ds through them.  `forward` takes the optional
    `pair_ids` of `info_nce_loss` (same-item pairs are excluded from the negatives)."""

    def __init__(self, temperature: float = 0.07, *, learnable: bool = True, max_logit_scale: float = 100.0, normalize: bool = True,
                 compute_mode: str = "fp32"):
        super().__init__()
        if not temperature > 0:
            raise ValueError(f"temperature must be positive, got {temperature}")
        init = torch.tensor(math.log(1.0 / temperature), dtype=torch.float32)
        if learnable:
            self.logit_scale = nn.Parameter(init)
        else:
            self.register_buffer("logit_scale", init)
        self.learnable = learnable
        self.max_logit_scale = max_logit_scale
        self.normalize = normalize
        self.compute_mode = compute_mode

    def forward(self, video_features, text_features, pair_ids=None):
        scale = self.logit_scale.exp().clamp(max=self.max_logit_scale)
        return info_nce_loss(video_features, text_features, scale, normalize=self.normalize, compute_mode=self.compute_mode,
                             pair_ids=pair_ids)

    def extra_repr(self):
        return (f"learnable={self.learnable}, max_logit_scale={self.max_logit_scale}, normalize={self.normalize}, "
                f"compute_mode={self.compute_mode!r}")
