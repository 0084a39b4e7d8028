"""Score statistics of the video x text similarity matrix: the reference's max-margin ranking loss and retrieval ranks.

Mirrors `trainer/loss.py:7-41` of amazon-science/crossmodal-contrastive-learning:

    criterion = MaxMargin_coot(use_cuda=True, margin=0.1)
    loss = criterion(im, s)          # [B, D], [B, D] -> 0-dim; scores = im @ s.T, no normalisation (loss.py:7-15, 30)

The reference class cannot be constructed (`super(ContrastiveLoss_coot, self)` at loss.py:24 names an undefined class); its
`forward` (loss.py:29-41) is what is implemented, with the constructor arguments and attributes the reference declares
(`use_cuda`, `margin`, `sim`).  The B x B score matrix, its two hinge matrices and the eye mask are never materialised: two
tiled passes over the inter-modal block through the C-ABI (`crossclr_score_diag`, `crossclr_score_rows`) for the forward, the
generic tiled backward with indicator weights (`crossclr_maxmargin_backward[_finish]`) for the gradients.

`retrieval_ranks` is the evaluation step that follows training in the CrossCLR / COOT pipelines (not in the reference
repository): rank of each sample's partner among all candidates of the other modality, both directions, from the same kernels
with margin 0 (count of candidates scoring strictly higher than the partner).  `retrieval_topk` is its other half: WHO was retrieved --
the k best candidates of every query over two independent sets of any sizes, from the same tiled product with a selection epilogue
(`crossclr_topk_select`, `crossclr_topk_merge`).

`max_violation=True` is the hardest-negative form most COOT / VSE++ users train: one line between the reference's lines 40 and 41,
`cost_s = cost_s.max(1)[0]; cost_im = cost_im.max(0)[0]`.  One pass over the scores with a max + argmax epilogue in both directions
(`crossclr_hardneg_select`, `crossclr_hardneg_finish`), a sparse O(B D) gather for the gradients (`crossclr_hardneg_backward`);
`hardest_negatives` returns the selections themselves.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Tuple

import torch
from torch import nn

from . import _native as nat
from .loss import _IN_DTYPE, _device_of, _plan_for, _ptr, _refuse_double_backward, _resolve_mode, _row_major, _stream_for, _validate


def cosine_sim(emb1: torch.Tensor, emb2: torch.Tensor) -> torch.Tensor:
    """`trainer/loss.py:7-15`: the plain product emb1 @ emb2^T (a cosine only when the caller normalised the rows)."""
    return emb1.mm(emb2.t())


class _Scores:
    __slots__ = ("plan", "xhat", "ones", "diag", "hinge", "active", "loss_sum", "in_dtype", "margin", "mask")


def _score_rows(im: torch.Tensor, s: torch.Tensor, margin: float, compute_mode: str, normalize: bool, save_mask: bool = False) -> _Scores:
    lib = nat.library()
    b, D = im.shape
    dev = im.device
    mode = _resolve_mode(compute_mode, b, im.dtype)
    plan = _plan_for(b, D, 1, 0, mode)
    pp = ctypes.byref(plan)
    stream = _stream_for(im)
    f32 = dict(dtype=torch.float32, device=dev)
    sc = _Scores()
    sc.plan, sc.in_dtype, sc.margin = plan, _IN_DTYPE[im.dtype], float(margin)
    sc.xhat = torch.empty(plan.operand_bytes, dtype=torch.uint8, device=dev)
    sc.ones = torch.empty(2 * plan.bpad, **f32)          # inv_norm: all ones when the rows are used as given
    pair_cos = torch.empty(plan.bpad, **f32)
    lay_out = lib.crossclr_normalize if normalize else lib.crossclr_pack
    nat.check(lay_out(pp, _ptr(im), _ptr(s), im.stride(0), s.stride(0), sc.in_dtype, _ptr(sc.xhat), _ptr(sc.ones), _ptr(pair_cos), stream))
    sc.diag = torch.empty(2 * plan.bpad, **f32)
    nat.check(lib.crossclr_score_diag(pp, _ptr(sc.xhat), _ptr(sc.diag), stream))
    part = torch.empty(plan.fwd_ws_floats, **f32)
    sc.hinge, sc.active = torch.empty(2 * plan.bpad, **f32), torch.empty(2 * plan.bpad, **f32)
    sc.loss_sum = torch.empty(plan.loss_ws_doubles, dtype=torch.float64, device=dev)
    # With a backward to follow the same pass also leaves every pair's number of active hinges (one byte per pair, 64 MiB at B = 8192: the
    # reference's autograd keeps two B x B float hinge matrices for this): the backward is then one product with that mask instead of a
    # second evaluation of the scores.  CROSSCLR_MAXMARGIN_SAVE=0, or a library that declines (CROSSCLR_DISABLE_SYMMETRIC): the recomputing pair.
    sc.mask = None
    if save_mask and os.environ.get("CROSSCLR_MAXMARGIN_SAVE", "1") != "0":
        mask = torch.empty(lib.crossclr_maxmargin_mask_bytes(pp), dtype=torch.uint8, device=dev)
        if lib.crossclr_score_rows_save(pp, _ptr(sc.xhat), _ptr(sc.diag), sc.margin, _ptr(part), _ptr(sc.hinge), _ptr(sc.active),
                                        _ptr(sc.loss_sum), _ptr(mask), stream) == 0:
            sc.mask = mask
            return sc
    nat.check(lib.crossclr_score_rows(pp, _ptr(sc.xhat), _ptr(sc.diag), sc.margin, _ptr(part), _ptr(sc.hinge), _ptr(sc.active),
                                      _ptr(sc.loss_sum), stream))
    return sc


class _MaxMarginFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, im, s, margin, compute_mode):
        im_c, s_c = _row_major(im.detach()), _row_major(s.detach())
        with _device_of(im_c):
            sc = _score_rows(im_c, s_c, margin, compute_mode, normalize=False, save_mask=any(ctx.needs_input_grad[:2]))
        ctx.sc = sc
        ctx.save_for_backward(im_c, s_c)
        # (cost_s.sum() + cost_im.sum()).div(B * B) (loss.py:41), in the input dtype like the reference's eager ops
        return sc.loss_sum[1].to(im.dtype if im.dtype != torch.float64 else torch.float64)

    @staticmethod
    def backward(ctx, grad_out):
        _refuse_double_backward("MaxMargin_coot")
        im_c, s_c = ctx.saved_tensors
        sc, lib = ctx.sc, nat.library()
        plan = sc.plan
        pp = ctypes.byref(plan)
        dev = im_c.device
        with _device_of(im_c):
            stream = _stream_for(im_c)
            gbuf = torch.empty(plan.gbuf_bytes // 4, dtype=torch.float32, device=dev)
            if sc.mask is not None:
                nat.check(lib.crossclr_maxmargin_backward_saved(pp, _ptr(sc.xhat), _ptr(sc.mask), _ptr(gbuf), stream))
            else:
                nat.check(lib.crossclr_maxmargin_backward(pp, _ptr(sc.xhat), _ptr(sc.diag), sc.margin, _ptr(gbuf), stream))
            go = grad_out.detach().to(device=dev, dtype=torch.float64).reshape(1).contiguous()
            g_im, g_s = torch.empty_like(im_c), torch.empty_like(s_c)
            nat.check(lib.crossclr_maxmargin_backward_finish(pp, _ptr(gbuf), _ptr(im_c), _ptr(s_c), im_c.stride(0), s_c.stride(0),
                                                             sc.in_dtype, _ptr(sc.ones), _ptr(sc.active), _ptr(go), _ptr(g_im), _ptr(g_s),
                                                             g_im.stride(0), g_s.stride(0), stream))
        return (g_im if ctx.needs_input_grad[0] else None, g_s if ctx.needs_input_grad[1] else None, None, None)


class _HardNeg:
    __slots__ = ("plan", "in_dtype", "index", "score", "hinge", "pair", "loss_sum")


def _hardneg(im: torch.Tensor, s: torch.Tensor, margin: float, compute_mode: str, normalize: bool, splits: int = 0) -> _HardNeg:
    """Select + finish: per video row the best-scoring text that is not its partner, per text column the best-scoring video, the two
    hinges per sample and the loss.  `splits` (0 = the library's choice) cuts the launch; the result does not depend on it."""
    lib = nat.library()
    b, D = im.shape
    dev = im.device
    plan = _plan_for(b, D, 1, 0, _resolve_mode(compute_mode, b, im.dtype))
    pp = ctypes.byref(plan)
    stream = _stream_for(im)
    f32 = dict(dtype=torch.float32, device=dev)
    hn = _HardNeg()
    hn.plan, hn.in_dtype = plan, _IN_DTYPE[im.dtype]
    xhat = torch.empty(plan.operand_bytes, dtype=torch.uint8, device=dev)
    inv_norm, pair_cos = torch.empty(2 * plan.bpad, **f32), torch.empty(plan.bpad, **f32)
    lay_out = lib.crossclr_normalize if normalize else lib.crossclr_pack
    nat.check(lay_out(pp, _ptr(im), _ptr(s), im.stride(0), s.stride(0), hn.in_dtype, _ptr(xhat), _ptr(inv_norm), _ptr(pair_cos), stream))
    ws = torch.empty(lib.crossclr_hardneg_workspace_bytes(pp, splits), dtype=torch.uint8, device=dev)
    nat.check(lib.crossclr_hardneg_select(pp, _ptr(xhat), splits, _ptr(ws), ws.numel(), stream))
    hn.index = torch.empty(2 * plan.bpad, dtype=torch.int32, device=dev)
    hn.score, hn.hinge, hn.pair = torch.empty(2 * plan.bpad, **f32), torch.empty(2 * plan.bpad, **f32), torch.empty(plan.bpad, **f32)
    hn.loss_sum = torch.empty(plan.loss_ws_doubles, dtype=torch.float64, device=dev)
    nat.check(lib.crossclr_hardneg_finish(pp, _ptr(ws), splits, float(margin), _ptr(hn.index), _ptr(hn.score), _ptr(hn.hinge), _ptr(hn.pair),
                                          _ptr(hn.loss_sum), stream))
    return hn


class _MaxViolationFunction(torch.autograd.Function):
    """The hardest-negative form.  Saved for backward: the two index arrays and the two hinge arrays (4 * bpad * 4 bytes) and the caller's
    tensors -- no B x B mask, no packed operand.  Outputs: the loss and, not differentiable, the stacked selections of the pass
    (index [2 bpad] int32 and score [2 bpad] float32: video rows, then text columns from bpad on)."""

    @staticmethod
    def forward(ctx, im, s, margin, compute_mode, splits):
        im_c, s_c = _row_major(im.detach()), _row_major(s.detach())
        with _device_of(im_c):
            hn = _hardneg(im_c, s_c, margin, compute_mode, normalize=False, splits=splits)
        ctx.plan, ctx.in_dtype = hn.plan, hn.in_dtype
        ctx.save_for_backward(im_c, s_c, hn.index, hn.hinge)
        ctx.mark_non_differentiable(hn.index, hn.score)
        return hn.loss_sum[1].to(im.dtype if im.dtype != torch.float64 else torch.float64), hn.index, hn.score

    @staticmethod
    def backward(ctx, grad_out, _grad_index, _grad_score):
        _refuse_double_backward("MaxMargin_coot")
        im_c, s_c, index, hinge = ctx.saved_tensors
        lib, dev = nat.library(), im_c.device
        with _device_of(im_c):
            go = grad_out.detach().to(device=dev, dtype=torch.float64).reshape(1).contiguous()
            g_im = torch.empty_like(im_c) if ctx.needs_input_grad[0] else None
            g_s = torch.empty_like(s_c) if ctx.needs_input_grad[1] else None
            nat.check(lib.crossclr_hardneg_backward(ctypes.byref(ctx.plan), _ptr(im_c), _ptr(s_c), im_c.stride(0), s_c.stride(0), ctx.in_dtype,
                                                    _ptr(index), _ptr(hinge), _ptr(go), _ptr(g_im), _ptr(g_s),
                                                    0 if g_im is None else g_im.stride(0), 0 if g_s is None else g_s.stride(0),
                                                    _stream_for(im_c)))
        return g_im, g_s, None, None, None


def _check(im: torch.Tensor, s: torch.Tensor) -> None:
    _validate(im, s)
    if not im.is_cuda and nat.backend() != "emu-host":
        raise RuntimeError("the HIP path needs inputs on the GPU (got a CPU tensor); there is no CPU fallback")
    if im.shape[0] == 0:
        raise RuntimeError("empty batch")


def _max_margin(im: torch.Tensor, s: torch.Tensor, margin: float, compute_mode: str, max_violation: bool, splits: int = 0) -> torch.Tensor:
    """`max_margin_loss` with the number of column splits of the hardest-negative pass exposed (0 = the library's choice): the result does
    not depend on it."""
    _check(im, s)
    if max_violation:
        return _MaxViolationFunction.apply(im, s, float(margin), compute_mode, int(splits))[0]
    return _MaxMarginFunction.apply(im, s, float(margin), compute_mode)


def max_margin_loss(im: torch.Tensor, s: torch.Tensor, margin: float = 0.1, *, compute_mode: str = "fp32",
                    max_violation: bool = False) -> torch.Tensor:
    """Functional form of `MaxMargin_coot.forward` (trainer/loss.py:29-41).  compute_mode="fp32" (default) = exact-fp32 products like the
    reference's `mm`; "bf16" is opt-in: the scores are products of the caller's UN-normalised rows, so there is no a-priori error bar.

    max_violation=True is the hardest-negative form (VSE++; COOT's `max_violation`): `cost_s = cost_s.max(1)[0]; cost_im = cost_im.max(0)[0]`
    between the reference's lines 40 and 41, i.e. (sum_i max_j cost_s[i, j] + sum_j max_i cost_im[i, j]) / (B * B).  The divisor stays
    B * B so that the two forms differ by that one line: `B * loss` is VSE++'s per-sample mean.  Among bit-equal scores the lower index is
    the hardest negative; only active hinges (> 0) carry gradient, through the caller's own tensors.  All three compute modes ("fp32",
    "bf16", "bf16x3") are available in this form; NaN inputs are not ordered (the rows must be finite)."""
    return _max_margin(im, s, margin, compute_mode, max_violation)


class MaxMargin_coot(nn.Module):
    """Regular contrastive (max-margin ranking) loss between two groups of embeddings, inputs [batch, embed_dim]
    (`trainer/loss.py:17-41`; COOT, NeurIPS 2020).  Constructor arguments and attributes as the reference declares them
    (loss.py:23-27); `use_cuda` is kept for signature compatibility -- the inputs must be on the GPU either way.
    max_violation=True: the hardest-negative form (see `max_margin_loss`)."""

    def __init__(self, use_cuda: bool = True, margin: float = 0.1, *, compute_mode: str = "fp32", max_violation: bool = False):
        super().__init__()
        self.margin = margin
        self.sim = cosine_sim
        self.use_cuda = use_cuda
        self.compute_mode = compute_mode
        self.max_violation = max_violation

    def forward(self, im, s):
        return max_margin_loss(im, s, self.margin, compute_mode=self.compute_mode, max_violation=self.max_violation)

    def extra_repr(self):
        return f"margin={self.margin}, compute_mode={self.compute_mode!r}, max_violation={self.max_violation}"


def _hardest(im: torch.Tensor, s: torch.Tensor, normalize: bool, compute_mode: str, splits: int = 0) -> Dict[str, torch.Tensor]:
    """`hardest_negatives` with the number of column splits exposed (0 = the library's choice): the result does not depend on it."""
    _check(im, s)
    v, t = _row_major(im.detach()), _row_major(s.detach())
    with _device_of(v):
        hn = _hardneg(v, t, 0.0, compute_mode, normalize=normalize, splits=splits)
    b, bpad = hn.plan.b, hn.plan.bpad
    return {"v2t_index": hn.index[:b].to(torch.int64), "t2v_index": hn.index[bpad:bpad + b].to(torch.int64),
            "v2t_score": hn.score[:b], "t2v_score": hn.score[bpad:bpad + b], "pair_score": hn.pair[:b]}


def hardest_negatives(video_features: torch.Tensor, text_features: torch.Tensor, *, normalize: bool = False,
                      compute_mode: str = "fp32") -> Dict[str, torch.Tensor]:
    """Each sample's hardest negative in both directions over S = video @ text^T (normalize=True: cosines, rows L2-normalised like the
    loss does; default: rows as given, what `MaxMargin_coot(max_violation=True)` trains on) -- the selections of that loss's training
    pass, from the same kernels.

    Returns device tensors (no autograd, nothing synchronises the host): `v2t_index[i]` = argmax_{j != i} S[i, j] and `t2v_index[j]` =
    argmax_{i != j} S[i, j] (int64; higher score first, among bit-equal scores the lower index; -1 when B = 1 leaves no candidate),
    `v2t_score` / `t2v_score` (float32) the scores at those indices, `pair_score[i]` = S[i, i].  NaN inputs are not ordered."""
    return _hardest(video_features, text_features, normalize, compute_mode)


def retrieval_ranks(video_features: torch.Tensor, text_features: torch.Tensor, *, normalize: bool = True,
                    compute_mode: str = "fp32") -> Dict[str, torch.Tensor]:
    """Ranks of the partners in both retrieval directions over the B x B cosine matrix (normalize=False: plain products).

    Returns device tensors (nothing synchronises the host): `v2t_ranks[i]` = number of texts scoring strictly higher than text i
    for video i (0 = retrieved first), `t2v_ranks[j]` likewise; `v2t` / `t2v` = [R@1, R@5, R@10, median rank, mean rank] with
    ranks counted from 1 as in the CrossCLR / COOT evaluation tables.  compute_mode="fp32" (default) = exact-fp32 products."""
    _check(video_features, text_features)
    v, t = _row_major(video_features.detach()), _row_major(text_features.detach())
    with _device_of(v):
        sc = _score_rows(v, t, 0.0, compute_mode, normalize=normalize)
    b, bpad = sc.plan.b, sc.plan.bpad
    out = {"v2t_ranks": sc.active[:b].to(torch.int64), "t2v_ranks": sc.active[bpad:bpad + b].to(torch.int64)}
    for key in ("v2t", "t2v"):
        r = out[key + "_ranks"].to(torch.float64)
        out[key] = torch.stack([(r < 1).double().mean(), (r < 5).double().mean(), (r < 10).double().mean(),
                                r.median() + 1.0, r.mean() + 1.0])
    return out


def _topk(queries: torch.Tensor, gallery: torch.Tensor, k: int, normalize: bool, compute_mode: str, splits: int = 0):
    """`retrieval_topk` with the number of column splits exposed (0 = the library's choice): the result does not depend on it."""
    for name, t in (("queries", queries), ("gallery", gallery)):
        if t.dim() != 2:
            raise RuntimeError(f"retrieval_topk expects 2-D [rows, embed_dim] inputs, got {name} of shape {tuple(t.shape)}")
    if queries.shape[1] != gallery.shape[1]:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({queries.shape[0]}x{queries.shape[1]} and "
                           f"{gallery.shape[1]}x{gallery.shape[0]})")
    if queries.dtype != gallery.dtype:
        raise RuntimeError(f"expected both inputs to have the same dtype, got {queries.dtype} and {gallery.dtype}")
    if queries.dtype not in _IN_DTYPE:
        raise RuntimeError(f"unsupported input dtype {queries.dtype}")
    if queries.device != gallery.device:
        raise RuntimeError("queries and gallery must be on the same device")
    if not queries.is_cuda and nat.backend() != "emu-host":
        raise RuntimeError("the HIP path needs inputs on the GPU (got a CPU tensor); there is no CPU fallback")
    nq, D = queries.shape
    ng = gallery.shape[0]
    if nq == 0 or ng == 0 or D == 0:
        raise RuntimeError("empty set")
    lib = nat.library()
    k = int(k)
    if k < 1:
        raise ValueError(f"k must be at least 1, got {k}")
    if k > ng:
        raise ValueError(f"k = {k} is larger than the gallery ({ng} rows)")
    if k > lib.crossclr_topk_max_k():
        raise ValueError(f"k = {k} is above the library's limit of {lib.crossclr_topk_max_k()}")
    mode = _resolve_mode(compute_mode, max(nq, ng), queries.dtype)
    q, g = _row_major(queries.detach()), _row_major(gallery.detach())
    dev, in_dtype = q.device, _IN_DTYPE[q.dtype]
    with _device_of(q):
        stream = _stream_for(q)
        qp = torch.empty(lib.crossclr_topk_operand_bytes(nq, D, mode), dtype=torch.uint8, device=dev)
        gp = torch.empty(lib.crossclr_topk_operand_bytes(ng, D, mode), dtype=torch.uint8, device=dev)
        nat.check(lib.crossclr_topk_pack(_ptr(q), q.stride(0), nq, D, in_dtype, mode, int(normalize), _ptr(qp), stream))
        nat.check(lib.crossclr_topk_pack(_ptr(g), g.stride(0), ng, D, in_dtype, mode, int(normalize), _ptr(gp), stream))
        ws = torch.empty(lib.crossclr_topk_workspace_bytes(nq, ng, k, splits), dtype=torch.uint8, device=dev)
        scores = torch.empty(nq, k, dtype=torch.float32, device=dev)
        index = torch.empty(nq, k, dtype=torch.int32, device=dev)
        nat.check(lib.crossclr_topk_select(_ptr(qp), _ptr(gp), nq, ng, D, mode, k, splits, _ptr(ws), ws.numel(), stream))
        nat.check(lib.crossclr_topk_merge(_ptr(ws), nq, ng, k, splits, _ptr(scores), _ptr(index), stream))
        return scores, index.to(torch.int64)


def retrieval_topk(queries: torch.Tensor, gallery: torch.Tensor, k: int, *, normalize: bool = True,
                   compute_mode: str = "fp32") -> Tuple[torch.Tensor, torch.Tensor]:
    """The k best gallery rows of every query: `scores` [Nq, k] float32 and `indices` [Nq, k] int64 of the k largest
    S[i, j] = q_i . g_j (cosines with normalize=True: rows L2-normalised like the loss does; normalize=False: rows as given).

    `queries` [Nq, D] and `gallery` [Ng, D] are independent sets (several captions per clip, a few queries against a large gallery); the
    Nq x Ng score matrix is never materialised.  Row i is sorted: higher score first, among bit-equal scores the lower gallery index first
    (identical gallery rows score bit-equal); the result does not depend on how the launch is cut.  No autograd (inputs are detached);
    device tensors come back and nothing synchronises the host.  compute_mode: "fp32" (default, exact-fp32 products), "bf16", "bf16x3",
    or "auto" (decided on max(Nq, Ng)).  ValueError for k < 1, k > Ng or k above the library's limit (64); RuntimeError for mismatched D or
    an empty set.

    R@k against arbitrary ground truth (`target[i]` = the gallery row that is right for query i):

        scores, indices = retrieval_topk(text_emb, video_emb, 10)
        hit = (indices == target[:, None]).any(1)          # R@10 = hit.float().mean()

    Hard negatives for the next epoch, a set against itself (column 0 is the row itself):

        _, indices = retrieval_topk(emb, emb, 1 + n_neg)
        hard_negatives = indices[:, 1:]
    """
    return _topk(queries, gallery, k, normalize, compute_mode)
