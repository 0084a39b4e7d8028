"""The hardest-negative (max_violation=True) ranking loss: its dense float64 definition and the checks shared by
tests/test_hardneg_cpu.py (emulated library) and tests/test_gpu_hardneg.py (MI355X).  A helper module like tests/exact_inputs.py:
pytest collects nothing here.

DEFINITION (float64, dense; trainer/loss.py:30-41 with `cost_s = cost_s.max(1)[0]; cost_im = cost_im.max(0)[0]` between lines 40 and 41):
    S = im @ s^T,  cost_s[i, j] = max(0, m + S[i, j] - S[i, i]),  cost_im[i, j] = max(0, m + S[i, j] - S[j, j]),  both 0 at i == j
    loss = (sum_i max_j cost_s[i, j] + sum_j max_i cost_im[i, j]) / B^2
The positive pair's score is constant along a row of cost_s and a column of cost_im, so the maxima are selections on S itself:
    jr[i] = argmax_{j != i} S[i, j],  ic[j] = argmax_{i != j} S[i, j]      (among equal scores the LOWER index)
    hr[i] = max(0, m + S[i, jr[i]] - S[i, i]),  hc[j] = max(0, m + S[ic[j], j] - S[j, j])
and the gradient of B^2 loss has, per ACTIVE hinge only: hr[i]: s[jr[i]] - s[i] on grad_im[i], +im[i] on grad_s[jr[i]], -im[i] on
grad_s[i]; hc[j]: im[ic[j]] - im[j] on grad_s[j], +s[j] on grad_im[ic[j]], -s[j] on grad_im[j]."""
import torch

import crossclr_amd
import exact_inputs as xi
from crossclr_amd import ranking as R
from oracle import crossclr_oracle as orc

MODES = ("fp32", "bf16x3", "bf16")
EXACT_CASES = [("inter", 8, 16, 4), ("inter", 70, 48, 16), ("inter", 130, 200, None), ("mixed", 300, 40, 16), ("inter", 257, 64, None)]
EXACT_MARGIN = 0.25
RANDOM_CASES = [(70, 48, 1), (257, 72, 2), (130, 200, 11)]
RANDOM_MARGIN = 0.1
SPLIT_CASES = [(130, 200), (300, 40)]


def first_argmax(M, dim):
    """max and the LOWEST index that attains it along `dim` (torch.max does not promise which of several it returns)"""
    best = M.max(dim, keepdim=True).values
    n = M.shape[dim]
    idx = torch.arange(n).view(-1, 1) if dim == 0 else torch.arange(n).view(1, -1)
    return best.squeeze(dim), torch.where(M == best, idx, n).min(dim).values


def definition(im, s, margin):
    """The selections, hinges and loss of the definition above on float64 copies of (im, s); B >= 2."""
    im, s = im.double().cpu(), s.double().cpu()
    B = im.shape[0]
    S = im @ s.t()
    d = S.diag()
    Sm = S.masked_fill(torch.eye(B, dtype=torch.bool), float("-inf"))
    sr, jr = first_argmax(Sm, 1)
    sc, ic = first_argmax(Sm, 0)
    hr, hc = (margin + sr - d).clamp_min(0), (margin + sc - d).clamp_min(0)
    return dict(S=S, Sm=Sm, d=d, jr=jr, ic=ic, sr=sr, sc=sc, hr=hr, hc=hc, loss=float((hr.sum() + hc.sum()) / (B * B)))


def dense_loss(im, s, margin):
    """The reference's forward with the one inserted line, as eager float64 ops (for autograd)."""
    scores = im.mm(s.t())
    diagonal = scores.diag().view(im.size(0), 1)
    d1 = diagonal.expand_as(scores)
    d2 = diagonal.t().expand_as(scores)
    cost_s = (margin + scores - d1).clamp(min=0)
    cost_im = (margin + scores - d2).clamp(min=0)
    mask = torch.eye(scores.size(0)) > .5
    cost_s = cost_s.masked_fill(mask, 0)
    cost_im = cost_im.masked_fill(mask, 0)
    cost_s = cost_s.max(1)[0]
    cost_im = cost_im.max(0)[0]
    return (cost_s.sum() + cost_im.sum()).div(im.shape[0] * s.shape[0])


def closed_form_grads(im, s, jr, ic, active_r, active_c, grad_out):
    """The gradient's closed form in float64 from given selections and active flags, times grad_out / B^2."""
    im, s = im.double().cpu(), s.double().cpu()
    jr, ic = jr.cpu().long(), ic.cpu().long()
    B = im.shape[0]
    g_im, g_s = torch.zeros_like(im), torch.zeros_like(s)
    i = active_r.cpu().nonzero().flatten()
    g_im[i] += s[jr[i]] - s[i]
    g_s.index_add_(0, jr[i], im[i])
    g_s[i] -= im[i]
    j = active_c.cpu().nonzero().flatten()
    g_s[j] += im[ic[j]] - im[j]
    g_im.index_add_(0, ic[j], s[j])
    g_im[j] -= s[j]
    return g_im * (grad_out / (B * B)), g_s * (grad_out / (B * B))


def run(im, s, margin, mode, device, grad_out=3.0, splits=0):
    """(loss, grad_im, grad_s) of max_margin_loss(max_violation=True) on `device`, gradients of grad_out * loss."""
    a, b = im.detach().clone().to(device).requires_grad_(), s.detach().clone().to(device).requires_grad_()      # (fresh leaves: .grad accumulates)
    loss = R._max_margin(a, b, margin, mode, True, splits)
    (grad_out * loss).backward()
    return loss.detach(), a.grad, b.grad


_exact = {}


def exact_case(kind, B, D, nnz):
    """inputs and float64 definition of an exact-operand case, made once"""
    key = (kind, B, D, nnz)
    if key not in _exact:
        v, t = xi.planted(kind, B, D, nnz, seed=B + D)
        ref = definition(v, t, EXACT_MARGIN)
        ref["grads"] = closed_form_grads(v, t, ref["jr"], ref["ic"], ref["hr"] > 0, ref["hc"] > 0, 3.0)
        # the tie rule is exercised: a share of the rows and columns has a tied maximum
        ties = ((ref["Sm"] == ref["sr"][:, None]).sum(1) > 1).double().mean() + ((ref["Sm"] == ref["sc"][None, :]).sum(0) > 1).double().mean()
        assert ties > 0, "no tied maximum in this case"
        _exact[key] = (v, t, ref)
    return _exact[key]


def check_exact_case(kind, B, D, nnz, mode, device):
    """Test 1: indices equal the definition's with first-index ties, scores bit-equal, loss within 1e-6 max(1, |loss|), gradient rows 1e-6."""
    v, t, ref = exact_case(kind, B, D, nnz)
    hn = crossclr_amd.hardest_negatives(v.to(device), t.to(device), compute_mode=mode)
    assert hn["v2t_index"].dtype == torch.int64 and hn["v2t_score"].dtype == torch.float32
    assert torch.equal(hn["v2t_index"].cpu(), ref["jr"]), "video -> text selections"
    assert torch.equal(hn["t2v_index"].cpu(), ref["ic"]), "text -> video selections"
    assert torch.equal(hn["v2t_score"].cpu().double(), ref["sr"]) and torch.equal(hn["t2v_score"].cpu().double(), ref["sc"])
    assert torch.equal(hn["pair_score"].cpu().double(), ref["d"])
    loss, g_im, g_s = run(v, t, EXACT_MARGIN, mode, device)
    err = abs(float(loss) - ref["loss"])
    print(f"{kind} B={B} D={D} {mode}: loss {float(loss):.9g} ref {ref['loss']:.9g} |delta| {err:.3e}")
    assert err <= 1e-6 * max(1.0, abs(ref["loss"]))
    for got, want, what in ((g_im, ref["grads"][0], "grad_im"), (g_s, ref["grads"][1], "grad_s")):
        worst, row = xi.check_rows(got, want)
        print(f"  {what}: worst row {row} at {worst:.3e}")
        xi.check_rows(got, want, bar=1e-6)


_random = {}


def random_case(B, D, seed, rounded):
    """unit-row random inputs and their reference: autograd of the dense float64 definition (rounded: the definition on
    x.bfloat16().float() operands, the gradient's row terms from the unrounded tensors); the gap between the best and the second-best
    cost of every row and column is asserted (>= 1e-4) and every hinge is active"""
    key = (B, D, seed, rounded)
    if key not in _random:
        v, t = orc.make_inputs("randn", B, D, seed)
        v, t = torch.nn.functional.normalize(v, dim=1), torch.nn.functional.normalize(t, dim=1)
        ov, ot = (v.bfloat16().float(), t.bfloat16().float()) if rounded else (v, t)
        ref = definition(ov, ot, RANDOM_MARGIN)
        top_r, top_c = ref["Sm"].topk(2, dim=1).values, ref["Sm"].topk(2, dim=0).values
        gap = min(float((top_r[:, 0] - top_r[:, 1]).min()), float((top_c[0] - top_c[1]).min()))
        assert gap >= 1e-4, gap
        assert (ref["hr"] > 0).all() and (ref["hc"] > 0).all()
        if rounded:
            ref["grads"] = closed_form_grads(v, t, ref["jr"], ref["ic"], ref["hr"] > 0, ref["hc"] > 0, 3.0)
        else:
            a, b = v.double().requires_grad_(), t.double().requires_grad_()
            loss = dense_loss(a, b, RANDOM_MARGIN)
            assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12
            (3.0 * loss).backward()
            ref["grads"] = (a.grad, b.grad)
        _random[key] = (v, t, ref)
    return _random[key]


def check_random_case(B, D, seed, mode, device):
    """Test 2: indices equal, loss within 1e-5 max(1, |loss|), gradient rows within 1e-5 of the row's largest entry."""
    v, t, ref = random_case(B, D, seed, mode == "bf16")
    hn = crossclr_amd.hardest_negatives(v.to(device), t.to(device), compute_mode=mode)
    assert torch.equal(hn["v2t_index"].cpu(), ref["jr"]) and torch.equal(hn["t2v_index"].cpu(), ref["ic"])
    loss, g_im, g_s = run(v, t, RANDOM_MARGIN, mode, device)
    err = abs(float(loss) - ref["loss"])
    print(f"B={B} D={D} {mode}: loss {float(loss):.9g} ref {ref['loss']:.9g} |delta| {err:.3e}")
    assert err <= 1e-5 * max(1.0, abs(ref["loss"]))
    for got, want, what in ((g_im, ref["grads"][0], "grad_im"), (g_s, ref["grads"][1], "grad_s")):
        worst, row = xi.check_rows(got, want)
        print(f"  {what}: worst row {row} at {worst:.3e}")
        xi.check_rows(got, want, bar=1e-5)


def check_split_independence(B, D, device):
    """Test 3: indices, scores, loss and gradients are the same bits for every split count (each from ONE training pass: the autograd
    function hands its selections out beside the loss), and so is what `hardest_negatives` reports."""
    v, t = orc.make_inputs("cluster", B, D, B + D)      # 16 centres: many near-ties
    v, t = v.to(device), t.to(device)

    def one(splits):
        a, b = v.clone().requires_grad_(), t.clone().requires_grad_()
        loss, index, score = R._MaxViolationFunction.apply(a, b, RANDOM_MARGIN, "fp32", splits)
        (3.0 * loss).backward()
        return loss.detach(), index, score, a.grad, b.grad

    base = one(0)
    assert (base[1][:B] >= 0).all() and base[3].abs().sum() > 0
    for splits in (1, 2, 3):
        for x, y in zip(base, one(splits)):
            assert torch.equal(x, y), splits
    public, bpad = R._hardest(v, t, False, "fp32", 2), base[1].numel() // 2
    assert torch.equal(public["v2t_index"], base[1][:B].long()) and torch.equal(public["t2v_index"], base[1][bpad:bpad + B].long())
    assert torch.equal(public["v2t_score"], base[2][:B]) and torch.equal(public["t2v_score"], base[2][bpad:bpad + B])
