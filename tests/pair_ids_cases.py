"""pair_ids of the InfoNCE and the sigmoid loss (same-item pairs are excluded from the negatives): the dense float64 definitions, the id
patterns and the checks shared by tests/test_pair_ids_cpu.py (emulated library) and tests/test_gpu_pair_ids.py (MI355X).  A helper module
like tests/infonce_cases.py: pytest collects nothing here.

DEFINITION: `infonce_cases.definition` / `sigmoid_cases.definition` with  ex = (ids[:, None] == ids[None, :]) & ~eye:
    InfoNCE   Z.masked_fill(ex, -inf) before both logsumexps; the divisor stays 2 B; W = 0 on ex, A from that W
    sigmoid   the term matrix and W are 0 on ex; the divisor stays B; A_s and A_b from that W
The dicts have the keys of the two modules' definitions (and S, ex), so THEIR `check` / `check_lse` / `check_rows` and THEIR bars are used
as they stand.  grad_out = 3.

ID PATTERNS
    runs3     ids[i] = i // 3: groups inside a fragment; rows 126-128 straddle the 128-row block boundary, 255-256 the next (B = 257)
    stride7   ids[i] = i % 7: about B / 7 exclusions per row, in every tile, every split and every gradient slice
    equal     all 0: every negative is excluded
    distinct  arange(B);   low32  i << 32: all distinct, all equal in their low 32 bits
    relabel(ids) = (ids - 3) * (2**40 + 7): injective, reaches negative values and values beyond 32 bits"""
import torch
import torch.nn.functional as F

import infonce_cases as ic
import sigmoid_cases as sc
from crossclr_amd import infonce as N
from crossclr_amd import sigmoid as G

GRAD_OUT = 3.0
MODES = ic.MODES
SHAPES = ic.SHAPES
RANDOM_CASES = ic.RANDOM_CASES
PATTERNS = {
    "runs3": lambda B: torch.arange(B, dtype=torch.int64) // 3,
    "stride7": lambda B: torch.arange(B, dtype=torch.int64) % 7,
    "equal": lambda B: torch.zeros(B, dtype=torch.int64),
    "distinct": lambda B: torch.arange(B, dtype=torch.int64),
    "low32": lambda B: torch.arange(B, dtype=torch.int64) << 32,
}


def ids_of(pattern, B):
    return PATTERNS[pattern](B)


def relabel(ids):
    return (ids - 3) * (2 ** 40 + 7)


def excluded(ids):
    ids = ids.detach().cpu().to(torch.int64)
    return (ids[:, None] == ids[None, :]) & ~torch.eye(ids.numel(), dtype=torch.bool)


def infonce_definition(v, t, s, normalize, ids, grad_out=GRAD_OUT):
    a, b = v.detach().double().cpu().clone().requires_grad_(), t.detach().double().cpu().clone().requires_grad_()
    sc_ = torch.tensor(ic.f32_value(s), dtype=torch.float64, requires_grad=True)
    B = a.shape[0]
    ex = excluded(ids)
    va, tb = (F.normalize(a, dim=1), F.normalize(b, dim=1)) if normalize else (a, b)
    S = va @ tb.t()
    Z = sc_ * S
    Zm = Z.masked_fill(ex, float("-inf"))
    lr, lc = torch.logsumexp(Zm, 1), torch.logsumexp(Zm, 0)
    loss = (lr + lc - 2 * Z.diag()).sum() / (2 * B)
    (grad_out * loss).backward()
    with torch.no_grad():
        W = torch.exp(Z - lr[:, None]) + torch.exp(Z - lc[None, :]) - 2 * torch.eye(B, dtype=torch.float64)
        W[ex] = 0.0
        A = float((W * S).abs().sum() / (2 * B))
    return dict(loss=float(loss.detach()), gv=a.grad, gt=b.grad, gs=float(sc_.grad), lr=lr.detach(), lc=lc.detach(), pair=S.detach().diag(),
                A=A, s=float(sc_.detach()), B=B, S=S.detach(), ex=ex)


def sigmoid_definition(v, t, s, beta, normalize, ids, grad_out=GRAD_OUT):
    a, b = v.detach().double().cpu().clone().requires_grad_(), t.detach().double().cpu().clone().requires_grad_()
    sc_ = torch.tensor(ic.f32_value(s), dtype=torch.float64, requires_grad=True)
    bc = torch.tensor(ic.f32_value(beta), dtype=torch.float64, requires_grad=True)
    B = a.shape[0]
    ex = excluded(ids)
    va, tb = (F.normalize(a, dim=1), F.normalize(b, dim=1)) if normalize else (a, b)
    S = va @ tb.t()
    Z = sc_ * S + bc
    eye = torch.eye(B, dtype=torch.float64)
    terms = (-F.logsigmoid((2 * eye - 1) * Z)).masked_fill(ex, 0.0)
    loss = terms.sum() / B
    (grad_out * loss).backward()
    with torch.no_grad():
        W = torch.sigmoid(Z) - eye
        W[eye.bool()] = -torch.sigmoid(-Z.diag())      # (not sigma(z) - 1: that cancels)
        W[ex] = 0.0
        A_s, A_b = float((W * S).abs().sum() / B), float(W.abs().sum() / B)
    return dict(loss=float(loss.detach()), gv=a.grad, gt=b.grad, gs=float(sc_.grad), gb=float(bc.grad), row_loss=terms.detach().sum(1),
                pair=S.detach().diag(), A_s=A_s, A_b=A_b, s=float(sc_.detach()), beta=float(bc.detach()), B=B, S=S.detach(), ex=ex)


def _ids_on(ids, device):
    return None if ids is None else ids.to(device)


def run_infonce(v, t, s, mode, normalize, device, ids, splits=0, grad_out=GRAD_OUT):
    """`infonce_cases.run` with pair_ids (None: the keyword's default); ids are handed on as they are (dtype, strides), on `device`"""
    a, b = v.detach().clone().to(device).requires_grad_(), t.detach().clone().to(device).requires_grad_()
    sc_ = torch.tensor(float(s), dtype=torch.float32, device=device, requires_grad=True)
    loss, lse, pair = N._info_nce(a, b, sc_, normalize, mode, splits, pair_ids=_ids_on(ids, device))
    (grad_out * loss).backward()
    return dict(loss=loss.detach(), gv=a.grad, gt=b.grad, gs=sc_.grad, lse=lse, pair=pair)


def run_sigmoid(v, t, s, beta, mode, normalize, device, ids, splits=0, grad_out=GRAD_OUT):
    a, b = v.detach().clone().to(device).requires_grad_(), t.detach().clone().to(device).requires_grad_()
    sc_ = torch.tensor(float(s), dtype=torch.float32, device=device, requires_grad=True)
    bc = torch.tensor(float(beta), dtype=torch.float32, device=device, requires_grad=True)
    loss, row_loss, pair = G._sigmoid(a, b, sc_, bc, normalize, mode, splits, pair_ids=_ids_on(ids, device))
    (grad_out * loss).backward()
    return dict(loss=loss.detach(), gv=a.grad, gt=b.grad, gs=sc_.grad, gb=bc.grad, row_loss=row_loss, pair=pair)


def same_bits(x, y, what):
    assert x.keys() == y.keys()
    for key in x:
        assert torch.equal(x[key], y[key]), f"{what}: {key} differs"


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def operands(kind, B, D, seed, rounded):
    """infonce_cases.inputs; rounded: F.normalize(x).bfloat16().float(), to be fed with normalize=False"""
    def make():
        v, t = ic.inputs(kind, B, D, seed)
        if rounded:
            v, t = F.normalize(v, dim=1).bfloat16().float(), F.normalize(t, dim=1).bfloat16().float()
        return v, t
    return cached(("in", kind, B, D, seed, rounded), make)


def infonce_case(kind, B, D, seed, s, pattern, rounded=False):
    """(v, t, ids, definition), made once"""
    v, t = operands(kind, B, D, seed, rounded)
    ids = ids_of(pattern, B)
    return v, t, ids, cached(("n", kind, B, D, seed, ic.f32_value(s), pattern, rounded), lambda: infonce_definition(v, t, s, not rounded, ids))


def sigmoid_case(kind, B, D, seed, s, beta, pattern, rounded=False):
    v, t = operands(kind, B, D, seed, rounded)
    ids = ids_of(pattern, B)
    key = ("g", kind, B, D, seed, ic.f32_value(s), ic.f32_value(beta), pattern, rounded)
    return v, t, ids, cached(key, lambda: sigmoid_definition(v, t, s, beta, not rounded, ids))


def check_infonce_case(B, D, seed, s, mode, pattern, device, kind="randn"):
    """Check 1: fp32 / bf16x3 against the definition on randn rows; bf16 on bf16-rounded unit rows fed with normalize=False"""
    rounded = mode == "bf16"
    v, t, ids, ref = infonce_case(kind, B, D, seed, s, pattern, rounded)
    out = run_infonce(v, t, s, mode, not rounded, device, ids)
    what = f"{pattern} B={B} D={D}"
    ic.check(out, ref, mode, what)
    ic.check_lse(out, ref, what)
    return out, ref


def check_sigmoid_case(B, D, seed, s, beta, mode, pattern, device, kind="randn"):
    rounded = mode == "bf16"
    v, t, ids, ref = sigmoid_case(kind, B, D, seed, s, beta, pattern, rounded)
    out = run_sigmoid(v, t, s, beta, mode, not rounded, device, ids)
    what = f"{pattern} B={B} D={D}"
    sc.check(out, ref, mode, what)
    sc.check_rows(out, ref, what)
    return out, ref


def _mode_inputs(B, D, seed, mode):
    rounded = mode == "bf16"
    v, t = operands("randn", B, D, seed, rounded)
    return v, t, not rounded


def check_distinct_ids_give_the_bits_of_none(B, D, mode, device):
    """Check 2: `distinct` and `low32` (all ids differ; low32's differ in their HIGH words only) exclude nothing: every output is the
    pair_ids=None run's, bit for bit"""
    v, t, normalize = _mode_inputs(B, D, B + D, mode)
    base_n = run_infonce(v, t, ic.SCALES[0], mode, normalize, device, None)
    base_g = run_sigmoid(v, t, 10.0, -10.0, mode, normalize, device, None)
    for pattern in ("distinct", "low32"):
        ids = ids_of(pattern, B)
        same_bits(run_infonce(v, t, ic.SCALES[0], mode, normalize, device, ids), base_n, f"InfoNCE {pattern} {mode}")
        same_bits(run_sigmoid(v, t, 10.0, -10.0, mode, normalize, device, ids), base_g, f"sigmoid {pattern} {mode}")


def id_forms(ids):
    """the same partition four ways: as given, relabelled (negative and > 32-bit values), int32, a non-contiguous view"""
    view = torch.stack([ids, ids], 1)[:, 0]
    assert not view.is_contiguous() or ids.numel() == 1
    return [("relabel", relabel(ids)), ("int32", ids.to(torch.int32)), ("strided", view)]


def check_labelling_does_not_matter(pattern, device, B=257, D=72):
    """Check 3"""
    v, t = operands("randn", B, D, 2, False)
    ids = ids_of(pattern, B)
    assert torch.equal(excluded(relabel(ids)), excluded(ids)) and int(relabel(ids).min()) < 0 and int(relabel(ids).max()) > 2 ** 32
    base_n = run_infonce(v, t, ic.SCALES[0], "fp32", True, device, ids)
    base_g = run_sigmoid(v, t, 10.0, -10.0, "fp32", True, device, ids)
    for name, other in id_forms(ids):
        same_bits(run_infonce(v, t, ic.SCALES[0], "fp32", True, device, other), base_n, f"InfoNCE {pattern} {name}")
        same_bits(run_sigmoid(v, t, 10.0, -10.0, "fp32", True, device, other), base_g, f"sigmoid {pattern} {name}")


def check_the_ids_matter(device, B=70, D=48):
    """Check 4: with stride7 the loss is far (> 100 loss bars) from the pair_ids=None loss"""
    v, t, ids, ref = infonce_case("randn", B, D, 1, ic.SCALES[0], "stride7")
    with_ids = run_infonce(v, t, ic.SCALES[0], "fp32", True, device, ids)
    without = run_infonce(v, t, ic.SCALES[0], "fp32", True, device, None)
    d = abs(float(with_ids["loss"]) - float(without["loss"]))
    print(f"InfoNCE: |loss(ids) - loss(None)| = {d:.3e}, 100 bars = {100 * ic.loss_bar(ref):.3e}")
    assert d > 100 * ic.loss_bar(ref)
    # (at SigLIP's (10, -10) a negative's softplus is 4.5e-5: (100, 0) gives the excluded terms a size)
    v, t, ids, ref = sigmoid_case("randn", B, D, 1, 100.0, 0.0, "stride7")
    with_ids = run_sigmoid(v, t, 100.0, 0.0, "fp32", True, device, ids)
    without = run_sigmoid(v, t, 100.0, 0.0, "fp32", True, device, None)
    d = abs(float(with_ids["loss"]) - float(without["loss"]))
    print(f"sigmoid: |loss(ids) - loss(None)| = {d:.3e}, 100 bars = {100 * sc.loss_bar(ref):.3e}")
    assert d > 100 * sc.loss_bar(ref)


def check_equal_ids(B, D, mode, device):
    """Check 5: every negative excluded.  InfoNCE: the definition is 0 throughout (loss, gradients, dL/ds); the floor term of the
    gradient bar is all there is.  Sigmoid: 1/B sum_i softplus(-z_ii), at the ordinary bars."""
    s = ic.SCALES[0]
    v, t, ids, ref = infonce_case("randn", B, D, B + D, s, "equal")
    assert abs(ref["loss"]) < 1e-12 and float(ref["gv"].abs().max()) < 1e-12 and abs(ref["gs"]) < 1e-12
    out = run_infonce(v, t, s, mode, True, device, ids)
    floor = 1e-7 * abs(ref["s"]) / B
    figures = [("loss", abs(float(out["loss"])), ic.loss_bar(ref)), ("gv", float(out["gv"].abs().max()), floor),
               ("gt", float(out["gt"].abs().max()), floor), ("ds", abs(float(out["gs"])), floor)]
    print(f"equal InfoNCE B={B} D={D} {mode}: " + "  ".join(f"{k} {e:.3e} (bar {b:.3e})" for k, e, b in figures))
    assert torch.isfinite(out["gv"]).all() and torch.isfinite(out["gt"]).all() and torch.isfinite(out["gs"]).all()
    for k, e, b in figures:
        assert e <= b, (k, e, b)
    ic.check_lse(out, ref, f"equal B={B} D={D}")
    v, t, ids, ref = sigmoid_case("randn", B, D, B + D, 10.0, -10.0, "equal")
    want = float(F.softplus(-(ref["s"] * ref["pair"] + ref["beta"])).sum() / B)
    assert abs(ref["loss"] - want) <= 1e-12 * max(1.0, abs(want))
    out = run_sigmoid(v, t, 10.0, -10.0, mode, True, device, ids)
    sc.check(out, ref, mode, f"equal B={B} D={D}")
    sc.check_rows(out, ref, f"equal B={B} D={D}")


# Check 6: (min over the excluded entries of (s S[i, j] - lr[i]) log2(e), the definition's loss), in SHAPES order
DOMINANT_S = 300.0
DOMINANT = {(8, 16): (167.7, 121.2), (70, 48): (226.4, 101.0), (257, 72): (249.2, 95.5), (130, 200): (321.3, 53.5), (300, 40): (177.5, 129.0)}


def dominant_inputs(B, D):
    """every excluded score is 1, the maximum of its row and of its column: pairs (2k, 2k + 1) are one item, t[2k + 1] = v[2k] and
    t[2k] = v[2k + 1]"""
    def make():
        g = torch.Generator().manual_seed(B + D)
        v = torch.randn(B, D, generator=g)
        t = torch.randn(B, D, generator=g)
        n = B // 2 * 2
        t[1:n:2] = v[0:n:2]
        t[0:n:2] = v[1:n:2]
        return v, t, torch.arange(B, dtype=torch.int64) // 2
    return cached(("dominant", B, D), make)


def check_dominant_excluded_entries(B, D, device):
    v, t, ids = dominant_inputs(B, D)
    ref = cached(("dominant n", B, D), lambda: infonce_definition(v, t, DOMINANT_S, True, ids))
    over = (ref["s"] * ref["S"] - ref["lr"][:, None]) * 1.4426950408889634
    margin = float(over[ref["ex"]].min())
    print(f"dominant B={B} D={D}: min excluded (s S - lr) log2(e) = {margin:.1f}, loss {ref['loss']:.1f}")
    assert margin > 128, margin      # an exp2 of the unmasked entry overflows fp32: masking after it, or by a product, gives inf / NaN
    assert abs(margin - DOMINANT[(B, D)][0]) <= 0.06 and abs(ref["loss"] - DOMINANT[(B, D)][1]) <= 0.06
    out = run_infonce(v, t, DOMINANT_S, "fp32", True, device, ids)
    ic.check(out, ref, "fp32", f"dominant B={B} D={D}")
    ic.check_lse(out, ref, f"dominant B={B} D={D}")
    ref = cached(("dominant g", B, D), lambda: sigmoid_definition(v, t, 100.0, -10.0, True, ids))
    out = run_sigmoid(v, t, 100.0, -10.0, "fp32", True, device, ids)
    sc.check(out, ref, "fp32", f"dominant B={B} D={D}")
    sc.check_rows(out, ref, f"dominant B={B} D={D}")


def check_splits(device, B=300, D=40):
    """Check 7: stride7 under every split count, as infonce_cases.check_splits / sigmoid_cases.check_splits do without ids"""
    s = ic.SCALES[0]
    v, t, ids, ref = infonce_case("randn", B, D, 5, s, "stride7")
    base = run_infonce(v, t, s, "fp32", True, device, ids, splits=0)
    total = lambda lse: lse.double().view(2, -1).sum(0)      # value + rounding remainder
    for splits in (0, 1, 2, 3):
        out = base if splits == 0 else run_infonce(v, t, s, "fp32", True, device, ids, splits=splits)
        d = float(((total(out["lse"]) - total(base["lse"])).abs() / total(base["lse"]).abs().clamp_min(1.0)).max())
        e = abs(float(out["loss"]) - ref["loss"])
        print(f"InfoNCE B={B} D={D} splits={splits}: lse rel {d:.3e} (bar 1e-6) loss {e:.3e} (bar {ic.loss_bar(ref):.3e})")
        assert d <= 1e-6 and e <= ic.loss_bar(ref)
        same_bits(run_infonce(v, t, s, "fp32", True, device, ids, splits=splits), out, f"InfoNCE splits={splits}")
    s, beta = sc.SCALE_BIAS[1]
    v, t, ids, ref = sigmoid_case("randn", B, D, 5, s, beta, "stride7")
    base = run_sigmoid(v, t, s, beta, "fp32", True, device, ids, splits=0)
    for splits in (0, 1, 2, 3):
        out = base if splits == 0 else run_sigmoid(v, t, s, beta, "fp32", True, device, ids, splits=splits)
        d = float(((out["row_loss"].double() - base["row_loss"].double()).abs() / base["row_loss"].double().abs().clamp_min(1.0)).max())
        e = abs(float(out["loss"]) - ref["loss"])
        print(f"sigmoid B={B} D={D} splits={splits}: row_loss rel {d:.3e} (bar 1e-6) loss {e:.3e} (bar {sc.loss_bar(ref):.3e})")
        assert d <= 1e-6 and e <= sc.loss_bar(ref)
        same_bits(run_sigmoid(v, t, s, beta, "fp32", True, device, ids, splits=splits), out, f"sigmoid splits={splits}")


def check_interface(device):
    """Check 8, the refusals and the modules' forward"""
    import pytest

    import crossclr_amd
    B, D = 8, 16
    v, t = (x.to(device) for x in ic.inputs("randn", B, D, 0))
    ids = ids_of("runs3", B).to(device)
    calls = (lambda p: crossclr_amd.info_nce_loss(v, t, pair_ids=p), lambda p: crossclr_amd.sigmoid_loss(v, t, pair_ids=p),
             lambda p: crossclr_amd.InfoNCE().to(device)(v, t, pair_ids=p), lambda p: crossclr_amd.SigmoidLoss().to(device)(v, t, p))
    for call in calls:
        with pytest.raises(RuntimeError, match="shape"):
            call(ids[:7])
        with pytest.raises(RuntimeError, match="shape"):
            call(ids.view(B, 1))
        with pytest.raises(RuntimeError, match="integer"):
            call(ids.float())
        with pytest.raises(RuntimeError, match="integer"):
            call(ids.bool())
        with pytest.raises(RuntimeError, match="pair_ids is on"):
            call(torch.empty(B, dtype=torch.int64, device="meta"))
        with pytest.raises(RuntimeError, match="requires_grad"):
            call(ids.float().requires_grad_())
        assert call(ids).dim() == 0 and torch.equal(call(ids), call(ids.to(torch.int32)))
    assert torch.equal(crossclr_amd.info_nce_loss(v, t, pair_ids=None), crossclr_amd.info_nce_loss(v, t))
    assert torch.equal(crossclr_amd.sigmoid_loss(v, t, pair_ids=None), crossclr_amd.sigmoid_loss(v, t))


def check_module_step(device, mode="fp32", B=257, D=72):
    """Check 8: gradients reach logit_scale (and logit_bias) with ids present, and one step is the definition's"""
    import crossclr_amd
    v, t = operands("randn", B, D, 2, False)
    ids = ids_of("runs3", B)
    m = crossclr_amd.InfoNCE(temperature=0.05, compute_mode=mode).to(device)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    before = m.logit_scale.detach().clone()
    m(v.to(device), t.to(device), pair_ids=ids.to(device)).backward()
    ref = infonce_definition(v, t, 20.0, True, ids, grad_out=1.0)
    assert abs(float(m.logit_scale.grad) - ref["gs"] * 20.0) <= 2e-4 * ref["A"] * 20.0 + 1e-6 * abs(ref["gs"] * 20.0)
    opt.step()
    assert not torch.equal(m.logit_scale.detach(), before)
    g = crossclr_amd.SigmoidLoss(compute_mode=mode).to(device)
    g(v.to(device), t.to(device), pair_ids=ids.to(device)).backward()
    ref = sigmoid_definition(v, t, 10.0, -10.0, True, ids, grad_out=1.0)
    assert abs(float(g.logit_scale.grad) - ref["gs"] * 10.0) <= 2e-4 * ref["A_s"] * 10.0 + 1e-6 * abs(ref["gs"] * 10.0)
    assert abs(float(g.logit_bias.grad) - ref["gb"]) <= 2e-4 * ref["A_b"]
    assert float(g.logit_scale.grad) != 0.0 and float(g.logit_bias.grad) != 0.0
