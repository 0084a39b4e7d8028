"""The pairwise sigmoid loss with a device-resident logit scale and bias: its dense float64 definition, the bars and the checks shared by
tests/test_sigmoid_cpu.py (emulated library) and tests/test_gpu_sigmoid.py (MI355X).  A helper module like tests/infonce_cases.py:
pytest collects nothing here.

DEFINITION (float64, dense, autograd):  x^ = F.normalize(x) (normalize=True) or x (normalize=False),
    S = v^ t^T,  z = s S + beta,  y = 2 I - 1,  L = -1/B sum_ij logsigmoid(y_ij z_ij)
      = 1/B [ sum_i softplus(-z_ii) + sum_{i != j} softplus(z_ij) ],   row_loss[i] = -sum_j logsigmoid(y_ij z_ij)
    W = sigmoid(z) - I,   A_s = 1/B sum_ij |W S|  (the scale of dL/ds),   A_b = 1/B sum_ij |W|  (the scale of dL/dbeta)
evaluated at the fp32 values of s and beta, which is what the kernels are handed (a float argument is written into a one-element fp32
tensor).  Gradients are those of grad_out * L with grad_out = 3.

BARS (the project's, from tests/infonce_cases.py; `rel` = max(2e-4, 4e-7 |s|) for fp32 / bf16x3, 1e-2 for bf16):
    loss       2e-5 max(1, |L|) + 2e-8 (|s| + |beta|)
    gradients  rel max|grad| + 1e-7 |s| / B          (max over the whole tensor of the definition's gradient)
    dL/ds      rel A_s
    dL/dbeta   rel A_b
    row_loss   2e-5 max(1, max|row_loss|) + 2e-8 (|s| + |beta|), per entry
bf16 is compared with the definition on the SAME bf16-exact operands (exact sign rows, or F.normalize(x).bfloat16().float() fed with
normalize=False); bf16 with normalize=True against the exact definition has bars of its own (loss 1e-3, gradients, dL/ds and dL/dbeta
1e-2)."""
import torch
import torch.nn.functional as F

import exact_inputs as xi
from crossclr_amd import sigmoid as G
from infonce_cases import f32_value, inputs

MODES = ("fp32", "bf16x3", "bf16")
GRAD_OUT = 3.0
SHAPES = [(8, 16), (70, 48), (257, 72), (130, 200), (300, 40)]
EXACT_CASES = [("inter", 8, 16, 4), ("inter", 70, 48, 16), ("inter", 257, 72, None), ("inter", 130, 200, None), ("mixed", 300, 40, 16)]
EXACT_SB = (16.0, -8.0)
RANDOM_CASES = [(70, 48, 1), (257, 72, 2), (130, 200, 11), (300, 40, 5)]
SCALE_BIAS = ((10.0, -10.0), (1 / 0.07, -3.0), (100.0, -10.0), (100.0, 0.0))      # (SigLIP's initial values first)


def definition(v, t, s, beta, normalize, grad_out=GRAD_OUT):
    """loss, gradients of grad_out * loss, row_loss, S[i, i], A_s and A_b of the definition above on float64 copies of (v, t)."""
    a, b = v.detach().double().cpu().clone().requires_grad_(), t.detach().double().cpu().clone().requires_grad_()
    sc = torch.tensor(f32_value(s), dtype=torch.float64, requires_grad=True)
    bc = torch.tensor(f32_value(beta), dtype=torch.float64, requires_grad=True)
    B = a.shape[0]
    va, tb = (F.normalize(a, dim=1), F.normalize(b, dim=1)) if normalize else (a, b)
    S = va @ tb.t()
    Z = sc * S + bc
    eye = torch.eye(B, dtype=torch.float64)
    terms = -F.logsigmoid((2 * eye - 1) * Z)
    loss = terms.sum() / B
    (grad_out * loss).backward()
    with torch.no_grad():
        W = torch.sigmoid(Z) - eye
        W[eye.bool()] = -torch.sigmoid(-Z.diag())      # (not sigma(z) - 1: that cancels)
        A_s, A_b = float((W * S).abs().sum() / B), float(W.abs().sum() / B)
    return dict(loss=float(loss.detach()), gv=a.grad, gt=b.grad, gs=float(sc.grad), gb=float(bc.grad), row_loss=terms.detach().sum(1),
                pair=S.detach().diag(), A_s=A_s, A_b=A_b, s=float(sc.detach()), beta=float(bc.detach()), B=B)


def rel_bar(mode, s):
    return 1e-2 if mode == "bf16" else max(2e-4, 4e-7 * abs(s))


def loss_bar(ref):
    return 2e-5 * max(1.0, abs(ref["loss"])) + 2e-8 * (abs(ref["s"]) + abs(ref["beta"]))


def run(v, t, s, beta, mode, normalize, device, splits=0, grad_out=GRAD_OUT):
    """loss, gradients of grad_out * loss, row_loss [bpad] and pair [bpad] through `_sigmoid` with a tensor scale and bias on `device`"""
    a, b = v.detach().clone().to(device).requires_grad_(), t.detach().clone().to(device).requires_grad_()      # (fresh leaves: .grad accumulates)
    sc = torch.tensor(float(s), dtype=torch.float32, device=device, requires_grad=True)
    bc = torch.tensor(float(beta), dtype=torch.float32, device=device, requires_grad=True)
    loss, row_loss, pair = G._sigmoid(a, b, sc, bc, normalize, mode, splits)
    (grad_out * loss).backward()
    return dict(loss=loss.detach(), gv=a.grad, gt=b.grad, gs=sc.grad, gb=bc.grad, row_loss=row_loss, pair=pair)


def check(out, ref, mode, what, loss_abs=None, rel=None, skip_rows=()):
    """`out` of `run` against `ref` of `definition` at the bars of the module docstring (loss_abs / rel: the bars of bf16 against the
    exact definition); prints every figure beside its bar before it asserts.  skip_rows: rows left to the caller."""
    s, B = ref["s"], ref["B"]
    rel = rel_bar(mode, s) if rel is None else rel
    figures = []
    e_loss, b_loss = abs(float(out["loss"]) - ref["loss"]), (loss_bar(ref) if loss_abs is None else loss_abs)
    figures.append(("loss", e_loss, b_loss))
    keep = torch.ones(B, dtype=torch.bool)
    keep[list(skip_rows)] = False
    for key in ("gv", "gt"):
        want = ref[key][keep]
        got = out[key].detach().double().cpu()[keep]
        assert torch.isfinite(got).all(), (what, key)
        figures.append((key, float((got - want).abs().max()), rel * float(want.abs().max()) + 1e-7 * abs(s) / B))
    figures.append(("ds", abs(float(out["gs"]) - ref["gs"]), rel * ref["A_s"]))
    figures.append(("dbeta", abs(float(out["gb"]) - ref["gb"]), rel * ref["A_b"]))
    print(f"{what} {mode} s={s:.6g} beta={ref['beta']:.6g}: " + "  ".join(f"{k} {e:.3e} (bar {b:.3e})" for k, e, b in figures))
    for k, e, b in figures:
        assert e <= b, f"{what} {mode}: {k} off by {e:.3e}, bar {b:.3e}"
    return figures


def check_rows(out, ref, what):
    """row_loss (nats) against the definition's, per entry, and the positive pairs' scores; padding entries are 0"""
    B, bpad = ref["B"], out["pair"].numel()
    assert out["row_loss"].numel() == bpad and bpad % 128 == 0
    e_r = float((out["row_loss"].double().cpu()[:B] - ref["row_loss"]).abs().max())
    e_p = float((out["pair"].double().cpu()[:B] - ref["pair"]).abs().max())
    bar = 2e-5 * max(1.0, float(ref["row_loss"].abs().max())) + 2e-8 * (abs(ref["s"]) + abs(ref["beta"]))
    print(f"{what}: row_loss {e_r:.3e} (bar {bar:.3e}) pair {e_p:.3e}")
    assert e_r <= bar and e_p <= 2e-5 * max(1.0, float(ref["pair"].abs().max()))
    assert not out["row_loss"][B:].any() and not out["pair"][B:].any(), "padding entries"


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def exact_case(kind, B, D, nnz):
    """inputs and the float64 definition of an exact-operand case (normalize=True, (s, beta) = EXACT_SB), made once"""
    def make():
        v, t = xi.planted(kind, B, D, nnz, seed=B + D)
        return v, t, definition(v, t, *EXACT_SB, True)
    return cached(("exact", kind, B, D, nnz), make)


def check_exact_outputs(v, t, ref, device, what):
    """Rows and cosines are exact in all three modes: loss, row_loss and pair are the same bits in all of them (same accumulators, same
    epilogue), equal to float64 at the fp32 bars; gradients at each mode's bar."""
    outs = {mode: run(v, t, *EXACT_SB, mode, True, device) for mode in MODES}
    for mode in MODES[1:]:
        for key in ("loss", "row_loss", "pair"):
            assert torch.equal(outs[mode][key], outs["fp32"][key]), f"{key} differs between fp32 and {mode}"
    assert torch.equal(outs["fp32"]["pair"].double().cpu()[:ref["B"]], ref["pair"])
    check_rows(outs["fp32"], ref, what)
    for mode in MODES:
        check(outs[mode], ref, mode, what)


def check_exact_case(kind, B, D, nnz, device):
    v, t, ref = exact_case(kind, B, D, nnz)
    check_exact_outputs(v, t, ref, device, f"exact {kind} B={B} D={D}")


def reference_case(kind, B, D, seed, s, beta, normalize, rounded=False):
    """(v, t, definition) made once; kinds: those of infonce_cases.inputs ("randn", "cluster", "noisy": t = v + 2 n, "anti": every row's
    positive-looking score on the anti-diagonal); rounded: the operands are F.normalize(x).bfloat16().float(), used as given"""
    def make():
        v, t = inputs(kind, B, D, seed)
        if rounded:
            v, t = F.normalize(v, dim=1).bfloat16().float(), F.normalize(t, dim=1).bfloat16().float()
        return v, t, definition(v, t, s, beta, normalize and not rounded)
    return cached((kind, B, D, seed, f32_value(s), f32_value(beta), normalize, rounded), make)


def check_case(kind, B, D, seed, s, beta, mode, device, normalize=True):
    """fp32 / bf16x3 against the exact definition; bf16 on bf16-rounded unit rows fed with normalize=False"""
    rounded = mode == "bf16"
    v, t, ref = reference_case(kind, B, D, seed, s, beta, normalize, rounded)
    out = run(v, t, s, beta, mode, normalize and not rounded, device)
    check(out, ref, mode, f"{kind} B={B} D={D}")
    return out, ref


def check_bf16_normalized(B, D, seed, device):
    """bf16 with normalize=True against the EXACT definition at SigLIP's initial values: loss 1e-3, gradients, dL/ds and dL/dbeta 1e-2"""
    s, beta = SCALE_BIAS[0]
    v, t, ref = reference_case("randn", B, D, seed, s, beta, True)
    out = run(v, t, s, beta, "bf16", True, device)
    check(out, ref, "bf16", f"randn normalize=True B={B} D={D}", loss_abs=1e-3, rel=1e-2)


def check_splits(B, D, device):
    """Every split count gives row_loss within 1e-6 relative and the loss within the fp32 bar; two runs with the same split count are
    the same bits in everything."""
    s, beta = SCALE_BIAS[1]
    v, t, ref = reference_case("cluster", B, D, B + D, s, beta, True)
    base = run(v, t, s, beta, "fp32", True, device, splits=0)
    for splits in (0, 1, 2, 3):
        out = base if splits == 0 else run(v, t, s, beta, "fp32", True, device, splits=splits)
        d = float(((out["row_loss"].double() - base["row_loss"].double()).abs() / base["row_loss"].double().abs().clamp_min(1.0)).max())
        e = abs(float(out["loss"]) - ref["loss"])
        print(f"B={B} D={D} splits={splits}: row_loss rel {d:.3e} (bar 1e-6) loss {e:.3e} (bar {loss_bar(ref):.3e})")
        assert d <= 1e-6 and e <= loss_bar(ref)
        again = run(v, t, s, beta, "fp32", True, device, splits=splits)
        for key in out:
            assert torch.equal(out[key], again[key]), (splits, key)
