"""The symmetric InfoNCE loss with a device-resident logit scale: its dense float64 definition, the bars and the checks shared by
tests/test_infonce_cpu.py (emulated library) and tests/test_gpu_infonce.py (MI355X).  A helper module like tests/hardneg_cases.py:
pytest collects nothing here.

DEFINITION (float64, dense, autograd):  x^ = F.normalize(x) (normalize=True) or x (normalize=False),
    S = v^ t^T,  lr[i] = logsumexp_j s S[i, j],  lc[j] = logsumexp_i s S[i, j],  L = 1/(2B) sum_i (lr[i] + lc[i] - 2 s S[i, i])
    W[i, j] = exp(s S[i, j] - lr[i]) + exp(s S[i, j] - lc[j]) - 2 [i == j],   A = 1/(2B) sum_ij |W S|   (the scale of dL/ds)
evaluated at the fp32 value of s, which is what the kernels are handed (a float argument is written into a one-element fp32 tensor).
Gradients are those of grad_out * L with grad_out = 3.

BARS (1 / tau of the project's bars read as |s|; `rel` = max(2e-4, 4e-7 |s|) for fp32 / bf16x3, 1e-2 for bf16):
    loss      2e-5 max(1, |L|) + 2e-8 |s|
    gradients rel max|grad| + 1e-7 |s| / B          (max over the whole tensor of the definition's gradient)
    dL/ds     rel A
bf16 is compared with the definition on the SAME bf16-exact operands (exact sign rows, or F.normalize(x).bfloat16().float() fed with
normalize=False); bf16 with normalize=True against the exact definition has bars of its own (loss 1e-3, gradients and dL/ds 1e-2)."""
import torch
import torch.nn.functional as F

import exact_inputs as xi
from crossclr_amd import infonce as N
from oracle import crossclr_oracle as orc

MODES = ("fp32", "bf16x3", "bf16")
GRAD_OUT = 3.0
SHAPES = [(8, 16), (70, 48), (257, 72), (130, 200), (300, 40)]
EXACT_CASES = [("inter", 8, 16, 4), ("inter", 70, 48, 16), ("inter", 257, 72, None), ("inter", 130, 200, None), ("mixed", 300, 40, 16)]
EXACT_SCALE = 16.0
RANDOM_CASES = [(70, 48, 1), (257, 72, 2), (130, 200, 11), (300, 40, 5)]
SCALES = (1 / 0.07, 100.0)


def f32_value(s):
    return float(torch.tensor(float(s), dtype=torch.float32))


def definition(v, t, s, normalize, grad_out=GRAD_OUT):
    """loss, gradients of grad_out * loss, lr, lc, S[i, i] and A of the definition above on float64 copies of (v, t)."""
    a, b = v.detach().double().cpu().clone().requires_grad_(), t.detach().double().cpu().clone().requires_grad_()
    sc = torch.tensor(f32_value(s), dtype=torch.float64, requires_grad=True)
    B = a.shape[0]
    va, tb = (F.normalize(a, dim=1), F.normalize(b, dim=1)) if normalize else (a, b)
    S = va @ tb.t()
    Z = sc * S
    lr, lc = torch.logsumexp(Z, 1), torch.logsumexp(Z, 0)
    loss = (lr + lc - 2 * Z.diag()).sum() / (2 * B)
    (grad_out * loss).backward()
    with torch.no_grad():
        W = torch.exp(Z - lr[:, None]) + torch.exp(Z - lc[None, :]) - 2 * torch.eye(B, dtype=torch.float64)
        A = float((W * S).abs().sum() / (2 * B))
    return dict(loss=float(loss.detach()), gv=a.grad, gt=b.grad, gs=float(sc.grad), lr=lr.detach(), lc=lc.detach(), pair=S.detach().diag(),
                A=A, s=float(sc.detach()), B=B)


def rel_bar(mode, s):
    return 1e-2 if mode == "bf16" else max(2e-4, 4e-7 * abs(s))


def loss_bar(ref):
    return 2e-5 * max(1.0, abs(ref["loss"])) + 2e-8 * abs(ref["s"])


def run(v, t, s, mode, normalize, device, splits=0, grad_out=GRAD_OUT):
    """loss, gradients of grad_out * loss, lse [2, 2 bpad] (log2 domain: value, remainder) and pair [bpad] through `_info_nce` with a tensor scale on `device`"""
    a, b = v.detach().clone().to(device).requires_grad_(), t.detach().clone().to(device).requires_grad_()      # (fresh leaves: .grad accumulates)
    sc = torch.tensor(float(s), dtype=torch.float32, device=device, requires_grad=True)
    loss, lse, pair = N._info_nce(a, b, sc, normalize, mode, splits)
    (grad_out * loss).backward()
    return dict(loss=loss.detach(), gv=a.grad, gt=b.grad, gs=sc.grad, lse=lse, pair=pair)


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
    figures.append(("ds", abs(float(out["gs"]) - ref["gs"]), rel * ref["A"]))
    print(f"{what} {mode} s={s:.6g}: " + "  ".join(f"{k} {e:.3e} (bar {b:.3e})" for k, e, b in figures))
    for k, e, b in figures:
        assert e <= b, f"{what} {mode}: {k} off by {e:.3e}, bar {b:.3e}"
    return figures


def check_lse(out, ref, what):
    """lse (log2 domain) against the definition's lr / lc and the positive pairs' scores, at the loss bar per entry"""
    B, bpad = ref["B"], out["pair"].numel()
    assert out["lse"].numel() == 4 * bpad
    lse = (out["lse"][:2 * bpad].double() + out["lse"][2 * bpad:].double()).cpu() * 0.6931471805599453      # value + rounding remainder
    e_r, e_c = float((lse[:B] - ref["lr"]).abs().max()), float((lse[bpad:bpad + B] - ref["lc"]).abs().max())
    e_p = float((out["pair"].double().cpu()[:B] - ref["pair"]).abs().max())
    bar = 2e-5 * max(1.0, float(ref["lr"].abs().max()), float(ref["lc"].abs().max())) + 2e-8 * abs(ref["s"])
    print(f"{what}: lr {e_r:.3e} lc {e_c:.3e} (bar {bar:.3e}) pair {e_p:.3e}")
    assert e_r <= bar and e_c <= bar and e_p <= 2e-5 * max(1.0, float(ref["pair"].abs().max()))
    assert not out["lse"].view(4, bpad)[:, B:].any() and not out["pair"][B:].any(), "padding entries"


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def exact_case(kind, B, D, nnz):
    """inputs and the float64 definition of an exact-operand case (normalize=True, s = 16), made once"""
    def make():
        v, t = xi.planted(kind, B, D, nnz, seed=B + D)
        return v, t, definition(v, t, EXACT_SCALE, True)
    return cached(("exact", kind, B, D, nnz), make)


def check_exact_case(kind, B, D, nnz, device):
    """Case 1: rows and cosines are exact in all three modes: lse, pair and loss are the same bits in all of them (same accumulators, same
    epilogue), equal to float64 at the fp32 bars; gradients at each mode's bar."""
    v, t, ref = exact_case(kind, B, D, nnz)
    outs = {mode: run(v, t, EXACT_SCALE, mode, True, device) for mode in MODES}
    for mode in MODES[1:]:
        for key in ("lse", "pair", "loss"):
            assert torch.equal(outs[mode][key], outs["fp32"][key]), f"{key} differs between fp32 and {mode}"
    assert torch.equal(outs["fp32"]["pair"].double().cpu()[:B], ref["pair"])
    check_lse(outs["fp32"], ref, f"exact {kind} B={B} D={D}")
    for mode in MODES:
        check(outs[mode], ref, mode, f"exact {kind} B={B} D={D}")


def inputs(kind, B, D, seed):
    """"randn" / "cluster": the oracle's; "noisy": t = v + 2 n; "anti": t[B - 1 - i] = v[i] + 0.05 n (every row's maximum on the
    anti-diagonal: in a late tile for early rows, in an early tile for late rows)"""
    if kind in ("randn", "cluster"):
        return orc.make_inputs(kind, B, D, seed)
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, D, generator=g)
    n = torch.randn(B, D, generator=g)
    return (v, v + 2 * n) if kind == "noisy" else (v, (v + 0.05 * n).flip(0))


def reference_case(kind, B, D, seed, s, normalize, rounded=False):
    """(v, t, definition) made once; rounded: the operands are F.normalize(x).bfloat16().float(), used as given"""
    def make():
        v, t = inputs(kind, B, D, seed)
        if rounded:
            v, t = F.normalize(v, dim=1).bfloat16().float(), F.normalize(t, dim=1).bfloat16().float()
        return v, t, definition(v, t, s, normalize and not rounded)
    return cached((kind, B, D, seed, f32_value(s), normalize, rounded), make)


def check_case(kind, B, D, seed, s, mode, device, normalize=True):
    """Cases 2 and 4: fp32 / bf16x3 against the exact definition; bf16 on bf16-rounded unit rows fed with normalize=False"""
    rounded = mode == "bf16"
    v, t, ref = reference_case(kind, B, D, seed, s, normalize, rounded)
    out = run(v, t, s, mode, normalize and not rounded, device)
    check(out, ref, mode, f"{kind} B={B} D={D}")
    return out, ref


def check_bf16_normalized(B, D, seed, device):
    """Case 3: bf16 with normalize=True against the EXACT definition, s = 1 / 0.07: loss 1e-3, gradients and dL/ds 1e-2 (a float64
    model of the kernel -- bf16 operands, bf16 weights -- gives <= 4.9e-4 and <= 4.8e-3 on these four inputs)"""
    v, t, ref = reference_case("randn", B, D, seed, SCALES[0], True)
    out = run(v, t, SCALES[0], "bf16", True, device)
    check(out, ref, "bf16", f"randn normalize=True B={B} D={D}", loss_abs=1e-3, rel=1e-2)


def check_splits(B, D, device):
    """Case 7: every split count gives lse within 1e-6 relative and the loss within the fp32 bar; two runs with the same split count are
    the same bits in everything."""
    v, t, ref = reference_case("cluster", B, D, B + D, SCALES[0], True)
    base = run(v, t, SCALES[0], "fp32", True, device, splits=0)
    total = lambda lse: lse.double().view(2, -1).sum(0)      # value + rounding remainder
    for splits in (0, 1, 2, 3):
        out = base if splits == 0 else run(v, t, SCALES[0], "fp32", True, device, splits=splits)
        d = float(((total(out["lse"]) - total(base["lse"])).abs() / total(base["lse"]).abs().clamp_min(1.0)).max())
        e = abs(float(out["loss"]) - ref["loss"])
        print(f"B={B} D={D} splits={splits}: lse rel {d:.3e} (bar 1e-6) loss {e:.3e} (bar {loss_bar(ref):.3e})")
        assert d <= 1e-6 and e <= loss_bar(ref)
        again = run(v, t, SCALES[0], "fp32", True, device, splits=splits)
        for key in out:
            assert torch.equal(out[key], again[key]), (splits, key)
