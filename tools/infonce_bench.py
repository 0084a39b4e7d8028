#!/usr/bin/env python3
"""Timing and memory of the symmetric InfoNCE loss against the kernels it shares its tiled product with, and against eager PyTorch.

In ONE process on one device, for exact-fp32 and bf16 operands at (B, D) = (8192, 512) and (4096, 1024), HIP events around repeated
launches; the quantities of a group ALTERNATE window by window (warm-up, then `--reps` rounds of one window of `--inner` launches per
quantity; the median per quantity), so that clock and box drift fall on both sides of every ratio:
  forward    crossclr_infonce_stats + crossclr_infonce_finish   against   crossclr_score_rows (the same 2 B^2 D product with a hinge epilogue)
  backward   crossclr_infonce_backward (scores a second time + the gradient product: 8 B^2 D)   against   crossclr_maxmargin_backward
             (the same skeleton and flops, indicator weights), alone and with their finish kernels
  module     InfoNCE forward + backward (unit rows in, normalize=True, s = 1 / 0.07)   against   eager PyTorch doing the same loss
             (F.normalize, mm, two cross_entropy): fp32 against fp32 eager, bf16 against eager under torch.autocast(bfloat16)
  memory     torch.cuda.max_memory_allocated above the inputs for one fused step and for one eager step
usage: infonce_bench.py [--reps 7] [--inner 5]"""
import argparse, ctypes, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import crossclr_amd
from crossclr_amd import _native as nat, loss as L

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--shapes", default="8192x512,4096x1024")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("infonce_bench.py measures on the GPU: no device found")
lib, p = nat.library(), L._ptr
SCALE = 1 / 0.07


def alternate(fns):
    """fns: name -> callable.  name -> (median, min, max) ms per launch over args.reps windows of args.inner launches, the windows of the
    different callables taking turns"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / args.inner)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def fmt(t):
    return f"{t[0]:8.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def eager_loss(v, t, s, autocast):
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        logits = s * F.normalize(v, dim=1).mm(F.normalize(t, dim=1).t())
        labels = torch.arange(v.shape[0], device=v.device)
        return 0.5 * (F.cross_entropy(logits, labels) + F.cross_entropy(logits.t(), labels))


def peak_above_inputs(step):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def shape(B, D, mode, name):
    g = torch.Generator().manual_seed(1)
    v, t = torch.randn(B, D, generator=g).cuda(), torch.randn(B, D, generator=g).cuda()
    v, t = F.normalize(v, dim=1), F.normalize(t, dim=1)
    plan = nat.make_plan(B, D, 1, 0, mode); pp = ctypes.byref(plan)
    st = L._stream_for(v); f32 = dict(dtype=torch.float32, device="cuda")
    x = torch.empty(plan.operand_bytes, dtype=torch.uint8, device="cuda"); ones = torch.empty(2 * plan.bpad, **f32); dg = torch.empty(plan.bpad, **f32)
    nat.check(lib.crossclr_pack(pp, p(v), p(t), D, D, nat.IN_F32, p(x), p(ones), p(dg), st))
    scale = torch.full((1,), SCALE, **f32)
    # the max-margin sum form: the same product, another epilogue
    diag = torch.empty(2 * plan.bpad, **f32); part = torch.empty(plan.fwd_ws_floats, **f32)
    hinge, act = torch.empty(2 * plan.bpad, **f32), torch.empty(2 * plan.bpad, **f32)
    ls = torch.empty(plan.loss_ws_doubles, dtype=torch.float64, device="cuda")
    gbuf = torch.empty(plan.gbuf_bytes // 4, **f32)
    go = torch.ones(1, dtype=torch.float64, device="cuda")
    g_v, g_t = torch.empty_like(v), torch.empty_like(t)
    nat.check(lib.crossclr_score_diag(pp, p(x), p(diag), st))
    # InfoNCE
    ws = torch.empty(lib.crossclr_infonce_workspace_bytes(pp, 0), dtype=torch.uint8, device="cuda")
    lse, pair = torch.empty(4 * plan.bpad, **f32), torch.empty(plan.bpad, **f32)
    nls = torch.empty(plan.loss_ws_doubles, dtype=torch.float64, device="cuda")
    dscale = torch.empty(plan.loss_ws_doubles, dtype=torch.float64, device="cuda")

    def stats():
        nat.check(lib.crossclr_infonce_stats(pp, p(x), p(scale), 0, p(ws), ws.numel(), st))

    def stats_finish():
        stats()
        nat.check(lib.crossclr_infonce_finish(pp, p(ws), 0, p(scale), p(lse), p(pair), p(nls), st))

    def backward():
        nat.check(lib.crossclr_infonce_backward(pp, p(x), p(scale), p(lse), p(pair), p(gbuf), st))

    def backward_finish():
        backward()
        nat.check(lib.crossclr_infonce_backward_finish(pp, p(gbuf), p(v), p(t), D, D, nat.IN_F32, p(ones), 0, p(scale), p(go), p(g_v), p(g_t), D, D,
                                                       p(dscale), st))

    def mm_backward():
        nat.check(lib.crossclr_maxmargin_backward(pp, p(x), p(diag), 0.1, p(gbuf), st))

    def mm_backward_finish():
        mm_backward()
        nat.check(lib.crossclr_maxmargin_backward_finish(pp, p(gbuf), p(v), p(t), D, D, nat.IN_F32, p(ones), p(act), p(go), p(g_v), p(g_t), D, D, st))

    nat.check(lib.crossclr_score_rows(pp, p(x), p(diag), 0.1, p(part), p(hinge), p(act), p(ls), st))
    stats_finish()
    print(f"  B={B} D={D} {name}: splits={lib.crossclr_infonce_splits(pp, 0)} workspace={ws.numel() / 2**20:.1f} MiB, gradient slices={plan.bwd_slices} "
          f"({plan.gbuf_bytes / 2**20:.0f} MiB), operand {plan.operand_bytes / 2**20:.0f} MiB; loss {float(nls[1]):.6f}")
    fw = alternate({
        "score_rows": lambda: nat.check(lib.crossclr_score_rows(pp, p(x), p(diag), 0.1, p(part), p(hinge), p(act), p(ls), st)),
        "infonce": stats_finish,
        "stats": stats,
    })
    print(f"      crossclr_score_rows                 {fmt(fw['score_rows'])}")
    print(f"      infonce stats + finish              {fmt(fw['infonce'])}   (stats alone {fw['stats'][0]:.3f} ms, "
          f"{2.0 * B * B * D / fw['stats'][0] / 1e9:.1f} TFLOP/s of the 2 B^2 D product)")
    print(f"      stats + finish = {fw['infonce'][0] / fw['score_rows'][0]:.3f} x crossclr_score_rows")
    bw = alternate({"maxmargin": mm_backward, "maxmargin_finish": mm_backward_finish, "infonce": backward, "infonce_finish": backward_finish})
    print(f"      crossclr_maxmargin_backward         {fmt(bw['maxmargin'])}")
    print(f"        ... + crossclr_maxmargin_backward_finish {fmt(bw['maxmargin_finish'])}")
    print(f"      crossclr_infonce_backward           {fmt(bw['infonce'])}   ({8.0 * B * B * D / bw['infonce'][0] / 1e9:.1f} TFLOP/s of 8 B^2 D)")
    print(f"        ... + crossclr_infonce_backward_finish   {fmt(bw['infonce_finish'])}")
    print(f"      infonce backward = {bw['infonce'][0] / bw['maxmargin'][0]:.3f} x crossclr_maxmargin_backward")

    a, b = v.clone().requires_grad_(), t.clone().requires_grad_()
    s = torch.tensor(SCALE, **f32).requires_grad_()
    crit = crossclr_amd.InfoNCE(temperature=0.07, compute_mode=name).cuda()

    def fused():
        a.grad = b.grad = crit.logit_scale.grad = None
        crit(a, b).backward()

    def eager():
        a.grad = b.grad = s.grad = None
        eager_loss(a, b, s, name == "bf16").backward()
    md = alternate({"fused": fused, "eager": eager})
    print(f"      InfoNCE forward + backward          {fmt(md['fused'])}")
    print(f"      eager PyTorch ({'autocast bf16' if name == 'bf16' else 'fp32'}) fwd + bwd    {fmt(md['eager'])}   (eager / fused = {md['eager'][0] / md['fused'][0]:.2f} x)")
    a.grad = b.grad = s.grad = crit.logit_scale.grad = None
    m_fused, m_eager = peak_above_inputs(fused), peak_above_inputs(eager)
    a.grad = b.grad = s.grad = crit.logit_scale.grad = None
    print(f"      max_memory_allocated above the inputs: fused {m_fused:.0f} MiB, eager {m_eager:.0f} MiB  (one B x B fp32 matrix: {B * B * 4 / 2**20:.0f} MiB;"
          f" fused = {m_fused / (B * B * 4 / 2**20):.2f} of it)")


print(f"device: {torch.cuda.get_device_name(0)}; reps={args.reps} x inner={args.inner}, median of alternating windows (HIP events)")
for mode, name in ((nat.MODE_FP32, "fp32"), (nat.MODE_BF16, "bf16")):
    print(f"compute_mode={name}")
    for sh in args.shapes.split(","):
        B, D = (int(x) for x in sh.split("x"))
        shape(B, D, mode, name)
