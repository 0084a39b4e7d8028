#!/usr/bin/env python3
"""Timing and memory of the pairwise sigmoid loss against the InfoNCE kernels it shares its main loops with, and against eager PyTorch.

In ONE process on one device, for exact-fp32 and bf16 operands at (B, D) = (8192, 512) and (4096, 1024), HIP events around repeated
launches; the quantities of a group ALTERNATE window by window (warm-up, then `--reps` rounds of one window of `--inner` launches per
quantity; the median per quantity), so that clock and box drift fall on both sides of every ratio:
  forward    crossclr_sigmoid_stats + crossclr_sigmoid_finish   against   crossclr_infonce_stats + crossclr_infonce_finish (the same
             2 B^2 D product; soft-max statistics in both directions where this one has a softplus and a sigmoid per element)
  backward   crossclr_sigmoid_backward   against   crossclr_infonce_backward (the same skeleton and 8 B^2 D flops), alone and with their
             finish calls (one kernel, pairloss_backward_finish_kernel, with the divisor B or 2 B)
  module     SigmoidLoss forward + backward (unit rows in, normalize=True, s = 10, beta = -10)   against   eager PyTorch doing the same
             loss (F.normalize, mm, F.logsigmoid): fp32 against fp32 eager, bf16 against eager under torch.autocast(bfloat16)
  memory     torch.cuda.max_memory_allocated above the inputs for one fused step and for one eager step
usage: sigmoid_bench.py [--reps 7] [--inner 5]"""
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
    sys.exit("sigmoid_bench.py measures on the GPU: no device found")
lib, p = nat.library(), L._ptr
SCALE, BIAS = 10.0, -10.0


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


def eager_loss(v, t, s, beta, autocast):
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        logits = s * F.normalize(v, dim=1).mm(F.normalize(t, dim=1).t()) + beta
        labels = 2 * torch.eye(v.shape[0], device=v.device, dtype=logits.dtype) - 1
        return -F.logsigmoid(labels * logits).sum() / v.shape[0]


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
    f64 = dict(dtype=torch.float64, device="cuda")
    x = torch.empty(plan.operand_bytes, dtype=torch.uint8, device="cuda"); ones = torch.empty(2 * plan.bpad, **f32); dg = torch.empty(plan.bpad, **f32)
    nat.check(lib.crossclr_pack(pp, p(v), p(t), D, D, nat.IN_F32, p(x), p(ones), p(dg), st))
    scale, bias = torch.full((1,), SCALE, **f32), torch.full((1,), BIAS, **f32)
    gbuf = torch.empty(plan.gbuf_bytes // 4, **f32)
    go = torch.ones(1, **f64)
    g_v, g_t = torch.empty_like(v), torch.empty_like(t)
    dscale = torch.empty(plan.loss_ws_doubles, **f64)
    # InfoNCE (at the same scale)
    nws = torch.empty(lib.crossclr_infonce_workspace_bytes(pp, 0), dtype=torch.uint8, device="cuda")
    lse, npair = torch.empty(4 * plan.bpad, **f32), torch.empty(plan.bpad, **f32)
    nls = torch.empty(plan.loss_ws_doubles, **f64)
    # sigmoid
    ws = torch.empty(lib.crossclr_sigmoid_workspace_bytes(pp, 0), dtype=torch.uint8, device="cuda")
    row_loss, pair = torch.empty(plan.bpad, **f32), torch.empty(plan.bpad, **f32)
    sls, sgs = torch.empty(plan.loss_ws_doubles, **f64), torch.empty(plan.loss_ws_doubles, **f64)

    def n_stats():
        nat.check(lib.crossclr_infonce_stats(pp, p(x), p(scale), 0, p(nws), nws.numel(), st))

    def n_stats_finish():
        n_stats()
        nat.check(lib.crossclr_infonce_finish(pp, p(nws), 0, p(scale), p(lse), p(npair), p(nls), st))

    def n_backward():
        nat.check(lib.crossclr_infonce_backward(pp, p(x), p(scale), p(lse), p(npair), p(gbuf), st))

    def n_backward_finish():
        n_backward()
        nat.check(lib.crossclr_infonce_backward_finish(pp, p(gbuf), p(v), p(t), D, D, nat.IN_F32, p(ones), 0, p(scale), p(go), p(g_v), p(g_t), D, D,
                                                       p(dscale), st))

    def s_stats():
        nat.check(lib.crossclr_sigmoid_stats(pp, p(x), p(scale), p(bias), 0, p(ws), ws.numel(), st))

    def s_stats_finish():
        s_stats()
        nat.check(lib.crossclr_sigmoid_finish(pp, p(ws), 0, p(scale), p(bias), p(row_loss), p(pair), p(sls), p(sgs), st))

    def s_backward():
        nat.check(lib.crossclr_sigmoid_backward(pp, p(x), p(scale), p(bias), p(gbuf), st))

    def s_backward_finish():
        s_backward()
        nat.check(lib.crossclr_sigmoid_backward_finish(pp, p(gbuf), p(v), p(t), D, D, nat.IN_F32, p(ones), 0, p(scale), p(go), p(g_v), p(g_t), D, D,
                                                       p(dscale), st))

    n_stats_finish()
    s_stats_finish()
    print(f"  B={B} D={D} {name}: splits={lib.crossclr_sigmoid_splits(pp, 0)} workspace={ws.numel() / 2**20:.1f} MiB (InfoNCE {nws.numel() / 2**20:.1f}), "
          f"gradient slices={plan.bwd_slices} ({plan.gbuf_bytes / 2**20:.0f} MiB), operand {plan.operand_bytes / 2**20:.0f} MiB; loss {float(sls[1]):.6f}")
    fw = alternate({"infonce": n_stats_finish, "sigmoid": s_stats_finish, "infonce_stats": n_stats, "sigmoid_stats": s_stats})
    print(f"      infonce stats + finish              {fmt(fw['infonce'])}   (stats alone {fw['infonce_stats'][0]:.3f} ms)")
    print(f"      sigmoid stats + finish              {fmt(fw['sigmoid'])}   (stats alone {fw['sigmoid_stats'][0]:.3f} ms, "
          f"{2.0 * B * B * D / fw['sigmoid_stats'][0] / 1e9:.1f} TFLOP/s of the 2 B^2 D product)")
    print(f"      sigmoid stats + finish = {fw['sigmoid'][0] / fw['infonce'][0]:.3f} x infonce stats + finish")
    bw = alternate({"infonce": n_backward, "infonce_finish": n_backward_finish, "sigmoid": s_backward, "sigmoid_finish": s_backward_finish})
    print(f"      crossclr_infonce_backward           {fmt(bw['infonce'])}")
    print(f"        ... + crossclr_infonce_backward_finish   {fmt(bw['infonce_finish'])}")
    print(f"      crossclr_sigmoid_backward           {fmt(bw['sigmoid'])}   ({8.0 * B * B * D / bw['sigmoid'][0] / 1e9:.1f} TFLOP/s of 8 B^2 D)")
    print(f"        ... + crossclr_sigmoid_backward_finish   {fmt(bw['sigmoid_finish'])}")
    print(f"      sigmoid backward = {bw['sigmoid'][0] / bw['infonce'][0]:.3f} x crossclr_infonce_backward; with finish "
          f"{bw['sigmoid_finish'][0] / bw['infonce_finish'][0]:.3f} x")

    a, b = v.clone().requires_grad_(), t.clone().requires_grad_()
    s = torch.tensor(SCALE, **f32).requires_grad_()
    beta = torch.tensor(BIAS, **f32).requires_grad_()
    crit = crossclr_amd.SigmoidLoss(SCALE, BIAS, compute_mode=name).cuda()

    def clear():
        a.grad = b.grad = s.grad = beta.grad = crit.logit_scale.grad = crit.logit_bias.grad = None

    def fused():
        clear()
        crit(a, b).backward()

    def eager():
        clear()
        eager_loss(a, b, s, beta, name == "bf16").backward()
    md = alternate({"fused": fused, "eager": eager})
    print(f"      SigmoidLoss forward + backward      {fmt(md['fused'])}")
    print(f"      eager PyTorch ({'autocast bf16' if name == 'bf16' else 'fp32'}) fwd + bwd    {fmt(md['eager'])}   (eager / fused = {md['eager'][0] / md['fused'][0]:.2f} x)")
    clear()
    m_fused, m_eager = peak_above_inputs(fused), peak_above_inputs(eager)
    clear()
    print(f"      max_memory_allocated above the inputs: fused {m_fused:.0f} MiB, eager {m_eager:.0f} MiB  (one B x B fp32 matrix: {B * B * 4 / 2**20:.0f} MiB;"
          f" fused = {m_fused / (B * B * 4 / 2**20):.2f} of it)")


print(f"device: {torch.cuda.get_device_name(0)}; reps={args.reps} x inner={args.inner}, median of alternating windows (HIP events)")
for mode, name in ((nat.MODE_FP32, "fp32"), (nat.MODE_BF16, "bf16")):
    print(f"compute_mode={name}")
    for sh in args.shapes.split(","):
        B, D = (int(x) for x in sh.split("x"))
        shape(B, D, mode, name)
