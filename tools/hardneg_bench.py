#!/usr/bin/env python3
"""Timing of the hardest-negative (max_violation=True) ranking loss against the sum form's kernels it shares its tiled product with.

In ONE process on one device, for exact-fp32 and bf16 operands at (B, D) = (8192, 512) and (4096, 1024), HIP events around repeated
launches; the quantities of a group ALTERNATE window by window (warm-up, then `--reps` rounds of one window of `--inner` launches per
quantity; the median per quantity), so that clock and box drift fall on both sides of every ratio:
  forward    crossclr_hardneg_select + crossclr_hardneg_finish   against   crossclr_score_rows (the sum form's one-pass hinge mode: the
             same product, two compares, two adds and a mask-free epilogue per element).  Expectation: <= 1.10 x.
  backward   crossclr_hardneg_backward (an O(B D) gather)   against   crossclr_maxmargin_backward_saved (the sum form's product with the
             saved hinge mask, 8 B^2 D executed), alone and with its crossclr_maxmargin_backward_finish.  Expectation: several times faster.
  module     MaxMargin_coot(max_violation=True) forward + backward   against   MaxMargin_coot() forward + backward, end to end.
usage: hardneg_bench.py [--reps 7] [--inner 5]"""
import argparse, ctypes, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import crossclr_amd
from crossclr_amd import _native as nat, loss as L

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=5)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("hardneg_bench.py measures on the GPU: no device found")
lib, p = nat.library(), L._ptr
MARGIN = 0.1


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


def shape(B, D, mode, name):
    g = torch.Generator().manual_seed(1)
    v, t = torch.randn(B, D, generator=g).cuda(), torch.randn(B, D, generator=g).cuda()
    v, t = torch.nn.functional.normalize(v, dim=1), torch.nn.functional.normalize(t, dim=1)
    plan = nat.make_plan(B, D, 1, 0, mode); pp = ctypes.byref(plan)
    st = L._stream_for(v); f32 = dict(dtype=torch.float32, device="cuda")
    x = torch.empty(plan.operand_bytes, dtype=torch.uint8, device="cuda"); ones = torch.empty(2 * plan.bpad, **f32); dg = torch.empty(plan.bpad, **f32)
    nat.check(lib.crossclr_pack(pp, p(v), p(t), D, D, nat.IN_F32, p(x), p(ones), p(dg), st))
    # the sum form
    diag = torch.empty(2 * plan.bpad, **f32); part = torch.empty(plan.fwd_ws_floats, **f32)
    hinge, act = torch.empty(2 * plan.bpad, **f32), torch.empty(2 * plan.bpad, **f32)
    ls = torch.empty(plan.loss_ws_doubles, dtype=torch.float64, device="cuda")
    mask = torch.empty(lib.crossclr_maxmargin_mask_bytes(pp), dtype=torch.uint8, device="cuda")
    gbuf = torch.empty(plan.gbuf_bytes // 4, **f32)
    go = torch.ones(1, dtype=torch.float64, device="cuda")
    g_im, g_s = torch.empty_like(v), torch.empty_like(t)
    nat.check(lib.crossclr_score_diag(pp, p(x), p(diag), st))
    nat.check(lib.crossclr_score_rows_save(pp, p(x), p(diag), MARGIN, p(part), p(hinge), p(act), p(ls), p(mask), st))
    # the hardest-negative form
    ws = torch.empty(lib.crossclr_hardneg_workspace_bytes(pp, 0), dtype=torch.uint8, device="cuda")
    index = torch.empty(2 * plan.bpad, dtype=torch.int32, device="cuda")
    score, hn_hinge, pair = torch.empty(2 * plan.bpad, **f32), torch.empty(2 * plan.bpad, **f32), torch.empty(plan.bpad, **f32)
    hn_ls = torch.empty(plan.loss_ws_doubles, dtype=torch.float64, device="cuda")

    def select_finish():
        nat.check(lib.crossclr_hardneg_select(pp, p(x), 0, p(ws), ws.numel(), st))
        nat.check(lib.crossclr_hardneg_finish(pp, p(ws), 0, MARGIN, p(index), p(score), p(hn_hinge), p(pair), p(hn_ls), st))

    def saved_backward():
        nat.check(lib.crossclr_maxmargin_backward_saved(pp, p(x), p(mask), p(gbuf), st))

    def saved_backward_finish():
        saved_backward()
        nat.check(lib.crossclr_maxmargin_backward_finish(pp, p(gbuf), p(v), p(t), D, D, nat.IN_F32, p(ones), p(act), p(go), p(g_im), p(g_s), D, D, st))

    select_finish()
    print(f"  B={B} D={D} {name}: splits={lib.crossclr_hardneg_splits(pp, 0)} workspace={ws.numel() / 2**20:.1f} MiB, "
          f"saved for backward {4 * plan.bpad * 4 / 2**10:.0f} KiB (sum form: mask {mask.numel() / 2**20:.0f} MiB); "
          f"active hinges {int((hn_hinge > 0).sum())} of {2 * B}")
    fw = alternate({
        "score_rows": lambda: nat.check(lib.crossclr_score_rows(pp, p(x), p(diag), MARGIN, p(part), p(hinge), p(act), p(ls), st)),
        "score_rows_save": lambda: nat.check(lib.crossclr_score_rows_save(pp, p(x), p(diag), MARGIN, p(part), p(hinge), p(act), p(ls), p(mask), st)),
        "hardneg": select_finish,
        "hardneg_select": lambda: nat.check(lib.crossclr_hardneg_select(pp, p(x), 0, p(ws), ws.numel(), st)),
    })
    print(f"      crossclr_score_rows                 {fmt(fw['score_rows'])}")
    print(f"      crossclr_score_rows_save            {fmt(fw['score_rows_save'])}")
    print(f"      hardneg select + finish             {fmt(fw['hardneg'])}   (select alone {fw['hardneg_select'][0]:.3f} ms, "
          f"{2.0 * B * B * D / fw['hardneg_select'][0] / 1e9:.1f} TFLOP/s of the 2 B^2 D product)")
    r = fw["hardneg"][0] / fw["score_rows"][0]
    print(f"      select + finish = {r:.3f} x crossclr_score_rows (bound: <= 1.10) -- {'met' if r <= 1.10 else 'MISSED'}")
    select_finish()      # (the hinges the backward reads)
    bw = alternate({
        "saved": saved_backward,
        "saved_finish": saved_backward_finish,
        "hardneg": lambda: nat.check(lib.crossclr_hardneg_backward(pp, p(v), p(t), D, D, nat.IN_F32, p(index), p(hn_hinge), p(go), p(g_im), p(g_s), D, D, st)),
    })
    print(f"      crossclr_maxmargin_backward_saved   {fmt(bw['saved'])}")
    print(f"        ... + crossclr_maxmargin_backward_finish {fmt(bw['saved_finish'])}")
    print(f"      crossclr_hardneg_backward           {fmt(bw['hardneg'])}")
    print(f"      sum-form backward / hardest-negative backward = {bw['saved'][0] / bw['hardneg'][0]:.1f} x (saved product alone), "
          f"{bw['saved_finish'][0] / bw['hardneg'][0]:.1f} x (with its finish)")

    def module(criterion):
        a, b = v.clone().requires_grad_(), t.clone().requires_grad_()

        def step():
            a.grad = b.grad = None
            criterion(a, b).backward()
        return step
    md = alternate({"sum": module(crossclr_amd.MaxMargin_coot(margin=MARGIN, compute_mode=name)),
                    "hard": module(crossclr_amd.MaxMargin_coot(margin=MARGIN, compute_mode=name, max_violation=True))})
    print(f"      MaxMargin_coot() forward + backward                     {fmt(md['sum'])}")
    print(f"      MaxMargin_coot(max_violation=True) forward + backward   {fmt(md['hard'])}   ({md['sum'][0] / md['hard'][0]:.2f} x)")


print(f"device: {torch.cuda.get_device_name(0)}; reps={args.reps} x inner={args.inner}, median of alternating windows (HIP events)")
for mode, name in ((nat.MODE_FP32, "fp32"), (nat.MODE_BF16, "bf16")):
    print(f"compute_mode={name}")
    shape(8192, 512, mode, name)
    shape(4096, 1024, mode, name)
