#!/usr/bin/env python3
"""What pair_ids cost: the _ids kernels of the InfoNCE and the sigmoid loss against the plain kernels OF THE SAME RUN.

In ONE process on one device, for exact-fp32 and bf16 operands at (B, D) = (8192, 512) and (4096, 1024), HIP events around repeated
launches; the quantities of a group ALTERNATE window by window (warm-up, then `--reps` rounds of one window of `--inner` launches per
quantity; the median per quantity), so that clock and box drift fall on both sides of every ratio:
  forward    stats + finish:   crossclr_{infonce,sigmoid}_stats      against   crossclr_{infonce,sigmoid}_stats_ids, each followed by its finish
  backward   the gradient product:   crossclr_{infonce,sigmoid}_backward   against   crossclr_{infonce,sigmoid}_backward_ids
  groups     crossclr_pair_groups alone (int64 ids -> int32 groups, once per step)
with two id vectors: all distinct (nothing excluded: what the masking itself costs) and ids = i // 4 (three exclusions per row).
The target is ids / plain <= 1.10 (what the hardest-negative selection epilogue was accepted at against its baseline).
usage: pair_ids_bench.py [--reps 7] [--inner 5]"""
import argparse, ctypes, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from crossclr_amd import _native as nat, loss as L

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--shapes", default="8192x512,4096x1024")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("pair_ids_bench.py measures on the GPU: no device found")
lib, p = nat.library(), L._ptr
SCALE, BIAS = 1 / 0.07, -10.0


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


def report(title, res):
    print(f"      {title:<28} plain        {fmt(res['plain'])}")
    for k in ("distinct", "by4"):
        print(f"      {'':<28} ids {k:<8} {fmt(res[k])}   ids / plain = {res[k][0] / res['plain'][0]:.3f}")


def shape(B, D, mode, name):
    g = torch.Generator().manual_seed(1)
    v, t = torch.randn(B, D, generator=g).cuda(), torch.randn(B, D, generator=g).cuda()
    v, t = F.normalize(v, dim=1), F.normalize(t, dim=1)
    plan = nat.make_plan(B, D, 1, 0, mode); pp = ctypes.byref(plan)
    st = L._stream_for(v); f32 = dict(dtype=torch.float32, device="cuda")
    x = torch.empty(plan.operand_bytes, dtype=torch.uint8, device="cuda"); ones = torch.empty(2 * plan.bpad, **f32); dg = torch.empty(plan.bpad, **f32)
    nat.check(lib.crossclr_pack(pp, p(v), p(t), D, D, nat.IN_F32, p(x), p(ones), p(dg), st))
    scale, bias = torch.full((1,), SCALE, **f32), torch.full((1,), BIAS, **f32)
    ids = {"distinct": torch.arange(B, device="cuda"), "by4": torch.arange(B, device="cuda") // 4}
    groups = {k: torch.empty(plan.bpad, dtype=torch.int32, device="cuda") for k in ids}
    for k in ids:
        nat.check(lib.crossclr_pair_groups(pp, p(ids[k]), p(groups[k]), st))
    gbuf = torch.empty(plan.gbuf_bytes // 4, **f32)
    nws = torch.empty(lib.crossclr_infonce_workspace_bytes(pp, 0), dtype=torch.uint8, device="cuda")
    gws = torch.empty(lib.crossclr_sigmoid_workspace_bytes(pp, 0), dtype=torch.uint8, device="cuda")
    lse, pair, row_loss = torch.empty(4 * plan.bpad, **f32), torch.empty(plan.bpad, **f32), torch.empty(plan.bpad, **f32)
    ls, sg = (torch.empty(plan.loss_ws_doubles, dtype=torch.float64, device="cuda") for _ in range(2))

    def infonce_fwd(group):
        if group is None:
            nat.check(lib.crossclr_infonce_stats(pp, p(x), p(scale), 0, p(nws), nws.numel(), st))
        else:
            nat.check(lib.crossclr_infonce_stats_ids(pp, p(x), p(scale), p(group), 0, p(nws), nws.numel(), st))
        nat.check(lib.crossclr_infonce_finish(pp, p(nws), 0, p(scale), p(lse), p(pair), p(ls), st))

    def infonce_bwd(group):
        if group is None:
            nat.check(lib.crossclr_infonce_backward(pp, p(x), p(scale), p(lse), p(pair), p(gbuf), st))
        else:
            nat.check(lib.crossclr_infonce_backward_ids(pp, p(x), p(scale), p(lse), p(pair), p(group), p(gbuf), st))

    def sigmoid_fwd(group):
        if group is None:
            nat.check(lib.crossclr_sigmoid_stats(pp, p(x), p(scale), p(bias), 0, p(gws), gws.numel(), st))
        else:
            nat.check(lib.crossclr_sigmoid_stats_ids(pp, p(x), p(scale), p(bias), p(group), 0, p(gws), gws.numel(), st))
        nat.check(lib.crossclr_sigmoid_finish(pp, p(gws), 0, p(scale), p(bias), p(row_loss), p(pair), p(ls), p(sg), st))

    def sigmoid_bwd(group):
        if group is None:
            nat.check(lib.crossclr_sigmoid_backward(pp, p(x), p(scale), p(bias), p(gbuf), st))
        else:
            nat.check(lib.crossclr_sigmoid_backward_ids(pp, p(x), p(scale), p(bias), p(group), p(gbuf), st))

    def three(fn):
        return {"plain": lambda: fn(None), "distinct": lambda: fn(groups["distinct"]), "by4": lambda: fn(groups["by4"])}

    print(f"  B={B} D={D} {name}: splits={lib.crossclr_infonce_splits(pp, 0)}, gradient slices={plan.bwd_slices}")
    # the statistics of the by4 ids stay in lse / pair for the InfoNCE backward of every variant (its time does not depend on them)
    infonce_fwd(groups["by4"])
    report("InfoNCE stats + finish", alternate(three(infonce_fwd)))
    infonce_fwd(groups["by4"])
    report("InfoNCE backward product", alternate(three(infonce_bwd)))
    report("sigmoid stats + finish", alternate(three(sigmoid_fwd)))
    report("sigmoid backward product", alternate(three(sigmoid_bwd)))
    cn = alternate({k: (lambda k=k: nat.check(lib.crossclr_pair_groups(pp, p(ids[k]), p(groups[k]), st))) for k in ids})
    for k in ids:
        print(f"      crossclr_pair_groups         ids {k:<8} {fmt(cn[k])}")


print(f"device: {torch.cuda.get_device_name(0)}; reps={args.reps} x inner={args.inner}, median of alternating windows (HIP events)")
for mode, name in ((nat.MODE_FP32, "fp32"), (nat.MODE_BF16, "bf16")):
    print(f"compute_mode={name}")
    for sh in args.shapes.split(","):
        B, D = (int(x) for x in sh.split("x"))
        shape(B, D, mode, name)
