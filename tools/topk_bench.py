#!/usr/bin/env python3
"""Timing of retrieval_topk (fused similarity + top-k) against the score pass it shares its tiled product with.

In ONE process on one device, for fp32 and bf16 operands, HIP events around repeated launches (warm-up, then the median of `--reps`
windows of `--inner` launches each):
  * retrieval_topk end to end (pack both sets, select, merge, index widening) and its two kernels alone (crossclr_topk_select,
    crossclr_topk_merge) at (Nq, Ng, D, k) = (8192, 8192, 512, 10) and (1000, 100000, 512, 10);
  * crossclr_score_rows at B = 8192, D = 512 in the same mode: the retrieval-ranks pass over the same 2 B^2 D product, one compare per
    score in its epilogue -- the yardstick: select + merge at the square shape should take at most 2x its time;
  * for information, torch.topk(q_hat @ g_hat.T, 10) and its peak memory (the dense matrix this feature avoids).
usage: topk_bench.py [--reps 7] [--inner 5] [--skip-dense]"""
import argparse, ctypes, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import crossclr_amd
from crossclr_amd import _native as nat, loss as L

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--skip-dense", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("topk_bench.py measures on the GPU: no device found")
lib, p = nat.library(), L._ptr
K = 10


def timeit(fn):
    """median over args.reps windows of args.inner launches, in ms per launch"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / args.inner)
    return statistics.median(out), min(out), max(out)


def fmt(t):
    return f"{t[0]:8.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def score_rows_time(B, D, mode):
    g = torch.Generator().manual_seed(1)
    v, t = torch.randn(B, D, generator=g).cuda(), torch.randn(B, D, generator=g).cuda()
    plan = nat.make_plan(B, D, 1, 0, mode); pp = ctypes.byref(plan)
    st = L._stream_for(v); f32 = dict(dtype=torch.float32, device="cuda")
    x = torch.empty(plan.operand_bytes, dtype=torch.uint8, device="cuda"); inv = torch.empty(2 * plan.bpad, **f32); dg = torch.empty(plan.bpad, **f32)
    nat.check(lib.crossclr_normalize(pp, p(v), p(t), D, D, nat.IN_F32, p(x), p(inv), p(dg), st))
    diag = torch.empty(2 * plan.bpad, **f32); part = torch.empty(plan.fwd_ws_floats, **f32)
    hinge, act = torch.empty(2 * plan.bpad, **f32), torch.empty(2 * plan.bpad, **f32)
    ls = torch.empty(plan.loss_ws_doubles, dtype=torch.float64, device="cuda")
    nat.check(lib.crossclr_score_diag(pp, p(x), p(diag), st))
    return timeit(lambda: nat.check(lib.crossclr_score_rows(pp, p(x), p(diag), 0.0, p(part), p(hinge), p(act), p(ls), st)))


def topk_times(nq, ng, D, mode, name):
    g = torch.Generator().manual_seed(2)
    q, gal = torch.randn(nq, D, generator=g).cuda(), torch.randn(ng, D, generator=g).cuda()
    st = L._stream_for(q)
    qp = torch.empty(lib.crossclr_topk_operand_bytes(nq, D, mode), dtype=torch.uint8, device="cuda")
    gp = torch.empty(lib.crossclr_topk_operand_bytes(ng, D, mode), dtype=torch.uint8, device="cuda")
    nat.check(lib.crossclr_topk_pack(p(q), D, nq, D, nat.IN_F32, mode, 1, p(qp), st))
    nat.check(lib.crossclr_topk_pack(p(gal), D, ng, D, nat.IN_F32, mode, 1, p(gp), st))
    ws = torch.empty(lib.crossclr_topk_workspace_bytes(nq, ng, K, 0), dtype=torch.uint8, device="cuda")
    sc = torch.empty(nq, K, dtype=torch.float32, device="cuda"); ix = torch.empty(nq, K, dtype=torch.int32, device="cuda")
    t_sel = timeit(lambda: nat.check(lib.crossclr_topk_select(p(qp), p(gp), nq, ng, D, mode, K, 0, p(ws), ws.numel(), st)))
    t_mrg = timeit(lambda: nat.check(lib.crossclr_topk_merge(p(ws), nq, ng, K, 0, p(sc), p(ix), st)))
    t_e2e = timeit(lambda: crossclr_amd.retrieval_topk(q, gal, K, compute_mode=name))
    print(f"  retrieval_topk Nq={nq} Ng={ng} D={D} k={K} {name}: splits={lib.crossclr_topk_splits(nq, ng, K, 0)} workspace={ws.numel() / 2**20:.1f} MiB")
    print(f"      end to end            {fmt(t_e2e)}")
    print(f"      topk_select_kernel    {fmt(t_sel)}   {2.0 * nq * ng * D / t_sel[0] / 1e9:.1f} TFLOP/s of the 2 Nq Ng D product")
    print(f"      topk_merge_kernel     {fmt(t_mrg)}")
    return t_sel, t_mrg, q, gal


def dense_topk(q, gal):
    qh, gh = torch.nn.functional.normalize(q, dim=1), torch.nn.functional.normalize(gal, dim=1)
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); before = torch.cuda.memory_allocated()
    t = timeit(lambda: torch.topk(qh @ gh.t(), K, dim=1))
    peak = torch.cuda.max_memory_allocated() - before
    print(f"      (information) torch.topk(q_hat @ g_hat.T, {K}), fp32 eager: {fmt(t)}, peak extra memory {peak / 2**20:.0f} MiB")


print(f"device: {torch.cuda.get_device_name(0)}; reps={args.reps} x inner={args.inner}, median of windows (HIP events)")
for mode, name in ((nat.MODE_FP32, "fp32"), (nat.MODE_BF16, "bf16")):
    print(f"compute_mode={name}")
    t_rows = score_rows_time(8192, 512, mode)
    print(f"  crossclr_score_rows B=8192 D=512 {name}: {fmt(t_rows)}")
    t_sel, t_mrg, q, gal = topk_times(8192, 8192, 512, mode, name)
    ratio = (t_sel[0] + t_mrg[0]) / t_rows[0]
    print(f"      select + merge = {t_sel[0] + t_mrg[0]:.3f} ms = {ratio:.2f} x crossclr_score_rows (bar: <= 2)")
    if not args.skip_dense:
        dense_topk(q, gal)
    _, _, q, gal = topk_times(1000, 100000, 512, mode, name)
    if not args.skip_dense:
        dense_topk(q, gal)
