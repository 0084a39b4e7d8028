#!/usr/bin/env python3
"""compute_mode A/B in ONE process: fp32, bf16x3 and bf16 steps (module forward + backward) timed in alternating blocks, so that the
three modes see the same clocks and the same box.  Shapes: B = 8192 with D = 512 and 1024 (fwd+bwd), and B = 4096, D = 512 forward
only (BASELINE config 2).  usage: mode_ab.py [blocks] [steps per block]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, crossclr_amd

R = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N = int(sys.argv[2]) if len(sys.argv) > 2 else 20
MODES = ("fp32", "bf16x3", "bf16")


def timer(B, D, mode, fwd_only):
    g = torch.Generator().manual_seed(1234)
    v = torch.randn(B, D, generator=g).cuda().requires_grad_(not fwd_only)
    t = torch.randn(B, D, generator=g).cuda().requires_grad_(not fwd_only)
    crit = crossclr_amd.CrossCLR_onlyIntraModality(0.03, 0.8, compute_mode=mode).cuda()

    def block(n):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            if fwd_only:
                with torch.no_grad():
                    crit(v, t)
            else:
                v.grad = t.grad = None
                crit(v, t).backward()
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z) / n
    return block


for B, D, fwd_only in ((8192, 512, False), (8192, 1024, False), (4096, 512, True)):
    blocks = {m: timer(B, D, m, fwd_only) for m in MODES}
    for m in MODES:
        blocks[m](3)                       # warm-up: plans, workspaces, first launches
    xs = {m: [] for m in MODES}
    for r in range(R):
        for m in (MODES if r % 2 == 0 else MODES[::-1]):
            xs[m].append(blocks[m](N))
    med = {m: sorted(x)[len(x) // 2] for m, x in xs.items()}
    what = "fwd" if fwd_only else "fwd+bwd"
    for m in MODES:
        print(f"B={B} D={D} {what:8s} {m:7s} ms/step per block: " + " ".join(f"{x:.4f}" for x in xs[m]) + f" | median {med[m]:.4f}", flush=True)
    print(f"B={B} D={D} {what:8s} bf16x3 / fp32 = {med['bf16x3'] / med['fp32']:.3f}, bf16x3 / bf16 = {med['bf16x3'] / med['bf16']:.3f}", flush=True)
    del blocks
    torch.cuda.empty_cache()
