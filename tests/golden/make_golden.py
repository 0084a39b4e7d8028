#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by IMPORTING THE REFERENCE.

Writing fixtures needs the reference's trainer/loss.py, named by the environment
variable CROSSCLR_REFERENCE_FILE.  The reference file itself is never committed:
what is committed is data -- generator kind and seed, shapes, hyper-parameters,
the SHA-256 of the inputs, and the reference's outputs (loss, gradients or
gradient samples).

The reference hard-codes `.cuda()` for its masks (trainer/loss.py:66,103,104);
in THIS process only, `torch.Tensor.cuda` is made the identity so the forward
runs on CPU tensors.  While at it the script proves the oracle's op-for-op form
bit-identical to the reference (torch.equal on loss and both gradients) for
every case it can afford to run twice, and refuses to write fixtures otherwise.

    python tests/golden/make_golden.py            # small + medium cases
    python tests/golden/make_golden.py --large    # adds B=4096 / B=8192 (12.5 GB RAM, ~1 min)
    python tests/golden/make_golden.py --check    # regenerate in memory, compare with the committed
                                                  # index.json / *.npz bit for bit, write nothing
    python tests/golden/make_golden.py --check --only g1_b64_d256_s0 g2_b8_d16_s1

`--check` without CROSSCLR_REFERENCE_FILE regenerates every case through the oracle's op-for-op
form in the reference's place (the form this script proved bit-identical to the reference when
it wrote the fixtures): the recipe -> fixture path is then checked on any machine.

The reference module is loaded BY FILE PATH under the private name `ref_loss` (the repository
has its own `trainer/loss.py` drop-in shim, so `import trainer.loss` would find the product, not
the reference); the script asserts that the class it calls comes from that file.
"""
import argparse
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REFERENCE_FILE = os.environ.get("CROSSCLR_REFERENCE_FILE")


def load_reference():
    """The reference class, loaded from its file (never through `import trainer.loss`); None without one."""
    if not REFERENCE_FILE:
        return None
    if not os.path.exists(REFERENCE_FILE):
        raise SystemExit(f"CROSSCLR_REFERENCE_FILE={REFERENCE_FILE} not found")
    spec = importlib.util.spec_from_file_location("ref_loss", REFERENCE_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ref = mod.CrossCLR_onlyIntraModality
    assert ref.__module__ == "ref_loss" and os.path.samefile(mod.__file__, REFERENCE_FILE), \
        "the class under test is not the reference"
    assert not hasattr(ref, "compute_mode") and "crossclr_amd" not in sys.modules, "product code leaked in"
    return ref


torch.Tensor.cuda = lambda self, *a, **k: self          # oracle process only
Reference = load_reference()
from oracle import crossclr_oracle as orc                          # noqa: E402

DT = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32,
      "float64": torch.float64}


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def run_reference(v, t, tau, w):
    if Reference is None:       # (--check only: the oracle's op-for-op form stands in for the reference)
        return orc.eager_loss_and_grads(v, t, tau, w)
    v = v.detach().clone().requires_grad_(True)
    t = t.detach().clone().requires_grad_(True)
    crit = Reference(temperature=tau, negative_weight=w)
    loss = crit(v, t)
    loss.backward()
    assert loss.dtype == torch.float64 and loss.dim() == 0
    return loss.detach(), v.grad, t.grad


CHECK = {"on": False, "only": None, "bad": [], "seen": 0}


def same_arrays(a, b):
    return set(a) == set(b) and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and
                                    np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def case(name, kind, B, D, seed, tau=0.03, w=0.8, dtype="float32", full=True, mutate=None,
         check_eager=True):
    if CHECK["only"] is not None and name not in CHECK["only"]:
        return None
    v, t = orc.make_inputs(kind, B, D, seed, DT[dtype])
    if mutate == "zero_row":
        v[min(3, B - 1)] = 0
    if mutate == "tiny_row":   # 0 < ||v_3|| < eps of F.normalize: its clamp_min backward drops the projection term
        v[min(3, B - 1)] *= 1e-14 / float(v[min(3, B - 1)].double().norm())
    loss, gv, gt = run_reference(v, t, tau, w)
    if check_eager:
        el, egv, egt = orc.eager_loss_and_grads(v, t, tau, w)
        ok = torch.equal(el, loss) and torch.equal(egv, gv) and torch.equal(egt, gt)
        if not ok:
            raise SystemExit(f"{name}: oracle eager form is NOT bit-identical to the reference")
    meta = dict(name=name, kind=kind, B=B, D=D, seed=seed, temperature=tau, negative_weight=w,
                dtype=dtype, mutate=mutate, input_sha256=sha(v, t), loss=float(loss),
                loss_repr=repr(float(loss)), grad_dtype=str(gv.dtype).replace("torch.", ""),
                grad_v_norm=float(gv.double().norm()), grad_t_norm=float(gt.double().norm()),
                grad_v_absmax=float(gv.double().abs().max()),
                grad_t_absmax=float(gt.double().abs().max()), eager_bit_identical=check_eager)
    arrays = {}
    if full:
        arrays["grad_v"] = gv.double().numpy() if dtype != "float32" else gv.numpy()
        arrays["grad_t"] = gt.double().numpy() if dtype != "float32" else gt.numpy()
    else:
        rows = np.linspace(0, B - 1, 8).astype(np.int64)
        arrays["rows"] = rows
        arrays["grad_v_rows"] = gv[rows].numpy()
        arrays["grad_t_rows"] = gt[rows].numpy()
    # per-row intermediates from the float64 closed form (what the kernels expose)
    if B <= 4096:
        st = orc.streaming_stats(v.float(), t.float(), tau, w)
        arrays["logZv"] = st["logZv"].numpy()
        arrays["logZt"] = st["logZt"].numpy()
        arrays["diag"] = st["diag"].numpy()
        meta["streaming_loss"] = float(st["loss"])
    if CHECK["on"]:
        CHECK["seen"] += 1
        committed = {m["name"]: m for m in json.load(open(os.path.join(HERE, "index.json")))["cases"]}.get(name)
        stored = dict(np.load(os.path.join(HERE, name + ".npz"))) if os.path.exists(os.path.join(HERE, name + ".npz")) else None
        ok = committed is not None and stored is not None and committed == json.loads(json.dumps(meta)) and \
            same_arrays(arrays, stored)
        print(f"{name:28s} {'identical to the committed fixture' if ok else 'DIFFERS from the committed fixture'}")
        if not ok:
            CHECK["bad"].append(name)
        return meta
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrays)
    print(f"{name:28s} loss={meta['loss_repr']:>22s}  |gv|={meta['grad_v_norm']:.6e}")
    return meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large", action="store_true")
    ap.add_argument("--check", action="store_true", help="compare with the committed fixtures instead of writing")
    ap.add_argument("--only", nargs="*", default=None, help="restrict to these case names")
    args = ap.parse_args()
    CHECK["on"], CHECK["only"] = args.check, (set(args.only) if args.only else None)
    if Reference is None and not args.check:
        raise SystemExit("writing fixtures needs the reference: set CROSSCLR_REFERENCE_FILE to its trainer/loss.py")
    torch.manual_seed(0)

    class _Metas(list):
        def append(self, m):
            if m is not None:
                super().append(m)
    metas = _Metas()
    # G1: BASELINE config 1 (B=64, D=256)
    for s in (0, 7, 1234):
        metas.append(case(f"g1_b64_d256_s{s}", "randn", 64, 256, s))
    # G2: hand-checkable
    metas.append(case("g2_b8_d16_s1", "randn", 8, 16, 1))
    # G3
    metas.append(case("g3_b256_d512_s2", "randn", 256, 512, 2))
    # G4: dtype sweep
    for dt in ("float16", "bfloat16", "float32", "float64"):
        metas.append(case(f"g4_b16_d32_s3_{dt}", "randn", 16, 32, 3, dtype=dt))
    # G5: edge cases
    metas.append(case("g5_zero_row_b16_d32", "randn", 16, 32, 3, mutate="zero_row"))
    metas.append(case("g5_b1_d32", "randn", 1, 32, 3))
    metas.append(case("g5_w0_tau01_b16_d32", "randn", 16, 32, 3, tau=0.1, w=0.0))
    metas.append(case("g5_tau01_b16_d32", "randn", 16, 32, 3, tau=0.1))
    metas.append(case("g5_ragged_b100_d48", "randn", 100, 48, 5))
    metas.append(case("g5_ragged_b130_d200", "randn", 130, 200, 6, tau=0.05, w=0.5))
    metas.append(case("g5_tau002_b32_d64", "randn", 32, 64, 8, tau=0.02, w=1.0))
    # small temperatures: |logit| up to 1/tau = 200 / 500, beyond any fixed soft-max shift in fp32 (the reference's
    # soft-max is float64 with a per-row maximum, loss.py:60,96-100)
    metas.append(case("g5_tau0005_b32_d64", "randn", 32, 64, 9, tau=0.005, w=0.8))
    metas.append(case("g5_tau0002_b64_d128", "randn", 64, 128, 10, tau=0.002, w=1.0))
    metas.append(case("g5_tau0002_aligned_b128_d96", "aligned", 128, 96, 14, tau=0.002, w=0.8))
    metas.append(case("g5_tau0005_w4_b48_d40", "cluster", 48, 40, 15, tau=0.005, w=4.0))
    metas.append(case("g5_tiny_row_b16_d32", "randn", 16, 32, 3, mutate="tiny_row"))
    # G6: aligned / clustered (bf16 stress), sampled rows only
    metas.append(case("g6_aligned_b2048_d512", "aligned", 2048, 512, 11, full=False))
    metas.append(case("g6_cluster_b2048_d512", "cluster", 2048, 512, 12, full=False))
    metas.append(case("g6_aligned_b256_d128", "aligned", 256, 128, 13))
    metas.append(case("g6_tau0005_b2048_d512", "randn", 2048, 512, 16, tau=0.005, full=False))
    metas.append(case("g6_tau0002_cluster_b1024_d256", "cluster", 1024, 256, 17, tau=0.002, w=1.0, full=False))
    # G9: the regime compute_mode="auto" resolves to bf16 in (global batch >= 1024) at temperatures between the two-pass threshold
    # (0.0078) and the other goldens' 0.02: the logit carries the bf16 rounding of a cosine times 1/tau.  (No "aligned" case here: at
    # these temperatures its reference loss is exactly 0.0 and its gradients ~1e-24 .. 1e-34 -- nothing a tolerance can be stated against.)
    for tau, tag in ((0.01, "tau001"), (0.015, "tau0015")):
        metas.append(case(f"g9_{tag}_b2048_d512", "randn", 2048, 512, 21, tau=tau, full=False))
        metas.append(case(f"g9_{tag}_cluster_b2048_d512", "cluster", 2048, 512, 23, tau=tau, full=False))
    # G10: wide embeddings -- the XP = 2 (D = 1024) and XP = 3 (D = 1536, beyond the register-resident forward) instantiations of the saved
    # backward's pair kernel meet reference-generated numbers directly (round-4 review: they were checked against the streaming oracle only)
    metas.append(case("g10_b2048_d1024", "randn", 2048, 1024, 31, full=False))
    metas.append(case("g10_b2048_d1536", "randn", 2048, 1536, 32, full=False))
    # round 6: wide plans beyond 4096 (10 and 12 column parts of the saved D-slice backward; the second one at a batch the pair kernel takes)
    metas.append(case("g10_b1024_d5000", "randn", 1024, 5000, 33, full=False))
    metas.append(case("g10_b4096_d6000", "randn", 4096, 6000, 34, full=False))
    # G7: large
    if args.large:
        metas.append(case("g7_b4096_d512_s1234", "randn", 4096, 512, 1234, full=False))
        metas.append(case("g7_b8192_d512_s1234", "randn", 8192, 512, 1234, full=False,
                          check_eager=False))
    if args.check:
        if CHECK["bad"] or not CHECK["seen"]:
            raise SystemExit(f"golden check FAILED: {CHECK['bad'] or 'no case selected'}")
        source = REFERENCE_FILE or "the oracle's op-for-op form (no CROSSCLR_REFERENCE_FILE)"
        print(f"golden check ok: {CHECK['seen']} cases regenerated from {source} match the committed fixtures")
        return
    out = os.path.join(HERE, "index.json")
    prev = {}
    if os.path.exists(out):
        prev = {m["name"]: m for m in json.load(open(out))["cases"]}
    for m in metas:
        prev[m["name"]] = m
    json.dump({"generator": "tests/golden/make_golden.py",
               "reference": "amazon-science/crossmodal-contrastive-learning @ v1, trainer/loss.py",
               "torch": torch.__version__, "numpy": np.__version__,
               "cases": sorted(prev.values(), key=lambda m: m["name"])},
              open(out, "w"), indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
