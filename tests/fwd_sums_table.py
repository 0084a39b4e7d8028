"""The launches of fwd_sums_kernel<T, SW, MODE, ST, SYM> that the C ABI reaches at small D, as one table, and the check both suites run
over it: tests/test_kernels_emulated.py on the host emulation of the kernel sources, tests/test_gpu_parity.py (`-m gpu`) on the hipcc
build -- the only place where a wrong template choice of THAT build would show.

A row is (operand type, weighted, pass, save, symmetric).  check_row() calls the entry point that reaches it, asserts the exact
crossclr_last_kernel(0) string, finishes the forward and compares the loss with the float64 oracle at the bar the neighbouring tests
already use for that mode:

  fp32        1e-5 relative, two-pass regime 1e-4                       (tests/test_kernels_emulated.py)
  bf16x3      2e-5 relative + 2e-8 / tau                                (tests/test_bf16x3_cpu.py)
  bf16        5e-5 against the bf16-operand model where there is one (single pass, no sample weights:
              test_bf16_generic_kernels_match_bf16_model); 3e-3 against the float64 oracle with sample weights
              (tests/test_sample_weights_cpu.py); 2e-2 in the two-pass regime (test_small_temperatures_take_the_two_pass_soft_max)
  score modes fp32 2e-6, bf16 2e-5 against the closed form on the rounded operands   (tests/test_ranking_cpu.py)

Rows that need an environment knob (`knob`) run on the emulation only: the product library reads its knobs once per process.
Not in the table, because no plan at D <= 1024 reaches them: the bf16 records of the wide plans' single pass ("symmetric, save, bf16
records" and "rectangular, save, bf16 records"; tests test_wide_bf16_plans_save_their_exponentials and the sharded GPU tests cover them)."""
import ctypes
import functools
from collections import namedtuple

import torch

from crossclr_amd import _native as nat
from oracle import crossclr_oracle as orc
from oracle import influence_oracle as inf
from oracle import ranking_oracle as rk

SHAPES = [(150, 24), (70, 16)]      # 512 stacked rows in two paired row blocks: mirrored tiles + column partials; one pair: diagonal tile only
W = 0.8
TAU = {"sums": 0.05, "rowmax": 0.004, "shifted": 0.004}
MARGIN = 0.1

Row = namedtuple("Row", "mode weighted what save symmetric knob label")


def _rows():
    rows = []
    sym_knob = "CROSSCLR_DISABLE_SYMMETRIC"
    for mode, tag in (("fp32", ""), ("bf16x3", "<x3_t>")):
        for weighted in (False, True):
            for what in ("sums", "rowmax", "shifted"):
                rows.append(Row(mode, weighted, what, False, True, None, f"fwd_sums_kernel{tag} (symmetric)"))
                rows.append(Row(mode, weighted, what, False, False, None, f"fwd_sums_kernel{tag}"))
                if what != "rowmax":    # the saving forwards take one operand: only the knob makes them walk every tile
                    rows.append(Row(mode, weighted, what, True, True, None, f"fwd_sums_kernel{tag} (symmetric, save)"))
                    rows.append(Row(mode, weighted, what, True, False, sym_knob, f"fwd_sums_kernel{tag} (save)"))
    for weighted in (False, True):      # bf16 plans of these D are register-resident: their single pass reaches the generic kernel by knob only
        for symmetric, label in ((True, "fwd_sums_kernel (symmetric)"), (False, "fwd_sums_kernel")):
            rows.append(Row("bf16", weighted, "sums", False, symmetric, "CROSSCLR_DISABLE_FAST", label))
            rows.append(Row("bf16", weighted, "rowmax", False, symmetric, None, label))
            rows.append(Row("bf16", weighted, "shifted", False, symmetric, None, label))
        rows.append(Row("bf16", weighted, "shifted", True, False, None, "fwd_sums_kernel (save, bf16 records)"))
    for mode in ("fp32", "bf16"):       # score statistics: no scales, no split operand
        rows.append(Row(mode, False, "score_diag", False, False, None, "fwd_sums_kernel (positive-pair scores)"))
        rows.append(Row(mode, False, "score_rows", False, True, None, "fwd_sums_kernel (score rows)"))
        rows.append(Row(mode, False, "score_rows", False, False, sym_knob, "fwd_sums_kernel (score rows)"))
    return rows


ROWS = _rows()


def row_id(row):
    return "-".join([row.mode, "weighted" if row.weighted else "plain", row.what, "save" if row.save else "nosave",
                     "sym" if row.symmetric else "full"])


MODES = {"fp32": nat.MODE_FP32, "bf16x3": nat.MODE_BF16X3, "bf16": nat.MODE_BF16}


@functools.lru_cache(maxsize=None)
def _inputs(B, D):
    v, t = orc.make_inputs("randn", B, D, 11)
    g = torch.Generator().manual_seed(5)
    kv, kt = (torch.rand(B, generator=g) > 0.3).float(), (torch.rand(B, generator=g) > 0.3).float()
    ov, ot = 0.5 + torch.rand(B, generator=g), 0.5 + torch.rand(B, generator=g)
    return v, t, kv, kt, ov, ot


@functools.lru_cache(maxsize=None)
def _reference(B, D, weighted, tau, bf16_model):
    """float64 loss of the oracle (computed once per shape and regime, shared by the rows)."""
    v, t, kv, kt, ov, ot = _inputs(B, D)
    if weighted:
        return float(inf.streaming_weighted_loss_and_grads(v, t, tau, W, kv, kt, ov, ot)["loss"])
    if bf16_model:
        return float(orc.bf16_operand_model_loss(v, t, tau, W))
    return float(orc.streaming_stats(v, t, tau, W)["loss"])


@functools.lru_cache(maxsize=None)
def _score_reference(B, D, rounded):
    v, t = _inputs(B, D)[:2]
    im, s = torch.nn.functional.normalize(v, dim=1), torch.nn.functional.normalize(t, dim=1)
    if rounded:
        im, s = im.bfloat16().float(), s.bfloat16().float()
    return float(rk.max_margin_streaming(im, s, MARGIN)["loss"])


def _bar(row, tau, ref):
    rel = max(1.0, abs(ref))
    if row.what.startswith("score"):
        return (2e-6 if row.mode == "fp32" else 2e-5) * rel
    two_pass = row.what != "sums"
    if row.mode == "fp32":
        return (1e-4 if two_pass else 1e-5) * rel
    if row.mode == "bf16x3":
        return 2e-5 * rel + 2e-8 / tau
    return (2e-2 if two_pass else 3e-3 if row.weighted else 5e-5) * rel


def check_row(row, B, D, dev):
    """Run `row` at batch B, width D on device `dev` through nat.library(); the caller has set row.knob, if any."""
    lib = nat.library()
    v, t, kv, kt, ov, ot = _inputs(B, D)
    plan = nat.make_plan(B, D, 1, 0, MODES[row.mode])
    pp = ctypes.byref(plan)
    f32 = dict(dtype=torch.float32, device=dev)
    vd, td = v.to(dev), t.to(dev)
    x = torch.empty(plan.operand_bytes, dtype=torch.uint8, device=dev)
    inv, diag = torch.empty(2 * plan.bpad, **f32), torch.empty(plan.bpad, **f32)
    nat.check(lib.crossclr_normalize(pp, vd.data_ptr(), td.data_ptr(), vd.stride(0), td.stride(0), nat.IN_F32, x.data_ptr(), inv.data_ptr(),
                                     diag.data_ptr(), None))
    part = torch.zeros(plan.fwd_ws_floats, **f32)
    ls = torch.zeros(plan.loss_ws_doubles, dtype=torch.float64, device=dev)

    def last_kernel():
        return lib.crossclr_last_kernel(0).decode()

    if row.what.startswith("score"):
        sdiag = torch.empty(2 * plan.bpad, **f32)
        nat.check(lib.crossclr_score_diag(pp, x.data_ptr(), sdiag.data_ptr(), None))
        if row.what == "score_diag":
            assert last_kernel() == row.label
        hinge, active = torch.empty(2 * plan.bpad, **f32), torch.empty(2 * plan.bpad, **f32)
        nat.check(lib.crossclr_score_rows(pp, x.data_ptr(), sdiag.data_ptr(), MARGIN, part.data_ptr(), hinge.data_ptr(), active.data_ptr(),
                                          ls.data_ptr(), None))
        if row.what == "score_rows":
            assert last_kernel() == row.label
        ref = _score_reference(B, D, row.mode == "bf16")
        got = ls.cpu()[1].item()
        assert abs(got - ref) <= _bar(row, None, ref), (row_id(row), got, ref)
        return

    tau = TAU[row.what]
    keep = []       # (the struct only holds addresses)
    sw = None
    if row.weighted:
        k, lw = torch.zeros(2, plan.bpad, **f32), torch.zeros(2, plan.bpad, **f32)
        k[0, :B], k[1, :B], lw[0, :B], lw[1, :B] = kv.to(dev), kt.to(dev), ov.to(dev), ot.to(dev)
        keep += [k, lw]
        sw = ctypes.pointer(nat.SampleWeights(k.data_ptr(), k.data_ptr(), lw.data_ptr()))
    # a second copy of the operand: other columns than the rows' own buffer take the pass over every tile
    cols = x if row.symmetric else x.clone()
    stash = None
    if row.save:
        nbytes = plan.stash_bytes if row.what == "sums" else lib.crossclr_stash_bytes_s(pp)
        assert nbytes > 0, row_id(row)
        stash = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if row.what == "sums":
        if row.save:
            nat.check(lib.crossclr_forward_save(pp, x.data_ptr(), tau, W, sw, part.data_ptr(), 0, stash.data_ptr(), None))
        else:
            nat.check(lib.crossclr_forward_w(pp, x.data_ptr(), cols.data_ptr(), 1, 0, -1, tau, W, sw, part.data_ptr(), 0, None))
        assert last_kernel() == row.label
        logz, rz, wrz = (torch.empty(2 * plan.bpad, **f32) for _ in range(3))
        nat.check(lib.crossclr_forward_finish_w(pp, part.data_ptr(), plan.fwd_slots, diag.data_ptr(), tau, W, sw, logz.data_ptr(), rz.data_ptr(),
                                                wrz.data_ptr(), ls.data_ptr(), None))
    else:
        assert lib.crossclr_needs_row_shift(tau, W) == 1
        shift = torch.empty(2 * plan.bpad, **f32)
        first_cols = cols if row.what == "rowmax" else x
        nat.check(lib.crossclr_forward_rowmax(pp, x.data_ptr(), first_cols.data_ptr(), 1, 0, -1, tau, W, sw, part.data_ptr(), shift.data_ptr(), 0,
                                              None))
        if row.what == "rowmax":
            assert last_kernel() == row.label
            cols = x
        if row.save:
            nat.check(lib.crossclr_forward_save_s(pp, x.data_ptr(), tau, W, sw, shift.data_ptr(), part.data_ptr(), 0, stash.data_ptr(), None))
        else:
            nat.check(lib.crossclr_forward_s(pp, x.data_ptr(), cols.data_ptr(), 1, 0, -1, tau, W, sw, shift.data_ptr(), part.data_ptr(), 0, None))
        if row.what == "shifted":
            assert last_kernel() == row.label
        logz, rz, wrz = (torch.empty(2 * plan.bpad, **f32) for _ in range(3))
        nat.check(lib.crossclr_forward_finish_s(pp, part.data_ptr(), plan.fwd_slots, diag.data_ptr(), tau, W, sw, shift.data_ptr(), logz.data_ptr(),
                                                rz.data_ptr(), wrz.data_ptr(), ls.data_ptr(), None))
    ref = _reference(B, D, row.weighted, tau, row.mode == "bf16" and row.what == "sums" and not row.weighted)
    got = ls.cpu()[1].item()
    assert abs(got - ref) <= _bar(row, tau, ref), (row_id(row), got, ref)
    del keep
