"""The row kernels alone, through the C-ABI, on synthetic inputs (tests/test_gpu_row_kernels.py, tests/test_row_kernels_cpu.py).  A helper module
like tests/exact_inputs.py: pytest collects nothing here.  It holds the case tables, the synthetic inputs, the float64 closed forms, the C-ABI
runners and the checkers of the eleven entry points that read or write the CALLER'S OWN tensors through (pointer, row stride, in_dtype):

  (1) crossclr_infonce_backward_finish / crossclr_sigmoid_backward_finish   pairloss_backward_finish_kernel<TIN>
  (2) crossclr_backward_finish_w / _p                                      bwd_finish_pair_kernel<TIN, KC>, bwd_finish_kernel<TIN>
  (3) crossclr_maxmargin_backward_finish                                   (the kernels of (2), unit rows, active-hinge counts as weights)
  (4) crossclr_hardneg_backward                                            hardneg_backward_kernel<TIN>
  (5) crossclr_normalize / _pack / _normalize_xf / _pack_xf / _topk_pack   normalize_kernel, normalize_xf_kernel, topk_pack_kernel

Every kernel is O(b D) and runs without an MFMA kernel in front: `gbuf`, `inv_norm`, `best_index`, `hinge` and `active` are made by hand.
Conventions (all of them asserted by the runners and checkers below):
* inputs are laid out with exact_inputs.lay_out (contiguous, ld+1, ld+3, offset; NaN between the rows) in each of the four input dtypes, and the
  float64 reference is taken on the values AFTER the conversion to the dtype;
* output tensors get a layout of their own (OUT_LAYOUT: another row stride than the input's), are prefilled with NaN, and everything outside
  [b, D] is still NaN afterwards; packed operands are prefilled with 0x55 and their padding comes back as zeros;
* the synthetic gbuf has the plan's own size and slice count; every slice holds integer multiples of 2^-6, |n| <= 64, so the fp32 sum over the
  slices is exact in any order; rows >= b and columns >= D are NaN (the kernels may load them, they must not use them).

THE BAR (derived, not measured).  The finish kernels do their row arithmetic in fp64 and store through (float) v and then the 16-bit conversion:
    |got - want| <= 1/2 ulp_T(max(|want|, |got|)) + 2^-24 |want| + 1e-12 A
ulp_T: 23 (fp32), 10 (fp16; subnormal below 2^-14) or 7 (bf16) fraction bits; for T = fp64 the first two terms are zero.  2^-24 |want| is the
intermediate fp32 rounding, A the largest magnitude among the terms the element is a difference of (from the reference, never from the
kernel's output), 1e-12 the summation order of an fp64 dot product of up to 8192 terms (8192 2^-53).  An element whose bar is zero must be
exact; every element is checked.  An element whose value rounds to infinity in T (fp16 only: the gradients of the row with inv_norm = 1e12 are
~1e11, fp16 ends at 65504) must BE the infinity of its sign.  fp64 scalars: 1e-12 of the sum of the absolute terms."""
import ctypes
import math

import torch

import exact_inputs as xi
from crossclr_amd import _native as nat
from crossclr_amd import loss as L

F32, BF16, F16, F64 = xi.F32, xi.BF16, xi.F16, xi.F64
DTYPES = (F32, F16, BF16, F64)
assert set(DTYPES) == set(L._IN_DTYPE), "the four input dtypes of loss._IN_DTYPE"
LAYOUTS = xi.LAYOUTS
OUT_LAYOUT = {"contiguous": "offset", "ld+1": "ld+3", "ld+3": "ld+1", "offset": "contiguous"}      # input layout -> the outputs' (ld_g != ld)
MODE_NAME = {nat.MODE_FP32: "fp32", nat.MODE_BF16: "bf16", nat.MODE_BF16X3: "bf16x3"}
GRAD_OUT = 3.0
NAN = float("nan")
ROW_KERNEL = 2          # crossclr_last_kernel(2): the most recent row kernel


def dtype_name(dtype):
    return str(dtype).split(".")[1]


def case_id(c):
    return "-".join(MODE_NAME[x] if i == 4 and isinstance(x, int) else (dtype_name(x) if isinstance(x, torch.dtype) else str(x)) for i, x in enumerate(c))


def cross(shapes, dtypes=DTYPES, layouts=LAYOUTS):
    return [(b, D, dtype, layout) for b, D in shapes for dtype in dtypes for layout in layouts]


def with_modes(cases, modes=(nat.MODE_FP32, nat.MODE_BF16)):
    """one plan mode per case: the modes alternate from case to case and start the other way round every four cases, so that in a
    dtype x layout cross every dtype AND every layout sees both, as does every D of a table (asserted below)"""
    return [c + (modes[(i + i // 4) % len(modes)],) for i, c in enumerate(cases)]


def modes_per_width(cases):
    seen = {}
    for c in cases:
        seen.setdefault(c[1], set()).add(c[4])
    return seen


# ----------------------------------------------------------------------------------------------------------------------------------
# case tables.  (b, D, dtype, layout, plan mode)
# ----------------------------------------------------------------------------------------------------------------------------------
# (70, 101): odd D -- the alignment of contiguous fp32 rows alternates from row to row, the last block of 4 rows is ragged;
# (130, 40) .. (70, 1024): 1 to 4 cached stretches of 256 elements (KC of bwd_finish_pair_kernel), 1024 fills the cache; (130, 1100): the
# second pass beyond kRowCache (bwd_finish_kernel, the uncached loop of pairloss_backward_finish_kernel)
FINISH_CROSS = [(70, 101), (130, 1100)]
FINISH_OTHERS = [(130, 40), (130, 300), (130, 600), (70, 1024)]
FINISH_CASES = with_modes(cross(FINISH_CROSS) + cross(FINISH_OTHERS, (F32, BF16), ("contiguous", "ld+1")))
# D -> KC = ceil(D / 256) of bwd_finish_pair_kernel<TIN, KC>.  (crossclr_last_kernel(2) reports the template's name without KC: the runtime
# assertion tells bwd_finish_pair_kernel from bwd_finish_kernel, WHICH instantiation ran follows from this table and the host's switch on D)
STRETCHES = {101: 1, 40: 1, 300: 2, 600: 3, 1024: 4}
DPAD = {300: {nat.MODE_FP32: 512, nat.MODE_BF16: 384}}               # gbuf rows are Dpad apart, and Dpad depends on the plan's mode
WORLD3_CASE = (70, 101, F32, "ld+1", nat.MODE_BF16)                 # B = b * world in the divisor
MAXMARGIN_CASES = with_modes(cross([(70, 101)]) + cross([(130, 300)], (F32, BF16), ("contiguous", "ld+1")))
# hardneg_backward_kernel: stages of kHardnegStage = 2048 entries, slabs of 64 * kHardnegSlab = 1024 columns
HARDNEG_STAGE, HARDNEG_SLAB = 2048, 1024
HARDNEG_CASES = cross([(70, 48), (2049, 1100)]) + cross([(2049, 48), (4100, 48), (70, 1100)], (F32, BF16), ("contiguous",))
LAYOUT_CASES = [c + (m,) for c in cross([(70, 101)]) for m in (nat.MODE_FP32, nat.MODE_BF16, nat.MODE_BF16X3)] + \
               [c + (nat.MODE_BF16,) for c in cross([(130, 600), (130, 1100)], (F32, BF16), ("contiguous", "ld+3"))]
# the emulated subset: every family at (70, 101) (hardneg: (70, 48) and (2049, 48)), {fp32, bf16} x {contiguous, ld+3, offset}
CPU_DTYPES, CPU_LAYOUTS = (F32, BF16), ("contiguous", "ld+3", "offset")
CPU_FINISH_CASES = with_modes(cross([(70, 101)], CPU_DTYPES, CPU_LAYOUTS))
CPU_MAXMARGIN_CASES = CPU_FINISH_CASES
CPU_HARDNEG_CASES = cross([(70, 48), (2049, 48)], CPU_DTYPES, CPU_LAYOUTS)
CPU_LAYOUT_CASES = [c + (m,) for c in cross([(70, 101)], CPU_DTYPES, CPU_LAYOUTS) for m in (nat.MODE_FP32, nat.MODE_BF16, nat.MODE_BF16X3)]

assert all(modes_per_width(t)[D] == {nat.MODE_FP32, nat.MODE_BF16} for t in (FINISH_CASES, CPU_FINISH_CASES) for D in modes_per_width(t))
for _shape in FINISH_CROSS:          # (the plan mode is confounded neither with the dtype nor with the layout)
    for _axis in (2, 3):
        _seen = {}
        for c in FINISH_CASES:
            if c[:2] == _shape:
                _seen.setdefault(c[_axis], set()).add(c[4])
        assert all(v == {nat.MODE_FP32, nat.MODE_BF16} for v in _seen.values()), (_shape, _axis)
# `with_in_dtype` x {aligned, misaligned} of row_load4<float> / row_store4<float>, each KC, the uncached pass, a second stage and slab:
assert {(c[2], c[3]) for c in FINISH_CASES if c[:2] == (70, 101)} == {(d, l) for d in DTYPES for l in LAYOUTS}
assert {STRETCHES[c[1]] for c in FINISH_CASES if c[1] <= 1024} == {1, 2, 3, 4} and any(c[1] > 1024 for c in FINISH_CASES)
assert any(c[0] > HARDNEG_STAGE and c[1] > HARDNEG_SLAB for c in HARDNEG_CASES) and any(c[0] > 2 * HARDNEG_STAGE for c in HARDNEG_CASES)
assert any(c[1] > 1024 for c in LAYOUT_CASES)


# ----------------------------------------------------------------------------------------------------------------------------------
# the bar and the checkers
# ----------------------------------------------------------------------------------------------------------------------------------
FRACTION_BITS = {F32: (23, -126), F16: (10, -14), BF16: (7, -126), "bf16x3": (15, -126)}
# (the split operand hi = bf16(x), lo = bf16(x - hi): |x - hi| <= 2^(e-8), which lo holds to 2^(e-16) = half a unit of 15 fraction bits)
FMAX = {dt: float(torch.finfo(dt).max) for dt in (F32, F16, BF16)}


def half_ulp(kind, want, got):
    """1/2 ulp_T(max(|want|, |got|)) per element; zero for fp64"""
    if kind == F64:
        return torch.zeros_like(want)
    bits, emin = FRACTION_BITS[kind]
    mag = torch.maximum(want.abs(), torch.nan_to_num(got.abs(), nan=0.0, posinf=0.0)).clamp_min(2.0 ** emin)
    return 0.5 * torch.exp2(torch.floor(torch.log2(mag)).clamp_min(emin) - bits)


def element_bar(kind, want, got, A, via_fp32=True):
    """via_fp32 = False: a value rounded ONCE, from fp64 to fp32 (inv_norm, diag_cos): no intermediate rounding in front of the last one"""
    if kind == F64:
        return 1e-12 * A
    return half_ulp(kind, want, got) + (2.0 ** -24 * want.abs() if via_fp32 else 0.0) + 1e-12 * A


def rounds_to_infinity(kind, want):
    """elements that round-to-nearest-even takes to infinity in T: from the largest finite value plus half a unit on"""
    if kind not in FMAX:
        return torch.zeros_like(want, dtype=torch.bool)
    top = math.floor(math.log2(FMAX[kind]))
    return want.abs() >= FMAX[kind] + 0.5 * 2.0 ** (top - FRACTION_BITS[kind][0])


def check_elements(got, want, A, kind, what, via_fp32=True):
    """every element of got [n, m] against want within `element_bar`; returns the worst err / bar (0 where both are zero)"""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    A = torch.as_tensor(A, dtype=torch.float64).expand_as(want)
    err = (got - want).abs()
    bar = element_bar(kind, want, got, A, via_fp32)
    over = rounds_to_infinity(kind, want)
    bad = torch.where(over, got != torch.copysign(torch.full_like(want, float("inf")), want), ~(err <= bar))      # (NaN fails; inf elsewhere too)
    err, bar = err.masked_fill(over, 0.0), bar.masked_fill(over, 1.0)
    if bad.any():
        at = bad.nonzero()[0].tolist()
        i = tuple(at)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond their bar, the first at {at}: got {float(got[i])!r}, "
                             f"want {float(want[i])!r}, |delta| {float(err[i]):.3e}, bar {float(bar[i]):.3e}")
    ratio = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.zeros_like(err))
    return float(ratio.max())


def check_scalar(got, want, abs_terms, what):
    """fp64 scalars: relative 1e-12 of the sum of the absolute terms; returns err / bar"""
    bar = 1e-12 * abs_terms
    err = abs(got - want)
    assert err <= bar, f"{what}: got {got!r}, want {want!r}, |delta| {err:.3e}, bar {bar:.3e}"
    return err / bar if bar > 0 else 0.0


def sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def lay_in(x, dtype, layout, device):
    return xi.lay_out(x, dtype, layout, device)


class Out:
    """an output [b, D] of `dtype` in `layout`, the view's whole buffer prefilled with NaN"""

    def __init__(self, b, D, dtype, layout, device):
        self.view = xi.lay_out(torch.full((b, D), NAN, dtype=torch.float64), dtype, layout, device)
        self.buf = self.view if self.view._base is None else self.view._base
        assert bool(torch.isnan(self.buf).all())
        self.ld = self.view.stride(0)

    def read(self, what):
        """the [b, D] values on the CPU; asserts that everything outside them is still NaN"""
        b, D = self.view.shape
        off = (self.view.data_ptr() - self.buf.data_ptr()) // self.buf.element_size()
        flat = self.buf.detach().cpu().reshape(-1)
        idx = off + torch.arange(b)[:, None] * self.ld + torch.arange(D)[None, :]
        inside = torch.zeros(flat.numel(), dtype=torch.bool)
        inside[idx.reshape(-1)] = True
        assert bool(torch.isnan(flat[~inside]).all()), f"{what}: written outside [b, D]"
        return flat[idx]

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


def last_row_kernel():
    return nat.library().crossclr_last_kernel(ROW_KERNEL).decode()


def device_scalar(value, dtype, device):
    return torch.tensor([value], dtype=dtype, device=device)


# ----------------------------------------------------------------------------------------------------------------------------------
# synthetic inputs
# ----------------------------------------------------------------------------------------------------------------------------------
def synthetic_gbuf(plan, seed):
    """[slices][2][bpad][Dpad] float32 of the plan's own size: n 2^-6 with |n| <= 64 on [b, D], NaN on the padding"""
    S, bp, Dp, b, D = plan.bwd_slices, plan.bpad, plan.Dpad, plan.b, plan.D
    assert plan.gbuf_bytes == S * 2 * bp * Dp * 4, "the layout of crossclr_backward: [bwd_slices][2][bpad][Dpad] floats"
    g = torch.Generator().manual_seed(11000 + seed)
    buf = torch.full((S, 2, bp, Dp), NAN, dtype=torch.float32)
    buf[:, :, :b, :D] = torch.randint(-64, 65, (S, 2, b, D), generator=g).float() * 2.0 ** -6
    return buf


def slice_sum(gbuf, plan, skip=None):
    """M [2, b, D] float64: the sum of the slices (exact in fp32 in any order); skip = a slice left out (the teeth tests)"""
    keep = [s for s in range(plan.bwd_slices) if s != skip]
    return gbuf[keep][:, :, :plan.b, :plan.D].double().sum(0)


EPS_ROW = 3             # the video row whose inv_norm is 1e12: F.normalize's eps rule (x / eps, no projection)

_rows = {}


def raw_rows(b, D, dtype, eps_row=True):
    """(video, text) random rows as values of `dtype` (float64 tensors holding them) and the float32 inv_norm [2, b] of the rows.  eps_row: video
    row EPS_ROW = n 2^-24 with integer |n| <= 8 -- all four dtypes hold those (fp16 as subnormals) -- and its inv_norm is SET to (float) 1e12,
    the value crossclr_normalize writes for a row below eps (a row that small is no fp16 value: inv_norm is synthetic like gbuf)"""
    key = (b, D, dtype, eps_row)
    if key not in _rows:
        g = torch.Generator().manual_seed(12000 + b + D)
        x = torch.randn(2, b, D, generator=g, dtype=torch.float64)
        if eps_row:
            x[0, EPS_ROW] = torch.randint(-8, 9, (D,), generator=g).double() * 2.0 ** -24
        x = x.to(dtype).double()
        n = x.norm(dim=2)
        inv = torch.where(n > 1e-12, 1.0 / n.clamp_min(1e-300), torch.full_like(n, 1e12)).float()
        if eps_row:
            inv[0, EPS_ROW] = 1e12
            assert float(inv[0, EPS_ROW]) == 999999995904.0 and float(x[0, EPS_ROW].abs().max()) > 0
        _rows[key] = (x, inv)
    return _rows[key]


def unit_rows(b, D, dtype):
    """unit rows as values of `dtype` (for the prenormalized entry points), and inv_norm = 1 / ||y|| of made-up vectors they came from"""
    x, _ = raw_rows(b, D, F64, eps_row=False)
    u = torch.nn.functional.normalize(x, dim=2).to(dtype).double()
    g = torch.Generator().manual_seed(13000 + b + D)
    inv = (1.0 / (0.5 + 4.0 * torch.rand(2, b, generator=g, dtype=torch.float64))).float()
    return u, inv


def stats(values, plan, pad=0.0):
    """[2, b] -> the statistics layout [2][bpad] float32"""
    out = torch.full((2, plan.bpad), pad, dtype=torch.float32)
    out[:, :plan.b] = values
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# (1) pairloss_backward_finish_kernel through crossclr_infonce_backward_finish / crossclr_sigmoid_backward_finish
# ----------------------------------------------------------------------------------------------------------------------------------
PAIRLOSS = {"crossclr_infonce_backward_finish": (2.0, 0.25), "crossclr_sigmoid_backward_finish": (1.0, 0.5)}      # (divisor / B, dscale[1] / dscale[0] * B)
PAIRLOSS_VARIANTS = [(1, 1.0 / 0.07), (0, -5.0)]                      # (normalized, logit_scale)


EPS_INV = float(torch.tensor(1e12, dtype=torch.float32))      # inv_norm of a row below F.normalize's eps = 1e-12, as crossclr_normalize stores it


def normalize_backward(g, unit, inv_norm, g_terms):
    """The backward of y = x / max(||x||, eps) (torch.nn.functional.normalize) written out, for an upstream gradient g = dL/dy:
        dL/dx = (g - y (y . g)) / ||x||   above eps,      dL/dx = g / eps   below it (y = x / eps is linear there),
    with inv_norm = 1 / max(||x||, eps) as handed to the kernels.  tests/test_row_kernels_cpu.py holds this against autograd of F.normalize.
    g, unit [..., D]; inv_norm, g_terms [..., 1]; g_terms = the largest magnitude among the terms g is a sum of.
    Returns (dL/dx, A): A = the largest magnitude among the terms an element of dL/dx is a difference of."""
    below_eps = inv_norm == EPS_INV
    along = (unit * g).sum(-1, keepdim=True)
    grad = torch.where(below_eps, g, g - unit * along) * inv_norm
    A = inv_norm.abs() * (g_terms + torch.where(below_eps, torch.zeros_like(along), along.abs() * unit.abs().amax(-1, keepdim=True)))
    return grad, A


def pairloss_reference(x, M, inv, normalized, scale, per_b, reduce_num, go=GRAD_OUT, neighbour_inv=False):
    """include/crossclr.h (crossclr_infonce_backward_finish, crossclr_sigmoid_backward_finish) in float64:
        dL/dx^ = s / (per_b B) M  (per_b = 2: InfoNCE, 1: sigmoid), M = the sum of the slices; times grad_out; `normalized`: followed by the
        normalize backward (`normalize_backward`) with x^ = x inv_norm;  dscale[0] = grad_out sum_p <x^_p, M_p> over the 2 B stacked rows,
        dscale[1] = dscale[0] reduce_num / B = grad_out dL/ds.
    x, M [2, b, D] float64; inv [2, b] (the values the kernel is handed); scale: rounded to the float32 value in device memory.
    neighbour_inv: row i formed with row i + 1's inv_norm (a defect, for the teeth tests).
    Returns {"grads": [2, b, D], "A": [2, b, 1], "dscale": (d0, d1), "dscale_abs": (a0, a1)}"""
    b = x.shape[1]
    s = float(torch.tensor(scale, dtype=torch.float32))
    upstream = go * s / (per_b * b) * M
    terms = upstream.abs().amax(2, keepdim=True)
    if normalized:
        inv_norm = inv.double()[:, :, None]
        if neighbour_inv:
            inv_norm = torch.roll(inv_norm, -1, 1)
        unit = x * inv_norm
        grads, A = normalize_backward(upstream, unit, inv_norm, terms)
    else:
        unit, grads, A = x, upstream, terms
    d0, a0 = float(go * (unit * M).sum()), float(abs(go) * (unit * M).abs().sum())
    return {"grads": grads, "A": A, "dscale": (d0, d0 * reduce_num / b), "dscale_abs": (a0, a0 * reduce_num / b)}


def run_pairloss(entry, plan, gbuf_d, xs, inv_d, normalized, scale, want_video=True, want_text=True, go=GRAD_OUT, out_layout="contiguous"):
    """one call; xs = the (video, text) views on the device.  Returns (Out | None, Out | None, dscale [loss_ws_doubles] on the CPU)"""
    lib, dev = nat.library(), xs[0].device
    b, D, dtype = plan.b, plan.D, xs[0].dtype
    outs = [Out(b, D, dtype, out_layout, dev), Out(b, D, dtype, out_layout, dev)]
    scale_d, go_d = device_scalar(scale, torch.float32, dev), device_scalar(go, torch.float64, dev)
    dscale = torch.full((plan.loss_ws_doubles,), NAN, dtype=torch.float64, device=dev)
    nat.check(getattr(lib, entry)(ctypes.byref(plan), L._ptr(gbuf_d), L._ptr(xs[0]), L._ptr(xs[1]), xs[0].stride(0), xs[1].stride(0), L._IN_DTYPE[dtype],
                                  L._ptr(inv_d), normalized, L._ptr(scale_d), L._ptr(go_d), L._ptr(outs[0].view) if want_video else 0,
                                  L._ptr(outs[1].view) if want_text else 0, outs[0].ld, outs[1].ld, L._ptr(dscale), L._stream_for(xs[0])))
    sync(dev)
    assert last_row_kernel() == "pairloss_backward_finish_kernel"
    return outs[0], outs[1], dscale.cpu()


def check_pairloss_case(b, D, dtype, layout, mode, device):
    """both entry points, normalized = 1 (real inv_norm, one eps row, logit_scale 1 / 0.07) and 0 (logit_scale -5), grad_out = 3; and with either
    gradient omitted.  Returns the worst err / bar."""
    plan = nat.make_plan(b, D, 1, 0, mode)
    assert plan.bwd_slices > 1 and plan.Dpad == DPAD.get(D, {}).get(mode, plan.Dpad)
    gbuf = synthetic_gbuf(plan, b + D)
    M = slice_sum(gbuf, plan)
    x, inv = raw_rows(b, D, dtype)
    gbuf_d, inv_d = gbuf.to(device), stats(inv, plan, NAN).to(device)
    xs = [lay_in(x[m], dtype, layout, device) for m in range(2)]
    worst = 0.0
    for entry, (per_b, reduce_num) in PAIRLOSS.items():
        for normalized, scale in PAIRLOSS_VARIANTS:
            what = f"{entry} b={b} D={D} {dtype_name(dtype)} {layout} {MODE_NAME[mode]} normalized={normalized}"
            ref = pairloss_reference(x, M, inv, normalized, scale, per_b, reduce_num)
            ov, ot, dscale = run_pairloss(entry, plan, gbuf_d, xs, inv_d if normalized else None, normalized, scale, out_layout=OUT_LAYOUT[layout])
            assert ov.ld != xs[0].stride(0)
            full = []
            for m, o in enumerate((ov, ot)):
                got = o.read(what)
                full.append(got)
                worst = max(worst, check_elements(got, ref["grads"][m], ref["A"][m], dtype, f"{what} modality {m}"))
            for k in range(2):
                worst = max(worst, check_scalar(float(dscale[k]), ref["dscale"][k], ref["dscale_abs"][k], f"{what} dscale[{k}]"))
            if normalized:      # either gradient omitted: the other and dscale are the same bits, the omitted buffer stays as it was
                for keep in range(2):
                    o2 = run_pairloss(entry, plan, gbuf_d, xs, inv_d, normalized, scale, want_video=keep == 0, want_text=keep == 1,
                                      out_layout=OUT_LAYOUT[layout])
                    assert torch.equal(o2[keep].read(what).view(torch.uint8), full[keep].view(torch.uint8)), f"{what}: only gradient {keep} asked for"
                    assert o2[1 - keep].untouched(), f"{what}: the omitted gradient {1 - keep} was written"
                    assert torch.equal(o2[2][:2].view(torch.int64), dscale[:2].view(torch.int64)), f"{what}: dscale with gradient {1 - keep} omitted"
    print(f"MEASURE pairloss finish b={b} D={D} {dtype_name(dtype)} {layout} {MODE_NAME[mode]}: worst err / bar = {worst:.3f}")
    return worst


# ----------------------------------------------------------------------------------------------------------------------------------
# (2) crossclr_backward_finish_w / _p, (3) crossclr_maxmargin_backward_finish
# ----------------------------------------------------------------------------------------------------------------------------------
TAU = 0.07
FINISH_VARIANTS = [(0, False), (0, True), (2, False), (1, True)]      # (prenormalized, loss_weight given)


def finish_reference(x, M, inv, inv_tau, B, lw, prenormalized, go=GRAD_OUT, neighbour_inv=False, own_modality_pair=False):
    """include/crossclr.h (crossclr_backward_finish, _w, _p) in float64.  The gradient w.r.t. the unit rows is
        dL/dx^_i = M_i / (2 B tau) - (omega_v,i + omega_t,i) / (2 B tau) partner^_i,      partner^ = the OTHER modality's unit row i,
    times grad_out, and what is returned for the rows as given is
        prenormalized = 0:  its normalize backward (`normalize_backward`) with x^ = x inv_norm
        prenormalized = 1:  itself -- the rows are unit vectors as given (times inv_norm = 1, as crossclr_pack wrote it)
        prenormalized = 2:  its normalize backward with x^ = the rows as given and inv_norm = 1 / ||y|| of the vectors they came from.
    x, M [2, b, D] float64; inv [2, b]; inv_tau: 1 / tau (the float32 reciprocal the host forms from its float argument); lw [2, b] or None.
    neighbour_inv / own_modality_pair: defects for the teeth tests (row i + 1's inv_norm; the positive-pair term from the row's own modality)."""
    inv_norm = inv.double()[:, :, None]
    if neighbour_inv:
        inv_norm = torch.roll(inv_norm, -1, 1)
    unit = x * inv_norm if prenormalized == 0 else x
    partner = unit if own_modality_pair else unit.flip(0)
    omega = 0.5 * (lw[0] + lw[1]).double()[None, :, None] if lw is not None else 1.0
    slices, pair = go * inv_tau / (2.0 * B) * M, go * inv_tau / B * omega * partner
    upstream = slices - pair
    terms = slices.abs().amax(2, keepdim=True) + pair.abs().amax(2, keepdim=True)
    if prenormalized == 1:
        return {"grads": upstream * inv_norm, "A": terms * inv_norm.abs()}
    grads, A = normalize_backward(upstream, unit, inv_norm, terms)
    return {"grads": grads, "A": A}


def run_finish(plan, gbuf_d, xs, inv_d, tau, lw_d, prenormalized, out_layout, go=GRAD_OUT):
    """crossclr_backward_finish_w (prenormalized = 0) or _p; returns the two Outs"""
    lib, dev = nat.library(), xs[0].device
    dtype = xs[0].dtype
    outs = [Out(plan.b, plan.D, dtype, out_layout, dev) for _ in range(2)]
    go_d = device_scalar(go, torch.float64, dev)
    sw = L._sw(None, None, lw_d)
    head = (ctypes.byref(plan), L._ptr(gbuf_d), L._ptr(xs[0]), L._ptr(xs[1]), xs[0].stride(0), xs[1].stride(0), L._IN_DTYPE[dtype], L._ptr(inv_d), tau, sw,
            L._ptr(go_d), L._ptr(outs[0].view), L._ptr(outs[1].view), outs[0].ld, outs[1].ld)
    if prenormalized == 0:
        nat.check(lib.crossclr_backward_finish_w(*head, L._stream_for(xs[0])))
    else:
        nat.check(lib.crossclr_backward_finish_p(*head, prenormalized, L._stream_for(xs[0])))
    sync(dev)
    return outs


def finish_kernel_name(D):
    return "bwd_finish_pair_kernel" if D <= 1024 else "bwd_finish_kernel"


def float32_reciprocal(tau):
    """1.0f / temperature: the temperature is a float argument of the C-ABI and the host hands the kernel its float reciprocal"""
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(tau, dtype=torch.float32))


def check_finish_case(b, D, dtype, layout, mode, device, world=1):
    plan = nat.make_plan(b, D, world, 0, mode)
    assert plan.bwd_slices > 1 and plan.Dpad == DPAD.get(D, {}).get(mode, plan.Dpad)
    gbuf = synthetic_gbuf(plan, b + D + 1)
    M = slice_sum(gbuf, plan)
    gbuf_d = gbuf.to(device)
    lw = torch.stack(xi.sample_weights(b, seed=b + D)[1])                # powers of two, zeros included
    assert bool((lw == 0).any())
    lw_d = stats(lw, plan).to(device)
    raw, raw_inv = raw_rows(b, D, dtype)
    unit, unit_inv = unit_rows(b, D, dtype)
    inputs = {0: (raw, raw_inv), 1: (unit, torch.ones(2, b)), 2: (unit, unit_inv)}
    worst = 0.0
    for prenormalized, weighted in FINISH_VARIANTS:
        x, inv = inputs[prenormalized]
        what = f"backward_finish b={b} D={D} world={world} {dtype_name(dtype)} {layout} {MODE_NAME[mode]} prenormalized={prenormalized} weights={weighted}"
        xs = [lay_in(x[m], dtype, layout, device) for m in range(2)]
        ref = finish_reference(x, M, inv, float32_reciprocal(TAU), b * world, lw if weighted else None, prenormalized)
        outs = run_finish(plan, gbuf_d, xs, stats(inv, plan, NAN).to(device), TAU, lw_d if weighted else None, prenormalized, OUT_LAYOUT[layout])
        assert last_row_kernel() == finish_kernel_name(D), last_row_kernel()
        assert outs[0].ld != xs[0].stride(0)
        for m in range(2):
            worst = max(worst, check_elements(outs[m].read(what), ref["grads"][m], ref["A"][m], dtype, f"{what} modality {m}"))
    print(f"MEASURE backward finish b={b} D={D} world={world} {dtype_name(dtype)} {layout} {MODE_NAME[mode]}: worst err / bar = {worst:.3f}")
    return worst


def maxmargin_reference(x, M, active, go=GRAD_OUT, own_modality_pair=False):
    """include/crossclr.h, crossclr_maxmargin_backward_finish, in float64: column slices summed, positive-pair terms
    -(active_im_i + active_s_i) partner_i, / (B B), x grad_out.  x, M [2, b, D]; active [2, b] (integers as floats)"""
    b = x.shape[1]
    a = (active[0] + active[1]).double()[None, :, None]
    partner = x if own_modality_pair else x.flip(0)
    scale = go / (float(b) * float(b))
    grads = (M - a * partner) * scale
    A = abs(scale) * (M.abs().amax(2, keepdim=True) + (a * partner).abs().amax(2, keepdim=True))
    return {"grads": grads, "A": A.expand(2, b, 1)}


def check_maxmargin_case(b, D, dtype, layout, mode, device):
    lib = nat.library()
    plan = nat.make_plan(b, D, 1, 0, mode)
    assert plan.bwd_slices > 1
    gbuf = synthetic_gbuf(plan, b + D + 2)
    M = slice_sum(gbuf, plan)
    x, _ = unit_rows(b, D, dtype)
    g = torch.Generator().manual_seed(14000 + b + D)
    active = torch.randint(0, b + 1, (2, b), generator=g).float()
    active[0, 0], active[1, 0], active[0, 1], active[1, 1] = 0.0, 0.0, float(b), float(b)
    what = f"maxmargin_backward_finish b={b} D={D} {dtype_name(dtype)} {layout} {MODE_NAME[mode]}"
    xs = [lay_in(x[m], dtype, layout, device) for m in range(2)]
    outs = [Out(b, D, dtype, OUT_LAYOUT[layout], device) for _ in range(2)]
    gbuf_d, act_d, ones_d = gbuf.to(device), stats(active, plan).to(device), stats(torch.ones(2, b), plan).to(device)
    go_d = device_scalar(GRAD_OUT, torch.float64, device)
    nat.check(lib.crossclr_maxmargin_backward_finish(ctypes.byref(plan), L._ptr(gbuf_d), L._ptr(xs[0]), L._ptr(xs[1]), xs[0].stride(0), xs[1].stride(0),
                                                     L._IN_DTYPE[dtype], L._ptr(ones_d), L._ptr(act_d), L._ptr(go_d), L._ptr(outs[0].view),
                                                     L._ptr(outs[1].view), outs[0].ld, outs[1].ld, L._stream_for(xs[0])))
    sync(device)
    assert last_row_kernel() == finish_kernel_name(D), last_row_kernel()
    ref = maxmargin_reference(x, M, active)
    worst = max(check_elements(outs[m].read(what), ref["grads"][m], ref["A"][m], dtype, f"{what} modality {m}") for m in range(2))
    print(f"MEASURE {what}: worst err / bar = {worst:.3f}")
    return worst


# ----------------------------------------------------------------------------------------------------------------------------------
# (4) crossclr_hardneg_backward
# ----------------------------------------------------------------------------------------------------------------------------------
HOT_ROW, FAR_ROW = 5, 2050
_hardneg, _hardneg_ref = {}, {}


def hardneg_inputs(b, D):
    """(x [2, b, D] integers |x| <= 8 -- exact in all four dtypes, and the fp32 sum of up to 4100 of them is exact --, best_index [2, b] int32,
    hinge [2, b] float32):
      (a) modality 0's selections are a random map (never the row itself);
      (b) every entry of modality 1's first stage (entries 0 .. 2047) names HOT_ROW; beyond it a random map again, and for b > 4096 row
          FAR_ROW (an entry of the SECOND stage) is named from the first and the third stage;
      (c) entries of -1 with a positive hinge in both modalities: the documented "no candidate" value, they contribute nothing;
      (d) about half the hinges are zero; the entries that open a stage (2048, 4096) and the last one are active."""
    if (b, D) not in _hardneg:
        g = torch.Generator().manual_seed(15000 + b + D)
        x = torch.randint(-8, 9, (2, b, D), generator=g).double()
        i = torch.arange(b)
        idx = torch.stack([(i + 1 + torch.randint(0, b - 1, (b,), generator=g)) % b for _ in range(2)]).int()
        hinge = torch.where(torch.rand(2, b, generator=g) < 0.5, torch.zeros(2, b), 0.125 + torch.rand(2, b, generator=g)).float()
        idx[1, :min(b, HARDNEG_STAGE)] = HOT_ROW
        for e in (HARDNEG_STAGE, 2 * HARDNEG_STAGE, b - 1):
            if HARDNEG_STAGE <= e < b:
                hinge[:, e] = 0.75
        if b > 2 * HARDNEG_STAGE:
            idx[1, 10], idx[1, 2 * HARDNEG_STAGE + 1] = FAR_ROW, FAR_ROW
            hinge[1, 10], hinge[1, 2 * HARDNEG_STAGE + 1] = 0.5, 0.5
        idx[0, 3], hinge[0, 3], idx[1, 4], hinge[1, 4] = -1, 0.5, -1, 0.25
        assert (idx[0] != i.int()).all() and int((hinge == 0).sum()) > b // 2
        _hardneg[(b, D)] = (x, idx, hinge)
    return _hardneg[(b, D)]


def hardneg_reference(x, idx, hinge, go=GRAD_OUT, stages=None):
    """The closed form of hardneg_backward_kernel's comment in float64.  With O = the OTHER modality's rows, idx / h this modality's selections and
    hinges, idx' / h' the other's, an entry being ACTIVE when its hinge is positive and its index lies in [0, b):
        out[r] = ( [r active] (O[idx[r]] - O[r]) - [r active'] O[r] + sum over the active' entries i with idx'[i] == r of O[i] ) grad_out / B^2
    stages: the stages of kHardnegStage selectors that are taken (a defect for the teeth tests: the second stage dropped)."""
    b = x.shape[1]
    valid = (hinge > 0) & (idx >= 0) & (idx < b)
    out = []
    for m in range(2):
        O = x[1 - m]
        acc = torch.zeros_like(O)
        own = valid[m].nonzero().flatten()
        acc[own] += O[idx[m][own].long()] - O[own]
        other = valid[1 - m].nonzero().flatten()
        acc[other] -= O[other]
        sel = other if stages is None else other[torch.isin(other // HARDNEG_STAGE, torch.tensor(stages))]
        acc.index_add_(0, idx[1 - m][sel].long(), O[sel])
        out.append(acc)
    acc = torch.stack(out)
    assert float(acc.abs().max()) < 2 ** 24
    grads = acc * (go / (float(b) * float(b)))
    return {"grads": grads, "A": grads.abs()}


def check_hardneg_case(b, D, dtype, layout, device):
    lib = nat.library()
    plan = nat.make_plan(b, D, 1, 0, nat.MODE_FP32)
    x, idx, hinge = hardneg_inputs(b, D)
    assert torch.equal(x.to(dtype).double(), x)
    if (b, D) not in _hardneg_ref:          # (integers: the same reference for all four dtypes)
        _hardneg_ref[(b, D)] = hardneg_reference(x, idx, hinge)
    ref = _hardneg_ref[(b, D)]
    what = f"hardneg_backward b={b} D={D} {dtype_name(dtype)} {layout}"
    xs = [lay_in(x[m], dtype, layout, device) for m in range(2)]
    idx_d = torch.full((2, plan.bpad), -1, dtype=torch.int32)
    idx_d[:, :b] = idx
    idx_d, hinge_d = idx_d.to(device), stats(hinge, plan).to(device)
    go_d = device_scalar(GRAD_OUT, torch.float64, device)

    def run(want_im, want_s):
        outs = [Out(b, D, dtype, OUT_LAYOUT[layout], device) for _ in range(2)]
        nat.check(lib.crossclr_hardneg_backward(ctypes.byref(plan), L._ptr(xs[0]), L._ptr(xs[1]), xs[0].stride(0), xs[1].stride(0), L._IN_DTYPE[dtype],
                                                L._ptr(idx_d), L._ptr(hinge_d), L._ptr(go_d), L._ptr(outs[0].view) if want_im else 0,
                                                L._ptr(outs[1].view) if want_s else 0, outs[0].ld, outs[1].ld, L._stream_for(xs[0])))
        sync(device)
        assert last_row_kernel() == "hardneg_backward_kernel"
        return outs
    outs = run(True, True)
    full = [o.read(what) for o in outs]
    worst = max(check_elements(full[m], ref["grads"][m], ref["A"][m], dtype, f"{what} modality {m}") for m in range(2))
    for keep in range(2):
        o2 = run(keep == 0, keep == 1)
        assert torch.equal(o2[keep].read(what).view(torch.uint8), full[keep].view(torch.uint8)), f"{what}: only gradient {keep} asked for"
        assert o2[1 - keep].untouched(), f"{what}: the omitted gradient {1 - keep} was written"
    print(f"MEASURE {what} stages={(b + HARDNEG_STAGE - 1) // HARDNEG_STAGE} slabs={(D + HARDNEG_SLAB - 1) // HARDNEG_SLAB}: worst err / bar = {worst:.3f}")
    return worst


# ----------------------------------------------------------------------------------------------------------------------------------
# (5) the lay-out kernels
# ----------------------------------------------------------------------------------------------------------------------------------
ELEM_BYTES = {nat.MODE_FP32: 4, nat.MODE_BF16: 2, nat.MODE_BF16X3: 4}
OPERAND_KIND = {nat.MODE_FP32: F32, nat.MODE_BF16: BF16, nat.MODE_BF16X3: "bf16x3"}


def decode_operand(raw, mode, rows, Dpad):
    """bytes of a packed operand -> (values [rows, Dpad] float64, the integer view the bit-for-bit comparisons use)"""
    assert raw.dtype == torch.uint8 and raw.numel() == rows * Dpad * ELEM_BYTES[mode]
    if mode == nat.MODE_FP32:
        v = raw.view(torch.float32).view(rows, Dpad)
        return v.double(), v.view(torch.int32)
    if mode == nat.MODE_BF16:
        v = raw.view(torch.bfloat16).view(rows, Dpad)
        return v.double(), v.view(torch.int16)
    v = raw.view(torch.bfloat16).view(rows, Dpad // 32, 2, 32)            # every 32 elements of a row: 32 hi, then 32 lo
    return v[:, :, 0].double().reshape(rows, Dpad) + v[:, :, 1].double().reshape(rows, Dpad), v.view(torch.int16)


def encode_exact(values, mode):
    """the integer view of [rows, Dpad] values that the operand type holds exactly (bf16 values; split operand: lo = 0)"""
    rows, Dpad = values.shape
    assert torch.equal(values.bfloat16().double(), values.double())
    if mode == nat.MODE_FP32:
        return values.float().view(torch.int32)
    if mode == nat.MODE_BF16:
        return values.bfloat16().view(torch.int16)
    hi = values.bfloat16().view(rows, Dpad // 32, 1, 32)
    return torch.cat([hi, torch.zeros_like(hi)], 2).view(torch.int16)


def xf_of_packed(x16):
    """the fragment-major copy of a packed bf16 operand [2 bpad, Dpad] (any 16-bit view), as tests/test_gpu_xf.py decodes it:
    xf[u][dt][ks][h][n][e] = x[32 u + 16 ks + 8 (e >> 2) + 4 h + (e & 3)][32 dt + n]"""
    rows, Dpad = x16.shape
    e = torch.arange(8)
    want = torch.empty(rows // 32, Dpad // 32, 2, 2, 32, 8, dtype=x16.dtype)
    for ks in range(2):
        for h in range(2):
            r = 16 * ks + 8 * (e >> 2) + 4 * h + (e & 3)
            want[:, :, ks, h] = x16.view(rows // 32, 32, Dpad // 32, 32)[:, r].permute(0, 2, 3, 1)
    return want


def layout_reference(x, normalize):
    """x [2, b, D] float64 -> (unit rows x iv in float64, iv [2, b], diag = <x_v, x_t> iv_v iv_t, sum of |terms| of diag): iv = 1 / max(||x||, 1e-12),
    or 1 for the pack entry points"""
    n = x.norm(dim=2)
    iv = torch.where(n > 1e-12, 1.0 / n.clamp_min(1e-300), torch.full_like(n, 1e12)) if normalize else torch.ones_like(n)
    dot, dabs = (x[0] * x[1]).sum(1), (x[0] * x[1]).abs().sum(1)
    return x * iv[:, :, None], iv, dot * iv[0] * iv[1], dabs * iv[0] * iv[1]


def run_layout(entry, plan, xs, with_xf):
    """crossclr_normalize / crossclr_pack (with_xf: the _xf forms) on outputs prefilled with 0x55 / NaN.
    Returns (operand bytes, xf bytes | None, inv_norm [2 bpad], diag_cos [bpad]) on the CPU"""
    lib, dev = nat.library(), xs[0].device
    xhat = torch.full((plan.operand_bytes,), 0x55, dtype=torch.uint8, device=dev)
    xf = torch.full((plan.xf_bytes,), 0x55, dtype=torch.uint8, device=dev) if with_xf else None
    inv = torch.full((2 * plan.bpad,), NAN, dtype=torch.float32, device=dev)
    diag = torch.full((plan.bpad,), NAN, dtype=torch.float32, device=dev)
    head = (ctypes.byref(plan), L._ptr(xs[0]), L._ptr(xs[1]), xs[0].stride(0), xs[1].stride(0), L._IN_DTYPE[xs[0].dtype], L._ptr(xhat))
    tail = (L._ptr(inv), L._ptr(diag), L._stream_for(xs[0]))
    nat.check(getattr(lib, entry + ("_xf" if with_xf else ""))(*head, *((L._ptr(xf),) if with_xf else ()), *tail))
    sync(dev)
    return xhat.cpu(), None if xf is None else xf.cpu(), inv.cpu(), diag.cpu()


def run_topk_pack(x_view, mode, normalize):
    lib, dev = nat.library(), x_view.device
    rows, D = x_view.shape
    n = lib.crossclr_topk_operand_bytes(rows, D, mode)
    rows_pad, Dpad = (rows + 127) // 128 * 128, (D + 63) // 64 * 64
    assert n == rows_pad * Dpad * ELEM_BYTES[mode]
    packed = torch.full((n,), 0x55, dtype=torch.uint8, device=dev)
    nat.check(lib.crossclr_topk_pack(L._ptr(x_view), x_view.stride(0), rows, D, L._IN_DTYPE[x_view.dtype], mode, normalize, L._ptr(packed), L._stream_for(x_view)))
    sync(dev)
    assert last_row_kernel() == "topk_pack_kernel"
    return packed.cpu(), rows_pad, Dpad


def check_packed_values(raw, mode, rows_pad, Dpad, sets, b, D, want, what, exact):
    """a packed operand of `sets` sets of rows_pad rows: rows [b, D] of each against want [sets, b, D] -- bit for bit (exact: the values are bf16
    values) or under the element bar of the operand type --, and zeros on all padding"""
    values, ints = decode_operand(raw, mode, sets * rows_pad, Dpad)
    full = torch.zeros(sets, rows_pad, Dpad, dtype=torch.float64)
    full[:, :b, :D] = want
    worst = 0.0
    if exact:
        assert torch.equal(ints, encode_exact(full.view(sets * rows_pad, Dpad), mode)), f"{what}: packed rows, padding included"
    else:
        v = values.view(sets, rows_pad, Dpad)
        pad = v.clone()
        pad[:, :b, :D] = 0.0
        assert bool((pad == 0).all()) and bool((ints.reshape(sets, rows_pad, -1)[:, b:] == 0).all()), f"{what}: padding of the packed operand"
        worst = check_elements(v[:, :b, :D].reshape(sets * b, D), want.reshape(sets * b, D), want.abs().reshape(sets * b, D), OPERAND_KIND[mode], what)
    return worst


def check_statistics(inv, diag, plan, iv, dg, dabs, what, exact):
    b, bp = plan.b, plan.bpad
    assert bool((inv[b:bp] == 0).all()) and bool((inv[bp + b:] == 0).all()) and bool((diag[b:] == 0).all()), f"{what}: statistics of the padding rows"
    got_iv = torch.stack([inv[:b], inv[bp:bp + b]])
    if exact:
        assert torch.equal(got_iv.double(), iv) and torch.equal(diag[:b].double(), dg), f"{what}: inv_norm / diag_cos"
        return 0.0
    # within 1/2 ulp_fp32 + 1e-12 relative (diag_cos: of the sum of its absolute terms)
    w1 = check_elements(got_iv, iv, iv.abs(), F32, f"{what} inv_norm", via_fp32=False)
    w2 = check_elements(diag[None, :b], dg[None], dabs[None], F32, f"{what} diag_cos", via_fp32=False)
    return max(w1, w2)


_layout_inputs = {}


def layout_inputs(b, D, dtype):
    """(i) the planted sign rows of exact_inputs.planted("mixed") and their unit rows; (ii) random rows with one zero row and one row of norm
    1e-14 (which fp16 cannot hold: there it is a second zero row), as values of `dtype`"""
    key = (b, D, dtype)
    if key not in _layout_inputs:
        yv, yt = xi.planted("mixed", b, D)
        signs = torch.stack([yv, yt]).double()
        x, _ = raw_rows(b, D, F64, eps_row=False)
        x = x.clone()
        x[1, 7] = 0.0
        x[0, 11] *= 1e-14 / x[0, 11].norm()
        _layout_inputs[key] = (signs, torch.nn.functional.normalize(signs, dim=2), x.to(dtype).double())
    return _layout_inputs[key]


def check_layout_case(b, D, dtype, layout, mode, device):
    """crossclr_normalize, crossclr_pack, their _xf forms (bf16 plans up to Dpad = 1024) and crossclr_topk_pack with normalize 0 and 1"""
    plan = nat.make_plan(b, D, 1, 0, mode)
    bp, Dp = plan.bpad, plan.Dpad
    assert plan.operand_bytes == 2 * bp * Dp * ELEM_BYTES[mode]
    signs, sign_units, rnd = layout_inputs(b, D, dtype)
    xf_too = mode == nat.MODE_BF16 and Dp <= 1024
    assert not xf_too or plan.xf_bytes == plan.operand_bytes
    worst = 0.0
    tag = f"b={b} D={D} {dtype_name(dtype)} {layout} {MODE_NAME[mode]}"
    # (entry point, the rows it is given, what they are normalised by, exact)
    runs = [("crossclr_normalize", signs, True, True), ("crossclr_pack", sign_units, False, True),
            ("crossclr_normalize", rnd, True, False), ("crossclr_pack", rnd, False, False)]
    for entry, x, normalize, exact in runs:
        what = f"{entry} {tag} {'sign rows' if exact else 'random rows'}"
        assert torch.equal(x.to(dtype).double(), x)
        xs = [lay_in(x[m], dtype, layout, device) for m in range(2)]
        want, iv, dg, dabs = layout_reference(x, normalize)
        raw, _, inv, diag = run_layout(entry, plan, xs, False)
        assert last_row_kernel() == "normalize_kernel", last_row_kernel()
        worst = max(worst, check_packed_values(raw, mode, bp, Dp, 2, b, D, want, what, exact))
        worst = max(worst, check_statistics(inv, diag, plan, iv, dg, dabs, what, exact))
        if xf_too:      # the row-major half is the plain entry point's bytes, the fragment-major half their permutation
            raw2, xf, inv2, diag2 = run_layout(entry, plan, xs, True)
            assert last_row_kernel() == "normalize_xf_kernel", last_row_kernel()
            assert torch.equal(raw2, raw) and torch.equal(inv2.view(torch.int32), inv.view(torch.int32)) and \
                torch.equal(diag2.view(torch.int32), diag.view(torch.int32)), f"{what}: the _xf form's row-major half"
            assert torch.equal(xf.view(torch.int16).view(2 * bp // 32, Dp // 32, 2, 2, 32, 8), xf_of_packed(raw.view(torch.int16).view(2 * bp, Dp))), \
                f"{what}: the fragment-major half"
        # crossclr_topk_pack on the video rows alone: the same row arithmetic, Dpad = D rounded up to 64
        packed, rows_pad, Dpad64 = run_topk_pack(xs[0], mode, int(normalize))
        worst = max(worst, check_packed_values(packed, mode, rows_pad, Dpad64, 1, b, D, want[:1], f"crossclr_topk_pack normalize={int(normalize)} {tag}", exact))
    print(f"MEASURE lay-out kernels {tag}: worst err / bar = {worst:.3f}")
    return worst
