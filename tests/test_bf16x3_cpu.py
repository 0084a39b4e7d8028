"""CPU tests (host emulation) of compute_mode="bf16x3" (include/crossclr.h ABI 8, CROSSCLR_MODE_BF16X3): fp32-accurate products on
the bf16 matrix cores -- every unit row split into hi = bf16(x), lo = bf16(x - hi), every product hi.hi + hi.lo + lo.hi.
* plans: single device only; the split plan is refused by the entry points it has no kernels for;
* the reference's float32 goldens with B <= 256 at the fp32 mode's bars (tests/test_gpu_parity.py), through the saved, the
  recomputing and the forward-only step, which agree with each other;
* per-sample weights against oracle/influence_oracle.py;
* a float64 model of the split (products exact, positive-pair logit from the fp32 rows) pins the emulated loss;
* crossclr_last_kernel names the split instantiations: the mode did not quietly run the f32 MFMA kernels."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import crossclr_amd
from conftest import golden_arrays, golden_index, golden_inputs
from crossclr_amd import _native as nat
from crossclr_amd import loss as L
from oracle import crossclr_oracle as orc
from oracle import influence_oracle as inf

IDX = golden_index()
SMALL = [n for n, m in IDX.items() if m["B"] <= 256 and m["dtype"] == "float32"]


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    from emu import build_emu
    nat.use_library_for_testing(build_emu.build())
    yield
    nat.use_library_for_testing(None)


def split_model_loss(v, t, tau, w):
    """float64 model of the split products: unit rows in fp32 (as the normalisation kernel leaves them), hi = bf16(x), lo = bf16(x - hi),
    S = hi hi' + hi lo' + lo hi' evaluated exactly; the positive-pair logit from the fp32 rows."""
    vh, th = F.normalize(v.double(), dim=1).float(), F.normalize(t.double(), dim=1).float()

    def parts(x):
        hi = x.bfloat16().float()
        return hi.double(), (x - hi).bfloat16().double()
    vhi, vlo = parts(vh)
    thi, tlo = parts(th)

    def prod(ahi, alo, bhi, blo):
        return ahi @ bhi.t() + ahi @ blo.t() + alo @ bhi.t()
    B = v.shape[0]
    a = prod(vhi, vlo, thi, tlo) / tau
    cv = prod(vhi, vlo, vhi, vlo) * (w / tau)
    ct = prod(thi, tlo, thi, tlo) * (w / tau)
    eye = torch.eye(B, dtype=torch.bool)
    cv[eye] = 0.0
    ct[eye] = 0.0
    lzv = torch.logsumexp(torch.cat([a, cv], 1), 1)
    lzt = torch.logsumexp(torch.cat([a.t(), ct], 1), 1)
    diag = (vh.double() * th.double()).sum(1) / tau
    return float((lzv + lzt - 2 * diag).sum() / (2 * B))


def loss_and_grads(v, t, tau, w, **kw):
    vv, tt = v.clone().requires_grad_(True), t.clone().requires_grad_(True)
    loss = crossclr_amd.crossclr_loss(vv, tt, tau, w, compute_mode="bf16x3", **kw)
    loss.backward()
    return loss.item(), vv.grad, tt.grad


def bars(m):
    """the fp32 mode's bars (tests/test_gpu_parity.py) with the issue's allowance: twice the gradient bar in the two-pass regime"""
    tau, B = m["temperature"], m["B"]
    ltol = 2e-5 * max(1.0, abs(m["loss"])) + 2e-8 / tau
    scale = max(m["grad_v_absmax"], m["grad_t_absmax"])
    gtol = max(2e-4, 4e-7 / tau) * scale + 1e-7 / (B * tau)
    if max(1.0, abs(m["negative_weight"])) / tau > 128:
        gtol *= 2
    if scale < 1e-9:
        # aligned goldens (loss ~0, reference gradients <= 3e-12): only the floor term is left, where the split's positive-pair
        # exponential (hi/lo products, lo.lo left out) and the fp32 positive-pair logit of the numerator differ: twice the floor
        gtol *= 2
    return ltol, gtol


def test_plan_is_single_device_and_shaped_like_fp32():
    p3 = nat.make_plan(200, 300, 1, 0, nat.MODE_BF16X3)
    p32 = nat.make_plan(200, 300, 1, 0, nat.MODE_FP32)
    assert p3.mode == nat.MODE_BF16X3 and p3.fast_path == 0 and p3.fast_bwd == 0 and p3.xf_bytes == 0
    assert (p3.bpad, p3.Dpad, p3.operand_bytes, p3.stash_bytes, p3.gbuf_bytes) == \
           (p32.bpad, p32.Dpad, p32.operand_bytes, p32.stash_bytes, p32.gbuf_bytes)
    assert p3.operand_bytes == 2 * p3.bpad * p3.Dpad * 4 and p3.stash_bytes == (2 * p3.bpad) ** 2 * 4
    with pytest.raises(nat.CrossCLRNativeError, match="single-device"):
        nat.make_plan(200, 300, 2, 0, nat.MODE_BF16X3)
    assert nat.library().crossclr_abi_version() == 8


def test_entry_points_without_split_kernels_refuse_the_plan():
    lib = nat.library()
    plan = nat.make_plan(64, 64, 1, 0, nat.MODE_BF16X3)
    pp = ctypes.byref(plan)
    buf = torch.zeros(1 << 20, dtype=torch.float32)
    p = buf.data_ptr()
    assert lib.crossclr_score_diag(pp, p, p, 0) == -1
    assert "BF16X3" in lib.crossclr_last_error().decode()
    assert lib.crossclr_maxmargin_backward(pp, p, p, ctypes.c_float(0.1), p, 0) == -1
    assert lib.crossclr_normalize_xf(pp, p, p, 64, 64, nat.IN_F32, p, p, p, p, 0) == -1
    assert lib.crossclr_project_backward_prep(pp, p, p, 64, 64, p, p, p, p, 64, 0) == -1
    assert lib.crossclr_backward_saved_xf(pp, p, p, ctypes.c_float(0.05), ctypes.c_float(0.8), p, p, None, p, 0, 0) == -1
    assert lib.crossclr_backward_ranks(pp, p, p, 0, 1, ctypes.c_float(0.05), ctypes.c_float(0.8), p, p, p, p, None, p, 0, 0) == -1
    v, t = orc.make_inputs("randn", 16, 32, 1)
    with pytest.raises(nat.CrossCLRNativeError):      # the score statistics keep their own modes
        crossclr_amd.max_margin_loss(v, t, 0.1, compute_mode="bf16x3")


@pytest.mark.parametrize("name", SMALL)
def test_goldens_at_the_fp32_bars(name):
    m = IDX[name]
    v, t = golden_inputs(m)
    loss, gv, gt = loss_and_grads(v, t, m["temperature"], m["negative_weight"])
    lib = nat.library()
    assert lib.crossclr_last_kernel(0).startswith(b"fwd_sums_kernel<x3_t>")
    assert lib.crossclr_last_kernel(1).startswith(b"bwd_saved_x3_kernel")
    ltol, gtol = bars(m)
    assert abs(loss - m["loss"]) <= ltol, (loss, m["loss"])
    arr = golden_arrays(name)
    assert np.abs(gv.double().numpy() - arr["grad_v"].astype(np.float64)).max() <= gtol
    assert np.abs(gt.double().numpy() - arr["grad_t"].astype(np.float64)).max() <= gtol
    if m["temperature"] >= 0.02:
        model = split_model_loss(v, t, m["temperature"], m["negative_weight"])
        # (+ the fp32 accumulation floor of the logits, 2e-8 / tau: the model's products are exact; it decides at loss ~0, aligned rows)
        assert abs(loss - model) <= 1e-6 * max(1.0, abs(model)) + 2e-8 / m["temperature"], (loss, model)


@pytest.mark.parametrize("B,D,tau,w", [(100, 48, 0.05, 0.8), (130, 200, 0.004, 1.0)])
def test_saved_recomputing_and_forward_only_agree(B, D, tau, w, monkeypatch):
    v, t = orc.make_inputs("randn", B, D, 11)
    lib = nat.library()
    loss_s, gv_s, gt_s = loss_and_grads(v, t, tau, w)
    assert lib.crossclr_last_kernel(1).startswith(b"bwd_saved_x3_kernel")
    monkeypatch.setenv("CROSSCLR_DISABLE_SAVE", "1")
    loss_r, gv_r, gt_r = loss_and_grads(v, t, tau, w)
    assert lib.crossclr_last_kernel(1).startswith(b"bwd_kernel<x3_t>")
    monkeypatch.delenv("CROSSCLR_DISABLE_SAVE")
    with torch.no_grad():
        loss_f = crossclr_amd.crossclr_loss(v, t, tau, w, compute_mode="bf16x3").item()
    assert lib.crossclr_last_kernel(0).startswith(b"fwd_sums_kernel<x3_t>")
    # the forward is the same launch whether or not it saves: the same sums, the same loss
    assert loss_s == loss_r == loss_f
    scale = max(gv_s.abs().max().item(), gt_s.abs().max().item())
    # the saved weights are the forward's fp32 exponentials, the recomputed ones come from a differently ordered product: fp32 noise
    gtol = 2e-5 * scale + 1e-7 / (B * tau)
    assert (gv_s - gv_r).abs().max().item() <= gtol and (gt_s - gt_r).abs().max().item() <= gtol
    ref = orc.streaming_loss_and_grads(v, t, tau, w)
    assert abs(loss_s - float(ref["loss"])) <= 2e-5 * max(1.0, abs(float(ref["loss"]))) + 2e-8 / tau


@pytest.mark.parametrize("tau", [0.05, 0.004])
def test_sample_weights_against_the_influence_oracle(tau):
    B, D = 96, 40
    v, t = orc.make_inputs("randn", B, D, 5)
    g = torch.Generator().manual_seed(2)
    kv, kt = (torch.rand(B, generator=g) > 0.3).float(), 2 * torch.rand(B, generator=g)
    ov, ot = 2 * torch.rand(B, generator=g), 0.5 + torch.rand(B, generator=g)
    loss, gv, gt = loss_and_grads(v, t, tau, 0.8, negative_scale=(kv, kt), loss_weight=(ov, ot))
    want = inf.streaming_weighted_loss_and_grads(v, t, tau, 0.8, kv, kt, ov, ot)
    wl = float(want["loss"])
    assert abs(loss - wl) <= 2e-5 * max(1.0, abs(wl)) + 2e-8 / tau
    scale = max(want["grad_v"].abs().max().item(), want["grad_t"].abs().max().item())
    gtol = max(2e-4, 4e-7 / tau) * scale + 1e-7 / (B * tau)
    if 1.0 / tau > 128:
        gtol *= 2
    assert (gv.double() - want["grad_v"]).abs().max().item() <= gtol
    assert (gt.double() - want["grad_t"]).abs().max().item() <= gtol


def test_mode_resolution_and_the_single_device_rule(tmp_path, monkeypatch):
    assert L._resolve_mode("bf16x3", 8192) == nat.MODE_BF16X3
    with pytest.raises(ValueError, match="bf16x3"):
        L._resolve_mode("tf32", 16)
    crit = crossclr_amd.CrossCLR_onlyIntraModality(0.03, 0.8, compute_mode="bf16x3")
    assert "bf16x3" in repr(crit)
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'store'}", rank=0, world_size=1)
    try:
        monkeypatch.setenv("CROSSCLR_FORCE_SHARDED_PATH", "1")
        v, t = orc.make_inputs("randn", 16, 32, 1)
        with pytest.raises(ValueError, match="bf16x3 is single-device"):
            crossclr_amd.crossclr_loss(v, t, 0.05, 0.8, compute_mode="bf16x3", process_group=dist.group.WORLD)
    finally:
        dist.destroy_process_group()
