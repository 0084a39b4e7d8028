"""CPU tests of loss._xf_gate -- the one place that decides whether a hand-scheduled fragment-major backward is verified on a device -- and of
what its three callers make of its answers.  The self-tests are stubs (no kernel runs); the library behind the binding is the host
emulation, told apart from a product build only by `nat.injected_for_testing`, which these tests patch to False."""
import ctypes
import types
import warnings

import pytest
import torch

from crossclr_amd import _native as nat
from crossclr_amd import loss as L

XFP, XF, LDS = "crossclr_backward_saved_xfp", "crossclr_backward_saved_xf", "crossclr_backward_saved"
CPU = torch.device("cpu")
PLAN = types.SimpleNamespace(D=500, Dpad=512, stash_bytes=1 << 20, operand_bytes=1 << 20)


class _FakeGpu:
    """str() and .type of a device; with `capturing` patched in, what the gate sees inside a HIP-graph capture"""
    type = "cuda"

    def __str__(self):
        return "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    from emu import build_emu
    nat.use_library_for_testing(build_emu.build())
    yield
    nat.use_library_for_testing(None)


@pytest.fixture(autouse=True)
def fresh_gate(monkeypatch):
    monkeypatch.setattr(L, "_xf_verified", {})
    monkeypatch.setattr(L, "_xf_launches", {})
    monkeypatch.setattr(L, "_XF_RECHECK", 0)
    monkeypatch.setattr(nat, "injected_for_testing", lambda: False)


@pytest.fixture
def capturing(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)


class _Selftest:
    """A self-test that answers from a list (the last answer repeats) and records how it was asked"""
    def __init__(self, *verdicts):
        self.verdicts, self.calls = list(verdicts), []

    def __call__(self, dev, D, weighted, name):
        self.calls.append((dev, D, weighted, name))
        return self.verdicts.pop(0) if len(self.verdicts) > 1 else self.verdicts[0]


def _key(name, dev="cpu", weighted=False):
    return (dev, PLAN.Dpad, weighted, name, nat.library_path())


def test_verified_once_then_cached():
    st = _Selftest(True)
    assert L._xf_gate(CPU, PLAN, False, XFP, st) is True
    assert L._xf_gate(CPU, PLAN, False, XFP, st) is True
    assert st.calls == [(CPU, PLAN.D, False, XFP)]                # asked once, with the unpadded width
    assert L._xf_verified == {_key(XFP): True}
    assert L._xf_gate(CPU, PLAN, True, XFP, st) is True           # sample weights: another instantiation, verified on its own
    assert len(st.calls) == 2 and L._xf_verified == {_key(XFP): True, _key(XFP, weighted=True): True}


@pytest.mark.parametrize("name,text", [(XFP, XFP + " disagrees"), (L._XF_REMOTE, "_t_xfp disagree with the LDS-staged kernels")])
def test_a_false_verdict_warns_once_and_is_cached(name, text):
    st = _Selftest(False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert L._xf_gate(CPU, PLAN, False, name, st) is False
        assert L._xf_gate(CPU, PLAN, False, name, st) is False
    assert len(st.calls) == 1 and L._xf_verified == {_key(name): False}
    assert [text in str(x.message) and "Dpad = 512" in str(x.message) for x in w] == [True]


def test_nothing_to_compare_is_cached_as_false_without_a_warning():
    st = _Selftest(None)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert L._xf_gate(CPU, PLAN, False, XF, st) is False
        assert L._xf_gate(CPU, PLAN, False, XF, st) is False
    assert len(st.calls) == 1 and L._xf_verified == {_key(XF): False} and not w


def test_recheck_every_nth_question_and_never_at_zero(monkeypatch):
    st = _Selftest(True)
    for _ in range(10):
        assert L._xf_gate(CPU, PLAN, False, XFP, st) is True
    assert len(st.calls) == 1 and L._xf_launches == {}            # CROSSCLR_XF_RECHECK_STEPS = 0: verified once, for good
    monkeypatch.setattr(L, "_XF_RECHECK", 3)
    asked = []
    for _ in range(9):                                            # questions about a verified instantiation: the 3rd, 6th and 9th run the self-test
        assert L._xf_gate(CPU, PLAN, False, XFP, st) is True
        asked.append(len(st.calls) - 1)
    assert asked == [0, 0, 1, 1, 1, 2, 2, 2, 3]
    st.verdicts = [False]                                         # a recheck that fails disables the kernel like a first check does
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        answers = [L._xf_gate(CPU, PLAN, False, XFP, st) for _ in range(6)]
    assert answers == [True, True, False, False, False, False] and len(w) == 1 and len(st.calls) == 5


def test_inside_a_capture_nothing_is_verified_and_nothing_written(capturing, monkeypatch):
    st, gpu = _Selftest(True), _FakeGpu()
    assert L._xf_gate(gpu, PLAN, False, XFP, st) is None
    assert st.calls == [] and L._xf_verified == {}
    assert L._xf_gate(CPU, PLAN, False, XFP, st) is True          # (a CPU tensor's stream is never capturing)
    # verified before the capture: the answer stands inside it, and a recheck that falls due there is skipped
    L._xf_verified[_key(XFP, "cuda:0")] = True
    monkeypatch.setattr(L, "_XF_RECHECK", 1)
    assert L._xf_gate(gpu, PLAN, False, XFP, st) is True and len(st.calls) == 1


def test_the_injected_build_answers_true(monkeypatch):
    monkeypatch.setattr(nat, "injected_for_testing", lambda: True)
    st = _Selftest(False)
    assert L._xf_gate(CPU, PLAN, False, XFP, st) is True and st.calls == []


# ---- the callers: what each makes of None (cannot be verified now) and of False ----

def _step_plan():
    plan = nat.make_plan(2048, 512, 1, 0, nat.MODE_BF16)          # the library's choice here: the pair kernel on the fragment-major copy
    lay = nat.StepLayout()
    nat.check(nat.library().crossclr_step_plan(ctypes.byref(plan), 0.05, 0.8, 0, 0, ctypes.byref(lay)))
    assert lay.backward_kernel == 3
    return plan


def test_step_flags_inside_a_capture_takes_both_kernels_out(capturing, monkeypatch):
    monkeypatch.setattr(L, "_xf_selftest", _Selftest(True))
    flags, lay = L._step_flags(_step_plan(), 0, 0.05, 0.8, False, _FakeGpu())
    assert flags == nat.STEP_NO_XFP | nat.STEP_NO_XF and lay.backward_kernel == 1 and lay.saved == 1
    assert L._xf_selftest.calls == [] and L._xf_verified == {}


def test_step_flags_takes_a_rejected_kernel_out_and_plans_again(monkeypatch):
    monkeypatch.setattr(L, "_xf_selftest", _Selftest(False, True))      # the pair kernel disagrees, the one-tile kernel is fine
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        flags, lay = L._step_flags(_step_plan(), 0, 0.05, 0.8, False, CPU)
    assert flags == nat.STEP_NO_XFP and lay.backward_kernel == 2 and len(w) == 1
    assert [c[3] for c in L._xf_selftest.calls] == [XFP, XF]
    flags, lay = L._step_flags(_step_plan(), 0, 0.05, 0.8, False, CPU)      # both verdicts cached
    assert flags == nat.STEP_NO_XFP and lay.backward_kernel == 2 and len(L._xf_selftest.calls) == 2


def test_saved_backward_entry_translations(capturing, monkeypatch):
    ws = types.SimpleNamespace(xf=object(), k_rows=None)
    monkeypatch.setattr(L, "_xf_selftest", _Selftest(False))
    assert L._saved_backward_entry(ws, PLAN, _FakeGpu()) == LDS and L._xf_selftest.calls == []      # None: the LDS-staged kernel, nothing asked
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert L._saved_backward_entry(ws, PLAN, CPU) == LDS                                        # False: the next candidate, then the LDS-staged kernel
    assert [c[3] for c in L._xf_selftest.calls] == [XFP, XF] and len(w) == 2
    L._xf_verified[_key(XF)] = True
    assert L._saved_backward_entry(ws, PLAN, CPU) == XF


def test_remote_xfp_translations(capturing, monkeypatch):
    ws = types.SimpleNamespace(xf=object(), k_rows=None, world=3, saved_blocks=[])
    monkeypatch.setattr(L, "_xf_selftest_remote", _Selftest(False))
    gpu = _FakeGpu()
    L._xf_verified[_key(XFP, "cuda:0")] = L._xf_verified[_key(XFP)] = True      # the local block's pair kernel is verified on both devices
    assert L._remote_xfp(ws, PLAN, nat.library(), None, gpu) is False           # None: remote blocks keep the LDS-staged kernels
    assert L._xf_selftest_remote.calls == [] and _key(L._XF_REMOTE, "cuda:0") not in L._xf_verified
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert L._remote_xfp(ws, PLAN, nat.library(), None, CPU) is False       # False
    assert len(w) == 1 and L._xf_verified[_key(L._XF_REMOTE)] is False
    L._xf_verified[_key(L._XF_REMOTE)] = True
    assert L._remote_xfp(ws, PLAN, nat.library(), None, CPU) is True
