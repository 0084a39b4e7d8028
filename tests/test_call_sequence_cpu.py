"""The host path of the sharded and the fused-projection step (`loss._forward_impl` / `_backward_impl`) decides which kernels run, in which
order, and which collectives every rank enters together.  This test pins that order: per rank, every launch through the C-ABI (entry
name, the non-pointer arguments, null / non-null for each pointer) and every `torch.distributed` collective, with the waits on their
handles where they fall between the launches.  The expected sequences below were recorded on the host path as it stood before it was cut
into stages; a restructuring of that path must reproduce them line for line (a deliberate change of the order regenerates the table:
`python tests/test_call_sequence_cpu.py` prints it).

Each run is a forward + backward, then a forward under no_grad, on the emulated build of the kernel sources (tests/emu)."""
import ctypes
import io
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# queries that launch nothing and enter no collective: how often the host asks them is not part of the order
_QUERIES = ("crossclr_abi_version", "crossclr_make_plan", "crossclr_needs_row_shift", "crossclr_step_plan")
_COLLECTIVES = ("all_reduce", "all_gather_into_tensor", "all_to_all_single", "batch_isend_irecv")
_XF_ALL_WIDTHS = "128,256,384,512,768,1024"

# name -> (world, B, D, compute mode, temperature, environment)
CONFIGS = {
    "fp32_w2": (2, 24, 20, "fp32", 0.05, {}),
    "fp32_w2_two_pass": (2, 24, 20, "fp32", 0.004, {}),       # small temperature; the remote block saves U and Ut (remote save is on)
    "bf16_w3": (3, 24, 16, "bf16", 0.05, {}),
    "bf16_w4_p2p_each": (4, 24, 16, "bf16", 0.05, {"CROSSCLR_EXCHANGE": "p2p_each"}),
    "bf16_w4_allgather": (4, 24, 16, "bf16", 0.05, {"CROSSCLR_EXCHANGE": "allgather"}),
    "bf16_w5": (5, 20, 16, "bf16", 0.05, {}),
    "bf16_w3_recompute": (3, 24, 16, "bf16", 0.05, {"CROSSCLR_PARTNER_GRADS": "0"}),
    "bf16_w3_nopairs": (3, 24, 16, "bf16", 0.05, {"CROSSCLR_DISABLE_PAIR_FORWARD": "1"}),
    # 130 rows per rank; every width takes the fragment-major pair: local block on crossclr_backward_saved_xfp, remote blocks on _rect_saved_xfp
    "bf16_w3_xf": (3, 390, 16, "bf16", 0.05, {"CROSSCLR_XF_WIDTHS": _XF_ALL_WIDTHS}),
    # one process, no group: projected_crossclr_loss, b = 40, Din = 48, D = 32
    "projection": (1, 40, 32, "projection", 0.05, {}),
}


def _format(x, ctype) -> str:
    if ctype is ctypes.c_float:
        return "%g" % x
    if ctype is ctypes.c_void_p:
        addr = x.value if isinstance(x, ctypes.c_void_p) else x
        return "p" if addr else "0"
    if ctype in (ctypes.c_int, ctypes.c_long, ctypes.c_uint, ctypes.c_size_t):
        return str(int(x))
    return "0" if x is None else "s"        # pointer to a structure (plan, sample weights)


class _Work:
    """A collective's handle whose wait() is logged"""
    def __init__(self, work, what, log):
        self._work, self._what, self._log = work, what, log

    def wait(self, *a):
        self._log.append("wait " + self._what)
        return self._work.wait(*a)


def _install_recorder(nat, log) -> None:
    lib = nat.library()
    for name in nat.EXPORTED_SYMBOLS:
        res, argtypes = nat._SIGNATURES[name]
        if res is not ctypes.c_int or name in _QUERIES:
            continue

        def entry(*args, _name=name, _real=getattr(lib, name), _types=argtypes):
            assert len(args) == len(_types), _name
            log.append(_name.replace("crossclr_", "", 1) + " " + " ".join(_format(x, t) for x, t in zip(args, _types)))
            return _real(*args)
        setattr(lib, name, entry)
    for name in _COLLECTIVES:
        def collective(*args, _name=name, _real=getattr(dist, name), **kw):
            log.append("dist." + _name)
            got = _real(*args, **kw)
            if isinstance(got, list):
                return [_Work(w, _name, log) for w in got]
            return got if got is None else _Work(got, _name, log)
        setattr(dist, name, collective)


def _worker(rank, name, port, q):
    try:
        world, B, D, mode, tau, env = CONFIGS[name]
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.update(env)
        group = None
        if world > 1:
            os.environ["MASTER_ADDR"] = "127.0.0.1"
            os.environ["MASTER_PORT"] = str(port)
            dist.init_process_group("gloo", rank=rank, world_size=world)
            group = dist.group.WORLD
        import crossclr_amd
        from crossclr_amd import _native as nat
        from emu import build_emu
        from oracle import crossclr_oracle as orc
        nat.use_library_for_testing(build_emu.OUT)
        log = []
        _install_recorder(nat, log)
        b = B // world
        if mode == "projection":
            g = torch.Generator().manual_seed(91)
            leaves = [torch.randn(b, 48, generator=g), torch.randn(b, 48, generator=g),                       # inputs of the two heads,
                      torch.randn(D, 48, generator=g) / 48 ** 0.5, 0.1 * torch.randn(D, generator=g),         # their weights and biases
                      torch.randn(D, 48, generator=g) / 48 ** 0.5, 0.1 * torch.randn(D, generator=g)]
            leaves = [x.requires_grad_(True) for x in leaves]
            step = lambda: crossclr_amd.projected_crossclr_loss(*leaves, tau, 0.7)
        else:
            v, t = orc.make_inputs("randn", B, D, 77)
            leaves = [v[rank * b:(rank + 1) * b].clone().requires_grad_(True), t[rank * b:(rank + 1) * b].clone().requires_grad_(True)]
            crit = crossclr_amd.CrossCLR_onlyIntraModality(tau, 0.7, compute_mode=mode, process_group=group)
            step = lambda: crit(*leaves)
        loss = step()
        loss.backward()
        # (detached inputs: an autograd function sees `needs_input_grad` of inputs that require grad under no_grad as well, and would save)
        log.append("-- forward under no_grad --")
        grads = [x.grad for x in leaves[:2]]
        leaves = [x.detach() for x in leaves]
        with torch.no_grad():
            step()
        blob = io.BytesIO()       # (by value: a tensor in a queue is a file descriptor of a process that may be gone when it is read)
        torch.save([loss.detach()] + grads, blob)
        q.put((rank, "\n".join(log), blob.getvalue()))
        if world > 1:
            dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc()))


def run(name):
    """[(call sequence as one string, torch.save of [loss, grad_video, grad_text])] by rank; the tensors are for comparing two trees"""
    from emu import build_emu
    build_emu.build()
    world = CONFIGS[name][0]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000) + 60 + world
    procs = [ctx.Process(target=_worker, args=(r, name, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    for rank, log, info in results:
        assert log != "error", info
    return [(log, info) for _, log, info in results]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_call_sequence_per_rank(name):
    got = [log for log, _ in run(name)]
    want = [s.strip() for s in EXPECTED[name]]
    assert len(got) == len(want)
    for rank, (g, w) in enumerate(zip(got, want)):
        if g != w:
            import difflib
            diff = "\n".join(difflib.unified_diff(w.split("\n"), g.split("\n"), "expected", "this tree", lineterm=""))
            pytest.fail(f"{name}, rank {rank}: the sequence of C-ABI calls / collectives moved\n{diff}")


# one string per rank, in rank order (pointers: p / 0; structures: s / 0; integers and floats as passed)
EXPECTED = {
    "fp32_w2": [
        """
dist.all_reduce
normalize s p p 20 20 0 p p p 0
dist.all_gather_into_tensor
forward_save s p 0.05 0.7 0 p 0 p 0
wait all_gather_into_tensor
forward_rect_save s p p 1 1 0 0.05 0.7 0 p 2 0 p 0
forward_finish_w s p 4 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved s p p 1 1 0.05 0.7 p p p p 0 p 1 0
backward_finish_p s p p p 20 20 0 p 0.05 0 p p p 20 20 0 0
-- forward under no_grad --
normalize s p p 20 20 0 p p p 0
dist.all_gather_into_tensor
forward_w s p p 1 0 -1 0.05 0.7 0 p 0 0
wait all_gather_into_tensor
forward_w s p p 2 0 0 0.05 0.7 0 p 2 0
forward_finish_w s p 4 p 0.05 0.7 0 p p p p 0
dist.all_reduce
""",
        """
dist.all_reduce
normalize s p p 20 20 0 p p p 0
dist.all_gather_into_tensor
forward_save s p 0.05 0.7 0 p 0 p 0
wait all_gather_into_tensor
forward_rect_save s p p 0 1 0 0.05 0.7 0 p 2 0 p 0
forward_finish_w s p 4 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved s p p 0 1 0.05 0.7 p p p p 0 p 1 0
backward_finish_p s p p p 20 20 0 p 0.05 0 p p p 20 20 0 0
-- forward under no_grad --
normalize s p p 20 20 0 p p p 0
dist.all_gather_into_tensor
forward_w s p p 1 1 -1 0.05 0.7 0 p 0 0
wait all_gather_into_tensor
forward_w s p p 2 0 1 0.05 0.7 0 p 2 0
forward_finish_w s p 4 p 0.05 0.7 0 p p p p 0
dist.all_reduce
""",
    ],
    "fp32_w2_two_pass": [
        """
dist.all_reduce
normalize s p p 20 20 0 p p p 0
dist.all_gather_into_tensor
forward_rowmax s p p 1 0 -1 0.004 0.7 0 p p 0 0
wait all_gather_into_tensor
forward_rowmax s p p 2 0 0 0.004 0.7 0 p p 1 0
dist.all_gather_into_tensor
forward_save_s s p 0.004 0.7 0 p p 0 p 0
forward_rect_save_s s p p 1 1 0.004 0.7 0 p p p 2 p 0
forward_finish_s s p 4 p 0.004 0.7 0 p p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved_s s p p 0.004 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_s s p p 1 1 0.004 0.7 p p p p 0 p 1 0
backward_finish_p s p p p 20 20 0 p 0.004 0 p p p 20 20 0 0
-- forward under no_grad --
normalize s p p 20 20 0 p p p 0
dist.all_gather_into_tensor
forward_rowmax s p p 1 0 -1 0.004 0.7 0 p p 0 0
wait all_gather_into_tensor
forward_rowmax s p p 2 0 0 0.004 0.7 0 p p 1 0
forward_s s p p 1 0 -1 0.004 0.7 0 p p 0 0
forward_s s p p 2 0 0 0.004 0.7 0 p p 2 0
forward_finish_s s p 4 p 0.004 0.7 0 p p p p p 0
dist.all_reduce
""",
        """
dist.all_reduce
normalize s p p 20 20 0 p p p 0
dist.all_gather_into_tensor
forward_rowmax s p p 1 1 -1 0.004 0.7 0 p p 0 0
wait all_gather_into_tensor
forward_rowmax s p p 2 0 1 0.004 0.7 0 p p 1 0
dist.all_gather_into_tensor
forward_save_s s p 0.004 0.7 0 p p 0 p 0
forward_rect_save_s s p p 0 1 0.004 0.7 0 p p p 2 p 0
forward_finish_s s p 4 p 0.004 0.7 0 p p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved_s s p p 0.004 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_s s p p 0 1 0.004 0.7 p p p p 0 p 1 0
backward_finish_p s p p p 20 20 0 p 0.004 0 p p p 20 20 0 0
-- forward under no_grad --
normalize s p p 20 20 0 p p p 0
dist.all_gather_into_tensor
forward_rowmax s p p 1 1 -1 0.004 0.7 0 p p 0 0
wait all_gather_into_tensor
forward_rowmax s p p 2 0 1 0.004 0.7 0 p p 1 0
forward_s s p p 1 1 -1 0.004 0.7 0 p p 0 0
forward_s s p p 2 0 1 0.004 0.7 0 p p 2 0
forward_finish_s s p 4 p 0.004 0.7 0 p p p p p 0
dist.all_reduce
""",
    ],
    "bf16_w3": [
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 1 1 1 0.05 0.7 0 p 8 p p 0
dist.all_to_all_single
forward_add s p 16 p 0
forward_finish_w s p 24 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 1 1 0 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 1 1 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 0 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 1 1 0.05 0.7 0 p 8 p 0
dist.all_to_all_single
forward_add s p 16 p 0
forward_finish_w s p 24 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 2 1 1 0.05 0.7 0 p 8 p p 0
dist.all_to_all_single
forward_add s p 16 p 0
forward_finish_w s p 24 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 2 1 0 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 2 1 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 1 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 2 1 0.05 0.7 0 p 8 p 0
dist.all_to_all_single
forward_add s p 16 p 0
forward_finish_w s p 24 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 0 1 1 0.05 0.7 0 p 8 p p 0
dist.all_to_all_single
forward_add s p 16 p 0
forward_finish_w s p 24 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 0 1 0 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 0 1 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 2 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 0 1 0.05 0.7 0 p 8 p 0
dist.all_to_all_single
forward_add s p 16 p 0
forward_finish_w s p 24 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
""",
    ],
    "bf16_w4_p2p_each": [
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 1 1 1 0.05 0.7 0 p 12 p p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 2 1 0 0.05 0.7 0 p 24 0 p 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 1 1 0 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 1 1 0.05 0.7 p p p p 0 p 1 0
backward_rect_saved s p p 2 1 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 0 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 1 1 0.05 0.7 0 p 12 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_w s p p 1 2 -1 0.05 0.7 0 p 24 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 2 1 1 0.05 0.7 0 p 12 p p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 3 1 0 0.05 0.7 0 p 24 0 p 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 2 1 0 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 2 1 0.05 0.7 p p p p 0 p 1 0
backward_rect_saved s p p 3 1 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 1 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 2 1 0.05 0.7 0 p 12 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_w s p p 1 3 -1 0.05 0.7 0 p 24 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 3 1 1 0.05 0.7 0 p 12 p p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 0 1 0 0.05 0.7 0 p 24 0 p 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 3 1 0 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 3 1 0.05 0.7 p p p p 0 p 1 0
backward_rect_saved s p p 0 1 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 2 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 3 1 0.05 0.7 0 p 12 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_w s p p 1 0 -1 0.05 0.7 0 p 24 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 0 1 1 0.05 0.7 0 p 12 p p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 1 1 0 0.05 0.7 0 p 24 0 p 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 0 1 0 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 0 1 0.05 0.7 p p p p 0 p 1 0
backward_rect_saved s p p 1 1 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 3 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 0 1 0.05 0.7 0 p 12 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_w s p p 1 1 -1 0.05 0.7 0 p 24 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
""",
    ],
    "bf16_w4_allgather": [
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.all_gather_into_tensor
forward_save s p 0.05 0.7 0 p 0 p 0
wait all_gather_into_tensor
forward_rect_save s p p 1 1 1 0.05 0.7 0 p 12 p p 0
forward_rect_save s p p 2 1 0 0.05 0.7 0 p 24 0 p 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 1 1 0 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 1 1 0.05 0.7 p p p p 0 p 1 0
backward_rect_saved s p p 2 1 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.all_gather_into_tensor
forward_w s p p 1 0 -1 0.05 0.7 0 p 0 0
wait all_gather_into_tensor
forward_pairs s p p 1 1 0.05 0.7 0 p 12 p 0
forward_w s p p 1 2 -1 0.05 0.7 0 p 24 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.all_gather_into_tensor
forward_save s p 0.05 0.7 0 p 0 p 0
wait all_gather_into_tensor
forward_rect_save s p p 2 1 1 0.05 0.7 0 p 12 p p 0
forward_rect_save s p p 3 1 0 0.05 0.7 0 p 24 0 p 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 2 1 0 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 2 1 0.05 0.7 p p p p 0 p 1 0
backward_rect_saved s p p 3 1 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.all_gather_into_tensor
forward_w s p p 1 1 -1 0.05 0.7 0 p 0 0
wait all_gather_into_tensor
forward_pairs s p p 2 1 0.05 0.7 0 p 12 p 0
forward_w s p p 1 3 -1 0.05 0.7 0 p 24 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.all_gather_into_tensor
forward_save s p 0.05 0.7 0 p 0 p 0
wait all_gather_into_tensor
forward_rect_save s p p 3 1 1 0.05 0.7 0 p 12 p p 0
forward_rect_save s p p 0 1 0 0.05 0.7 0 p 24 0 p 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 3 1 0 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 3 1 0.05 0.7 p p p p 0 p 1 0
backward_rect_saved s p p 0 1 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.all_gather_into_tensor
forward_w s p p 1 2 -1 0.05 0.7 0 p 0 0
wait all_gather_into_tensor
forward_pairs s p p 3 1 0.05 0.7 0 p 12 p 0
forward_w s p p 1 0 -1 0.05 0.7 0 p 24 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.all_gather_into_tensor
forward_save s p 0.05 0.7 0 p 0 p 0
wait all_gather_into_tensor
forward_rect_save s p p 0 1 1 0.05 0.7 0 p 12 p p 0
forward_rect_save s p p 1 1 0 0.05 0.7 0 p 24 0 p 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 0 1 0 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 0 1 0.05 0.7 p p p p 0 p 1 0
backward_rect_saved s p p 1 1 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.all_gather_into_tensor
forward_w s p p 1 3 -1 0.05 0.7 0 p 0 0
wait all_gather_into_tensor
forward_pairs s p p 0 1 0.05 0.7 0 p 12 p 0
forward_w s p p 1 1 -1 0.05 0.7 0 p 24 0
dist.all_to_all_single
forward_add s p 36 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
""",
    ],
    "bf16_w5": [
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 1 2 1 0.05 0.7 0 p 16 p p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 1 2 0 0.05 0.7 p p p p 0 p 0
backward_rect_saved_t s p p 1 2 1 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 1 2 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 0 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 1 2 0.05 0.7 0 p 16 p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 2 2 1 0.05 0.7 0 p 16 p p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 2 2 0 0.05 0.7 p p p p 0 p 0
backward_rect_saved_t s p p 2 2 1 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 2 2 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 1 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 2 2 0.05 0.7 0 p 16 p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 3 2 1 0.05 0.7 0 p 16 p p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 3 2 0 0.05 0.7 p p p p 0 p 0
backward_rect_saved_t s p p 3 2 1 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 3 2 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 2 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 3 2 0.05 0.7 0 p 16 p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 4 2 1 0.05 0.7 0 p 16 p p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 4 2 0 0.05 0.7 p p p p 0 p 0
backward_rect_saved_t s p p 4 2 1 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 4 2 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 3 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 4 2 0.05 0.7 0 p 16 p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 0 2 1 0.05 0.7 0 p 16 p p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved_t s p p 0 2 0 0.05 0.7 p p p p 0 p 0
backward_rect_saved_t s p p 0 2 1 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved s p p 0 2 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 4 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 0 2 0.05 0.7 0 p 16 p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
wait batch_isend_irecv
""",
    ],
    "bf16_w3_recompute": [
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 1 1 1 0.05 0.7 0 p 8 p p 0
dist.all_to_all_single
forward_add s p 16 p 0
forward_finish_w s p 24 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved s p p 1 1 0.05 0.7 p p p p 0 p 1 0
wait batch_isend_irecv
wait batch_isend_irecv
backward_ranks s p p 2 1 0.05 0.7 p p p p 0 p 1 0
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 0 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 1 1 0.05 0.7 0 p 8 p 0
dist.all_to_all_single
forward_add s p 16 p 0
forward_finish_w s p 24 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 2 1 1 0.05 0.7 0 p 8 p p 0
dist.all_to_all_single
forward_add s p 16 p 0
forward_finish_w s p 24 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved s p p 2 1 0.05 0.7 p p p p 0 p 1 0
wait batch_isend_irecv
wait batch_isend_irecv
backward_ranks s p p 0 1 0.05 0.7 p p p p 0 p 1 0
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 1 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 2 1 0.05 0.7 0 p 8 p 0
dist.all_to_all_single
forward_add s p 16 p 0
forward_finish_w s p 24 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 0 1 1 0.05 0.7 0 p 8 p p 0
dist.all_to_all_single
forward_add s p 16 p 0
forward_finish_w s p 24 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_rect_saved s p p 0 1 0.05 0.7 p p p p 0 p 1 0
wait batch_isend_irecv
wait batch_isend_irecv
backward_ranks s p p 1 1 0.05 0.7 p p p p 0 p 1 0
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 2 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 0 1 0.05 0.7 0 p 8 p 0
dist.all_to_all_single
forward_add s p 16 p 0
forward_finish_w s p 24 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
""",
    ],
    "bf16_w3_nopairs": [
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.all_gather_into_tensor
forward_save s p 0.05 0.7 0 p 0 p 0
wait all_gather_into_tensor
forward_w s p p 3 0 0 0.05 0.7 0 p 8 0
forward_finish_w s p 16 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_w s p p 3 0 0 0.05 0.7 p p p p 0 p 1 0
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.all_gather_into_tensor
forward_w s p p 1 0 -1 0.05 0.7 0 p 0 0
wait all_gather_into_tensor
forward_w s p p 3 0 0 0.05 0.7 0 p 8 0
forward_finish_w s p 16 p 0.05 0.7 0 p p p p 0
dist.all_reduce
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.all_gather_into_tensor
forward_save s p 0.05 0.7 0 p 0 p 0
wait all_gather_into_tensor
forward_w s p p 3 0 1 0.05 0.7 0 p 8 0
forward_finish_w s p 16 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_w s p p 3 0 1 0.05 0.7 p p p p 0 p 1 0
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.all_gather_into_tensor
forward_w s p p 1 1 -1 0.05 0.7 0 p 0 0
wait all_gather_into_tensor
forward_w s p p 3 0 1 0.05 0.7 0 p 8 0
forward_finish_w s p 16 p 0.05 0.7 0 p p p p 0
dist.all_reduce
""",
        """
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.all_gather_into_tensor
forward_save s p 0.05 0.7 0 p 0 p 0
wait all_gather_into_tensor
forward_w s p p 3 0 2 0.05 0.7 0 p 8 0
forward_finish_w s p 16 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
backward_w s p p 3 0 2 0.05 0.7 p p p p 0 p 1 0
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.all_gather_into_tensor
forward_w s p p 1 2 -1 0.05 0.7 0 p 0 0
wait all_gather_into_tensor
forward_w s p p 3 0 2 0.05 0.7 0 p 8 0
forward_finish_w s p 16 p 0.05 0.7 0 p p p p 0
dist.all_reduce
""",
    ],
    "bf16_w3_xf": [
        """
dist.all_reduce
normalize_xf s p p 16 16 0 p p p p 0
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 1 1 1 0.05 0.7 0 p 16 p p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved_xfp s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
pack_xf_from_packed s p 1 p 0
backward_rect_saved_t_xfp s p p 1 1 0 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved_xfp s p p 1 1 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 0 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 1 1 0.05 0.7 0 p 16 p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
""",
        """
dist.all_reduce
normalize_xf s p p 16 16 0 p p p p 0
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 2 1 1 0.05 0.7 0 p 16 p p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved_xfp s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
pack_xf_from_packed s p 1 p 0
backward_rect_saved_t_xfp s p p 2 1 0 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved_xfp s p p 2 1 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 1 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 2 1 0.05 0.7 0 p 16 p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
""",
        """
dist.all_reduce
normalize_xf s p p 16 16 0 p p p p 0
dist.batch_isend_irecv
forward_save s p 0.05 0.7 0 p 0 p 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_rect_save s p p 0 1 1 0.05 0.7 0 p 16 p p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_gather_into_tensor
dist.all_reduce
backward_saved_xfp s p p 0.05 0.7 p p 0 p 0 0
wait all_gather_into_tensor
pack_xf_from_packed s p 1 p 0
backward_rect_saved_t_xfp s p p 0 1 0 0.05 0.7 p p p p 0 p 0
dist.all_to_all_single
backward_rect_saved_xfp s p p 0 1 0.05 0.7 p p p p 0 p 1 0
wait all_to_all_single
backward_finish_p s p p p 16 16 0 p 0.05 0 p p p 16 16 0 0
-- forward under no_grad --
dist.all_reduce
normalize s p p 16 16 0 p p p 0
dist.batch_isend_irecv
dist.batch_isend_irecv
forward_w s p p 1 2 -1 0.05 0.7 0 p 0 0
wait batch_isend_irecv
wait batch_isend_irecv
forward_pairs s p p 0 1 0.05 0.7 0 p 16 p 0
dist.all_to_all_single
forward_add s p 32 p 0
forward_finish_w s p 48 p 0.05 0.7 0 p p p p 0
dist.all_reduce
wait batch_isend_irecv
wait batch_isend_irecv
""",
    ],
    "projection": [
        """
project_pack_wf s p p 48 48 48 48 0 p p 64 64 p p p p p 0
forward_save s p 0.05 0.7 0 p 0 p 0
forward_finish_w s p 4 p 0.05 0.7 0 p p p p 0
backward_saved s p p 0.05 0.7 p p 0 p 0 0
backward_finish_p s p p p 128 128 2 p 0.05 0 p p p 32 32 2 0
project_dw 40 32 p p 32 p p 48 48 48 48 0 p p p 48 48 p p 0
-- forward under no_grad --
project_pack_wf s p p 48 48 48 48 0 p p 64 64 p p p p p 0
forward_w s p p 1 0 -1 0.05 0.7 0 p 0 0
forward_finish_w s p 4 p 0.05 0.7 0 p p p p 0
""",
    ],
}

if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    print("EXPECTED = {")
    for name in CONFIGS:
        print(f'    "{name}": [')
        for log, _ in run(name):
            print('        """\n' + log + '\n""",')
        print("    ],")
    print("}")
