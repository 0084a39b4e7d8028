"""CPU tests of pair_ids on the InfoNCE and the sigmoid loss (same-item pairs are excluded from the negatives): the REAL kernel sources
(lane-level emulation) against the dense float64 definitions of tests/pair_ids_cases.py, at the bars of tests/infonce_cases.py and
tests/sigmoid_cases.py.  grad_out = 3 throughout.

  1  against the definition: runs3 and stride7 over the random cases, all three modes, both losses
  2  distinct / low32 ids give the bits of pair_ids=None;  3  the labelling does not matter;  4  the ids do
  5  all ids equal;  6  excluded entries that dominate their row and column (an unmasked exp2 overflows)
  7  split counts;  8  the interface and the modules"""
import pytest
import torch

import infonce_cases as ic
import pair_ids_cases as pc
from crossclr_amd import _native as nat

DEV = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    from emu import build_emu
    nat.use_library_for_testing(build_emu.build())
    yield
    nat.use_library_for_testing(None)


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("pattern", ("runs3", "stride7"))
@pytest.mark.parametrize("B,D,seed", pc.RANDOM_CASES)
def test_infonce_against_the_definition(B, D, seed, pattern, mode):
    pc.check_infonce_case(B, D, seed, ic.SCALES[0], mode, pattern, DEV)


@pytest.mark.parametrize("mode", ("fp32", "bf16x3"))
@pytest.mark.parametrize("pattern", ("runs3", "stride7"))
@pytest.mark.parametrize("B,D,seed", [(257, 72, 2), (300, 40, 5)])
def test_infonce_against_the_definition_at_scale_100(B, D, seed, pattern, mode):
    pc.check_infonce_case(B, D, seed, 100.0, mode, pattern, DEV)


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("s,beta", [(10.0, -10.0), (100.0, -10.0)])
@pytest.mark.parametrize("pattern", ("runs3", "stride7"))
@pytest.mark.parametrize("B,D,seed", pc.RANDOM_CASES)
def test_sigmoid_against_the_definition(B, D, seed, pattern, s, beta, mode):
    pc.check_sigmoid_case(B, D, seed, s, beta, mode, pattern, DEV)


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("B,D", [(70, 48), (257, 72)])
def test_distinct_ids_give_the_bits_of_none(B, D, mode):
    pc.check_distinct_ids_give_the_bits_of_none(B, D, mode, DEV)


@pytest.mark.parametrize("pattern", ("runs3", "stride7"))
def test_labelling_does_not_matter(pattern):
    pc.check_labelling_does_not_matter(pattern, DEV)


def test_the_ids_matter():
    pc.check_the_ids_matter(DEV)


@pytest.mark.parametrize("mode", ("fp32", "bf16x3"))
@pytest.mark.parametrize("B,D", [(8, 16), (300, 40)])
def test_all_ids_equal(B, D, mode):
    pc.check_equal_ids(B, D, mode, DEV)


@pytest.mark.parametrize("B,D", pc.SHAPES)
def test_dominant_excluded_entries(B, D):
    pc.check_dominant_excluded_entries(B, D, DEV)


def test_split_counts():
    pc.check_splits(DEV)


def test_the_interface():
    pc.check_interface(DEV)


def test_a_module_step():
    pc.check_module_step(DEV)


def test_new_symbols_are_bound_and_the_abi_version_is_unchanged():
    lib = nat.library()
    for sym in ("crossclr_pair_groups", "crossclr_infonce_stats_ids", "crossclr_infonce_backward_ids", "crossclr_sigmoid_stats_ids",
                "crossclr_sigmoid_backward_ids"):
        assert sym in nat.EXPORTED_SYMBOLS and getattr(lib, sym).argtypes is not None
    assert lib.crossclr_abi_version() == 8 == nat.ABI_VERSION
    plan = nat.make_plan(130, 200, 1, 0, nat.MODE_FP32)
    ids = torch.tensor([5, -1, 5, 2 ** 40, -1, 2 ** 40 + 2 ** 32] + list(range(100, 224)), dtype=torch.int64)
    group = torch.full((plan.bpad,), -7, dtype=torch.int32)
    assert lib.crossclr_pair_groups(plan, ids.data_ptr(), group.data_ptr(), 0) == 0
    want = torch.arange(plan.bpad, dtype=torch.int32)
    want[2], want[4] = 0, 1      # (entries 3 and 5 agree in their low words only)
    assert torch.equal(group, want)
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    need = lib.crossclr_infonce_workspace_bytes(plan, 0)
    assert lib.crossclr_pair_groups(plan, 0, group.data_ptr(), 0) == -1 and b"NULL" in lib.crossclr_last_error()      # CROSSCLR_E_ARG
    assert lib.crossclr_infonce_stats_ids(plan, buf.data_ptr(), buf.data_ptr(), 0, 0, buf.data_ptr(), need, 0) == -1
    assert b"group is NULL" in lib.crossclr_last_error()
    assert lib.crossclr_infonce_stats_ids(plan, buf.data_ptr(), buf.data_ptr(), group.data_ptr(), 0, buf.data_ptr(), need - 1, 0) == -4
    assert lib.crossclr_sigmoid_backward_ids(plan, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 0, buf.data_ptr(), 0) == -1
    sharded = nat.make_plan(130, 200, 2, 0, nat.MODE_FP32)
    for rc in (lib.crossclr_pair_groups(sharded, ids.data_ptr(), group.data_ptr(), 0),
               lib.crossclr_infonce_backward_ids(sharded, *[buf.data_ptr()] * 6, 0),
               lib.crossclr_sigmoid_stats_ids(sharded, *[buf.data_ptr()] * 4, 0, buf.data_ptr(), need, 0)):
        assert rc == -1 and b"single-device" in lib.crossclr_last_error()
