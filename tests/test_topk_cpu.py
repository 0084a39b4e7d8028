"""CPU tests of retrieval_topk (fused similarity + top-k over two independent sets): the REAL kernel sources (lane-level emulation)
against the float64 dense definition torch.topk(q_hat @ g_hat^T, k), written out below.

Conditions checked for every row i (the float64 definition satisfies them trivially, so no case is exempt), tol = 1e-5 max|S| for fp32
products (the bar of test_ranking_cpu.py) and 2e-2 max|S| for bf16 operands (the project's bf16 score bar):
  (a) scores non-increasing, indices in [0, Ng) and distinct
  (b) |scores[i, r] - S64[i, indices[i, r]]| <= tol
  (c) |scores[i, r] - ref_scores[i, r]| <= tol
  (d) every j with S64[i, j] > ref_scores[i, k - 1] + 2 tol is among indices[i]"""
import pytest
import torch

import crossclr_amd
from crossclr_amd import _native as nat
from crossclr_amd import ranking
from oracle import crossclr_oracle as orc


@pytest.fixture(scope="module")
def emulated_library():
    from emu import build_emu
    nat.use_library_for_testing(build_emu.build())
    yield
    nat.use_library_for_testing(None)


def dense_definition(q, g, k, normalize):
    qd, gd = q.double(), g.double()
    if normalize:
        qd = qd / qd.norm(dim=1, keepdim=True).clamp_min(1e-12)
        gd = gd / gd.norm(dim=1, keepdim=True).clamp_min(1e-12)
    S = qd @ gd.t()
    return S, torch.topk(S, k, dim=1).values


def check_conditions(scores, indices, S, ref_scores, rel_tol):
    nq, ng = S.shape
    k = ref_scores.shape[1]
    tol = rel_tol * float(S.abs().max())
    assert scores.shape == (nq, k) and indices.shape == (nq, k)
    assert scores.dtype == torch.float32 and indices.dtype == torch.int64
    s = scores.double()
    assert (s[:, :-1] >= s[:, 1:]).all(), "(a) scores must be non-increasing"
    assert ((indices >= 0) & (indices < ng)).all(), "(a) indices must lie in [0, Ng)"
    srt = indices.sort(dim=1).values
    assert (srt[:, :-1] != srt[:, 1:]).all(), "(a) indices must be distinct"
    err_b = (s - S.gather(1, indices)).abs().max().item()
    err_c = (s - ref_scores).abs().max().item()
    print(f"tol {tol:.3e}  (b) {err_b:.3e}  (c) {err_c:.3e}")
    assert err_b <= tol, "(b)"
    assert err_c <= tol, "(c)"
    must = S > ref_scores[:, -1:] + 2 * tol
    present = torch.zeros(nq, ng, dtype=torch.bool)
    present.scatter_(1, indices, True)
    assert (~must | present).all(), "(d) a candidate clearly above the k-th best is missing"


def make_sets(nq, ng, D, seed):
    q = orc.make_inputs("cluster", nq, D, seed)[0]
    g = orc.make_inputs("cluster", ng, D, seed)[1]      # the same 16 centres: many near-ties
    return q, g + 0.05 * torch.randn(ng, D, generator=torch.Generator().manual_seed(seed + 1))


SHAPES = [(8, 8, 16), (70, 200, 48), (130, 300, 24), (5, 260, 40)]


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("k", [1, 5, 10, 64])
@pytest.mark.parametrize("nq,ng,D", SHAPES)
def test_emulated_topk_matches_the_dense_definition(emulated_library, nq, ng, D, k, normalize):
    if k > ng:
        with pytest.raises(ValueError):      # (k <= Ng is part of the interface: the rest of the grid covers the values)
            crossclr_amd.retrieval_topk(torch.zeros(nq, D), torch.zeros(ng, D), k)
        return
    q, g = make_sets(nq, ng, D, 9)
    scores, indices = crossclr_amd.retrieval_topk(q, g, k, normalize=normalize, compute_mode="fp32")
    S, ref = dense_definition(q, g, k, normalize)
    check_conditions(scores, indices, S, ref, 1e-5)


@pytest.mark.parametrize("k", [5, 64])
def test_emulated_topk_bf16(emulated_library, k):
    q, g = make_sets(70, 200, 48, 4)
    scores, indices = crossclr_amd.retrieval_topk(q, g, k, compute_mode="bf16")
    S, ref = dense_definition(q, g, k, True)
    check_conditions(scores, indices, S, ref, 2e-2)
    # operands that are exact in bf16, used as given: the products are exact, only the fp32 accumulation is left
    qr, gr = q.bfloat16().float(), g.bfloat16().float()
    scores, indices = crossclr_amd.retrieval_topk(qr, gr, k, normalize=False, compute_mode="bf16")
    S, ref = dense_definition(qr, gr, k, False)
    check_conditions(scores, indices, S, ref, 1e-5)


def test_emulated_topk_bf16x3_is_fp32_accurate(emulated_library):
    q, g = make_sets(70, 200, 48, 5)
    scores, indices = crossclr_amd.retrieval_topk(q, g, 10, compute_mode="bf16x3")
    S, ref = dense_definition(q, g, 10, True)
    check_conditions(scores, indices, S, ref, 1e-5)


def test_duplicate_gallery_rows_come_lower_index_first(emulated_library):
    q, g = make_sets(40, 200, 32, 6)
    g[77] = g[3]
    g[150] = g[3]
    q[:8] = g[3] + 0.01 * torch.randn(8, 32, generator=torch.Generator().manual_seed(1))     # queries whose best match is the triplet
    for mode in ("fp32", "bf16"):
        scores, indices = crossclr_amd.retrieval_topk(q, g, 10, compute_mode=mode)
        S, ref = dense_definition(q, g, 10, True)
        check_conditions(scores, indices, S, ref, 1e-5 if mode == "fp32" else 2e-2)
        seen = 0
        for i in range(q.shape[0]):
            row = indices[i].tolist()
            if 3 not in row:
                assert 77 not in row and 150 not in row      # equal scores: the lowest index is never the one left out
                continue
            r = row.index(3)
            if r + 2 < len(row):
                assert row[r:r + 3] == [3, 77, 150], (i, row)
                assert scores[i, r] == scores[i, r + 1] == scores[i, r + 2]
                seen += 1
        assert seen >= 8
        # ties everywhere: with all-equal rows every score of a query is the same, so the answer is 0 .. k - 1 in order
        flat = g[3:4].repeat(200, 1)
        _, ind = crossclr_amd.retrieval_topk(q, flat, 10, compute_mode=mode)
        assert torch.equal(ind, torch.arange(10).repeat(q.shape[0], 1))


@pytest.mark.parametrize("k", [1, 10, 64])
def test_all_negative_scores_with_a_ragged_gallery(emulated_library, k):
    """Padding rows of the packed gallery are zeros and score 0 -- above every real score here: they must be masked by index."""
    gen = torch.Generator().manual_seed(3)
    q = torch.rand(70, 24, generator=gen) + 0.2               # rows in the positive orthant: every product with -q is negative
    g = -q[torch.randint(0, 70, (200,), generator=gen)] + 0.05 * torch.randn(200, 24, generator=gen)
    S, ref = dense_definition(q, g, k, True)
    assert float(S.max()) < 0.0
    scores, indices = crossclr_amd.retrieval_topk(q, g, k)
    assert int(indices.max()) < 200 and float(scores.max()) < 0.0
    check_conditions(scores, indices, S, ref, 1e-5)


def test_identical_sets_retrieve_themselves(emulated_library):
    x = torch.randn(130, 40, generator=torch.Generator().manual_seed(12))
    scores, indices = crossclr_amd.retrieval_topk(x, x.clone(), 5)
    assert torch.equal(indices[:, 0], torch.arange(130))
    assert (scores[:, 0] - 1.0).abs().max().item() <= 1e-6


def test_two_calls_and_every_split_count_give_the_same_bits(emulated_library):
    q, g = make_sets(70, 520, 32, 8)          # 5 gallery tiles
    s0, i0 = crossclr_amd.retrieval_topk(q, g, 10)
    s1, i1 = crossclr_amd.retrieval_topk(q, g, 10)
    assert torch.equal(s0, s1) and torch.equal(i0, i1)
    lib = nat.library()
    assert lib.crossclr_topk_splits(70, 520, 10, 0) == 5
    for splits in (1, 2, 3):
        assert lib.crossclr_topk_splits(70, 520, 10, splits) == splits
        s2, i2 = ranking._topk(q, g, 10, True, "fp32", splits=splits)
        assert torch.equal(s0, s2) and torch.equal(i0, i2), splits


def test_errors(emulated_library):
    q, g = torch.randn(6, 16), torch.randn(20, 16)
    limit = nat.library().crossclr_topk_max_k()
    assert limit >= 64
    with pytest.raises(ValueError):
        crossclr_amd.retrieval_topk(q, g, 0)
    with pytest.raises(ValueError):
        crossclr_amd.retrieval_topk(q, g, 21)
    with pytest.raises(ValueError, match="limit"):
        crossclr_amd.retrieval_topk(q, torch.randn(limit + 10, 16), limit + 1)
    with pytest.raises(RuntimeError):
        crossclr_amd.retrieval_topk(q, torch.randn(20, 17), 3)
    with pytest.raises(RuntimeError):
        crossclr_amd.retrieval_topk(q, torch.randn(0, 16), 1)
    with pytest.raises(RuntimeError):
        crossclr_amd.retrieval_topk(torch.randn(0, 16), g, 1)
    with pytest.raises(ValueError):
        crossclr_amd.retrieval_topk(q, g, 3, compute_mode="fp8")
    # the library refuses the same arguments itself, with its usual text
    lib = nat.library()
    assert lib.crossclr_topk_workspace_bytes(6, 20, 21, 0) == 0 and lib.crossclr_topk_workspace_bytes(6, 200, limit + 1, 0) == 0
    assert lib.crossclr_topk_splits(6, 20, 0, 0) < 0 and b"k must be at least 1" in lib.crossclr_last_error()
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    assert lib.crossclr_topk_select(buf.data_ptr(), buf.data_ptr(), 6, 20, 16, 0, 3, 0, buf.data_ptr(), 8, 0) == -4     # CROSSCLR_E_WORKSPACE
    assert lib.crossclr_topk_select(buf.data_ptr(), buf.data_ptr(), 6, 20, 16, 7, 3, 0, buf.data_ptr(), buf.numel(), 0) == -1
    assert b"bad mode" in lib.crossclr_last_error()


def test_new_symbols_are_bound_and_the_abi_version_is_unchanged(emulated_library):
    lib = nat.library()
    for sym in ("crossclr_topk_max_k", "crossclr_topk_operand_bytes", "crossclr_topk_pack", "crossclr_topk_splits",
                "crossclr_topk_workspace_bytes", "crossclr_topk_select", "crossclr_topk_merge"):
        assert sym in nat.EXPORTED_SYMBOLS and getattr(lib, sym).argtypes is not None
    assert lib.crossclr_abi_version() == 8 == nat.ABI_VERSION
    assert lib.crossclr_topk_operand_bytes(130, 70, nat.MODE_FP32) == 256 * 128 * 4
    assert lib.crossclr_topk_operand_bytes(130, 70, nat.MODE_BF16) == 256 * 128 * 2
    assert crossclr_amd.retrieval_topk is ranking.retrieval_topk and "retrieval_topk" in crossclr_amd.__all__
