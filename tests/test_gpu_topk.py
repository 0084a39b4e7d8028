"""MI355X tests of retrieval_topk (fused similarity + top-k over two independent sets) against the float64 dense definition
torch.topk(q_hat @ g_hat^T, k) computed on the CPU.

Conditions for every row i, tol = 1e-5 max|S| for fp32 products and 2e-2 max|S| for bf16 operands (the bars of test_gpu_ranking.py):
  (a) scores non-increasing, indices in [0, Ng) and distinct
  (b) |scores[i, r] - S64[i, indices[i, r]]| <= tol
  (c) |scores[i, r] - ref_scores[i, r]| <= tol
  (d) every j with S64[i, j] > ref_scores[i, k - 1] + 2 tol is among indices[i]"""
import pytest
import torch

import crossclr_amd
from crossclr_amd import _native as nat
from oracle import crossclr_oracle as orc

pytestmark = pytest.mark.gpu
REL_TOL = {"fp32": 1e-5, "bf16": 2e-2}


def dense_definition(q, g, k, normalize=True):
    qd, gd = q.double(), g.double()
    if normalize:
        qd = qd / qd.norm(dim=1, keepdim=True).clamp_min(1e-12)
        gd = gd / gd.norm(dim=1, keepdim=True).clamp_min(1e-12)
    S = qd @ gd.t()
    return S, torch.topk(S, k, dim=1).values


def check_conditions(scores, indices, S, ref_scores, rel_tol):
    assert scores.is_cuda and indices.is_cuda and scores.dtype == torch.float32 and indices.dtype == torch.int64
    scores, indices = scores.cpu(), indices.cpu()
    nq, ng = S.shape
    k = ref_scores.shape[1]
    tol = rel_tol * float(S.abs().max())
    assert scores.shape == (nq, k) and indices.shape == (nq, k)
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
    g = orc.make_inputs("cluster", ng, D, seed)[1]      # the same 16 centres: near-ties exist
    return q, g + 0.3 * torch.randn(ng, D, generator=torch.Generator().manual_seed(seed + 1))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("nq,ng,D,k", [(8192, 8192, 512, 10), (1000, 20000, 512, 10), (130, 4099, 72, 64), (4096, 4096, 1024, 5)])
def test_topk_matches_the_dense_definition(nq, ng, D, k, mode):
    assert nat.backend() == "hip-gfx950"
    q, g = make_sets(nq, ng, D, 21)
    scores, indices = crossclr_amd.retrieval_topk(q.cuda(), g.cuda(), k, compute_mode=mode)
    S, ref = dense_definition(q, g, k)
    check_conditions(scores, indices, S, ref, REL_TOL[mode])


def test_rows_as_given_and_bf16x3():
    q, g = make_sets(300, 3000, 200, 5)
    S, ref = dense_definition(q, g, 20, normalize=False)
    scores, indices = crossclr_amd.retrieval_topk(q.cuda(), g.cuda(), 20, normalize=False)
    check_conditions(scores, indices, S, ref, 1e-5)
    S, ref = dense_definition(q, g, 20)
    scores, indices = crossclr_amd.retrieval_topk(q.cuda(), g.cuda(), 20, compute_mode="bf16x3")
    check_conditions(scores, indices, S, ref, 1e-5)


@pytest.mark.parametrize("nq,ng,D,k", [(1000, 20000, 512, 10), (130, 4099, 72, 64), (2048, 8192, 256, 16)])
def test_bf16_selection_is_exact_on_operands_that_bf16_holds_exactly(nq, ng, D, k):
    """The 2e-2 bar of the bf16 cases above is wide on clustered data.  Rows already rounded to bf16 and used as given have exact
    operands and exact products; only the fp32 accumulation is left, so the fp32 tolerance applies and a wrong selection shows."""
    q, g = make_sets(nq, ng, D, 31)
    q, g = q.bfloat16().float(), g.bfloat16().float()
    scores, indices = crossclr_amd.retrieval_topk(q.cuda(), g.cuda(), k, normalize=False, compute_mode="bf16")
    S, ref = dense_definition(q, g, k, normalize=False)
    check_conditions(scores, indices, S, ref, 1e-5)


@pytest.mark.parametrize("case", ["strided", "fp16", "bf16"])
def test_input_dtypes_and_strided_rows(case):
    q, g = make_sets(500, 2100, 80, 7)
    if case == "strided":
        wide = torch.zeros(2100, 160, device="cuda")
        wide[:, :80] = g.cuda()
        qd, gd = q.cuda(), wide[:, :80]          # row stride 160
        assert gd.stride(0) == 160
    else:
        dt = torch.float16 if case == "fp16" else torch.bfloat16
        q, g = q.to(dt), g.to(dt)                # the definition is taken on the rows the kernels are given
        qd, gd = q.cuda(), g.cuda()
    scores, indices = crossclr_amd.retrieval_topk(qd, gd, 10)
    S, ref = dense_definition(q, g, 10)
    check_conditions(scores, indices, S, ref, 1e-5)


def test_duplicate_gallery_rows_and_determinism():
    q, g = make_sets(2000, 9000, 256, 11)
    g[4077] = g[3]
    g[8150] = g[3]
    q[:64] = g[3] + 0.01 * torch.randn(64, 256, generator=torch.Generator().manual_seed(1))
    qd, gd = q.cuda(), g.cuda()
    for mode in ("fp32", "bf16"):
        s0, i0 = crossclr_amd.retrieval_topk(qd, gd, 10, compute_mode=mode)
        s1, i1 = crossclr_amd.retrieval_topk(qd, gd, 10, compute_mode=mode)
        assert torch.equal(s0, s1) and torch.equal(i0, i1)
        for splits in (1, 3):      # the result does not depend on how the gallery is cut
            s2, i2 = crossclr_amd.ranking._topk(qd, gd, 10, True, mode, splits=splits)
            assert torch.equal(s0, s2) and torch.equal(i0, i2), splits
        assert torch.equal(i0[:64, :3].cpu(), torch.tensor([3, 4077, 8150]).repeat(64, 1))
        assert torch.equal(s0[:64, 0], s0[:64, 1]) and torch.equal(s0[:64, 0], s0[:64, 2])


def test_all_negative_scores_with_a_ragged_gallery():
    gen = torch.Generator().manual_seed(3)
    q = torch.rand(700, 96, generator=gen) + 0.2
    g = -q[torch.randint(0, 700, (4099,), generator=gen)] + 0.05 * torch.randn(4099, 96, generator=gen)
    S, ref = dense_definition(q, g, 64)
    assert float(S.max()) < 0.0
    scores, indices = crossclr_amd.retrieval_topk(q.cuda(), g.cuda(), 64)
    assert int(indices.max()) < 4099 and float(scores.max()) < 0.0
    check_conditions(scores, indices, S, ref, 1e-5)


def test_peak_memory_stays_far_below_the_dense_matrix():
    """Nq = 4096, Ng = 32768: the dense fp32 score matrix would be 512 MiB; the packed operands are ~38 MB."""
    nq, ng, D, k = 4096, 32768, 256, 10
    gen = torch.Generator().manual_seed(5)
    q, g = torch.randn(nq, D, generator=gen).cuda(), torch.randn(ng, D, generator=gen).cuda()
    crossclr_amd.retrieval_topk(q[:256], g[:256], k)          # library loaded, context warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    scores, indices = crossclr_amd.retrieval_topk(q, g, k)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"peak extra memory {extra / 2**20:.1f} MiB")
    assert extra < 128 * 2**20
    assert scores.shape == (nq, k) and indices.shape == (nq, k) and int(indices.max()) < ng


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_recall_agrees_with_retrieval_ranks_on_a_paired_set(mode):
    """The partner is among the 10 best exactly when fewer than 10 candidates beat it.  retrieval_ranks counts them (v2t_ranks); per row
    only candidates within rounding of the partner's score may be counted differently -- near[i] of them, the per-row allowance of
    test_retrieval_ranks_match_the_dense_definition -- so hit[i] is decided wherever v2t_ranks[i] is at least near[i] away from 10."""
    B, D = 4096, 512
    v, t = orc.make_inputs("cluster", B, D, 21)
    t = t + 0.3 * torch.randn(B, D, generator=torch.Generator().manual_seed(2))
    vd, td = v.cuda(), t.cuda()
    _, indices = crossclr_amd.retrieval_topk(vd, td, 10, compute_mode=mode)
    hit = (indices[:, :10] == torch.arange(B, device="cuda")[:, None]).any(1).cpu()
    got = crossclr_amd.retrieval_ranks(vd, td, compute_mode=mode)
    ranks = got["v2t_ranks"].cpu()
    S, _ = dense_definition(v, t, 1)
    tol = REL_TOL[mode] * float(S.abs().max())
    near = ((S - S.diag()[:, None]).abs() < tol).sum(1) - 1
    must_hit, must_miss = ranks + near < 10, ranks - near >= 10
    band = ~(must_hit | must_miss)
    r10_topk, r10_ranks = hit.double().mean().item(), float(got["v2t"][2])
    print(f"R@10 from top-k {r10_topk:.6f}, from retrieval_ranks {r10_ranks:.6f}; rows decided {int((~band).sum())} of {B}, "
          f"rows where hit != (rank < 10): {int((hit != (ranks < 10)).sum())}")
    assert hit[must_hit].all() and not hit[must_miss].any()
    # Both paths normalise with the same arithmetic and form every score with the same MFMA sequence, so the scores are the same bits and the
    # two answers can differ only where a candidate ties the partner's score exactly: none on these seeded inputs.  (This is what decides
    # the bf16 case, whose tolerance band above covers every row.)
    assert torch.equal(hit, ranks < 10)
    assert abs(r10_topk - r10_ranks) <= band.double().mean().item()
