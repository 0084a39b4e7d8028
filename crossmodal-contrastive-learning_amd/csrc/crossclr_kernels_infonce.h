// crossclr_kernels_infonce.h -- the symmetric InfoNCE (CLIP) loss with a logit scale read from device memory (crossclr_infonce_* of
// include/crossclr.h):  L = 1/2 [ CE(s S, diag) + CE(s S^T, diag) ],  S = v^ . t^T, on the tiled-similarity skeleton.  Neither s S, the two
// soft-max outputs nor their gradients are materialised.
//
//   infonce_stats_kernel            grid (video row blocks, column splits): online soft-max of every row over the split's columns and of
//                                   every column over the block's rows, as (max, sum relative to that max, less one) pairs, and S[i][i]
//   infonce_finish_kernel           merges the partials in a fixed order -> lse[2][2][bpad] (log2 domain, hi and lo) and the loss
//   infonce_backward_kernel         the three-phase gradient product on the stacked rows against the tiles of the other modality:
//                                   W = P_row + P_col - 2 [positive pair], G = W . x^
//   pairloss_backward_finish_kernel (crossclr_kernels_pairloss.h) with g = s / (2 B) M_p
//
// LOG2 DOMAIN: every logit is x = c S with c = s log2(e), ONE fp32 product of the device scalar and the accumulator, formed by the same
// expression in every kernel of this file: the statistics, the loss and the weights see the same bits.  Any finite s (0 and negative
// values included): all maxima are maxima of x, not of S.
#pragma once
#include <type_traits>

#include "crossclr_kernels_generic.h"
#include "crossclr_kernels_pairids.h"
#include "crossclr_kernels_pairloss.h"

namespace crossclr {

constexpr float kInfonceMasked = -3.0e38f;      // "no entry" in a slot's maximum: below every logit, finite (differences stay numbers)

// The logit of a score: ONE rounded fp32 product.  The statistics compare logits for equality and the backward subtracts the row's
// log-sum-exp from the logit it forms anew: contracted into a neighbouring subtraction (an fma sees the unrounded product) the two
// kernels would disagree by the product's rounding -- 4e-6 at a logit of 65, 2 % of a saturated soft-max's 1 - P.
__device__ __forceinline__ float infonce_logit(float c, float score) {
#pragma clang fp contract(off)
    return c * score;
}

// A slot's soft-max statistics are a pair (m, u): m = the maximum of its logits, u = sum exp2(x - m) - 1 -- the sum WITHOUT the term of
// one entry that attains the maximum, which is exactly 1.  Where a soft-max is saturated (s = 100: the sum is 1 + 1e-4) the gradient is
// made of what lies beyond that 1, and an fp32 sum that carries the 1 keeps it to 6e-8 only, 1e-3 of itself.  An empty slot is
// (kInfonceMasked, -1).
// (m, u) <- the pair of the union of two slots; one exponential.  1 + u + (1 + u2) e - 1 with the larger maximum's pair in front; the
// smaller one's (1 + u2) e as e + u2 e: an empty slot adds e - e = 0 (two empty ones: -1 + 0).
__device__ __forceinline__ void infonce_merge(float& m, float& u, float m2, float u2) {
    const float e = fast_exp2(-fabsf(m - m2));
    const bool keep = m >= m2;
    u = keep ? u + fmaf(u2, e, e) : u2 + fmaf(u, e, e);
    m = keep ? m : m2;
}
// halving_sum16's exchange pattern on (m, u) pairs: every lane ends up with the pair of element halving_elem16(l31) over the 32 lanes
// of its wave half, merged in an order that depends on the lane's position alone.
__device__ __forceinline__ void halving_lse16(const float (&m)[16], const float (&s)[16], int l31, float* out_m, float* out_s) {
    float m8[8], m4[4], m2[2], s8[8], s4[4], s2[2];
    {
        const bool up = (l31 >> 3) & 1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            m8[i] = up ? m[8 + i] : m[i];
            s8[i] = up ? s[8 + i] : s[i];
            infonce_merge(m8[i], s8[i], lane_xor<15>(up ? m[i] : m[8 + i]), lane_xor<15>(up ? s[i] : s[8 + i]));
        }
    }
    {
        const bool up = (l31 >> 2) & 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            m4[i] = up ? m8[4 + i] : m8[i];
            s4[i] = up ? s8[4 + i] : s8[i];
            infonce_merge(m4[i], s4[i], lane_xor<7>(up ? m8[i] : m8[4 + i]), lane_xor<7>(up ? s8[i] : s8[4 + i]));
        }
    }
    {
        const bool up = (l31 >> 1) & 1;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            m2[i] = up ? m4[2 + i] : m4[i];
            s2[i] = up ? s4[2 + i] : s4[i];
            infonce_merge(m2[i], s2[i], lane_xor<2>(up ? m4[i] : m4[2 + i]), lane_xor<2>(up ? s4[i] : s4[2 + i]));
        }
    }
    const bool up = l31 & 1;
    float m1 = up ? m2[1] : m2[0], s1 = up ? s2[1] : s2[0];
    infonce_merge(m1, s1, lane_xor<1>(up ? m2[0] : m2[1]), lane_xor<1>(up ? s2[0] : s2[1]));
    infonce_merge(m1, s1, lane_xor<16>(m1), lane_xor<16>(s1));      // (the merge gives the same bits with its operands exchanged)
    *out_m = m1;
    *out_s = s1;
}

// ---------------------------------------------------------------------------------------------
// Tiled similarity with an online soft-max epilogue in both directions: the main loop of hardneg_select_kernel (128 video rows x 128 text
// rows of the packed operand X[2][bpad][Dpad], K-chunks of 128 bytes, two in flight, MFMA operands swapped: a lane owns video row
// p = l31 of each 32 x 32 fragment and 16 of its columns).  grid = (bpad / 128, nsplit); no atomics; every slot has one writer.
//   Row side: a lane carries the pair (m, u) of its two rows across the tiles -- the tile's maximum first, one rescale of the running
//   pair when the maximum moves, then the tile's exponentials, entries equal to the maximum counted instead of added (each is exactly
//   1; one of them is the term u leaves out); the four lanes (wc, half) of a row meet once, at the end, in LDS -> row_m / row_s
//   [nsplit][bpad].
//   Column side, per tile: a lane's pair of each of its 32 columns over its two rows, halving_lse16 over the 32 lanes of the wave half,
//   the two row waves through LDS -> col_m / col_s [bpad / 128][bpad].
//   The shift of every slot is the TRUE maximum of its entries.  Masking BY INDEX: padding rows and columns (>= b: zeros in the operand,
//   they would add exp2(0 - max)) contribute nothing; the positive pair is a term of both soft-maxes.
//   pair[i] = S[i][i] from the diagonal tile's accumulators.
//   LDS: 2 x 16 KiB operand chunks + 4 KiB of reduction slots.
// ---------------------------------------------------------------------------------------------
//   IDS (pair ids, crossclr_kernels_pairids.h): group [bpad]; an entry (i, j), i != j, with group[i] == group[j] is left out of row i's and
//   of column j's soft-max -- kInfonceMasked in both maxima, no term of either sum, exactly like padding; every tile takes the masked
//   epilogue.  A slot whose entries are all left out is the empty slot.  ONE wave per SIMD for these instantiations: the masks do not fit
//   beside the 254 registers of the plain ones.
template <typename T, bool IDS = false, typename... GROUP>
__global__ void __launch_bounds__(256, IDS ? 1 : 2) infonce_stats_kernel(const T* X, int b, int bpad, int Dpad, int tiles_per_split,
                                                                         const float* logit_scale, float* row_m, float* row_s, float* col_m,
                                                                         float* col_s, float* pair, GROUP... group_arg) {
    typedef Operand<T> Op;
    static_assert(sizeof...(GROUP) == (IDS ? 1 : 0), "IDS instantiations take the group array as their last argument");
    const int* group = group_of(group_arg...);
    CROSSCLR_SHARED __attribute__((aligned(16))) unsigned char lds[2 * 128 * 128];
    CROSSCLR_SHARED float red_m[4 * 128];
    CROSSCLR_SHARED float red_s[4 * 128];
    int* colg = nullptr;      // IDS: the groups of the tile's 128 columns, two tiles' worth (a tile's readers and the next one's writers
    int rg[2] = {0, 0};       // never meet in one half), and of the lane's two rows
    if constexpr (IDS) {
        CROSSCLR_SHARED __attribute__((aligned(16))) int col_groups[2 * 128];
        colg = col_groups;
    }
    unsigned char* tileP = lds;                 // video chunk [128][128 B]
    unsigned char* tileQ = lds + 128 * 128;     // text chunk  [128][128 B]
    float* const redm = red_m;
    float* const reds = red_s;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int wr = wave & 1, wc = wave >> 1;
    const size_t pitch = (size_t)Dpad * sizeof(T);
    const int nchunks = Dpad / Op::kChunkElems;
    const int rb = blockIdx.x, row0 = rb * 128, split = blockIdx.y;
    const int ntiles = bpad / 128;
    const int t_begin = split * tiles_per_split;
    const int t_end = t_begin + tiles_per_split < ntiles ? t_begin + tiles_per_split : ntiles;
    const unsigned char* rbase = reinterpret_cast<const unsigned char*>(X) + (size_t)row0 * pitch;
    const unsigned char* tbase = reinterpret_cast<const unsigned char*>(X) + (size_t)bpad * pitch;
    const bool ragged_rows = row0 + 128 > b;
    const float c = logit_scale[0] * kLog2e;

    float run_m[2] = {kInfonceMasked, kInfonceMasked};
    float run_u[2] = {-1.f, -1.f};
    if constexpr (IDS) {
        rg[0] = group[row0 + 64 * wr + l31];
        rg[1] = group[row0 + 64 * wr + 32 + l31];
    }

    KTileStage<128, 256> sp, sq, sp2, sq2;
    for (int t = t_begin; t < t_end; ++t) {
        const unsigned char* cbase = tbase + (size_t)t * 128 * pitch;
        if constexpr (IDS) {      // read in the epilogue, behind the main loop's barriers
            if (tid < 128) colg[(t & 1) * 128 + tid] = group[t * 128 + tid];
        }
        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][cc][r] = 0.f;

        auto chunk = [&](KTileStage<128, 256>& fp, KTileStage<128, 256>& fq, int kc) {
            fp.commit(tileP, tid);
            fq.commit(tileQ, tid);
            __syncthreads();
            if (kc + 2 < nchunks) {
                fp.fetch(rbase, pitch, (kc + 2) * 128, tid);
                fq.fetch(cbase, pitch, (kc + 2) * 128, tid);
            }
#pragma unroll
            for (int s = 0; s < Op::kSteps; ++s) {
                typename Op::frag a[2], bfr[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    a[x] = Op::load(tileQ, 64 * wc + 32 * x + l31, s, half);
                    bfr[x] = Op::load(tileP, 64 * wr + 32 * x + l31, s, half);
                }
#pragma unroll
                for (int qi = 0; qi < 2; ++qi)
#pragma unroll
                    for (int pi = 0; pi < 2; ++pi) acc[qi][pi] = Op::mma(a[qi], bfr[pi], acc[qi][pi]);
            }
            __syncthreads();
        };
        sp.fetch(rbase, pitch, 0, tid);
        sq.fetch(cbase, pitch, 0, tid);
        if (nchunks > 1) {
            sp2.fetch(rbase, pitch, 128, tid);
            sq2.fetch(cbase, pitch, 128, tid);
        }
        for (int kc = 0; kc < nchunks; kc += 2) {
            chunk(sp, sq, kc);
            if (kc + 1 < nchunks) chunk(sp2, sq2, kc + 1);
        }

        // epilogue.  acc[qi][pi][r] = S[row0 + p_t][col0 + 32 qi + frag_row(r, half)], p_t = 64 wr + 32 pi + l31
        const int col0 = t * 128 + 64 * wc;
        if (t == rb) {      // the positive pairs' scores (block-uniform)
#pragma unroll
            for (int qi = 0; qi < 2; ++qi)
#pragma unroll
                for (int r = 0; r < 16; ++r)
#pragma unroll
                    for (int pi = 0; pi < 2; ++pi) {
                        const int row = row0 + 64 * wr + 32 * pi + l31;
                        if (row == col0 + 32 * qi + frag_row(r, half)) pair[row] = acc[qi][pi][r];
                    }
        }
        auto epilogue = [&](auto masked_c) {
            constexpr bool MASKED = decltype(masked_c)::value;
            const bool row_ok[2] = {row0 + 64 * wr + l31 < b, row0 + 64 * wr + 32 + l31 < b};
            // IDS: an entry of another pair of the row's own item is no entry at all -- out of both maxima and both sums, like padding
            auto same_item = [&](int pi, int qi, int r) {
                if constexpr (IDS) {
                    const int cl = 64 * wc + 32 * qi + frag_row(r, half);
                    return colg[(t & 1) * 128 + cl] == rg[pi] && t * 128 + cl != row0 + 64 * wr + 32 * pi + l31;
                } else {
                    return false;
                }
            };
            // row side, step 1: the tile's maximum of each of the lane's two rows, one rescale of the running sum
            float tm[2] = {kInfonceMasked, kInfonceMasked};
#pragma unroll
            for (int qi = 0; qi < 2; ++qi)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool col_ok = !MASKED || col0 + 32 * qi + frag_row(r, half) < b;
#pragma unroll
                    for (int pi = 0; pi < 2; ++pi) {
                        const float x = infonce_logit(c, acc[qi][pi][r]);
                        bool ok = !MASKED || (col_ok && row_ok[pi]);
                        if constexpr (IDS) ok = ok && !same_item(pi, qi, r);
                        tm[pi] = fmaxf(tm[pi], ok ? x : kInfonceMasked);
                    }
                }
            float ts[2] = {0.f, 0.f}, ties[2] = {0.f, 0.f};      // the tile's terms below the maximum, and how many attain it
#pragma unroll
            for (int pi = 0; pi < 2; ++pi) {
                const float nm = fmaxf(run_m[pi], tm[pi]);
                if (nm > run_m[pi]) {      // the maximum moves into this tile: (1 + u) r, and one of the tile's ties is the new left-out term
                    const float r = fast_exp2(run_m[pi] - nm);
                    run_u[pi] = fmaf(run_u[pi], r, r);
                    ties[pi] = -1.f;
                }
                run_m[pi] = nm;
            }
#pragma unroll
            for (int qi = 0; qi < 2; ++qi) {
                float cm[16], cs[16];      // column side: the lane's pair of each of its 16 columns over its two rows
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool col_ok = !MASKED || col0 + 32 * qi + frag_row(r, half) < b;
                    const float x0 = infonce_logit(c, acc[qi][0][r]), x1 = infonce_logit(c, acc[qi][1][r]);
                    bool ok0 = !MASKED || (col_ok && row_ok[0]), ok1 = !MASKED || (col_ok && row_ok[1]);
                    if constexpr (IDS) {
                        ok0 = ok0 && !same_item(0, qi, r);
                        ok1 = ok1 && !same_item(1, qi, r);
                    }
                    const bool top0 = x0 == run_m[0], top1 = x1 == run_m[1];
                    ts[0] += (ok0 && !top0) ? fast_exp2(x0 - run_m[0]) : 0.f;
                    ts[1] += (ok1 && !top1) ? fast_exp2(x1 - run_m[1]) : 0.f;
                    ties[0] += (ok0 && top0) ? 1.f : 0.f;
                    ties[1] += (ok1 && top1) ? 1.f : 0.f;
                    if (!MASKED) {
                        cm[r] = fmaxf(x0, x1);
                        cs[r] = fast_exp2(-fabsf(x0 - x1));
                    } else {
                        cm[r] = fmaxf(ok0 ? x0 : kInfonceMasked, ok1 ? x1 : kInfonceMasked);
                        cs[r] = (ok0 && ok1) ? fast_exp2(-fabsf(x0 - x1)) : ((ok0 || ok1) ? 0.f : -1.f);
                    }
                }
                // the 32 lanes of the wave half (rows); the two row waves meet in LDS
                float hm, hs;
                halving_lse16(cm, cs, l31, &hm, &hs);
                if (l31 < 16) {
                    const int o = wr * 128 + 64 * wc + 32 * qi + frag_row(halving_elem16(l31), half);
                    redm[o] = hm;
                    reds[o] = hs;
                }
            }
#pragma unroll
            for (int pi = 0; pi < 2; ++pi) run_u[pi] += ts[pi] + ties[pi];
        };
        if (IDS || ragged_rows || t * 128 + 128 > b) epilogue(std::true_type());      // (block-uniform)
        else epilogue(std::false_type());
        __syncthreads();
        if (tid < 128) {
            float m0 = redm[tid], s0 = reds[tid];
            infonce_merge(m0, s0, redm[128 + tid], reds[128 + tid]);
            const size_t o = (size_t)rb * bpad + (size_t)t * 128 + tid;
            col_m[o] = m0;
            col_s[o] = s0;
        }
        __syncthreads();
    }
    // row side: the four lanes (wc, half) that share a row
#pragma unroll
    for (int pi = 0; pi < 2; ++pi) {
        const int o = (2 * wc + half) * 128 + 64 * wr + 32 * pi + l31;
        redm[o] = run_m[pi];
        reds[o] = run_u[pi];
    }
    __syncthreads();
    if (tid < 128) {
        float m0 = redm[tid], s0 = reds[tid];
#pragma unroll
        for (int k = 1; k < 4; ++k) infonce_merge(m0, s0, redm[k * 128 + tid], reds[k * 128 + tid]);
        const size_t o = (size_t)split * bpad + row0 + tid;
        row_m[o] = m0;
        row_s[o] = s0;
    }
}

// Merge and loss.  Entry p of the stacked [2][bpad] outputs: p < bpad the video row p over the texts (its nsplit row partials, in split
// order), p >= bpad the text column p - bpad over the videos (its bpad / 128 column partials, in row-block order); the (m, u) pairs are
// rescaled to the largest maximum M and added in fp64 with the first partial that attains M keeping its left-out term:
// U = u_first + sum over the others of (1 + u_k) exp2(m_k - M).  lse[p] + lse[2 bpad + p] = M + log2(1 + U) (log1p): the LOG2-DOMAIN log-sum-exp of x = c S,
// c = s log2(e) (ln 2 times it is the definition's lr / lc), as an fp32 value and what the rounding left over: where a soft-max is
// saturated the backward's P - 1 cancels against x - lse, and one fp32 of a value near 100 would leave 4e-6 of P in it.  0 for the
// padding entries.  The entry's share of the loss, ln 2 * (lse - c S[q][q]) with the
// positive pair's logit formed as the statistics kernel formed it, goes to fp64 block partials loss_ws[1 + block] (added up in index
// order by fwd_finish_reduce_kernel).
__global__ void __launch_bounds__(256) infonce_finish_kernel(const float* row_m, const float* row_s, int nsplit, const float* col_m,
                                                             const float* col_s, const float* pair, int bpad, int b,
                                                             const float* logit_scale, float* lse, float* pair_score, double* loss_ws) {
    CROSSCLR_SHARED double sh[256];
    const int n = 2 * bpad;
    const float c = logit_scale[0] * kLog2e;
    double acc = 0.0;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        const int q = p < bpad ? p : p - bpad;
        const float* pm = p < bpad ? row_m : col_m;
        const float* ps = p < bpad ? row_s : col_s;
        const int np = p < bpad ? nsplit : bpad / 128;
        float out = 0.f, out_lo = 0.f;
        if (q < b) {
            float mx = kInfonceMasked;
            for (int k = 0; k < np; ++k) mx = fmaxf(mx, pm[(size_t)k * bpad + q]);
            double U = 0.0;
            bool first = true;
            for (int k = 0; k < np; ++k) {
                const float mk = pm[(size_t)k * bpad + q];
                const double uk = (double)ps[(size_t)k * bpad + q];
                if (first && mk == mx) { U += uk; first = false; }
                else U += (1.0 + uk) * exp2((double)mk - (double)mx);
            }
            const double lg = log1p(U) * 1.4426950408889634;
            const double l2 = (double)mx + lg;
            out = (float)l2;
            out_lo = (float)(l2 - (double)out);
            acc += 0.6931471805599453 * (((double)mx - (double)infonce_logit(c, pair[q])) + lg);      // (saturated: mx IS the pair's logit, lg is all of it)
        }
        lse[p] = out;
        lse[n + p] = out_lo;
        if (p < bpad) pair_score[q] = q < b ? pair[q] : 0.f;
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_ws[1 + blockIdx.x] = sh[0];
}

// ---------------------------------------------------------------------------------------------
// Gradient product: the three-phase skeleton of bwd_kernel<..., LOSS = 1> on the stacked [2 bpad] rows, against the 64-column tiles of
// the OTHER modality only.  For a block of 64 rows P and an output slice of DC embedding columns:
//   phase A  S^T[q][p] = x^_Q . x^_P
//   phase B  W[p][q] = exp2(c S - lse[p]) + exp2(c S - lse[q]) - 2 [q is p's partner], lse = hi + lo subtracted in that order; the
//            partner's entry as expm1 + expm1 of the two arguments formed from pair[] = S[i][i] of the statistics pass: the very logit
//            lse was built on (a second evaluation may add the split operand's three products in another order: 4e-6 at a logit of 65,
//            2 % of a saturated 1 - P)   (the soft-max of p's own direction plus the one
//            of q's; both arguments <= 0 up to rounding; the partner's -2 inside the tile, against the same operand rounding as the
//            product), 0 for padding rows and columns; to LDS in operand type (bf16, or hi / lo for the split operand)
//   phase C  G[p][d] += W[p][:] . x^_Q[:, d]
// grid = (2 bpad / 64, Dpad / DC, slices); slice z walks tiles [z tps, (z + 1) tps) of the other modality's bpad / 64 and writes its own
// gbuf slice [2 bpad][Dpad] (a slice without tiles writes zeros).  Every score is evaluated here a second time.
// ---------------------------------------------------------------------------------------------
// IDS (pair ids): group [bpad], the same array for the video rows and the text rows: W is SELECTED to 0 where the statistics left the
// entry out (its logit was in neither log-sum-exp and may lie far above both: exp2 gives inf), before the operand split sees it.
template <typename T, int DC, bool IDS = false, typename... GROUP>
__global__ void __launch_bounds__(256) infonce_backward_kernel(const T* X, int b, int bpad, int Dpad, const float* logit_scale, const float* lse,
                                                               const float* pair, float* gbuf, int tiles_per_slice, GROUP... group_arg) {
    typedef Operand<T> Op;
    static_assert(sizeof...(GROUP) == (IDS ? 1 : 0), "IDS instantiations take the group array as their last argument");
    const int* group = group_of(group_arg...);
    typedef BwdLds<T, DC> L;
    CROSSCLR_SHARED __attribute__((aligned(16))) unsigned char lds[L::kTotal];
    unsigned char* tileP = lds + L::kTileP;
    unsigned char* tileQ = lds + L::kTileQ;
    unsigned char* wt = lds + L::kW;
    unsigned char* xq = lds + L::kXQ;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const size_t pitch = (size_t)Dpad * sizeof(T);
    const int nchunks = Dpad / Op::kChunkElems;
    const int row0 = blockIdx.x * 64;
    const int rmod = row0 / bpad;
    const int r_in_mod0 = row0 - rmod * bpad;
    const int d0 = blockIdx.y * DC;
    const unsigned char* rbase = reinterpret_cast<const unsigned char*>(X) + (size_t)row0 * pitch;
    const unsigned char* obase = reinterpret_cast<const unsigned char*>(X) + (size_t)(1 - rmod) * bpad * pitch;   // the other modality
    const float* lse_cols = lse + (size_t)(1 - rmod) * bpad;
    const int wq = wave & 1, wp = wave >> 1;      // phase A / B: columns 32 wq.., rows 32 wp..
    const int wr = wave & 1, wc = wave >> 1;      // phase C: rows 32 wr.., embedding columns wc (DC / 2)..
    const float c = logit_scale[0] * kLog2e;

    f32x16 acc2[DC / 64];
#pragma unroll
    for (int dt = 0; dt < DC / 64; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[dt][r] = 0.f;

    const int p_t = 32 * wp + l31;      // this lane's row inside the block (phase B)
    const float lse_p = lse[row0 + p_t], lse_p_lo = lse[2 * bpad + row0 + p_t];
    const bool p_ok = r_in_mod0 + p_t < b;
    const float x_pp = infonce_logit(c, pair[r_in_mod0 + p_t]);      // the positive pair's logit as the statistics saw it
    int grp_p = 0;
    if constexpr (IDS) grp_p = group[r_in_mod0 + p_t];

    const int ntiles = bpad / 64;
    const int t_begin = blockIdx.z * tiles_per_slice;
    int t_stop = t_begin + tiles_per_slice;
    if (t_stop > ntiles) t_stop = ntiles;
    KTileStage<64, 256> sp, sq;
    for (int u = t_begin; u < t_stop; ++u) {
        const int in_mod0 = u * 64;
        const unsigned char* cbase = obase + (size_t)in_mod0 * pitch;
        // ---------------- phase A ----------------
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        sp.fetch(rbase, pitch, 0, tid);
        sq.fetch(cbase, pitch, 0, tid);
        for (int kc = 0; kc < nchunks; ++kc) {
            sp.commit(tileP, tid);
            sq.commit(tileQ, tid);
            __syncthreads();  // also: every wave is past phase C of the previous tile
            if (kc == 0) {
                // column slice for phase C: [64][DC] elements, 16-byte pieces
                constexpr int kPiecesPerRow = DC * (int)sizeof(T) / 16;
                constexpr int kElemsPerPiece = 16 / (int)sizeof(T);
                for (int id = tid; id < 64 * kPiecesPerRow; id += 256) {
                    const int q = id / kPiecesPerRow, cc = id - q * kPiecesPerRow;
                    u32x4 v = *reinterpret_cast<const u32x4*>(cbase + (size_t)q * pitch + ((size_t)d0 + cc * kElemsPerPiece) * sizeof(T));
                    *reinterpret_cast<u32x4*>(xq + xq_off<T, DC>(q, cc * kElemsPerPiece)) = v;
                }
            }
            if (kc + 1 < nchunks) {
                sp.fetch(rbase, pitch, (kc + 1) * 128, tid);
                sq.fetch(cbase, pitch, (kc + 1) * 128, tid);
            }
#pragma unroll
            for (int s = 0; s < Op::kSteps; ++s) {
                typename Op::frag a = Op::load(tileQ, 32 * wq + l31, s, half);
                typename Op::frag bfr = Op::load(tileP, 32 * wp + l31, s, half);
                acc = Op::mma(a, bfr, acc);
            }
            __syncthreads();
        }
        // ---------------- phase B ----------------
        const bool diag_tile = in_mod0 == r_in_mod0;
        const bool ragged = in_mod0 + 64 > b;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int q0 = 32 * wq + 8 * r4 + 4 * half;  // frag_row(4 r4 + j, half) = q0 - 32 wq + j
            const f32x4 lq = *reinterpret_cast<const f32x4*>(lse_cols + in_mod0 + q0);
            const f32x4 lq_lo = *reinterpret_cast<const f32x4*>(lse_cols + 2 * bpad + in_mod0 + q0);
            i32x4 gq = {0, 0, 0, 0};
            if constexpr (IDS) gq = *reinterpret_cast<const i32x4*>(group + in_mod0 + q0);
            f32x4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x = infonce_logit(c, acc[4 * r4 + j]);
                const float ap = (x - lse_p) - lse_p_lo, aq = (x - lq[j]) - lq_lo[j];
                float v = fast_exp2(ap) + fast_exp2(aq);
                if (diag_tile && q0 + j == p_t)      // (P - 1) + (P' - 1) without forming a P near 1
                    v = expm1f(((x_pp - lse_p) - lse_p_lo) * kLn2) + expm1f(((x_pp - lq[j]) - lq_lo[j]) * kLn2);
                if (!p_ok || (ragged && in_mod0 + q0 + j >= b)) v = 0.f;
                // IDS: another pair of the row's own item.  Its logit was in neither log-sum-exp and may lie far above both (v = inf):
                // the weight is SELECTED to 0 before the operand split sees it
                if constexpr (IDS) v = (gq[j] == grp_p && in_mod0 + q0 + j != r_in_mod0 + p_t) ? 0.f : v;
                w[j] = v;
            }
            w_store4(wt, p_t, q0, w, (T*)nullptr);
        }
        __syncthreads();
        // ---------------- phase C ----------------
        bwd_gemm2<DC>(wt, xq, wr, wc * (DC / 2), lane, acc2, (T*)nullptr);
    }
    // G[row][d]: a lane holds column d = l31 of each fragment, 16 rows, into its own slice
    float* gslice = gbuf + (size_t)blockIdx.z * 2 * bpad * Dpad;
#pragma unroll
    for (int dt = 0; dt < DC / 64; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            gslice[(size_t)(row0 + 32 * wr + frag_row(r, half)) * Dpad + d0 + wc * (DC / 2) + 32 * dt + l31] = acc2[dt][r];
}

}  // namespace crossclr
