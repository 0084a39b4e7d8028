// crossclr_kernels_sigmoid.h -- the pairwise sigmoid loss (SigLIP) with a logit scale and a logit bias read from device memory
// (crossclr_sigmoid_* of include/crossclr.h):  z = s S + beta, S = v^ . t^T,
//   L = 1/B [ sum_i softplus(-z_ii) + sum_{i != j} softplus(z_ij) ],  W = sigma(z) - I,
// on the tiled-similarity skeleton of crossclr_kernels_infonce.h.  Neither z, sigma(z) nor their gradients are materialised.
//
//   sigmoid_stats_kernel            grid (video row blocks, column splits): per row, the sums of softplus(z) / ln 2 and of sigma(z) over the
//                                   split's NEGATIVE pairs, and S[i][i]
//   sigmoid_finish_kernel           adds the partials in split order and the positive pair's two terms, in fp64 -> row_loss, the loss and
//                                   sum_ij W_ij (dL/dbeta)
//   sigmoid_backward_kernel         the three-phase gradient product on the stacked rows against the tiles of the other modality:
//                                   W = sigma(z) - [positive pair], G = W . x^
//   pairloss_backward_finish_kernel (crossclr_kernels_pairloss.h) with g = s / B M_p
//
// LOG2 DOMAIN: x = c S + b2 with c = s log2(e) and b2 = beta log2(e), t = exp2(-|x|):
//   softplus(z) / ln 2 = max(x, 0) + log2(1 + t),   sigma(z) = x >= 0 ? 1 / (1 + t) : t / (1 + t)
// one exp2, one log2 and one reciprocal per element, no overflow for any finite x.  W needs no row or column statistics: nothing couples
// the bits of the statistics pass to those of the gradient product, each evaluates its own x.  Any finite s and beta (0 and negative
// values included).
#pragma once
#include <type_traits>

#include "crossclr_kernels_generic.h"
#include "crossclr_kernels_pairids.h"
#include "crossclr_kernels_pairloss.h"

namespace crossclr {

// t = exp2(-|x|) and 1 / (1 + t): what both softplus and sigma are made of
struct SigmoidTerms { float t, u, rcp; };
__device__ __forceinline__ SigmoidTerms sigmoid_terms(float x) {
    SigmoidTerms e;
    e.t = fast_exp2(-fabsf(x));
    e.u = 1.f + e.t;
    e.rcp = fast_rcp(e.u);
    return e;
}
// softplus(z) / ln 2.  log2(1 + t) of the rounded 1 + t: off by at most 2^-24 log2(e) ABSOLUTE per element, with either sign
__device__ __forceinline__ float sigmoid_softplus2(float x, const SigmoidTerms& e) { return fmaxf(x, 0.f) + fast_log2(e.u); }
__device__ __forceinline__ float sigmoid_sigma(float x, const SigmoidTerms& e) { return x >= 0.f ? e.rcp : e.t * e.rcp; }
// -sigma(-z), the positive pair's weight, from the same t and reciprocal: never sigma(z) - 1, which at z = 12 keeps 1 % of it
__device__ __forceinline__ float sigmoid_pair_weight(float x, const SigmoidTerms& e) { return x >= 0.f ? -(e.t * e.rcp) : -e.rcp; }

// ---------------------------------------------------------------------------------------------
// Tiled similarity with a softplus / sigmoid epilogue: the main loop of infonce_stats_kernel (128 video rows x 128 text rows of the packed
// operand X[2][bpad][Dpad], K-chunks of 128 bytes, two in flight, MFMA operands swapped: a lane owns video row p = l31 of each 32 x 32
// fragment and 16 of its columns).  grid = (bpad / 128, nsplit); no column side, no atomics; every slot has one writer.
//   A lane adds each tile's 32 terms of its two rows (fp32) and carries the two sums of each row across the tiles; the four lanes
//   (wc, half) of a row meet once, at the end, in LDS -> row_sp / row_sig [nsplit][bpad].
//   Masking BY INDEX: padding rows and columns (>= b: zeros in the operand, they would add softplus(beta) each) contribute nothing, and
//   neither does THE POSITIVE PAIR: at SigLIP's initial values its softplus is about 10 next to negatives of 4.5e-5 each, and an fp32 sum
//   that holds both loses the small ones.  sigmoid_finish_kernel forms its terms from pair[i] = S[i][i], written here from the diagonal
//   tile's accumulators.
//   LDS: 2 x 16 KiB operand chunks + 4 KiB of reduction slots.
// ---------------------------------------------------------------------------------------------
//   IDS (pair ids, crossclr_kernels_pairids.h): group [bpad]; an entry (i, j), i != j, with group[i] == group[j] is no negative pair and
//   stays out of both row sums; every tile takes the masked epilogue.
template <typename T, bool IDS = false, typename... GROUP>
__global__ void __launch_bounds__(256, 2) sigmoid_stats_kernel(const T* X, int b, int bpad, int Dpad, int tiles_per_split,
                                                               const float* logit_scale, const float* logit_bias, float* row_sp,
                                                               float* row_sig, float* pair, GROUP... group_arg) {
    typedef Operand<T> Op;
    static_assert(sizeof...(GROUP) == (IDS ? 1 : 0), "IDS instantiations take the group array as their last argument");
    const int* group = group_of(group_arg...);
    CROSSCLR_SHARED __attribute__((aligned(16))) unsigned char lds[2 * 128 * 128];
    CROSSCLR_SHARED float red_sp[4 * 128];
    CROSSCLR_SHARED float red_sg[4 * 128];
    int* colg = nullptr;      // IDS: the groups of the tile's 128 columns, two tiles' worth (a tile's readers and the next one's writers
    int rg[2] = {0, 0};       // never meet in one half), and of the lane's two rows
    if constexpr (IDS) {
        CROSSCLR_SHARED __attribute__((aligned(16))) int col_groups[2 * 128];
        colg = col_groups;
    }
    unsigned char* tileP = lds;                 // video chunk [128][128 B]
    unsigned char* tileQ = lds + 128 * 128;     // text chunk  [128][128 B]

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
    const float c = logit_scale[0] * kLog2e, b2 = logit_bias[0] * kLog2e;

    float run_sp[2] = {0.f, 0.f}, run_sg[2] = {0.f, 0.f};
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
        const int row[2] = {row0 + 64 * wr + l31, row0 + 64 * wr + 32 + l31};
        if (t == rb) {      // the positive pairs' scores (block-uniform)
#pragma unroll
            for (int qi = 0; qi < 2; ++qi)
#pragma unroll
                for (int r = 0; r < 16; ++r)
#pragma unroll
                    for (int pi = 0; pi < 2; ++pi)
                        if (row[pi] == col0 + 32 * qi + frag_row(r, half)) pair[row[pi]] = acc[qi][pi][r];
        }
        auto epilogue = [&](auto masked_c) {
            constexpr bool MASKED = decltype(masked_c)::value;
            float ts[2] = {0.f, 0.f}, tg[2] = {0.f, 0.f};      // the tile's terms of the lane's two rows
#pragma unroll
            for (int qi = 0; qi < 2; ++qi)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int col = col0 + 32 * qi + frag_row(r, half);
                    int cg = 0;
                    if constexpr (IDS) cg = colg[(t & 1) * 128 + col - t * 128];
#pragma unroll
                    for (int pi = 0; pi < 2; ++pi) {
                        const float x = fmaf(c, acc[qi][pi][r], b2);
                        const SigmoidTerms e = sigmoid_terms(x);
                        // IDS: the pairs of the row's own item are no negatives (the positive pair, of the same group, is the finish's)
                        const bool ok = !MASKED || (col < b && row[pi] < b && (IDS ? cg != rg[pi] : col != row[pi]));
                        ts[pi] += ok ? sigmoid_softplus2(x, e) : 0.f;
                        tg[pi] += ok ? sigmoid_sigma(x, e) : 0.f;
                    }
                }
#pragma unroll
            for (int pi = 0; pi < 2; ++pi) {
                run_sp[pi] += ts[pi];
                run_sg[pi] += tg[pi];
            }
        };
        if (IDS || ragged_rows || t * 128 + 128 > b || t == rb) epilogue(std::true_type());      // (block-uniform)
        else epilogue(std::false_type());
    }
    // the four lanes (wc, half) that share a row, in a fixed order
#pragma unroll
    for (int pi = 0; pi < 2; ++pi) {
        const int o = (2 * wc + half) * 128 + 64 * wr + 32 * pi + l31;
        red_sp[o] = run_sp[pi];
        red_sg[o] = run_sg[pi];
    }
    __syncthreads();
    if (tid < 128) {
        float s0 = red_sp[tid], g0 = red_sg[tid];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            s0 += red_sp[k * 128 + tid];
            g0 += red_sg[k * 128 + tid];
        }
        const size_t o = (size_t)split * bpad + row0 + tid;
        row_sp[o] = s0;
        row_sig[o] = g0;
    }
}

// Per video row i < b, in fp64: the row's nsplit partials in split order, then the positive pair's softplus(-z_ii) and -sigma(-z_ii)
// evaluated from pair[i], s and beta.  row_loss[i] = softplus(-z_ii) + sum_{j != i} softplus(z_ij) in nats (0 for padding entries);
// the block's sums of row_loss and of sum_j W_ij go to fp64 block partials loss_ws[1 + block] / sig_ws[1 + block] (added up in index
// order by fwd_finish_reduce_kernel).
__global__ void __launch_bounds__(256) sigmoid_finish_kernel(const float* row_sp, const float* row_sig, int nsplit, const float* pair, int bpad,
                                                             int b, const float* logit_scale, const float* logit_bias, float* row_loss,
                                                             float* pair_score, double* loss_ws, double* sig_ws) {
    CROSSCLR_SHARED double sh_l[256];
    CROSSCLR_SHARED double sh_g[256];
    const double s = (double)logit_scale[0], beta = (double)logit_bias[0];
    double acc_l = 0.0, acc_g = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < bpad; i += gridDim.x * 256) {
        float out = 0.f, ps = 0.f;
        if (i < b) {
            double sp = 0.0, sg = 0.0;
            for (int k = 0; k < nsplit; ++k) {
                sp += (double)row_sp[(size_t)k * bpad + i];
                sg += (double)row_sig[(size_t)k * bpad + i];
            }
            ps = pair[i];
            const double z = s * (double)ps + beta;
            const double e = exp(-fabs(z));
            const double l = 0.6931471805599453 * sp + (fmax(-z, 0.0) + log1p(e));      // softplus(-z_ii)
            out = (float)l;
            acc_l += l;
            acc_g += sg - (z >= 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e));                  // -sigma(-z_ii)
        }
        row_loss[i] = out;
        pair_score[i] = ps;
    }
    sh_l[threadIdx.x] = acc_l;
    sh_g[threadIdx.x] = acc_g;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sh_l[threadIdx.x] += sh_l[threadIdx.x + o];
            sh_g[threadIdx.x] += sh_g[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss_ws[1 + blockIdx.x] = sh_l[0];
        sig_ws[1 + blockIdx.x] = sh_g[0];
    }
}

// ---------------------------------------------------------------------------------------------
// Gradient product: the three-phase skeleton of infonce_backward_kernel on the stacked [2 bpad] rows, against the 64-column tiles of
// the OTHER modality only.  For a block of 64 rows P and an output slice of DC embedding columns:
//   phase A  S^T[q][p] = x^_Q . x^_P
//   phase B  W[p][q] = sigma(z) of the score just evaluated; the partner's entry in the diagonal tile is -sigma(-z) from the same t
//            and reciprocal; 0 for padding rows and columns; to LDS in operand type (bf16, or hi / lo for the split operand)
//   phase C  G[p][d] += W[p][:] . x^_Q[:, d]
// grid = (2 bpad / 64, Dpad / DC, slices); slice z walks tiles [z tps, (z + 1) tps) of the other modality's bpad / 64 and writes its own
// gbuf slice [2 bpad][Dpad] (a slice without tiles writes zeros).  Inputs: the packed operand, s and beta -- no saved statistics.
// ---------------------------------------------------------------------------------------------
// IDS (pair ids): group [bpad], the same array for the video rows and the text rows: W = 0 where the statistics left the entry out.
template <typename T, int DC, bool IDS = false, typename... GROUP>
__global__ void __launch_bounds__(256) sigmoid_backward_kernel(const T* X, int b, int bpad, int Dpad, const float* logit_scale,
                                                               const float* logit_bias, float* gbuf, int tiles_per_slice,
                                                               GROUP... group_arg) {
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
    const int wq = wave & 1, wp = wave >> 1;      // phase A / B: columns 32 wq.., rows 32 wp..
    const int wr = wave & 1, wc = wave >> 1;      // phase C: rows 32 wr.., embedding columns wc (DC / 2)..
    const float c = logit_scale[0] * kLog2e, b2 = logit_bias[0] * kLog2e;

    f32x16 acc2[DC / 64];
#pragma unroll
    for (int dt = 0; dt < DC / 64; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[dt][r] = 0.f;

    const int p_t = 32 * wp + l31;      // this lane's row inside the block (phase B)
    const bool p_ok = r_in_mod0 + p_t < b;
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
            i32x4 gq = {0, 0, 0, 0};
            if constexpr (IDS) gq = *reinterpret_cast<const i32x4*>(group + in_mod0 + q0);
            f32x4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x = fmaf(c, acc[4 * r4 + j], b2);
                const SigmoidTerms e = sigmoid_terms(x);
                float v = sigmoid_sigma(x, e);
                if (diag_tile && q0 + j == p_t) v = sigmoid_pair_weight(x, e);
                if (!p_ok || (ragged && in_mod0 + q0 + j >= b)) v = 0.f;
                if constexpr (IDS) v = (gq[j] == grp_p && in_mod0 + q0 + j != r_in_mod0 + p_t) ? 0.f : v;      // another pair of the row's own item
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
