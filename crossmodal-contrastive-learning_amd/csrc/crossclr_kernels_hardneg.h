// crossclr_kernels_hardneg.h -- the maximum-violation (hardest-negative) form of the max-margin ranking loss (crossclr_hardneg_* of
// include/crossclr.h; VSE++ / COOT `max_violation=True`): per video row the best-scoring text that is not its partner, per text column the
// best-scoring video that is not its partner, over S = im . s^T on the tiled-similarity skeleton of fwd_sums_kernel.  S is never materialised.
//
//   hardneg_select_kernel    grid (video row blocks, column splits): best (score, column) of every row over the split's columns, best
//                            (score, row) of every column over the block's rows, and the positive pairs' scores S[i][i]
//   hardneg_finish_kernel    merges the partials in a fixed order, forms the two hinges per sample and the loss
//   hardneg_backward_kernel  the sparse gradient: every row and every column contributes at most one pair -- an O(B D) gather
//
// TOTAL ORDER (topk_better of crossclr_kernels_topk.h, everywhere in this file): (s, i) is better than (s', i') when s > s', or s == s' and
// i < i'.  Indices are distinct, so the order is strict and the best of a set is ONE element: neither the grid, the split count nor the
// order in which blocks run can change what is selected.  NaN scores are not ordered (every comparison with them is false): a NaN is never
// selected over a number, and which index a row of NaNs reports is unspecified.
#pragma once
#include "crossclr_kernels_topk.h"

namespace crossclr {

constexpr int kHardnegNone = 0x7fffffff;      // "no candidate" in the partials: worse than every real index at any score
constexpr int kHardnegNoRow = 1 << 24;        // the same inside a block (in-block row numbers travel through lane_xor as float bits)

template <int MASK> __device__ __forceinline__ int lane_xor_int(int v) {
    return __builtin_bit_cast(int, lane_xor<MASK>(__builtin_bit_cast(float, v)));
}
__device__ __forceinline__ void hardneg_take(float& s, int& i, float s2, int i2) {
    if (topk_better(s2, i2, s, i)) { s = s2; i = i2; }
}
// halving_sum16's exchange pattern on (score, index) pairs under the total order: every lane ends up with the best pair of element
// halving_elem16(l31) over the 32 lanes of its wave half.
__device__ __forceinline__ void halving_best16(const float (&s)[16], const int (&ix)[16], int l31, float* out_s, int* out_i) {
    float s8[8], s4[4], s2[2];
    int i8[8], i4[4], i2[2];
    {
        const bool up = (l31 >> 3) & 1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            s8[i] = up ? s[8 + i] : s[i];
            i8[i] = up ? ix[8 + i] : ix[i];
            hardneg_take(s8[i], i8[i], lane_xor<15>(up ? s[i] : s[8 + i]), lane_xor_int<15>(up ? ix[i] : ix[8 + i]));
        }
    }
    {
        const bool up = (l31 >> 2) & 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            s4[i] = up ? s8[4 + i] : s8[i];
            i4[i] = up ? i8[4 + i] : i8[i];
            hardneg_take(s4[i], i4[i], lane_xor<7>(up ? s8[i] : s8[4 + i]), lane_xor_int<7>(up ? i8[i] : i8[4 + i]));
        }
    }
    {
        const bool up = (l31 >> 1) & 1;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            s2[i] = up ? s4[2 + i] : s4[i];
            i2[i] = up ? i4[2 + i] : i4[i];
            hardneg_take(s2[i], i2[i], lane_xor<2>(up ? s4[i] : s4[2 + i]), lane_xor_int<2>(up ? i4[i] : i4[2 + i]));
        }
    }
    const bool up = l31 & 1;
    float s1 = up ? s2[1] : s2[0];
    int i1 = up ? i2[1] : i2[0];
    hardneg_take(s1, i1, lane_xor<1>(up ? s2[0] : s2[1]), lane_xor_int<1>(up ? i2[0] : i2[1]));
    hardneg_take(s1, i1, lane_xor<16>(s1), lane_xor_int<16>(i1));
    *out_s = s1;
    *out_i = i1;
}

// ---------------------------------------------------------------------------------------------
// Tiled similarity with a max + argmax epilogue in both directions.
//   block = 256 threads (4 waves as 2x2), tile = 128 video rows x 128 text rows of the packed operand X[2][bpad][Dpad], K-chunks of 128
//   bytes, two chunks in flight, MFMA operands swapped (A = text rows, B = video rows) -- the main loop of fwd_sums_kernel's one-pass score
//   mode: a lane owns one video row p = l31 of each 32x32 fragment and 16 of its columns.
//   grid = (bpad / 128, nsplit); split y walks tiles [y * tiles_per_split, (y + 1) * tiles_per_split).  No atomics; every slot of the
//   partials has exactly one writer.
//   Row side: a lane carries the best (score, column) of its two rows across the tiles; it meets its columns in ascending order, so a
//   strict > keeps the lowest index among equal scores.  The four lanes (wc, half) that share a row are reduced once, at the end, through
//   LDS -> row_s / row_i [nsplit][bpad] (column indices, kHardnegNone when the split held no candidate for the row).
//   Column side, per tile: a lane's best (score, row) of each of its 32 columns over its two rows, halving_best16 over the 32 lanes of the
//   wave half, the two row waves through LDS -> col_s / col_i [bpad / 128][bpad] (row numbers inside the block, kHardnegNoRow for none).
//   Masking BY INDEX (all real scores may be negative): padding rows and columns (>= b, zeros in the operand) and the positive pair.
//   The positive pairs' scores S[i][i] are on the diagonal of tile t == row block and go to pair[bpad]: the very accumulator values the
//   selections are compared with, in every compute mode.
//   LDS: 2 x 16 KiB operand chunks + 4 KiB of reduction slots.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256, 2) hardneg_select_kernel(const T* X, int b, int bpad, int Dpad, int tiles_per_split, float* row_s,
                                                                int* row_i, float* col_s, int* col_i, float* pair) {
    typedef Operand<T> Op;
    CROSSCLR_SHARED __attribute__((aligned(16))) unsigned char lds[2 * 128 * 128];
    CROSSCLR_SHARED float red_s[4 * 128];
    CROSSCLR_SHARED int red_i[4 * 128];
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

    const float kNegInf = -__builtin_inff();
    float best_s[2] = {kNegInf, kNegInf};
    int best_i[2] = {kHardnegNone, kHardnegNone};

    KTileStage<128, 256> sp, sq, sp2, sq2;
    for (int t = t_begin; t < t_end; ++t) {
        const unsigned char* cbase = tbase + (size_t)t * 128 * pitch;
        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;

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
        const bool diag_tile = t == rb;
        const bool masked_tile = diag_tile || ragged_rows || t * 128 + 128 > b;      // (block-uniform)
#pragma unroll
        for (int qi = 0; qi < 2; ++qi) {
            float cs[16];      // column side: the lane's best (score, row inside the block) of each of its 16 columns
            int ci[16];
            if (!masked_tile) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int col = col0 + 32 * qi + frag_row(r, half);
                    const float v0 = acc[qi][0][r], v1 = acc[qi][1][r];
                    if (v0 > best_s[0]) { best_s[0] = v0; best_i[0] = col; }
                    if (v1 > best_s[1]) { best_s[1] = v1; best_i[1] = col; }
                    const bool second = v1 > v0;      // (rows ascend with pi: a tie keeps the first)
                    cs[r] = second ? v1 : v0;
                    ci[r] = 64 * wr + l31 + (second ? 32 : 0);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int col = col0 + 32 * qi + frag_row(r, half);
                    float bs = kNegInf;
                    int bi = kHardnegNoRow;
#pragma unroll
                    for (int pi = 0; pi < 2; ++pi) {
                        const int p_t = 64 * wr + 32 * pi + l31, row = row0 + p_t;
                        const float v = acc[qi][pi][r];
                        if (diag_tile && row == col) pair[row] = v;
                        const bool ok = row < b && col < b && row != col;
                        if (ok && v > best_s[pi]) { best_s[pi] = v; best_i[pi] = col; }
                        if (ok && (bi == kHardnegNoRow || v > bs)) { bs = v; bi = p_t; }
                    }
                    cs[r] = bs;
                    ci[r] = bi;
                }
            }
            // the 32 lanes of the wave half (rows); the two row waves meet in LDS
            float hs;
            int hi;
            halving_best16(cs, ci, l31, &hs, &hi);
            if (l31 < 16) {
                const int c = wr * 128 + 64 * wc + 32 * qi + frag_row(halving_elem16(l31), half);
                red_s[c] = hs;
                red_i[c] = hi;
            }
        }
        __syncthreads();
        if (tid < 128) {
            float s0 = red_s[tid];
            int i0 = red_i[tid];
            hardneg_take(s0, i0, red_s[128 + tid], red_i[128 + tid]);
            const size_t o = (size_t)rb * bpad + (size_t)t * 128 + tid;
            col_s[o] = s0;
            col_i[o] = i0;
        }
        __syncthreads();
    }
    // row side: the four lanes (wc, half) that share a row
#pragma unroll
    for (int pi = 0; pi < 2; ++pi) {
        const int c = (2 * wc + half) * 128 + 64 * wr + 32 * pi + l31;
        red_s[c] = best_s[pi];
        red_i[c] = best_i[pi];
    }
    __syncthreads();
    if (tid < 128) {
        float s0 = red_s[tid];
        int i0 = red_i[tid];
#pragma unroll
        for (int k = 1; k < 4; ++k) hardneg_take(s0, i0, red_s[k * 128 + tid], red_i[k * 128 + tid]);
        const size_t o = (size_t)split * bpad + row0 + tid;
        row_s[o] = s0;
        row_i[o] = i0;
    }
}

// Merge and hinges.  Entry p of the stacked [2][bpad] outputs: p < bpad the video row p against the texts (its nsplit row partials, in split
// order), p >= bpad the text column p - bpad against the videos (its bpad / 128 column partials, in row-block order), both under the total
// order.  hinge = max(0, margin + best - pair) in fp32, the arithmetic of the sum form's one-pass kernel.  A sample without a candidate
// (B = 1) and the padding entries report index -1, score -inf and hinge 0.  The block partials of the hinge sum go to loss_ws[1 + block]
// (double; added up in index order by fwd_finish_reduce_kernel).
__global__ void __launch_bounds__(256) hardneg_finish_kernel(const float* row_s, const int* row_i, int nsplit, const float* col_s, const int* col_i,
                                                             const float* pair, int bpad, int b, float margin, int* best_index,
                                                             float* best_score, float* hinge, float* pair_score, double* loss_ws) {
    CROSSCLR_SHARED double sh[256];
    const int n = 2 * bpad;
    double acc = 0.0;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        const int q = p < bpad ? p : p - bpad;
        float s = -__builtin_inff();
        int i = kHardnegNone;
        if (p < bpad) {
            for (int k = 0; k < nsplit; ++k) hardneg_take(s, i, row_s[(size_t)k * bpad + q], row_i[(size_t)k * bpad + q]);
        } else {
            const int nrb = bpad / 128;
            for (int k = 0; k < nrb; ++k) {
                const int r = col_i[(size_t)k * bpad + q];
                hardneg_take(s, i, col_s[(size_t)k * bpad + q], r >= 128 ? kHardnegNone : k * 128 + r);
            }
        }
        const bool found = q < b && i >= 0 && i < b;
        const float h = found ? fmaxf(0.f, margin + s - pair[q]) : 0.f;
        best_index[p] = found ? i : -1;
        best_score[p] = found ? s : -__builtin_inff();
        hinge[p] = h;
        if (p < bpad) pair_score[q] = q < b ? pair[q] : 0.f;
        acc += (double)h;
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
// Gradient of the hardest-negative loss: a deterministic gather, no atomics.  With O = the OTHER modality's rows (the caller's own tensors,
// not the packed copy), idx / h = this modality's selections and hinges, idx' / h' = the other's, and an entry ACTIVE when its hinge is positive
// and its index lies in [0, b) (index -1 = no candidate: such an entry contributes nothing, whatever its hinge):
//   out[r] = ( [r active] (O[idx[r]] - O[r])  -  [r active'] O[r]  +  sum over i ascending, i active' and idx'[i] == r, of O[i] ) * grad_out / B^2
//   grid = (ceil(b / 4), 2 modalities); one wave per output row, a lane owns columns lane + 64 k of a slab of 64 * kHardnegSlab columns
//   (the scan is repeated per slab: once for D <= 1024).
//   The scan: idx' and h' are staged through LDS kHardnegStage entries at a time; every thread marks which of the block's four rows its
//   entries select (-1: none) and, for a mark, raises two flags with plain stores of the same value: (row, stage) and (row, group of 32
//   entries).  A wave whose row has no mark in the stage skips it; otherwise it walks the stage's group flags and, inside a flagged group,
//   the 32 marks, in ascending order, and adds the rows that name its row -- a row's ~1 selector costs it ~100 broadcast LDS reads, not
//   one per entry.  Every index is checked against [0, b) before it becomes an address: a wrong index gives a wrong number.
//   Accumulation in fp32 (fp64 for fp64 inputs) in that fixed order; output in the input dtype.
// ---------------------------------------------------------------------------------------------
constexpr int kHardnegSlab = 16;
constexpr int kHardnegStage = 2048;     // entries of the index array per LDS stage: 8 per thread, 64 groups of 32
template <typename TIN> struct HardnegAcc { typedef float type; };
template <> struct HardnegAcc<double> { typedef double type; };

template <typename TIN>
__global__ void __launch_bounds__(256) hardneg_backward_kernel(const TIN* im, const TIN* s, long ld_im, long ld_s, int b, int bpad, int D,
                                                               const int* best_index, const float* hinge, const double* grad_out, TIN* g_im,
                                                               TIN* g_s, long ld_gim, long ld_gs) {
    typedef typename HardnegAcc<TIN>::type ACC;
    CROSSCLR_SHARED int mark[kHardnegStage];
    CROSSCLR_SHARED int group_flag[kHardnegStage / 32 * 4];      // [group][row of the block]
    CROSSCLR_SHARED int stage_flag[4];
    static_assert(kHardnegStage / 32 * 4 == 256, "one group flag per thread to clear");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = blockIdx.y;                                   // 0: grad_im (O = s), 1: grad_s (O = im)
    TIN* out = m == 0 ? g_im : g_s;
    if (!out) return;                                           // (block-uniform)
    const long ld_out = m == 0 ? ld_gim : ld_gs;
    const TIN* O = m == 0 ? s : im;
    const long ld_o = m == 0 ? ld_s : ld_im;
    const int* idx = best_index + (size_t)m * bpad;
    const float* h = hinge + (size_t)m * bpad;
    const int* idx2 = best_index + (size_t)(1 - m) * bpad;
    const float* h2 = hinge + (size_t)(1 - m) * bpad;
    const int r0 = blockIdx.x * 4, r = r0 + wave;
    const bool live = r < b;                                    // (wave-uniform; the waves of a ragged last block still take part in the barriers)
    const double scale = grad_out[0] / ((double)b * (double)b);
    int own = -1;
    bool own_active = false, other_active = false;
    if (live) {
        own = idx[r];
        own_active = h[r] > 0.f && own >= 0 && own < b;
        other_active = h2[r] > 0.f && idx2[r] >= 0 && idx2[r] < b;      // (an entry without a candidate, index -1, contributes nothing)
    }
    for (int d0 = 0; d0 < D; d0 += 64 * kHardnegSlab) {
        ACC acc[kHardnegSlab];
#pragma unroll
        for (int k = 0; k < kHardnegSlab; ++k) acc[k] = 0;
        auto add_row = [&](int i, ACC sign) {
            const TIN* po = O + (size_t)i * ld_o;
#pragma unroll
            for (int k = 0; k < kHardnegSlab; ++k) {
                const int d = d0 + lane + 64 * k;
                if (d < D) acc[k] += sign * (ACC)in_load(po, d);
            }
        };
        if (own_active) { add_row(own, (ACC)1); add_row(r, (ACC)-1); }
        if (other_active) add_row(r, (ACC)-1);
        for (int i0 = 0; i0 < b; i0 += kHardnegStage) {
            group_flag[tid] = 0;
            if (tid < 4) stage_flag[tid] = 0;
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kHardnegStage / 256; ++u) {
                const int e = tid + 256 * u, i = i0 + e;
                int mk = -1;
                if (i < b && h2[i] > 0.f) {
                    const int rel = idx2[i] - r0;
                    if (rel >= 0 && rel < 4 && r0 + rel < b) mk = rel;
                }
                mark[e] = mk;
                if (mk >= 0) { group_flag[(e >> 5) * 4 + mk] = 1; stage_flag[mk] = 1; }      // (every writer stores the same value)
            }
            __syncthreads();
            if (stage_flag[wave]) {                             // (wave-uniform: broadcast reads)
                const int n = b - i0 < kHardnegStage ? b - i0 : kHardnegStage;
                for (int g = 0; g * 32 < n; ++g) {
                    if (!group_flag[g * 4 + wave]) continue;
                    for (int e = g * 32; e < g * 32 + 32; ++e)
                        if (mark[e] == wave) add_row(i0 + e, (ACC)1);
                }
            }
            __syncthreads();
        }
        if (live) {
            TIN* po = out + (size_t)r * ld_out;
#pragma unroll
            for (int k = 0; k < kHardnegSlab; ++k) {
                const int d = d0 + lane + 64 * k;
                if (d < D) in_store(po, d, (double)acc[k] * scale);
            }
        }
    }
}

}  // namespace crossclr
