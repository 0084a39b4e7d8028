// crossclr_kernels_topk.h -- retrieval: the k best gallery rows of every query row over S = Q . G^T (crossclr_topk_* of
// include/crossclr.h), on the tiled-similarity skeleton of fwd_sums_kernel with a SELECTION epilogue.  S is never materialised.
//
//   topk_pack_kernel     one set of rows -> the packed operand X[rows_pad][Dpad] (the row arithmetic of normalize_kernel)
//   topk_select_kernel   grid (query row blocks, column splits): per query row the k best (score, index) pairs over the split's columns
//   topk_merge_kernel    per query row: its nsplit * k candidates -> the final k, sorted
//
// TOTAL ORDER (everywhere in this file): (s, i) is better than (s', i') when s > s', or s == s' and i < i'.  Gallery indices are distinct, so
// the order is strict, the k best of a set are ONE set, and neither the split count nor the order in which lanes insert can change the result.
#pragma once
#include "crossclr_kernels_generic.h"

namespace crossclr {

constexpr int kTopkMaxK = 64;            // crossclr_topk_max_k
constexpr int kTopkMaxCandidates = 1024; // nsplit * k candidates per query row (the merge kernel's LDS)
constexpr int kTopkSentinel = 0x7fffffff;

__device__ __forceinline__ bool topk_better(float s, int i, float s2, int i2) { return s > s2 || (s == s2 && i < i2); }

// One set of rows, cast / L2-normalised (x / max(||x||, 1e-12), float64 sums: term by term what normalize_kernel does for a modality) into
// X[rows_pad][Dpad]; rows >= `rows` and columns >= D are zeros.  One wavefront per row; HBM-bound.
template <typename TIN, typename T, bool NORM>
__global__ void __launch_bounds__(256) topk_pack_kernel(const TIN* x, long ld, int rows, int rows_pad, int D, int Dpad, T* X) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wave;
    if (i >= rows_pad) return;
    T* xo = X + (size_t)i * Dpad;
    const float zero4[4] = {0.f, 0.f, 0.f, 0.f};
    if (i >= rows) {
        for (int d = 4 * lane; d < Dpad; d += 256) op_store4(xo, d, zero4);
        return;
    }
    const TIN* px = x + (size_t)i * ld;
    const bool cached = D <= 256 * kRowCache;
    double cv[kRowCache][4];
    double ss = 0;
    if (cached) {
#pragma unroll
        for (int k = 0; k < kRowCache; ++k) {
            const int d = 4 * lane + 256 * k;
            if (d < D) {
                row_load4(px, d, D, cv[k]);
                if (NORM) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) ss += cv[k][j] * cv[k][j];
                }
            }
        }
    } else if (NORM) {
        for (int d = lane; d < D; d += 64) { const double a = in_load(px, d); ss += a * a; }
    }
    double iv = 1.0;
    if (NORM) {       // (a wave-collective: every lane of the row's wave is here)
        ss = wave_sum_f64(ss);
        const double n = sqrt(ss);
        iv = 1.0 / (n > 1e-12 ? n : 1e-12);
    }
    if (cached) {
#pragma unroll
        for (int k = 0; k < kRowCache; ++k) {
            const int d = 4 * lane + 256 * k;
            if (d < Dpad) {
                float a[4] = {0.f, 0.f, 0.f, 0.f};
                if (d < D) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) a[j] = (float)(cv[k][j] * iv);
                }
                op_store4(xo, d, a);
            }
        }
        for (int d = 4 * lane + 256 * kRowCache; d < Dpad; d += 256) op_store4(xo, d, zero4);
    } else {
        for (int d = lane; d < Dpad; d += 64) op_store(xo, d, d < D ? (float)(in_load(px, d) * iv) : 0.f);
    }
}

// ---------------------------------------------------------------------------------------------
// Tiled similarity with a selection epilogue.
//   block = 256 threads (4 waves as 2x2), tile = 128 query rows x 128 gallery rows, K-chunks of 128 bytes, two chunks in flight, MFMA
//   operands swapped (A = gallery rows, B = query rows) -- the main loop of fwd_sums_kernel: a lane owns one query row p = l31 of each 32x32
//   fragment and 16 of its columns; row p of the tile is shared by the four lanes (wc, half) of two waves.
//   grid = (nq_pad / 128, nsplit); split y walks tiles [y * tiles_per_split, (y + 1) * tiles_per_split) and writes its own workspace slot
//   ws[y][nq_pad][k] (scores, then indices): no atomics, no dependence on block order.
//   Candidate lists: per query row k (score, index) pairs in LDS, UNSORTED, with the row's WORST entry (score, index, position) cached next to
//   them.  Common path per score: one compare (>=) against the worst score, held in a register, into a 32-bit mask per row.  Lanes with a
//   non-empty mask then take turns -- four phases (wc, half), so that a row has one writer at a time -- and for every marked score that beats
//   the worst entry under the total order overwrite that entry and rescan the k entries for the new worst.  A row sees ~ k ln(N / k)
//   insertions over N columns, so after the first tiles the phases are four barriers and nothing else.
//   Unused entries are sentinels (-inf, distinct indices counting down from INT_MAX): worse than every real candidate; a split with fewer
//   than k real columns hands them to the merge, where they lose against the >= k real candidates of the whole gallery.
//   Gallery padding rows (index >= ng) are zeros and would score 0: they are masked BY INDEX (all real scores may be negative).
//   LDS per block: 2 x 16 KiB operand chunks + 128 x (KC + 1) x 8 B lists (+1: rows on distinct banks) + 1.5 KiB worst entries
//     KC = 16 (k <= 16): 32 + 17 + 1.5 = 50.5 KiB -> 3 blocks of a CU's 160 KiB; launch bounds ask for 2 (8 waves per CU, as fwd_sums_kernel)
//     KC = 64 (k <= 64): 32 + 65 + 1.5 = 98.5 KiB -> 1 block per CU (4 waves)
// ---------------------------------------------------------------------------------------------
template <typename T, int KC>
__global__ void __launch_bounds__(256, KC <= 16 ? 2 : 1) topk_select_kernel(const T* Q, const T* G, int nq, int ng, int nq_pad, int Dpad, int k,
                                                                            int tiles_per_split, float* ws_scores, int* ws_index) {
    typedef Operand<T> Op;
    constexpr int LS = KC + 1;      // list stride, in entries
    CROSSCLR_SHARED __attribute__((aligned(16))) unsigned char lds[2 * 128 * 128];
    CROSSCLR_SHARED float cand_s[128 * LS];
    CROSSCLR_SHARED int cand_i[128 * LS];
    CROSSCLR_SHARED float worst_s[128];
    CROSSCLR_SHARED int worst_i[128];
    CROSSCLR_SHARED int worst_p[128];
    unsigned char* tileP = lds;                 // query chunk   [128][128 B]
    unsigned char* tileQ = lds + 128 * 128;     // gallery chunk [128][128 B]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int wr = wave & 1, wc = wave >> 1;
    const size_t pitch = (size_t)Dpad * sizeof(T);
    const int nchunks = Dpad / Op::kChunkElems;
    const int row0 = blockIdx.x * 128, split = blockIdx.y;
    const int ntiles = (ng + 127) / 128;
    const int t_begin = split * tiles_per_split;
    const int t_end = t_begin + tiles_per_split < ntiles ? t_begin + tiles_per_split : ntiles;
    const unsigned char* rbase = reinterpret_cast<const unsigned char*>(Q) + (size_t)row0 * pitch;

    const float kNegInf = -__builtin_inff(), kPosInf = __builtin_inff();
    // the rescan walks the list in groups of 8 (loads first, compares after): slots k .. kscan - 1 hold (+inf, -2), never the worst entry
    const int kscan = (k + 7) & ~7;
    if (tid < 128) {
        for (int j = 0; j < k; ++j) { cand_s[tid * LS + j] = kNegInf; cand_i[tid * LS + j] = kTopkSentinel - (split * KC + j); }
        for (int j = k; j < kscan; ++j) { cand_s[tid * LS + j] = kPosInf; cand_i[tid * LS + j] = -2; }
        worst_s[tid] = kNegInf; worst_i[tid] = kTopkSentinel - split * KC; worst_p[tid] = 0;
    }
    __syncthreads();

    KTileStage<128, 256> sp, sq, sp2, sq2;
    for (int t = t_begin; t < t_end; ++t) {
        const unsigned char* cbase = reinterpret_cast<const unsigned char*>(G) + (size_t)t * 128 * pitch;
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

        // selection epilogue.  Bit 16 qi + r of mask[pi] <-> the score acc[qi][pi][r] of gallery row col0 + 32 qi + frag_row(r, half).
        const int col0 = t * 128 + 64 * wc;
        const bool ragged = t * 128 + 128 > ng;
        unsigned mask[2];
#pragma unroll
        for (int pi = 0; pi < 2; ++pi) {
            const int p_t = 64 * wr + 32 * pi + l31;
            const float thr = worst_s[p_t];      // (as the previous tile's last phase left it: a barrier lies between)
            unsigned m = 0;
#pragma unroll
            for (int qi = 0; qi < 2; ++qi)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool in = !ragged || col0 + 32 * qi + frag_row(r, half) < ng;
                    if (acc[qi][pi][r] >= thr && in) m |= 1u << (16 * qi + r);
                }
            mask[pi] = row0 + p_t < nq ? m : 0u;      // (padding query rows keep their sentinels)
        }
        __syncthreads();      // (every owner of a row has read its threshold before the first of them moves it)
        const int my_phase = 2 * wc + half;
        for (int ph = 0; ph < 4; ++ph) {
            if (ph == my_phase) {
#pragma unroll
                for (int pi = 0; pi < 2; ++pi) {
                    unsigned m = mask[pi];
                    if (m == 0) continue;
                    const int p_t = 64 * wr + 32 * pi + l31;
                    float* ls = cand_s + p_t * LS;
                    int* li = cand_i + p_t * LS;
                    float w_s = worst_s[p_t];
                    int w_i = worst_i[p_t], w_p = worst_p[p_t];
                    while (m) {
                        const int bit = __builtin_ctz(m);
                        m &= m - 1;
                        float s = 0.f;       // acc[bit >> 4][pi][bit & 15] without a run-time register index
#pragma unroll
                        for (int e = 0; e < 32; ++e) s = bit == e ? acc[e >> 4][pi][e & 15] : s;
                        const int idx = col0 + 32 * (bit >> 4) + frag_row(bit & 15, half);
                        if (!topk_better(s, idx, w_s, w_i)) continue;
                        ls[w_p] = s;
                        li[w_p] = idx;
                        w_s = kPosInf; w_i = -1; w_p = 0;      // (better than every entry, not better than the filler)
                        for (int j0 = 0; j0 < kscan; j0 += 8) {
                            float a[8];
                            int b[8];
#pragma unroll
                            for (int u = 0; u < 8; ++u) { a[u] = ls[j0 + u]; b[u] = li[j0 + u]; }
#pragma unroll
                            for (int u = 0; u < 8; ++u)
                                if (topk_better(w_s, w_i, a[u], b[u])) { w_s = a[u]; w_i = b[u]; w_p = j0 + u; }
                        }
                    }
                    worst_s[p_t] = w_s; worst_i[p_t] = w_i; worst_p[p_t] = w_p;
                }
            }
            __syncthreads();
        }
    }
    // the split's lists, as they are (the merge orders them)
    for (int e = tid; e < 128 * k; e += 256) {
        const int r = e / k, j = e - r * k;
        const size_t o = ((size_t)split * nq_pad + row0 + r) * k + j;
        ws_scores[o] = cand_s[r * LS + j];
        ws_index[o] = cand_i[r * LS + j];
    }
}

// Merge: `lpr` lanes per query row (64: four rows per block; 256: one, for long lists).  The row's M = nsplit * k candidates (distinct indices, sentinels included) are ranked by counting --
// rank(c) = number of candidates better than c under the total order, a permutation of 0 .. M - 1 -- and the candidates of rank < k are written
// at their rank: sorted output, every slot written exactly once, no exchange between lanes.  M <= 1024: 4 row slots x 8 KiB = 32 KiB of LDS per block (5 blocks of a CU's 160 KiB).
__global__ void __launch_bounds__(256) topk_merge_kernel(const float* ws_scores, const int* ws_index, int nq, int nq_pad, int nsplit, int k,
                                                         int lpr, float* scores, int* index) {
    CROSSCLR_SHARED float ms[4][kTopkMaxCandidates];
    CROSSCLR_SHARED int mi[4][kTopkMaxCandidates];
    const int wave = threadIdx.x / lpr, lane = threadIdx.x - wave * lpr;      // (the row's slot in the block, the lane's place in the row)
    const int row = blockIdx.x * (256 / lpr) + wave;
    const int M = nsplit * k;
    if (row < nq)
        for (int c = lane; c < M; c += lpr) {
            const int sp = c / k, j = c - sp * k;
            const size_t o = ((size_t)sp * nq_pad + row) * k + j;
            ms[wave][c] = ws_scores[o];
            mi[wave][c] = ws_index[o];
        }
    __syncthreads();
    if (row >= nq) return;
    for (int c = lane; c < M; c += lpr) {
        const float s = ms[wave][c];
        const int i = mi[wave][c];
        int rank = 0;
        for (int m = 0; m < M; ++m) rank += topk_better(ms[wave][m], mi[wave][m], s, i) ? 1 : 0;
        if (rank < k) { scores[(size_t)row * k + rank] = s; index[(size_t)row * k + rank] = i; }
    }
}

}  // namespace crossclr
