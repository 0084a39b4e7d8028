// crossclr_kernels_pairloss.h -- the gradient finish shared by the InfoNCE loss (crossclr_kernels_infonce.h) and the pairwise sigmoid loss
// (crossclr_kernels_sigmoid.h), which differ in it by one divisor.
//
//   pairloss_backward_finish_kernel slices -> gradient rows (normalize backward, grad_out, input dtype) and <x^_p, M_p> for dL/ds
#pragma once
#include "crossclr_kernels_generic.h"
#include "crossclr_kernels_pairids.h"

namespace crossclr {

// ---------------------------------------------------------------------------------------------
// Gradient finish, one wave per output row (grid-stride over the 2 b rows: 4 rows per block and round), like bwd_finish_kernel:
//   M_p = sum of the slices (fp32, slice order), x^_p = the caller's row times inv_norm (normalized) or as given, dot_p = <x^_p, M_p>,
//   g = s / divisor M_p, divisor = 2 B (InfoNCE) or B (sigmoid loss);  normalized: (g - x^ (x^ . g)) inv_norm (F.normalize's eps rule:
//   inv_norm = 1e12 rows take g inv_norm);  times grad_out, cast to the input dtype.  Row arithmetic in fp64.  gvideo or gtext may be NULL:
//   that gradient is not written.
//   dL/ds: since sum_q W[p][q] S[p][q] = <x^_p, M_p>, summed over the video rows and again over the text rows (each alone gives the whole
//   sum_ij W S), the block's grad_out * dot_p go to dscale_ws[1 + block] (fp64, fixed order); fwd_finish_reduce_kernel adds them up and
//   scales by the caller's 1 / (4 B) or 1 / (2 B).
//   Rows up to 1024 columns stay in registers between the dot product and the output pass; what lies beyond is formed twice.
// ---------------------------------------------------------------------------------------------
template <typename TIN>
__global__ void __launch_bounds__(256) pairloss_backward_finish_kernel(const float* gbuf, int nslices, const TIN* video, const TIN* text, long ldv,
                                                                       long ldt, int b, int bpad, int D, int Dpad, const float* inv_norm,
                                                                       int normalized, const float* logit_scale, double divisor,
                                                                       const double* grad_out, TIN* gvideo, TIN* gtext, long ldgv, long ldgt,
                                                                       double* dscale_ws) {
    CROSSCLR_SHARED double wave_dot[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t slice = (size_t)2 * bpad * Dpad;
    const double go = grad_out[0];
    const double sc = (double)logit_scale[0] / divisor;
    double dots = 0.0;
    for (int idx = blockIdx.x * 4 + wave; idx < 2 * b; idx += gridDim.x * 4) {
        const int mod = idx / b, i = idx - mod * b;
        const TIN* own = mod == 0 ? video + (size_t)i * ldv : text + (size_t)i * ldt;
        TIN* out = mod == 0 ? gvideo : gtext;
        if (out) out += (size_t)i * (mod == 0 ? ldgv : ldgt);
        const double io = normalized ? (double)inv_norm[mod * bpad + i] : 1.0;
        const bool project = normalized && io < 9.99e11;
        const float* grow = gbuf + ((size_t)mod * bpad + i) * Dpad;
        auto row4 = [&](int d, double (&m)[4], double (&xh)[4]) {
            f32x4 sum = *reinterpret_cast<const f32x4*>(grow + d);          // Dpad is a multiple of 64: aligned, in range
            for (int sl = 1; sl < nslices; ++sl) sum += *reinterpret_cast<const f32x4*>(grow + sl * slice + d);      // fixed order
            double x[4];
            row_load4(own, d, D, x);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m[j] = d + j < D ? (double)sum[j] : 0.0;
                xh[j] = x[j] * io;
            }
        };
        double mc[kRowCache][4], xc[kRowCache][4];
        double dot = 0.0;
#pragma unroll
        for (int k = 0; k < kRowCache; ++k) {
            const int d = 4 * lane + 256 * k;
            if (d < D) {
                row4(d, mc[k], xc[k]);
#pragma unroll
                for (int j = 0; j < 4; ++j) dot += xc[k][j] * mc[k][j];
            }
        }
        for (int d = 4 * lane + 256 * kRowCache; d < D; d += 256) {
            double m[4], xh[4];
            row4(d, m, xh);
#pragma unroll
            for (int j = 0; j < 4; ++j) dot += xh[j] * m[j];
        }
        dot = wave_sum_f64(dot);
        dots += dot * go;
        if (!out) continue;      // (wave-uniform)
        const double post = (normalized ? io : 1.0) * go;
        auto emit = [&](int d, const double (&m)[4], const double (&xh)[4]) {
            double v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = sc * (project ? m[j] - xh[j] * dot : m[j]) * post;
            row_store4(out, d, D, v);
        };
#pragma unroll
        for (int k = 0; k < kRowCache; ++k) {
            const int d = 4 * lane + 256 * k;
            if (d < D) emit(d, mc[k], xc[k]);
        }
        for (int d = 4 * lane + 256 * kRowCache; d < D; d += 256) {
            double m[4], xh[4];
            row4(d, m, xh);
            emit(d, m, xh);
        }
    }
    if (lane == 0) wave_dot[wave] = dots;
    __syncthreads();
    if (threadIdx.x == 0) dscale_ws[1 + blockIdx.x] = ((wave_dot[0] + wave_dot[1]) + wave_dot[2]) + wave_dot[3];
}

}  // namespace crossclr
