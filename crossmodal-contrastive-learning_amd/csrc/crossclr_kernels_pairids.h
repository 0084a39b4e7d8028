// crossclr_kernels_pairids.h -- pair_ids of the InfoNCE and the sigmoid loss (crossclr_pair_groups and the *_ids calls of
// include/crossclr.h): pair i of the batch belongs to item ids[i], and a pair (i, j), i != j, of ONE item is no negative -- it is left out
// of the loss and carries weight 0.  The B x B mask ids[i] == ids[j] is never formed: the epilogues of the tiled kernels evaluate it per
// entry from a length-B vector.
//
//   pair_groups_kernel    int64 ids [b] -> int32 group [bpad]: group[i] = the smallest j with ids[j] == ids[i] (all 64 bits compared);
//                         group[i] = i for the padding rows.  Two pairs share an item exactly when their groups are equal, so the hot
//                         kernels (the IDS instantiations of infonce_stats_kernel, infonce_backward_kernel, sigmoid_stats_kernel
//                         and sigmoid_backward_kernel) compare ONE dword per entry and hold one register per row where an int64 id takes
//                         two; the result depends on the partition the ids induce, not on how they are labelled; a padding row's group
//                         (>= b) is no valid row's, so padding needs no case of its own.
#pragma once
#include "crossclr_device.h"

namespace crossclr {

// The four tiled kernels end in a parameter pack: the group array where a kernel is instantiated with IDS, nothing where it is not (those
// instantiations keep the argument list and the code they had before there were ids).
__device__ __forceinline__ const int* group_of() { return nullptr; }
__device__ __forceinline__ const int* group_of(const int* group) { return group; }

// grid = bpad / 256, one output per thread.  Block k stages ids[256 c .. 256 c + 255] in LDS for c = 0 .. k (the ids at and below its
// own rows) and every thread scans the chunk upwards for the first entry equal to its own: O(B^2 / 2) compares, about 1e3 per lane and
// chunk pair at B = 8192, next to the 2 B^2 D of the product.  The loop count is block-uniform (the barriers); a thread's own entry ends
// its scan at the latest.
__global__ void __launch_bounds__(256) pair_groups_kernel(const long long* ids, int b, int bpad, int* group) {
    CROSSCLR_SHARED long long chunk[256];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const bool valid = i < b;
    const long long mine = valid ? ids[i] : 0;
    int g = i;
    for (int cb = 0; cb <= (int)blockIdx.x; ++cb) {
        const int j0 = cb * 256;
        chunk[tid] = j0 + tid < b ? ids[j0 + tid] : 0;
        __syncthreads();
        if (valid) {
            const int n = g - j0 < 256 ? g - j0 : 256;      // entries below the best match so far (all of them rows < b)
            for (int k = 0; k < n; ++k)
                if (chunk[k] == mine) {
                    g = j0 + k;
                    break;
                }
        }
        __syncthreads();
    }
    if (i < bpad) group[i] = g;
}

}  // namespace crossclr
