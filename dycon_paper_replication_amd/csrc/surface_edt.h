// The y and x passes of the exact int32 squared Euclidean distance transform, shared by csrc/surface.hip (distance to the border of a
// mask) and csrc/sdf.hip (distance to the background and to the foreground).  The z pass is each file's own: it decides what a seed is.
#pragma once
#include "common.h"

#define SURFACE_FAR (1 << 29)                     // + 2 * 511^2 stays below 2^31
#define SURFACE_MAX_AXIS 512

namespace {                                       // a copy per translation unit: each registers its own code object

// In place along one of the two outer axes: blockIdx.z picks the volume of d2, blockIdx.y the index along the other outer axis,
// blockIdx.x the 64-wide z tile.  The whole (L x 64) tile is in LDS before anything is written back.
template <int LMAX>
__global__ __launch_bounds__(256) void surface_axis_pass_kernel(int* __restrict__ d2, long long V, int L, long long line_stride,
                                                                long long other_stride, int Z) {
    __shared__ int tile[LMAX][64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int z = blockIdx.x * 64 + lane;
    const bool live = z < Z;
    int* __restrict__ base = d2 + (long long)blockIdx.z * V + (long long)blockIdx.y * other_stride + z;
    for (int l = w; l < L; l += 4) tile[l][lane] = live ? base[l * line_stride] : SURFACE_FAR;
    __syncthreads();
    if (!live) return;
    for (int l = w; l < L; l += 4) {
        int best = tile[l][lane];
        const int reach = max(l, L - 1 - l);
        // four distances per trip, so that eight independent LDS reads are in flight; a candidate past the pruning bound cannot win
        for (int d = 1; d <= reach && d * d < best; d += 4) {
            int cand = best;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = d + j, ee = e * e, lo = l - e, hi = l + e;
                const int below = tile[max(lo, 0)][lane], above = tile[min(hi, L - 1)][lane];
                cand = min(cand, min(lo >= 0 ? below + ee : SURFACE_FAR, hi < L ? above + ee : SURFACE_FAR));
            }
            best = cand;
        }
        base[l * line_stride] = best;
    }
}

// n_maps int32 volumes of V voxels each, one after the other in d2, all transformed along one axis in one launch
static void surface_axis_pass(int* d2, long long V, int L, long long line_stride, int n_other, long long other_stride, int Z, int n_maps,
                              hipStream_t stream) {
    dim3 grid(cdiv(Z, 64), n_other, n_maps);
    if (L <= 128) surface_axis_pass_kernel<128><<<grid, 256, 0, stream>>>(d2, V, L, line_stride, other_stride, Z);
    else if (L <= 256) surface_axis_pass_kernel<256><<<grid, 256, 0, stream>>>(d2, V, L, line_stride, other_stride, Z);
    else surface_axis_pass_kernel<SURFACE_MAX_AXIS><<<grid, 256, 0, stream>>>(d2, V, L, line_stride, other_stride, Z);
}

}  // namespace
