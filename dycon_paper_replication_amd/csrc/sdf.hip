// Signed distance maps on the device: the reference's compute_sdf (code/utils/util.py:205-236), the per-sample normalised signed
// distance of the SASSNet / DTC family, for a batch of label volumes and without a host copy.
//
// The reference takes two scipy distance transforms per sample (to the background inside the mask, to the foreground outside it),
// scales each by its own maximum and zeroes skimage's inner boundary.  With both a foreground and a background voxel in the sample
// both minima are 0 and one of the two terms is 0 at every voxel, so the value is -posdis / max(posdis) inside and
// +negdis / max(negdis) outside, and scipy's distances are sqrt of an exact integer squared distance.  Here:
//
//   z pass      two maps per sample from the row's membership ballots: squared distance along z to the nearest background voxel
//               (to_bg) and to the nearest foreground voxel (to_fg); SURFACE_FAR when the row has none
//   y, x pass   the lower-envelope pass of csrc/surface_edt.h over all 2 S maps, one launch per axis
//   reduce      per sample: max to_bg over the foreground, max to_fg over the background, any-foreground and any-background flags;
//               unsigned atomicMax / atomicOr only, reduced per wave first: the same bits whatever the order
//   finalise    fp64: -(sqrt(d2) / sqrt(max)) inside, +(sqrt(d2) / sqrt(max)) outside, +0.0 where to_bg == 1 (the inner boundary of
//               connectivity 1: a foreground voxel with a background 6-neighbour INSIDE the volume; the faces of the volume make no
//               boundary, unlike the border rule of csrc/surface.hip), +0.0 for a sample without foreground, NaN for one without
//               background (the reference's 0 / 0)
//
// A voxel is foreground exactly when its to_fg is 0, so nothing after the z pass reads the labels again.
#include "common.h"
#include "surface_edt.h"

#define SDF_STAT_WORDS 4                          // per map: max to_bg over the foreground, max to_fg over the background, flags, spare
#define SDF_ANY_FG 1u
#define SDF_ANY_BG 2u

namespace {

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned wave_or_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

// squared distance from z = c * 64 + lane to the nearest set bit of the row's words (wave-uniform), SURFACE_FAR when there is none:
// a bit scan in the lane's own word and the closest end of every other non-empty word
template <int WORDS>
__device__ __forceinline__ int sdf_row_nearest(const unsigned long long (&word)[WORDS], int c, int lane) {
    constexpr int NONE = 1 << 14;
    const int z = c * 64 + lane;
    int best = NONE;
#pragma unroll
    for (int k = 0; k < WORDS; ++k) {
        const unsigned long long m = word[k];
        if (m) {                                             // wave-uniform
            int d = NONE;
            if (k < c) d = z - (k * 64 + 63 - __clzll((long long)m));
            else if (k > c) d = k * 64 + (__ffsll((unsigned long long)m) - 1) - z;
            else {
                const unsigned long long below = m & (~0ull >> (63 - lane)), above = m >> lane;
                if (below) d = lane - (63 - __clzll((long long)below));
                if (above) d = min(d, (int)__ffsll((unsigned long long)above) - 1);
            }
            best = min(best, d);
        }
    }
    return best < NONE ? best * best : SURFACE_FAR;
}

// One wave per row (x, y) of map blockIdx.y; lanes run along z.  The foreground and the background flags of the row are the wave's
// ballots, one 64-bit word per 64 z (at most 8 each); bits at z >= Z are clear in both.  No LDS, no barrier, no atomic.
template <typename T>
__global__ __launch_bounds__(256) void sdf_row_kernel(const T* __restrict__ vol, int n_cls, int cls_lo, int XY, int Z,
                                                      int* __restrict__ d2) {
    constexpr int WORDS = SURFACE_MAX_AXIS / 64;
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.y;
    const long long V = (long long)XY * Z;
    const long long want = cls_lo + s % n_cls;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= XY) return;                                   // the whole wave
    const T* __restrict__ p = vol + (long long)(s / n_cls) * V + (long long)row * Z;
    unsigned long long fg[WORDS], bg[WORDS];
#pragma unroll
    for (int c = 0; c < WORDS; ++c) {
        fg[c] = bg[c] = 0;
        if (c * 64 < Z) {
            const int z = c * 64 + lane;
            const bool in = z < Z;
            const bool m = in && (cls_lo ? (long long)p[z] == want : p[z] != 0);
            fg[c] = __ballot(m);
            bg[c] = __ballot(in && !m);
        }
    }
    int* __restrict__ to_bg = d2 + (long long)(2 * s) * V + (long long)row * Z;
    int* __restrict__ to_fg = to_bg + V;
#pragma unroll
    for (int c = 0; c < WORDS; ++c) {
        if (c * 64 < Z) {
            const int z = c * 64 + lane;
            const int b = sdf_row_nearest<WORDS>(bg, c, lane), f = sdf_row_nearest<WORDS>(fg, c, lane);
            if (z < Z) {
                to_bg[z] = b;
                to_fg[z] = f;
            }
        }
    }
}

// stats[s] = { max to_bg over the foreground voxels, max to_fg over the background voxels, SDF_ANY_FG | SDF_ANY_BG, 0 }, zeroed by
// the caller.  Maxima and ORs of unsigned integers: the order of the atomics does not show in the result.
__global__ __launch_bounds__(256) void sdf_reduce_kernel(const int* __restrict__ d2, long long V, unsigned* __restrict__ stats) {
    const int s = blockIdx.y;
    const int* __restrict__ to_bg = d2 + (long long)(2 * s) * V;
    const int* __restrict__ to_fg = to_bg + V;
    unsigned mx_in = 0, mx_out = 0, flags = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        const int f = to_fg[i];
        if (f == 0) {
            mx_in = max(mx_in, (unsigned)to_bg[i]);
            flags |= SDF_ANY_FG;
        } else {
            mx_out = max(mx_out, (unsigned)f);
            flags |= SDF_ANY_BG;
        }
    }
    mx_in = wave_max_u32(mx_in);
    mx_out = wave_max_u32(mx_out);
    flags = wave_or_u32(flags);
    if ((threadIdx.x & 63) == 0) {
        unsigned* __restrict__ st = stats + (long long)SDF_STAT_WORDS * s;
        if (mx_in) atomicMax(st + 0, mx_in);
        if (mx_out) atomicMax(st + 1, mx_out);
        if (flags) atomicOr(st + 2, flags);
    }
}

// One thread per voxel of map blockIdx.y; the value goes to the n_rep consecutive copies of the map in out (the channels of an output
// with a channel axis).  Two correctly rounded fp64 square roots and one correctly rounded division, nothing fused or reassociated;
// an fp32 output is that value rounded once.
template <typename O>
__global__ __launch_bounds__(256) void sdf_finalize_kernel(const int* __restrict__ d2, const unsigned* __restrict__ stats, long long V,
                                                           int n_rep, int normalize, O* __restrict__ out) {
    const int s = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const unsigned* __restrict__ st = stats + (long long)SDF_STAT_WORDS * s;
    const unsigned flags = st[2];
    double v;
    if (!(flags & SDF_ANY_FG)) v = 0.0;
    else if (!(flags & SDF_ANY_BG)) v = __longlong_as_double(0x7ff8000000000000ll);
    else {
        const int b = d2[(long long)(2 * s) * V + i], f = d2[(long long)(2 * s + 1) * V + i];
        if (f == 0) {
            if (b == 1) v = 0.0;
            else {
                const double r = sqrt((double)b);
                v = normalize ? -(r / sqrt((double)st[0])) : -r;
            }
        } else {
            const double r = sqrt((double)f);
            v = normalize ? r / sqrt((double)st[1]) : r;
        }
    }
    O* __restrict__ o = out + (long long)s * n_rep * V + i;
    for (int r = 0; r < n_rep; ++r) o[(long long)r * V] = (O)v;
}

}  // namespace

extern "C" size_t dycon_sdf_workspace(int S, int X, int Y, int Z) {
    if (S <= 0 || X <= 0 || Y <= 0 || Z <= 0) return 0;
    return (size_t)S * 2 * (size_t)X * Y * Z * sizeof(int) + (size_t)S * SDF_STAT_WORDS * sizeof(unsigned);
}

extern "C" int dycon_sdf(const void* labels, int label_bytes, int n_vol, int cls_lo, int n_cls, int X, int Y, int Z, int normalize,
                         int n_rep, int out_bytes, void* out, void* workspace, size_t ws_bytes, dycon_stream_t stream) {
    DYCON_REQUIRE(labels && out && workspace, "sdf: null pointer");
    DYCON_REQUIRE(label_bytes == 1 || label_bytes == 8, "sdf: labels must be uint8 or int64 (label_bytes = %d)", label_bytes);
    DYCON_REQUIRE(out_bytes == 4 || out_bytes == 8, "sdf: the output must be fp32 or fp64 (out_bytes = %d)", out_bytes);
    DYCON_REQUIRE(X >= 1 && X <= SURFACE_MAX_AXIS && Y >= 1 && Y <= SURFACE_MAX_AXIS && Z >= 1 && Z <= SURFACE_MAX_AXIS,
                  "sdf: volume %dx%dx%d (every axis 1..%d)", X, Y, Z, SURFACE_MAX_AXIS);
    DYCON_REQUIRE(n_vol >= 1 && n_cls >= 1 && cls_lo >= 0 && (cls_lo > 0 || n_cls == 1) && cls_lo + n_cls <= 256,
                  "sdf: bad class range (cls_lo = %d, n_cls = %d; cls_lo = 0 means voxel != 0 and takes n_cls = 1)", cls_lo, n_cls);
    DYCON_REQUIRE(n_rep >= 1, "sdf: n_rep = %d copies of each map (at least 1)", n_rep);
    const long long S = (long long)n_vol * n_cls;
    DYCON_REQUIRE(2 * S <= 65535, "sdf: %lld maps in one call (at most 32767)", S);
    DYCON_REQUIRE(ws_bytes >= dycon_sdf_workspace((int)S, X, Y, Z), "sdf: workspace of %zu bytes, %zu needed", ws_bytes,
                  dycon_sdf_workspace((int)S, X, Y, Z));
    hipStream_t st = (hipStream_t)stream;
    const long long V = (long long)X * Y * Z;
    int* d2 = (int*)workspace;
    unsigned* stats = (unsigned*)(d2 + 2 * S * V);
    if (hipMemsetAsync(stats, 0, (size_t)S * SDF_STAT_WORDS * sizeof(unsigned), st) != hipSuccess) {
        dycon_set_error("sdf: hipMemsetAsync failed");
        return DYCON_ERR_LAUNCH;
    }
    dim3 rows(cdiv(X * Y, 4), (int)S);
    if (label_bytes == 1) sdf_row_kernel<unsigned char><<<rows, 256, 0, st>>>((const unsigned char*)labels, n_cls, cls_lo, X * Y, Z, d2);
    else sdf_row_kernel<long long><<<rows, 256, 0, st>>>((const long long*)labels, n_cls, cls_lo, X * Y, Z, d2);
    if (Y > 1) surface_axis_pass(d2, V, Y, Z, X, (long long)Y * Z, Z, 2 * (int)S, st);      // lines along y at fixed x
    if (X > 1) surface_axis_pass(d2, V, X, (long long)Y * Z, Y, Z, Z, 2 * (int)S, st);      // lines along x at fixed y
    const long long blocks = (V + 256 * 16 - 1) / (256 * 16);                              // 16 voxels per thread, 256 workgroups at most
    sdf_reduce_kernel<<<dim3((int)(blocks > 256 ? 256 : blocks), (int)S), 256, 0, st>>>(d2, V, stats);
    dim3 vox(cdiv(V, 256), (int)S);
    if (out_bytes == 8) sdf_finalize_kernel<double><<<vox, 256, 0, st>>>(d2, stats, V, n_rep, normalize, (double*)out);
    else sdf_finalize_kernel<float><<<vox, 256, 0, st>>>(d2, stats, V, n_rep, normalize, (float*)out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}
