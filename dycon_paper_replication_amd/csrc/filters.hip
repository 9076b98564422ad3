// scipy.ndimage.gaussian_filter of fp32 volumes on the device (utils/filters.py), bit for bit.
//
// scipy filters one axis after the other (0, 1, 2), stores every intermediate in the output's type (fp32 here) and, because a
// Gaussian kernel is symmetric, sums a line in its symmetric form (ni_filters.c, NI_Correlate1D), all in fp64:
//     acc = x[c] * w[r];   for ii = -r .. -1:  acc += (x[c + ii] + x[c - ii]) * w[ii + r];   out = (float)acc
// with the line extended by the boundary mode (reflect: d c b a | a b c d | d c b a, as often as the radius asks; constant: zeros;
// nearest: the edge value).  One operation, one rounding: the file is built with -ffp-contract=off and says so itself below.
//
// A pass is laid out as a bandwidth kernel: every voxel is read once from HBM (the halo re-reads of neighbouring tiles hit the L2) and written
// once.  Along z (the contiguous axis) a block stages its rows with their halo in LDS and every thread owns one output.  Along x
// and y the lanes stay along the contiguous extent (y * z for the x pass, z for the y pass), so global accesses are coalesced, and
// a block stages a slab of CH + 2 r lines of 64 lanes in LDS, from which every thread slides along the filtered axis.  The weights
// w[0 .. r] travel in the kernel arguments.  First version, correct and not tuned: the 2 r + 1 fp64
// taps per voxel, not the bytes, set its time (0.17 - 0.27 of a device copy at r = 8, 0.04 - 0.08 at r = 44: profiles/warp_micro.txt).
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

struct Weights {
    double w[DYCON_GAUSS_RMAX + 1];      // w[0 .. r]: the left half and the centre of the 2 r + 1 symmetric weights
};

// index of element i of a line of n extended by `mode`; -1: the constant 0
__device__ __forceinline__ int extend(int i, int n, int mode) {
    if ((unsigned)i < (unsigned)n) return i;
    if (mode == DYCON_FILTER_CONSTANT) return -1;
    if (mode == DYCON_FILTER_NEAREST) return i < 0 ? 0 : n - 1;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// scipy's symmetric sum around s[c * stride] of an extended line held in LDS
__device__ __forceinline__ float line_sum(const float* s, int c, int stride, int r, const Weights& wt, float scale) {
    double acc = (double)s[c * stride] * wt.w[r];
    for (int ii = -r; ii < 0; ++ii) acc += ((double)s[(c + ii) * stride] + (double)s[(c - ii) * stride]) * wt.w[ii + r];
    return (float)acc * scale;
}

constexpr int ROW_LDS = 8 * (32 + 2 * DYCON_GAUSS_RMAX);      // floats: the largest RPB * (TZ + 2 r), reached at TZ = 32

// the pass along the contiguous axis: `rows` lines of Z elements.  A block owns RPB rows x TZ outputs (RPB * TZ <= 256).
__global__ __launch_bounds__(256) void gauss_row_kernel(const float* __restrict__ in, float* __restrict__ out, long long rows, int Z,
                                                        int TZ, int RPB, int ztiles, int r, int mode, float scale, Weights wt) {
    __shared__ float s[ROW_LDS];
    const int W = TZ + 2 * r;
    const long long nblk = (rows + RPB - 1) / RPB * ztiles;
    for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int zt = (int)(blk % ztiles);
        const long long row0 = blk / ztiles * RPB;
        const int z0 = zt * TZ;
        __syncthreads();                                           // the previous tile has been read
        for (int e = threadIdx.x; e < RPB * W; e += 256) {
            const int rr = e / W, q = e - rr * W;
            float v = 0.f;
            if (row0 + rr < rows) {
                const int zi = extend(z0 - r + q, Z, mode);
                if (zi >= 0) v = in[(row0 + rr) * Z + zi];
            }
            s[e] = v;
        }
        __syncthreads();
        const int rr = threadIdx.x / TZ, q = threadIdx.x - rr * TZ;
        if (rr < RPB && row0 + rr < rows && z0 + q < Z) out[(row0 + rr) * Z + z0 + q] = line_sum(s + rr * W, q + r, 1, r, wt, scale);
    }
}

// a pass along a strided axis: `outer` slabs of L lines of `inner` contiguous elements, filtered along L.  A block owns CH lines
// x 64 lanes of one slab: thread (lane, g) of 64 x 4 computes lines g, g + 4, ... of the chunk.  LDS: (CH + 2 r) x 64 floats.
__global__ __launch_bounds__(256) void gauss_col_kernel(const float* __restrict__ in, float* __restrict__ out, long long outer, int L,
                                                        long long inner, int CH, int chunks, long long itiles, int r, int mode,
                                                        float scale, Weights wt) {
    extern __shared__ __align__(16) float sc[];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int H = CH + 2 * r;
    const long long nblk = outer * chunks * itiles;
    for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const long long it = blk % itiles;
        const int ch = (int)(blk / itiles % chunks);
        const long long o = blk / itiles / chunks;
        const long long i0 = it * 64 + lane;
        const int l0 = ch * CH;
        const float* src = in + o * L * inner;
        __syncthreads();
        for (int h = g; h < H; h += 4) {
            float v = 0.f;
            if (i0 < inner) {
                const int li = extend(l0 - r + h, L, mode);
                if (li >= 0) v = src[li * inner + i0];
            }
            sc[h * 64 + lane] = v;
        }
        __syncthreads();
        if (i0 < inner) {
            float* dst = out + o * L * inner + i0;
            for (int c = g; c < CH && l0 + c < L; c += 4) dst[(l0 + c) * inner] = line_sum(sc + lane, c + r, 64, r, wt, scale);
        }
    }
}

int count_axes(const double* w0, const double* w1, const double* w2) { return (w0 != nullptr) + (w1 != nullptr) + (w2 != nullptr); }

}  // namespace

extern "C" size_t dycon_gaussian_filter_workspace(int N, int X, int Y, int Z, int naxes, int inplace) {
    if (N <= 0 || X <= 0 || Y <= 0 || Z <= 0 || naxes < 0 || naxes > 3) return 0;
    const size_t bytes = (size_t)N * X * Y * Z * sizeof(float);
    if (inplace) return naxes == 0 ? 0 : naxes == 3 ? 2 * bytes : bytes;
    return naxes >= 2 ? bytes : 0;
}

extern "C" int dycon_gaussian_filter(const float* in, float* out, int N, int X, int Y, int Z, const double* w0, int r0,
                                     const double* w1, int r1, const double* w2, int r2, int mode, float scale, void* workspace,
                                     size_t ws_bytes, dycon_stream_t stream) {
    DYCON_REQUIRE(in && out, "gaussian_filter: null pointer");
    DYCON_REQUIRE(N > 0 && X > 0 && Y > 0 && Z > 0, "gaussian_filter: %d volumes of %d x %d x %d", N, X, Y, Z);
    DYCON_REQUIRE((long long)N * X * Y * Z <= 0x7fffffffLL * 64, "gaussian_filter: too many voxels");
    DYCON_REQUIRE(mode == DYCON_FILTER_REFLECT || mode == DYCON_FILTER_CONSTANT || mode == DYCON_FILTER_NEAREST,
                  "gaussian_filter: mode %d is not reflect (0), constant (1) or nearest (2)", mode);
    DYCON_REQUIRE((uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)workspace % 4 == 0, "gaussian_filter: misaligned pointer");
    const double* ws_[3] = {w0, w1, w2};
    const int rs[3] = {r0, r1, r2};
    const int dims[3] = {X, Y, Z};
    Weights wt[3];
    memset(wt, 0, sizeof(wt));
    for (int a = 0; a < 3; ++a) {
        if (!ws_[a]) continue;
        DYCON_REQUIRE(rs[a] >= 0 && rs[a] <= DYCON_GAUSS_RMAX, "gaussian_filter: axis %d: radius %d is not in 0..%d (DYCON_GAUSS_RMAX)", a,
                      rs[a], DYCON_GAUSS_RMAX);
        for (int i = 0; i <= rs[a]; ++i) {
            DYCON_REQUIRE(isfinite(ws_[a][i]) && ws_[a][i] == ws_[a][2 * rs[a] - i],
                          "gaussian_filter: axis %d: the %d weights are not finite and symmetric", a, 2 * rs[a] + 1);
            wt[a].w[i] = ws_[a][i];
        }
    }
    const int naxes = count_axes(w0, w1, w2);
    const size_t bytes = (size_t)N * X * Y * Z * sizeof(float);
    const bool inplace = in == out;
    DYCON_REQUIRE(inplace || (uintptr_t)in + bytes <= (uintptr_t)out || (uintptr_t)out + bytes <= (uintptr_t)in,
                  "gaussian_filter: the output overlaps the input without being the input");
    const size_t need = dycon_gaussian_filter_workspace(N, X, Y, Z, naxes, inplace);
    DYCON_REQUIRE(need == 0 || (workspace && ws_bytes >= need), "gaussian_filter: the workspace holds %zu bytes, %zu needed", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    float* wa = (float*)workspace;
    float* wb = wa + (size_t)N * X * Y * Z;
    // the buffer each pass writes; the last one is `out`, and no pass reads what it writes
    float* dst[3] = {out, out, out};
    bool copy_back = false;
    if (inplace) {
        if (naxes == 1) dst[0] = wa, copy_back = true;
        else if (naxes == 2) dst[0] = wa;
        else if (naxes == 3) dst[0] = wa, dst[1] = wb;
    } else if (naxes == 2) dst[0] = wa;
    else if (naxes == 3) dst[1] = wa;
    if (naxes == 0) {
        DYCON_REQUIRE(scale == 1.f, "gaussian_filter: a scale needs at least one filtered axis");
        if (!inplace && hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            dycon_set_error("gaussian_filter: the copy failed");
            return DYCON_ERR_LAUNCH;
        }
        return DYCON_OK;
    }
    const float* cur = in;
    int pass = 0;
    for (int a = 0; a < 3; ++a) {
        if (!ws_[a]) continue;
        float* to = dst[pass];
        const float sc = pass == naxes - 1 ? scale : 1.f;          // the scale multiplies the fp32 result of the last pass
        const int r = rs[a], L = dims[a];
        if (a == 2) {
            const long long rows = (long long)N * X * Y;
            const int TZ = Z >= 128 ? 128 : (Z + 31) / 32 * 32, RPB = 256 / TZ, ztiles = (Z + TZ - 1) / TZ;
            const long long nblk = (rows + RPB - 1) / RPB * ztiles;
            gauss_row_kernel<<<(unsigned)(nblk > 0x7fffffffLL ? 0x7fffffffLL : nblk), 256, 0, st>>>(cur, to, rows, Z, TZ, RPB, ztiles, r,
                                                                                                    mode, sc, wt[a]);
        } else {
            const long long outer = a == 0 ? N : (long long)N * X, inner = a == 0 ? (long long)Y * Z : Z;
            const int CH = r <= 16 ? 32 : 64, chunks = (L + CH - 1) / CH;
            const long long itiles = (inner + 63) / 64, nblk = outer * chunks * itiles;
            const size_t lds = (size_t)(CH + 2 * r) * 64 * sizeof(float);      // at most 192 lines: 48 KiB
            gauss_col_kernel<<<(unsigned)(nblk > 0x7fffffffLL ? 0x7fffffffLL : nblk), 256, lds, st>>>(cur, to, outer, L, inner, CH, chunks,
                                                                                                      itiles, r, mode, sc, wt[a]);
        }
        DYCON_LAUNCH_CHECK();
        cur = to;
        ++pass;
    }
    if (copy_back && hipMemcpyAsync(out, wa, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        dycon_set_error("gaussian_filter: the copy failed");
        return DYCON_ERR_LAUNCH;
    }
    return DYCON_OK;
}
