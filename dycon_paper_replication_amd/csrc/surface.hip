// Surface distances on the device for unit voxel spacing: the border voxels of two binary masks, the exact squared Euclidean distance
// transform of each border set in int32, and the histogram of the squared distances from every border voxel of one mask to the border
// of the other.  HD95 and ASD (medpy.metric.binary.hd95 / asd behind code/utils/test_3d_patch.py:496-508 and code/utils/metrics.py:
// 112-131) are read off the histograms in fp64 in a fixed order.
//
// Everything before the last square root is an integer, so the result does not depend on the grid or on the order of the atomics
// (unsigned int adds only); no floating-point atomic is used anywhere in this file.
//
//   border      b = m & ~erode6(m), a voxel outside the volume counting as background (scipy's border_value = 0)
//   z pass      squared distance to the nearest border voxel of the row, SURFACE_FAR when the row has none (bit scans of ballots)
//   y, x pass   out[l] = min_l' g[l'] + (l - l')^2 from a (line x 64 z) tile in LDS, the search pruned at (l - l')^2 >= best
//   histogram   a border voxel is a voxel whose own transform is 0
#include "common.h"
#include "surface_edt.h"

#define SURFACE_TILE_BINS 256
#define SURFACE_LDS_BINS 2048                     // squared distances below 45^2 are counted in LDS first
#define SURFACE_MAX_TILES 3072                    // 3 * 511^2 + 1 bins in tiles of 256

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

// One wave per row (x, y) of pair blockIdx.y; lanes run along z.  side 0 reads the prediction, side 1 the ground truth.  The border
// flags of the row are the wave's ballots, one 64-bit word per 64 z (at most 8): the nearest border voxel of a lane is a bit scan in
// its own word and the closest end of the nearest non-empty word on either side.  No LDS, no barrier, no atomic.
template <typename T>
__global__ __launch_bounds__(256) void surface_border_z_kernel(const T* __restrict__ vol, int n_cls, int cls_lo, int X, int Y, int Z,
                                                               int side, int* __restrict__ d2) {
    constexpr int WORDS = SURFACE_MAX_AXIS / 64, NONE = 1 << 14;
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.y;
    const long long V = (long long)X * Y * Z, plane = (long long)Y * Z;
    const long long want = cls_lo + s % n_cls;
    const T* __restrict__ p = vol + (long long)(s / n_cls) * V;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= X * Y) return;                                // the whole wave
    const int x = row / Y, y = row % Y;
    const long long r0 = (long long)row * Z;
    auto member = [&](long long i) { return cls_lo ? (long long)p[i] == want : p[i] != 0; };
    const bool xy_inner = x > 0 && x < X - 1 && y > 0 && y < Y - 1;
    unsigned long long word[WORDS];
#pragma unroll
    for (int c = 0; c < WORDS; ++c) {
        word[c] = 0;
        if (c * 64 < Z) {
            const int z = c * 64 + lane;
            bool b = false;
            if (z < Z && member(r0 + z)) {
                const long long i = r0 + z;
                const bool inner = xy_inner && z > 0 && z < Z - 1 && member(i - 1) && member(i + 1) && member(i - Z) &&
                                   member(i + Z) && member(i - plane) && member(i + plane);
                b = !inner;
            }
            word[c] = __ballot(b);
        }
    }
    int* __restrict__ out = d2 + (long long)(2 * s + side) * V + r0;
#pragma unroll
    for (int c = 0; c < WORDS; ++c) {
        if (c * 64 < Z) {
            const int z = c * 64 + lane;
            int best = NONE;
#pragma unroll
            for (int k = 0; k < WORDS; ++k) {
                const unsigned long long m = word[k];
                if (m) {                                     // wave-uniform
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
            if (z < Z) out[z] = best < NONE ? best * best : SURFACE_FAR;
        }
    }
}

// hist[s][0][d2_b] += 1 for the border voxels of a, hist[s][1][d2_a] += 1 for those of b, and nborder[s] += the border voxels of
// each (a voxel whose own transform is 0).  A direction whose target border is empty adds nothing: its distances are SURFACE_FAR or
// more, past every bin.  Most distances are short, so the first SURFACE_LDS_BINS bins of both directions are counted in LDS and each
// workgroup adds its non-zero cells to the global histogram once; bin 0 (the borders coincide) is summed per wave first.
__global__ __launch_bounds__(256) void surface_hist_kernel(const int* __restrict__ d2, long long V, int nbins,
                                                           unsigned* __restrict__ nborder, unsigned* __restrict__ hist) {
    __shared__ unsigned low[2][SURFACE_LDS_BINS];
    __shared__ unsigned nsrc[2];
    const int s = blockIdx.y;
    if (threadIdx.x < 2) nsrc[threadIdx.x] = 0;
    for (int i = threadIdx.x; i < 2 * SURFACE_LDS_BINS; i += 256) (&low[0][0])[i] = 0;
    __syncthreads();
    const int* __restrict__ da = d2 + (long long)(2 * s) * V;
    const int* __restrict__ db = da + V;
    unsigned* __restrict__ h0 = hist + (long long)(2 * s) * nbins;
    unsigned* __restrict__ h1 = h0 + nbins;
    unsigned z0 = 0, z1 = 0, na = 0, nb = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        const int a = da[i], b = db[i];
        na += a == 0;
        nb += b == 0;
        if (a == 0) {
            if (b == 0) ++z0;
            else if (b < SURFACE_LDS_BINS) atomicAdd(&low[0][b], 1u);
            else if (b < nbins) atomicAdd(h0 + b, 1u);
        }
        if (b == 0) {
            if (a == 0) ++z1;
            else if (a < SURFACE_LDS_BINS) atomicAdd(&low[1][a], 1u);
            else if (a < nbins) atomicAdd(h1 + a, 1u);
        }
    }
    z0 = wave_sum_u32(z0);
    z1 = wave_sum_u32(z1);
    na = wave_sum_u32(na);
    nb = wave_sum_u32(nb);
    if ((threadIdx.x & 63) == 0) {
        if (z0) atomicAdd(&low[0][0], z0);
        if (z1) atomicAdd(&low[1][0], z1);
        if (na) atomicAdd(&nsrc[0], na);
        if (nb) atomicAdd(&nsrc[1], nb);
    }
    __syncthreads();
    if (threadIdx.x < 2 && nsrc[threadIdx.x]) atomicAdd(nborder + 2 * s + threadIdx.x, nsrc[threadIdx.x]);
    for (int i = threadIdx.x; i < SURFACE_LDS_BINS && i < nbins; i += 256) {
        const unsigned c0 = low[0][i], c1 = low[1][i];
        if (c0) atomicAdd(h0 + i, c0);
        if (c1) atomicAdd(h1 + i, c1);
    }
}

// One workgroup per pair.  Bins ascending: thread t owns the bins t, t + 256, ...; its fp64 partial sums are added in thread order.
// The percentile is numpy's default ("linear") rule on the union of both directions, written as numpy evaluates it.
__global__ __launch_bounds__(256) void surface_metrics_kernel(const unsigned* __restrict__ hist, const unsigned* __restrict__ nborder,
                                                              int nbins, double q, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ unsigned tilecnt[SURFACE_MAX_TILES];
    __shared__ double part[2][256];
    const int s = blockIdx.x, t = threadIdx.x;
    const unsigned* __restrict__ h0 = hist + (long long)(2 * s) * nbins;
    const unsigned* __restrict__ h1 = h0 + nbins;
    const unsigned na = nborder[2 * s], nb = nborder[2 * s + 1];
    double* __restrict__ o = out + 5 * s;
    if (na == 0 || nb == 0) {
        if (t == 0) {
            o[0] = o[1] = o[2] = __longlong_as_double(0x7ff8000000000000ll);
            o[3] = (double)na;
            o[4] = (double)nb;
        }
        return;
    }
    const int ntiles = (nbins + SURFACE_TILE_BINS - 1) / SURFACE_TILE_BINS;
    for (int i = t; i < ntiles; i += 256) tilecnt[i] = 0;
    __syncthreads();
    double s0 = 0.0, s1 = 0.0;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int bin = tile * SURFACE_TILE_BINS + t;
        unsigned c0 = 0, c1 = 0;
        if (bin < nbins) { c0 = h0[bin]; c1 = h1[bin]; }
        if (c0 | c1) {
            const double r = sqrt((double)bin);
            s0 += (double)c0 * r;
            s1 += (double)c1 * r;
        }
        const unsigned c = wave_sum_u32(c0 + c1);
        if ((t & 63) == 0 && c) atomicAdd(tilecnt + tile, c);
    }
    part[0][t] = s0;
    part[1][t] = s1;
    __syncthreads();
    if (t != 0) return;
    double sum0 = 0.0, sum1 = 0.0;
    for (int i = 0; i < 256; ++i) { sum0 += part[0][i]; sum1 += part[1][i]; }
    // np.percentile(x, q): virtual index (n - 1) * p with p = q / 100, neighbours floor and floor + 1
    const long long n = (long long)na + (long long)nb;
    const double p = q / 100.0;
    const double vi = (double)(n - 1) * p;
    const double fl = floor(vi);
    const double gamma = vi - fl;
    long long lo = (long long)fl, hi = lo + 1;
    if (vi >= (double)(n - 1)) lo = hi = n - 1;
    if (vi < 0.0) lo = hi = 0;
    // order statistics lo <= hi (0-based) of the union.  seen = the elements in the bins below `bin`; a whole tile is stepped over
    // while it ends at or below the rank, then single bins.  The walk never leaves [0, nbins - 1].
    long long seen = 0;
    int bin = 0;
    double v[2];
    for (int k = 0; k < 2; ++k) {
        const long long rank = k ? hi : lo;
        while (bin < nbins - 1) {
            if (bin % SURFACE_TILE_BINS == 0 && bin + SURFACE_TILE_BINS < nbins) {
                const long long c = tilecnt[bin / SURFACE_TILE_BINS];
                if (seen + c <= rank) { seen += c; bin += SURFACE_TILE_BINS; continue; }
            }
            const long long c = (long long)h0[bin] + h1[bin];
            if (seen + c > rank) break;
            seen += c;
            ++bin;
        }
        v[k] = sqrt((double)bin);
    }
    const double diff = v[1] - v[0];
    double r = v[0] + diff * gamma;
    if (gamma >= 0.5) r = v[1] - diff * (1.0 - gamma);
    o[0] = r;
    o[1] = sum0 / (double)na;
    o[2] = sum1 / (double)nb;
    o[3] = (double)na;
    o[4] = (double)nb;
}

static int surface_nbins(int X, int Y, int Z) { return (X - 1) * (X - 1) + (Y - 1) * (Y - 1) + (Z - 1) * (Z - 1) + 1; }

extern "C" size_t dycon_surface_workspace(int S, int X, int Y, int Z) {
    if (S <= 0 || X <= 0 || Y <= 0 || Z <= 0) return 0;
    return (size_t)S * 2 * (size_t)X * Y * Z * sizeof(int);
}

extern "C" int dycon_surface_hist(const void* a, int a_bytes, const void* b, int b_bytes, int n_vol, int cls_lo, int n_cls, int X, int Y,
                                  int Z, unsigned int* hist, unsigned int* nborder, void* workspace, size_t ws_bytes,
                                  dycon_stream_t stream) {
    DYCON_REQUIRE(a && b && hist && nborder && workspace, "surface_hist: null pointer");
    DYCON_REQUIRE(a_bytes == 1, "surface_hist: the prediction must be uint8 (a_bytes = %d)", a_bytes);
    DYCON_REQUIRE(b_bytes == 1 || b_bytes == 8, "surface_hist: ground truth must be uint8 or int64 (b_bytes = %d)", b_bytes);
    DYCON_REQUIRE(X >= 1 && X <= SURFACE_MAX_AXIS && Y >= 1 && Y <= SURFACE_MAX_AXIS && Z >= 1 && Z <= SURFACE_MAX_AXIS,
                  "surface_hist: volume %dx%dx%d (every axis 1..%d)", X, Y, Z, SURFACE_MAX_AXIS);
    DYCON_REQUIRE(n_vol >= 1 && n_cls >= 1 && cls_lo >= 0 && (cls_lo > 0 || n_cls == 1) && cls_lo + n_cls <= 256,
                  "surface_hist: bad class range (cls_lo = %d, n_cls = %d; cls_lo = 0 means voxel != 0 and takes n_cls = 1)", cls_lo,
                  n_cls);
    const long long S = (long long)n_vol * n_cls;
    DYCON_REQUIRE(2 * S <= 65535, "surface_hist: %lld pairs in one call (at most 32767)", S);
    DYCON_REQUIRE(ws_bytes >= dycon_surface_workspace((int)S, X, Y, Z), "surface_hist: workspace of %zu bytes, %zu needed", ws_bytes,
                  dycon_surface_workspace((int)S, X, Y, Z));
    hipStream_t st = (hipStream_t)stream;
    const long long V = (long long)X * Y * Z;
    const int nbins = surface_nbins(X, Y, Z);
    int* d2 = (int*)workspace;
    if (hipMemsetAsync(hist, 0, (size_t)S * 2 * nbins * sizeof(unsigned), st) != hipSuccess ||
        hipMemsetAsync(nborder, 0, (size_t)S * 2 * sizeof(unsigned), st) != hipSuccess) {
        dycon_set_error("surface_hist: hipMemsetAsync failed");
        return DYCON_ERR_LAUNCH;
    }
    dim3 rows(cdiv(X * Y, 4), (int)S);
    surface_border_z_kernel<unsigned char><<<rows, 256, 0, st>>>((const unsigned char*)a, n_cls, cls_lo, X, Y, Z, 0, d2);
    if (b_bytes == 1)
        surface_border_z_kernel<unsigned char><<<rows, 256, 0, st>>>((const unsigned char*)b, n_cls, cls_lo, X, Y, Z, 1, d2);
    else
        surface_border_z_kernel<long long><<<rows, 256, 0, st>>>((const long long*)b, n_cls, cls_lo, X, Y, Z, 1, d2);
    if (Y > 1) surface_axis_pass(d2, V, Y, Z, X, (long long)Y * Z, Z, 2 * (int)S, st);  // lines along y at fixed x
    if (X > 1) surface_axis_pass(d2, V, X, (long long)Y * Z, Y, Z, Z, 2 * (int)S, st);  // lines along x at fixed y
    const long long blocks = (V + 256 * 16 - 1) / (256 * 16);                              // 16 voxels per thread, 256 workgroups at most
    surface_hist_kernel<<<dim3((int)(blocks > 256 ? 256 : blocks), (int)S), 256, 0, st>>>(d2, V, nbins, nborder, hist);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_surface_metrics(const unsigned int* hist, const unsigned int* nborder, int S, int nbins, double q, double* out,
                                     dycon_stream_t stream) {
    DYCON_REQUIRE(hist && nborder && out, "surface_metrics: null pointer");
    DYCON_REQUIRE(S >= 1 && nbins >= 1 && nbins <= SURFACE_MAX_TILES * SURFACE_TILE_BINS, "surface_metrics: S = %d, nbins = %d (1..%d)",
                  S, nbins, SURFACE_MAX_TILES * SURFACE_TILE_BINS);
    DYCON_REQUIRE(q >= 0.0 && q <= 100.0, "surface_metrics: percentile %g outside [0, 100]", q);
    surface_metrics_kernel<<<S, 256, 0, (hipStream_t)stream>>>(hist, nborder, nbins, q, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}
