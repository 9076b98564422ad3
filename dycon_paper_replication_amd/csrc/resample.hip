// Preprocessing on the device: the reference's normalize_image (code/BraTS19_DataPreprocessing.py:8-31,
// code/ISLES22_DataPreprocessing.py:10-33) and the scipy.ndimage.zoom calls of its two case functions
// (BraTS19_DataPreprocessing.py:189-198, ISLES22_DataPreprocessing.py:147-159), for a batch of volumes and without a host copy.
//
//   stats       per sample, three launches: (1) per-workgroup fp64 partial sums of the voxels > 0, their count, the extremes and the
//               "any voxel <= 0" flag; (2) every workgroup folds the partials of (1) in index order into the same mean and adds up
//               its centred squares; (3) one workgroup per sample folds those, takes the square root and writes the statistics and
//               the record normalize_image needs.  Sums: a fixed order (thread, wave tree, waves in order; the partials likewise:
//               thread t adds partials t, t + 256, ... in index order, then the same tree).
//               Counts, flags and extremes: integer atomicAdd / atomicOr / atomicMax on bit patterns.  No floating-point atomic:
//               the same bits on every run, whatever the alignment of the input.
//   zoom        a small launch writes the per-axis tables (source index per output index for order 0; two indices and two fp64
//               weights for order 1) from c = double(i) * step, step = double(n_in - 1) / double(n_out - 1) divided on the host;
//               the main kernel gathers: four consecutive z outputs per thread, one 16-byte store (4-byte for uint8) where the
//               output allows it.  A normalisation record is applied to every tap value on load, in fp32.
//
// Everything here must round as numpy and scipy do: one operation, one rounding.  hipcc contracts a * b + c into an FMA by
// default for device code; the pragma below switches that off for the whole file (the Makefile passes -ffp-contract=off for it
// as well).  fp32 divisions and the fp64 square root are the correctly rounded ones (hipcc's default).
#include "common.h"

#pragma clang fp contract(off)

#define RS_THREADS 256
#define RS_MAX_GROUPS 1024                        // workgroups per sample of the statistics passes
#define RS_GROUP_VOXELS 4096                      // voxels per workgroup before a second one is worth its launch
#define RS_HEAD_WORDS 8                           // per sample: n_pos (2 words), ~min_pos, max_pos, ~min_all, max_all, any <= 0, spare

namespace {

struct NormRec {                                  // dycon_norm_record_t by value
    int apply_z;
    float mean, std;
    int apply_mm;
    float lo, hi;
};

// the reference's two fp32 expressions (BraTS19_DataPreprocessing.py:22, :29), each operation rounded on its own
__device__ __forceinline__ float norm_value(float x, const NormRec& r, float span) {
    if (r.apply_z) x = x > 0.f ? (x - r.mean) / r.std : 0.f;
    if (r.apply_mm) x = (x - r.lo) / span;
    return x;
}

// unsigned key with the order of the floats (-0.0 below +0.0), and back
__device__ __forceinline__ unsigned float_key(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ unsigned wave_max_u(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the workgroup's sum in thread 0: wave trees, then the four waves in order
__device__ __forceinline__ double group_sum_d(double v, double* smem) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < RS_THREADS / 64; ++w) r += smem[w];
    __syncthreads();
    return r;
}

// voxels 4 q .. 4 q + 3 of a sample (fewer at the end); one 16-byte load when the sample allows it, the same values otherwise
__device__ __forceinline__ int load_quad(const float* __restrict__ p, long long q, long long V, bool vec, float (&v)[4]) {
    const long long i = 4 * q;
    if (vec) {
        const float4 f = *reinterpret_cast<const float4*>(p + i);
        v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        return 4;
    }
    const int n = (int)min(4ll, V - i);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < n ? p[i + k] : 0.f;
    return n;
}

// the sum of a sample's G partials, the same bits in every thread of every workgroup that asks: thread t adds p[t], p[t + 256], ...
// in index order, then the workgroup's tree; one load per thread and step, no serial chain of G loads
__device__ __forceinline__ double fold_partials(const double* __restrict__ p, int G, double* smem) {
    double v = 0.0;
    for (int g = threadIdx.x; g < G; g += RS_THREADS) v += p[g];
    const double s = group_sum_d(v, smem);
    if (threadIdx.x == 0) smem[RS_THREADS / 64] = s;
    __syncthreads();
    const double r = smem[RS_THREADS / 64];
    __syncthreads();
    return r;
}

// the voxels of up to four quads of a thread's stride loop, loaded before any is used (four loads in flight); n[j]: voxels of quad j
struct QuadBlock {
    float v[4][4];
    int n[4];
};
__device__ __forceinline__ void load_block(const float* __restrict__ p, long long q, long long stride, long long Q, long long V, bool vec,
                                           QuadBlock& b) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long qj = q + j * stride;
        b.n[j] = qj < Q ? load_quad(p, qj, V, vec, b.v[j]) : 0;
    }
}

// pass 1.  grid (G, B).  head: RS_HEAD_WORDS zeroed words per sample; part: B x 2 x G doubles
__global__ __launch_bounds__(RS_THREADS) void stats_sum_kernel(const float* __restrict__ x, long long V, unsigned* __restrict__ head,
                                                               double* __restrict__ part) {
    __shared__ double smem[RS_THREADS / 64 + 1];
    const int b = blockIdx.y, G = gridDim.x;
    const float* __restrict__ p = x + (long long)b * V;
    const bool vec = (V & 3) == 0 && ((uintptr_t)p & 15) == 0;
    const long long Q = (V + 3) >> 2;
    double sum = 0.0;
    unsigned long long n = 0;
    unsigned inv_min_pos = 0, max_pos = 0, inv_min_all = 0, max_all = 0, nonpos = 0;
    const long long stride = (long long)G * RS_THREADS;
    for (long long q = (long long)blockIdx.x * RS_THREADS + threadIdx.x; q < Q; q += 4 * stride) {
        QuadBlock blk;
        load_block(p, q, stride, Q, V, vec, blk);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {                             // quad by quad, voxel by voxel: the order of the sum
                if (k >= blk.n[j]) continue;
                const float v = blk.v[j][k];
                const unsigned key = float_key(v);
                inv_min_all = max(inv_min_all, ~key);
                max_all = max(max_all, key);
                if (v > 0.f) {
                    sum += (double)v;
                    ++n;
                    const unsigned bits = __float_as_uint(v);         // positive floats order as their bit patterns
                    inv_min_pos = max(inv_min_pos, ~bits);
                    max_pos = max(max_pos, bits);
                } else nonpos = 1;
            }
    }
    const double s = group_sum_d(sum, smem);
    inv_min_pos = wave_max_u(inv_min_pos), max_pos = wave_max_u(max_pos);
    inv_min_all = wave_max_u(inv_min_all), max_all = wave_max_u(max_all);
    nonpos = wave_max_u(nonpos);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += (unsigned long long)__shfl_xor((long long)n, o, 64);
    // one set of atomics per workgroup, and none that could not change the word: thousands of atomics on one cache line cost more
    // than both passes over the volume.  The word read first may be stale; it only grows, so a stale read costs an atomic, no more
    __shared__ unsigned su[RS_THREADS / 64][5];
    __shared__ unsigned long long sn[RS_THREADS / 64];
    if ((threadIdx.x & 63) == 0) {
        unsigned* w = su[threadIdx.x >> 6];
        w[0] = inv_min_pos, w[1] = max_pos, w[2] = inv_min_all, w[3] = max_all, w[4] = nonpos;
        sn[threadIdx.x >> 6] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned u[5] = {0, 0, 0, 0, 0};
        unsigned long long nb = 0;
        for (int w = 0; w < RS_THREADS / 64; ++w) {
            nb += sn[w];
#pragma unroll
            for (int k = 0; k < 5; ++k) u[k] = max(u[k], su[w][k]);
        }
        unsigned* h = head + (long long)RS_HEAD_WORDS * b;
        const volatile unsigned* seen = h;
        if (nb) atomicAdd(reinterpret_cast<unsigned long long*>(h), nb);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (u[k] > seen[2 + k]) atomicMax(h + 2 + k, u[k]);
        if (u[4] && !seen[6]) atomicOr(h + 6, 1u);
        part[((long long)b * 2 + 0) * G + blockIdx.x] = s;
    }
}

// pass 2: the mean from pass 1's partials (every thread folds them in the same order: the same mean everywhere), then the centred squares
__global__ __launch_bounds__(RS_THREADS) void stats_sq_kernel(const float* __restrict__ x, long long V, const unsigned* __restrict__ head,
                                                              double* __restrict__ part) {
    __shared__ double smem[RS_THREADS / 64 + 1];
    const int b = blockIdx.y, G = gridDim.x;
    const unsigned long long n = *reinterpret_cast<const unsigned long long*>(head + (long long)RS_HEAD_WORDS * b);
    double sq = 0.0;
    if (n) {                                                          // uniform over the sample
        const double mean = fold_partials(part + ((long long)b * 2 + 0) * G, G, smem) / (double)n;
        const float* __restrict__ p = x + (long long)b * V;
        const bool vec = (V & 3) == 0 && ((uintptr_t)p & 15) == 0;
        const long long Q = (V + 3) >> 2, stride = (long long)G * RS_THREADS;
        for (long long q = (long long)blockIdx.x * RS_THREADS + threadIdx.x; q < Q; q += 4 * stride) {
            QuadBlock blk;
            load_block(p, q, stride, Q, V, vec, blk);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < blk.n[j] && blk.v[j][k] > 0.f) {
                        const double d = (double)blk.v[j][k] - mean;
                        sq += d * d;
                    }
        }
    }
    const double s = group_sum_d(sq, smem);
    if (threadIdx.x == 0) part[((long long)b * 2 + 1) * G + blockIdx.x] = s;
}

// pass 3: one workgroup per sample folds the partials; its first thread writes dycon_volume_stats_t and, when asked,
// dycon_norm_record_t
__global__ __launch_bounds__(RS_THREADS) void stats_finish_kernel(const unsigned* __restrict__ head, const double* __restrict__ part,
                                                                  int G, dycon_volume_stats_t* __restrict__ stats,
                                                                  dycon_norm_record_t* __restrict__ norm) {
    __shared__ double smem[RS_THREADS / 64 + 1];
    const int b = blockIdx.x;
    const unsigned* __restrict__ h = head + (long long)RS_HEAD_WORDS * b;
    const unsigned long long n = *reinterpret_cast<const unsigned long long*>(h);
    double mean = 0.0, sd = 0.0;
    if (n) {                                                          // uniform over the workgroup
        mean = fold_partials(part + ((long long)b * 2 + 0) * G, G, smem) / (double)n;
        sd = sqrt(fold_partials(part + ((long long)b * 2 + 1) * G, G, smem) / (double)n);
    }
    if (threadIdx.x) return;
    const float min_pos = n ? __uint_as_float(~h[2]) : 0.f, max_pos = n ? __uint_as_float(h[3]) : 0.f;
    const float min_all = key_float(~h[4]), max_all = key_float(h[5]);
    const int nonpos = (int)h[6];
    if (stats) {
        dycon_volume_stats_t s;
        s.n_pos = (long long)n, s.mean = mean, s.std = sd;
        s.min_pos = min_pos, s.max_pos = max_pos, s.min_all = min_all, s.max_all = max_all;
        s.any_nonpos = nonpos, s.reserved = 0;
        stats[b] = s;
    }
    if (norm) {
        dycon_norm_record_t r;
        r.mean32 = (float)mean, r.std32 = (float)sd;                   // the fp64 results rounded once
        r.apply_z = n && r.std32 > 0.f;
        if (r.apply_z) {                                               // the z-score is monotone over the voxels > 0; 0 where x <= 0
            r.lo32 = (min_pos - r.mean32) / r.std32;
            r.hi32 = (max_pos - r.mean32) / r.std32;
            if (nonpos) r.lo32 = fminf(r.lo32, 0.f), r.hi32 = fmaxf(r.hi32, 0.f);
        } else r.lo32 = min_all, r.hi32 = max_all;                     // no voxel > 0, or std == 0: the raw values are min-maxed
        r.apply_mm = r.hi32 > r.lo32;                                  // an all-zero (or constant) volume comes back unchanged
        norm[b] = r;
    }
}

__global__ __launch_bounds__(RS_THREADS) void normalize_apply_kernel(const float* __restrict__ x, long long V,
                                                                     const dycon_norm_record_t* __restrict__ norm, float* __restrict__ out) {
    const int b = blockIdx.y;
    const dycon_norm_record_t d = norm[b];
    const NormRec r = {d.apply_z, d.mean32, d.std32, d.apply_mm, d.lo32, d.hi32};
    const float span = r.hi - r.lo;
    const float* __restrict__ p = x + (long long)b * V;
    float* __restrict__ o = out + (long long)b * V;
    const bool vec = (V & 3) == 0 && (((uintptr_t)p | (uintptr_t)o) & 15) == 0;
    const long long Q = (V + 3) >> 2;
    for (long long q = (long long)blockIdx.x * RS_THREADS + threadIdx.x; q < Q; q += (long long)gridDim.x * RS_THREADS) {
        float v[4];
        const int m = load_quad(p, q, V, vec, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = norm_value(v[k], r, span);
        if (vec) *reinterpret_cast<float4*>(o + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < m) o[4 * q + k] = v[k];
        }
    }
}

// ------------------------------------------------------------------ zoom
// tables in the workspace: wgt[(Xo + Yo + Zo) * 2] doubles (order 1 only), then idx[(Xo + Yo + Zo) * 2] ints; axis a starts at
// entry off_a = 0, Xo, Xo + Yo
struct ZoomAxes {
    int n_in[3], n_out[3];
    double step[3];
};

__global__ void zoom_tables_kernel(ZoomAxes ax, int order, double* __restrict__ wgt, int* __restrict__ idx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, a = blockIdx.y;
    if (i >= ax.n_out[a]) return;
    const int e = i + (a > 0 ? ax.n_out[0] : 0) + (a > 1 ? ax.n_out[1] : 0), last = ax.n_in[a] - 1;
    const double c = (double)i * ax.step[a];                           // scipy's zoom: one multiplication
    if (order == 0) {
        idx[2 * e] = idx[2 * e + 1] = min((int)floor(c + 0.5), last);
        return;
    }
    const double f = floor(c), t = c - f;
    const int i0 = min((int)f, last);
    idx[2 * e] = i0, idx[2 * e + 1] = min(i0 + 1, last);               // a tap beyond the last voxel: clamped, weight 0 or dust
    wgt[2 * e] = 1.0 - t, wgt[2 * e + 1] = t;
}

template <typename O> struct Quad;
template <> struct Quad<float> { typedef float4 type; };
template <> struct Quad<unsigned char> { typedef uchar4 type; };

template <typename O> __device__ __forceinline__ void store_quad(O* __restrict__ o, const O (&v)[4], int m, bool vec) {
    if (vec) {
        typename Quad<O>::type q;
        q.x = v[0], q.y = v[1], q.z = v[2], q.w = v[3];
        *reinterpret_cast<typename Quad<O>::type*>(o) = q;
    } else
        for (int k = 0; k < m; ++k) o[k] = v[k];
}
template <> __device__ __forceinline__ void store_quad<double>(double* __restrict__ o, const double (&v)[4], int m, bool vec) {
    if (vec) {
        reinterpret_cast<double2*>(o)[0] = make_double2(v[0], v[1]);
        reinterpret_cast<double2*>(o)[1] = make_double2(v[2], v[3]);
    } else
        for (int k = 0; k < m; ++k) o[k] = v[k];
}

// One thread per four consecutive z outputs of a row (xo, yo) of sample b.  order 0: a gather; binarize: the gathered value > thr as
// 0 / 1.  S: source type, O: output type.
template <typename S, typename O, bool BIN>
__global__ __launch_bounds__(RS_THREADS) void zoom_nearest_kernel(const S* __restrict__ src, int X, int Y, int Z, int Xo, int Yo, int Zo,
                                                                  long long n_quads, const int* __restrict__ idx,
                                                                  const dycon_norm_record_t* __restrict__ norm, float thr,
                                                                  O* __restrict__ out, int vec) {
    const long long q = (long long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (q >= n_quads) return;
    const int ZQ = (Zo + 3) >> 2;
    const int zq = (int)(q % ZQ);
    long long r = q / ZQ;
    const int yo = (int)(r % Yo);
    r /= Yo;
    const int xo = (int)(r % Xo), b = (int)(r / Xo);
    const S* __restrict__ row = src + (((long long)b * X + idx[2 * xo]) * Y + idx[2 * (Xo + yo)]) * Z;
    NormRec nr = {0, 0.f, 1.f, 0, 0.f, 1.f};
    if constexpr (!BIN && sizeof(S) == 4)
        if (norm) {
            const dycon_norm_record_t d = norm[b];
            nr = {d.apply_z, d.mean32, d.std32, d.apply_mm, d.lo32, d.hi32};
        }
    const float span = nr.hi - nr.lo;
    O v[4];
    const int m = min(4, Zo - 4 * zq);
    for (int k = 0; k < m; ++k) {
        const S s = row[idx[2 * (Xo + Yo + 4 * zq + k)]];
        if constexpr (BIN) v[k] = (O)((float)s > thr);
        else if constexpr (sizeof(S) == 4) v[k] = (O)norm_value((float)s, nr, span);
        else v[k] = (O)s;
    }
    store_quad<O>(out + (((long long)b * Xo + xo) * Yo + yo) * Zo + 4 * zq, v, m, vec != 0);
}

// order 1: eight taps in the order x, y, z with z fastest, weight (wx * wy) * wz, acc += weight * double(value) from 0.0 in fp64,
// rounded once to O
template <typename O>
__global__ __launch_bounds__(RS_THREADS) void zoom_linear_kernel(const float* __restrict__ src, int X, int Y, int Z, int Xo, int Yo,
                                                                 int Zo, long long n_quads, const double* __restrict__ wgt,
                                                                 const int* __restrict__ idx, const dycon_norm_record_t* __restrict__ norm,
                                                                 O* __restrict__ out, int vec) {
    const long long q = (long long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (q >= n_quads) return;
    const int ZQ = (Zo + 3) >> 2;
    const int zq = (int)(q % ZQ);
    long long r = q / ZQ;
    const int yo = (int)(r % Yo);
    r /= Yo;
    const int xo = (int)(r % Xo), b = (int)(r / Xo);
    const int ex = xo, ey = Xo + yo;
    const float* __restrict__ vol = src + (long long)b * X * Y * Z;
    const float* __restrict__ rows[4];
    double wxy[4];
#pragma unroll
    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            rows[2 * dx + dy] = vol + ((long long)idx[2 * ex + dx] * Y + idx[2 * ey + dy]) * Z;
            wxy[2 * dx + dy] = wgt[2 * ex + dx] * wgt[2 * ey + dy];
        }
    NormRec nr = {0, 0.f, 1.f, 0, 0.f, 1.f};
    if (norm) {
        const dycon_norm_record_t d = norm[b];
        nr = {d.apply_z, d.mean32, d.std32, d.apply_mm, d.lo32, d.hi32};
    }
    const float span = nr.hi - nr.lo;
    O v[4];
    const int m = min(4, Zo - 4 * zq);
    for (int k = 0; k < m; ++k) {
        const int ez = Xo + Yo + 4 * zq + k;
        const int z0 = idx[2 * ez], z1 = idx[2 * ez + 1];
        const double wz0 = wgt[2 * ez], wz1 = wgt[2 * ez + 1];
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            acc += (wxy[t] * wz0) * (double)norm_value(rows[t][z0], nr, span);
            acc += (wxy[t] * wz1) * (double)norm_value(rows[t][z1], nr, span);
        }
        v[k] = (O)acc;
    }
    store_quad<O>(out + (((long long)b * Xo + xo) * Yo + yo) * Zo + 4 * zq, v, m, vec != 0);
}

int stats_groups(long long V) {
    const long long g = (V + RS_GROUP_VOXELS - 1) / RS_GROUP_VOXELS;
    return (int)(g < 1 ? 1 : g > RS_MAX_GROUPS ? RS_MAX_GROUPS : g);
}

}  // namespace

extern "C" size_t dycon_volume_stats_workspace(int B, long long V) {
    if (B <= 0 || V <= 0) return 0;
    return (size_t)B * ((size_t)2 * stats_groups(V) * sizeof(double) + RS_HEAD_WORDS * sizeof(unsigned));
}

extern "C" int dycon_volume_stats(const float* x, int B, long long V, dycon_volume_stats_t* stats, dycon_norm_record_t* norm,
                                  void* workspace, size_t ws_bytes, dycon_stream_t stream) {
    DYCON_REQUIRE(x && workspace && (stats || norm), "volume_stats: null pointer");
    DYCON_REQUIRE(B >= 1 && B <= 65535 && V >= 1, "volume_stats: %d samples of %lld voxels (1..65535 samples, at least 1 voxel)", B, V);
    DYCON_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0 && ((uintptr_t)norm & 3) == 0,
                  "volume_stats: misaligned pointer (input and record 4 bytes, statistics and workspace 8)");
    DYCON_REQUIRE(ws_bytes >= dycon_volume_stats_workspace(B, V), "volume_stats: workspace of %zu bytes, %zu needed", ws_bytes,
                  dycon_volume_stats_workspace(B, V));
    hipStream_t st = (hipStream_t)stream;
    const int G = stats_groups(V);
    double* part = (double*)workspace;
    unsigned* head = (unsigned*)(part + (size_t)B * 2 * G);
    if (hipMemsetAsync(head, 0, (size_t)B * RS_HEAD_WORDS * sizeof(unsigned), st) != hipSuccess) {
        dycon_set_error("volume_stats: hipMemsetAsync failed");
        return DYCON_ERR_LAUNCH;
    }
    stats_sum_kernel<<<dim3(G, B), RS_THREADS, 0, st>>>(x, V, head, part);
    stats_sq_kernel<<<dim3(G, B), RS_THREADS, 0, st>>>(x, V, head, part);
    stats_finish_kernel<<<B, RS_THREADS, 0, st>>>(head, part, G, stats, norm);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_normalize_apply(const float* x, int B, long long V, const dycon_norm_record_t* norm, float* out,
                                     dycon_stream_t stream) {
    DYCON_REQUIRE(x && norm && out, "normalize_apply: null pointer");
    DYCON_REQUIRE(B >= 1 && B <= 65535 && V >= 1, "normalize_apply: %d samples of %lld voxels (1..65535 samples, at least 1 voxel)", B, V);
    DYCON_REQUIRE((((uintptr_t)x | (uintptr_t)out | (uintptr_t)norm) & 3) == 0, "normalize_apply: pointers must be 4-byte aligned");
    const long long blocks = (V + 4 * RS_THREADS * 4 - 1) / (4 * RS_THREADS * 4);        // four quads per thread, 2048 workgroups at most
    normalize_apply_kernel<<<dim3((int)(blocks > 2048 ? 2048 : blocks), B), RS_THREADS, 0, (hipStream_t)stream>>>(x, V, norm, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" size_t dycon_zoom_workspace(int order, int Xo, int Yo, int Zo) {
    if ((order != 0 && order != 1) || Xo <= 0 || Yo <= 0 || Zo <= 0) return 0;
    const size_t n = (size_t)Xo + Yo + Zo;
    return n * 2 * sizeof(double) + n * 2 * sizeof(int);
}

extern "C" int dycon_zoom(const void* src, int src_bytes, int B, int X, int Y, int Z, int Xo, int Yo, int Zo, int order,
                          const dycon_norm_record_t* norm, int binarize, float threshold, void* out, int out_bytes, void* workspace,
                          size_t ws_bytes, dycon_stream_t stream) {
    DYCON_REQUIRE(src && out && workspace, "zoom: null pointer");
    DYCON_REQUIRE(order == 0 || order == 1, "zoom: order %d (0: nearest, 1: linear; higher spline orders are not built)", order);
    DYCON_REQUIRE(B >= 1 && X >= 1 && Y >= 1 && Z >= 1 && Xo >= 1 && Yo >= 1 && Zo >= 1,
                  "zoom: %d samples, %dx%dx%d -> %dx%dx%d (every axis and the batch at least 1)", B, X, Y, Z, Xo, Yo, Zo);
    DYCON_REQUIRE((long long)X * Y * Z < (1ll << 31) && (long long)Xo * Yo * Zo < (1ll << 31), "zoom: a volume of 2^31 voxels or more");
    DYCON_REQUIRE(src_bytes == 4 || (src_bytes == 1 && order == 0), "zoom: the source is fp32, or uint8 with order 0 (src_bytes = %d)",
                  src_bytes);
    if (binarize)
        DYCON_REQUIRE(order == 0 && out_bytes == 1 && !norm, "zoom: binarize takes order 0, a uint8 output and no record");
    else if (order == 0)
        DYCON_REQUIRE(out_bytes == src_bytes, "zoom: order 0 keeps the type (src_bytes = %d, out_bytes = %d)", src_bytes, out_bytes);
    else
        DYCON_REQUIRE(out_bytes == 4 || out_bytes == 8, "zoom: order 1 writes fp32 or fp64 (out_bytes = %d)", out_bytes);
    DYCON_REQUIRE(!norm || src_bytes == 4, "zoom: a normalisation record needs an fp32 source");
    DYCON_REQUIRE(((uintptr_t)src & (src_bytes - 1)) == 0 && ((uintptr_t)out & (out_bytes - 1)) == 0 && ((uintptr_t)norm & 3) == 0 &&
                      ((uintptr_t)workspace & 7) == 0,
                  "zoom: misaligned pointer (elements at their size, the workspace at 8 bytes)");
    DYCON_REQUIRE(ws_bytes >= dycon_zoom_workspace(order, Xo, Yo, Zo), "zoom: workspace of %zu bytes, %zu needed", ws_bytes,
                  dycon_zoom_workspace(order, Xo, Yo, Zo));
    const long long n_quads = (long long)B * Xo * Yo * ((Zo + 3) >> 2);
    DYCON_REQUIRE((n_quads + RS_THREADS - 1) / RS_THREADS < (1ll << 31), "zoom: too many output voxels in one call");
    hipStream_t st = (hipStream_t)stream;
    ZoomAxes ax;
    const int n_in[3] = {X, Y, Z}, n_out[3] = {Xo, Yo, Zo};
    int longest = 1;
    for (int a = 0; a < 3; ++a) {
        ax.n_in[a] = n_in[a], ax.n_out[a] = n_out[a];
        ax.step[a] = n_out[a] > 1 ? (double)(n_in[a] - 1) / (double)(n_out[a] - 1) : 0.0;
        longest = n_out[a] > longest ? n_out[a] : longest;
    }
    const size_t n_tab = (size_t)Xo + Yo + Zo;
    double* wgt = (double*)workspace;
    int* idx = (int*)(wgt + 2 * n_tab);
    zoom_tables_kernel<<<dim3(cdiv(longest, 64), 3), 64, 0, st>>>(ax, order, wgt, idx);
    // 16-byte stores (4 for uint8, two of 16 for fp64) where every row of four starts aligned
    const int vec = (Zo & 3) == 0 && ((uintptr_t)out & (out_bytes == 1 ? 3 : 15)) == 0;
    const dim3 grid((unsigned)((n_quads + RS_THREADS - 1) / RS_THREADS));
#define ZOOM_ARGS X, Y, Z, Xo, Yo, Zo, n_quads
    if (order == 1) {
        if (out_bytes == 8)
            zoom_linear_kernel<double><<<grid, RS_THREADS, 0, st>>>((const float*)src, ZOOM_ARGS, wgt, idx, norm, (double*)out, vec);
        else zoom_linear_kernel<float><<<grid, RS_THREADS, 0, st>>>((const float*)src, ZOOM_ARGS, wgt, idx, norm, (float*)out, vec);
    } else if (binarize) {
        if (src_bytes == 4)
            zoom_nearest_kernel<float, unsigned char, true>
                <<<grid, RS_THREADS, 0, st>>>((const float*)src, ZOOM_ARGS, idx, nullptr, threshold, (unsigned char*)out, vec);
        else
            zoom_nearest_kernel<unsigned char, unsigned char, true>
                <<<grid, RS_THREADS, 0, st>>>((const unsigned char*)src, ZOOM_ARGS, idx, nullptr, threshold, (unsigned char*)out, vec);
    } else if (src_bytes == 4)
        zoom_nearest_kernel<float, float, false><<<grid, RS_THREADS, 0, st>>>((const float*)src, ZOOM_ARGS, idx, norm, 0.f, (float*)out, vec);
    else
        zoom_nearest_kernel<unsigned char, unsigned char, false>
            <<<grid, RS_THREADS, 0, st>>>((const unsigned char*)src, ZOOM_ARGS, idx, nullptr, 0.f, (unsigned char*)out, vec);
#undef ZOOM_ARGS
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}
