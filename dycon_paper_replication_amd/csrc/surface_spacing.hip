// Surface distances on the device for any voxel spacing and border connectivity: medpy.metric.binary.hd95 / asd with their
// `voxelspacing` and `connectivity` arguments.  csrc/surface.hip (unit spacing, 6 neighbours, integer histograms) is untouched; this
// file is the path for everything else.  With a spacing the squared distances are arbitrary doubles, so there are no bins: the
// transform carries fp64 costs, the percentile is a radix select over their bit patterns and the means are sums in a fixed order.
//
//   border      b = m ^ erode(m) with scipy's generate_binary_structure(3, connectivity): 6, 18 or 26 neighbours, a voxel outside the
//               volume counting as background (border_value = 0)
//   cost        of an integer offset (dx, dy, dz), with w = s * s per axis in fp64 and contraction off:
//                   c = fl(fl(fl(wz * dz^2) + fl(wy * dy^2)) + fl(wx * dx^2))
//   z pass      g[z] = fl(wz * dz^2) to the nearest border voxel of the row (bit scans of ballots), +inf when the row has none
//   y, x pass   out[l] = min_l' fl(g[l'] + fl(w * (l - l')^2)) from a (line x z) tile of doubles in LDS, in place
//   sums        per pair, direction and workgroup: the count of source voxels and the fp64 sum of sqrt(c) over them
//   select      the two order statistics of the percentile by a radix select over the bit patterns of c, 11 bits per pass
//
// Exactness.  Rounding to nearest is monotone: u <= v gives fl(u + k) <= fl(v + k) for every k.  So the minimum over l' of
// fl(g[l'] + k) is fl(min g + k) for each fixed k, and by induction over the three passes the value a voxel ends with is the exact
// minimum of c over all border voxels: each pass takes a minimum of values that are already rounded the way c rounds them, and
// taking a minimum rounds nothing.  Nothing here depends on the grid, the tiling or the order in which candidates are visited.  A
// candidate at axis distance d costs at least fl(w * d^2) (g >= 0 and monotone rounding again), so the search stops at
// w * d^2 >= best without losing a candidate that could win.
//
// Metrics.  The sources of direction a -> b are the voxels whose own cost in a's transform is 0 (the border of a; w > 0, so only the
// offset 0 costs 0); their distances are sqrt of b's transform there.  The means are sums of sqrt(c) in an order fixed by the shape
// alone: a fixed grid, each thread over its own voxels in ascending order, a fixed tree inside the workgroup, and the workgroups'
// partial sums added in index order by one thread.  The percentile selects on c itself: the bit patterns of non-negative doubles
// order as unsigned integers, and sqrt is monotone, so the order statistics of sqrt(c) are sqrt of those of c.  All counters are
// unsigned integers; no floating-point atomic is used anywhere in this file.  Two runs give the same bits.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

#define SPACED_MAX_AXIS 512
#define SPACED_MAX_BLOCKS 256                      // workgroups per pair of the sums and select passes
#define SPACED_DIGIT_BITS 11
#define SPACED_BINS (1 << SPACED_DIGIT_BITS)
#define SPACED_PASSES 6                            // 5 * 11 + 9 = 64 bits

// per-pair state behind the 2 * S cost volumes
struct spaced_pair_t {
    double part[2][SPACED_MAX_BLOCKS];             // sum of sqrt(c) per direction and workgroup
    unsigned cnt[2][SPACED_MAX_BLOCKS];            // sources per direction and workgroup
    unsigned hist[2][SPACED_BINS];                 // digit counts of the two ranks, zero between passes
    unsigned long long prefix[2];                  // the bits of the two order statistics found so far
    unsigned long long rank[2];                    // their 0-based ranks among the keys that share the prefix
    double gamma;                                  // the fraction of numpy's virtual index
    unsigned live, pad;                            // 0: an empty border, the row is NaN and the select passes skip the pair
};

__device__ __forceinline__ unsigned spaced_wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

__device__ __forceinline__ double spaced_wave_sum_f64(double v) {      // a fixed tree: the same bits on every run
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per row (x, y) of pair blockIdx.y; lanes run along z, as surface_border_z_kernel.  A member voxel is interior when all of
// its neighbours within `conn` axis steps are members; a neighbour outside the volume is not.
template <typename T>
__global__ __launch_bounds__(256) void spaced_border_z_kernel(const T* __restrict__ vol, int n_cls, int cls_lo, int X, int Y, int Z,
                                                              int conn, int side, double wz, double* __restrict__ cost) {
    constexpr int WORDS = SPACED_MAX_AXIS / 64, NONE = 1 << 14;
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
    unsigned long long word[WORDS];
#pragma unroll
    for (int c = 0; c < WORDS; ++c) {
        word[c] = 0;
        if (c * 64 < Z) {
            const int z = c * 64 + lane;
            bool b = false;
            if (z < Z && member(r0 + z)) {
                bool inner = true;
                for (int dx = -1; dx <= 1 && inner; ++dx)
                    for (int dy = -1; dy <= 1 && inner; ++dy)
                        for (int dz = -1; dz <= 1 && inner; ++dz) {
                            const int steps = (dx != 0) + (dy != 0) + (dz != 0);
                            if (steps == 0 || steps > conn) continue;
                            const int nx = x + dx, ny = y + dy, nz = z + dz;
                            inner = nx >= 0 && nx < X && ny >= 0 && ny < Y && nz >= 0 && nz < Z &&
                                    member(r0 + z + dx * plane + (long long)dy * Z + dz);
                        }
                b = !inner;
            }
            word[c] = __ballot(b);
        }
    }
    double* __restrict__ out = cost + (long long)(2 * s + side) * V + r0;
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
            if (z < Z) out[z] = best < NONE ? wz * (double)(best * best) : (double)INFINITY;
        }
    }
}

// In place along one of the two outer axes, as surface_axis_pass_kernel: blockIdx.z picks the volume, blockIdx.y the index along the
// other outer axis, blockIdx.x the ZT-wide z tile.  The whole (L x ZT) tile of doubles is in LDS before anything is written back:
// 128 x 64, 256 x 64 (128 KB) or 512 x 32 (128 KB).  256 threads = 256 / ZT lines at a time.
template <int LMAX, int ZT>
__global__ __launch_bounds__(256) void spaced_axis_pass_kernel(double* __restrict__ cost, long long V, int L, long long line_stride,
                                                               long long other_stride, int Z, double w) {
    __shared__ double tile[LMAX][ZT];
    constexpr int NL = 256 / ZT;
    const int g = threadIdx.x / ZT, lane = threadIdx.x % ZT;
    const int z = blockIdx.x * ZT + lane;
    const bool live = z < Z;
    const double far = (double)INFINITY;
    double* __restrict__ base = cost + (long long)blockIdx.z * V + (long long)blockIdx.y * other_stride + z;
    for (int l = g; l < L; l += NL) tile[l][lane] = live ? base[l * line_stride] : far;
    __syncthreads();
    if (!live) return;
    for (int l = g; l < L; l += NL) {
        double best = tile[l][lane];
        const int reach = max(l, L - 1 - l);
        // four distances per trip, as the unit-spacing pass; a candidate past the pruning bound cannot win
        for (int d = 1; d <= reach && w * (double)(d * d) < best; d += 4) {
            double cand = best;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = d + j, lo = l - e, hi = l + e;
                const double ee = w * (double)(e * e);
                const double below = tile[max(lo, 0)][lane], above = tile[min(hi, L - 1)][lane];
                cand = fmin(cand, fmin(lo >= 0 ? below + ee : far, hi < L ? above + ee : far));
            }
            best = cand;
        }
        base[l * line_stride] = best;
    }
}

// Workgroup blockIdx.x of pair blockIdx.y over the voxels i = blockIdx.x * 256 + t, + gridDim.x * 256, ...: the sources of each
// direction and the sum of their distances.  Every workgroup writes its own cells; nothing is accumulated across workgroups here.
__global__ __launch_bounds__(256) void spaced_sums_kernel(const double* __restrict__ cost, long long V, spaced_pair_t* __restrict__ pairs) {
    __shared__ double wsum[2][4];
    __shared__ unsigned wcnt[2][4];
    const int s = blockIdx.y, t = threadIdx.x;
    const double* __restrict__ ca = cost + (long long)(2 * s) * V;
    const double* __restrict__ cb = ca + V;
    double s0 = 0.0, s1 = 0.0;
    unsigned na = 0, nb = 0;
    for (long long i = (long long)blockIdx.x * 256 + t; i < V; i += (long long)gridDim.x * 256) {
        const double a = ca[i], b = cb[i];
        if (a == 0.0) { ++na; s0 += sqrt(b); }
        if (b == 0.0) { ++nb; s1 += sqrt(a); }
    }
    s0 = spaced_wave_sum_f64(s0);
    s1 = spaced_wave_sum_f64(s1);
    na = spaced_wave_sum_u32(na);
    nb = spaced_wave_sum_u32(nb);
    if ((t & 63) == 0) {
        wsum[0][t >> 6] = s0;
        wsum[1][t >> 6] = s1;
        wcnt[0][t >> 6] = na;
        wcnt[1][t >> 6] = nb;
    }
    __syncthreads();
    if (t < 2) {
        spaced_pair_t* __restrict__ P = pairs + s;
        P->part[t][blockIdx.x] = ((wsum[t][0] + wsum[t][1]) + wsum[t][2]) + wsum[t][3];
        P->cnt[t][blockIdx.x] = wcnt[t][0] + wcnt[t][1] + wcnt[t][2] + wcnt[t][3];
    }
}

// One workgroup per pair: the border sizes and the means from the workgroups' cells in index order, the two ranks of the
// percentile (np.percentile's default "linear" rule, written as surface_metrics_kernel writes it), and a clean select state.
__global__ __launch_bounds__(256) void spaced_begin_kernel(spaced_pair_t* __restrict__ pairs, int nblocks, double q,
                                                           double* __restrict__ out) {
    __shared__ double part[2][SPACED_MAX_BLOCKS];
    __shared__ unsigned cnt[2][SPACED_MAX_BLOCKS];
    spaced_pair_t* __restrict__ P = pairs + blockIdx.x;
    for (int i = threadIdx.x; i < 2 * SPACED_BINS; i += 256) (&P->hist[0][0])[i] = 0;
    for (int r = 0; r < 2; ++r) {
        part[r][threadIdx.x] = threadIdx.x < nblocks ? P->part[r][threadIdx.x] : 0.0;
        cnt[r][threadIdx.x] = threadIdx.x < nblocks ? P->cnt[r][threadIdx.x] : 0u;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum0 = 0.0, sum1 = 0.0;
    unsigned long long na = 0, nb = 0;
    for (int i = 0; i < nblocks; ++i) {                      // index order, one thread
        sum0 += part[0][i];
        sum1 += part[1][i];
        na += cnt[0][i];
        nb += cnt[1][i];
    }
    double* __restrict__ o = out + 5 * blockIdx.x;
    o[3] = (double)na;
    o[4] = (double)nb;
    P->prefix[0] = P->prefix[1] = 0;
    if (na == 0 || nb == 0) {
        o[0] = o[1] = o[2] = __longlong_as_double(0x7ff8000000000000ll);
        P->live = 0;
        return;
    }
    o[1] = sum0 / (double)na;
    o[2] = sum1 / (double)nb;
    const long long n = (long long)(na + nb);
    const double p = q / 100.0;
    const double vi = (double)(n - 1) * p;
    const double fl = floor(vi);
    long long lo = (long long)fl, hi = lo + 1;
    if (vi >= (double)(n - 1)) lo = hi = n - 1;
    if (vi < 0.0) lo = hi = 0;
    P->rank[0] = (unsigned long long)lo;
    P->rank[1] = (unsigned long long)hi;
    P->gamma = vi - fl;
    P->live = 1;
}

// One pass of the select: the keys are the costs of the source voxels of both directions (a voxel on both borders gives two keys 0).
// A key that shares the prefix of a rank found so far adds one to that rank's count of its next digit; while both ranks share one
// prefix only the first is counted.  Counted in LDS, each workgroup then adds its non-zero cells to the pair's counts once.
__global__ __launch_bounds__(256) void spaced_digit_kernel(const double* __restrict__ cost, long long V, spaced_pair_t* __restrict__ pairs,
                                                           int shift, int width) {
    __shared__ unsigned low[2][SPACED_BINS];
    const int s = blockIdx.y;
    spaced_pair_t* __restrict__ P = pairs + s;
    if (!P->live) return;                                    // the whole workgroup
    const unsigned long long p0 = P->prefix[0], p1 = P->prefix[1];
    const bool both = p0 != p1;
    const int top = shift + width;                           // 64 in the first pass: every key matches
    const unsigned mask = (1u << width) - 1;
    for (int i = threadIdx.x; i < 2 * SPACED_BINS; i += 256) (&low[0][0])[i] = 0;
    __syncthreads();
    const double* __restrict__ ca = cost + (long long)(2 * s) * V;
    const double* __restrict__ cb = ca + V;
    auto count = [&](unsigned long long key) {
        const unsigned long long head = top >= 64 ? 0ull : key >> top;
        const unsigned digit = (unsigned)(key >> shift) & mask;
        if (head == p0) atomicAdd(&low[0][digit], 1u);
        if (both && head == p1) atomicAdd(&low[1][digit], 1u);
    };
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        const double a = ca[i], b = cb[i];
        if (a == 0.0) count((unsigned long long)__double_as_longlong(b));
        if (b == 0.0) count((unsigned long long)__double_as_longlong(a));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * SPACED_BINS; i += 256) {
        const unsigned c = (&low[0][0])[i];
        if (c) atomicAdd(&P->hist[0][0] + i, c);
    }
}

// One workgroup per pair after each pass: the digit of each rank is the first bin whose cumulative count passes the rank; the rank
// becomes the rank inside that bin and the counts are zeroed for the next pass.  After the last pass the prefixes are the two order
// statistics themselves and the percentile is written.
__global__ __launch_bounds__(256) void spaced_pick_kernel(spaced_pair_t* __restrict__ pairs, int width, int last, double* __restrict__ out) {
    __shared__ unsigned bins[2][SPACED_BINS];
    __shared__ unsigned long long chunk[2][256];
    spaced_pair_t* __restrict__ P = pairs + blockIdx.x;
    if (!P->live) return;
    const int t = threadIdx.x;
    const bool both = P->prefix[0] != P->prefix[1];
    constexpr int PER = SPACED_BINS / 256;
    for (int r = 0; r < 2; ++r) {
        unsigned long long c = 0;
        for (int j = 0; j < PER; ++j) {
            const unsigned v = P->hist[both ? r : 0][t * PER + j];
            bins[r][t * PER + j] = v;
            c += v;
        }
        chunk[r][t] = c;
    }
    __syncthreads();
    for (int i = t; i < 2 * SPACED_BINS; i += 256) (&P->hist[0][0])[i] = 0;
    if (t == 0 || t == 64) {                                 // one lane of two waves: a rank each
        const int r = t >> 6;
        unsigned long long rank = P->rank[r];
        int k = 0;
        while (k < 255 && chunk[r][k] <= rank) rank -= chunk[r][k++];
        int bin = k * PER;
        while (bin < k * PER + PER - 1 && bins[r][bin] <= rank) rank -= bins[r][bin++];
        P->rank[r] = rank;
        chunk[r][0] = (P->prefix[r] << width) | (unsigned long long)bin;
    }
    __syncthreads();
    if (t != 0) return;
    P->prefix[0] = chunk[0][0];
    P->prefix[1] = chunk[1][0];
    if (!last) return;
    const double v0 = sqrt(__longlong_as_double((long long)chunk[0][0])), v1 = sqrt(__longlong_as_double((long long)chunk[1][0]));
    const double gamma = P->gamma;
    const double diff = v1 - v0;
    double r = v0 + diff * gamma;
    if (gamma >= 0.5) r = v1 - diff * (1.0 - gamma);
    out[5 * blockIdx.x] = r;
}

extern "C" size_t dycon_surface_spaced_workspace(int S, int X, int Y, int Z) {
    if (S <= 0 || X <= 0 || Y <= 0 || Z <= 0) return 0;
    return (size_t)S * (2 * (size_t)X * Y * Z * sizeof(double) + sizeof(spaced_pair_t));
}

static void spaced_axis_pass(double* cost, long long V, int L, long long line_stride, int n_other, long long other_stride, int Z, int S,
                             double w, hipStream_t stream) {
    if (L <= 128)
        spaced_axis_pass_kernel<128, 64><<<dim3(cdiv(Z, 64), n_other, 2 * S), 256, 0, stream>>>(cost, V, L, line_stride, other_stride, Z, w);
    else if (L <= 256)
        spaced_axis_pass_kernel<256, 64><<<dim3(cdiv(Z, 64), n_other, 2 * S), 256, 0, stream>>>(cost, V, L, line_stride, other_stride, Z, w);
    else
        spaced_axis_pass_kernel<SPACED_MAX_AXIS, 32><<<dim3(cdiv(Z, 32), n_other, 2 * S), 256, 0, stream>>>(cost, V, L, line_stride,
                                                                                                           other_stride, Z, w);
}

extern "C" int dycon_surface_spaced_metrics(const void* a, int a_bytes, const void* b, int b_bytes, int n_vol, int cls_lo, int n_cls,
                                            int X, int Y, int Z, const double* spacing, int connectivity, double q, double* out,
                                            void* workspace, size_t ws_bytes, dycon_stream_t stream) {
    DYCON_REQUIRE(a && b && spacing && out && workspace, "surface_spaced_metrics: null pointer");
    DYCON_REQUIRE(a_bytes == 1, "surface_spaced_metrics: the prediction must be uint8 (a_bytes = %d)", a_bytes);
    DYCON_REQUIRE(b_bytes == 1 || b_bytes == 8, "surface_spaced_metrics: ground truth must be uint8 or int64 (b_bytes = %d)", b_bytes);
    DYCON_REQUIRE(X >= 1 && X <= SPACED_MAX_AXIS && Y >= 1 && Y <= SPACED_MAX_AXIS && Z >= 1 && Z <= SPACED_MAX_AXIS,
                  "surface_spaced_metrics: volume %dx%dx%d (every axis 1..%d)", X, Y, Z, SPACED_MAX_AXIS);
    DYCON_REQUIRE(n_vol >= 1 && n_cls >= 1 && cls_lo >= 0 && (cls_lo > 0 || n_cls == 1) && cls_lo + n_cls <= 256,
                  "surface_spaced_metrics: bad class range (cls_lo = %d, n_cls = %d; cls_lo = 0 means voxel != 0 and takes n_cls = 1)",
                  cls_lo, n_cls);
    double w[3];
    for (int i = 0; i < 3; ++i) {
        // the squares and 3 * 511^2 of them stay normal fp64 numbers: no cost underflows to 0 or overflows to inf
        DYCON_REQUIRE(isfinite(spacing[i]) && spacing[i] >= 1e-150 && spacing[i] <= 1e150,
                      "surface_spaced_metrics: voxel spacing (%g, %g, %g): every entry finite, > 0 and within 1e-150..1e150", spacing[0],
                      spacing[1], spacing[2]);
        w[i] = spacing[i] * spacing[i];
    }
    DYCON_REQUIRE(connectivity >= 1 && connectivity <= 3, "surface_spaced_metrics: connectivity %d (1, 2 or 3)", connectivity);
    DYCON_REQUIRE(q >= 0.0 && q <= 100.0, "surface_spaced_metrics: percentile %g outside [0, 100]", q);
    const long long S = (long long)n_vol * n_cls;
    DYCON_REQUIRE(2 * S <= 65535, "surface_spaced_metrics: %lld pairs in one call (at most 32767)", S);
    DYCON_REQUIRE(ws_bytes >= dycon_surface_spaced_workspace((int)S, X, Y, Z), "surface_spaced_metrics: workspace of %zu bytes, %zu needed",
                  ws_bytes, dycon_surface_spaced_workspace((int)S, X, Y, Z));
    DYCON_REQUIRE(((uintptr_t)workspace & 7) == 0, "surface_spaced_metrics: the workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long V = (long long)X * Y * Z;
    double* cost = (double*)workspace;
    spaced_pair_t* pairs = (spaced_pair_t*)(cost + 2 * S * V);
    dim3 rows(cdiv(X * Y, 4), (int)S);
    spaced_border_z_kernel<unsigned char><<<rows, 256, 0, st>>>((const unsigned char*)a, n_cls, cls_lo, X, Y, Z, connectivity, 0, w[2], cost);
    if (b_bytes == 1)
        spaced_border_z_kernel<unsigned char><<<rows, 256, 0, st>>>((const unsigned char*)b, n_cls, cls_lo, X, Y, Z, connectivity, 1, w[2],
                                                                    cost);
    else
        spaced_border_z_kernel<long long><<<rows, 256, 0, st>>>((const long long*)b, n_cls, cls_lo, X, Y, Z, connectivity, 1, w[2], cost);
    if (Y > 1) spaced_axis_pass(cost, V, Y, Z, X, (long long)Y * Z, Z, (int)S, w[1], st);        // lines along y at fixed x
    if (X > 1) spaced_axis_pass(cost, V, X, (long long)Y * Z, Y, Z, Z, (int)S, w[0], st);        // lines along x at fixed y
    const long long want = (V + 256 * 16 - 1) / (256 * 16);                                        // 16 voxels per thread or more
    const int nblocks = (int)(want > SPACED_MAX_BLOCKS ? SPACED_MAX_BLOCKS : want);
    const dim3 grid(nblocks, (int)S);
    spaced_sums_kernel<<<grid, 256, 0, st>>>(cost, V, pairs);
    spaced_begin_kernel<<<(int)S, 256, 0, st>>>(pairs, nblocks, q, out);
    for (int pass = 0; pass < SPACED_PASSES; ++pass) {
        const int shift = 64 - SPACED_DIGIT_BITS * (pass + 1) > 0 ? 64 - SPACED_DIGIT_BITS * (pass + 1) : 0;
        const int width = pass + 1 < SPACED_PASSES ? SPACED_DIGIT_BITS : 64 - SPACED_DIGIT_BITS * (SPACED_PASSES - 1);
        spaced_digit_kernel<<<grid, 256, 0, st>>>(cost, V, pairs, shift, width);
        spaced_pick_kernel<<<(int)S, 256, 0, st>>>(pairs, width, pass + 1 == SPACED_PASSES, out);
    }
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}
