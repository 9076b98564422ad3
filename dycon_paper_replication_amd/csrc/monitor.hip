// Pair-similarity histograms of the reference's training monitor (code/utils/monitor.py:7-50), without the (B, N, N) matrix.
//
// Restated semantics, pooled over the batch:
//   s_bij = <x_bi / max(|x_bi|, 1e-12), x_bj / max(|x_bj|, 1e-12)> / tau      (F.normalize, matmul, / tau)
//   the pair (b, i, j) is positive when mask[b, i] == mask[b, j] (float equality, torch.eq), negative otherwise; all B*N^2 ordered
//   pairs count, the diagonal as positive.  Each set is binned as np.histogram(values_f32, bins) bins it (plt.hist):
//   range = the set's float32 (min, max), (min - 0.5, max + 0.5) when they are equal, (0, 1) when the set is empty;
//   step = (hi - lo) / bins and edge[k] = k * step + lo in float32 with two roundings, edge[bins] = hi;
//   v goes in bin k when edge[k] <= v < edge[k + 1], the last bin closed.
//
// Launches: prep (inverse row norms, accumulators reset) -> sweep 0 (min / max of each set) -> finalize (edges) -> sweep 1 (bins).
// Each sweep recomputes 64 x 64 Gram tiles on MFMA with fp32 accumulation (bf16: 32x32x16_bf16, exact products of the stored
// values; fp32: 32x32x2f32, exact fp32 products) over the tile pairs j >= i only: the value and the pair class are symmetric, so
// an off-diagonal tile counts twice.  Sweep 1 bins into 8 LDS sub-histograms per workgroup (one per half-wave: similar pairs
// cluster in a few bins) and adds one 64-bit integer atomic per non-empty bin per workgroup.  Min / max go through atomics on
// order-preserving integer images of the floats.  Everything is integer-exact: the result is bitwise reproducible.
// Workspace: B*N inverse norms + 4 ints; nothing scales with N^2.
#include "common.h"

namespace {

constexpr int ST = 64;          // tile edge: rows i and columns j of one workgroup step (4 waves, one 32 x 32 quadrant each)
constexpr int NCOPY = 8;        // LDS sub-histograms per workgroup
constexpr int MAX_BINS = 256;
constexpr int MAX_WG = 1024;    // sweep grid: contiguous runs of tile pairs per workgroup

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// LDS row image per storage type: KS = k-elements per MFMA step of one lane pair, PAD keeps rows 16-byte aligned and staggered
template <typename T> struct SimTile;
template <> struct SimTile<float> {
    typedef float E;
    static constexpr int KS = 8, PAD = 4;
};
template <> struct SimTile<bf16> {
    typedef unsigned short E;
    static constexpr int KS = 16, PAD = 8;
};

__device__ __forceinline__ int f2ord(float f) {   // monotone float -> int map (its own inverse)
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float ord2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

// rows [row0, row0 + 64) of one sample into LDS, zero past N and past Dm (k < Dp)
template <typename E>
__device__ __forceinline__ void stage_tile(E* __restrict__ dst, int stride, int Dp, const E* __restrict__ src, int row0, int N, int Dm,
                                           bool vec) {
    constexpr int V = 16 / sizeof(E);
    if (vec) {   // Dm % V == 0 and a 16-byte aligned base: 16-byte pieces
        const int ppr = Dp / V;
        for (int e = threadIdx.x; e < ST * ppr; e += 256) {
            const int r = e / ppr, k = (e - r * ppr) * V;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (row0 + r < N && k < Dm) v = *reinterpret_cast<const uint4*>(src + (long long)(row0 + r) * Dm + k);
            *reinterpret_cast<uint4*>(dst + r * stride + k) = v;
        }
    } else {
        for (int e = threadIdx.x; e < ST * Dp; e += 256) {
            const int r = e / Dp, k = e - r * Dp;
            dst[r * stride + k] = (row0 + r < N && k < Dm) ? src[(long long)(row0 + r) * Dm + k] : E(0);
        }
    }
}

// 32 x 32 Gram quadrant: acc[reg] = <Ai[row], Bj[col]> with col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
__device__ __forceinline__ f32x16 gram32(const float* __restrict__ Ai, const float* __restrict__ Bj, int stride, int nq, int lane) {
    f32x16 acc = {};
    const int r = lane & 31, h = lane >> 5;
    const float* ap = Ai + r * stride + 4 * h;
    const float* bp = Bj + r * stride + 4 * h;
    for (int q = 0; q < nq; ++q) {   // lane half h supplies k = 8q + 4h + e to the e-th MFMA of the step, on both operands
        const float4 a = *reinterpret_cast<const float4*>(ap + 8 * q);
        const float4 b = *reinterpret_cast<const float4*>(bp + 8 * q);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    }
    return acc;
}
__device__ __forceinline__ f32x16 gram32(const unsigned short* __restrict__ Ai, const unsigned short* __restrict__ Bj, int stride, int nq,
                                         int lane) {
    f32x16 acc = {};
    const int r = lane & 31, h = lane >> 5;
    const unsigned short* ap = Ai + r * stride + 8 * h;
    const unsigned short* bp = Bj + r * stride + 8 * h;
    for (int q = 0; q < nq; ++q) {   // k = 16q + 8h + e
        const bf16x8 a = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(ap + 16 * q));
        const bf16x8 b = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(bp + 16 * q));
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
    return acc;
}

// inverse norms (one wave per row) and the accumulators reset (block 0)
template <typename T>
__global__ __launch_bounds__(256) void simhist_prep_kernel(const T* __restrict__ F, long long R, int Dm, float* __restrict__ rinv,
                                                           int* __restrict__ mm, unsigned long long* __restrict__ counts, int ncounts) {
    if (blockIdx.x == 0) {
        for (int t = threadIdx.x; t < ncounts; t += 256) counts[t] = 0ull;
        if (threadIdx.x < 4) mm[threadIdx.x] = (threadIdx.x & 1) ? f2ord(-INFINITY) : f2ord(INFINITY);   // {min, max} x {pos, neg}
    }
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= R) return;
    float ss = 0.f;
    for (int k = lane; k < Dm; k += 64) {
        const float v = ldf(F + row * Dm + k);
        ss += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    if (lane == 0) rinv[row] = 1.f / fmaxf(sqrtf(ss), 1e-12f);
}

// PASS 0: min / max of each set into mm;  PASS 1: counts from the edges written by simhist_finalize_kernel
template <typename T, int PASS>
__global__ __launch_bounds__(256) void simhist_kernel(const T* __restrict__ F, const float* __restrict__ mask, const float* __restrict__ rinv,
                                                      int N, int Dm, int Dp, int stride, bool vec, float inv_tau, int NT, long long npairs,
                                                      long long per_wg, int bins, int* __restrict__ mm, const float* __restrict__ edges,
                                                      unsigned long long* __restrict__ counts) {
    typedef typename SimTile<T>::E E;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    E* Ai = reinterpret_cast<E*>(lds_raw);                      // [64][stride] rows of tile i
    E* Bj = Ai + ST * stride;                                   // [64][stride] rows of tile j
    float* info = reinterpret_cast<float*>(Bj + ST * stride);   // mask_i, rinv_i, mask_j, rinv_j: [4][64]
    float* sedge = info + 4 * ST;                               // [2][bins + 1]
    unsigned* hist = reinterpret_cast<unsigned*>(sedge + 2 * (bins + 1));   // [NCOPY][2 bins + 1]
    const int hs = 2 * bins + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;

    float scale[2] = {0.f, 0.f};
    if (PASS == 1) {
        for (int t = threadIdx.x; t < 2 * (bins + 1); t += 256) sedge[t] = edges[t];
        for (int t = threadIdx.x; t < NCOPY * hs; t += 256) hist[t] = 0u;
        __syncthreads();
        for (int s = 0; s < 2; ++s) scale[s] = (float)bins / (sedge[s * (bins + 1) + bins] - sedge[s * (bins + 1)]);   // first guess only
    }
    float pmin = INFINITY, pmax = -INFINITY, nmin = INFINITY, nmax = -INFINITY;
    unsigned* myhist = hist + (2 * wave + h) * hs;

    long long p = (long long)blockIdx.x * per_wg;
    const long long p_end = min(npairs, p + per_wg);
    // pair index -> (sample, tile i, tile j >= i), row-major over the upper triangle of each sample
    const long long tri = (long long)NT * (NT + 1) / 2;
    int b = (int)(p / tri), ti = 0;
    long long q = p - b * tri;
    while (q >= NT - ti) q -= NT - ti++;
    int tj = ti + (int)q, cb = -1, cti = -1;

    for (; p < p_end; ++p) {
        const E* Fb = reinterpret_cast<const E*>(F) + (long long)b * N * Dm;
        const float* mb = mask + (long long)b * N;
        const float* rb = rinv + (long long)b * N;
        __syncthreads();   // the previous tile pair is consumed
        if (b != cb || ti != cti) {
            stage_tile(Ai, stride, Dp, Fb, ti * ST, N, Dm, vec);
            if (threadIdx.x < ST) {
                const int gi = ti * ST + threadIdx.x;
                info[threadIdx.x] = gi < N ? mb[gi] : 0.f;
                info[ST + threadIdx.x] = gi < N ? rb[gi] : 0.f;
            }
            cb = b;
            cti = ti;
        }
        if (tj != ti) stage_tile(Bj, stride, Dp, Fb, tj * ST, N, Dm, vec);
        if (threadIdx.x < ST) {
            const int gj = tj * ST + threadIdx.x;
            info[2 * ST + threadIdx.x] = gj < N ? mb[gj] : 0.f;
            info[3 * ST + threadIdx.x] = gj < N ? rb[gj] : 0.f;
        }
        __syncthreads();

        const int i0 = 32 * (wave >> 1), j0 = 32 * (wave & 1);
        const f32x16 acc = gram32(Ai + i0 * stride, (tj != ti ? Bj : Ai) + j0 * stride, stride, Dp / SimTile<T>::KS, lane);
        const int jl = j0 + (lane & 31);
        const bool jv = tj * ST + jl < N;
        const float mj = info[2 * ST + jl], rj = info[3 * ST + jl];
        const unsigned w = tj != ti ? 2u : 1u;   // an off-diagonal tile stands for its mirror image too
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int il = i0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            if (!jv || ti * ST + il >= N) continue;
            const float s = acc[reg] * (info[ST + il] * rj) * inv_tau;   // (ri * rj): the same bits for (i, j) and (j, i)
            const bool pos = info[il] == mj;
            if (PASS == 0) {
                if (pos) { pmin = fminf(pmin, s); pmax = fmaxf(pmax, s); }
                else     { nmin = fminf(nmin, s); nmax = fmaxf(nmax, s); }
            } else {
                const int set = pos ? 0 : 1;
                const float* e = sedge + set * (bins + 1);
                const float g = (s - e[0]) * scale[set];
                int k = g >= (float)(bins - 1) ? bins - 1 : (g > 0.f ? (int)g : 0);
                while (k > 0 && s < e[k]) --k;                 // the edge rule decides, the guess only starts the search
                while (k < bins - 1 && s >= e[k + 1]) ++k;
                atomicAdd(myhist + set * bins + k, w);
            }
        }

        if (++tj == NT) {
            if (++ti == NT) { ++b; ti = 0; }
            tj = ti;
        }
    }

    if (PASS == 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            pmin = fminf(pmin, __shfl_xor(pmin, o));
            pmax = fmaxf(pmax, __shfl_xor(pmax, o));
            nmin = fminf(nmin, __shfl_xor(nmin, o));
            nmax = fmaxf(nmax, __shfl_xor(nmax, o));
        }
        if (lane == 0) {
            if (pmin <= pmax) { atomicMin(mm + 0, f2ord(pmin)); atomicMax(mm + 1, f2ord(pmax)); }
            if (nmin <= nmax) { atomicMin(mm + 2, f2ord(nmin)); atomicMax(mm + 3, f2ord(nmax)); }
        }
    } else {
        __syncthreads();
        for (int t = threadIdx.x; t < 2 * bins; t += 256) {
            unsigned long long c = 0;
#pragma unroll
            for (int z = 0; z < NCOPY; ++z) c += hist[z * hs + t];
            if (c) atomicAdd(counts + t, c);
        }
    }
}

// ranges and float32 edges of both sets (np.histogram's rule, see the top of the file); minmax = {pos lo, hi, neg lo, hi}
__global__ void simhist_finalize_kernel(const int* __restrict__ mm, int bins, float* __restrict__ edges, float* __restrict__ minmax) {
#pragma clang fp contract(off)   // two roundings per edge; __fmul_rn / __fadd_rn inline as contractible ops, so plain operators here
    for (int s = 0; s < 2; ++s) {
        float lo = ord2f(mm[2 * s]), hi = ord2f(mm[2 * s + 1]);
        if (lo > hi) { lo = 0.f; hi = 1.f; }                      // empty set
        if (threadIdx.x == 0) { minmax[2 * s] = lo; minmax[2 * s + 1] = hi; }
        if (lo == hi) { lo = lo - 0.5f; hi = hi + 0.5f; }
        const float step = (hi - lo) / (float)bins;
        float* e = edges + s * (bins + 1);
        for (int k = threadIdx.x; k <= bins; k += blockDim.x) e[k] = k == bins ? hi : (float)k * step + lo;
    }
}

template <typename T> size_t simhist_lds_bytes(int Dm, int bins, int pass) {
    typedef SimTile<T> G;
    const int Dp = (Dm + G::KS - 1) / G::KS * G::KS;
    size_t n = (size_t)2 * ST * (Dp + G::PAD) * sizeof(typename G::E) + 4 * ST * sizeof(float);
    if (pass == 1) n += 2 * (bins + 1) * sizeof(float) + (size_t)NCOPY * (2 * bins + 1) * sizeof(unsigned);
    return n;
}

template <typename T, int PASS>
int simhist_sweep(const void* feat, const float* mask, const float* rinv, int B, int N, int Dm, float tau, int bins, int* mm,
                  const float* edges, unsigned long long* counts, dycon_stream_t stream) {
    typedef SimTile<T> G;
    const size_t lds = simhist_lds_bytes<T>(Dm, bins, PASS);
    if (hipFuncSetAttribute((const void*)simhist_kernel<T, PASS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        dycon_set_error("simhist: cannot reserve %zu bytes of LDS", lds);
        return DYCON_ERR_LAUNCH;
    }
    const int Dp = (Dm + G::KS - 1) / G::KS * G::KS, NT = (N + ST - 1) / ST;
    const long long npairs = (long long)B * NT * (NT + 1) / 2;
    const long long nwg = npairs < MAX_WG ? npairs : MAX_WG, per_wg = (npairs + nwg - 1) / nwg;
    const bool vec = Dm % (16 / (int)sizeof(typename G::E)) == 0 && ((uintptr_t)feat & 15) == 0;
    simhist_kernel<T, PASS><<<(unsigned)((npairs + per_wg - 1) / per_wg), 256, lds, stream>>>(
        (const T*)feat, mask, rinv, N, Dm, Dp, Dp + G::PAD, vec, 1.f / tau, NT, npairs, per_wg, bins, mm, edges, counts);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

}  // namespace

extern "C" size_t dycon_simhist_workspace(int B, int N, int Dm, int bins) {
    (void)Dm;
    (void)bins;
    if (B <= 0 || N <= 0) return 0;
    return (4 + (size_t)B * N) * sizeof(float);   // 4 ordered-int min / max slots, then the B*N inverse norms
}

extern "C" int dycon_simhist(const void* feat, const float* mask, int dtype, int B, int N, int Dm, float tau, int bins,
                             long long* counts, float* edges, float* minmax, float* workspace, size_t ws_bytes,
                             dycon_stream_t stream) {
    DYCON_REQUIRE(feat && mask && counts && edges && minmax && workspace, "simhist: null pointer");
    DYCON_REQUIRE(B > 0 && N > 0 && Dm > 0, "simhist: bad shape (B=%d, N=%d, Dm=%d)", B, N, Dm);
    DYCON_REQUIRE(Dm <= 256, "simhist: feature dim %d > 256 not supported", Dm);
    DYCON_REQUIRE(bins >= 1 && bins <= MAX_BINS, "simhist: bins = %d outside 1..%d", bins, MAX_BINS);
    DYCON_REQUIRE(tau > 0.f && tau < INFINITY, "simhist: tau must be positive and finite");
    DYCON_REQUIRE(dtype == DYCON_F32 || dtype == DYCON_BF16, "simhist: bad dtype %d", dtype);
    DYCON_REQUIRE(ws_bytes >= dycon_simhist_workspace(B, N, Dm, bins), "simhist: workspace too small");
    int* mm = reinterpret_cast<int*>(workspace);
    float* rinv = workspace + 4;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    const long long R = (long long)B * N;
    int e = DYCON_OK;
    DYCON_DISPATCH(dtype, {
        simhist_prep_kernel<T><<<(unsigned)((R + 3) / 4), 256, 0, stream>>>((const T*)feat, R, Dm, rinv, mm, cnt, 2 * bins);
        DYCON_LAUNCH_CHECK();
        e = simhist_sweep<T, 0>(feat, mask, rinv, B, N, Dm, tau, bins, mm, edges, cnt, stream);
        if (e) return e;
        simhist_finalize_kernel<<<1, 256, 0, stream>>>(mm, bins, edges, minmax);
        DYCON_LAUNCH_CHECK();
        e = simhist_sweep<T, 1>(feat, mask, rinv, B, N, Dm, tau, bins, mm, edges, cnt, stream);
    });
    return e;
}
