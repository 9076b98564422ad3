// 3-D ASPP on the feature branch (networks/assp.py:28-82, UNet3D_contrastive.py:304-310).
//
// The dilated k=3 convolutions run as GEMMs over the taps that can touch data: per axis of extent n an off-centre offset +-d
// reads only padding unless d < n, so the live taps are the product over axes of {0} u {+-d : d < n} (the host plans them from
// the shape).  The live taps of all branches become the K blocks of one GEMM on the existing MFMA path (dycon_conv_gemm, 1x1):
//   A = [x shifted by tap 0 | x shifted by tap 1 | ...]   (dycon_tap_gather; the centre tap is x itself)
//   B = block table of the branches' weights, one 256-column block per branch (dycon_pack_wblocks; blocks a branch does not
//       have stay zero)
// Data gradient: the same GEMM on the output gradient gathered at the negated offsets, B = the branches' transposed taps (one fp32
// accumulation and one rounding, like the forward).
// Weight gradient: dense A^T * gy (dycon_conv_wgrad, 1x1), then dycon_unpack_wgrad writes every branch's (Co, Ci, 3, 3, 3)
// gradient, zeros on the pruned taps.
// The pool branch is constant over space: its share of conv1 is a per-sample bias (dycon_small_gemm + dycon_sample_bcast),
// its backward a per-sample column sum (dycon_sample_colsum).
#include "common.h"

// ------------------------------------------------------------------------------------------------ tap gather / scatter
struct TapTable {
    int n;
    int dz[DYCON_TAPS_MAX], dy[DYCON_TAPS_MAX], dx[DYCON_TAPS_MAX];
};

template <typename T>
__device__ __forceinline__ Vec16<T> zero16() {
    Vec16<T> v;
#pragma unroll
    for (int e = 0; e < Vec16<T>::N; ++e) v.set(e, 0.f);
    return v;
}

// Y[row][t*C + c] = X[row shifted by tap t][c], zero outside the grid
template <typename T>
__global__ __launch_bounds__(256) void tap_gather_kernel(const T* __restrict__ X, T* __restrict__ Y, int D, int H, int W, int C,
                                                         TapTable tt, long long total) {
    constexpr int VN = Vec16<T>::N;
    const int cv = C / VN;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c8 = (int)(i % cv);
        long long q = i / cv;
        const int t = (int)(q % tt.n);
        long long r = q / tt.n;
        const int x = (int)(r % W); r /= W;
        const int y = (int)(r % H); r /= H;
        const int z = (int)(r % D);
        const long long b = r / D;
        const int zi = z + tt.dz[t], yi = y + tt.dy[t], xi = x + tt.dx[t];
        Vec16<T> v = zero16<T>();
        if ((unsigned)zi < (unsigned)D && (unsigned)yi < (unsigned)H && (unsigned)xi < (unsigned)W)
            v = ld16(X + (((b * D + zi) * H + yi) * W + xi) * C + c8 * VN);
        st16(Y + i * VN, v);
    }
}

static int tap_table(const int* taps_host, int ntaps, TapTable& tt) {
    DYCON_REQUIRE(taps_host && ntaps > 0 && ntaps <= DYCON_TAPS_MAX, "tap table: 1..%d taps", DYCON_TAPS_MAX);
    tt.n = ntaps;
    for (int t = 0; t < ntaps; ++t) {
        tt.dz[t] = taps_host[3 * t];
        tt.dy[t] = taps_host[3 * t + 1];
        tt.dx[t] = taps_host[3 * t + 2];
    }
    return DYCON_OK;
}

static int vec_of(int dtype) { return dtype == DYCON_BF16 ? 8 : 4; }

extern "C" int dycon_tap_gather(const void* x, void* y, int dtype, int B, int D, int H, int W, int C, const int* taps_host, int ntaps,
                                dycon_stream_t stream) {
    DYCON_REQUIRE(x && y && B > 0 && D > 0 && H > 0 && W > 0 && C > 0, "tap_gather: bad arguments");
    DYCON_REQUIRE(dtype == DYCON_F32 || dtype == DYCON_BF16, "tap_gather: bad dtype %d", dtype);
    DYCON_REQUIRE(C % vec_of(dtype) == 0, "tap_gather: C must be a multiple of %d", vec_of(dtype));
    TapTable tt;
    if (tap_table(taps_host, ntaps, tt)) return DYCON_ERR_INVALID;
    const long long total = (long long)B * D * H * W * ntaps * (C / vec_of(dtype));
    const int grid = cdiv(total, 256) > 8192 ? 8192 : cdiv(total, 256);
    DYCON_DISPATCH(dtype, tap_gather_kernel<T><<<grid, 256, 0, stream>>>((const T*)x, (T*)y, D, H, W, C, tt, total));
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

// ------------------------------------------------------------------------------------------------ block-table weight packing
struct WBlocks {
    const float* w[DYCON_WBLK_SRC_MAX];
    long long sk[DYCON_WBLK_SRC_MAX], sn[DYCON_WBLK_SRC_MAX];
    short blk[DYCON_WBLK_MAX];      // (k block, n block) -> src * 32 + tap, or -1 (zero block)
};

// same fragment order as pack_bfrag_kernel (conv.hip) with T = 1, Cin = KB * kblk, N = NB * nblk
template <typename T, int G, int KC>
__global__ __launch_bounds__(256) void pack_wblocks_kernel(WBlocks wb, T* __restrict__ out, int KB, int NB, int kblk, int nblk, int NT,
                                                           long long total) {
    const int K = KB * kblk, N = NB * nblk;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int e = (int)(i % G);
        long long q = i / G;
        const int lane = (int)(q % 64);
        q /= 64;
        const int nt = (int)(q % NT);
        const int kc = (int)(q / NT);
        const int k = kc * KC + G * (lane >> 4) + e;
        const int n = nt * 16 + (lane & 15);
        float v = 0.f;
        if (k < K && n < N) {
            const int b = wb.blk[(k / kblk) * NB + n / nblk];
            if (b >= 0) {
                const int s = b >> 5, tap = b & 31;
                v = wb.w[s][tap + (long long)(k % kblk) * wb.sk[s] + (long long)(n % nblk) * wb.sn[s]];
            }
        }
        stf(out + i, v);
    }
}

extern "C" int dycon_pack_wblocks(const float* const* w_host, const long long* strides_host, int nsrc, const short* blk_host, int KB,
                                  int NB, int kblk, int nblk, void* out, size_t out_bytes, int dtype, dycon_stream_t stream) {
    DYCON_REQUIRE(w_host && strides_host && blk_host && out, "pack_wblocks: null pointer");
    DYCON_REQUIRE(nsrc > 0 && nsrc <= DYCON_WBLK_SRC_MAX, "pack_wblocks: 1..%d sources", DYCON_WBLK_SRC_MAX);
    DYCON_REQUIRE(KB > 0 && NB > 0 && KB * NB <= DYCON_WBLK_MAX && kblk > 0 && nblk > 0, "pack_wblocks: bad block grid");
    DYCON_REQUIRE(dtype == DYCON_F32 || dtype == DYCON_BF16, "pack_wblocks: bad dtype %d", dtype);
    DYCON_REQUIRE(out_bytes >= dycon_bfrag_bytes(dtype, 1, KB * kblk, NB * nblk), "pack_wblocks: output too small");
    WBlocks wb;
    for (int s = 0; s < DYCON_WBLK_SRC_MAX; ++s) {
        wb.w[s] = s < nsrc ? w_host[s] : nullptr;
        wb.sk[s] = s < nsrc ? strides_host[2 * s] : 0;
        wb.sn[s] = s < nsrc ? strides_host[2 * s + 1] : 0;
    }
    for (int i = 0; i < KB * NB; ++i) {
        const int b = blk_host[i];
        DYCON_REQUIRE(b == -1 || (b >= 0 && (b >> 5) < nsrc && (b & 31) < 27 && w_host[b >> 5]), "pack_wblocks: bad block entry %d", b);
        wb.blk[i] = (short)b;
    }
    const int NT = (NB * nblk + 15) / 16;
    if (dtype == DYCON_BF16) {
        const long long total = (((long long)KB * kblk + 31) / 32) * NT * 64 * 8;
        const int grid = cdiv(total, 256) > 4096 ? 4096 : cdiv(total, 256);
        pack_wblocks_kernel<bf16, 8, 32><<<grid, 256, 0, stream>>>(wb, (bf16*)out, KB, NB, kblk, nblk, NT, total);
    } else {
        const long long total = (((long long)KB * kblk + 15) / 16) * NT * 64 * 4;
        const int grid = cdiv(total, 256) > 4096 ? 4096 : cdiv(total, 256);
        pack_wblocks_kernel<float, 4, 16><<<grid, 256, 0, stream>>>(wb, (float*)out, KB, NB, kblk, nblk, NT, total);
    }
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

// ------------------------------------------------------------------------------------------------ weight-gradient unpack
struct WDest {
    float* g[DYCON_WBLK_SRC_MAX];
    int T[DYCON_WBLK_SRC_MAX];
    short kb[DYCON_WBLK_SRC_MAX][27];     // k block holding (dest, tap), -1: pruned tap (written as 0)
};

// g_j[co][ci][tap] = dense[(kb * Ci + ci) * ldd + j * Co + co]
__global__ __launch_bounds__(256) void unpack_wgrad_kernel(const float* __restrict__ dense, long long ldd, WDest d, int Ci, int Co) {
    const int j = blockIdx.y;
    const int Tn = d.T[j];
    const long long total = (long long)Co * Ci * Tn;
    float* g = d.g[j];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int tap = (int)(i % Tn);
        const long long q = i / Tn;
        const int ci = (int)(q % Ci);
        const int co = (int)(q / Ci);
        const int kb = d.kb[j][tap];
        g[i] = kb >= 0 ? dense[((long long)kb * Ci + ci) * ldd + (long long)j * Co + co] : 0.f;
    }
}

extern "C" int dycon_unpack_wgrad(const float* dense, long long ldd, int KB, float* const* g_host, const int* taps_host,
                                  const short* kb_host, int ndst, int Ci, int Co, dycon_stream_t stream) {
    DYCON_REQUIRE(dense && g_host && taps_host && kb_host, "unpack_wgrad: null pointer");
    DYCON_REQUIRE(ndst > 0 && ndst <= DYCON_WBLK_SRC_MAX && Ci > 0 && Co > 0, "unpack_wgrad: bad arguments");
    DYCON_REQUIRE(ldd >= (long long)ndst * Co, "unpack_wgrad: ldd < ndst * Co");
    WDest d;
    for (int j = 0; j < DYCON_WBLK_SRC_MAX; ++j) {
        d.g[j] = j < ndst ? g_host[j] : nullptr;
        d.T[j] = j < ndst ? taps_host[j] : 1;
        for (int t = 0; t < 27; ++t) {
            const int kb = j < ndst && t < d.T[j] ? kb_host[j * 27 + t] : -1;
            DYCON_REQUIRE(kb >= -1 && kb < KB, "unpack_wgrad: bad k block %d", kb);
            d.kb[j][t] = (short)kb;
        }
        if (j < ndst) DYCON_REQUIRE(d.g[j] && (d.T[j] == 1 || d.T[j] == 27), "unpack_wgrad: destination %d needs 1 or 27 taps", j);
    }
    const int grid = cdiv((long long)Co * Ci * 27, 256) > 1024 ? 1024 : cdiv((long long)Co * Ci * 27, 256);
    unpack_wgrad_kernel<<<dim3(grid, ndst), 256, 0, stream>>>(dense, ldd, d, Ci, Co);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

// ------------------------------------------------------------------------------------------------ per-sample reductions
// out[b][c] (+)= scale * sum_v X[b][v][c]: 16 channels x 16 row lanes per workgroup, fixed summation order
template <typename T>
__global__ __launch_bounds__(256) void sample_colsum_kernel(const T* __restrict__ X, float* __restrict__ out, long long V, int C,
                                                            float scale, int accumulate) {
    __shared__ float part[16][16];
    const int b = blockIdx.y, cl = threadIdx.x & 15, r0 = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    float s = 0.f;
    if (c < C)
        for (long long v = r0; v < V; v += 16) s += ldf(X + ((long long)b * V + v) * C + c);
    part[r0][cl] = s;
    __syncthreads();
    if (r0 == 0 && c < C) {
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += part[r][cl];
        t *= scale;
        out[(long long)b * C + c] = accumulate ? out[(long long)b * C + c] + t : t;
    }
}

extern "C" int dycon_sample_colsum(const void* x, int dtype, float* out, int B, long long V, int C, float scale, int accumulate,
                                   dycon_stream_t stream) {
    DYCON_REQUIRE(x && out && B > 0 && V > 0 && C > 0 && B <= 65535, "sample_colsum: bad arguments");
    DYCON_DISPATCH(dtype, sample_colsum_kernel<T><<<dim3(cdiv(C, 16), B), 256, 0, stream>>>((const T*)x, out, V, C, scale, accumulate));
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

// Y[b][v][c] = (X ? X[b][v][c] : 0) + scale * vec[b][c]   (X may alias Y)
template <typename T>
__global__ __launch_bounds__(256) void sample_bcast_kernel(const T* X, const float* __restrict__ vec, T* Y, long long V, int C,
                                                           float scale, long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long b = i / ((long long)V * C);
        const float base = X ? ldf(X + i) : 0.f;
        stf(Y + i, base + scale * vec[b * C + c]);
    }
}

extern "C" int dycon_sample_bcast(const void* x, const float* vec, void* y, int dtype, int B, long long V, int C, float scale,
                                  dycon_stream_t stream) {
    DYCON_REQUIRE(vec && y && B > 0 && V > 0 && C > 0, "sample_bcast: bad arguments");
    const long long total = (long long)B * V * C;
    const int grid = cdiv(total, 256) > 8192 ? 8192 : cdiv(total, 256);
    DYCON_DISPATCH(dtype, sample_bcast_kernel<T><<<grid, 256, 0, stream>>>((const T*)x, vec, (T*)y, V, C, scale, total));
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

// C[i*ldc + j] (+)= sum_r A[r*sar + i*sai] * B[r*sbr + j*sbj]   (fp32; the pool branch's (B x 256) products): one wave per output,
// its lanes take r = lane, lane + 64, ... and the butterfly sum closes it -- a fixed order, bitwise reproducible
__global__ __launch_bounds__(256) void small_gemm_kernel(const float* __restrict__ A, long long sar, long long sai,
                                                         const float* __restrict__ Bm, long long sbr, long long sbj, float* __restrict__ Cm,
                                                         long long ldc, int I, int J, int R, int accumulate) {
    const long long idx = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (idx >= (long long)I * J) return;
    const int i = (int)(idx / J), j = (int)(idx % J);
    float s = 0.f;
    for (int r = lane; r < R; r += 64) s = fmaf(A[r * sar + i * sai], Bm[r * sbr + j * sbj], s);
    s = wave_sum(s);
    if (lane == 0) {
        float* c = Cm + i * ldc + j;
        *c = accumulate ? *c + s : s;
    }
}

extern "C" int dycon_small_gemm(const float* a, long long sar, long long sai, const float* b, long long sbr, long long sbj, float* c,
                                long long ldc, int I, int J, int R, int accumulate, dycon_stream_t stream) {
    DYCON_REQUIRE(a && b && c && I > 0 && J > 0 && R > 0 && ldc >= J, "small_gemm: bad arguments");
    small_gemm_kernel<<<cdiv((long long)I * J, 4), 256, 0, stream>>>(a, sar, sai, b, sbr, sbj, c, ldc, I, J, R, accumulate);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

// ------------------------------------------------------------------------------------------------ vector segments
struct Segs {
    const float* src[DYCON_SEGS_MAX];
    float* dst[DYCON_SEGS_MAX];
    int n[DYCON_SEGS_MAX];
};

__global__ __launch_bounds__(256) void copy_segments_kernel(Segs s) {
    const int k = blockIdx.y;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < s.n[k]; i += gridDim.x * 256) s.dst[k][i] = s.src[k][i];
}

extern "C" int dycon_copy_segments(const float* const* src_host, float* const* dst_host, const int* n_host, int nseg,
                                   dycon_stream_t stream) {
    DYCON_REQUIRE(src_host && dst_host && n_host && nseg > 0 && nseg <= DYCON_SEGS_MAX, "copy_segments: 1..%d segments", DYCON_SEGS_MAX);
    Segs s;
    int nmax = 0;
    for (int k = 0; k < DYCON_SEGS_MAX; ++k) {
        s.src[k] = k < nseg ? src_host[k] : nullptr;
        s.dst[k] = k < nseg ? dst_host[k] : nullptr;
        s.n[k] = k < nseg ? n_host[k] : 0;
        if (k < nseg) DYCON_REQUIRE(s.src[k] && s.dst[k] && s.n[k] >= 0, "copy_segments: bad segment %d", k);
        if (s.n[k] > nmax) nmax = s.n[k];
    }
    if (nmax == 0) return DYCON_OK;
    copy_segments_kernel<<<dim3(cdiv(nmax, 256), nseg), 256, 0, stream>>>(s);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}
