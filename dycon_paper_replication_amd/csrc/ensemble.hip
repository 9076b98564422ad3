// Model-ensemble sliding-window evaluation on the device: code/utils/test_3d_patch.py:415-476 (test_single_case_plus).
//
// The reference runs every window through two models, averages their logits ((y1_l + y1_r) / 2, :460-462), takes the softmax and
// accumulates class 1 into score / count maps on the host.  Two kernels serve that loop here:
//   - sw_gather_kernel builds the (n, 1, p0, p1, p2) batch of windows of one chunk in one launch from the UNPADDED volume and a
//     table of window origins that was uploaded once per case.  The centre pad of a volume smaller than the window (:418-439) is
//     index arithmetic: the origins are in padded coordinates, a source index outside the stored volume reads as 0 (the convention
//     of csrc/datapath.hip).  A pure copy: bit for bit the slices of the zero-padded volume.
//   - sw_accumulate_ens_kernel is the voxel-centric accumulate of csrc/eval.hip (fixed window order, no atomics) over M = 2..4
//     models: per covered voxel and class the logits are summed in model order in fp32, divided by M, and class 1 of the softmax is
//     scored with the expressions of sw_accumulate_kernel (C == 2) and sw_accumulate_c_kernel (C > 2).  (a + a) / 2 == a in fp32, so
//     an ensemble of a model with itself gives the single-model kernels' bits.
// Both are bandwidth-bound passes with coalesced access along the last axis and nothing else was tuned.  dycon_sw_finalize (eval.hip)
// turns the maps into the label and the probability.
#include "common.h"

// blockIdx.y = window of the chunk; blockIdx.x strides over its p0 * p1 rows x G groups of 4 elements of the last axis
__global__ __launch_bounds__(256) void sw_gather_kernel(const float* __restrict__ vol, int w, int h, int d, int lo0, int lo1, int lo2,
                                                        const int* __restrict__ origins, int p0, int p1, int p2, int G, int vec,
                                                        float* __restrict__ out) {
    const int* o = origins + 3 * blockIdx.y;
    // window corner in stored coordinates (negative inside the pad).  64-bit: the table is device data, and no value in it may wrap
    // a source index back into the volume
    const long long ox = (long long)o[0] - lo0, oy = (long long)o[1] - lo1, oz = (long long)o[2] - lo2;
    const long long per = (long long)p0 * p1 * G;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long long)gridDim.x * 256) {
        const int g = (int)(e % G);
        const int row = (int)(e / G);
        const int j = row % p1, i = row / p1;
        const long long sx = ox + i, sy = oy + j;
        const int z0 = 4 * g;
        const long long sz0 = oz + z0;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (sx >= 0 && sx < w && sy >= 0 && sy < h) {
            const float* ip = vol + (sx * h + sy) * d;
            if (sz0 >= 0 && sz0 <= d - 4 && z0 + 3 < p2) {
                __builtin_memcpy(v, ip + sz0, 16);                    // the run starts at an arbitrary element: no alignment promised
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (z0 + t < p2 && sz0 + t >= 0 && sz0 + t < d) v[t] = ip[sz0 + t];
            }
        }
        const long long q = (((long long)blockIdx.y * p0 + i) * p1 + j) * p2 + z0;
        if (vec) {
            *reinterpret_cast<float4*>(out + q) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (z0 + t < p2) out[q + t] = v[t];
        }
    }
}

extern "C" int dycon_sw_gather(const float* vol, int w, int h, int d, const int* origins_dev, int n_origins, int first, int n, int p0,
                               int p1, int p2, float* out, dycon_stream_t stream) {
    DYCON_REQUIRE(vol && origins_dev && out, "sw_gather: null pointer");
    const int lim = 1 << 30;
    DYCON_REQUIRE(w > 0 && h > 0 && d > 0 && w < lim && h < lim && d < lim, "sw_gather: volume %d x %d x %d", w, h, d);
    DYCON_REQUIRE(p0 > 0 && p1 > 0 && p2 > 0 && p0 < lim && p1 < lim && p2 < lim && (long long)p0 * p1 <= 0x7fffffffLL,
                  "sw_gather: window %d x %d x %d", p0, p1, p2);
    DYCON_REQUIRE(n >= 1 && n <= 64 && first >= 0 && n_origins >= 1 && first <= n_origins - n,
                  "sw_gather: windows [%d, %d + %d) of a table of %d (1..64 per launch)", first, first, n, n_origins);
    // :418-439: an axis shorter than the window is centre-padded, the smaller half in front
    const int lo0 = (p0 > w ? p0 - w : 0) / 2, lo1 = (p1 > h ? p1 - h : 0) / 2, lo2 = (p2 > d ? p2 - d : 0) / 2;
    const int G = (p2 + 3) / 4;
    const int vec = p2 % 4 == 0 && (uintptr_t)out % 16 == 0;
    const long long per = (long long)p0 * p1 * G;
    const dim3 grid(cdiv(per, 256) > 1024 ? 1024 : cdiv(per, 256), n);
    sw_gather_kernel<<<grid, 256, 0, stream>>>(vol, w, h, d, lo0, lo1, lo2, origins_dev + 3 * (long long)first, p0, p1, p2, G, vec, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

struct EnsLogits {
    const float* l[4];
};

// mean over the models of logit k of one voxel of one window: ((l0 + l1) + l2) + l3, then / M
template <int M> __device__ __forceinline__ float ens_mean(const EnsLogits& in, long long at) {
    float x = in.l[0][at] + in.l[1][at];
    if constexpr (M > 2) x += in.l[2][at];
    if constexpr (M > 3) x += in.l[3][at];
    return x / (float)M;
}

template <int M>
__global__ __launch_bounds__(256) void sw_accumulate_ens_kernel(EnsLogits in, int C, int nb, int p0, int p1, int p2,
                                                                const int* __restrict__ origins, float* __restrict__ score,
                                                                float* __restrict__ cnt, int D0, int D1, int D2) {
    __shared__ int org[3 * 64];
    for (int i = threadIdx.x; i < 3 * nb; i += 256) org[i] = origins[i];
    __syncthreads();
    const long long total = (long long)D0 * D1 * D2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % D2);
        const long long q = i / D2;
        const int b_ = (int)(q % D1), a = (int)(q / D1);
        float s = 0.f, n = 0.f;
        for (int p = 0; p < nb; ++p) {
            const int la = a - org[3 * p], lb = b_ - org[3 * p + 1], lc = c - org[3 * p + 2];
            if ((unsigned)la < (unsigned)p0 && (unsigned)lb < (unsigned)p1 && (unsigned)lc < (unsigned)p2) {
                const long long at = ((((long long)p * p0 + la) * p1 + lb) * p2 + lc) * C;
                if (C == 2) {
                    const float x0 = ens_mean<M>(in, at), x1 = ens_mean<M>(in, at + 1);
                    s += 1.f / (1.f + __expf(x0 - x1));      // softmax(mean logits)[1]: the expression of sw_accumulate_kernel
                } else {
                    float x[8], m = -INFINITY, z = 0.f;       // the max-shifted form of sw_accumulate_c_kernel
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k < C) { x[k] = ens_mean<M>(in, at + k); m = fmaxf(m, x[k]); }
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k < C) { x[k] = expf(x[k] - m); z += x[k]; }
                    s += x[1] / z;
                }
                n += 1.f;
            }
        }
        if (n > 0.f) { score[i] += s; cnt[i] += n; }
    }
}

extern "C" int dycon_sw_accumulate_ens(const float* logits0, const float* logits1, const float* logits2, const float* logits3, int M,
                                       int C, int n_patches, int p0, int p1, int p2, const int* origins_dev, float* score, float* cnt,
                                       int D0, int D1, int D2, dycon_stream_t stream) {
    DYCON_REQUIRE(M >= 2 && M <= 4, "sw_accumulate_ens: M = %d models (2..4)", M);
    DYCON_REQUIRE(C >= 2 && C <= 8, "sw_accumulate_ens: C = %d (2..8: class 1 is scored)", C);
    EnsLogits in = {{logits0, logits1, logits2, logits3}};
    for (int m = 0; m < M; ++m) DYCON_REQUIRE(in.l[m], "sw_accumulate_ens: logits of model %d are null (M = %d)", m, M);
    for (int m = M; m < 4; ++m) in.l[m] = nullptr;
    DYCON_REQUIRE(origins_dev && score && cnt, "sw_accumulate_ens: null pointer");
    DYCON_REQUIRE(n_patches > 0 && n_patches <= 64 && p0 > 0 && p1 > 0 && p2 > 0 && D0 >= p0 && D1 >= p1 && D2 >= p2,
                  "sw_accumulate_ens: bad shape (%d patches of %dx%dx%d in %dx%dx%d)", n_patches, p0, p1, p2, D0, D1, D2);
    long long blocks = ((long long)D0 * D1 * D2 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (M == 2)
        sw_accumulate_ens_kernel<2><<<(int)blocks, 256, 0, stream>>>(in, C, n_patches, p0, p1, p2, origins_dev, score, cnt, D0, D1, D2);
    else if (M == 3)
        sw_accumulate_ens_kernel<3><<<(int)blocks, 256, 0, stream>>>(in, C, n_patches, p0, p1, p2, origins_dev, score, cnt, D0, D1, D2);
    else
        sw_accumulate_ens_kernel<4><<<(int)blocks, 256, 0, stream>>>(in, C, n_patches, p0, p1, p2, origins_dev, score, cnt, D0, D1, D2);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}
