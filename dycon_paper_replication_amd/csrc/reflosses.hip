// The reference's loss callables with the reference's OWN argument meaning (code/utils/losses.py:8-16, 65-104, 156-192):
// probabilities (or any float tensor) in, element-wise tensor / scalar out.  The fused step (trainer.py) does not use these -- it
// reads the logits once (losses.hip) -- they exist so that the reference's training-loop body runs unchanged on this package
// (INTEGRATION.md section 1).  All are streaming kernels over a strided (n, C, V) view: channel stride 1 for the package's
// channels-last tensors, channel stride V for a plain NCDHW tensor, element stride 2 for `probs[:, 1]` of a 2-class map.
#include "common.h"

constexpr int MAXC = 8;

struct View { const float* p; long long sn, sc, sv; };
static inline View mkview(const dycon_view_t* v) { return View{(const float*)v->p, v->sn, v->sc, v->sv}; }

template <int DUMMY = 0>
__device__ __forceinline__ void load_probs(const View& a, long long n, long long v, int C, int sigmoid, float* p, float* lp) {
    // p = softmax over the C channels (or element-wise sigmoid); lp = log p
    const float* base = a.p + n * a.sn + v * a.sv;
    float x[MAXC], m = -INFINITY;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) { x[c] = base[c * a.sc]; m = fmaxf(m, x[c]); }
    if (sigmoid) {
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) { p[c] = 1.f / (1.f + expf(-x[c])); lp[c] = logf(p[c]); }
        return;
    }
    float z = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) { p[c] = expf(x[c] - m); z += p[c]; }
    const float lz = logf(z);
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) { lp[c] = x[c] - m - lz; p[c] = p[c] / z; }
}

// ------------------------------------------------------------------ softmax_mse_loss (losses.py:65-82): element-wise (p - q)^2
__global__ __launch_bounds__(256) void softmax_mse_fwd_kernel(View a, View b, float* __restrict__ out, long long osn, long long osc,
                                                              long long osv, long long n_, int C, long long V, int sigmoid) {
    const long long total = n_ * V;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / V, v = i - n * V;
        float p[MAXC], q[MAXC], lp[MAXC];
        load_probs(a, n, v, C, sigmoid, p, lp);
        load_probs(b, n, v, C, sigmoid, q, lp);
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) { const float d = p[c] - q[c]; out[n * osn + c * osc + v * osv] = d * d; }
    }
}

// gradient w.r.t. the FIRST argument (the loss is symmetric: call with (b, a) for the second)
__global__ __launch_bounds__(256) void softmax_mse_bwd_kernel(View a, View b, View g, float* __restrict__ ga, long long osn,
                                                              long long osc, long long osv, long long n_, int C, long long V,
                                                              int sigmoid) {
    const long long total = n_ * V;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / V, v = i - n * V;
        float p[MAXC], q[MAXC], lp[MAXC], h[MAXC];
        load_probs(a, n, v, C, sigmoid, p, lp);
        load_probs(b, n, v, C, sigmoid, q, lp);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) { h[c] = 2.f * g.p[n * g.sn + c * g.sc + v * g.sv] * (p[c] - q[c]); dot += h[c] * p[c]; }
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) ga[n * osn + c * osc + v * osv] = sigmoid ? h[c] * p[c] * (1.f - p[c]) : p[c] * (h[c] - dot);
    }
}

// ------------------------------------------------------------------ softmax_kl_loss (losses.py:85-104): F.kl_div(log p, q, 'mean')
__device__ __forceinline__ void block_atomic_double(float v, double* dst) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = wave_sum(v);
    if (lane == 0) red[w] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(dst, (double)red[0] + (double)red[1] + (double)red[2] + (double)red[3]);
    __syncthreads();
}

__global__ __launch_bounds__(256) void softmax_kl_fwd_kernel(View a, View b, long long n_, int C, long long V, int sigmoid,
                                                             double* __restrict__ sum) {
    const long long total = n_ * V;
    float acc = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / V, v = i - n * V;
        float p[MAXC], q[MAXC], lp[MAXC], lq[MAXC];
        load_probs(a, n, v, C, sigmoid, p, lp);
        load_probs(b, n, v, C, sigmoid, q, lq);
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) acc += q[c] > 0.f ? q[c] * (lq[c] - lp[c]) : 0.f;     // xlogy: 0 where the target is 0
    }
    block_atomic_double(acc, sum);
}

__global__ void scalar_mean_kernel(const double* __restrict__ sum, double count, float* __restrict__ out) {
    out[0] = (float)(sum[0] / count);
}

// which = 0: d/d input logits = g/count * (p * sum(q) - q)   (sigmoid: -q (1 - p));
// which = 1: d/d target logits = g/count * q (r - sum q r), r = log q - log p + 1   (sigmoid: q (1-q) r)
__global__ __launch_bounds__(256) void softmax_kl_bwd_kernel(View a, View b, long long n_, int C, long long V, int sigmoid,
                                                             int which, const float* __restrict__ g_up, double count,
                                                             float* __restrict__ gr, long long osn, long long osc, long long osv) {
    const long long total = n_ * V;
    const float s = g_up[0] / (float)count;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / V, v = i - n * V;
        float p[MAXC], q[MAXC], lp[MAXC], lq[MAXC];
        load_probs(a, n, v, C, sigmoid, p, lp);
        load_probs(b, n, v, C, sigmoid, q, lq);
        float qs = 0.f, qr = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) { qs += q[c]; qr += q[c] * (lq[c] - lp[c] + 1.f); }
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) {
                float r;
                if (which == 0) r = sigmoid ? -q[c] * (1.f - p[c]) : p[c] * qs - q[c];
                else {
                    const float rc = lq[c] - lp[c] + 1.f;
                    r = sigmoid ? q[c] * (1.f - q[c]) * rc : q[c] * (rc - qr);
                }
                gr[n * osn + c * osc + v * osv] = s * r;
            }
    }
}

// ------------------------------------------------------------------ dice_loss / DiceLoss (losses.py:8-16, 156-192)
// target kinds: 0 float32, 1 one byte (uint8 / bool), 2 int64.  onehot = 1: the target is a label map (n, V) and class c's target is
// (label == c) (DiceLoss._one_hot_encoder); onehot = 0: the target has the score's logical shape and is used as is (dice_loss).
__device__ __forceinline__ float load_target(const void* t, int kind, long long off) {
    return kind == 0 ? ((const float*)t)[off] : kind == 1 ? (float)((const uint8_t*)t)[off] : (float)((const long long*)t)[off];
}

__device__ __forceinline__ void load_scores(const View& a, long long n, long long v, int C, int softmax, float* s) {
    if (softmax) {
        float lp[MAXC];
        load_probs(a, n, v, C, 0, s, lp);
    } else {
        const float* base = a.p + n * a.sn + v * a.sv;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) s[c] = base[c * a.sc];
    }
}

__global__ __launch_bounds__(256) void dice_sums_kernel(View a, const void* __restrict__ tgt, int tkind, int onehot, long long tsn,
                                                        long long tsc, long long tsv, long long n_, int C, long long V, int softmax,
                                                        double* __restrict__ sums) {
    __shared__ float red[4][MAXC * 3];
    float acc[MAXC * 3];
#pragma unroll
    for (int k = 0; k < MAXC * 3; ++k) acc[k] = 0.f;
    const long long total = n_ * V;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / V, v = i - n * V;
        float s[MAXC];
        load_scores(a, n, v, C, softmax, s);
        const float lab = onehot ? load_target(tgt, tkind, n * tsn + v * tsv) : 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) {
                const float t = onehot ? (lab == (float)c ? 1.f : 0.f) : load_target(tgt, tkind, n * tsn + c * tsc + v * tsv);
                acc[3 * c] += s[c] * t; acc[3 * c + 1] += s[c] * s[c]; acc[3 * c + 2] += t * t;
            }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < MAXC * 3; ++k) {
        const float v = wave_sum(acc[k]);
        if (lane == 0) red[w][k] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < 3 * C) {
        const int k = threadIdx.x;
        atomicAdd(&sums[k], (double)red[0][k] + (double)red[1][k] + (double)red[2][k] + (double)red[3][k]);
    }
}

struct Weights { float w[MAXC]; };

// loss = sum_c w_c (1 - (2 I_c + smooth) / (Z_c + Y_c + smooth)) / n_div
__global__ void dice_finalize_kernel(const double* __restrict__ sums, int C, Weights wt, float n_div, float* __restrict__ out) {
    const float smooth = 1e-5f;
    float loss = 0.f;
    for (int c = 0; c < C; ++c) {
        const float I = (float)sums[3 * c], Z = (float)sums[3 * c + 1], Y = (float)sums[3 * c + 2];
        loss += wt.w[c] * (1.f - (2.f * I + smooth) / (Z + Y + smooth));
    }
    out[0] = loss / n_div;
}

__global__ __launch_bounds__(256) void dice_bwd_kernel(View a, const void* __restrict__ tgt, int tkind, int onehot, long long tsn,
                                                       long long tsc, long long tsv, long long n_, int C, long long V, int softmax,
                                                       const double* __restrict__ sums, const float* __restrict__ g_up, Weights wt,
                                                       float n_div, float* __restrict__ gr, long long osn, long long osc,
                                                       long long osv) {
    const float smooth = 1e-5f;
    float I2[MAXC], D[MAXC], k[MAXC];
    const float gu = g_up[0] / n_div;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) {
            I2[c] = 2.f * (float)sums[3 * c] + smooth;
            D[c] = (float)sums[3 * c + 1] + (float)sums[3 * c + 2] + smooth;
            k[c] = gu * wt.w[c];
        }
    const long long total = n_ * V;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / V, v = i - n * V;
        float s[MAXC], h[MAXC];
        load_scores(a, n, v, C, softmax, s);
        const float lab = onehot ? load_target(tgt, tkind, n * tsn + v * tsv) : 0.f;
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) {
                const float t = onehot ? (lab == (float)c ? 1.f : 0.f) : load_target(tgt, tkind, n * tsn + c * tsc + v * tsv);
                h[c] = -k[c] * (2.f * t * D[c] - I2[c] * 2.f * s[c]) / (D[c] * D[c]);
                dot += h[c] * s[c];
            }
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) gr[n * osn + c * osc + v * osv] = softmax ? s[c] * (h[c] - dot) : h[c];
    }
}

// ------------------------------------------------------------------ host entry points
static inline int grid_for(long long total) {
    long long b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
#define CHECK_VIEW(v) DYCON_REQUIRE((v) && (v)->p, "null view")
#define CHECK_DIMS() DYCON_REQUIRE(n >= 0 && V >= 0 && C >= 1 && C <= MAXC, "bad dims n=%lld C=%d V=%lld (1 <= C <= %d)", n, C, V, MAXC)

extern "C" int dycon_softmax_mse_fwd(const dycon_view_t* a, const dycon_view_t* b, const dycon_view_t* out, long long n, int C,
                                     long long V, int sigmoid, dycon_stream_t stream) {
    CHECK_VIEW(a); CHECK_VIEW(b); CHECK_VIEW(out); CHECK_DIMS();
    if (n * V == 0) return DYCON_OK;
    softmax_mse_fwd_kernel<<<grid_for(n * V), 256, 0, stream>>>(mkview(a), mkview(b), (float*)out->p, out->sn, out->sc, out->sv, n, C, V,
                                                                sigmoid);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_softmax_mse_bwd(const dycon_view_t* a, const dycon_view_t* b, const dycon_view_t* g, const dycon_view_t* ga,
                                     long long n, int C, long long V, int sigmoid, dycon_stream_t stream) {
    CHECK_VIEW(a); CHECK_VIEW(b); CHECK_VIEW(g); CHECK_VIEW(ga); CHECK_DIMS();
    if (n * V == 0) return DYCON_OK;
    softmax_mse_bwd_kernel<<<grid_for(n * V), 256, 0, stream>>>(mkview(a), mkview(b), mkview(g), (float*)ga->p, ga->sn, ga->sc, ga->sv,
                                                                n, C, V, sigmoid);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_softmax_kl_fwd(const dycon_view_t* a, const dycon_view_t* b, long long n, int C, long long V, int sigmoid,
                                    double* sum, float* out, dycon_stream_t stream) {
    CHECK_VIEW(a); CHECK_VIEW(b); CHECK_DIMS();
    DYCON_REQUIRE(sum && out && n * V > 0, "softmax_kl: empty input or null output");
    if (hipMemsetAsync(sum, 0, sizeof(double), stream) != hipSuccess) { dycon_set_error("memset failed"); return DYCON_ERR_LAUNCH; }
    softmax_kl_fwd_kernel<<<grid_for(n * V), 256, 0, stream>>>(mkview(a), mkview(b), n, C, V, sigmoid, sum);
    scalar_mean_kernel<<<1, 1, 0, stream>>>(sum, (double)n * C * V, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_softmax_kl_bwd(const dycon_view_t* a, const dycon_view_t* b, long long n, int C, long long V, int sigmoid,
                                    int which, const float* g_up, const dycon_view_t* grad, dycon_stream_t stream) {
    CHECK_VIEW(a); CHECK_VIEW(b); CHECK_VIEW(grad); CHECK_DIMS();
    DYCON_REQUIRE(g_up && (which == 0 || which == 1), "softmax_kl_bwd: bad arguments");
    if (n * V == 0) return DYCON_OK;
    softmax_kl_bwd_kernel<<<grid_for(n * V), 256, 0, stream>>>(mkview(a), mkview(b), n, C, V, sigmoid, which, g_up, (double)n * C * V,
                                                               (float*)grad->p, grad->sn, grad->sc, grad->sv);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

static inline Weights mkweights(const float* w_host, int C) {
    Weights wt;
    for (int c = 0; c < MAXC; ++c) wt.w[c] = (w_host && c < C) ? w_host[c] : 1.f;
    return wt;
}

extern "C" int dycon_dice_fwd(const dycon_view_t* score, const dycon_view_t* target, int target_kind, int onehot, long long n, int C,
                              long long V, int softmax, const float* weights_host, float n_div, double* sums, float* out,
                              dycon_stream_t stream) {
    CHECK_VIEW(score); CHECK_VIEW(target); CHECK_DIMS();
    DYCON_REQUIRE(sums && out && target_kind >= 0 && target_kind <= 2, "dice_fwd: bad arguments");
    if (hipMemsetAsync(sums, 0, sizeof(double) * 3 * MAXC, stream) != hipSuccess) { dycon_set_error("memset failed"); return DYCON_ERR_LAUNCH; }
    if (n * V > 0)
        dice_sums_kernel<<<grid_for(n * V), 256, 0, stream>>>(mkview(score), target->p, target_kind, onehot, target->sn, target->sc,
                                                              target->sv, n, C, V, softmax, sums);
    dice_finalize_kernel<<<1, 1, 0, stream>>>(sums, C, mkweights(weights_host, C), n_div, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_dice_bwd(const dycon_view_t* score, const dycon_view_t* target, int target_kind, int onehot, long long n, int C,
                              long long V, int softmax, const float* weights_host, float n_div, const double* sums, const float* g_up,
                              const dycon_view_t* grad, dycon_stream_t stream) {
    CHECK_VIEW(score); CHECK_VIEW(target); CHECK_VIEW(grad); CHECK_DIMS();
    DYCON_REQUIRE(sums && g_up && target_kind >= 0 && target_kind <= 2, "dice_bwd: bad arguments");
    if (n * V == 0) return DYCON_OK;
    dice_bwd_kernel<<<grid_for(n * V), 256, 0, stream>>>(mkview(score), target->p, target_kind, onehot, target->sn, target->sc, target->sv,
                                                         n, C, V, softmax, sums, g_up, mkweights(weights_host, C), n_div,
                                                         (float*)grad->p, grad->sn, grad->sc, grad->sv);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

// ====================================================================================================================
// The rest of the reference's utils/losses.py: dice_loss1 / softmax_dice_loss (:19-27, :39-56), the entropy family (:30-36, :59-62,
// :195-205), symmetric_mse_loss (:107-116), compute_kl_loss (:208-219) and FocalLoss (:119-153).  Same conventions as above: strided
// (n, C, V) views, fp32 in and out, every global sum in a double (one wave reduction, one atomic per block), a one-thread finalize
// that writes the fp32 scalar, nothing allocated and no host synchronisation inside an entry point.

// ------------------------------------------------------------------ dice_loss1 (losses.py:19-27) / softmax_dice_loss (:39-56)
// sums[3c..3c+2] = sum s_c t_c, sum s_c, sum t_c (PLAIN sums, not squared).  softmax = 1: both sides are logits and s, t are their
// softmax over the C channels (softmax_dice_loss); softmax = 0: C = 1 and the target may be float / one byte / int64 (dice_loss1).
__global__ __launch_bounds__(256) void dice1_sums_kernel(View a, const void* __restrict__ tgt, int tkind, long long tsn, long long tsc,
                                                         long long tsv, long long n_, int C, long long V, int softmax,
                                                         double* __restrict__ sums) {
    __shared__ float red[4][MAXC * 3];
    float acc[MAXC * 3];
#pragma unroll
    for (int k = 0; k < MAXC * 3; ++k) acc[k] = 0.f;
    const View b{(const float*)tgt, tsn, tsc, tsv};
    const long long total = n_ * V;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / V, v = i - n * V;
        float s[MAXC], t[MAXC];
        load_scores(a, n, v, C, softmax, s);
        if (softmax) load_scores(b, n, v, C, 1, t);
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) {
                const float tc = softmax ? t[c] : load_target(tgt, tkind, n * tsn + c * tsc + v * tsv);
                acc[3 * c] += s[c] * tc; acc[3 * c + 1] += s[c]; acc[3 * c + 2] += tc;
            }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < MAXC * 3; ++k) {
        const float v = wave_sum(acc[k]);
        if (lane == 0) red[w][k] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < 3 * C) {
        const int k = threadIdx.x;
        atomicAdd(&sums[k], (double)red[0][k] + (double)red[1][k] + (double)red[2][k] + (double)red[3][k]);
    }
}

// out = mean over the C classes of 1 - (2 I_c + 1e-5) / (Z_c + Y_c + 1e-5)
__global__ void dice1_finalize_kernel(const double* __restrict__ sums, int C, float* __restrict__ out) {
    double loss = 0.0;
    for (int c = 0; c < C; ++c) loss += 1.0 - (2.0 * sums[3 * c] + 1e-5) / (sums[3 * c + 1] + sums[3 * c + 2] + 1e-5);
    out[0] = (float)(loss / C);
}

// gradient w.r.t. the FIRST argument: d/ds_c = -(2 t_c D_c - (2 I_c + 1e-5)) / D_c^2 / C, through the softmax when softmax = 1.
// D = Z + Y + 1e-5 is symmetric in the two arguments: call with (b, a) and the same sums for the gradient of the second.
__global__ __launch_bounds__(256) void dice1_bwd_kernel(View a, const void* __restrict__ tgt, int tkind, long long tsn, long long tsc,
                                                        long long tsv, long long n_, int C, long long V, int softmax,
                                                        const double* __restrict__ sums, const float* __restrict__ g_up,
                                                        float* __restrict__ gr, long long osn, long long osc, long long osv) {
    float k1[MAXC], k0[MAXC];        // h_c = k1_c t_c + k0_c
    const double gu = (double)g_up[0] / C;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) {
            const double D = sums[3 * c + 1] + sums[3 * c + 2] + 1e-5;
            k1[c] = (float)(-gu * 2.0 / D);
            k0[c] = (float)(gu * (2.0 * sums[3 * c] + 1e-5) / (D * D));
        }
    const View b{(const float*)tgt, tsn, tsc, tsv};
    const long long total = n_ * V;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / V, v = i - n * V;
        float s[MAXC], t[MAXC], h[MAXC];
        if (softmax) { load_scores(a, n, v, C, 1, s); load_scores(b, n, v, C, 1, t); }
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) {
                const float tc = softmax ? t[c] : load_target(tgt, tkind, n * tsn + c * tsc + v * tsv);
                h[c] = k1[c] * tc + k0[c];
                if (softmax) dot += h[c] * s[c];
            }
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) gr[n * osn + c * osc + v * osv] = softmax ? s[c] * (h[c] - dot) : h[c];
    }
}

// ------------------------------------------------------------------ entropy_minmization / entropy_map (losses.py:195-205),
// entropy_loss / entropy_loss_map (:30-36, :59-62: the same two divided by log C).  H = -sum_c p_c log(p_c + 1e-6) of ANY float
// tensor (the reference passes probabilities).  map != NULL: map[n V + v] = scale * H; sum != NULL: sum += H.
__global__ __launch_bounds__(256) void entropy_fwd_kernel(View a, long long n_, int C, long long V, float scale, float* __restrict__ map,
                                                          double* __restrict__ sum) {
    const long long total = n_ * V;
    float acc = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / V, v = i - n * V;
        const float* base = a.p + n * a.sn + v * a.sv;
        float H = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) { const float p = base[c * a.sc]; H -= p * logf(p + 1e-6f); }
        if (map) map[i] = scale * H;
        acc += H;
    }
    if (sum) block_atomic_double(acc, sum);
}

// dH/dp_c = -(log(p_c + 1e-6) + p_c / (p_c + 1e-6)); times scale * g_map[n V + v] (map) or scale * g_up[0] / (n V) (mean)
__global__ __launch_bounds__(256) void entropy_bwd_kernel(View a, long long n_, int C, long long V, float scale,
                                                          const float* __restrict__ g_map, const float* __restrict__ g_up,
                                                          float* __restrict__ gr, long long osn, long long osc, long long osv) {
    const long long total = n_ * V;
    const float k = g_map ? scale : (float)((double)scale * (double)g_up[0] / (double)total);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / V, v = i - n * V;
        const float* base = a.p + n * a.sn + v * a.sv;
        const float kk = g_map ? k * g_map[i] : k;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) {
                const float p = base[c * a.sc], pe = p + 1e-6f;
                gr[n * osn + c * osc + v * osv] = -kk * (logf(pe) + p / pe);
            }
    }
}

// ------------------------------------------------------------------ symmetric_mse_loss (losses.py:107-116): mean((a - b)^2)
// flat views (element stride sv); 16-byte loads and stores when every stride is 1 and every pointer is 16-byte aligned
__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__global__ __launch_bounds__(256) void sym_mse_fwd_kernel(const float* __restrict__ a, long long sa, const float* __restrict__ b,
                                                          long long sb, long long total, double* __restrict__ sum) {
    float acc = 0.f;
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nth = (long long)gridDim.x * 256;
    if (sa == 1 && sb == 1 && aligned16(a) && aligned16(b)) {
        const long long n4 = total >> 2;
        for (long long i = tid; i < n4; i += nth) {
            const float4 x = ((const float4*)a)[i], y = ((const float4*)b)[i];
            const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
            acc += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
        }
        for (long long i = (n4 << 2) + tid; i < total; i += nth) { const float d = a[i] - b[i]; acc += d * d; }
    } else {
        for (long long i = tid; i < total; i += nth) { const float d = a[i * sa] - b[i * sb]; acc += d * d; }
    }
    block_atomic_double(acc, sum);
}

// ga = 2 (a - b) g_up / count: the gradient of the FIRST argument (pass (b, a) for the second)
__global__ __launch_bounds__(256) void sym_mse_bwd_kernel(const float* __restrict__ a, long long sa, const float* __restrict__ b,
                                                          long long sb, long long total, const float* __restrict__ g_up,
                                                          float* __restrict__ ga, long long sg) {
    const float k = (float)(2.0 * (double)g_up[0] / (double)total);
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nth = (long long)gridDim.x * 256;
    if (sa == 1 && sb == 1 && sg == 1 && aligned16(a) && aligned16(b) && aligned16(ga)) {
        const long long n4 = total >> 2;
        for (long long i = tid; i < n4; i += nth) {
            const float4 x = ((const float4*)a)[i], y = ((const float4*)b)[i];
            ((float4*)ga)[i] = make_float4(k * (x.x - y.x), k * (x.y - y.y), k * (x.z - y.z), k * (x.w - y.w));
        }
        for (long long i = (n4 << 2) + tid; i < total; i += nth) ga[i] = k * (a[i] - b[i]);
    } else {
        for (long long i = tid; i < total; i += nth) ga[i * sg] = k * (a[i * sa] - b[i * sb]);
    }
}

// ------------------------------------------------------------------ compute_kl_loss (losses.py:208-219)
// (KL(softmax q || softmax p) + KL(softmax p || softmax q)) / 2, each F.kl_div(..., 'none').mean(), BOTH softmaxes over the LAST
// dimension (dim=-1, not the channels).  The tensor is n C V rows (strided like a View) of L elements with element stride sl; a row
// belongs to a group of G lanes (G a power of two, 2..64: G >= L for L <= 64) and each lane holds K elements of it (K = 1 for
// L <= 64, else ceil(L / 64) rounded up to 2, 4, 8 or 16), so the supported range is 1 <= L <= 1024.  Per row
// f = sum_i (q_i - p_i) (log q_i - log p_i); loss = sum f / (2 rows L).
constexpr int KL_MAX_L = 1024;

template <int G> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int G> __device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// p = softmax, lp = log softmax of the K elements this lane holds of its row (elements j = l + k G < L)
template <int G, int K>
__device__ __forceinline__ void row_softmax(const float* __restrict__ row, long long sl, int L, int l, bool live, float* p, float* lp) {
    float x[K], m = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int j = l + k * G;
        x[k] = (live && j < L) ? row[j * sl] : -INFINITY;
        m = fmaxf(m, x[k]);
    }
    m = group_max<G>(m);
    float z = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int j = l + k * G;
        p[k] = (live && j < L) ? expf(x[k] - m) : 0.f;
        z += p[k];
    }
    z = group_sum<G>(z);
    const float lz = logf(z), rz = 1.f / z;
#pragma unroll
    for (int k = 0; k < K; ++k) { lp[k] = x[k] - m - lz; p[k] *= rz; }
}

struct Rows { long long n, C, V; };     // rows = n C V, row (in, ic, iv) starts at p + in sn + ic sc + iv sv
__device__ __forceinline__ long long row_offset(const View& a, const Rows& r, long long row) {
    const long long iv = row % r.V, t = row / r.V;
    return (t / r.C) * a.sn + (t % r.C) * a.sc + iv * a.sv;
}

template <int G, int K>
__global__ __launch_bounds__(256) void kl_rows_fwd_kernel(View a, long long sla, View b, long long slb, Rows r, int L,
                                                          double* __restrict__ sum) {
    const long long rows = r.n * r.C * r.V;
    const int l = threadIdx.x % G;
    float acc = 0.f;
    const long long ngroups = (long long)gridDim.x * (256 / G), iters = (rows + ngroups - 1) / ngroups;
    long long row = (long long)blockIdx.x * (256 / G) + threadIdx.x / G;
    for (long long it = 0; it < iters; ++it, row += ngroups) {        // every lane runs every iteration: the shuffles need the group
        const bool live = row < rows;
        const long long rr = live ? row : 0;
        float p[K], lp[K], q[K], lq[K];
        row_softmax<G, K>(a.p + row_offset(a, r, rr), sla, L, l, live, p, lp);
        row_softmax<G, K>(b.p + row_offset(b, r, rr), slb, L, l, live, q, lq);
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (live && l + k * G < L) acc += (q[k] - p[k]) * (lq[k] - lp[k]);
    }
    block_atomic_double(acc, sum);
}

// d f / d a_j = p_j (S - d_j + 1) - q_j with d = log q - log p, S = sum_i p_i d_i: the gradient of the FIRST argument (the loss is
// symmetric: pass (b, a) for the second); times g_up / (2 rows L)
template <int G, int K>
__global__ __launch_bounds__(256) void kl_rows_bwd_kernel(View a, long long sla, View b, long long slb, Rows r, int L,
                                                          const float* __restrict__ g_up, float* __restrict__ gr, View gv,
                                                          long long slg) {
    const long long rows = r.n * r.C * r.V;
    const int l = threadIdx.x % G;
    const float s = (float)((double)g_up[0] / (2.0 * (double)rows * (double)L));
    const long long ngroups = (long long)gridDim.x * (256 / G), iters = (rows + ngroups - 1) / ngroups;
    long long row = (long long)blockIdx.x * (256 / G) + threadIdx.x / G;
    for (long long it = 0; it < iters; ++it, row += ngroups) {
        const bool live = row < rows;
        const long long rr = live ? row : 0;
        float p[K], lp[K], q[K], lq[K];
        row_softmax<G, K>(a.p + row_offset(a, r, rr), sla, L, l, live, p, lp);
        row_softmax<G, K>(b.p + row_offset(b, r, rr), slb, L, l, live, q, lq);
        float S = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (live && l + k * G < L) S += p[k] * (lq[k] - lp[k]);
        S = group_sum<G>(S);
        float* out = gr + row_offset(gv, r, rr);
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (live && l + k * G < L) out[(l + k * G) * slg] = s * (p[k] * (S - (lq[k] - lp[k]) + 1.f) - q[k]);
    }
}

// ------------------------------------------------------------------ FocalLoss (losses.py:119-153)
// per voxel -(1 - pt)^gamma alpha[t] log pt with pt = softmax(x)[t]; the target is the label of voxel n V + v (natural order, as the
// reference's view(-1, 1)); mean or sum.  pt is DETACHED in the reference (Variable(logpt.data.exp())), so the gradient flows through
// log pt only.  A label outside 0..C-1 (the reference's gather raises) makes the loss NaN.
__device__ __forceinline__ float focal_mod(float pt, float gamma) {
    const float u = 1.f - pt;
    return gamma == 0.f ? 1.f : gamma == 1.f ? u : gamma == 2.f ? u * u : powf(u, gamma);
}

__device__ __forceinline__ long long load_label(const void* t, int kind, long long off) {
    return kind == 1 ? (long long)((const uint8_t*)t)[off] : ((const long long*)t)[off];
}

__global__ __launch_bounds__(256) void focal_fwd_kernel(View a, const void* __restrict__ tgt, int tkind, long long n_, int C, long long V,
                                                        float gamma, Weights alpha, double* __restrict__ sum) {
    const long long total = n_ * V;
    float acc = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / V, v = i - n * V;
        float p[MAXC], lp[MAXC];
        load_probs(a, n, v, C, 0, p, lp);
        const long long t = load_label(tgt, tkind, i);
        float logpt = NAN, at = NAN;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C && t == c) { logpt = lp[c]; at = alpha.w[c]; }
        acc -= focal_mod(expf(logpt), gamma) * at * logpt;
    }
    block_atomic_double(acc, sum);
}

// d/dx_c = -(1 - pt)^gamma alpha_t (delta_ct - p_c) * g_up / count    (count = n V for the mean, 1 for the sum)
__global__ __launch_bounds__(256) void focal_bwd_kernel(View a, const void* __restrict__ tgt, int tkind, long long n_, int C, long long V,
                                                        float gamma, Weights alpha, const float* __restrict__ g_up, double count,
                                                        float* __restrict__ gr, long long osn, long long osc, long long osv) {
    const long long total = n_ * V;
    const float s = (float)((double)g_up[0] / count);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / V, v = i - n * V;
        float p[MAXC], lp[MAXC];
        load_probs(a, n, v, C, 0, p, lp);
        const long long t = load_label(tgt, tkind, i);
        float logpt = NAN, at = NAN;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C && t == c) { logpt = lp[c]; at = alpha.w[c]; }
        const float k = -s * focal_mod(expf(logpt), gamma) * at;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) gr[n * osn + c * osc + v * osv] = k * ((t == c ? 1.f : 0.f) - p[c]);
    }
}

// ------------------------------------------------------------------ host entry points of the second family
static inline bool zero_doubles(double* p, int count, dycon_stream_t stream) {
    if (hipMemsetAsync(p, 0, sizeof(double) * count, stream) == hipSuccess) return true;
    dycon_set_error("memset failed");
    return false;
}

extern "C" int dycon_dice1_fwd(const dycon_view_t* score, const dycon_view_t* target, int target_kind, long long n, int C, long long V,
                               int softmax, double* sums, float* out, dycon_stream_t stream) {
    CHECK_VIEW(score); CHECK_VIEW(target); CHECK_DIMS();
    DYCON_REQUIRE(sums && out && target_kind >= 0 && target_kind <= 2, "dice1_fwd: bad arguments");
    DYCON_REQUIRE(!softmax || target_kind == 0, "dice1_fwd: softmax needs float32 target logits");
    if (!zero_doubles(sums, 3 * MAXC, stream)) return DYCON_ERR_LAUNCH;
    if (n * V > 0)
        dice1_sums_kernel<<<grid_for(n * V), 256, 0, stream>>>(mkview(score), target->p, target_kind, target->sn, target->sc, target->sv, n,
                                                               C, V, softmax, sums);
    dice1_finalize_kernel<<<1, 1, 0, stream>>>(sums, C, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_dice1_bwd(const dycon_view_t* a, const dycon_view_t* b, int b_kind, long long n, int C, long long V, int softmax,
                               const double* sums, const float* g_up, const dycon_view_t* grad, dycon_stream_t stream) {
    CHECK_VIEW(a); CHECK_VIEW(b); CHECK_VIEW(grad); CHECK_DIMS();
    DYCON_REQUIRE(sums && g_up && b_kind >= 0 && b_kind <= 2, "dice1_bwd: bad arguments");
    DYCON_REQUIRE(!softmax || b_kind == 0, "dice1_bwd: softmax needs float32 target logits");
    if (n * V == 0) return DYCON_OK;
    dice1_bwd_kernel<<<grid_for(n * V), 256, 0, stream>>>(mkview(a), b->p, b_kind, b->sn, b->sc, b->sv, n, C, V, softmax, sums, g_up,
                                                          (float*)grad->p, grad->sn, grad->sc, grad->sv);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_entropy_fwd(const dycon_view_t* p, long long n, int C, long long V, float scale, float* map, double* sum,
                                 float* out, dycon_stream_t stream) {
    CHECK_VIEW(p); CHECK_DIMS();
    DYCON_REQUIRE((map != nullptr) != (sum != nullptr && out != nullptr), "entropy_fwd: pass either map or (sum, out)");
    DYCON_REQUIRE(map || n * V > 0, "entropy_fwd: mean of an empty input");
    if (sum && !zero_doubles(sum, 1, stream)) return DYCON_ERR_LAUNCH;
    if (n * V == 0) return DYCON_OK;
    entropy_fwd_kernel<<<grid_for(n * V), 256, 0, stream>>>(mkview(p), n, C, V, scale, map, sum);
    if (sum) scalar_mean_kernel<<<1, 1, 0, stream>>>(sum, (double)n * V / (double)scale, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_entropy_bwd(const dycon_view_t* p, long long n, int C, long long V, float scale, const float* g_map,
                                 const float* g_up, const dycon_view_t* grad, dycon_stream_t stream) {
    CHECK_VIEW(p); CHECK_VIEW(grad); CHECK_DIMS();
    DYCON_REQUIRE((g_map != nullptr) != (g_up != nullptr), "entropy_bwd: pass either g_map or g_up");
    if (n * V == 0) return DYCON_OK;
    entropy_bwd_kernel<<<grid_for(n * V), 256, 0, stream>>>(mkview(p), n, C, V, scale, g_map, g_up, (float*)grad->p, grad->sn, grad->sc,
                                                            grad->sv);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

static inline int grid_for4(long long total) { return grid_for((total + 3) / 4); }

extern "C" int dycon_sym_mse_fwd(const dycon_view_t* a, const dycon_view_t* b, long long count, double* sum, float* out,
                                 dycon_stream_t stream) {
    CHECK_VIEW(a); CHECK_VIEW(b);
    DYCON_REQUIRE(sum && out && count > 0, "sym_mse_fwd: empty input or null output");
    if (!zero_doubles(sum, 1, stream)) return DYCON_ERR_LAUNCH;
    sym_mse_fwd_kernel<<<grid_for4(count), 256, 0, stream>>>((const float*)a->p, a->sv, (const float*)b->p, b->sv, count, sum);
    scalar_mean_kernel<<<1, 1, 0, stream>>>(sum, (double)count, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_sym_mse_bwd(const dycon_view_t* a, const dycon_view_t* b, long long count, const float* g_up,
                                 const dycon_view_t* grad, dycon_stream_t stream) {
    CHECK_VIEW(a); CHECK_VIEW(b); CHECK_VIEW(grad);
    DYCON_REQUIRE(g_up && count >= 0, "sym_mse_bwd: bad arguments");
    if (count == 0) return DYCON_OK;
    sym_mse_bwd_kernel<<<grid_for4(count), 256, 0, stream>>>((const float*)a->p, a->sv, (const float*)b->p, b->sv, count, g_up,
                                                             (float*)grad->p, grad->sv);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

// G lanes per row, K elements per lane
#define KL_DISPATCH(L, ...)                                                                                    \
    do {                                                                                                       \
        if ((L) <= 2) { constexpr int G = 2, K = 1; __VA_ARGS__; }                                             \
        else if ((L) <= 4) { constexpr int G = 4, K = 1; __VA_ARGS__; }                                        \
        else if ((L) <= 8) { constexpr int G = 8, K = 1; __VA_ARGS__; }                                        \
        else if ((L) <= 16) { constexpr int G = 16, K = 1; __VA_ARGS__; }                                      \
        else if ((L) <= 32) { constexpr int G = 32, K = 1; __VA_ARGS__; }                                      \
        else if ((L) <= 64) { constexpr int G = 64, K = 1; __VA_ARGS__; }                                      \
        else if ((L) <= 128) { constexpr int G = 64, K = 2; __VA_ARGS__; }                                     \
        else if ((L) <= 256) { constexpr int G = 64, K = 4; __VA_ARGS__; }                                     \
        else if ((L) <= 512) { constexpr int G = 64, K = 8; __VA_ARGS__; }                                     \
        else { constexpr int G = 64, K = 16; __VA_ARGS__; }                                                    \
    } while (0)

#define CHECK_ROWS()                                                                                                                 \
    DYCON_REQUIRE(n >= 0 && C >= 1 && V >= 0 && L >= 1 && L <= KL_MAX_L, "bad dims n=%lld C=%lld V=%lld L=%d (1 <= L <= %d)", n, C, V, L, \
                  KL_MAX_L)
static inline int grid_rows(long long rows, int G) { return grid_for(rows * G); }

extern "C" int dycon_kl_rows_fwd(const dycon_view_t* a, long long sla, const dycon_view_t* b, long long slb, long long n, long long C,
                                 long long V, int L, double* sum, float* out, dycon_stream_t stream) {
    CHECK_VIEW(a); CHECK_VIEW(b); CHECK_ROWS();
    DYCON_REQUIRE(sum && out && n * C * V > 0, "kl_rows_fwd: empty input or null output");
    if (!zero_doubles(sum, 1, stream)) return DYCON_ERR_LAUNCH;
    const Rows r{n, C, V};
    KL_DISPATCH(L, (kl_rows_fwd_kernel<G, K><<<grid_rows(n * C * V, G), 256, 0, stream>>>(mkview(a), sla, mkview(b), slb, r, L, sum)));
    scalar_mean_kernel<<<1, 1, 0, stream>>>(sum, 2.0 * (double)(n * C * V) * (double)L, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_kl_rows_bwd(const dycon_view_t* a, long long sla, const dycon_view_t* b, long long slb, long long n, long long C,
                                 long long V, int L, const float* g_up, const dycon_view_t* grad, long long slg,
                                 dycon_stream_t stream) {
    CHECK_VIEW(a); CHECK_VIEW(b); CHECK_VIEW(grad); CHECK_ROWS();
    DYCON_REQUIRE(g_up, "kl_rows_bwd: null g_up");
    if (n * C * V == 0) return DYCON_OK;
    const Rows r{n, C, V};
    KL_DISPATCH(L, (kl_rows_bwd_kernel<G, K><<<grid_rows(n * C * V, G), 256, 0, stream>>>(mkview(a), sla, mkview(b), slb, r, L, g_up,
                                                                                       (float*)grad->p, mkview(grad), slg)));
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

// alpha_host: C host floats or NULL (= 1, the reference's alpha=None)
extern "C" int dycon_focal_fwd(const dycon_view_t* x, const void* target, int target_kind, long long n, int C, long long V, float gamma,
                               const float* alpha_host, int size_average, double* sum, float* out, dycon_stream_t stream) {
    CHECK_VIEW(x); CHECK_DIMS();
    DYCON_REQUIRE(target && sum && out && (target_kind == 1 || target_kind == 2), "focal_fwd: bad arguments (target: uint8 or int64)");
    DYCON_REQUIRE(n * V > 0 || !size_average, "focal_fwd: mean of an empty input");
    if (!zero_doubles(sum, 1, stream)) return DYCON_ERR_LAUNCH;
    if (n * V > 0) focal_fwd_kernel<<<grid_for(n * V), 256, 0, stream>>>(mkview(x), target, target_kind, n, C, V, gamma,
                                                                         mkweights(alpha_host, C), sum);
    scalar_mean_kernel<<<1, 1, 0, stream>>>(sum, size_average ? (double)n * V : 1.0, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_focal_bwd(const dycon_view_t* x, const void* target, int target_kind, long long n, int C, long long V, float gamma,
                               const float* alpha_host, int size_average, const float* g_up, const dycon_view_t* grad,
                               dycon_stream_t stream) {
    CHECK_VIEW(x); CHECK_VIEW(grad); CHECK_DIMS();
    DYCON_REQUIRE(target && g_up && (target_kind == 1 || target_kind == 2), "focal_bwd: bad arguments (target: uint8 or int64)");
    if (n * V == 0) return DYCON_OK;
    focal_bwd_kernel<<<grid_for(n * V), 256, 0, stream>>>(mkview(x), target, target_kind, n, C, V, gamma, mkweights(alpha_host, C), g_up,
                                                          size_average ? (double)n * V : 1.0, (float*)grad->p, grad->sn, grad->sc,
                                                          grad->sv);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

// ------------------------------------------------------------------ UnCLoss for C classes (code/utils/dycon_losses.py:94-118)
// Per voxel: p = softmax(s), q = softmax(t), H = -sum_c p_c log(p_c + 1e-6),
//   l = sum_c (p_c - q_c)^2 / (e^{beta H_s} + e^{beta H_t}) + beta (H_s + H_t);      the loss is the mean of l over n V voxels.
// (The 2-class loss of the DyCON step lives in losses.hip, fused with the step's other voxel losses.)
__device__ __forceinline__ float uncl_probs(const View& a, long long n, long long v, int C, float* p) {
    // p = softmax over the C channels (exp(x - max) / sum, as torch); returns H
    const float* base = a.p + n * a.sn + v * a.sv;
    float x[MAXC], m = -INFINITY, z = 0.f, H = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) { x[c] = base[c * a.sc]; m = fmaxf(m, x[c]); }
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) { p[c] = expf(x[c] - m); z += p[c]; }
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) { p[c] = p[c] / z; H -= p[c] * logf(p[c] + 1e-6f); }
    return H;
}

__global__ __launch_bounds__(256) void uncl_fwd_kernel(View s, View t, long long n_, int C, long long V, float beta,
                                                       double* __restrict__ sum) {
    const long long total = n_ * V;
    float acc = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / V, v = i - n * V;
        float p[MAXC], q[MAXC];
        const float Hs = uncl_probs(s, n, v, C, p), Ht = uncl_probs(t, n, v, C, q);
        float d2 = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) { const float d = p[c] - q[c]; d2 += d * d; }
        acc += d2 / (expf(beta * Hs) + expf(beta * Ht)) + beta * (Hs + Ht);
    }
    block_atomic_double(acc, sum);
}

// gradient w.r.t. the student logits: dl/dp_c = 2 (p_c - q_c) / D + beta (1 - d2 e^{beta H_s} / D^2) dH_s/dp_c with
// D = e^{beta H_s} + e^{beta H_t}, dH_s/dp_c = -(log(p_c + 1e-6) + p_c / (p_c + 1e-6)); then through the softmax
__global__ __launch_bounds__(256) void uncl_bwd_kernel(View s, View t, long long n_, int C, long long V, float beta,
                                                       const float* __restrict__ g_up, float* __restrict__ gr, long long osn,
                                                       long long osc, long long osv) {
    const long long total = n_ * V;
    const float k = (float)((double)g_up[0] / (double)total);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / V, v = i - n * V;
        float p[MAXC], q[MAXC], h[MAXC];
        const float Hs = uncl_probs(s, n, v, C, p), Ht = uncl_probs(t, n, v, C, q);
        float d2 = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) { const float d = p[c] - q[c]; d2 += d * d; }
        const float es = expf(beta * Hs), D = es + expf(beta * Ht);
        const float gH = beta * (1.f - d2 * es / (D * D));
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) {
                const float pe = p[c] + 1e-6f;
                h[c] = 2.f * (p[c] - q[c]) / D - gH * (logf(pe) + p[c] / pe);
                dot += h[c] * p[c];
            }
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) gr[n * osn + c * osc + v * osv] = k * (p[c] * (h[c] - dot));
    }
}

extern "C" int dycon_uncl_fwd(const dycon_view_t* s, const dycon_view_t* t, long long n, int C, long long V, float beta, double* sum,
                              float* out, dycon_stream_t stream) {
    CHECK_VIEW(s); CHECK_VIEW(t); CHECK_DIMS();
    DYCON_REQUIRE(sum && out && n * V > 0, "uncl_fwd: bad arguments (mean of an empty input?)");
    if (!zero_doubles(sum, 1, stream)) return DYCON_ERR_LAUNCH;
    uncl_fwd_kernel<<<grid_for(n * V), 256, 0, stream>>>(mkview(s), mkview(t), n, C, V, beta, sum);
    scalar_mean_kernel<<<1, 1, 0, stream>>>(sum, (double)n * V, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_uncl_bwd(const dycon_view_t* s, const dycon_view_t* t, long long n, int C, long long V, float beta,
                              const float* g_up, const dycon_view_t* grad, dycon_stream_t stream) {
    CHECK_VIEW(s); CHECK_VIEW(t); CHECK_VIEW(grad); CHECK_DIMS();
    DYCON_REQUIRE(g_up && n * V > 0, "uncl_bwd: bad arguments");
    uncl_bwd_kernel<<<grid_for(n * V), 256, 0, stream>>>(mkview(s), mkview(t), n, C, V, beta, g_up, (float*)grad->p, grad->sn, grad->sc,
                                                         grad->sv);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}
