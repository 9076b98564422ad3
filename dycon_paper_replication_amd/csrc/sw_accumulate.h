// The accumulate pass of the sliding-window evaluators (code/utils/test_3d_patch.py:293-351, :415-476), shared by the entry points of
// csrc/eval.hip (one model, class 1), csrc/evalc.hip (one model, all classes) and csrc/ensemble.hip (2..4 models, class 1; the
// weighted form of all of them).
//
// The reference copies every patch's softmax to the host and accumulates score / count maps with numpy slicing.  Here the maps
// stay in HBM: after a batch of patches went through the network, one voxel-centric pass adds, for every voxel of a box of the
// volume, the softmax of each patch of the batch that covers it (fixed patch order: deterministic, no atomics although windows
// overlap).  A bandwidth-bound pass with coalesced access along the last axis.
#pragma once
#include "common.h"

// fp32 (n_patches, p0, p1, p2, C) logits of the M models of an ensemble; M == 1: the one model's
struct SwLogits {
    const float* l[4];
};

// logit `at` of one voxel of one window: the model's own for M == 1, else the mean over the models, ((l0 + l1) + l2) + l3, then / M
// ((y1_l + y1_r) / 2, :462).  (a + a) / 2 == a in fp32, so an ensemble of a model with itself gives the single model's bits.
template <int M> __device__ __forceinline__ float sw_logit(const SwLogits& in, long long at) {
    float x = in.l[0][at];
    if constexpr (M > 1) x += in.l[1][at];
    if constexpr (M > 2) x += in.l[2][at];
    if constexpr (M > 3) x += in.l[3][at];
    if constexpr (M > 1) x /= (float)M;
    return x;
}

// What the weighted form (BLEND) reads beside the logits: g[a][i], fp32, is the importance of local coordinate i of window axis a.
// The plain instantiations carry the empty struct: no argument is loaded and no code is generated for it.
template <bool BLEND> struct SwBlend {};
template <> struct SwBlend<true> {
    const float* g[3];
};

// What the moments form (MOM, dycon_sw_accumulate_moments, csrc/uncertainty.hip) writes beside score and cnt: hsum (D0, D1, D2) takes
// w * H(p) and sq (C, D0, D1, D2) takes w * p[k]^2 of every entry, the sums behind the uncertainty maps.  The other instantiations
// carry the empty struct, as with SwBlend.
template <bool MOM> struct SwMoments {};
template <> struct SwMoments<true> {
    float* hsum;
    float* sq;
};

// Sweeps the box [lo, lo + b) of the volume D0 x D1 x D2.  ALL: every class of the C-way softmax goes to the class-major score map
// (C, D0, D1, D2); otherwise class 1 goes to score (D0, D1, D2).  pair (C == 2, class 1 only): the two-logit expression
// 1 / (1 + exp(l0 - l1)) instead of the max-shifted softmax; dycon_sw_accumulate and the ensemble of 2-class models score that way.
// BLEND (dycon_sw_accumulate_weighted): `origins` holds (ox, oy, oz, mask) per entry.  The window went through the network flipped
// along every axis whose mask bit is set, so the logits of local coordinate l sit at the mirrored coordinate; the entry adds
// w * p to score and w to cnt with w = (g0[la] * g1[lb]) * g2[lc] at the UNmirrored coordinate.  Unit tables and mask 0 give the
// plain form's bits: 1 * p and n + 1 are exact.
// MOM (needs M == 1, ALL, BLEND): every entry is a member of the voxel's ensemble.  Beside s[k] += w * p[k] and n += w, the same
// expressions in the same order, the voxel keeps m2[k] += w * (p[k] * p[k]) and hs += w * H(p), H(p) = -sum_k p[k] ln p[k] over the
// classes in order, a class with p[k] == 0 adding nothing (a saturated softmax has entropy 0, not NaN): 2C + 2 accumulators.
template <int M, bool ALL, bool BLEND = false, bool MOM = false>
__global__ __launch_bounds__(256) void sw_accumulate_kernel(SwLogits in, int C, int pair, int nb, int p0, int p1, int p2,
                                                            const int* __restrict__ origins, float* __restrict__ score,
                                                            float* __restrict__ cnt, int D0, int D1, int D2, int lo0, int lo1, int lo2,
                                                            int b0, int b1, int b2, SwBlend<BLEND> bl, SwMoments<MOM> mo) {
    static_assert(!MOM || (M == 1 && ALL && BLEND), "the moments form is the weighted all-class accumulate of one model");
    constexpr int S = ALL ? 8 : 1, E = BLEND ? 4 : 3, Q = MOM ? 8 : 1;
    __shared__ int org[E * 64];
    for (int i = threadIdx.x; i < E * nb; i += 256) org[i] = origins[i];
    __syncthreads();
    const long long total = (long long)D0 * D1 * D2, box = (long long)b0 * b1 * b2;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < box; j += (long long)gridDim.x * 256) {
        const int c = lo2 + (int)(j % b2);
        const long long q = j / b2;
        const int b_ = lo1 + (int)(q % b1), a = lo0 + (int)(q / b1);
        float s[S], n = 0.f;
#pragma unroll
        for (int k = 0; k < S; ++k) s[k] = 0.f;
        float m2[Q], hs = 0.f;                                // MOM only
#pragma unroll
        for (int k = 0; k < Q; ++k) m2[k] = 0.f;
        for (int p = 0; p < nb; ++p) {
            const int la = a - org[E * p], lb = b_ - org[E * p + 1], lc = c - org[E * p + 2];
            if ((unsigned)la < (unsigned)p0 && (unsigned)lb < (unsigned)p1 && (unsigned)lc < (unsigned)p2) {
                int ma = la, mb = lb, mc = lc;
                float wt = 1.f;                              // the plain form: 1.f * p folds to p
                if constexpr (BLEND) {
                    const int mask = org[E * p + 3];
                    if (mask & 1) ma = p0 - 1 - la;
                    if (mask & 2) mb = p1 - 1 - lb;
                    if (mask & 4) mc = p2 - 1 - lc;
                    wt = (bl.g[0][la] * bl.g[1][lb]) * bl.g[2][lc];
                }
                const long long at = ((((long long)p * p0 + ma) * p1 + mb) * p2 + mc) * C;
                if (!ALL && pair) {
                    const float pr = 1.f / (1.f + __expf(sw_logit<M>(in, at) - sw_logit<M>(in, at + 1)));   // softmax(logits)[1]  (:334-337)
                    s[0] += wt * pr;
                } else {
                    float x[8], m = -INFINITY, z = 0.f;
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k < C) { x[k] = sw_logit<M>(in, at + k); m = fmaxf(m, x[k]); }
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k < C) { x[k] = expf(x[k] - m); z += x[k]; }
                    if constexpr (MOM) {
                        float h = 0.f;
#pragma unroll
                        for (int k = 0; k < 8; ++k)
                            if (k < C) {
                                const float pk = x[k] / z;
                                s[k] += wt * pk;                       // the ALL branch's expression
                                m2[k] += wt * (pk * pk);
                                if (pk > 0.f) h -= pk * logf(pk);
                            }
                        hs += wt * h;
                    } else if constexpr (ALL) {
#pragma unroll
                        for (int k = 0; k < 8; ++k)
                            if (k < C) s[k] += wt * (x[k] / z);        // softmax(logits, 1)[k]   (:334-336)
                    } else {
                        s[0] += wt * (x[1] / z);                   // softmax(logits, 1)[1]   (:334-337)
                    }
                }
                n += wt;
            }
        }
        if (n > 0.f) {                                       // a voxel of the box that no window of the chunk covers stays untouched
            const long long i = ((long long)a * D1 + b_) * D2 + c;
#pragma unroll
            for (int k = 0; k < S; ++k)
                if (k < C) score[k * total + i] += s[k];
            cnt[i] += n;
            if constexpr (MOM) {
#pragma unroll
                for (int k = 0; k < Q; ++k)
                    if (k < C) mo.sq[k * total + i] += m2[k];
                mo.hsum[i] += hs;
            }
        }
    }
}

// the shape check of every accumulate entry point; `who` is the entry point's name without the dycon_ prefix
static int sw_check_shape(const char* who, int n_patches, int p0, int p1, int p2, int D0, int D1, int D2) {
    DYCON_REQUIRE(n_patches > 0 && n_patches <= 64 && p0 > 0 && p1 > 0 && p2 > 0 && D0 >= p0 && D1 >= p1 && D2 >= p2,
                  "%s: bad shape (%d patches of %dx%dx%d in %dx%dx%d)", who, n_patches, p0, p1, p2, D0, D1, D2);
    return DYCON_OK;
}

// box_lo == nullptr: the whole volume
template <int M, bool ALL, bool BLEND = false, bool MOM = false>
static int sw_accumulate_launch(const SwLogits& in, int C, int pair, int n_patches, int p0, int p1, int p2, const int* origins_dev,
                                float* score, float* cnt, int D0, int D1, int D2, const int* box_lo, const int* box_hi,
                                dycon_stream_t stream, SwBlend<BLEND> bl = {}, SwMoments<MOM> mo = {}) {
    const int zero[3] = {0, 0, 0}, D[3] = {D0, D1, D2};
    const int* lo = box_lo ? box_lo : zero;
    const int* hi = box_lo ? box_hi : D;
    const int b0 = hi[0] - lo[0], b1 = hi[1] - lo[1], b2 = hi[2] - lo[2];
    long long blocks = ((long long)b0 * b1 * b2 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    sw_accumulate_kernel<M, ALL, BLEND, MOM><<<(int)blocks, 256, 0, stream>>>(in, C, pair, n_patches, p0, p1, p2, origins_dev, score, cnt, D0,
                                                                              D1, D2, lo[0], lo[1], lo[2], b0, b1, b2, bl, mo);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}
