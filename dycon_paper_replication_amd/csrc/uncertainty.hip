// Uncertainty maps and calibration counts of the sliding-window evaluators (utils/uncertainty.py).  Not in the reference: its
// evaluator (code/utils/test_3d_patch.py:293-351) keeps the mean softmax only.  The definitions restated here are the standard ones
// over the members of a voxel's ensemble (every covering window x mirror orientation x model x Monte-Carlo pass), weighted as the
// blended mean is (sw_accumulate.h):
//     prob             = sum_e w_e p_e / sum_e w_e                    the mean of the members' softmaxes
//     entropy          = H(prob),  H(p) = -sum_k p_k ln p_k           predictive entropy; a term with p_k == 0 counts as 0
//     expected_entropy = sum_e w_e H(p_e) / sum_e w_e
//     mutual_info      = max(0, entropy - expected_entropy)           >= 0 by Jensen; the max removes rounding dust
//     variance         = sum_k max(0, sum_e w_e p_e[k]^2 / sum_e w_e - prob[k]^2)
// and, for a probability map against a label map, the counts behind ECE / MCE, the Brier score, the NLL and the error-detection
// curves (Guo et al. 2017's equal-width confidence bins).
//   - dycon_sw_accumulate_moments is sw_accumulate_kernel<1, true, true, true>: dycon_sw_accumulate_weighted's all-class form with two
//     more maps, the same score / cnt bits.
//   - dycon_sw_finalize_uncertainty is dycon_sw_finalize_argmax (csrc/evalc.hip) plus the four maps, one pass.
//   - dycon_calibration_counts: one streaming pass and a one-block fold.
// All three are bandwidth-bound passes with coalesced access along the voxel axis; nothing else was tuned.
#include "sw_accumulate.h"

extern "C" int dycon_sw_accumulate_moments(const float* logits, int C, int n, int p0, int p1, int p2, const int* entries_dev,
                                           const float* g0, const float* g1, const float* g2, float* score, float* cnt, float* hsum,
                                           float* sq, int D0, int D1, int D2, const int* box_lo, const int* box_hi,
                                           dycon_stream_t stream) {
    DYCON_REQUIRE(C >= 2 && C <= 8, "sw_accumulate_moments: C = %d (2..8)", C);
    DYCON_REQUIRE(logits && entries_dev && g0 && g1 && g2 && score && cnt && hsum && sq, "sw_accumulate_moments: null pointer");
    if (int e = sw_check_shape("sw_accumulate_moments", n, p0, p1, p2, D0, D1, D2)) return e;
    DYCON_REQUIRE(!box_lo == !box_hi, "sw_accumulate_moments: box_lo and box_hi come together or not at all");
    const int D[3] = {D0, D1, D2};
    for (int a = 0; box_lo && a < 3; ++a)
        DYCON_REQUIRE(box_lo[a] >= 0 && box_lo[a] < box_hi[a] && box_hi[a] <= D[a],
                      "sw_accumulate_moments: box [%d, %d) on axis %d lies outside the volume (extent %d)", box_lo[a], box_hi[a], a, D[a]);
    return sw_accumulate_launch<1, true, true, true>({{logits}}, C, 0, n, p0, p1, p2, entries_dev, score, cnt, D0, D1, D2, box_lo, box_hi,
                                                     stream, {{g0, g1, g2}}, {hsum, sq});
}

// first index of the maximum, a NaN counting as the maximum (numpy / torch argmax): csrc/evalc.hip's rule
__device__ __forceinline__ bool unc_argmax_takes(float x, float best) { return x > best || (x != x && best == best); }

// label and prob as sw_finalize_argmax_kernel forms them (the same division, the same tie rule), prob written over score; each thread
// reads its voxel's sums before it writes them.
__global__ __launch_bounds__(256) void sw_finalize_uncertainty_kernel(float* score, const float* __restrict__ cnt,
                                                                      const float* __restrict__ hsum, const float* __restrict__ sq,
                                                                      int C, long long n, unsigned char* __restrict__ label,
                                                                      float* __restrict__ entropy, float* __restrict__ expected,
                                                                      float* __restrict__ mutual, float* __restrict__ variance) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float d = cnt[i];                              // every voxel is covered by at least one window
        float best = score[i] / d;
        int arg = 0;
        score[i] = best;
        float h = best > 0.f ? -(best * logf(best)) : 0.f;
        float var = fmaxf(0.f, sq[i] / d - best * best);
        for (int k = 1; k < C; ++k) {
            const float p = score[k * n + i] / d;
            score[k * n + i] = p;
            if (unc_argmax_takes(p, best)) { best = p; arg = k; }
            if (p > 0.f) h -= p * logf(p);
            var += fmaxf(0.f, sq[k * n + i] / d - p * p);
        }
        const float ee = hsum[i] / d;
        label[i] = (unsigned char)arg;
        entropy[i] = h;
        expected[i] = ee;
        mutual[i] = fmaxf(0.f, h - ee);
        variance[i] = var;
    }
}

extern "C" int dycon_sw_finalize_uncertainty(float* score, const float* cnt, const float* hsum, const float* sq, int C, long long n,
                                             uint8_t* label, float* entropy, float* expected_entropy, float* mutual_info,
                                             float* variance, dycon_stream_t stream) {
    DYCON_REQUIRE(score && cnt && hsum && sq && label && entropy && expected_entropy && mutual_info && variance && n > 0,
                  "sw_finalize_uncertainty: bad arguments");
    DYCON_REQUIRE(C >= 2 && C <= 8, "sw_finalize_uncertainty: C = %d (2..8)", C);
    const long long blocks = (n + 255) / 256;
    sw_finalize_uncertainty_kernel<<<(int)(blocks > 4096 ? 4096 : blocks), 256, 0, stream>>>(score, cnt, hsum, sq, C, n, label, entropy,
                                                                                            expected_entropy, mutual_info, variance);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

// ---------------------------------------------------------------- calibration counts
// bin of a value t = x * K that was formed in fp32: min(K - 1, (int)t), a negative or NaN t in bin 0
__device__ __forceinline__ int calib_bin(float t, int K) { return t >= (float)K ? K - 1 : (t > 0.f ? (int)t : 0); }

// Integer cells of one workgroup, one private set per wave in LDS (the scheme of csrc/evalc.hip's ConfusionCells):
// n[K] | correct[K] | unc_hist[correct][K] | unc_hist[wrong][K] | n_scored | labels outside [0, C)      (4K + 2 <= 258 cells)
// Sums: thread t keeps the Brier and NLL terms of its voxels in fp64; the confidence sums go through a tile of 256 (bin, confidence)
// pairs in LDS: lane b < K of wave w adds, in index order, the confidences of bin b among entries [64w, 64w + 64) of the tile.  Every
// order is fixed by (V, K) alone, so the per-block partials, and the fold over them, give the same bits on every run.
constexpr int CALIB_MAX_BINS = 64, CALIB_CELLS = 4 * CALIB_MAX_BINS + 2;

__global__ __launch_bounds__(256) void calibration_counts_kernel(const float* __restrict__ prob, const unsigned char* __restrict__ label,
                                                                 const unsigned char* __restrict__ mask, const float* __restrict__ unc,
                                                                 float u_max, int C, long long V, int K,
                                                                 unsigned long long* __restrict__ counts, double* __restrict__ partials) {
    __shared__ unsigned long long cells[4][CALIB_CELLS];
    __shared__ float tile_c[256];
    __shared__ int tile_bin[256];
    __shared__ double red[256];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, ncell = 4 * K + 2;
    for (int i = tid; i < 4 * CALIB_CELLS; i += 256) (&cells[0][0])[i] = 0;
    __syncthreads();
    double conf = 0.0, brier = 0.0, nll = 0.0;
    for (long long base = (long long)blockIdx.x * 256; base < V; base += (long long)gridDim.x * 256) {      // uniform over the block
        const long long i = base + tid;
        int bin = -1;
        float c = 0.f;
        if (i < V && (!mask || mask[i])) {
            const unsigned g = label[i];
            if (g >= (unsigned)C) {
                atomicAdd(&cells[wave][4 * K + 1], 1ull);
            } else {
                float p[8];
                c = p[0] = prob[i];
                int arg = 0;
#pragma unroll
                for (int k = 1; k < 8; ++k)
                    if (k < C) {
                        p[k] = prob[k * V + i];
                        if (unc_argmax_takes(p[k], c)) { c = p[k]; arg = k; }
                    }
                bin = calib_bin(__fmul_rn(c, (float)K), K);
                const bool ok = arg == (int)g;
                double b = 0.0, pl = 0.0;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < C) {
                        const double dk = __dsub_rn((double)p[k], k == (int)g ? 1.0 : 0.0);
                        b = __dadd_rn(b, __dmul_rn(dk, dk));
                        if (k == (int)g) pl = (double)p[k];
                    }
                brier += b;
                nll += -log(fmax(pl, 1e-12));
                atomicAdd(&cells[wave][bin], 1ull);
                if (ok) atomicAdd(&cells[wave][K + bin], 1ull);
                atomicAdd(&cells[wave][4 * K], 1ull);
                if (unc) {
                    const int ub = calib_bin(__fmul_rn(__fdiv_rn(unc[i], u_max), (float)K), K);
                    atomicAdd(&cells[wave][(ok ? 2 : 3) * K + ub], 1ull);
                }
            }
        }
        __syncthreads();                                     // the previous tile was consumed
        tile_c[tid] = c;
        tile_bin[tid] = bin;
        __syncthreads();
        if (lane < K) {
            for (int j = 64 * wave; j < 64 * wave + 64; ++j)
                if (tile_bin[j] == lane) conf += (double)tile_c[j];
        }
    }
    __syncthreads();
    // integer cells: the four sets summed, one global atomic per non-zero cell
    for (int i = tid; i < ncell; i += 256) {
        const unsigned long long v = cells[0][i] + cells[1][i] + cells[2][i] + cells[3][i];
        if (v) atomicAdd(counts + i, v);
    }
    // fp64 partials of this block: conf[b] = ((wave 0 + wave 1) + wave 2) + wave 3; Brier and NLL by a fixed tree over the threads
    double* out = partials + (long long)blockIdx.x * (K + 2);
    red[tid] = conf;
    __syncthreads();
    if (tid < K) out[tid] = ((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid];
    for (int pass = 0; pass < 2; ++pass) {
        __syncthreads();
        red[tid] = pass ? nll : brier;
        for (int s = 128; s > 0; s >>= 1) {
            __syncthreads();
            if (tid < s) red[tid] += red[tid + s];
        }
        if (tid == 0) out[K + pass] = red[0];
    }
}

// one block: thread t adds column t of the (blocks, K + 2) partials in block order
__global__ __launch_bounds__(128) void calibration_fold_kernel(const double* __restrict__ partials, int blocks, int K,
                                                               double* __restrict__ sums) {
    const int t = threadIdx.x;
    if (t >= K + 2) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += partials[(long long)b * (K + 2) + t];
    sums[t] = s;
}

static int calibration_blocks(long long V) {
    const long long blocks = (V + 255) / 256;
    return (int)(blocks > 1024 ? 1024 : blocks);
}

extern "C" size_t dycon_calibration_workspace(long long V, int K) {
    if (V <= 0 || K < 1 || K > CALIB_MAX_BINS) return 0;
    return (size_t)calibration_blocks(V) * (K + 2) * sizeof(double);
}

extern "C" int dycon_calibration_counts(const float* prob, const uint8_t* label, const uint8_t* mask, const float* unc, float u_max, int C,
                                        long long V, int K, long long* counts, double* sums, void* workspace, size_t ws_bytes,
                                        dycon_stream_t stream) {
    DYCON_REQUIRE(prob && label && counts && sums && workspace && V > 0, "calibration_counts: bad arguments");
    DYCON_REQUIRE(C >= 2 && C <= 8, "calibration_counts: C = %d (2..8)", C);
    DYCON_REQUIRE(K >= 1 && K <= CALIB_MAX_BINS, "calibration_counts: K = %d bins (1..%d)", K, CALIB_MAX_BINS);
    DYCON_REQUIRE(!unc || u_max > 0.f, "calibration_counts: u_max = %g must be positive", (double)u_max);
    DYCON_REQUIRE((uintptr_t)workspace % 8 == 0 && ws_bytes >= dycon_calibration_workspace(V, K),
                  "calibration_counts: workspace of %zu bytes (8-byte aligned, >= %zu)", ws_bytes, dycon_calibration_workspace(V, K));
    const int blocks = calibration_blocks(V);
    if (hipMemsetAsync(counts, 0, (size_t)(4 * K + 2) * sizeof(long long), (hipStream_t)stream) != hipSuccess) {
        dycon_set_error("calibration_counts: hipMemsetAsync failed");
        return DYCON_ERR_LAUNCH;
    }
    calibration_counts_kernel<<<blocks, 256, 0, stream>>>(prob, label, mask, unc, u_max, C, V, K, (unsigned long long*)counts,
                                                          (double*)workspace);
    DYCON_LAUNCH_CHECK();
    calibration_fold_kernel<<<1, 128, 0, stream>>>((const double*)workspace, blocks, K, sums);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}
