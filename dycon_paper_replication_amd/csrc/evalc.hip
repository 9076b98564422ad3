// Multi-class evaluation on the device: the all-class form of the sliding-window evaluator (code/utils/test_3d_patch.py:293-351, which
// keeps class 1 only, :337-347), the argmax label map (code/train_DyCON_ISLES22.py:364-366) and the C x C confusion counts behind the
// per-class Dice / Jaccard (code/utils/metrics.py:14-27 cal_dice, code/utils/test_3d_patch.py:496-508).  The all-class accumulate is
// sw_accumulate_kernel<1, true> (sw_accumulate.h) over the bounding box of a chunk's windows; csrc/eval.hip holds the binary counts.
//
// Every kernel here streams its operands once and is HBM-bound; the counts are integers, so they do not depend on the grid.
#include "sw_accumulate.h"

// first index of the maximum, a NaN counting as the maximum (numpy / torch argmax)
__device__ __forceinline__ bool argmax_takes(float x, float best) { return x > best || (x != x && best == best); }

// p_c = score_c / cnt (:344), label = argmax_c p_c.  Each thread reads its voxel's C scores before it writes them: prob may be score.
__global__ __launch_bounds__(256) void sw_finalize_argmax_kernel(const float* score, const float* __restrict__ cnt, int C, long long n,
                                                                 unsigned char* __restrict__ label, float* prob) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float d = cnt[i];                              // every voxel is covered by at least one window
        float best = score[i] / d;
        int arg = 0;
        if (prob) prob[i] = best;
        for (int k = 1; k < C; ++k) {
            const float p = score[k * n + i] / d;
            if (prob) prob[k * n + i] = p;
            if (argmax_takes(p, best)) { best = p; arg = k; }
        }
        label[i] = (unsigned char)arg;
    }
}

__device__ __forceinline__ int argmax_row(const float* __restrict__ l, int C) {
    float best = l[0];
    int arg = 0;
    for (int k = 1; k < C; ++k) {
        const float x = l[k];
        if (argmax_takes(x, best)) { best = x; arg = k; }
    }
    return arg;
}

__global__ __launch_bounds__(256) void argmax_labels_kernel(const float* __restrict__ logits, int C, long long n,
                                                            unsigned char* __restrict__ label) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        label[i] = (unsigned char)argmax_row(logits + i * C, C);
}

// The counters of one workgroup: one private set per wave in LDS (C * C cells and the out-of-range cell, at most 65), added into by
// LDS atomics; after the sweep the four sets are summed and every non-zero cell costs one global atomic.
struct ConfusionCells {
    unsigned long long w[4][65];
};

__device__ __forceinline__ void confusion_clear(ConfusionCells& sm) {
    for (int i = threadIdx.x; i < 4 * 65; i += 256) (&sm.w[0][0])[i] = 0;
    __syncthreads();
}

__device__ __forceinline__ void confusion_count(ConfusionCells& sm, unsigned p, unsigned long long g, int C) {
    const int cell = (p < (unsigned)C && g < (unsigned long long)C) ? (int)p * C + (int)g : C * C;
    atomicAdd(&sm.w[threadIdx.x >> 6][cell], 1ull);
}

__device__ __forceinline__ void confusion_flush(ConfusionCells& sm, int C, unsigned long long* __restrict__ out) {
    __syncthreads();
    if ((int)threadIdx.x <= C * C) {
        const unsigned long long v = sm.w[0][threadIdx.x] + sm.w[1][threadIdx.x] + sm.w[2][threadIdx.x] + sm.w[3][threadIdx.x];
        if (v) atomicAdd(out + threadIdx.x, v);
    }
}

template <typename TG>
__global__ __launch_bounds__(256) void class_confusion_kernel(const unsigned char* __restrict__ pred, const TG* __restrict__ gt,
                                                              long long n, int C, unsigned long long* __restrict__ out) {
    __shared__ ConfusionCells sm;
    confusion_clear(sm);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        confusion_count(sm, pred[i], (unsigned long long)gt[i], C);      // a negative int64 label becomes a huge value: out of range
    confusion_flush(sm, C, out);
}

// The C-class sibling of batch_overlap_kernel (csrc/eval.hip): per sample, pred = argmax_c logit read straight from the (B, V, C) logits
template <typename TG>
__global__ __launch_bounds__(256) void batch_class_confusion_kernel(const float* __restrict__ logits, const TG* __restrict__ gt,
                                                                    long long V, int C, unsigned long long* __restrict__ out) {
    __shared__ ConfusionCells sm;
    confusion_clear(sm);
    const long long base = (long long)blockIdx.y * V;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256)
        confusion_count(sm, (unsigned)argmax_row(logits + (base + i) * C, C), (unsigned long long)gt[base + i], C);
    confusion_flush(sm, C, out + (long long)blockIdx.y * (C * C + 1));
}

static int capped_blocks(long long n, int cap) {
    const long long blocks = (n + 255) / 256;
    return (int)(blocks > cap ? cap : blocks);
}

extern "C" int dycon_sw_accumulate_all(const float* logits, int C, int n_patches, int p0, int p1, int p2, const int* origins_dev,
                                       float* score, float* cnt, int D0, int D1, int D2, const int* box_lo, const int* box_hi,
                                       dycon_stream_t stream) {
    DYCON_REQUIRE(logits && origins_dev && score && cnt && box_lo && box_hi, "sw_accumulate_all: null pointer");
    DYCON_REQUIRE(C >= 2 && C <= 8, "sw_accumulate_all: C = %d (2..8)", C);
    if (int e = sw_check_shape("sw_accumulate_all", n_patches, p0, p1, p2, D0, D1, D2)) return e;
    const int D[3] = {D0, D1, D2};
    for (int a = 0; a < 3; ++a)
        DYCON_REQUIRE(box_lo[a] >= 0 && box_lo[a] < box_hi[a] && box_hi[a] <= D[a],
                      "sw_accumulate_all: box [%d, %d) on axis %d lies outside the volume (extent %d)", box_lo[a], box_hi[a], a, D[a]);
    return sw_accumulate_launch<1, true>({{logits}}, C, 0, n_patches, p0, p1, p2, origins_dev, score, cnt, D0, D1, D2, box_lo, box_hi, stream);
}

extern "C" int dycon_sw_finalize_argmax(const float* score, const float* cnt, int C, long long n, uint8_t* label, float* prob,
                                        dycon_stream_t stream) {
    DYCON_REQUIRE(score && cnt && label && n > 0, "sw_finalize_argmax: bad arguments");
    DYCON_REQUIRE(C >= 2 && C <= 8, "sw_finalize_argmax: C = %d (2..8)", C);
    sw_finalize_argmax_kernel<<<capped_blocks(n, 4096), 256, 0, stream>>>(score, cnt, C, n, label, prob);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_argmax_labels(const float* logits, int C, long long nvox, uint8_t* label, dycon_stream_t stream) {
    DYCON_REQUIRE(logits && label && nvox > 0, "argmax_labels: bad arguments");
    DYCON_REQUIRE(C >= 2 && C <= 8, "argmax_labels: C = %d (2..8)", C);
    argmax_labels_kernel<<<capped_blocks(nvox, 4096), 256, 0, stream>>>(logits, C, nvox, label);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_class_confusion(const uint8_t* pred, const void* gt, int gt_bytes, long long n, int C, unsigned long long* out,
                                     dycon_stream_t stream) {
    DYCON_REQUIRE(pred && gt && out && n > 0, "class_confusion: bad arguments");
    DYCON_REQUIRE(C >= 2 && C <= 8, "class_confusion: C = %d (2..8)", C);
    DYCON_REQUIRE(gt_bytes == 1 || gt_bytes == 8, "class_confusion: ground truth must be uint8 or int64");
    const int blocks = capped_blocks(n, 1024);
    if (gt_bytes == 1) class_confusion_kernel<unsigned char><<<blocks, 256, 0, stream>>>(pred, (const unsigned char*)gt, n, C, out);
    else class_confusion_kernel<long long><<<blocks, 256, 0, stream>>>(pred, (const long long*)gt, n, C, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_batch_class_confusion(const float* logits, const void* gt, int gt_bytes, int B, long long V, int C,
                                           unsigned long long* out, dycon_stream_t stream) {
    DYCON_REQUIRE(logits && gt && out && B > 0 && B <= 65535 && V > 0, "batch_class_confusion: bad arguments");
    DYCON_REQUIRE(C >= 2 && C <= 8, "batch_class_confusion: C = %d (2..8)", C);
    DYCON_REQUIRE(gt_bytes == 1 || gt_bytes == 8, "batch_class_confusion: ground truth must be uint8 or int64");
    dim3 grid(capped_blocks(V, 512), B);
    if (gt_bytes == 1) batch_class_confusion_kernel<unsigned char><<<grid, 256, 0, stream>>>(logits, (const unsigned char*)gt, V, C, out);
    else batch_class_confusion_kernel<long long><<<grid, 256, 0, stream>>>(logits, (const long long*)gt, V, C, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}
