// Per-root voxel counts from a root map of dycon_cc_roots (csrc/components.hip): the wave-aggregated integer add that csrc/lesions.hip
// (lesion sizes and overlaps) and csrc/morphology.hip (the size filter) share.  Counts are addressed by root - 1 inside a volume.
#pragma once
#include "common.h"

// arr[q - 1] += 1 for every lane with q != 0.  One large lesion is the common case and consecutive lanes walk z, so the lanes of a
// wave mostly share a root: the wave loops on the root of its first pending lane, ballots the lanes that hold it and counts them
// once (at most 64 rounds: the leader leaves the pending set every round; exactly 64 for 64 distinct roots).  The count is held in
// (held, n), the same in every lane, and goes to memory by one atomicAdd of lane 0 only when the root changes or at les_flush:
// a wave inside one lesion costs one atomic for its whole walk.  Integer adds: the sum does not depend on where an add went.
__device__ __forceinline__ void les_wave_add(int* __restrict__ arr, int q, int lane, int& held, int& n) {
    bool pending = q != 0;
    for (;;) {
        const unsigned long long todo = __ballot(pending);
        if (!todo) break;                                    // wave-uniform
        const int lq = __shfl(q, __ffsll(todo) - 1, 64);
        const unsigned long long same = __ballot(pending && q == lq);
        if (lq != held) {
            if (n && lane == 0) atomicAdd(arr + held - 1, n);
            held = lq;
            n = 0;
        }
        n += __popcll(same);
        if (q == lq) pending = false;
    }
}

__device__ __forceinline__ void les_flush(int* __restrict__ arr, int lane, int held, int n) {
    if (n && lane == 0) atomicAdd(arr + held - 1, n);
}

// a root of this volume, or 0: anything outside 1..V is background, so no value of a root map can address outside the workspace
__device__ __forceinline__ int les_root(const int* __restrict__ r, long long i, long long V) {
    if (i >= V) return 0;
    const int q = r[i];
    return (q >= 1 && q <= V) ? q : 0;
}
