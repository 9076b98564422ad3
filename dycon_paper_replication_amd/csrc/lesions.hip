// Lesion-wise statistics of a prediction and a ground truth from their component roots (dycon_cc_roots, csrc/components.hip): per
// lesion its voxel count and the number of its voxels that are foreground in the other mask, per volume the detection counts the
// lesion-wise F1, the lesion-count difference and the volume difference are made of.  The host path this replaces is two
// scipy.ndimage.label calls and a loop over the lesions per case, after a copy of the label map off the device.
//
// A root is 1 + the smallest linear index (x*Y + y)*Z + z of the component INSIDE ITS VOLUME, so the per-lesion arrays of a volume
// start at volume * X*Y*Z and are addressed by root - 1: the entry of a lesion sits at its first voxel in raster order, every other
// entry stays 0.
//
//   sizes     size[root - 1] += 1 for every foreground voxel, both masks in one launch
//   overlaps  a voxel that is foreground in both masks, in lesions that both pass the size filter, adds 1 to the overlap of its
//             predicted lesion and of its ground-truth lesion
//   counts    the voxels that are their own root and pass the filter: one thread each adds its lesion to the eight per-volume sums,
//             reduced per workgroup, one atomic per workgroup and field
//
// The size filter removes whole components (size < min_voxels) from their own mask before anything else is counted; the survivors
// keep their roots.  Integer atomics only, so every output is the same on every run.  No kernel waits on another workgroup; a call
// is two hipMemsetAsync and three launches, allocates nothing and reads nothing back.
#include "common.h"
#include "root_counts.h"                          // les_wave_add, les_flush, les_root: shared with csrc/morphology.hip

#define LES_MAX_AXIS 512                          // the limits of dycon_cc_roots
#define LES_FIELDS 8
enum { LES_N_GT, LES_N_PRED, LES_TP, LES_FN, LES_FP, LES_VOX_GT, LES_VOX_PRED, LES_VOX_AND };

__global__ __launch_bounds__(256) void les_sizes_kernel(const int* __restrict__ root_p, const int* __restrict__ root_g, long long V,
                                                        int* __restrict__ size_p, int* __restrict__ size_g) {
    const long long off = (long long)blockIdx.y * V;
    const int* __restrict__ rp = root_p + off;
    const int* __restrict__ rg = root_g + off;
    int* __restrict__ sp = size_p + off;
    int* __restrict__ sg = size_g + off;
    const int lane = threadIdx.x & 63;
    int held_p = 0, n_p = 0, held_g = 0, n_g = 0;
    const long long span = (long long)gridDim.x * 256;
    for (long long base = (long long)blockIdx.x * 256; base < V; base += span) {        // workgroup-uniform trip count
        const long long i = base + threadIdx.x;
        les_wave_add(sp, les_root(rp, i, V), lane, held_p, n_p);
        les_wave_add(sg, les_root(rg, i, V), lane, held_g, n_g);
    }
    les_flush(sp, lane, held_p, n_p);
    les_flush(sg, lane, held_g, n_g);
}

__global__ __launch_bounds__(256) void les_overlaps_kernel(const int* __restrict__ root_p, const int* __restrict__ root_g, long long V,
                                                           int min_voxels, const int* __restrict__ size_p,
                                                           const int* __restrict__ size_g, int* __restrict__ over_p,
                                                           int* __restrict__ over_g) {
    const long long off = (long long)blockIdx.y * V;
    const int* __restrict__ rp = root_p + off;
    const int* __restrict__ rg = root_g + off;
    const int* __restrict__ sp = size_p + off;
    const int* __restrict__ sg = size_g + off;
    int* __restrict__ op = over_p + off;
    int* __restrict__ og = over_g + off;
    const int lane = threadIdx.x & 63;
    int held_p = 0, n_p = 0, held_g = 0, n_g = 0;
    const long long span = (long long)gridDim.x * 256;
    for (long long base = (long long)blockIdx.x * 256; base < V; base += span) {
        const long long i = base + threadIdx.x;
        const int qp = les_root(rp, i, V), qg = les_root(rg, i, V);
        const bool both = qp && qg && sp[qp - 1] >= min_voxels && sg[qg - 1] >= min_voxels;     // shared voxel of two surviving lesions
        les_wave_add(op, both ? qp : 0, lane, held_p, n_p);
        les_wave_add(og, both ? qg : 0, lane, held_g, n_g);
    }
    les_flush(op, lane, held_p, n_p);
    les_flush(og, lane, held_g, n_g);
}

// Every field of a volume is at most its voxel count (<= 2^27), so the sums of a thread, a wave and a workgroup fit an int.
__global__ __launch_bounds__(256) void les_counts_kernel(const int* __restrict__ root_p, const int* __restrict__ root_g, long long V,
                                                         int min_voxels, const int* __restrict__ size_p, const int* __restrict__ over_p,
                                                         const int* __restrict__ size_g, const int* __restrict__ over_g,
                                                         unsigned long long* __restrict__ counts) {
    __shared__ int part[4][LES_FIELDS];
    const long long off = (long long)blockIdx.y * V;
    const int* __restrict__ rp = root_p + off;
    const int* __restrict__ rg = root_g + off;
    int acc[LES_FIELDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        if (rp[i] == (int)(i + 1)) {
            const int s = size_p[off + i];
            if (s >= min_voxels) {
                const int o = over_p[off + i];
                acc[LES_N_PRED] += 1;
                acc[LES_VOX_PRED] += s;
                acc[LES_VOX_AND] += o;
                acc[LES_FP] += o == 0;
            }
        }
        if (rg[i] == (int)(i + 1)) {
            const int s = size_g[off + i];
            if (s >= min_voxels) {
                const int o = over_g[off + i];
                acc[LES_N_GT] += 1;
                acc[LES_VOX_GT] += s;
                acc[LES_TP] += o > 0;
                acc[LES_FN] += o == 0;
            }
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int f = 0; f < LES_FIELDS; ++f) {
        int v = acc[f];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) part[w][f] = v;
    }
    __syncthreads();
    if (threadIdx.x < LES_FIELDS) {
        const int v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (v) atomicAdd(counts + (long long)blockIdx.y * LES_FIELDS + threadIdx.x, (unsigned long long)v);
    }
}

// ------------------------------------------------------------------ host side
static size_t les_align(size_t n) { return (n + 255) & ~(size_t)255; }
static int les_grid(long long V) {                                                 // grid-stride passes: 8 voxels per thread, 2048 workgroups at most
    const long long blocks = (V + 256 * 8 - 1) / (256 * 8);
    return (int)(blocks > 2048 ? 2048 : blocks);
}
static bool les_shape_ok(int n_vol, int X, int Y, int Z) {
    return n_vol >= 1 && n_vol <= 65535 && X >= 1 && X <= LES_MAX_AXIS && Y >= 1 && Y <= LES_MAX_AXIS && Z >= 1 && Z <= LES_MAX_AXIS &&
           (long long)n_vol * X * Y * Z <= 2147483647ll;
}

// four sections of the same size: size of the prediction's lesions | their overlap | size of the ground truth's | their overlap
extern "C" size_t dycon_lesion_workspace(int n_vol, int X, int Y, int Z) {
    if (!les_shape_ok(n_vol, X, Y, Z)) return 0;
    return 4 * les_align((size_t)n_vol * X * Y * Z * sizeof(int));
}

extern "C" int dycon_lesion_counts(const int* root_pred, const int* root_gt, int n_vol, int X, int Y, int Z, int min_voxels,
                                   long long* counts, void* workspace, size_t ws_bytes, dycon_stream_t stream) {
    DYCON_REQUIRE(root_pred && root_gt && counts && workspace, "lesion_counts: null pointer");
    DYCON_REQUIRE(les_shape_ok(n_vol, X, Y, Z), "lesion_counts: %d volumes of %dx%dx%d (every axis 1..%d, at most 65535 volumes and "
                  "2^31 - 1 voxels in one call)", n_vol, X, Y, Z, LES_MAX_AXIS);
    DYCON_REQUIRE(min_voxels >= 1, "lesion_counts: min_voxels = %d (at least 1)", min_voxels);
    const size_t need = dycon_lesion_workspace(n_vol, X, Y, Z);
    DYCON_REQUIRE(ws_bytes >= need, "lesion_counts: workspace of %zu bytes, %zu needed", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const long long V = (long long)X * Y * Z;
    const size_t section = need / 4;
    int* size_p = (int*)workspace;
    int* over_p = (int*)((char*)workspace + section);
    int* size_g = (int*)((char*)workspace + 2 * section);
    int* over_g = (int*)((char*)workspace + 3 * section);
    if (hipMemsetAsync(workspace, 0, need, st) != hipSuccess ||
        hipMemsetAsync(counts, 0, (size_t)n_vol * LES_FIELDS * sizeof(long long), st) != hipSuccess) {
        dycon_set_error("lesion_counts: hipMemsetAsync failed");
        return DYCON_ERR_LAUNCH;
    }
    dim3 grid(les_grid(V), n_vol);
    les_sizes_kernel<<<grid, 256, 0, st>>>(root_pred, root_gt, V, size_p, size_g);
    les_overlaps_kernel<<<grid, 256, 0, st>>>(root_pred, root_gt, V, min_voxels, size_p, size_g, over_p, over_g);
    les_counts_kernel<<<grid, 256, 0, st>>>(root_pred, root_gt, V, min_voxels, size_p, over_p, size_g, over_g,
                                           (unsigned long long*)counts);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}
