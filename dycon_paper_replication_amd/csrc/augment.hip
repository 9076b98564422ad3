// Augmentation on the batch-assembly path (dataloaders/device_augment.py): the reference's RandomRot in front of the chain of
// csrc/datapath.hip and its CreateOnehotLabel behind it, in the same one launch per batch.
//
// RandomRot (code/dataloaders/isles22.py:24-28, :198-209) is scipy.ndimage.rotate(x, angle, order=0, reshape=False) about the last
// axis: the only augmentation of the reference that is not a permutation of voxels -- but still a gather.  scipy maps every output
// index (rx, ry) of a plane to the source coordinate m @ (rx, ry) + off in fp64, drops it when it lies outside [0, n - 1] on either
// axis (mode='constant', tested BEFORE the rounding) and reads the voxel at floor(c + 0.5).  The shape is kept, so crop origin, rot90
// count and flip address the rotated volume exactly as they address the stored one in datapath.hip, and the rotated volume never
// exists: output (i, j) -> index (rx, ry) of the rotated volume as there -> source (sx, sy) of the stored volume here.  The last axis
// is untouched, so an output row is still zero or one run of one source row: one (sx, sy) per thread, four consecutive elements,
// 16-byte stores.  The one-hot planes (label == c) are formed from the four labels a thread holds anyway.
//
// The source coordinates must round as scipy's C does: one operation, one rounding.  hipcc contracts a * b + c into an FMA by default
// for device code; the pragma below switches that off for the whole file (the Makefile passes -ffp-contract=off for it as well).
#include "common.h"
#include "gather_store.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

struct RotJobs {
    dycon_rot_job_t j[DYCON_CROP_JOBS_MAX];
};
struct Rotation {
    double m[4], off[2];
};

// scipy's source voxel of index (rx, ry) of the rotated plane; false: the coordinate lies outside the stored plane (reads as 0).
// The sums are scipy's, in its order, from 0.0.  The test is written so that a NaN fails it; what passes gives
// 0 <= floor(c + 0.5) <= n - 1, because c <= n - 1 and n - 1 is an integer.
__device__ __forceinline__ bool rot_source(int rx, int ry, int X, int Y, const double (&m)[4], const double (&off)[2], int& sx,
                                           int& sy) {
    const double x = (double)rx, y = (double)ry;
    const double cx = ((0.0 + x * m[0]) + y * m[1]) + off[0];
    const double cy = ((0.0 + x * m[2]) + y * m[3]) + off[1];
    if (!(cx >= 0.0 && cx <= (double)(X - 1) && cy >= 0.0 && cy <= (double)(Y - 1))) return false;
    sx = (int)floor(cx + 0.5), sy = (int)floor(cy + 0.5);
    return true;
}

// blockIdx.y = output sample; blockIdx.x strides over its P0 * P1 rows x G groups of 4 elements, as assemble_batch_kernel of
// datapath.hip does.  LB: label bytes (1 | 8); OB: one-hot element bytes (0: none | 1 | 4 | 8)
template <int LB, int OB>
__global__ __launch_bounds__(256) void assemble_batch_rot_kernel(const float* __restrict__ images, const uint8_t* __restrict__ labels,
                                                                 RotJobs jobs, int P0, int P1, int P2, int G, int vec,
                                                                 float* __restrict__ out_image, void* __restrict__ out_label,
                                                                 void* __restrict__ out_onehot, int C) {
    const dycon_rot_job_t& jb = jobs.j[blockIdx.y];
    const long long per = (long long)P0 * P1 * G;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long long)gridDim.x * 256) {
        const int g = (int)(e % G);
        const int row = (int)(e / G);
        const int j = row % P1, i = row / P1;
        // output (i, j) -> index (a, b) of the crop: undo the flip, then np.rot90(k) (odd k only with P0 == P1)
        const int fi = jb.flip_axis == 0 ? P0 - 1 - i : i;
        const int fj = jb.flip_axis == 1 ? P1 - 1 - j : j;
        int a, b;
        switch (jb.k) {
            case 1: a = fj; b = P1 - 1 - fi; break;
            case 2: a = P0 - 1 - fi; b = P1 - 1 - fj; break;
            case 3: a = P0 - 1 - fj; b = fi; break;
            default: a = fi; b = fj; break;
        }
        const int rx = jb.ox + a, ry = jb.oy + b;                      // index into the rotated volume; outside: the zero pad
        bool inside = (unsigned)rx < (unsigned)jb.X && (unsigned)ry < (unsigned)jb.Y;
        int sx = rx, sy = ry;
        if (inside && jb.rotate) inside = rot_source(rx, ry, jb.X, jb.Y, jb.m, jb.off, sx, sy);
        const int z0 = 4 * g, sz0 = jb.oz + z0;
        const int n = min(4, P2 - z0);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        uint8_t l[4] = {0, 0, 0, 0};
        if (inside) {
            const long long src = ((long long)sx * jb.Y + sy) * jb.Z;
            const float* ip = images + jb.image_off + src;
            const uint8_t* lp = labels + jb.label_off + src;
            if (sz0 >= 0 && sz0 + 3 < jb.Z && n == 4) {
                // whole group inside the source row; the run starts at an arbitrary element, so no alignment beyond the
                // element's own is promised to the compiler
                __builtin_memcpy(v, ip + sz0, 16);
                __builtin_memcpy(l, lp + sz0, 4);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < n && (unsigned)(sz0 + t) < (unsigned)jb.Z) {
                        v[t] = ip[sz0 + t];
                        l[t] = lp[sz0 + t];
                    }
            }
        }
        const long long r = ((long long)i * P1 + j) * P2 + z0;          // inside one (P0, P1, P2) block
        const long long vox = (long long)P0 * P1 * P2;
        store_group(out_image + blockIdx.y * vox + r, v, n, vec);
        if constexpr (LB == 1) {
            store_group((uint8_t*)out_label + blockIdx.y * vox + r, l, n, vec);
        } else {
            const long long w[4] = {l[0], l[1], l[2], l[3]};
            store_group((long long*)out_label + blockIdx.y * vox + r, w, n, vec);
        }
        if constexpr (OB != 0) {
            typedef typename Elem<OB>::type O;
            O* op = (O*)out_onehot + (long long)blockIdx.y * C * vox + r;
            for (int c = 0; c < C; ++c) {                              // a label >= C sets no plane
                const O h[4] = {(O)(l[0] == c), (O)(l[1] == c), (O)(l[2] == c), (O)(l[3] == c)};
                store_group(op + c * vox, h, n, vec);
            }
        }
    }
}

// a whole (X, Y, Z) volume of T: one thread per four consecutive z elements of an output row (i, j)
template <typename T>
__global__ __launch_bounds__(256) void rotate_nearest_kernel(const T* __restrict__ in, T* __restrict__ out, int X, int Y, int Z, int G,
                                                             int vec, Rotation rot) {
    const long long per = (long long)X * Y * G;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long long)gridDim.x * 256) {
        const int g = (int)(e % G);
        const int row = (int)(e / G);
        const int j = row % Y, i = row / Y;
        const int z0 = 4 * g, n = min(4, Z - z0);
        T v[4] = {0, 0, 0, 0};
        int sx, sy;
        if (rot_source(i, j, X, Y, rot.m, rot.off, sx, sy)) {
            const T* p = in + ((long long)sx * Y + sy) * Z + z0;
            if (n == 4) __builtin_memcpy(v, p, 4 * sizeof(T));
            else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < n) v[t] = p[t];
            }
        }
        store_group(out + ((long long)i * Y + j) * Z + z0, v, n, vec);
    }
}

bool finite6(const double* m, const double* off) {
    return isfinite(m[0]) && isfinite(m[1]) && isfinite(m[2]) && isfinite(m[3]) && isfinite(off[0]) && isfinite(off[1]);
}

template <int LB>
void launch_rot(int onehot_bytes, dim3 grid, hipStream_t st, const float* images, const uint8_t* labels, const RotJobs& jobs, int P0,
                int P1, int P2, int G, int vec, float* out_image, void* out_label, void* out_onehot, int C) {
#define ROT_ARGS images, labels, jobs, P0, P1, P2, G, vec, out_image, out_label, out_onehot, C
    switch (onehot_bytes) {
        case 1: assemble_batch_rot_kernel<LB, 1><<<grid, 256, 0, st>>>(ROT_ARGS); break;
        case 4: assemble_batch_rot_kernel<LB, 4><<<grid, 256, 0, st>>>(ROT_ARGS); break;
        case 8: assemble_batch_rot_kernel<LB, 8><<<grid, 256, 0, st>>>(ROT_ARGS); break;
        default: assemble_batch_rot_kernel<LB, 0><<<grid, 256, 0, st>>>(ROT_ARGS); break;
    }
#undef ROT_ARGS
}

}  // namespace

extern "C" int dycon_assemble_batch_rot(const float* images, const uint8_t* labels, const dycon_rot_job_t* jobs_host, int njobs,
                                        int P0, int P1, int P2, float* out_image, void* out_label, int label_bytes, void* out_onehot,
                                        int onehot_classes, int onehot_bytes, dycon_stream_t stream) {
    DYCON_REQUIRE(images && labels && jobs_host && out_image && out_label, "assemble_batch_rot: null pointer");
    DYCON_REQUIRE(njobs >= 1 && njobs <= DYCON_CROP_JOBS_MAX, "assemble_batch_rot: 1..%d jobs per launch, got %d", DYCON_CROP_JOBS_MAX,
                  njobs);
    DYCON_REQUIRE(P0 > 0 && P1 > 0 && P2 > 0, "assemble_batch_rot: patch %d x %d x %d", P0, P1, P2);
    DYCON_REQUIRE((long long)P0 * P1 <= 0x7fffffffLL, "assemble_batch_rot: patch %d x %d has too many rows", P0, P1);
    DYCON_REQUIRE(label_bytes == 1 || label_bytes == 8, "assemble_batch_rot: label_bytes must be 1 or 8, got %d", label_bytes);
    if (out_onehot) {
        DYCON_REQUIRE(onehot_classes >= 1 && onehot_classes <= 8, "assemble_batch_rot: onehot_classes must be in 1..8, got %d",
                      onehot_classes);
        DYCON_REQUIRE(onehot_bytes == 1 || onehot_bytes == 4 || onehot_bytes == 8,
                      "assemble_batch_rot: onehot_bytes must be 1, 4 or 8, got %d", onehot_bytes);
        DYCON_REQUIRE((uintptr_t)out_onehot % onehot_bytes == 0, "assemble_batch_rot: misaligned one-hot output");
    } else onehot_bytes = 0;
    DYCON_REQUIRE((uintptr_t)out_image % 4 == 0 && (uintptr_t)out_label % label_bytes == 0, "assemble_batch_rot: misaligned output");
    RotJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    for (int n = 0; n < njobs; ++n) {
        const dycon_rot_job_t& jb = jobs_host[n];
        DYCON_REQUIRE(jb.k >= 0 && jb.k <= 3, "assemble_batch_rot: job %d: k = %d is not in 0..3", n, jb.k);
        DYCON_REQUIRE(jb.flip_axis >= -1 && jb.flip_axis <= 1, "assemble_batch_rot: job %d: flip_axis = %d is not in {-1, 0, 1}", n,
                      jb.flip_axis);
        DYCON_REQUIRE(!(jb.k & 1) || P0 == P1, "assemble_batch_rot: job %d: k = %d needs P0 == P1 (patch %d x %d)", n, jb.k, P0, P1);
        DYCON_REQUIRE(jb.X > 0 && jb.Y > 0 && jb.Z > 0 && jb.image_off >= 0 && jb.label_off >= 0,
                      "assemble_batch_rot: job %d: stored shape %d x %d x %d, offsets %lld / %lld", n, jb.X, jb.Y, jb.Z, jb.image_off,
                      jb.label_off);
        const int lim = 1 << 30;   // origin + patch index stays an int
        DYCON_REQUIRE(jb.ox > -lim && jb.ox < lim && jb.oy > -lim && jb.oy < lim && jb.oz > -lim && jb.oz < lim && P0 < lim &&
                      P1 < lim && P2 < lim, "assemble_batch_rot: job %d: origin (%d, %d, %d) out of range", n, jb.ox, jb.oy, jb.oz);
        DYCON_REQUIRE(!jb.rotate || finite6(jb.m, jb.off), "assemble_batch_rot: job %d: the rotation holds a NaN or an infinity", n);
        jobs.j[n] = jb;
    }
    const int G = (P2 + 3) / 4;
    const int vec = P2 % 4 == 0 && (uintptr_t)out_image % 16 == 0 && (uintptr_t)out_label % (label_bytes == 1 ? 4 : 16) == 0 &&
                    (!out_onehot || (uintptr_t)out_onehot % (onehot_bytes == 1 ? 4 : 16) == 0);
    const long long per = (long long)P0 * P1 * G;
    const dim3 grid(cdiv(per, 256) > 1024 ? 1024 : cdiv(per, 256), njobs);
    if (label_bytes == 1)
        launch_rot<1>(onehot_bytes, grid, (hipStream_t)stream, images, labels, jobs, P0, P1, P2, G, vec, out_image, out_label,
                      out_onehot, onehot_classes);
    else
        launch_rot<8>(onehot_bytes, grid, (hipStream_t)stream, images, labels, jobs, P0, P1, P2, G, vec, out_image, out_label,
                      out_onehot, onehot_classes);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_rotate_nearest(const void* in, void* out, int elem_bytes, int X, int Y, int Z, const double* m, const double* off,
                                    dycon_stream_t stream) {
    DYCON_REQUIRE(in && out && m && off, "rotate_nearest: null pointer");
    DYCON_REQUIRE(elem_bytes == 1 || elem_bytes == 4 || elem_bytes == 8, "rotate_nearest: elements of 1, 4 or 8 bytes, got %d",
                  elem_bytes);
    DYCON_REQUIRE(X > 0 && Y > 0 && Z > 0 && (long long)X * Y <= 0x7fffffffLL, "rotate_nearest: volume %d x %d x %d", X, Y, Z);
    DYCON_REQUIRE((uintptr_t)in % elem_bytes == 0 && (uintptr_t)out % elem_bytes == 0, "rotate_nearest: misaligned pointer");
    const unsigned long long bytes = (unsigned long long)X * Y * Z * elem_bytes;
    DYCON_REQUIRE((uintptr_t)in + bytes <= (uintptr_t)out || (uintptr_t)out + bytes <= (uintptr_t)in,
                  "rotate_nearest: the output overlaps the input");
    DYCON_REQUIRE(finite6(m, off), "rotate_nearest: the rotation holds a NaN or an infinity");
    Rotation rot;
    memcpy(rot.m, m, sizeof(rot.m));
    memcpy(rot.off, off, sizeof(rot.off));
    const int G = (Z + 3) / 4;
    const int vec = Z % 4 == 0 && (uintptr_t)out % (elem_bytes == 1 ? 4 : 16) == 0;
    const long long per = (long long)X * Y * G;
    const dim3 grid(cdiv(per, 256) > 2048 ? 2048 : cdiv(per, 256));
    hipStream_t st = (hipStream_t)stream;
    if (elem_bytes == 1)
        rotate_nearest_kernel<uint8_t><<<grid, 256, 0, st>>>((const uint8_t*)in, (uint8_t*)out, X, Y, Z, G, vec, rot);
    else if (elem_bytes == 4)
        rotate_nearest_kernel<uint32_t><<<grid, 256, 0, st>>>((const uint32_t*)in, (uint32_t*)out, X, Y, Z, G, vec, rot);
    else
        rotate_nearest_kernel<unsigned long long>
            <<<grid, 256, 0, st>>>((const unsigned long long*)in, (unsigned long long*)out, X, Y, Z, G, vec, rot);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}
