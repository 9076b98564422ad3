// Interpolating geometric gathers (dataloaders/device_warp.py): scipy.ndimage.affine_transform / map_coordinates with
// mode='constant', cval=0, order 0 and 1, on the batch-assembly path and for one volume; and the pointwise intensity augmentation.
//
// An output index (i0, i1, i2) has the source coordinate, in fp64, every operation rounded on its own,
//     c_d = (((0.0 + i0 * M[d,0]) + i1 * M[d,1]) + i2 * M[d,2]) + off_d     [+ (double)disp_d: a displacement field, map_coordinates]
// and reads +0 unless 0 <= c_d <= n_d - 1 on every axis (the test comes before any rounding).  Order 1 (images): f = floor(c),
// t = c - f, w0 = 1 - t, w1 = 1 - w0 (scipy forms the last spline weight as one minus the others), and the eight corners are
// summed in scipy's order, from 0.0, dx outermost and dz innermost, each as ((v[f + d] * wx) * wy) * wz; a corner index == n (only
// where t == 0 on that axis) contributes v = 0.  fp32 outputs hide most of these choices behind their rounding; fp64 outputs
// (dycon_warp_volume) show every one.  Order 0 (labels): v[floor(c + 0.5)], the rule of csrc/augment.hip.  The file is built with
// -ffp-contract=off and says so itself below.
//
// dycon_assemble_batch_warp is dycon_assemble_batch_rot's launch with that source: an output voxel is taken back through the flip
// and np.rot90 to the patch index (a, b, z) exactly as there, (a, b, z) is the (i0, i1, i2) above, and the displacement is read at
// (a, b, z).  The warped volume never exists.  One thread holds four consecutive z of an output row, as in the other two assembly
// kernels, so the stores stay 16 bytes wide; the reads are a gather and are left to the caches.  First version, not tuned.
#include "common.h"
#include "gather_store.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

struct WarpJobs {
    dycon_warp_job_t j[DYCON_CROP_JOBS_MAX];
};
struct Affine {
    double m[9], off[3];
};

// the source coordinate of index (i0, i1, i2); false: outside [0, n - 1] on some axis (a NaN fails the test as well)
__device__ __forceinline__ bool warp_coord(int i0, int i1, int i2, const double (&m)[9], const double (&off)[3], const float* disp,
                                           long long dstride, int X, int Y, int Z, double (&c)[3]) {
    const double x = (double)i0, y = (double)i1, z = (double)i2;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        c[d] = (((0.0 + x * m[3 * d]) + y * m[3 * d + 1]) + z * m[3 * d + 2]) + off[d];
        if (disp) c[d] = c[d] + (double)disp[d * dstride];
    }
    return c[0] >= 0.0 && c[0] <= (double)(X - 1) && c[1] >= 0.0 && c[1] <= (double)(Y - 1) && c[2] >= 0.0 && c[2] <= (double)(Z - 1);
}

// order 1 at an inside coordinate: scipy's eight-corner sum of a (X, Y, Z) volume of T, in fp64
template <typename T> __device__ __forceinline__ double interp1(const T* __restrict__ v, int X, int Y, int Z, const double (&c)[3]) {
    const double fx = floor(c[0]), fy = floor(c[1]), fz = floor(c[2]);
    const double lx = 1.0 - (c[0] - fx), ly = 1.0 - (c[1] - fy), lz = 1.0 - (c[2] - fz);      // the lower corner's weights
    const double hx = 1.0 - lx, hy = 1.0 - ly, hz = 1.0 - lz;                                  // ... and the upper one's
    const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    double acc = 0.0;
#pragma unroll
    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dz = 0; dz < 2; ++dz) {
                const int sx = ix + dx, sy = iy + dy, sz = iz + dz;
                double val = 0.0;                                  // a corner at index n lies outside the volume: 0
                if (sx < X && sy < Y && sz < Z) val = (double)v[((long long)sx * Y + sy) * Z + sz];
                acc += ((val * (dx ? hx : lx)) * (dy ? hy : ly)) * (dz ? hz : lz);
            }
    return acc;
}

// order 0 at an inside coordinate: 0 <= floor(c + 0.5) <= n - 1, because c <= n - 1 and n - 1 is an integer
__device__ __forceinline__ long long nearest0(int Y, int Z, const double (&c)[3]) {
    return ((long long)floor(c[0] + 0.5) * Y + (long long)floor(c[1] + 0.5)) * Z + (long long)floor(c[2] + 0.5);
}

// blockIdx.y = output sample; blockIdx.x strides over its P0 * P1 rows x G groups of 4 elements, as assemble_batch_rot_kernel of
// augment.hip does.  LB: label bytes (1 | 8); OB: one-hot element bytes (0: none | 1 | 4 | 8).  disp: (njobs, 3, P0, P1, P2) or null
template <int LB, int OB>
__global__ __launch_bounds__(256) void assemble_batch_warp_kernel(const float* __restrict__ images, const uint8_t* __restrict__ labels,
                                                                  WarpJobs jobs, const float* __restrict__ disp, int P0, int P1, int P2,
                                                                  int G, int vec, float* __restrict__ out_image,
                                                                  void* __restrict__ out_label, void* __restrict__ out_onehot, int C) {
    const dycon_warp_job_t& jb = jobs.j[blockIdx.y];
    const long long per = (long long)P0 * P1 * G;
    const long long vox = (long long)P0 * P1 * P2;
    const float* ip = images + jb.image_off;
    const uint8_t* lp = labels + jb.label_off;
    const float* dp = disp && jb.elastic ? disp + (long long)blockIdx.y * 3 * vox : nullptr;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long long)gridDim.x * 256) {
        const int g = (int)(e % G);
        const int row = (int)(e / G);
        const int j = row % P1, i = row / P1;
        // output (i, j) -> index (a, b) of the patch: undo the flip, then np.rot90(k) (odd k only with P0 == P1)
        const int fi = jb.flip_axis == 0 ? P0 - 1 - i : i;
        const int fj = jb.flip_axis == 1 ? P1 - 1 - j : j;
        int a, b;
        switch (jb.k) {
            case 1: a = fj; b = P1 - 1 - fi; break;
            case 2: a = P0 - 1 - fi; b = P1 - 1 - fj; break;
            case 3: a = P0 - 1 - fj; b = fi; break;
            default: a = fi; b = fj; break;
        }
        const int z0 = 4 * g;
        const int n = min(4, P2 - z0);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        uint8_t l[4] = {0, 0, 0, 0};
        if (jb.warp) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t >= n) continue;
                double c[3];
                const float* d = dp ? dp + ((long long)a * P1 + b) * P2 + z0 + t : nullptr;
                if (warp_coord(a, b, z0 + t, jb.m, jb.off, d, vox, jb.X, jb.Y, jb.Z, c)) {
                    v[t] = (float)interp1(ip, jb.X, jb.Y, jb.Z, c);
                    l[t] = lp[nearest0(jb.Y, jb.Z, c)];
                }
            }
        } else {                                                       // the plain crop: dycon_assemble_batch's source and bits
            const int sx = jb.ox + a, sy = jb.oy + b;
            if ((unsigned)sx < (unsigned)jb.X && (unsigned)sy < (unsigned)jb.Y) {
                const long long src = ((long long)sx * jb.Y + sy) * jb.Z;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int sz = jb.oz + z0 + t;
                    if (t < n && (unsigned)sz < (unsigned)jb.Z) {
                        v[t] = ip[src + sz];
                        l[t] = lp[src + sz];
                    }
                }
            }
        }
        const long long r = ((long long)i * P1 + j) * P2 + z0;          // inside one (P0, P1, P2) block
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

// one (X, Y, Z) volume -> (O0, O1, O2); ORDER 1: T = float | double is interpolated, ORDER 0: T of 1, 4 or 8 bytes is moved
template <typename T, int ORDER>
__global__ __launch_bounds__(256) void warp_volume_kernel(const T* __restrict__ in, int X, int Y, int Z, T* __restrict__ out, int O0,
                                                          int O1, int O2, Affine af, const float* __restrict__ disp) {
    const long long total = (long long)O0 * O1 * O2;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int i2 = (int)(e % O2);
        const long long q = e / O2;
        const int i1 = (int)(q % O1), i0 = (int)(q / O1);
        double c[3];
        T o = 0;
        if (warp_coord(i0, i1, i2, af.m, af.off, disp ? disp + e : nullptr, total, X, Y, Z, c)) {
            if constexpr (ORDER == 1) o = (T)interp1(in, X, Y, Z, c);
            else o = in[nearest0(Y, Z, c)];
        }
        out[e] = o;
    }
}

struct IntensityJobs {
    long long sample[DYCON_CROP_JOBS_MAX];
    double p[DYCON_CROP_JOBS_MAX][5];       // gain, bias, gamma, lo, hi
};

__global__ __launch_bounds__(256) void intensity_kernel(const float* __restrict__ x, float* __restrict__ y, long long V,
                                                        IntensityJobs jobs) {
    const long long base = jobs.sample[blockIdx.y] * V;
    const double gain = jobs.p[blockIdx.y][0], bias = jobs.p[blockIdx.y][1], gamma = jobs.p[blockIdx.y][2];
    const double lo = jobs.p[blockIdx.y][3], hi = jobs.p[blockIdx.y][4];
    const double span = hi - lo;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < V; e += (long long)gridDim.x * 256) {
        double v = (double)x[base + e] * gain + bias;
        v = v < lo ? lo : (v > hi ? hi : v);                           // a NaN stays a NaN, as with np.clip
        double u = (v - lo) / span;
        if (gamma != 1.0) u = pow(u, gamma);
        y[base + e] = (float)(u * span + lo);
    }
}

bool finite_n(const double* p, int n) {
    for (int i = 0; i < n; ++i)
        if (!isfinite(p[i])) return false;
    return true;
}

template <int LB>
void launch_warp(int onehot_bytes, dim3 grid, hipStream_t st, const float* images, const uint8_t* labels, const WarpJobs& jobs,
                 const float* disp, int P0, int P1, int P2, int G, int vec, float* out_image, void* out_label, void* out_onehot, int C) {
#define WARP_ARGS images, labels, jobs, disp, P0, P1, P2, G, vec, out_image, out_label, out_onehot, C
    switch (onehot_bytes) {
        case 1: assemble_batch_warp_kernel<LB, 1><<<grid, 256, 0, st>>>(WARP_ARGS); break;
        case 4: assemble_batch_warp_kernel<LB, 4><<<grid, 256, 0, st>>>(WARP_ARGS); break;
        case 8: assemble_batch_warp_kernel<LB, 8><<<grid, 256, 0, st>>>(WARP_ARGS); break;
        default: assemble_batch_warp_kernel<LB, 0><<<grid, 256, 0, st>>>(WARP_ARGS); break;
    }
#undef WARP_ARGS
}

}  // namespace

extern "C" int dycon_assemble_batch_warp(const float* images, const uint8_t* labels, const dycon_warp_job_t* jobs_host, int njobs,
                                         const float* displacement, int P0, int P1, int P2, float* out_image, void* out_label,
                                         int label_bytes, void* out_onehot, int onehot_classes, int onehot_bytes,
                                         dycon_stream_t stream) {
    DYCON_REQUIRE(images && labels && jobs_host && out_image && out_label, "assemble_batch_warp: null pointer");
    DYCON_REQUIRE(njobs >= 1 && njobs <= DYCON_CROP_JOBS_MAX, "assemble_batch_warp: 1..%d jobs per launch, got %d", DYCON_CROP_JOBS_MAX,
                  njobs);
    DYCON_REQUIRE(P0 > 0 && P1 > 0 && P2 > 0, "assemble_batch_warp: patch %d x %d x %d", P0, P1, P2);
    DYCON_REQUIRE((long long)P0 * P1 <= 0x7fffffffLL, "assemble_batch_warp: patch %d x %d has too many rows", P0, P1);
    DYCON_REQUIRE(label_bytes == 1 || label_bytes == 8, "assemble_batch_warp: label_bytes must be 1 or 8, got %d", label_bytes);
    if (out_onehot) {
        DYCON_REQUIRE(onehot_classes >= 1 && onehot_classes <= 8, "assemble_batch_warp: onehot_classes must be in 1..8, got %d",
                      onehot_classes);
        DYCON_REQUIRE(onehot_bytes == 1 || onehot_bytes == 4 || onehot_bytes == 8,
                      "assemble_batch_warp: onehot_bytes must be 1, 4 or 8, got %d", onehot_bytes);
        DYCON_REQUIRE((uintptr_t)out_onehot % onehot_bytes == 0, "assemble_batch_warp: misaligned one-hot output");
    } else onehot_bytes = 0;
    DYCON_REQUIRE((uintptr_t)out_image % 4 == 0 && (uintptr_t)out_label % label_bytes == 0 && (uintptr_t)displacement % 4 == 0,
                  "assemble_batch_warp: misaligned pointer");
    WarpJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    for (int n = 0; n < njobs; ++n) {
        const dycon_warp_job_t& jb = jobs_host[n];
        DYCON_REQUIRE(jb.k >= 0 && jb.k <= 3, "assemble_batch_warp: job %d: k = %d is not in 0..3", n, jb.k);
        DYCON_REQUIRE(jb.flip_axis >= -1 && jb.flip_axis <= 1, "assemble_batch_warp: job %d: flip_axis = %d is not in {-1, 0, 1}", n,
                      jb.flip_axis);
        DYCON_REQUIRE(!(jb.k & 1) || P0 == P1, "assemble_batch_warp: job %d: k = %d needs P0 == P1 (patch %d x %d)", n, jb.k, P0, P1);
        DYCON_REQUIRE(jb.X > 0 && jb.Y > 0 && jb.Z > 0 && jb.image_off >= 0 && jb.label_off >= 0,
                      "assemble_batch_warp: job %d: stored shape %d x %d x %d, offsets %lld / %lld", n, jb.X, jb.Y, jb.Z, jb.image_off,
                      jb.label_off);
        const int lim = 1 << 30;   // origin + patch index stays an int
        DYCON_REQUIRE(jb.ox > -lim && jb.ox < lim && jb.oy > -lim && jb.oy < lim && jb.oz > -lim && jb.oz < lim && P0 < lim &&
                      P1 < lim && P2 < lim, "assemble_batch_warp: job %d: origin (%d, %d, %d) out of range", n, jb.ox, jb.oy, jb.oz);
        DYCON_REQUIRE(!jb.warp || (finite_n(jb.m, 9) && finite_n(jb.off, 3)),
                      "assemble_batch_warp: job %d: the transform holds a NaN or an infinity", n);
        DYCON_REQUIRE(!jb.elastic || (jb.warp && displacement), "assemble_batch_warp: job %d: elastic needs warp and a displacement", n);
        jobs.j[n] = jb;
    }
    const int G = (P2 + 3) / 4;
    const int vec = P2 % 4 == 0 && (uintptr_t)out_image % 16 == 0 && (uintptr_t)out_label % (label_bytes == 1 ? 4 : 16) == 0 &&
                    (!out_onehot || (uintptr_t)out_onehot % (onehot_bytes == 1 ? 4 : 16) == 0);
    const long long per = (long long)P0 * P1 * G;
    const dim3 grid(cdiv(per, 256) > 1024 ? 1024 : cdiv(per, 256), njobs);
    if (label_bytes == 1)
        launch_warp<1>(onehot_bytes, grid, (hipStream_t)stream, images, labels, jobs, displacement, P0, P1, P2, G, vec, out_image,
                       out_label, out_onehot, onehot_classes);
    else
        launch_warp<8>(onehot_bytes, grid, (hipStream_t)stream, images, labels, jobs, displacement, P0, P1, P2, G, vec, out_image,
                       out_label, out_onehot, onehot_classes);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_warp_volume(const void* in, int X, int Y, int Z, void* out, int O0, int O1, int O2, int order, int elem_bytes,
                                 const double* m, const double* off, const float* displacement, dycon_stream_t stream) {
    DYCON_REQUIRE(in && out && m && off, "warp_volume: null pointer");
    DYCON_REQUIRE(order == 0 || order == 1, "warp_volume: order must be 0 or 1, got %d", order);
    DYCON_REQUIRE(order == 1 ? (elem_bytes == 4 || elem_bytes == 8) : (elem_bytes == 1 || elem_bytes == 4 || elem_bytes == 8),
                  "warp_volume: order %d takes elements of %s bytes, got %d", order, order ? "4 (fp32) or 8 (fp64)" : "1, 4 or 8",
                  elem_bytes);
    DYCON_REQUIRE(X > 0 && Y > 0 && Z > 0 && O0 > 0 && O1 > 0 && O2 > 0, "warp_volume: %d x %d x %d -> %d x %d x %d", X, Y, Z, O0, O1, O2);
    DYCON_REQUIRE((uintptr_t)in % elem_bytes == 0 && (uintptr_t)out % elem_bytes == 0 && (uintptr_t)displacement % 4 == 0,
                  "warp_volume: misaligned pointer");
    DYCON_REQUIRE(finite_n(m, 9) && finite_n(off, 3), "warp_volume: the transform holds a NaN or an infinity");
    Affine af;
    memcpy(af.m, m, sizeof(af.m));
    memcpy(af.off, off, sizeof(af.off));
    const long long total = (long long)O0 * O1 * O2;
    const dim3 grid(cdiv(total, 256) > 4096 ? 4096 : cdiv(total, 256));
    hipStream_t st = (hipStream_t)stream;
#define VOL_ARGS(T) (const T*)in, X, Y, Z, (T*)out, O0, O1, O2, af, displacement
    if (order == 1) {
        if (elem_bytes == 4) warp_volume_kernel<float, 1><<<grid, 256, 0, st>>>(VOL_ARGS(float));
        else warp_volume_kernel<double, 1><<<grid, 256, 0, st>>>(VOL_ARGS(double));
    } else if (elem_bytes == 1) warp_volume_kernel<uint8_t, 0><<<grid, 256, 0, st>>>(VOL_ARGS(uint8_t));
    else if (elem_bytes == 4) warp_volume_kernel<uint32_t, 0><<<grid, 256, 0, st>>>(VOL_ARGS(uint32_t));
    else warp_volume_kernel<unsigned long long, 0><<<grid, 256, 0, st>>>(VOL_ARGS(unsigned long long));
#undef VOL_ARGS
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_intensity_augment(const float* x, float* y, long long V, const long long* samples, const double* params, int n,
                                       dycon_stream_t stream) {
    DYCON_REQUIRE(x && y && params, "intensity_augment: null pointer");
    DYCON_REQUIRE(V > 0 && n > 0, "intensity_augment: %d samples of %lld voxels", n, V);
    DYCON_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)y % 4 == 0, "intensity_augment: misaligned pointer");
    for (int i = 0; i < n; ++i) {
        const double* p = params + 5 * i;
        DYCON_REQUIRE(finite_n(p, 5) && p[2] > 0.0 && p[3] < p[4],
                      "intensity_augment: sample %d: gain, bias, gamma > 0 and lo < hi must be finite", i);
        DYCON_REQUIRE(!samples || samples[i] >= 0, "intensity_augment: sample %d: negative sample number", i);
    }
    for (int i0 = 0; i0 < n; i0 += DYCON_CROP_JOBS_MAX) {
        const int m = n - i0 < DYCON_CROP_JOBS_MAX ? n - i0 : DYCON_CROP_JOBS_MAX;
        IntensityJobs jobs;
        memset(&jobs, 0, sizeof(jobs));
        for (int i = 0; i < m; ++i) {
            jobs.sample[i] = samples ? samples[i0 + i] : i0 + i;
            memcpy(jobs.p[i], params + 5 * (i0 + i), 5 * sizeof(double));
        }
        const dim3 grid(cdiv(V, 256) > 2048 ? 2048 : cdiv(V, 256), m);
        intensity_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(x, y, V, jobs);
        DYCON_LAUNCH_CHECK();
    }
    return DYCON_OK;
}
