// Training batches assembled on the device from a volume cache in HBM (dataloaders/device_cache.py).
//
// The reference's training pipelines are RandomCrop -> RandomRotFlip -> ToTensor on the host (code/dataloaders/brats19.py:198-283,
// pancreas.py, isles22.py): a conditional zero pad, a crop, np.rot90(k) about the first two axes, a flip of axis 0 or 1 and a
// cast.  All of them are gathers, so one launch writes the whole (B, 1, P0, P1, P2) batch and its labels from the cached cases:
//   - the pad is never materialised: the crop origin is given in STORED coordinates (crop offset - pad, possibly negative) and a
//     source index outside the stored volume reads as 0;
//   - the last axis is neither rotated nor flipped, so an output row (b, i, j, :) is zero or one run of one source row with zero
//     ends: a thread maps its row (i, j) -> (sx, sy) once and moves 4 consecutive elements of it;
//   - image fp32 -> fp32; labels uint8 -> uint8 (packed) or int64 (what ToTensor yields).
// The job descriptors travel in the kernel arguments (<= DYCON_CROP_JOBS_MAX of them): no table on the device, no copy, nothing
// that has to outlive the call.
#include "common.h"

struct CropJobs {
    dycon_crop_job_t j[DYCON_CROP_JOBS_MAX];
};

// blockIdx.y = output sample; blockIdx.x strides over its P0 * P1 rows x G groups of 4 elements.  vec: P2 % 4 == 0 and aligned
// outputs (16-byte image / int64 stores, 4-byte packed label stores); otherwise every element is stored on its own.
template <int LB>
__global__ __launch_bounds__(256) void assemble_batch_kernel(const float* __restrict__ images, const uint8_t* __restrict__ labels,
                                                             CropJobs jobs, int P0, int P1, int P2, int G, int vec,
                                                             float* __restrict__ out_image, void* __restrict__ out_label) {
    const dycon_crop_job_t jb = jobs.j[blockIdx.y];
    const long long per = (long long)P0 * P1 * G;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long long)gridDim.x * 256) {
        const int g = (int)(e % G);
        const int row = (int)(e / G);
        const int j = row % P1, i = row / P1;
        // output (i, j) -> index (a, b) of the crop: undo the flip, then np.rot90(k): r[i][j] = m[j][N1-1-i] | m[N0-1-i][N1-1-j] |
        // m[N0-1-j][i] for k = 1 | 2 | 3 (odd k only with P0 == P1)
        const int fi = jb.flip_axis == 0 ? P0 - 1 - i : i;
        const int fj = jb.flip_axis == 1 ? P1 - 1 - j : j;
        int a, b;
        switch (jb.k) {
            case 1: a = fj; b = P1 - 1 - fi; break;
            case 2: a = P0 - 1 - fi; b = P1 - 1 - fj; break;
            case 3: a = P0 - 1 - fj; b = fi; break;
            default: a = fi; b = fj; break;
        }
        const int sx = jb.ox + a, sy = jb.oy + b;
        const int z0 = 4 * g, sz0 = jb.oz + z0;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        uint8_t l[4] = {0, 0, 0, 0};
        if ((unsigned)sx < (unsigned)jb.X && (unsigned)sy < (unsigned)jb.Y) {
            const long long src = ((long long)sx * jb.Y + sy) * jb.Z;
            const float* ip = images + jb.image_off + src;
            const uint8_t* lp = labels + jb.label_off + src;
            if (sz0 >= 0 && sz0 + 3 < jb.Z && z0 + 3 < P2) {
                // whole group inside the source row; the run starts at an arbitrary element, so no alignment beyond the
                // element's own is promised to the compiler
                __builtin_memcpy(v, ip + sz0, 16);
                __builtin_memcpy(l, lp + sz0, 4);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (z0 + t < P2 && (unsigned)(sz0 + t) < (unsigned)jb.Z) {
                        v[t] = ip[sz0 + t];
                        l[t] = lp[sz0 + t];
                    }
            }
        }
        const long long o = (((long long)blockIdx.y * P0 + i) * P1 + j) * P2 + z0;
        if (vec) {
            *reinterpret_cast<float4*>(out_image + o) = make_float4(v[0], v[1], v[2], v[3]);
            if constexpr (LB == 1) {
                *reinterpret_cast<uchar4*>((uint8_t*)out_label + o) = make_uchar4(l[0], l[1], l[2], l[3]);
            } else {
                long long* q = (long long*)out_label + o;
                *reinterpret_cast<longlong2*>(q) = make_longlong2(l[0], l[1]);
                *reinterpret_cast<longlong2*>(q + 2) = make_longlong2(l[2], l[3]);
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (z0 + t < P2) {
                    out_image[o + t] = v[t];
                    if constexpr (LB == 1) ((uint8_t*)out_label)[o + t] = l[t];
                    else ((long long*)out_label)[o + t] = l[t];
                }
        }
    }
}

extern "C" int dycon_assemble_batch(const float* images, const uint8_t* labels, const dycon_crop_job_t* jobs_host, int njobs,
                                    int P0, int P1, int P2, float* out_image, void* out_label, int label_bytes,
                                    dycon_stream_t stream) {
    DYCON_REQUIRE(images && labels && jobs_host && out_image && out_label, "assemble_batch: null pointer");
    DYCON_REQUIRE(njobs >= 1 && njobs <= DYCON_CROP_JOBS_MAX, "assemble_batch: 1..%d jobs per launch, got %d", DYCON_CROP_JOBS_MAX,
                  njobs);
    DYCON_REQUIRE(P0 > 0 && P1 > 0 && P2 > 0, "assemble_batch: patch %d x %d x %d", P0, P1, P2);
    DYCON_REQUIRE((long long)P0 * P1 <= 0x7fffffffLL, "assemble_batch: patch %d x %d has too many rows", P0, P1);
    DYCON_REQUIRE(label_bytes == 1 || label_bytes == 8, "assemble_batch: label_bytes must be 1 or 8, got %d", label_bytes);
    CropJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    for (int n = 0; n < njobs; ++n) {
        const dycon_crop_job_t& jb = jobs_host[n];
        DYCON_REQUIRE(jb.k >= 0 && jb.k <= 3, "assemble_batch: job %d: k = %d is not in 0..3", n, jb.k);
        DYCON_REQUIRE(jb.flip_axis >= -1 && jb.flip_axis <= 1, "assemble_batch: job %d: flip_axis = %d is not in {-1, 0, 1}", n,
                      jb.flip_axis);
        DYCON_REQUIRE(!(jb.k & 1) || P0 == P1, "assemble_batch: job %d: k = %d needs P0 == P1 (patch %d x %d)", n, jb.k, P0, P1);
        DYCON_REQUIRE(jb.X > 0 && jb.Y > 0 && jb.Z > 0 && jb.image_off >= 0 && jb.label_off >= 0,
                      "assemble_batch: job %d: stored shape %d x %d x %d, offsets %lld / %lld", n, jb.X, jb.Y, jb.Z, jb.image_off,
                      jb.label_off);
        const int lim = 1 << 30;   // origin + patch index stays an int
        DYCON_REQUIRE(jb.ox > -lim && jb.ox < lim && jb.oy > -lim && jb.oy < lim && jb.oz > -lim && jb.oz < lim && P0 < lim &&
                      P1 < lim && P2 < lim, "assemble_batch: job %d: origin (%d, %d, %d) out of range", n, jb.ox, jb.oy, jb.oz);
        jobs.j[n] = jb;
    }
    const int G = (P2 + 3) / 4;
    const int vec = P2 % 4 == 0 && (uintptr_t)out_image % 16 == 0 && (uintptr_t)out_label % (label_bytes == 1 ? 4 : 16) == 0;
    const long long per = (long long)P0 * P1 * G;
    const dim3 grid(cdiv(per, 256) > 1024 ? 1024 : cdiv(per, 256), njobs);
    if (label_bytes == 1)
        assemble_batch_kernel<1><<<grid, 256, 0, stream>>>(images, labels, jobs, P0, P1, P2, G, vec, out_image, out_label);
    else
        assemble_batch_kernel<8><<<grid, 256, 0, stream>>>(images, labels, jobs, P0, P1, P2, G, vec, out_image, out_label);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}
