// Model-ensemble sliding-window evaluation on the device: code/utils/test_3d_patch.py:415-476 (test_single_case_plus).
//
// The reference runs every window through two models, averages their logits ((y1_l + y1_r) / 2, :460-462), takes the softmax and
// accumulates class 1 into score / count maps on the host.  Two kernels serve that loop here:
//   - sw_gather_kernel builds the (n, 1, p0, p1, p2) batch of windows of one chunk in one launch from the UNPADDED volume and a
//     table of window origins that was uploaded once per case.  The centre pad of a volume smaller than the window (:418-439) is
//     index arithmetic: the origins are in padded coordinates, a source index outside the stored volume reads as 0 (the convention
//     of csrc/datapath.hip).  A pure copy: bit for bit the slices of the zero-padded volume.
//   - sw_accumulate_kernel<M, false> (sw_accumulate.h), M = 2..4, is the accumulate of the single-model evaluator reading the mean
//     of the models' logits: per covered voxel and class they are summed in model order in fp32 and divided by M, and class 1 of the
//     softmax is scored as dycon_sw_accumulate does for C == 2 and dycon_sw_accumulate_c for C > 2.
// The gather is a bandwidth-bound pass with coalesced access along the last axis and nothing else was tuned.  dycon_sw_finalize
// (eval.hip) turns the maps into the label and the probability.
//
// Beyond the reference (utils/sliding_window.py, Blend): dycon_sw_gather_mirror and dycon_sw_accumulate_weighted are the same two
// kernels with one more compile-time parameter each, for windows that also go through the network flipped (mirror test-time
// augmentation) and count with a per-voxel importance (Gaussian blending).  The plain instantiations are unchanged code.
#include "sw_accumulate.h"

// blockIdx.y = window of the chunk; blockIdx.x strides over its p0 * p1 rows x G groups of 4 elements of the last axis.
// MIRROR (dycon_sw_gather_mirror): the table holds (ox, oy, oz, mask) per entry and the window is written flipped along every axis
// whose mask bit is set.  Axes 0 and 1 only pick another source row; a flipped last axis reads the group's 16 bytes from the mirrored
// end of the row and reverses them, so loads and stores stay whole groups.
template <bool MIRROR>
__global__ __launch_bounds__(256) void sw_gather_kernel(const float* __restrict__ vol, int w, int h, int d, int lo0, int lo1, int lo2,
                                                        const int* __restrict__ origins, int p0, int p1, int p2, int G, int vec,
                                                        float* __restrict__ out) {
    const int* o = origins + (MIRROR ? 4 : 3) * blockIdx.y;
    int mask = 0;
    if constexpr (MIRROR) mask = o[3];
    const bool rev = mask & 4;
    // window corner in stored coordinates (negative inside the pad).  64-bit: the table is device data, and no value in it may wrap
    // a source index back into the volume
    const long long ox = (long long)o[0] - lo0, oy = (long long)o[1] - lo1, oz = (long long)o[2] - lo2;
    const long long per = (long long)p0 * p1 * G;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long long)gridDim.x * 256) {
        const int g = (int)(e % G);
        const int row = (int)(e / G);
        const int j = row % p1, i = row / p1;
        const long long sx = ox + ((mask & 1) ? p0 - 1 - i : i), sy = oy + ((mask & 2) ? p1 - 1 - j : j);
        const int z0 = 4 * g;
        // out[z0 + t] comes from source element sz0 + t, or, flipped, from sz0 + 3 - t: sz0 is the lowest source index of the group
        const long long sz0 = rev ? oz + p2 - 4 - z0 : oz + z0;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (sx >= 0 && sx < w && sy >= 0 && sy < h) {
            const float* ip = vol + (sx * h + sy) * d;
            if (sz0 >= 0 && sz0 <= d - 4 && z0 + 3 < p2) {
                __builtin_memcpy(v, ip + sz0, 16);                    // the run starts at an arbitrary element: no alignment promised
                if (rev) {
                    const float v0 = v[0], v1 = v[1];
                    v[0] = v[3]; v[1] = v[2]; v[2] = v1; v[3] = v0;
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const long long sz = rev ? sz0 + 3 - t : sz0 + t;
                    if (z0 + t < p2 && sz >= 0 && sz < d) v[t] = ip[sz];
                }
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

// `who`: the entry point's name without the dycon_ prefix; the table has 3 ints per row, with MIRROR 4
template <bool MIRROR>
static int sw_gather_launch(const char* who, const float* vol, int w, int h, int d, const int* origins_dev, int n_origins, int first, int n,
                            int p0, int p1, int p2, float* out, dycon_stream_t stream) {
    DYCON_REQUIRE(vol && origins_dev && out, "%s: null pointer", who);
    const int lim = 1 << 30;
    DYCON_REQUIRE(w > 0 && h > 0 && d > 0 && w < lim && h < lim && d < lim, "%s: volume %d x %d x %d", who, w, h, d);
    DYCON_REQUIRE(p0 > 0 && p1 > 0 && p2 > 0 && p0 < lim && p1 < lim && p2 < lim && (long long)p0 * p1 <= 0x7fffffffLL,
                  "%s: window %d x %d x %d", who, p0, p1, p2);
    DYCON_REQUIRE(n >= 1 && n <= 64 && first >= 0 && n_origins >= 1 && first <= n_origins - n,
                  "%s: windows [%d, %d + %d) of a table of %d (1..64 per launch)", who, first, first, n, n_origins);
    // :418-439: an axis shorter than the window is centre-padded, the smaller half in front
    const int lo0 = (p0 > w ? p0 - w : 0) / 2, lo1 = (p1 > h ? p1 - h : 0) / 2, lo2 = (p2 > d ? p2 - d : 0) / 2;
    const int G = (p2 + 3) / 4;
    const int vec = p2 % 4 == 0 && (uintptr_t)out % 16 == 0;
    const long long per = (long long)p0 * p1 * G;
    const dim3 grid(cdiv(per, 256) > 1024 ? 1024 : cdiv(per, 256), n);
    sw_gather_kernel<MIRROR><<<grid, 256, 0, stream>>>(vol, w, h, d, lo0, lo1, lo2, origins_dev + (MIRROR ? 4 : 3) * (long long)first, p0,
                                                       p1, p2, G, vec, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_sw_gather(const float* vol, int w, int h, int d, const int* origins_dev, int n_origins, int first, int n, int p0,
                               int p1, int p2, float* out, dycon_stream_t stream) {
    return sw_gather_launch<false>("sw_gather", vol, w, h, d, origins_dev, n_origins, first, n, p0, p1, p2, out, stream);
}

extern "C" int dycon_sw_gather_mirror(const float* vol, int w, int h, int d, const int* entries_dev, int n_entries, int first, int n,
                                      int p0, int p1, int p2, float* out, dycon_stream_t stream) {
    return sw_gather_launch<true>("sw_gather_mirror", vol, w, h, d, entries_dev, n_entries, first, n, p0, p1, p2, out, stream);
}

extern "C" int dycon_sw_accumulate_ens(const float* logits0, const float* logits1, const float* logits2, const float* logits3, int M,
                                       int C, int n_patches, int p0, int p1, int p2, const int* origins_dev, float* score, float* cnt,
                                       int D0, int D1, int D2, dycon_stream_t stream) {
    DYCON_REQUIRE(M >= 2 && M <= 4, "sw_accumulate_ens: M = %d models (2..4)", M);
    DYCON_REQUIRE(C >= 2 && C <= 8, "sw_accumulate_ens: C = %d (2..8: class 1 is scored)", C);
    SwLogits in = {{logits0, logits1, logits2, logits3}};
    for (int m = 0; m < M; ++m) DYCON_REQUIRE(in.l[m], "sw_accumulate_ens: logits of model %d are null (M = %d)", m, M);
    for (int m = M; m < 4; ++m) in.l[m] = nullptr;
    DYCON_REQUIRE(origins_dev && score && cnt, "sw_accumulate_ens: null pointer");
    if (int e = sw_check_shape("sw_accumulate_ens", n_patches, p0, p1, p2, D0, D1, D2)) return e;
    const auto launch = M == 2 ? sw_accumulate_launch<2, false> : M == 3 ? sw_accumulate_launch<3, false> : sw_accumulate_launch<4, false>;
    return launch(in, C, C == 2, n_patches, p0, p1, p2, origins_dev, score, cnt, D0, D1, D2, nullptr, nullptr, stream, {}, {});
}

// Every accumulate above with importance tables and mirrored windows: sw_accumulate_kernel<M, ALL, true>
extern "C" int dycon_sw_accumulate_weighted(const float* logits0, const float* logits1, const float* logits2, const float* logits3, int M,
                                            int C, int all_classes, int n, int p0, int p1, int p2, const int* entries_dev, const float* g0,
                                            const float* g1, const float* g2, float* score, float* cnt, int D0, int D1, int D2,
                                            const int* box_lo, const int* box_hi, dycon_stream_t stream) {
    DYCON_REQUIRE(M >= 1 && M <= 4, "sw_accumulate_weighted: M = %d models (1..4)", M);
    DYCON_REQUIRE(C >= 2 && C <= 8, "sw_accumulate_weighted: C = %d (2..8)", C);
    DYCON_REQUIRE((all_classes == 0 || all_classes == 1) && (!all_classes || M == 1),
                  "sw_accumulate_weighted: all_classes = %d with M = %d (0 | 1, and 1 takes one model)", all_classes, M);
    SwLogits in = {{logits0, logits1, logits2, logits3}};
    for (int m = 0; m < M; ++m) DYCON_REQUIRE(in.l[m], "sw_accumulate_weighted: logits of model %d are null (M = %d)", m, M);
    for (int m = M; m < 4; ++m) in.l[m] = nullptr;
    DYCON_REQUIRE(entries_dev && g0 && g1 && g2 && score && cnt, "sw_accumulate_weighted: null pointer");
    if (int e = sw_check_shape("sw_accumulate_weighted", n, p0, p1, p2, D0, D1, D2)) return e;
    DYCON_REQUIRE(!box_lo == !box_hi, "sw_accumulate_weighted: box_lo and box_hi come together or not at all");
    const int D[3] = {D0, D1, D2};
    for (int a = 0; box_lo && a < 3; ++a)
        DYCON_REQUIRE(box_lo[a] >= 0 && box_lo[a] < box_hi[a] && box_hi[a] <= D[a],
                      "sw_accumulate_weighted: box [%d, %d) on axis %d lies outside the volume (extent %d)", box_lo[a], box_hi[a], a, D[a]);
    const auto launch = all_classes ? sw_accumulate_launch<1, true, true>
                        : M == 1    ? sw_accumulate_launch<1, false, true>
                        : M == 2    ? sw_accumulate_launch<2, false, true>
                        : M == 3    ? sw_accumulate_launch<3, false, true>
                                    : sw_accumulate_launch<4, false, true>;
    return launch(in, C, !all_classes && C == 2, n, p0, p1, p2, entries_dev, score, cnt, D0, D1, D2, box_lo, box_hi, stream, {{g0, g1, g2}}, {});
}
