// Trilinear x2 up-sampling (align_corners=False) folded into the k=3 convolution that consumes it:
//
//   y = Conv3d_k3_pad1( Upsample_x2_trilinear(x) ) + bias            (networks/VNet.py:121-142, the `Upsampling` block)
//
// The composition trilinear_fwd -> conv_gemm writes and re-reads an activation 8x the size of x.  Here a workgroup owns a
// 4 x 8 x 8 tile of OUTPUT voxels and, per chunk of input channels,
//   1. stages the low-resolution halo it needs in LDS: (t/2 + 2) source points per axis for an output extent t plus the k=3
//      border, source indices clamped at both ends (an axis of extent 1 simply repeats);
//   2. forms the (t + 2)^3 up-sampled operand tile in LDS from it.  At scale 2 the per-axis taps are the constants {0.25, 0.75};
//      the association order is trilinear_fwd_kernel's (ATen's).  The ZERO PADDING of the convolution applies on the UP-SAMPLED
//      grid: a tile position outside [0, 2*Di) x [0, 2*Hi) x [0, 2*Wi) is 0, it is NOT the clamped interpolation;
//   3. runs the 27 taps through the matrix cores, A fragments read from that tile (one ds_read_b128 per lane), B fragments in the
//      dycon_pack_bfrag layout (T = 27) straight from L2 as in conv_gemm_kernel.
// fp32 storage: v_mfma_f32_16x16x4_f32 (exact fp32 FMA chain, the 1e-4 parity mode); bf16 storage: v_mfma_f32_16x16x32_bf16 with
// the up-sampled operand rounded to bf16 where the composition rounds it (its store), fp32 accumulate over all 27 taps.
// The up-sampled tensor never reaches HBM.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <typename T> struct UFrag;
template <> struct UFrag<float> { static constexpr int G = 4, KC = 16; };
template <> struct UFrag<bf16> { static constexpr int G = 8, KC = 32; };

__device__ __forceinline__ void umma(f32x4& acc, const Vec16<float>& a, const Vec16<float>& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v.x, b.v.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v.y, b.v.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v.z, b.v.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v.w, b.v.w, acc, 0, 0, 0);
}
__device__ __forceinline__ void umma(f32x4& acc, const Vec16<bf16>& a, const Vec16<bf16>& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a.v), __builtin_bit_cast(bf16x8, b.v), acc, 0, 0, 0);
}

constexpr int UC_TZ = 4, UC_TY = 8, UC_TX = 8;                                  // output tile: 256 rows, 64 per wave (wave = z plane)
constexpr int UC_UZ = UC_TZ + 2, UC_UY = UC_TY + 2, UC_UX = UC_TX + 2;          // up-sampled tile with the k=3 border
constexpr int UC_LZ = UC_TZ / 2 + 2, UC_LY = UC_TY / 2 + 2, UC_LX = UC_TX / 2 + 2;   // low-resolution halo
constexpr int UC_UV = UC_UZ * UC_UY * UC_UX, UC_LV = UC_LZ * UC_LY * UC_LX;     // 600, 144 voxels
constexpr size_t UC_LDS_PER_CU = 160 * 1024;                                    // gfx950
constexpr int UC_NTB = 4;                                                       // n-tiles (of 16 columns) per workgroup

// KMODE 0: Cin % KC == 0, LDS holds one KC-channel chunk at a time, a k-step is (tap, chunk)
//       1: the whole Cin in LDS (Cin % G == 0: 16 / 48 channels in bf16), k-steps run over the flat K = 27*Cin
template <typename T, int KMODE>
__global__ __launch_bounds__(256) void upconv_k3_kernel(const T* __restrict__ X, const T* __restrict__ Wf,
                                                        const float* __restrict__ bias, T* __restrict__ Y, int Di, int Hi, int Wi,
                                                        int Cin, int Cout, int NT, int CS, int VS, int nCC, int nKC, int tilesZ,
                                                        int tilesY, int tilesX) {
    constexpr int G = UFrag<T>::G, KC = UFrag<T>::KC;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    T* up = reinterpret_cast<T*>(lds_raw);
    T* low = up + UC_UV * VS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, kg = lane >> 4;
    int q = blockIdx.x;
    const int tx = q % tilesX; q /= tilesX;
    const int ty = q % tilesY; q /= tilesY;
    const int tz = q % tilesZ;
    const int b = q / tilesZ;
    const int Do = 2 * Di, Ho = 2 * Hi, Wo = 2 * Wi;
    const int oz0 = tz * UC_TZ, oy0 = ty * UC_TY, ox0 = tx * UC_TX;
    const int lz0 = oz0 / 2 - 1, ly0 = oy0 / 2 - 1, lx0 = ox0 / 2 - 1;      // source index of low-tile point 0 (before clamping)
    const int nt0 = blockIdx.y * UC_NTB;
    const int PV = VS / G - 1;                                             // 16-byte pieces per voxel that hold data
    const T* xb = X + (long long)b * Di * Hi * Wi * Cin;

    f32x4 acc[4][UC_NTB];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < UC_NTB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int cc = 0; cc < nCC; ++cc) {
        if (cc) __syncthreads();      // the previous chunk's fragments have been read
        // 1. low-resolution halo, clamped source indices
        for (int e = tid; e < UC_LV * PV; e += 256) {
            const int p = e % PV, v = e / PV;
            const int lx = v % UC_LX, ly = (v / UC_LX) % UC_LY, lz = v / (UC_LX * UC_LY);
            const int sz = min(max(lz0 + lz, 0), Di - 1), sy = min(max(ly0 + ly, 0), Hi - 1), sx = min(max(lx0 + lx, 0), Wi - 1);
            const T* src = xb + ((long long)(sz * Hi + sy) * Wi + sx) * Cin + cc * CS + p * G;
            const Vec16<T> val = ld16(src);
            st16(low + v * VS + p * G, val);
        }
        __syncthreads();
        // 2. the up-sampled tile; zero outside the up-sampled grid (the convolution's padding)
        for (int e = tid; e < UC_UV * PV; e += 256) {
            const int p = e % PV, v = e / PV;
            const int ux = v % UC_UX, uy = (v / UC_UX) % UC_UY, uz = v / (UC_UX * UC_UY);
            const int gz = oz0 - 1 + uz, gy = oy0 - 1 + uy, gx = ox0 - 1 + ux;
            Vec16<T> o;
            o.v = decltype(o.v){};
            if ((unsigned)gz < (unsigned)Do && (unsigned)gy < (unsigned)Ho && (unsigned)gx < (unsigned)Wo) {
                // output g = 2m: sources m-1, m with weights .25, .75; g = 2m+1: sources m, m+1 with .75, .25; g = 0 is the clamped
                // source 0 alone (ATen: src = max(-0.25, 0))
                const int az = (gz >> 1) - 1 + (gz & 1) - lz0, ay = (gy >> 1) - 1 + (gy & 1) - ly0, ax = (gx >> 1) - 1 + (gx & 1) - lx0;
                const float lz = gz == 0 ? 1.f : ((gz & 1) ? 0.25f : 0.75f);
                const float ly = gy == 0 ? 1.f : ((gy & 1) ? 0.25f : 0.75f);
                const float lx = gx == 0 ? 1.f : ((gx & 1) ? 0.25f : 0.75f);
                const float w0z = 1.f - lz, w0y = 1.f - ly, w0x = 1.f - lx;
                const T* l0 = low + ((az * UC_LY + ay) * UC_LX + ax) * VS + p * G;
                const int sy = UC_LX * VS, sz = UC_LY * UC_LX * VS;
                const Vec16<T> a000 = ld16(l0), a001 = ld16(l0 + VS), a010 = ld16(l0 + sy), a011 = ld16(l0 + sy + VS);
                const Vec16<T> a100 = ld16(l0 + sz), a101 = ld16(l0 + sz + VS), a110 = ld16(l0 + sz + sy), a111 = ld16(l0 + sz + sy + VS);
#pragma unroll
                for (int k = 0; k < G; ++k) {      // same association order as trilinear_fwd_kernel
                    const float val = w0z * (w0y * (w0x * a000.get(k) + lx * a001.get(k)) + ly * (w0x * a010.get(k) + lx * a011.get(k))) +
                                      lz * (w0y * (w0x * a100.get(k) + lx * a101.get(k)) + ly * (w0x * a110.get(k) + lx * a111.get(k)));
                    o.set(k, val);
                }
            }
            st16(up + v * VS + p * G, o);
        }
        __syncthreads();
        // 3. k-steps: A from the up-sampled tile, B fragments from L2
        const int nIt = KMODE == 0 ? 27 : nKC;
        const T* arow = up + ((wave * UC_UY + (r >> 3)) * UC_UX + (r & 7)) * VS;      // row r of m-tile 0 at tap (0, 0, 0)
        for (int it = 0; it < nIt; ++it) {
            int kc, t, cl;
            if (KMODE == 0) {
                kc = it * nCC + cc; t = it; cl = G * kg;
            } else {
                kc = it;
                const int k = it * KC + G * kg;
                t = k / Cin; cl = k - t * Cin;
            }
            Vec16<T> bq[UC_NTB];
            const T* wf = Wf + (((long long)kc * NT + nt0) * 64 + lane) * G;
#pragma unroll
            for (int j = 0; j < UC_NTB; ++j)
                if (nt0 + j < NT) bq[j] = ld16(wf + (long long)j * 64 * G);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                Vec16<T> a;
                a.v = decltype(a.v){};
                if (t < 27) {      // (the flat-K loop's last k-step runs past the 27 taps: zero operand, zero-padded weights)
                    const int dz = t / 9, dy = (t / 3) % 3, dx = t % 3;
                    a = ld16(arow + ((dz * UC_UY + 2 * i + dy) * UC_UX + dx) * VS + cl);
                }
#pragma unroll
                for (int j = 0; j < UC_NTB; ++j)
                    if (nt0 + j < NT) umma(acc[i][j], a, bq[j]);
            }
        }
    }

    // epilogue: one n-tile at a time through LDS (D fragment: column = lane & 15, row = 4 * (lane >> 4) + ii), 16-byte stores
    constexpr int VN = Vec16<T>::N, OS = 16 + VN, PPR = 16 / VN;
    T* Ot = reinterpret_cast<T*>(lds_raw);
#pragma unroll
    for (int j = 0; j < UC_NTB; ++j) {
        if (nt0 + j >= NT) break;
        __syncthreads();
        const int n = (nt0 + j) * 16 + r;
        const float bv = bias ? bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) stf(Ot + (wave * 64 + i * 16 + kg * 4 + ii) * OS + r, acc[i][j][ii] + bv);
        __syncthreads();
        for (int e = tid; e < 256 * PPR; e += 256) {
            const int row = e / PPR, pc = e % PPR;                 // row = z * 64 + y * 8 + x of the tile
            const int gz = oz0 + (row >> 6), gy = oy0 + ((row >> 3) & 7), gx = ox0 + (row & 7);
            if (gz >= Do || gy >= Ho || gx >= Wo) continue;
            const long long off = ((((long long)b * Do + gz) * Ho + gy) * Wo + gx) * Cout + (nt0 + j) * 16 + pc * VN;
            st16(Y + off, ld16(Ot + row * OS + pc * VN));
        }
    }
}

template <typename T, int KMODE>
int launch_upconv(const void* x, const void* wf, const float* bias, void* y, int B, int Di, int Hi, int Wi, int Cin, int Cout,
                  dycon_stream_t stream) {
    constexpr int G = UFrag<T>::G, KC = UFrag<T>::KC;
    const int CS = KMODE == 0 ? KC : Cin, nCC = Cin / CS, nKC = (27 * Cin + KC - 1) / KC, NT = Cout / 16;
    const int VS = (CS + G - 1) / G * G + G;          // one spare 16-byte piece per voxel: LDS rows of an A fragment 16 B apart in banks
    size_t lds = (size_t)(UC_UV + UC_LV) * VS * sizeof(T);
    const size_t epi = (size_t)256 * (16 + Vec16<T>::N) * sizeof(T);
    if (lds < epi) lds = epi;
    DYCON_REQUIRE(lds <= UC_LDS_PER_CU, "upconv_k3: Cin = %d needs %zu bytes of LDS", Cin, lds);
    static size_t reserved = 0;      // per instantiation: the attribute is raised once (and again only for a larger request)
    if (lds > 48 * 1024 && lds > reserved) {
        if (hipFuncSetAttribute((const void*)upconv_k3_kernel<T, KMODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            dycon_set_error("upconv_k3: cannot reserve %zu bytes of LDS", lds);
            return DYCON_ERR_LAUNCH;
        }
        reserved = lds;
    }
    const int tilesZ = cdiv(2 * Di, UC_TZ), tilesY = cdiv(2 * Hi, UC_TY), tilesX = cdiv(2 * Wi, UC_TX);
    const long long nwg = (long long)B * tilesZ * tilesY * tilesX;
    DYCON_REQUIRE(nwg < (1ll << 31), "upconv_k3: %lld tiles exceed the grid", nwg);
    dim3 grid((unsigned)nwg, (unsigned)cdiv(NT, UC_NTB));
    upconv_k3_kernel<T, KMODE><<<grid, 256, lds, stream>>>((const T*)x, (const T*)wf, bias, (T*)y, Di, Hi, Wi, Cin, Cout, NT, CS, VS,
                                                          nCC, nKC, tilesZ, tilesY, tilesX);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

}  // namespace

extern "C" int dycon_upconv_k3(const void* x, const void* wfrag, const float* bias, void* y, int dtype, int B, int Di, int Hi, int Wi,
                               int Cin, int Cout, dycon_stream_t stream) {
    DYCON_REQUIRE(x && wfrag && y, "upconv_k3: null tensor");
    DYCON_REQUIRE(B > 0 && Di > 0 && Hi > 0 && Wi > 0, "upconv_k3: bad shape (%d, %d, %d, %d)", B, Di, Hi, Wi);
    DYCON_REQUIRE(8ll * Di * Hi * Wi < (1ll << 31), "upconv_k3: %d x %d x %d exceeds 2^31 output voxels per sample", Di, Hi, Wi);
    DYCON_REQUIRE(dtype == DYCON_F32 || dtype == DYCON_BF16, "upconv_k3: bad dtype %d", dtype);
    DYCON_REQUIRE(Cout >= 16 && Cout % 16 == 0 && (Cin == 16 || Cin == 48 || (Cin >= 32 && Cin % 32 == 0)),
                  "upconv_k3: unsupported channels %d -> %d (Cin 16, 48 or a multiple of 32, Cout a multiple of 16)", Cin, Cout);
    DYCON_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)wfrag) & 15) == 0, "upconv_k3: x, y and wfrag must be 16-byte aligned");
    const int KC = dtype == DYCON_BF16 ? 32 : 16;
    DYCON_DISPATCH(dtype, {
        if (Cin % KC == 0) return launch_upconv<T, 0>(x, wfrag, bias, y, B, Di, Hi, Wi, Cin, Cout, stream);
        return launch_upconv<T, 1>(x, wfrag, bias, y, B, Di, Hi, Wi, Cin, Cout, stream);
    });
    return DYCON_OK;
}
