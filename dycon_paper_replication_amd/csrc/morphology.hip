// Binary morphology of predicted masks on the device: scipy.ndimage's binary_erosion / binary_dilation (and so opening and closing),
// binary_fill_holes and a component size filter, bit for bit, without the copy of the mask to the host and back.
//
// A mask is bit-packed: one 64-bit word holds 64 consecutive voxels along z (the 64-wide segment of csrc/components.hip), bit b of
// word w of a row is the voxel z = 64 w + b, a volume (X, Y, Z) is (X, Y, W) words with W = ceil(Z / 64) <= 8.  The bits z >= Z of a
// row's last word are 0 on entry and 0 after every operation.
//
//   pack / unpack   one wave ballot per word; one thread per voxel
//   stencil         one thread per word and iteration, up to 4 iterations per launch on a tile of rows staged in LDS with a halo.  The
//                   z-neighbours of a word are its 1-bit shifts with the carry bit of the adjacent word of the row; the x / y
//                   neighbours are the same word of the neighbouring rows.  With F(r) = the word of row r with its two z-shifts
//                   folded in and C(r) = the word alone, a dilation is the OR (an erosion the AND) of
//                     connectivity 1   F(centre), C(4 face rows)
//                     connectivity 2   F(centre), F(4 face rows), C(4 edge rows)
//                     connectivity 3   F(all 9 rows)
//                   A row or a word outside the volume reads 0 for both operations (scipy's border_value = 0): an erosion eats a
//                   mask from the faces of the volume, a dilation gains nothing from outside.  An erosion result is a subset of the
//                   centre word, so its unused bits stay 0; a dilation masks them.
//   fill_holes      the complement is unpacked and labelled by dycon_cc_roots; every background voxel on a face marks its root
//                   (plain stores of the value 1: whichever thread comes last writes the same byte); a last pass ballots
//                   mask | (background whose root is unmarked) back into words
//   keep_min_size   sizes[root - 1] by the wave-aggregated integer adds of csrc/lesions.hip (root_counts.h), then the mask
//
// Integers only; no kernel waits on another workgroup; every call issues a fixed number of launches and reads nothing back.
#include "common.h"
#include "root_counts.h"

#define MORPH_MAX_AXIS 512                        // the limits of dycon_cc_roots
typedef unsigned long long morph_word;

template <typename T> __device__ __forceinline__ bool morph_fg(T v, bool by_value, long long value) {
    return by_value ? (long long)v == value : v != 0;
}

// One wave per word: lane b takes the voxel z = 64 w + b of its row.
template <typename T>
__global__ __launch_bounds__(256) void morph_pack_kernel(const T* __restrict__ vol, long long n_words, int Z, int W, bool by_value,
                                                         long long value, morph_word* __restrict__ packed) {
    const int lane = threadIdx.x & 63;
    const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (word >= n_words) return;                             // the whole wave
    const long long row = word / W;
    const int z = (int)(word % W) * 64 + lane;
    const bool fg = z < Z && morph_fg(vol[row * Z + z], by_value, value);
    const morph_word bits = __ballot(fg);
    if (lane == 0) packed[word] = bits;
}

// out = the voxel's bit, or its complement with INVERT (the background of fill_holes)
template <bool INVERT>
__global__ __launch_bounds__(256) void morph_unpack_kernel(const morph_word* __restrict__ packed, long long n_voxels, int Z, int W,
                                                           unsigned char* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_voxels) return;
    const long long row = i / Z;
    const int z = (int)(i % Z);
    const unsigned bit = (unsigned)(packed[row * W + (z >> 6)] >> (z & 63)) & 1u;
    out[i] = (unsigned char)(INVERT ? bit ^ 1u : bit);
}

// the word w of a row with its neighbours at z - 1 and z + 1 folded in; a voxel outside the row is 0
template <bool ERODE> __device__ __forceinline__ morph_word morph_fold_z(const morph_word* __restrict__ row, int w, int W) {
    const morph_word c = row[w];
    const morph_word below = c << 1 | (w > 0 ? row[w - 1] >> 63 : 0ull);               // bit b = the voxel at z - 1
    const morph_word above = c >> 1 | (w + 1 < W ? row[w + 1] << 63 : 0ull);           // bit b = the voxel at z + 1
    return ERODE ? c & below & above : c | below | above;
}

// A workgroup stages a tile of MORPH_TILE x MORPH_TILE rows with an h-deep halo of rows in LDS, whole z-rows (W <= 8 words), and runs
// h <= MORPH_HMAX iterations there, ping-pong between two LDS images: after iteration k the rows at least k from the edge of the
// staged tile are exact, so after h iterations the tile itself is.  Rows outside the volume are held at 0 through every iteration,
// the unused bits of a row's last word are masked after every dilation.  Measured against one launch per iteration on global memory
// (profiles/morphology_stencil_ab.txt): the same time at 1 iteration, 0.4x at 3 and 7 with 6 neighbours, 0.5 .. 0.6x with 26.
#define MORPH_TILE 8
#define MORPH_HMAX 4
#define MORPH_EXT (MORPH_TILE + 2 * MORPH_HMAX)
template <int CONN, bool ERODE>
__global__ __launch_bounds__(256) void morph_stencil_kernel(const morph_word* __restrict__ in, morph_word* __restrict__ out, int X,
                                                            int Y, int W, int tiles_y, int h, morph_word tail) {
    __shared__ morph_word buf[2][MORPH_EXT * MORPH_EXT * 8];
    const int E = MORPH_TILE + 2 * h;
    const int x0 = (int)(blockIdx.x / tiles_y) * MORPH_TILE - h, y0 = (int)(blockIdx.x % tiles_y) * MORPH_TILE - h;
    const long long vol = (long long)blockIdx.y * X * Y * W;
    const int n = E * E * W;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int w = i % W, r = i / W, x = x0 + r / E, y = y0 + r % E;
        buf[0][i] = (x >= 0 && x < X && y >= 0 && y < Y) ? in[vol + ((long long)x * Y + y) * W + w] : 0ull;
    }
    __syncthreads();
    int cur = 0;
    for (int k = 1; k <= h; ++k) {
        for (int i = threadIdx.x; i < n; i += 256) {
            const int w = i % W, r = i / W, tx = r / E, ty = r % E;
            if (tx < k || tx >= E - k || ty < k || ty >= E - k) continue;
            const int x = x0 + tx, y = y0 + ty;
            morph_word acc = 0;
            if (x >= 0 && x < X && y >= 0 && y < Y) {
                const morph_word* centre = buf[cur] + r * W;
                acc = morph_fold_z<ERODE>(centre, w, W);
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy) {
                        const int d = (dx != 0) + (dy != 0);
                        if (d == 0 || d > CONN) continue;
                        const morph_word* row = centre + (dx * E + dy) * W;     // inside the staged tile: 1 <= tx, ty <= E - 2
                        const morph_word v = d + 1 <= CONN ? morph_fold_z<ERODE>(row, w, W) : row[w];
                        acc = ERODE ? acc & v : acc | v;
                    }
                }
                if (!ERODE && w == W - 1) acc &= tail;
            }
            buf[cur ^ 1][i] = acc;
        }
        __syncthreads();
        cur ^= 1;
    }
    for (int i = threadIdx.x; i < MORPH_TILE * MORPH_TILE * W; i += 256) {
        const int w = i % W, r = i / W, tx = r / MORPH_TILE + h, ty = r % MORPH_TILE + h, x = x0 + tx, y = y0 + ty;
        if (x < X && y < Y) out[vol + ((long long)x * Y + y) * W + w] = buf[cur][(tx * E + ty) * W + w];
    }
}

// flag[root - 1] = 1 for every background component with a voxel on a face of its volume
__global__ __launch_bounds__(256) void morph_mark_kernel(const int* __restrict__ root, int X, int Y, int Z,
                                                         unsigned char* __restrict__ flag) {
    const long long V = (long long)X * Y * Z;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const int z = (int)(i % Z), y = (int)(i / Z % Y), x = (int)(i / Z / Y);
    if (x != 0 && x != X - 1 && y != 0 && y != Y - 1 && z != 0 && z != Z - 1) return;
    const int q = root[(long long)blockIdx.y * V + i];
    if (q >= 1 && q <= V) flag[(long long)blockIdx.y * V + q - 1] = 1;
}

// One wave per word: a voxel of the mask has root 0 in the labelling of the complement; a background voxel is filled when its
// component is unmarked.
__global__ __launch_bounds__(256) void morph_fill_kernel(const int* __restrict__ root, const unsigned char* __restrict__ flag,
                                                         long long n_words, int XY, int Z, int W, morph_word* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (word >= n_words) return;                             // the whole wave
    const long long row = word / W, V = (long long)XY * Z;
    const long long vol0 = row / XY * V;
    const int z = (int)(word % W) * 64 + lane;
    bool set = false;
    if (z < Z) {
        const int q = root[row * Z + z];
        set = q < 1 || q > V || flag[vol0 + q - 1] == 0;
    }
    const morph_word bits = __ballot(set);
    if (lane == 0) out[word] = bits;
}

__global__ __launch_bounds__(256) void morph_sizes_kernel(const int* __restrict__ root, long long V, int* __restrict__ sizes) {
    const int* __restrict__ r = root + (long long)blockIdx.y * V;
    int* __restrict__ s = sizes + (long long)blockIdx.y * V;
    const int lane = threadIdx.x & 63;
    int held = 0, n = 0;
    const long long span = (long long)gridDim.x * 256;
    for (long long base = (long long)blockIdx.x * 256; base < V; base += span)         // workgroup-uniform trip count
        les_wave_add(s, les_root(r, base + threadIdx.x, V), lane, held, n);
    les_flush(s, lane, held, n);
}

__global__ __launch_bounds__(256) void morph_keep_kernel(const int* __restrict__ root, const int* __restrict__ sizes, long long V,
                                                         int min_voxels, unsigned char* __restrict__ out) {
    const long long off = (long long)blockIdx.y * V;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        const int q = les_root(root + off, i, V);
        out[off + i] = (unsigned char)(q != 0 && sizes[off + q - 1] >= min_voxels);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void morph_merge_class_kernel(const T* __restrict__ label_map, const unsigned char* __restrict__ mask,
                                                                int cls, long long n, unsigned char* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !mask[i]) return;
    const unsigned char have = out[i];
    if (have == 0 || (long long)label_map[i] != (long long)have) out[i] = (unsigned char)cls;
}

// ------------------------------------------------------------------ host side
static size_t morph_align(size_t n) { return (n + 255) & ~(size_t)255; }
static int morph_grid(long long V) {                                               // grid-stride passes: 8 voxels per thread, 2048 workgroups at most
    const long long blocks = (V + 256 * 8 - 1) / (256 * 8);
    return (int)(blocks > 2048 ? 2048 : blocks);
}
static bool morph_shape_ok(int n_vol, int X, int Y, int Z) {
    return n_vol >= 1 && n_vol <= 65535 && X >= 1 && X <= MORPH_MAX_AXIS && Y >= 1 && Y <= MORPH_MAX_AXIS && Z >= 1 &&
           Z <= MORPH_MAX_AXIS && (long long)n_vol * X * Y * Z <= 2147483647ll;
}
#define MORPH_REQUIRE_SHAPE(what)                                                                                                  \
    DYCON_REQUIRE(morph_shape_ok(n_vol, X, Y, Z), what ": %d volumes of %dx%dx%d (every axis 1..%d, at most 65535 volumes and 2^31 - " \
                  "1 voxels in one call)", n_vol, X, Y, Z, MORPH_MAX_AXIS)

// the unpacked complement, reused as the marks once it is labelled (one byte per voxel) | its roots (one int32 per voxel)
extern "C" size_t dycon_morph_fill_workspace(int n_vol, int X, int Y, int Z) {
    if (!morph_shape_ok(n_vol, X, Y, Z)) return 0;
    const size_t nv = (size_t)n_vol * X * Y * Z;
    return morph_align(nv) + morph_align(nv * sizeof(int));
}

extern "C" size_t dycon_cc_min_size_workspace(int n_vol, int X, int Y, int Z) {
    if (!morph_shape_ok(n_vol, X, Y, Z)) return 0;
    return morph_align((size_t)n_vol * X * Y * Z * sizeof(int));
}

extern "C" int dycon_morph_pack(const void* vol, int vol_bytes, int n_vol, int X, int Y, int Z, int by_value, long long value,
                                uint64_t* packed, dycon_stream_t stream) {
    DYCON_REQUIRE(vol && packed, "morph_pack: null pointer");
    DYCON_REQUIRE(vol_bytes == 1 || vol_bytes == 8, "morph_pack: the volume must be uint8 or int64 (vol_bytes = %d)", vol_bytes);
    MORPH_REQUIRE_SHAPE("morph_pack");
    hipStream_t st = (hipStream_t)stream;
    const int W = cdiv(Z, 64);
    const long long n_words = (long long)n_vol * X * Y * W;
    const int grid = cdiv(n_words, 4);
    if (vol_bytes == 1)
        morph_pack_kernel<<<grid, 256, 0, st>>>((const unsigned char*)vol, n_words, Z, W, by_value != 0, value, (morph_word*)packed);
    else
        morph_pack_kernel<<<grid, 256, 0, st>>>((const long long*)vol, n_words, Z, W, by_value != 0, value, (morph_word*)packed);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_morph_unpack(const uint64_t* packed, int n_vol, int X, int Y, int Z, uint8_t* out, dycon_stream_t stream) {
    DYCON_REQUIRE(packed && out, "morph_unpack: null pointer");
    MORPH_REQUIRE_SHAPE("morph_unpack");
    const long long nv = (long long)n_vol * X * Y * Z;
    morph_unpack_kernel<false><<<cdiv(nv, 256), 256, 0, (hipStream_t)stream>>>((const morph_word*)packed, nv, Z, cdiv(Z, 64), out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

template <int CONN>
static void morph_stencil_launch(const morph_word* in, morph_word* out, int n_vol, int X, int Y, int W, int h, morph_word tail, int op,
                                 hipStream_t st) {
    const int tiles_y = cdiv(Y, MORPH_TILE);
    dim3 grid(cdiv(X, MORPH_TILE) * tiles_y, n_vol);
    if (op == DYCON_MORPH_ERODE) morph_stencil_kernel<CONN, true><<<grid, 256, 0, st>>>(in, out, X, Y, W, tiles_y, h, tail);
    else morph_stencil_kernel<CONN, false><<<grid, 256, 0, st>>>(in, out, X, Y, W, tiles_y, h, tail);
}

extern "C" int dycon_morph_stencil(const uint64_t* in, uint64_t* out, uint64_t* scratch, int n_vol, int X, int Y, int Z,
                                   int connectivity, int op, int iterations, dycon_stream_t stream) {
    DYCON_REQUIRE(in && out, "morph_stencil: null pointer");
    MORPH_REQUIRE_SHAPE("morph_stencil");
    DYCON_REQUIRE(connectivity >= 1 && connectivity <= 3, "morph_stencil: connectivity %d (1, 2 or 3)", connectivity);
    DYCON_REQUIRE(op == DYCON_MORPH_ERODE || op == DYCON_MORPH_DILATE, "morph_stencil: op %d (%d = erosion, %d = dilation)", op,
                  DYCON_MORPH_ERODE, DYCON_MORPH_DILATE);
    DYCON_REQUIRE(iterations >= 1 && iterations <= 64, "morph_stencil: iterations = %d (1..64)", iterations);
    DYCON_REQUIRE(iterations == 1 || scratch, "morph_stencil: %d iterations need a scratch buffer", iterations);
    const int W = cdiv(Z, 64);
    {
        const char *a = (const char*)in, *b = (const char*)out, *c = (const char*)scratch;
        const long long bytes = (long long)n_vol * X * Y * W * 8;
        const bool apart = (a + bytes <= b || b + bytes <= a) &&
                           (!c || ((a + bytes <= c || c + bytes <= a) && (b + bytes <= c || c + bytes <= b)));
        DYCON_REQUIRE(apart, "morph_stencil: in, out and scratch must not overlap");
    }
    hipStream_t st = (hipStream_t)stream;
    const morph_word tail = Z % 64 ? (1ull << (Z % 64)) - 1 : ~0ull;
    const int launches = cdiv(iterations, MORPH_HMAX);
    const morph_word* src = (const morph_word*)in;
    int left = iterations;
    for (int k = 0; k < launches; ++k) {                     // the last launch writes `out`, the ones before alternate
        morph_word* dst = (launches - 1 - k) % 2 == 0 ? (morph_word*)out : (morph_word*)scratch;
        const int h = left < MORPH_HMAX ? left : MORPH_HMAX;
        if (connectivity == 1) morph_stencil_launch<1>(src, dst, n_vol, X, Y, W, h, tail, op, st);
        else if (connectivity == 2) morph_stencil_launch<2>(src, dst, n_vol, X, Y, W, h, tail, op, st);
        else morph_stencil_launch<3>(src, dst, n_vol, X, Y, W, h, tail, op, st);
        src = dst;
        left -= h;
    }
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_morph_fill_holes(const uint64_t* mask, int n_vol, int X, int Y, int Z, int connectivity, uint64_t* out,
                                      void* workspace, size_t ws_bytes, dycon_stream_t stream) {
    DYCON_REQUIRE(mask && out && workspace, "morph_fill_holes: null pointer");
    MORPH_REQUIRE_SHAPE("morph_fill_holes");
    DYCON_REQUIRE(connectivity >= 1 && connectivity <= 3, "morph_fill_holes: connectivity %d (1, 2 or 3)", connectivity);
    const size_t need = dycon_morph_fill_workspace(n_vol, X, Y, Z);
    DYCON_REQUIRE(ws_bytes >= need, "morph_fill_holes: workspace of %zu bytes, %zu needed", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const long long V = (long long)X * Y * Z, nv = (long long)n_vol * V;
    const int W = cdiv(Z, 64);
    const long long n_words = (long long)n_vol * X * Y * W;
    unsigned char* comp = (unsigned char*)workspace;         // the complement, then the marks
    int* root = (int*)((char*)workspace + morph_align((size_t)nv));
    morph_unpack_kernel<true><<<cdiv(nv, 256), 256, 0, st>>>((const morph_word*)mask, nv, Z, W, comp);
    const int rc = dycon_cc_roots(comp, 1, n_vol, X, Y, Z, connectivity, 0, root, stream);
    if (rc != DYCON_OK) return rc;
    if (hipMemsetAsync(comp, 0, (size_t)nv, st) != hipSuccess) {
        dycon_set_error("morph_fill_holes: hipMemsetAsync failed");
        return DYCON_ERR_LAUNCH;
    }
    morph_mark_kernel<<<dim3(cdiv(V, 256), n_vol), 256, 0, st>>>(root, X, Y, Z, comp);
    morph_fill_kernel<<<cdiv(n_words, 4), 256, 0, st>>>(root, comp, n_words, X * Y, Z, W, (morph_word*)out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_cc_keep_min_size(const int* root, int n_vol, int X, int Y, int Z, int min_voxels, uint8_t* out, void* workspace,
                                      size_t ws_bytes, dycon_stream_t stream) {
    DYCON_REQUIRE(root && out && workspace, "cc_keep_min_size: null pointer");
    MORPH_REQUIRE_SHAPE("cc_keep_min_size");
    DYCON_REQUIRE(min_voxels >= 1, "cc_keep_min_size: min_voxels = %d (at least 1)", min_voxels);
    const size_t need = dycon_cc_min_size_workspace(n_vol, X, Y, Z);
    DYCON_REQUIRE(ws_bytes >= need, "cc_keep_min_size: workspace of %zu bytes, %zu needed", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const long long V = (long long)X * Y * Z;
    if (hipMemsetAsync(workspace, 0, need, st) != hipSuccess) {
        dycon_set_error("cc_keep_min_size: hipMemsetAsync failed");
        return DYCON_ERR_LAUNCH;
    }
    dim3 grid(morph_grid(V), n_vol);
    morph_sizes_kernel<<<grid, 256, 0, st>>>(root, V, (int*)workspace);
    morph_keep_kernel<<<grid, 256, 0, st>>>(root, (const int*)workspace, V, min_voxels, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_morph_merge_class(const void* label_map, int vol_bytes, const uint8_t* mask, int cls, long long n, uint8_t* out,
                                       dycon_stream_t stream) {
    DYCON_REQUIRE(label_map && mask && out, "morph_merge_class: null pointer");
    DYCON_REQUIRE(vol_bytes == 1 || vol_bytes == 8, "morph_merge_class: the label map must be uint8 or int64 (vol_bytes = %d)", vol_bytes);
    DYCON_REQUIRE(cls >= 1 && cls <= 255, "morph_merge_class: cls = %d (1..255)", cls);
    DYCON_REQUIRE(n >= 1 && n <= 2147483647ll, "morph_merge_class: n = %lld (1..2^31 - 1)", n);
    hipStream_t st = (hipStream_t)stream;
    if (vol_bytes == 1) morph_merge_class_kernel<<<cdiv(n, 256), 256, 0, st>>>((const unsigned char*)label_map, mask, cls, n, out);
    else morph_merge_class_kernel<<<cdiv(n, 256), 256, 0, st>>>((const long long*)label_map, mask, cls, n, out);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}
