// 3-D connected components on the device: the root of every voxel's component, scipy.ndimage.label's consecutive labels, the
// component sizes and the largest component per volume (or per value).  This is the `nms` step of the reference's test scripts
// (code/utils/test_3d_patch.py:19-26, getLargestCC) without the host round trip.
//
// Everything is an integer and defined independently of scheduling: the root of a component is 1 + the smallest linear index
// (x*Y + y)*Z + z among its voxels, labels are the ranks of the roots in raster order, sizes are integer counts, and the largest
// component is the maximum of the 64-bit key (size << 32) | (0xFFFFFFFF - root), so equal sizes go to the smallest root.
//
//   tile      a workgroup labels a tile of 4 x 4 rows by 64 z in LDS: runs along z by ballots, then union-find over the rows of
//             the tile; parent = the global id of the tile-local root
//   merge     unites across tile faces (half of the neighbourhood: the rows before, and the segment before along z): union-find,
//             every write a device-scope atomicMin
//   flatten   its own launch: every parent replaced by its root
//   labels    roots counted per chunk, one workgroup per volume scans the chunk counts, a fix-up pass ranks the roots, a last
//             pass copies each root's label to its voxels.  No workgroup waits on another.
//   largest   sizes by integer atomics aggregated per wave and per workgroup, a 64-bit atomicMax per root in LDS and per workgroup
//             in global memory, then the mask
//
// Ids are 1-based inside one volume (id = linear index + 1, 0 = background): they are the values of `root`, and a volume has at
// most 2^27 voxels.  No kernel here has a grid-wide barrier or reads a flag written by another workgroup; a call issues a fixed
// number of launches and reads nothing back.
#include "common.h"

#define CC_MAX_AXIS 512
#define CC_CHUNK 2048                             // voxels per workgroup of the label passes (256 threads x 8)
#define CC_MAX_CLS 255

// class of a voxel: 0 = background.  Binary: non-zero is class 1.  By value: the value itself when it lies in 1..255.
template <typename T, bool BINARY> __device__ __forceinline__ int cc_cls(T v) {
    if constexpr (BINARY) return v != 0;
    else return (v >= 1 && v <= CC_MAX_CLS) ? (int)v : 0;
}

// ------------------------------------------------------------------ union-find
// Invariants.  P1[v] <= v always, P1[v] only ever decreases, and every value P1[v] ever held is a voxel of v's final component.
// Every write in the merge kernel is a device-scope atomicMin, which acts on the one true copy of the word and returns its true
// previous value.
//
// Freshness.  The per-XCD L2s and per-CU L1s are not coherent inside a kernel, so a load may return an older parent.  Nothing here
// needs it to be fresh: an older parent is still a smaller-or-equal voxel of the same component, so cc_find over old values walks
// down a strictly decreasing chain and stops at a voxel that once was a root.  Whether it still is one is decided by the atomicMin
// in cc_unite alone: its return value is the true parent, and the loop goes on from that value.  The loads are relaxed agent-scope
// atomic loads so that they are neither register-cached nor served from a CU's L1.  The tile kernel's plain stores are visible
// because a kernel boundary lies between; the flatten pass runs in a launch of its own for the same reason.  (In the tile kernel
// the parents live in LDS, which the workgroup's waves share coherently; the same routine runs there at workgroup scope.)
//
// cc_find: the id strictly decreases every trip (a parent is smaller than a voxel that is no root), so the loop ends.
template <int SCOPE> __device__ __forceinline__ int cc_find(int* P1, int i) {
    for (;;) {
        const int p = __hip_atomic_load(P1 + i, __ATOMIC_RELAXED, SCOPE);
        if (p == i) return i;
        i = p;
    }
}

// Unite the components of a and b.  The larger root is linked to the smaller by atomicMin.  If the value it returns is a itself, a
// was a root and is linked now.  Otherwise a had a parent `old` already (old < a): when b < old the atomicMin has replaced the
// link a -> old by a -> b, when b > old it has changed nothing; either way old and b remain to be united, and the loop goes on
// with them.  max(a, b) strictly decreases every trip (old < a, b < a, and cc_find only lowers), so the loop ends; no link is ever
// lost for good, and a root is always the smallest voxel of its tree, so the final root of a component is its minimum whatever
// the order of execution.  SCOPE is the agent for parents in global memory and the workgroup for a tile's parents in LDS.
template <int SCOPE> __device__ __forceinline__ void cc_unite(int* P1, int a, int b) {
    a = cc_find<SCOPE>(P1, a);
    b = cc_find<SCOPE>(P1, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(P1 + a, b);
        if (old == a || old == b) return;
        a = cc_find<SCOPE>(P1, old);
        b = cc_find<SCOPE>(P1, b);
    }
}

// The rows before row (x, y) that hold neighbours of its voxels, with whether the neighbours at z - 1 and z + 1 of such a row
// count as well: connectivity 1 = faces (6 neighbours), 2 = faces and edges (18), 3 = all 26.
template <int CONN> struct CCRows {
    static constexpr int N = CONN == 1 ? 2 : 4;
    static __device__ __forceinline__ constexpr int dx(int k) { return k == 1 ? 0 : -1; }
    static __device__ __forceinline__ constexpr int dy(int k) { return k == 0 ? 0 : k == 3 ? 1 : -1; }
    static __device__ __forceinline__ constexpr bool diagz(int k) { return CONN == 3 || (CONN == 2 && k < 2); }
};

// Of all pairs of neighbours between a voxel v of a run and a row before it only these are needed, n being the voxel of that row at
// v's z; the others follow from them along z, since the voxels of one run of a row are united among themselves:
//   (v, n) at equal z                       unless (v - 1, n - 1) is such a pair too
//   (v, n - 1), (v, n + 1) when n differs   unless v - 1 (resp. v + 1) continues v's run: that voxel has the pair at equal z
//
// Tile-local pass: a workgroup labels a tile of CC_TX x CC_TY rows by 64 z in LDS (wave w takes the rows of x = w) and writes every
// voxel's parent as the global id of its tile-local root.  Local ids (row * 64 + z) grow with the global index, so the local root
// is the smallest voxel of the local component and parent <= voxel holds.  The pairs with both voxels in one tile are united
// here; cc_merge_kernel takes the others.
#define CC_TX 4
#define CC_TY 4
template <typename T, bool BINARY, int CONN>
__global__ __launch_bounds__(256) void cc_tile_kernel(const T* __restrict__ vol, int X, int Y, int Z, int tiles_y, int* __restrict__ root) {
    using R = CCRows<CONN>;
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    __shared__ int lab[CC_TX * CC_TY * 64];
    __shared__ unsigned char cl[CC_TX * CC_TY][64];
    const int lane = threadIdx.x & 63, tx = threadIdx.x >> 6;
    const long long V = (long long)X * Y * Z;
    const T* __restrict__ p = vol + (long long)blockIdx.z * V;
    int* __restrict__ out = root + (long long)blockIdx.z * V;
    const int x0 = (blockIdx.y / tiles_y) * CC_TX, y0 = (blockIdx.y % tiles_y) * CC_TY, z = blockIdx.x * 64 + lane;
    const int x = x0 + tx;
#pragma unroll
    for (int ty = 0; ty < CC_TY; ++ty) {
        const int row = tx * CC_TY + ty, y = y0 + ty;
        const int a = (x < X && y < Y && z < Z) ? cc_cls<T, BINARY>(p[((long long)x * Y + y) * Z + z]) : 0;
        const int prev = __shfl_up(a, 1, 64);
        const unsigned long long starts = __ballot(lane == 0 || a != prev);       // bit 0 is always set
        cl[row][lane] = (unsigned char)a;
        lab[row * 64 + lane] = row * 64 + 63 - __clzll((long long)(starts & (~0ull >> (63 - lane))));
    }
    __syncthreads();
#pragma unroll
    for (int ty = 0; ty < CC_TY; ++ty) {
        const int row = tx * CC_TY + ty;
        const int a = cl[row][lane];
        if (!a) continue;
        const int id = row * 64 + lane;
        const bool pv = lane > 0 && cl[row][lane - 1] == a, nv = lane < 63 && cl[row][lane + 1] == a;
#pragma unroll
        for (int k = 0; k < R::N; ++k) {
            const int nx = tx + R::dx(k), ny = ty + R::dy(k);
            if (nx < 0 || ny < 0 || ny >= CC_TY) continue;   // a row of another tile: cc_merge_kernel
            const int nrow = nx * CC_TY + ny;
            const bool below = lane > 0 && cl[nrow][lane - 1] == a;
            if (cl[nrow][lane] == a) {
                if (!(pv && below)) cc_unite<WG>(lab, id, nrow * 64 + lane);
            } else if (R::diagz(k)) {
                if (below && !pv) cc_unite<WG>(lab, id, nrow * 64 + lane - 1);
                if (!nv && lane < 63 && cl[nrow][lane + 1] == a) cc_unite<WG>(lab, id, nrow * 64 + lane + 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int ty = 0; ty < CC_TY; ++ty) {
        const int row = tx * CC_TY + ty, y = y0 + ty;
        if (x >= X || y >= Y || z >= Z) continue;
        int r = 0;
        if (cl[row][lane]) {
            r = lab[row * 64 + lane];
            for (int q = lab[r]; q != r; q = lab[r]) r = q; // the local id strictly decreases
            const int rrow = r >> 6;
            r = ((x0 + rrow / CC_TY) * Y + y0 + rrow % CC_TY) * Z + blockIdx.x * 64 + (r & 63) + 1;
        }
        out[((long long)x * Y + y) * Z + z] = r;
    }
}

// One wave per row, lanes along z: the pairs of the list above whose voxels lie in different tiles, and at lane 0 the run that goes
// on from the 64-wide segment before.
template <typename T, bool BINARY, int CONN>
__global__ __launch_bounds__(256) void cc_merge_kernel(const T* __restrict__ vol, int X, int Y, int Z, int* __restrict__ root) {
    using R = CCRows<CONN>;
    constexpr int AGENT = __HIP_MEMORY_SCOPE_AGENT;
    const int lane = threadIdx.x & 63;
    const long long V = (long long)X * Y * Z;
    const T* __restrict__ p = vol + (long long)blockIdx.y * V;
    int* P1 = root + (long long)blockIdx.y * V - 1;          // addressed by 1-based id only
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= X * Y) return;                                // the whole wave
    const int x = row / Y, y = row % Y;
    const int r0 = row * Z;
    for (int z0 = 0; z0 < Z; z0 += 64) {
        const int z = z0 + lane;
        if (z >= Z) continue;
        const int a = cc_cls<T, BINARY>(p[r0 + z]);
        if (!a) continue;
        const int id = r0 + z + 1;
        const bool pv = z > 0 && cc_cls<T, BINARY>(p[r0 + z - 1]) == a;
        const bool nv = z + 1 < Z && cc_cls<T, BINARY>(p[r0 + z + 1]) == a;
        if (lane == 0 && pv) cc_unite<AGENT>(P1, id, id - 1);       // the run goes on from the segment before
#pragma unroll
        for (int k = 0; k < R::N; ++k) {
            const int xx = x + R::dx(k), yy = y + R::dy(k);
            if (xx < 0 || yy < 0 || yy >= Y) continue;       // wave-uniform; xx < X always (dx <= 0)
            // the row lies in v's tile: only n - 1 at lane 0 and n + 1 at lane 63 belong to other tiles
            const bool same_tile = x % CC_TX + R::dx(k) >= 0 && y % CC_TY + R::dy(k) >= 0 && y % CC_TY + R::dy(k) < CC_TY;
            const int rn = (xx * Y + yy) * Z;
            const bool below = z > 0 && cc_cls<T, BINARY>(p[rn + z - 1]) == a;
            if (cc_cls<T, BINARY>(p[rn + z]) == a) {
                if (!same_tile && !(pv && below)) cc_unite<AGENT>(P1, id, rn + z + 1);
            } else if (R::diagz(k)) {
                if (below && !pv && (!same_tile || lane == 0)) cc_unite<AGENT>(P1, id, rn + z);
                if (!nv && z + 1 < Z && (!same_tile || lane == 63) && cc_cls<T, BINARY>(p[rn + z + 1]) == a)
                    cc_unite<AGENT>(P1, id, rn + z + 2);
            }
        }
    }
}

// Every parent replaced by its root, in place with plain loads and stores: a value read is the parent the merge pass left or a
// root another thread has written over it, both on the chain to the same root, and a root is never rewritten.  The id strictly
// decreases along the chain, so the loop ends.
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* __restrict__ root, long long V) {
    int* P1 = root + (long long)blockIdx.y * V - 1;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x + 1; i <= V; i += (long long)gridDim.x * 256) {
        int r = P1[i];
        if (r == 0 || r == (int)i) continue;
        for (int q = P1[r]; q != r; q = P1[r]) r = q;
        P1[i] = r;
    }
}

// ------------------------------------------------------------------ labels: rank of every root in raster order
// number of roots among the 256 x 8 voxels of a chunk below this thread's: thread t owns the 8 consecutive voxels from
// chunk * CC_CHUNK + 8 t.  Returns the exclusive prefix inside the workgroup; *total = roots of the whole chunk.
__device__ __forceinline__ int cc_chunk_prefix(int mine, int* wsum /* 4 ints of LDS */, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int s = wsum[k];
        if (k < w) before += s;
        all += s;
    }
    *total = all;
    return before + incl - mine;
}

__device__ __forceinline__ unsigned cc_root_flags(const int* __restrict__ r, long long V, long long first) {
    unsigned f = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const long long i = first + j;
        if (i < V && r[i] == (int)(i + 1)) f |= 1u << j;
    }
    return f;
}

__global__ __launch_bounds__(256) void cc_count_roots_kernel(const int* __restrict__ root, long long V, int nchunk,
                                                             int* __restrict__ chunk_count) {
    __shared__ int wsum[4];
    const int* __restrict__ r = root + (long long)blockIdx.y * V;
    const unsigned f = cc_root_flags(r, V, (long long)blockIdx.x * CC_CHUNK + 8 * threadIdx.x);
    int total;
    cc_chunk_prefix(__popc(f), wsum, &total);
    if (threadIdx.x == 0) chunk_count[(long long)blockIdx.y * nchunk + blockIdx.x] = total;
}

// One workgroup per volume: the chunk counts become their exclusive prefix sums, 256 at a time with a running carry.
__global__ __launch_bounds__(256) void cc_scan_chunks_kernel(int* __restrict__ chunk_count, int nchunk, int* __restrict__ ncomp) {
    __shared__ int wsum[4];
    int* __restrict__ c = chunk_count + (long long)blockIdx.x * nchunk;
    int carry = 0;
    for (int base = 0; base < nchunk; base += 256) {
        const int i = base + threadIdx.x;
        const int mine = i < nchunk ? c[i] : 0;
        int total;
        const int before = cc_chunk_prefix(mine, wsum, &total);
        if (i < nchunk) c[i] = carry + before;
        carry += total;
        __syncthreads();                                     // wsum is rewritten next trip
    }
    if (threadIdx.x == 0) ncomp[blockIdx.x] = carry;
}

// labels[root voxel] = 1 + the roots before it; every other voxel is written by cc_spread_labels_kernel
__global__ __launch_bounds__(256) void cc_rank_roots_kernel(const int* __restrict__ root, long long V, int nchunk,
                                                            const int* __restrict__ chunk_offset, int* __restrict__ labels) {
    __shared__ int wsum[4];
    const int* __restrict__ r = root + (long long)blockIdx.y * V;
    int* __restrict__ out = labels + (long long)blockIdx.y * V;
    const long long first = (long long)blockIdx.x * CC_CHUNK + 8 * threadIdx.x;
    const unsigned f = cc_root_flags(r, V, first);
    int total;
    int rank = chunk_offset[(long long)blockIdx.y * nchunk + blockIdx.x] + cc_chunk_prefix(__popc(f), wsum, &total);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (f >> j & 1) out[first + j] = ++rank;
}

__global__ __launch_bounds__(256) void cc_spread_labels_kernel(const int* __restrict__ root, long long V, int* __restrict__ labels) {
    const int* __restrict__ r = root + (long long)blockIdx.y * V;
    int* __restrict__ out = labels + (long long)blockIdx.y * V;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        const int q = r[i];
        if (q != (int)(i + 1)) out[i] = q ? out[q - 1] : 0;  // reads root voxels only, writes the others only
    }
}

// ------------------------------------------------------------------ sizes and the largest component
// sizes[root - 1] += voxels.  Lanes of a wave that share the root of the first pending lane add once: up to 4 such rounds (the
// pending set loses at least the leader every round), then whatever is left adds for itself.  An add goes to a table of the
// workgroup in LDS first (open addressing, at most 4 probes, then straight to global memory), so that a large component costs a
// workgroup one global atomic instead of one per wave and pass: adds to one address are serialised by the memory system.
// Unsigned integer adds only: the sums do not depend on where an add went.
#define CC_TABLE 256
__device__ __forceinline__ void cc_table_add(int* key, unsigned* cnt, unsigned* __restrict__ s, int q, unsigned n) {
    unsigned slot = ((unsigned)q * 2654435761u) >> 24;
#pragma unroll
    for (int probe = 0; probe < 4; ++probe) {
        const int old = atomicCAS(key + slot, 0, q);
        if (old == 0 || old == q) {
            atomicAdd(cnt + slot, n);
            return;
        }
        slot = (slot + 1) & (CC_TABLE - 1);
    }
    atomicAdd(s + q - 1, n);
}

__global__ __launch_bounds__(256) void cc_sizes_kernel(const int* __restrict__ root, long long V, unsigned* __restrict__ sizes) {
    __shared__ int key[CC_TABLE];
    __shared__ unsigned cnt[CC_TABLE];
    const int* __restrict__ r = root + (long long)blockIdx.y * V;
    unsigned* __restrict__ s = sizes + (long long)blockIdx.y * V;
    const int lane = threadIdx.x & 63;
    key[threadIdx.x] = 0;                                    // CC_TABLE == the workgroup size
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const long long span = (long long)gridDim.x * 256;
    for (long long base = (long long)blockIdx.x * 256; base < V; base += span) {       // workgroup-uniform trip count
        const long long i = base + threadIdx.x;
        const int q = i < V ? r[i] : 0;
        bool pending = q != 0;
        for (int round = 0; round < 4; ++round) {
            const unsigned long long todo = __ballot(pending);
            if (!todo) break;                                // wave-uniform
            const int leader = __ffsll(todo) - 1;
            const int lq = __shfl(q, leader, 64);
            const unsigned long long same = __ballot(pending && q == lq);
            if (lane == leader) cc_table_add(key, cnt, s, lq, (unsigned)__popcll(same));
            if (q == lq) pending = false;
        }
        if (pending) cc_table_add(key, cnt, s, q, 1u);
    }
    __syncthreads();
    const int k = key[threadIdx.x];
    if (k) atomicAdd(s + k - 1, cnt[threadIdx.x]);
}

// best[vol][class - 1] = max over the roots of the class of (size << 32) | (0xFFFFFFFF - root): the greatest size, the smallest
// root among equals.  Every root takes a 64-bit atomicMax on the workgroup's table in LDS; at the end the workgroup takes one global
// atomicMax per class it has seen, and none for a candidate that does not beat the `best` it loads first: best only grows, so an
// old value can only let more candidates through.  A maximum does not depend on the order of its operands.
template <typename T, bool BINARY>
__global__ __launch_bounds__(256) void cc_select_kernel(const T* __restrict__ vol, const int* __restrict__ root,
                                                        const unsigned* __restrict__ sizes, long long V, int n_cls,
                                                        unsigned long long* __restrict__ best) {
    __shared__ unsigned long long tab[256];
    const T* __restrict__ p = vol + (long long)blockIdx.y * V;
    const int* __restrict__ r = root + (long long)blockIdx.y * V;
    const unsigned* __restrict__ s = sizes + (long long)blockIdx.y * V;
    unsigned long long* b = best + (long long)blockIdx.y * n_cls;
    tab[threadIdx.x] = 0;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        if (r[i] != (int)(i + 1)) continue;
        const int c = cc_cls<T, BINARY>(p[i]);
        if (c <= n_cls) atomicMax(tab + c - 1, (unsigned long long)s[i] << 32 | (0xFFFFFFFFu - (unsigned)(i + 1)));
    }
    __syncthreads();
    const unsigned long long key = tab[threadIdx.x];         // n_cls <= 255 < the workgroup size
    if (key && key > __hip_atomic_load(b + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(b + threadIdx.x, key);
}

// out = the class (1 in binary mode) on the winner of the voxel's class, 0 elsewhere; workgroup 0 of a volume also unpacks the keys
template <typename T, bool BINARY>
__global__ __launch_bounds__(256) void cc_keep_kernel(const T* __restrict__ vol, const int* __restrict__ root,
                                                      const unsigned long long* __restrict__ best, long long V, int n_cls,
                                                      unsigned char* __restrict__ out, int* __restrict__ win_size,
                                                      int* __restrict__ win_root) {
    const T* __restrict__ p = vol + (long long)blockIdx.y * V;
    const int* __restrict__ r = root + (long long)blockIdx.y * V;
    const unsigned long long* __restrict__ b = best + (long long)blockIdx.y * n_cls;
    unsigned char* __restrict__ o = out + (long long)blockIdx.y * V;
    if (blockIdx.x == 0)
        for (int c = threadIdx.x; c < n_cls; c += 256) {
            const unsigned long long key = b[c];
            win_size[(long long)blockIdx.y * n_cls + c] = (int)(key >> 32);
            win_root[(long long)blockIdx.y * n_cls + c] = key ? (int)(0xFFFFFFFFu - (unsigned)key) : 0;
        }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        const int q = r[i];
        int keep = 0;
        if (q) {
            const int c = cc_cls<T, BINARY>(p[i]);
            if (c <= n_cls && (unsigned)q == 0xFFFFFFFFu - (unsigned)b[c - 1]) keep = c;
        }
        o[i] = (unsigned char)keep;
    }
}

// ------------------------------------------------------------------ host side
static int cc_nchunk(long long V) { return (int)((V + CC_CHUNK - 1) / CC_CHUNK); }
static size_t cc_align(size_t n) { return (n + 255) & ~(size_t)255; }
static int cc_stride_grid(long long V) {                                          // grid-stride passes: 8 voxels per thread, 2048 workgroups at most
    const long long blocks = (V + 256 * 8 - 1) / (256 * 8);
    return (int)(blocks > 2048 ? 2048 : blocks);
}

static bool cc_shape_ok(int n_vol, int X, int Y, int Z) {
    return n_vol >= 1 && n_vol <= 65535 && X >= 1 && X <= CC_MAX_AXIS && Y >= 1 && Y <= CC_MAX_AXIS && Z >= 1 && Z <= CC_MAX_AXIS &&
           (long long)n_vol * X * Y * Z <= 2147483647ll;
}
#define CC_REQUIRE_SHAPE(what)                                                                                                     \
    DYCON_REQUIRE(cc_shape_ok(n_vol, X, Y, Z), what ": %d volumes of %dx%dx%d (every axis 1..%d, at most 65535 volumes and 2^31 - 1 " \
                  "voxels in one call)", n_vol, X, Y, Z, CC_MAX_AXIS)

// sizes (one unsigned per voxel) | best (CC_MAX_CLS keys per volume) | chunk counts of the label scan
extern "C" size_t dycon_cc_workspace(int n_vol, int X, int Y, int Z) {
    if (!cc_shape_ok(n_vol, X, Y, Z)) return 0;
    const long long V = (long long)X * Y * Z;
    return cc_align((size_t)n_vol * V * sizeof(unsigned)) + cc_align((size_t)n_vol * CC_MAX_CLS * sizeof(unsigned long long)) +
           cc_align((size_t)n_vol * cc_nchunk(V) * sizeof(int));
}

template <typename T, bool BINARY, int CONN>
static void cc_roots_launch_conn(const T* vol, int n_vol, int X, int Y, int Z, int* root, hipStream_t st) {
    const long long V = (long long)X * Y * Z;
    const int tiles_y = cdiv(Y, CC_TY);
    cc_tile_kernel<T, BINARY, CONN><<<dim3(cdiv(Z, 64), cdiv(X, CC_TX) * tiles_y, n_vol), 256, 0, st>>>(vol, X, Y, Z, tiles_y, root);
    cc_merge_kernel<T, BINARY, CONN><<<dim3(cdiv(X * Y, 4), n_vol), 256, 0, st>>>(vol, X, Y, Z, root);
    cc_flatten_kernel<<<dim3(cc_stride_grid(V), n_vol), 256, 0, st>>>(root, V);
}

template <typename T, bool BINARY>
static void cc_roots_launch(const T* vol, int n_vol, int X, int Y, int Z, int connectivity, int* root, hipStream_t st) {
    if (connectivity == 1) cc_roots_launch_conn<T, BINARY, 1>(vol, n_vol, X, Y, Z, root, st);
    else if (connectivity == 2) cc_roots_launch_conn<T, BINARY, 2>(vol, n_vol, X, Y, Z, root, st);
    else cc_roots_launch_conn<T, BINARY, 3>(vol, n_vol, X, Y, Z, root, st);
}

extern "C" int dycon_cc_roots(const void* vol, int vol_bytes, int n_vol, int X, int Y, int Z, int connectivity, int by_value, int* root,
                              dycon_stream_t stream) {
    DYCON_REQUIRE(vol && root, "cc_roots: null pointer");
    DYCON_REQUIRE(vol_bytes == 1 || vol_bytes == 8, "cc_roots: the volume must be uint8 or int64 (vol_bytes = %d)", vol_bytes);
    CC_REQUIRE_SHAPE("cc_roots");
    DYCON_REQUIRE(connectivity >= 1 && connectivity <= 3, "cc_roots: connectivity %d (1, 2 or 3)", connectivity);
    hipStream_t st = (hipStream_t)stream;
    if (vol_bytes == 1) {
        if (by_value) cc_roots_launch<unsigned char, false>((const unsigned char*)vol, n_vol, X, Y, Z, connectivity, root, st);
        else cc_roots_launch<unsigned char, true>((const unsigned char*)vol, n_vol, X, Y, Z, connectivity, root, st);
    } else {
        if (by_value) cc_roots_launch<long long, false>((const long long*)vol, n_vol, X, Y, Z, connectivity, root, st);
        else cc_roots_launch<long long, true>((const long long*)vol, n_vol, X, Y, Z, connectivity, root, st);
    }
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

extern "C" int dycon_cc_labels(const int* root, int n_vol, int X, int Y, int Z, int* labels, int* ncomp, void* workspace,
                               size_t ws_bytes, dycon_stream_t stream) {
    DYCON_REQUIRE(root && labels && ncomp && workspace, "cc_labels: null pointer");
    CC_REQUIRE_SHAPE("cc_labels");
    DYCON_REQUIRE(ws_bytes >= dycon_cc_workspace(n_vol, X, Y, Z), "cc_labels: workspace of %zu bytes, %zu needed", ws_bytes,
                  dycon_cc_workspace(n_vol, X, Y, Z));
    hipStream_t st = (hipStream_t)stream;
    const long long V = (long long)X * Y * Z;
    const int nchunk = cc_nchunk(V);
    int* counts = (int*)((char*)workspace + cc_align((size_t)n_vol * V * sizeof(unsigned)) +
                         cc_align((size_t)n_vol * CC_MAX_CLS * sizeof(unsigned long long)));
    dim3 chunks(nchunk, n_vol);
    cc_count_roots_kernel<<<chunks, 256, 0, st>>>(root, V, nchunk, counts);
    cc_scan_chunks_kernel<<<n_vol, 256, 0, st>>>(counts, nchunk, ncomp);
    cc_rank_roots_kernel<<<chunks, 256, 0, st>>>(root, V, nchunk, counts, labels);
    cc_spread_labels_kernel<<<dim3(cc_stride_grid(V), n_vol), 256, 0, st>>>(root, V, labels);
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}

template <typename T, bool BINARY>
static void cc_largest_launch(const T* vol, const int* root, int n_vol, long long V, int n_cls, unsigned* sizes, unsigned long long* best,
                              unsigned char* out, int* win_size, int* win_root, hipStream_t st) {
    dim3 grid(cc_stride_grid(V), n_vol);
    cc_sizes_kernel<<<dim3(grid.x > 1024 ? 1024 : grid.x, n_vol), 256, 0, st>>>(root, V, sizes);       // fewer, longer workgroups: one flush each
    cc_select_kernel<T, BINARY><<<dim3(grid.x > 1024 ? 1024 : grid.x, n_vol), 256, 0, st>>>(vol, root, sizes, V, n_cls, best);
    cc_keep_kernel<T, BINARY><<<grid, 256, 0, st>>>(vol, root, best, V, n_cls, out, win_size, win_root);
}

extern "C" int dycon_cc_largest(const void* vol, int vol_bytes, const int* root, int n_vol, int X, int Y, int Z, int n_cls, uint8_t* out,
                                int* win_size, int* win_root, void* workspace, size_t ws_bytes, dycon_stream_t stream) {
    DYCON_REQUIRE(vol && root && out && win_size && win_root && workspace, "cc_largest: null pointer");
    DYCON_REQUIRE(vol_bytes == 1 || vol_bytes == 8, "cc_largest: the volume must be uint8 or int64 (vol_bytes = %d)", vol_bytes);
    CC_REQUIRE_SHAPE("cc_largest");
    DYCON_REQUIRE(n_cls >= 0 && n_cls <= CC_MAX_CLS, "cc_largest: n_cls = %d (0 = binary, 1..%d = the values 1..n_cls)", n_cls,
                  CC_MAX_CLS);
    DYCON_REQUIRE(ws_bytes >= dycon_cc_workspace(n_vol, X, Y, Z), "cc_largest: workspace of %zu bytes, %zu needed", ws_bytes,
                  dycon_cc_workspace(n_vol, X, Y, Z));
    hipStream_t st = (hipStream_t)stream;
    const long long V = (long long)X * Y * Z;
    const size_t size_bytes = cc_align((size_t)n_vol * V * sizeof(unsigned));
    unsigned* sizes = (unsigned*)workspace;
    unsigned long long* best = (unsigned long long*)((char*)workspace + size_bytes);
    const int slots = n_cls ? n_cls : 1;
    if (hipMemsetAsync(workspace, 0, size_bytes + (size_t)n_vol * slots * sizeof(unsigned long long), st) != hipSuccess) {
        dycon_set_error("cc_largest: hipMemsetAsync failed");
        return DYCON_ERR_LAUNCH;
    }
    if (vol_bytes == 1) {
        if (n_cls) cc_largest_launch<unsigned char, false>((const unsigned char*)vol, root, n_vol, V, slots, sizes, best, out, win_size, win_root, st);
        else cc_largest_launch<unsigned char, true>((const unsigned char*)vol, root, n_vol, V, slots, sizes, best, out, win_size, win_root, st);
    } else {
        if (n_cls) cc_largest_launch<long long, false>((const long long*)vol, root, n_vol, V, slots, sizes, best, out, win_size, win_root, st);
        else cc_largest_launch<long long, true>((const long long*)vol, root, n_vol, V, slots, sizes, best, out, win_size, win_root, st);
    }
    DYCON_LAUNCH_CHECK();
    return DYCON_OK;
}
