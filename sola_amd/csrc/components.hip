// Connected components of the set pixels of n independent frames [n,h,w], 4- or 8-connectivity (sola_mask_components), and
// the fused form that only rewrites small components (sola_mask_fill_small: SAM2's fill_holes_in_mask_scores, island and
// hole removal).  Union-find by MINIMUM RASTER INDEX over two int32 arrays in the caller's scratch, indexed like the
// pixels (i = (f*h + y)*w + x < 2^31):
//   parent[i]  -1 on clear pixels, else a pixel of i's component with parent[i] <= i.  It only ever decreases.
//   count[i]   pixels of the tile-local component rooted at i (0 anywhere else), later summed into the final root.
// Four launches on the stream; no workgroup ever waits for another, and what must be read exactly is read in a LATER launch:
//   1. cc_tile_kernel: one block of 256 threads per 64x16 tile.  Lanes lie along x, so __ballot gives a row of the tile as
//      one 64-bit word.  The union-find nodes are the ROW RUNS (a run is named by its first pixel): the first lane of every
//      run unions it in LDS with the runs of the row above that it touches (bit tricks on the two row words, atomicMin on
//      the LDS parents).  Every pixel then gets the global index of its tile-local root, every tile-local root its pixel
//      count.  Both arrays are written in full: nothing depends on what the scratch held.
//   2. cc_border_kernel: one thread per pixel of a tile's first row / first column unions it with its set neighbours in
//      the tile above / to the left (and, at 8-connectivity, the two diagonal ones, which covers the pairs that only meet
//      across a tile CORNER).  A pair is skipped where a neighbouring thread's pair plus in-tile adjacency already joins it
//      (see the kernel).  find / union use relaxed agent-scope atomic loads and atomicMin; a stale parent read would only
//      cost a step, because every value parent[i] ever held names a pixel of i's component.
//   3. cc_flatten_kernel: every tile-local root (count > 0) chases its chain to the final root - parents are final when
//      this launch starts, the chain strictly decreases - points at it and adds its count to the root's.  Integer atomics
//      only: the sums do not depend on the order.
//   4. cc_emit_*: root of a pixel = parent[parent[i]] (its tile-local root was flattened in 3), labels = 1 + root's index
//      inside its frame, areas = count[root]; or the fused rewrite of sola_mask_fill_small, which re-reads the input and
//      stores only what the contract changes when `out` aliases `in`.
#include "kernels.h"
#include "mask_elems.h"

namespace {

constexpr int CC_TW = SOLA_CC_TILE_W;  // 64: one wave along x
constexpr int CC_TH = SOLA_CC_TILE_H;  // 16
constexpr int CC_THREADS = 256;
constexpr int CC_ROWS_PER_WAVE = CC_TH / (CC_THREADS / 64);
static_assert(CC_TW == 64 && CC_TH % (CC_THREADS / 64) == 0, "a wave is one tile row");

typedef unsigned long long u64;

template <int KIND>  // element kinds 0 to 5: mask_elems.h
__device__ __forceinline__ bool cc_is_set(const void* p, long long i) {
    return mask_is_set<KIND>(static_cast<const typename mask_elem<KIND>::type*>(p)[i]);
}

__device__ __forceinline__ u64 bits_upto(int b) { return ~0ull >> (63 - b); }  // bits 0..b, b in 0..63
__device__ __forceinline__ int run_len(u64 m, int at) {                          // bit `at` of m is set: length of its run upwards
    const u64 z = ~(m >> at);
    return z ? __builtin_ctzll(z) : 64;
}

__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int lds_find(const int* par, int i) {
    int p = lds_load(par + i);
    while (p != i) {  // p < i
        i = p;
        p = lds_load(par + i);
    }
    return i;
}
__device__ __forceinline__ void lds_union(int* par, int a, int b) {
    for (;;) {  // a + b falls with every turn
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + a, b);
        if (old == a) return;
        a = old;  // somebody re-parented a to old < a in between: old's tree and b's still have to meet
    }
}

__device__ __forceinline__ int g_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(const int* parent, int i) {
    int p = g_load(parent + i);
    while (p != i) {  // p < i
        i = p;
        p = g_load(parent + i);
    }
    return i;
}
__device__ __forceinline__ void g_union(int* parent, int a, int b) {
    for (;;) {
        a = g_find(parent, a);
        b = g_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

struct CcDims {
    int n, h, w, tiles_x, tiles_y, conn8;
};

template <int KIND>
__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const void* __restrict__ in, const CcDims d, int* __restrict__ parent,
                                                             int* __restrict__ count) {
    __shared__ u64 rows[CC_TH];
    __shared__ int par[CC_TH * CC_TW];
    __shared__ int cnt[CC_TH * CC_TW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int t = blockIdx.x;
    const int tx = t % d.tiles_x;
    t /= d.tiles_x;
    const int ty = t % d.tiles_y, f = t / d.tiles_y;
    const int x = tx * CC_TW + lane;
    const int y0 = ty * CC_TH + wave * CC_ROWS_PER_WAVE;
    const int base = f * d.h * d.w;  // < 2^31 with the whole array

    u64 m[CC_ROWS_PER_WAVE];
#pragma unroll
    for (int k = 0; k < CC_ROWS_PER_WAVE; ++k) {
        const int ly = wave * CC_ROWS_PER_WAVE + k, y = y0 + k;
        const bool s = x < d.w && y < d.h && cc_is_set<KIND>(in, (long long)base + (long long)y * d.w + x);
        m[k] = __ballot(s);
        if (lane == 0) rows[ly] = m[k];
        par[ly * CC_TW + lane] = ly * CC_TW + lane;
        cnt[ly * CC_TW + lane] = 0;
    }
    __syncthreads();

    // the first lane of every run joins it to the runs of the row above that it touches
    bool start[CC_ROWS_PER_WAVE];
    int root[CC_ROWS_PER_WAVE];
#pragma unroll
    for (int k = 0; k < CC_ROWS_PER_WAVE; ++k) {
        const int ly = wave * CC_ROWS_PER_WAVE + k;
        start[k] = ((m[k] >> lane) & 1) && (lane == 0 || !((m[k] >> (lane - 1)) & 1));
        if (start[k] && ly > 0) {
            const u64 pm = rows[ly - 1];
            const int len = run_len(m[k], lane);
            u64 span = (len == 64 ? ~0ull : ((1ull << len) - 1)) << lane;
            if (d.conn8) span |= (span << 1) | (span >> 1);
            u64 ov = pm & span;
            const u64 pstarts = pm & ~(pm << 1);
            while (ov) {  // one turn per touched run of the row above
                const int b = __builtin_ctzll(ov);
                const int ps = 63 - __builtin_clzll(pstarts & bits_upto(b));
                lds_union(par, ly * CC_TW + lane, (ly - 1) * CC_TW + ps);
                const int e = b + run_len(pm, b);  // one past that run
                ov = e >= 64 ? 0ull : ov & ~((1ull << e) - 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_ROWS_PER_WAVE; ++k)  // the unions are complete: exact roots
        root[k] = start[k] ? lds_find(par, (wave * CC_ROWS_PER_WAVE + k) * CC_TW + lane) : 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_ROWS_PER_WAVE; ++k)
        if (start[k]) {
            par[(wave * CC_ROWS_PER_WAVE + k) * CC_TW + lane] = root[k];
            atomicAdd(cnt + root[k], run_len(m[k], lane));
        }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_ROWS_PER_WAVE; ++k) {
        const int ly = wave * CC_ROWS_PER_WAVE + k, y = y0 + k;
        if (x >= d.w || y >= d.h) continue;
        const int g = base + y * d.w + x;
        int p = -1, c = 0;
        if ((m[k] >> lane) & 1) {
            const u64 starts = m[k] & ~(m[k] << 1);
            const int rs = 63 - __builtin_clzll(starts & bits_upto(lane));
            const int r = par[ly * CC_TW + rs];
            p = base + (ty * CC_TH + r / CC_TW) * d.w + tx * CC_TW + r % CC_TW;
            if (r == ly * CC_TW + lane) c = cnt[r];
        }
        parent[g] = p;
        count[g] = c;
    }
}

// Pairs across tile edges.  Per frame: (tiles_y - 1) * w threads on the first rows of the tiles below the top one, then
// (tiles_x - 1) * h threads on the first columns.  p = the thread's pixel; u, l = the pixels above / left of it.
// Skipped pairs (every one rests on pairs that are NOT skipped, or skipped further along the same row / column):
//   row thread, p-u:     when the pixels left of both are set: thread x-1 joins those two, and horizontal neighbours are
//                        joined in their tile or by the column thread, which never skips on a tile's first row;
//   column thread, p-l:  the same one row up, except on a tile's first row;
//   diagonals:           when one of the two pixels that complete the square on the pair's side is set, since the pair
//                        is then joined through two straight pairs.
__global__ __launch_bounds__(256) void cc_border_kernel(const CcDims d, int* parent, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int h = d.h, w = d.w;
    const long long row_part = (long long)(d.tiles_y - 1) * w;
    const long long per_frame = row_part + (long long)(d.tiles_x - 1) * h;
    const int f = (int)(idx / per_frame);
    const long long rem = idx - (long long)f * per_frame;
    const int base = f * h * w;
    auto set = [&](int yy, int xx) { return yy >= 0 && yy < h && xx >= 0 && xx < w && parent[base + yy * w + xx] >= 0; };
    if (rem < row_part) {
        const int y = ((int)(rem / w) + 1) * CC_TH, x = (int)(rem % w);
        const int p = base + y * w + x;
        if (parent[p] < 0) return;
        const bool u = set(y - 1, x);
        if (u && !(set(y, x - 1) && set(y - 1, x - 1))) g_union(parent, p, p - w);
        if (d.conn8 && !u) {
            if (set(y - 1, x - 1) && !set(y, x - 1)) g_union(parent, p, p - w - 1);
            if (set(y - 1, x + 1) && !set(y, x + 1)) g_union(parent, p, p - w + 1);
        }
    } else {
        const long long r2 = rem - row_part;
        const int x = ((int)(r2 / h) + 1) * CC_TW, y = (int)(r2 % h);
        const int p = base + y * w + x;
        if (parent[p] < 0) return;
        const bool l = set(y, x - 1);
        if (l && !(y % CC_TH != 0 && set(y - 1, x) && set(y - 1, x - 1))) g_union(parent, p, p - 1);
        if (d.conn8 && !l) {
            if (set(y - 1, x - 1) && !set(y - 1, x)) g_union(parent, p, p - w - 1);
            if (set(y + 1, x - 1) && !set(y + 1, x)) g_union(parent, p, p + w - 1);
        }
    }
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(int* parent, int* count, int total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = count[i];  // > 0: a tile-local root.  Only final roots are added to in this launch, and those stop below
    if (c <= 0) return;
    const int r = g_find(parent, (int)i);
    if (r == (int)i) return;
    __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(count + r, c);
}

__device__ __forceinline__ int cc_root(const int* __restrict__ parent, int i, int p) {  // p = parent[i] >= 0, after the flatten launch
    return p == i ? p : parent[p];
}

__global__ __launch_bounds__(256) void cc_emit_labels_kernel(const int* __restrict__ parent, const int* __restrict__ count, int hw,
                                                             int* __restrict__ labels, int* __restrict__ areas, int total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int p = parent[i];
    int lab = 0, area = 0;
    if (p >= 0) {
        const int r = cc_root(parent, (int)i, p);
        lab = r - ((int)i / hw) * hw + 1;
        area = count[r];
    }
    labels[i] = lab;
    areas[i] = area;
}

template <int KIND>
__global__ __launch_bounds__(256) void cc_emit_fill_kernel(const void* in, void* out, const int* __restrict__ parent,
                                                           const int* __restrict__ count, long long max_area, uint32_t fill, int total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    constexpr bool BYTES = mask_elem<KIND>::size == 1;
    uint32_t v;  // the element's bits: floats pass through as integers, NaN payloads included
    if constexpr (BYTES) v = static_cast<const uint8_t*>(in)[i];
    else v = static_cast<const uint32_t*>(in)[i];
    const int p = parent[i];
    bool change = false;
    if (p >= 0) change = (long long)count[cc_root(parent, (int)i, p)] <= max_area;
    if (!change && in == out) return;
    if (change) v = fill;
    if constexpr (BYTES) static_cast<uint8_t*>(out)[i] = (uint8_t)v;
    else static_cast<uint32_t*>(out)[i] = v;
}

struct CcEvents {  // optional: the four launches between five events (sola_mask_fill_small_profile)
    hipEvent_t ev[5] = {};
    int made = 0;
    ~CcEvents() {
        for (int i = 0; i < made; ++i) (void)hipEventDestroy(ev[i]);
    }
};

// fused: the rewrite of sola_mask_fill_small into out; else labels and areas
int cc_run(bool fused, const void* in, int elem_type, int n, int h, int w, int connectivity, int32_t* labels, int32_t* areas,
           long long max_area, float fill_value, void* out, void* scratch, size_t scratch_bytes, hipStream_t s, float* launch_us) {
    const char* who = fused ? "mask_fill_small" : "mask_components";
    SOLA_ARG(n >= 0 && h >= 0 && w >= 0, "%s: negative size (n %d, h %d, w %d)", who, n, h, w);
    SOLA_ARG(elem_type >= 0 && elem_type <= 5, "%s: elem_type %d outside 0..5", who, elem_type);
    SOLA_ARG(connectivity == 4 || connectivity == 8, "%s: connectivity %d is neither 4 nor 8", who, connectivity);
    SOLA_ARG(max_area >= 0, "%s: max_area %lld < 0", who, max_area);
    if (launch_us) launch_us[0] = launch_us[1] = launch_us[2] = launch_us[3] = 0.f;
    if (n == 0 || h == 0 || w == 0) return SOLA_OK;
    const long long total = (long long)n * h * w;
    SOLA_ARG(total < (1ll << 31), "%s: n*h*w = %lld >= 2^31", who, total);
    SOLA_ARG(in && scratch && (fused ? out != nullptr : labels && areas), "%s: null argument", who);
    SOLA_ARG((reinterpret_cast<uintptr_t>(scratch) & 3) == 0, "%s: scratch must be 4-byte aligned", who);
    const size_t need = components_scratch_bytes(n, h, w);
    SOLA_ARG(scratch_bytes >= need, "%s: scratch of %zu bytes, %zu needed", who, scratch_bytes, need);

    CcDims d{n, h, w, (w + CC_TW - 1) / CC_TW, (h + CC_TH - 1) / CC_TH, connectivity == 8 ? 1 : 0};
    int* parent = static_cast<int*>(scratch);
    int* count = parent + total;
    const long long n_tiles = (long long)n * d.tiles_x * d.tiles_y;
    SOLA_ARG(n_tiles < (1ll << 24), "%s: %lld tiles of %dx%d, at most 2^24 - 1 in one call", who, n_tiles, CC_TW, CC_TH);
    const unsigned tiles = (unsigned)n_tiles;
    const unsigned px_blocks = (unsigned)((total + 255) / 256);
    CcEvents E;
    if (launch_us)
        for (; E.made < 5; ++E.made) SOLA_HIP(hipEventCreate(&E.ev[E.made]));
    auto mark = [&](int i) { return launch_us ? hipEventRecord(E.ev[i], s) : hipSuccess; };

    SOLA_HIP(mark(0));
    with_mask_kind<MASK_F32_CLEAR>(elem_type, [&](auto kind) {
        hipLaunchKernelGGL(cc_tile_kernel<decltype(kind)::value>, dim3(tiles), dim3(CC_THREADS), 0, s, in, d, parent, count);
    });
    SOLA_LAUNCH_CHECK();
    SOLA_HIP(mark(1));
    const long long edges = (long long)n * ((long long)(d.tiles_y - 1) * w + (long long)(d.tiles_x - 1) * h);
    if (edges > 0) {
        hipLaunchKernelGGL(cc_border_kernel, dim3((unsigned)((edges + 255) / 256)), dim3(256), 0, s, d, parent, edges);
        SOLA_LAUNCH_CHECK();
    }
    SOLA_HIP(mark(2));
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(px_blocks), dim3(256), 0, s, parent, count, (int)total);
    SOLA_LAUNCH_CHECK();
    SOLA_HIP(mark(3));
    if (!fused) {
        hipLaunchKernelGGL(cc_emit_labels_kernel, dim3(px_blocks), dim3(256), 0, s, parent, count, h * w, labels, areas, (int)total);
    } else {
        // what a small component becomes: kinds 0 to 2 are cleared; 3 takes fill_value, 4 and 5 a one of their type
        const uint32_t fill = elem_type == MASK_LOGIT_CLEAR ? __builtin_bit_cast(uint32_t, fill_value)
                              : elem_type == MASK_U8_CLEAR  ? 1u
                              : elem_type == MASK_F32_CLEAR ? 0x3f800000u
                                                            : 0u;
        with_mask_kind<MASK_F32_CLEAR>(elem_type, [&](auto kind) {
            hipLaunchKernelGGL(cc_emit_fill_kernel<decltype(kind)::value>, dim3(px_blocks), dim3(256), 0, s, in, out, parent, count, max_area,
                               fill, (int)total);
        });
    }
    SOLA_LAUNCH_CHECK();
    SOLA_HIP(mark(4));
    if (launch_us) {
        SOLA_HIP(hipEventSynchronize(E.ev[4]));
        for (int i = 0; i < 4; ++i) {
            float ms = 0.f;
            SOLA_HIP(hipEventElapsedTime(&ms, E.ev[i], E.ev[i + 1]));
            launch_us[i] = ms * 1000.f;
        }
    }
    return SOLA_OK;
}

}  // namespace

size_t components_scratch_bytes(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    const long long total = (long long)n * h * w;
    if (total >= (1ll << 31)) return 0;
    return ((size_t)total * 8 + 255) / 256 * 256;  // parent and count, int32 each
}

int launch_mask_components(const void* masks, int elem_type, int n, int h, int w, int connectivity, int32_t* labels, int32_t* areas,
                           void* scratch, size_t scratch_bytes, hipStream_t s) {
    return cc_run(false, masks, elem_type, n, h, w, connectivity, labels, areas, 0, 0.f, nullptr, scratch, scratch_bytes, s, nullptr);
}

int launch_mask_fill_small(const void* in, int elem_type, int n, int h, int w, int connectivity, long long max_area, float fill_value,
                           void* out, void* scratch, size_t scratch_bytes, hipStream_t s, float* launch_us) {
    return cc_run(true, in, elem_type, n, h, w, connectivity, nullptr, nullptr, max_area, fill_value, out, scratch, scratch_bytes, s, launch_us);
}
