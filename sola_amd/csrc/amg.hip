// The grid-prompt stage (SAM2's automatic mask generator in front of generate_prompts_grid.py) on the GPU: per-mask
// statistics from ONE read of the mask logits, and greedy box NMS.
//
// sola_mask_logit_stats: n maps [n,h,w] -> stats int64 [n,7] = (n_hi, n_lo, area, x0, y0, x1, y1): the pixels above thr_hi,
// thr_lo and thr, and the inclusive bounding box of the pixels above thr ((0,0,0,0) when there are none).  Three operations on
// the stream:
//   1. hipMemsetAsync of the table to zero.
//   2. amg_stats_kernel: one block of 256 threads per AMG_CHUNK_BYTES (64 KiB) piece of ONE map, taken over the map's flat
//      index p = y*w + x.  A lane reads 16 bytes at a time (4 float32 / 16 uint8 pixels) wherever the ADDRESS is 16-byte
//      aligned - the alignment is worked out on the absolute address, so rows of odd w and maps that start off a 16-byte
//      boundary lose nothing but the < 16 bytes at either end of a piece, which single lanes read pixel by pixel.  The
//      vector's pixels become bits (one word per threshold); counts are popcounts, the box comes from the first and last
//      set bit.  (x, y) of a lane's vector is divided out once and then advanced by the constant step of 256 vectors.
//      A vector that crosses a row end walks its set bits one by one, which is also what any w < 16 does.
//      The block's seven numbers meet in LDS and go to the table with 64-bit integer atomics: add for the counts, max for
//      the box, where x0 and y0 travel as w - x and h - y so that every slot starts from the memset's zero and only grows.
//   3. amg_stats_finish_kernel: one thread per map turns w - x0, h - y0 back (maps with area 0 stay all zero).
// Integer atomics only, nothing read before the launch that follows its writers: the table is identical from run to run.
//
// sola_box_nms: boxes [n,4] xyxy visited in the order dev_order; a box is kept unless an earlier KEPT box of its category has
// iou > iou_threshold.  Two launches:
//   1. nms_matrix_kernel: block (c, r), c >= r, of 64 threads: thread t holds box order[64r + t], the 64 boxes order[64c ..]
//      are staged in LDS, and the thread writes word (64r + t, c) of the suppression matrix: bit j = box 64c + j comes later
//      than the thread's, shares its category and overlaps it by more than the threshold.  Only the upper triangle (words with
//      c >= r) is ever written or read.  The IoU is float32 with every operation rounded on its own (no contraction, see below).
//   2. nms_resolve_kernel: ONE block of 1024 threads walks the 64-row chunks in order.  Wave 0 holds the chunk's diagonal
//      words, one per lane, and settles its 64 rows serially in registers (removed |= diag[j] for every j not yet removed);
//      then all threads OR the kept rows of the chunk into the removed words of the later columns (16 row groups x 64
//      columns, combined in LDS).  A chunk costs one global round trip, not 64.  Last, the kept bits are scanned and the
//      kept original indices written in visiting order.
// The scratch is the matrix alone, n * ceil(n/64) words of 64 bits; every word that is read was written by launch 1.
#include "kernels.h"
#include "mask_elems.h"

// The NMS decision is specified as separately rounded float32 operations: no a*b+c may become one fma in this file (the
// Makefile also passes -ffp-contract=off for it).
#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

// ---------------------------------------------------------------------------------------------------------------- stats
constexpr int AMG_THREADS = 256;
constexpr int AMG_CHUNK_BYTES = 64 * 1024;
constexpr int AMG_VECS = AMG_CHUNK_BYTES / 16 / AMG_THREADS;  // 16-byte vectors per thread and block
constexpr int AMG_BATCH = 8;                                  // of them loaded before the first is used
static_assert(AMG_VECS % AMG_BATCH == 0, "whole batches");

struct StatsArgs {
    const void* masks;
    u64* stats;
    long long hw;        // pixels of a map, < 2^31
    int h, w;
    int chunks;          // blocks per map
    int base_mod;        // (address of masks / element size) mod pixels per vector
    int step_y, step_x;  // (AMG_THREADS * pixels per vector) divided by w: quotient, remainder
    float thr, thr_hi, thr_lo;
};

struct StatsAcc {
    uint32_t n_hi = 0, n_lo = 0, area = 0;  // a thread sees at most AMG_CHUNK_BYTES / AMG_THREADS + 15 pixels
    int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
    __device__ __forceinline__ void pixel(int x, int y) {
        x0 = min(x0, x); x1 = max(x1, x);
        y0 = min(y0, y); y1 = max(y1, y);
    }
};

// kind 2 is read against the three thresholds; masks (kinds 0, 1) are the same bits for all three
template <int KIND>
__device__ __forceinline__ void amg_one(const void* masks, long long at, int x, int y, const StatsArgs& a, StatsAcc& s) {
    const auto v = static_cast<const typename mask_elem<KIND>::type*>(masks)[at];
    const bool on = mask_is_set<KIND>(v, a.thr);
    bool hi = on, lo = on;
    if constexpr (KIND == MASK_LOGIT) { hi = mask_is_set<KIND>(v, a.thr_hi); lo = mask_is_set<KIND>(v, a.thr_lo); }
    s.n_hi += hi; s.n_lo += lo;
    if (on) { s.area += 1; s.pixel(x, y); }
}

template <int KIND>
__global__ __launch_bounds__(AMG_THREADS) void amg_stats_kernel(const StatsArgs a) {
    constexpr int V = 16 / mask_elem<KIND>::size;    // pixels per 16-byte vector
    constexpr int CHUNK = AMG_CHUNK_BYTES / 16 * V;  // pixels per block
    __shared__ u64 red[7][AMG_THREADS / 64];
    const int tid = threadIdx.x;
    const int m = (int)(blockIdx.x / (unsigned)a.chunks);
    const int c = (int)(blockIdx.x - (unsigned)m * (unsigned)a.chunks);
    const long long first = (long long)m * a.hw;  // the map's first pixel in the whole array
    const int w = a.w;
    const int lo = c * CHUNK;                                             // < hw < 2^31
    const int hi = (int)min((long long)lo + CHUNK, a.hw);
    const MaskPiece pc = mask_piece<V>(a.base_mod, first, lo, hi);
    const int v_lo = pc.v_lo, n_vec = pc.n_vec;
    StatsAcc s;

    if (tid < pc.n_edge) {
        const int p = tid < pc.n_head ? lo + tid : pc.v_hi + (tid - pc.n_head);
        const int y = p / w;
        amg_one<KIND>(a.masks, first + p, p - y * w, y, a, s);
    }

    if (tid < n_vec) {
        const int p0 = v_lo + tid * V;
        int y = p0 / w, x = p0 - y * w;
        using Vec = typename mask_elem<KIND>::vec;
        const Vec* src = reinterpret_cast<const Vec*>(static_cast<const char*>(a.masks) + (first + p0) * mask_elem<KIND>::size);
        for (int k0 = 0; k0 < AMG_VECS && k0 * AMG_THREADS < n_vec; k0 += AMG_BATCH) {
            // AMG_BATCH loads in flight per lane; a vector past the end re-reads the piece's last one and is not counted
            Vec data[AMG_BATCH];
#pragma unroll
            for (int j = 0; j < AMG_BATCH; ++j) data[j] = src[(size_t)min((k0 + j) * AMG_THREADS, n_vec - 1 - tid)];
#pragma unroll
            for (int j = 0; j < AMG_BATCH; ++j) {
                if (tid + (k0 + j) * AMG_THREADS < n_vec) {
                    const Vec d = data[j];
                    const uint32_t b_on = vec_bits<KIND>(d, a.thr);
                    uint32_t b_hi = b_on, b_lo = b_on;
                    if constexpr (KIND == MASK_LOGIT) { b_hi = vec_bits<KIND>(d, a.thr_hi); b_lo = vec_bits<KIND>(d, a.thr_lo); }
                    s.n_hi += __popc(b_hi);
                    s.n_lo += __popc(b_lo);
                    s.area += __popc(b_on);
                    if (b_on) {
                        if (x + V <= w) {  // the vector lies in one row
                            s.pixel(x + __builtin_ctz(b_on), y);
                            s.pixel(x + 31 - __builtin_clz(b_on), y);
                        } else {
                            uint32_t b = b_on;
                            int xx = x, yy = y, at = 0;
                            while (b) {
                                const int i = __builtin_ctz(b);
                                b &= b - 1;
                                xx += i - at;
                                at = i;
                                while (xx >= w) { xx -= w; ++yy; }
                                s.pixel(xx, yy);
                            }
                        }
                    }
                }
                x += a.step_x;
                y += a.step_y;
                if (x >= w) { x -= w; ++y; }
            }
        }
    }

    // w - x0 and h - y0 grow as x0 and y0 fall; a thread without pixels contributes 0 everywhere
    u64 v[7] = {s.n_hi, s.n_lo, s.area, 0, 0, 0, 0};
    if (s.area) {
        v[3] = (u64)(w - s.x0); v[4] = (u64)(a.h - s.y0); v[5] = (u64)s.x1; v[6] = (u64)s.y1;
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        uint32_t r = (uint32_t)v[i];  // every one of them is below 2^31
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t other = __shfl_xor(r, o, 64);
            r = i < 3 ? r + other : max(r, other);
        }
        v[i] = r;
    }
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0)
        for (int i = 0; i < 7; ++i) red[i][wave] = v[i];
    __syncthreads();
    if (tid < 7) {
        u64 r = 0;
        for (int j = 0; j < AMG_THREADS / 64; ++j) r = tid < 3 ? r + red[tid][j] : max(r, red[tid][j]);
        if (r) {
            u64* slot = a.stats + (long long)m * 7 + tid;
            if (tid < 3) atomicAdd(slot, r);
            else atomicMax(slot, r);
        }
    }
}

__global__ __launch_bounds__(256) void amg_stats_finish_kernel(u64* stats, int n, int h, int w) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    u64* row = stats + (long long)i * 7;
    if (row[2] == 0) return;
    row[3] = (u64)w - row[3];
    row[4] = (u64)h - row[4];
}

// ------------------------------------------------------------------------------------------------------------------ NMS
constexpr int NMS_RESOLVE_THREADS = 1024;
constexpr int NMS_MAX_WORDS = SOLA_BOX_NMS_MAX_N / 64;
static_assert(SOLA_BOX_NMS_MAX_N % 64 == 0 && NMS_MAX_WORDS <= 65535, "the matrix kernel's grid is (words, words)");

struct NmsBox {
    float x0, y0, x1, y1, area;
    long long cat;
};

__device__ __forceinline__ NmsBox nms_load(const float* __restrict__ boxes, const long long* __restrict__ order,
                                           const long long* __restrict__ idxs, int i, int n) {
    NmsBox b{0.f, 0.f, 0.f, 0.f, 0.f, 0};
    if (i >= n) return b;
    long long o = order[i];
    if (o < 0 || o >= n) o = 0;  // never a read outside the arrays
    const float4 v = reinterpret_cast<const float4*>(boxes)[o];
    b.x0 = v.x; b.y0 = v.y; b.x1 = v.z; b.y1 = v.w;
    b.area = (v.z - v.x) * (v.w - v.y);
    b.cat = idxs ? idxs[o] : 0;
    return b;
}

__global__ __launch_bounds__(64) void nms_matrix_kernel(const float* __restrict__ boxes, const long long* __restrict__ order,
                                                        const long long* __restrict__ idxs, int n, int words, float thr,
                                                        u64* __restrict__ matrix) {
    const int c = blockIdx.x, r = blockIdx.y;
    if (c < r) return;
    __shared__ NmsBox col[64];
    const int t = threadIdx.x;
    col[t] = nms_load(boxes, order, idxs, c * 64 + t, n);
    __syncthreads();
    const int row = r * 64 + t;
    if (row >= n) return;
    const NmsBox a = nms_load(boxes, order, idxs, row, n);
    const int n_col = min(64, n - c * 64);
    u64 bits = 0;
    for (int j = (c == r ? t + 1 : 0); j < n_col; ++j) {
        const NmsBox b = col[j];
        const float iw = fmaxf(0.f, fminf(a.x1, b.x1) - fmaxf(a.x0, b.x0));
        const float ih = fmaxf(0.f, fminf(a.y1, b.y1) - fmaxf(a.y0, b.y0));
        const float inter = iw * ih;
        const float iou = inter / ((a.area + b.area) - inter);  // correctly rounded: the build has no fast-math flag
        if (a.cat == b.cat && iou > thr) bits |= 1ull << j;  // NaN (0/0) does not suppress
    }
    matrix[(size_t)row * words + c] = bits;
}

__device__ __forceinline__ u64 nms_lane_word(u64 v, int lane) {  // lane: the same constant in every thread
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return (u64)hi << 32 | lo;
}

__global__ __launch_bounds__(NMS_RESOLVE_THREADS) void nms_resolve_kernel(const u64* __restrict__ matrix,
                                                                          const long long* __restrict__ order, int n, int words,
                                                                          long long* __restrict__ keep, long long* __restrict__ n_keep) {
    __shared__ u64 removed[NMS_MAX_WORDS];
    __shared__ u64 kept[NMS_MAX_WORDS];
    __shared__ int offset[NMS_MAX_WORDS + 1];
    __shared__ u64 chunk_kept;
    const int tid = threadIdx.x, lane = tid & 63, group = tid >> 6;  // 16 row groups of 64 column lanes
    for (int i = tid; i < words; i += NMS_RESOLVE_THREADS) removed[i] = 0;
    __syncthreads();
    for (int k = 0; k < words; ++k) {
        if (group == 0) {  // wave 0: the chunk's own 64 rows, in order, in registers
            const int row = k * 64 + lane;
            const u64 diag = row < n ? matrix[(size_t)row * words + k] : 0ull;
            u64 rem = removed[k];
            if (n - k * 64 < 64) rem |= ~0ull << (n - k * 64);  // rows past the end are nobody's
#pragma unroll
            for (int j = 0; j < 64; ++j) {
                const u64 dj = nms_lane_word(diag, j);
                if (!((rem >> j) & 1)) rem |= dj;
            }
            if (lane == 0) {
                chunk_kept = ~rem;
                kept[k] = ~rem;
            }
        }
        __syncthreads();
        const u64 kp = chunk_kept;
        for (int c = k + 1 + lane; c < words; c += 64) {
            u64 acc = 0;
            for (int j = group; j < 64; j += NMS_RESOLVE_THREADS / 64)
                if ((kp >> j) & 1) acc |= matrix[(size_t)(k * 64 + j) * words + c];  // a kept row is a row < n
            if (acc) atomicOr(&removed[c], acc);
        }
        __syncthreads();
    }
    if (tid == 0) {
        int total = 0;
        for (int k = 0; k < words; ++k) {
            offset[k] = total;
            total += __popcll(kept[k]);
        }
        offset[words] = total;
        *n_keep = total;
    }
    __syncthreads();
    for (int i = tid; i < n; i += NMS_RESOLVE_THREADS) {
        const u64 kp = kept[i >> 6];
        const int j = i & 63;
        if ((kp >> j) & 1) keep[offset[i >> 6] + __popcll(kp & ((1ull << j) - 1))] = order[i];
    }
}

struct NmsEvents {
    hipEvent_t ev[3] = {};
    int made = 0;
    ~NmsEvents() {
        for (int i = 0; i < made; ++i) (void)hipEventDestroy(ev[i]);
    }
};

int nms_run(const float* boxes, const int64_t* order, const int64_t* idxs, int n, float thr, int64_t* keep, int64_t* n_keep,
            void* scratch, size_t scratch_bytes, hipStream_t s, float* launch_us) {
    SOLA_ARG(n >= 0, "box_nms: negative n (%d)", n);
    SOLA_ARG(n <= SOLA_BOX_NMS_MAX_N, "box_nms: n = %d, at most %d boxes in one call", n, SOLA_BOX_NMS_MAX_N);
    SOLA_ARG(n_keep, "box_nms: null n_keep");
    if (launch_us) launch_us[0] = launch_us[1] = 0.f;
    if (n == 0) {
        SOLA_HIP(hipMemsetAsync(n_keep, 0, sizeof(int64_t), s));
        return SOLA_OK;
    }
    SOLA_ARG(boxes && order && keep && scratch, "box_nms: null argument");
    SOLA_ARG((reinterpret_cast<uintptr_t>(boxes) & 15) == 0, "box_nms: boxes must be 16-byte aligned");
    SOLA_ARG((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "box_nms: scratch must be 8-byte aligned");
    const size_t need = sola_box_nms_scratch_bytes(n);
    SOLA_ARG(scratch_bytes >= need, "box_nms: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    const int words = (n + 63) / 64;
    u64* matrix = static_cast<u64*>(scratch);
    NmsEvents E;
    if (launch_us)
        for (; E.made < 3; ++E.made) SOLA_HIP(hipEventCreate(&E.ev[E.made]));
    auto mark = [&](int i) { return launch_us ? hipEventRecord(E.ev[i], s) : hipSuccess; };
    SOLA_HIP(mark(0));
    hipLaunchKernelGGL(nms_matrix_kernel, dim3(words, words), dim3(64), 0, s, boxes, reinterpret_cast<const long long*>(order),
                       reinterpret_cast<const long long*>(idxs), n, words, thr, matrix);
    SOLA_LAUNCH_CHECK();
    SOLA_HIP(mark(1));
    hipLaunchKernelGGL(nms_resolve_kernel, dim3(1), dim3(NMS_RESOLVE_THREADS), 0, s, matrix, reinterpret_cast<const long long*>(order), n,
                       words, reinterpret_cast<long long*>(keep), reinterpret_cast<long long*>(n_keep));
    SOLA_LAUNCH_CHECK();
    SOLA_HIP(mark(2));
    if (launch_us) {
        SOLA_HIP(hipEventSynchronize(E.ev[2]));
        for (int i = 0; i < 2; ++i) {
            float ms = 0.f;
            SOLA_HIP(hipEventElapsedTime(&ms, E.ev[i], E.ev[i + 1]));
            launch_us[i] = ms * 1000.f;
        }
    }
    return SOLA_OK;
}

}  // namespace

extern "C" int sola_mask_logit_stats(const void* masks, int elem_type, int n, int h, int w, float thr, float thr_hi, float thr_lo,
                                     int64_t* stats, void* stream_) {
    SOLA_ARG(n >= 0 && h >= 0 && w >= 0, "mask_logit_stats: negative size (n %d, h %d, w %d)", n, h, w);
    SOLA_ARG(elem_type >= 0 && elem_type <= 2, "mask_logit_stats: elem_type %d outside 0..2", elem_type);
    if (n == 0) return SOLA_OK;
    const long long hw = (long long)h * w;
    SOLA_ARG(hw < (1ll << 31), "mask_logit_stats: h*w = %lld >= 2^31", hw);
    SOLA_ARG(stats, "mask_logit_stats: null stats");
    hipStream_t s = as_stream(stream_);
    SOLA_ARG((reinterpret_cast<uintptr_t>(stats) & 7) == 0, "mask_logit_stats: stats must be 8-byte aligned");
    const int esize = elem_type == 0 ? 1 : 4, V = 16 / esize;
    const long long chunk = AMG_CHUNK_BYTES / esize;
    const long long chunks = (hw + chunk - 1) / chunk;  // <= 2^17
    const long long blocks = chunks * n;
    SOLA_ARG(blocks < (1ll << 31), "mask_logit_stats: %lld pieces of %d bytes, at most 2^31 - 1 in one call", blocks, AMG_CHUNK_BYTES);
    if (hw > 0) {
        SOLA_ARG(masks, "mask_logit_stats: null masks");
        SOLA_ARG(reinterpret_cast<uintptr_t>(masks) % esize == 0, "mask_logit_stats: masks must be aligned to their element");
    }
    SOLA_HIP(hipMemsetAsync(stats, 0, (size_t)n * 7 * sizeof(int64_t), s));
    if (hw == 0) return SOLA_OK;
    StatsArgs a{};
    a.masks = masks;
    a.stats = reinterpret_cast<u64*>(stats);
    a.hw = hw; a.h = h; a.w = w;
    a.chunks = (int)chunks;
    a.base_mod = (int)((reinterpret_cast<uintptr_t>(masks) / esize) % V);
    a.step_y = (AMG_THREADS * V) / w;
    a.step_x = (AMG_THREADS * V) % w;
    a.thr = thr; a.thr_hi = thr_hi; a.thr_lo = thr_lo;
    with_mask_kind<MASK_LOGIT>(elem_type, [&](auto kind) {
        hipLaunchKernelGGL(amg_stats_kernel<decltype(kind)::value>, dim3((unsigned)blocks), dim3(AMG_THREADS), 0, s, a);
    });
    SOLA_LAUNCH_CHECK();
    hipLaunchKernelGGL(amg_stats_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a.stats, n, h, w);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

extern "C" size_t sola_box_nms_scratch_bytes(int n) {
    if (n <= 0 || n > SOLA_BOX_NMS_MAX_N) return 0;
    return ((size_t)n * ((n + 63) / 64) * 8 + 255) / 256 * 256;
}

extern "C" int sola_box_nms(const float* boxes, const int64_t* order, const int64_t* idxs, int n, float iou_threshold, int64_t* keep,
                            int64_t* n_keep, void* scratch, size_t scratch_bytes, void* stream_) {
    return nms_run(boxes, order, idxs, n, iou_threshold, keep, n_keep, scratch, scratch_bytes, as_stream(stream_), nullptr);
}

extern "C" int sola_box_nms_profile(const float* boxes, const int64_t* order, const int64_t* idxs, int n, float iou_threshold,
                                    int64_t* keep, int64_t* n_keep, void* scratch, size_t scratch_bytes, void* stream_,
                                    float* launch_us) {
    SOLA_ARG(launch_us, "box_nms_profile: null launch_us");
    return nms_run(boxes, order, idxs, n, iou_threshold, keep, n_keep, scratch, scratch_bytes, as_stream(stream_), launch_us);
}
