// What the GEMM kernels (gemm.hip, gemm_f32p.hip, gemm_glds.hip, gemm_tn.hip, gemm_tn_f32p.hip, gemm_tn_tr.hip and the
// closed experiments lab/gemm_k16.hip, lab/gemm_pp.hip) share, stated once: the conv window of an output row, the order in which block or
// tile ids walk the output, the piece layout of the direct-to-LDS kernels and their zero page, and on the host the XCD-remap rule and the
// GemmDesc -> kernel-argument fill.  Every args struct keeps its own members and order (the kernarg layout is the kernel's); the templates
// below only rely on the shared member NAMES.  The f16 range guard, the 16-bit converters and launch_lds are in common.h: more than the
// GEMMs use them.  profiles/gemm_common_isa.txt: kernel by kernel, what the compiler makes of these helpers against the written-out forms,
// and which kernels kept a local form on that evidence.
#pragma once
#include "kernels.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// 16 bytes of zeros: what a conv tap outside its sequence (or a row beyond the reduction) reads - the LDS-DMA cannot predicate data - and
// the base of a buffer descriptor before its first tile.  Internal linkage: one per translation unit.
static __device__ __attribute__((aligned(16))) float g_zero_page[4] = {0.f, 0.f, 0.f, 0.f};

// ---- device: the conv window of an output row --------------------------------------------------------------------------------------
// bit kk set <=> 0 <= t0 + kk < T_in, for the (at most 8) taps of a conv window starting at time t0
__device__ __forceinline__ int conv_tap_bits(int t0, int T_in) {
    int bits = 0;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) bits |= ((unsigned)(t0 + kk) < (unsigned)T_in) ? (1 << kk) : 0;
    return bits;
}
// Output row m of an implicit-im2col conv (GemmDesc::conv == 1) reads its taps from consecutive source rows: row0 = the row of tap 0 (may
// lie outside the sequence), bit kk of bits = tap kk lies inside it.  From the ragged row map (GemmDesc::rowmap) where there is one, else
// from the uniform geometry: m = (sequence rr, step to), t0 = to * stride - pad.  `g` is any args struct with rowmap, T_in, T_out, stride, pad.
__device__ __forceinline__ void conv_window_map(const int2* rowmap, int m, long long& row0, int& bits) {
    const int2 rm = rowmap[m];
    row0 = rm.x;
    bits = rm.y;
}
template <class G>
__device__ __forceinline__ void conv_window_geom(const G& g, int m, long long& row0, int& bits) {
    const int rr = m / g.T_out, to = m - rr * g.T_out;
    const int t0 = to * g.stride - g.pad;
    row0 = (long long)rr * g.T_in + t0;
    bits = conv_tap_bits(t0, g.T_in);
}
template <class G>
__device__ __forceinline__ void conv_window(const G& g, int m, long long& row0, int& bits) {
    if (g.rowmap) conv_window_map(g.rowmap, m, row0, bits);
    else conv_window_geom(g, m, row0, bits);
}

// ---- device: tile order ------------------------------------------------------------------------------------------------------------
// id -> (row tile rt, column index c) over g.tiles_n columns per row tile.  Consecutive ids run on different XCDs (id % 8): with
// g.xcd_remap the ids of one XCD walk the columns of a row tile back to back, so the row panel of A is fetched into ONE L2 (the host's
// xcd_remap_rows says when the row tiles split evenly over the XCDs).  `g` is the kernel's args struct (one tile per block: the columns are
// its column tiles) or a TileGrid (persistent kernels: problems and k ranges are further columns, below).  The two members are
// read inside the branches, as the written-out forms did: handed over by value the kernel arguments are loaded in front of the branch
// and every kernel's prologue changes (profiles/gemm_common_isa.txt).
struct TileGrid { int tiles_n, xcd_remap; };
template <class G>
__device__ __forceinline__ void tile_decode(const G& g, int id, int& rt, int& c) {
    if (g.xcd_remap) {
        const int x = id & 7, j = id >> 3;
        rt = x + 8 * (j / g.tiles_n);
        c = j % g.tiles_n;
    } else {
        rt = id / g.tiles_n;
        c = id % g.tiles_n;
    }
}
// The persistent kernels' columns c are composite - column tile innermost, then the problems of the launch (q/k/v projections of the same
// rows), then the k ranges of a split-K launch as further "problems": zz = c / tiles_n, problem z = zz / ks_n, k range ks = zz % ks_n, column
// tile = c % tiles_n.  That rule is written at its three sites (the persistent split kernel and the ping-pong experiment, which keep their
// whole decode local, and gemm_f32p.hip, which has no k ranges): as a helper here it moved scalar instructions in all of them
// (profiles/gemm_common_isa.txt).

// ---- device: the DMA piece layout of the direct-to-LDS kernels ------------------------------------------------------------------------
// A 1-KiB piece is 8 tile rows of 128 bytes: lane -> (row = lane / 8, physical 16-byte chunk = lane % 8).  The DMA writes LDS linearly, so
// the bank-conflict swizzle is applied to the SOURCE: the logical chunk that must land in physical slot `chunk` of tile row r is
// chunk ^ ((r >> 1) & 7) (the fragment reads apply the same involution).  Rows beyond the matrix are clamped to its last row: their
// products only reach outputs no epilogue stores.
__device__ __forceinline__ int dma_lane_row(int lane) { return lane >> 3; }
__device__ __forceinline__ int dma_lane_chunk(int lane) { return lane & 7; }
__device__ __forceinline__ int dma_src_chunk_bytes(int chunk, int r) { return (chunk ^ ((r >> 1) & 7)) * 16; }
__device__ __forceinline__ int dma_clamp_row(int row, int rows) { return min(row, rows - 1); }

// ---- host ------------------------------------------------------------------------------------------------------------------------------
// the XCD remap of tile_decode applies when the row tiles split evenly over the eight XCDs
inline int xcd_remap_rows(int tiles_m) { return tiles_m % 8 == 0 ? 1 : 0; }

// The fields every GEMM args struct has under the same name: the problems (unused slots repeat problem 0), sizes and pitches, the conv
// geometry and the row-map rule (the map is only looked at by the window gather, conv == 1).  Every launcher starts from it.
template <class A, class D>
void gemm_fill_conv(A& a, const D& d) {  // (also from a GemmTnDesc: the weight-gradient kernels gather the same windows)
    a.conv = d.conv; a.T_in = d.T_in; a.T_out = d.T_out; a.stride = d.stride; a.pad = d.pad; a.Cin = d.Cin;
    a.rowmap = d.conv == 1 ? d.rowmap : nullptr;
}
template <class A>
void gemm_fill_common(A& a, const GemmDesc& d) {
    for (int i = 0; i < 3; ++i) a.p[i] = d.p[i < d.nprob ? i : 0];
    a.M = d.M; a.N = d.N; a.K = d.K; a.lda = d.lda; a.ldr = d.ldr; a.ldc = d.ldc;
    gemm_fill_conv(a, d);
}
