// Every format conversion of an f32 matrix, and the statistics passes that go with them.
// f32 -> "split-f16" for the 3 x f16-MFMA GEMM path (gemm.hip, ARITH 1):
// Every aligned group of 8 consecutive f32 values x[0..7] of a row becomes, in the SAME 32 bytes,
//   [ f16 hi[0..7] | f16 lo[0..7] ],  hi = f16(s*x), lo = f16(s*x - hi)         (s = a power of two, exact)
// so hi + lo carries 22 significant bits of s*x.  The weight matrices are pre-scaled (s = 64: |w| <= 1/32 would put
// the lo halves in the f16 subnormal range) and the GEMM epilogue multiplies the result by 1/s.
// HBM-bound streaming kernels: one thread per 8-element block (two 16-byte loads, two 16-byte stores).
// f32 -> plain f16 / bfloat16 rows (the 16-bit storage modes); max|x| and 64-row slab column sums of a gradient matrix (its scale and its
// bias gradients from one read); the transposing forms of both casts (cast_sp16_t_kernel: the operands of gemm_tn_split.hip's
// transposed-copy route; transpose_cast_kernel: W -> W^T for the dX GEMMs).
#include <algorithm>

#include "kernels.h"

namespace {

template <int N>
using halfN = _Float16 __attribute__((ext_vector_type(N)));

// The block layout, written once: N scaled values of one 8-value block -> their hi halves at `blk`, their lo halves 16 bytes behind.
// N = 8: the whole block [hi8 | lo8]; N = 4: the half block a thread of cast_sp16_t_kernel's row-major copy owns (blk = the block's
// byte 0 or 8).  Returns the hi halves - the plain f16 cast of the same values.
template <int N>
__device__ __forceinline__ halfN<N> store_sp16(const float (&v)[N], void* blk) {
    halfN<N> hi, lo;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        _Float16 h1, l1;
        split_f16(v[j], h1, l1);
        hi[j] = h1; lo[j] = l1;
    }
    *reinterpret_cast<halfN<N>*>(blk) = hi;
    *reinterpret_cast<halfN<N>*>(static_cast<char*>(blk) + 16) = lo;
    return hi;
}
// eight consecutive f32 values times the scale
__device__ __forceinline__ void load8_scaled(const float* p, float scale, float (&v)[8]) {
    const float4 v0 = *reinterpret_cast<const float4*>(p);
    const float4 v1 = *reinterpret_cast<const float4*>(p + 4);
    v[0] = v0.x * scale; v[1] = v0.y * scale; v[2] = v0.z * scale; v[3] = v0.w * scale;
    v[4] = v1.x * scale; v[5] = v1.y * scale; v[6] = v1.z * scale; v[7] = v1.w * scale;
}
__device__ __forceinline__ void cast_sp16_block(const float* in8, float scale, float* out8) {
    float v[8];
    load8_scaled(in8, scale, v);
    store_sp16<8>(v, out8);
}

// scale = 2^(13 - floor(log2(amax))): the largest magnitude lands in [2^13, 2^14), far from the f16 overflow at 65504
__device__ __forceinline__ float auto_scale(unsigned amax_bits, int target = 13) {
    const int e = (int)(amax_bits >> 23) - 127;  // floor(log2(amax)) for normal floats
    if (amax_bits == 0u) return 1.f;
    const int k = min(max(target - e, -100), 100);
    return __uint_as_float((unsigned)(k + 127) << 23);
}

// AUTO: the scale comes from the amax slot scal[0] (its inverse goes to scal[1] for the GEMM's out_scale_dev), else from the argument
// side (optional): the hi halves once more as plain f16 rows [rows][8 * blocks_per_row] - the plain f16 cast of the same values (the
// split-f16 training forward leaves it for the backward's weight-gradient products: SolaCtx::x16)
template <bool AUTO>
__global__ __launch_bounds__(256) void cast_sp16_kernel(const float* __restrict__ in, float* __restrict__ out, long long rows,
                                                        int blocks_per_row, int ld_in, int ld_out, float scale, float* __restrict__ scal,
                                                        _Float16* __restrict__ side) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (AUTO) {
        scale = auto_scale(reinterpret_cast<const unsigned*>(scal)[0]);
        if (i == 0) scal[1] = 1.f / scale;
    }
    if (i >= rows * blocks_per_row) return;
    const long long r = i / blocks_per_row;
    const int b = (int)(i - r * blocks_per_row);
    float v[8];
    load8_scaled(in + r * ld_in + b * 8, scale, v);
    const half8 hi = store_sp16<8>(v, out + r * ld_out + b * 8);
    if (side) *reinterpret_cast<half8*>(side + (r * blocks_per_row + b) * 8) = hi;
}

// block-wide max -> ONE atomic per block (a launch over 0.5 GB has 65 K blocks: an atomic per wave queued 260 K updates on one
// address and took as long as the read itself)
__device__ __forceinline__ void block_amax_commit(float m, unsigned* out) {
    __shared__ float bmax[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) bmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(bmax[0], bmax[1]), fmaxf(bmax[2], bmax[3]));
        if (m > 0.f && m <= 3.0e38f) atomicMax(out, __float_as_uint(m));
    }
}

// max |x| of a strided matrix as float bits (non-negative floats order like their bit patterns).  A thread owns one float4
// column of a 64-row slab: coalesced row reads, no index arithmetic in the loop, one atomic per wave.
// SUMS: also leaves the column sums of every 64-row slab in part[slab][cols] (bias gradients: the second, tiny pass over the slabs
// is colsum_kernel's) - the gradient matrix is read once for both.
template <bool SUMS>
__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ in, unsigned* __restrict__ out, float* __restrict__ part,
                                                   long long rows, int f4_per_row, int ld_in) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    float m = 0.f;
    if (c < f4_per_row) {
        const long long r0 = (long long)blockIdx.y * 64;
        const int nr = (int)min((long long)64, rows - r0);
        const float* p = in + r0 * ld_in + (long long)c * 4;
        float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
        for (int r = 0; r < nr; ++r, p += ld_in) {
            const float4 v = *reinterpret_cast<const float4*>(p);
            m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
            if (SUMS) { sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w; }
        }
        if (SUMS) *reinterpret_cast<float4*>(part + ((long long)blockIdx.y * f4_per_row + c) * 4) = sum;
    }
    block_amax_commit(m, out);
}

// The two bf16 slab kernels: a wave owns one 64-row slab x 64 column groups (of 4 or 8 values); the scale slot reads {2^13, 1}, and
// auto_scale() of it is 1 for every later consumer.  nr = the slab's rows for this lane, <= 0 outside the matrix.
struct SlabLane {
    int c;           // column group
    long long slab;
    long long r0;    // first row
    int nr;
};
__device__ __forceinline__ SlabLane bf16_slab_lane(float* __restrict__ scal, long long rows, int groups_per_row) {
    SlabLane l;
    l.c = blockIdx.x * 64 + (threadIdx.x & 63);
    l.slab = (long long)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        scal[0] = 8192.f;
        scal[1] = 1.f;
    }
    l.r0 = l.slab * 64;
    l.nr = l.c < groups_per_row ? (int)min((long long)64, rows - l.r0) : 0;
    return l;
}

// bf16 storage mode (round 5): bfloat16 has f32's exponent range, so the gradient cast needs no data-dependent scale - and no max|x|
// pass in front of it.  ONE read of the gradient matrix leaves its row-major bf16 cast (the operand of the dW and dX GEMMs) and
// the 64-row slab column sums amax_kernel<true> leaves (same slabs, same order: the bias gradients keep their bits).
typedef __bf16 bf16x4c __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void cast_bf16_colsum_kernel(const float* __restrict__ in, __bf16* __restrict__ out, float* __restrict__ scal,
                                                               float* __restrict__ part, long long rows, int f4_per_row, int ld_in, int ld_out) {
    const SlabLane l = bf16_slab_lane(scal, rows, f4_per_row);
    if (l.nr <= 0) return;
    const float* p = in + l.r0 * ld_in + (long long)l.c * 4;
    __bf16* o = out + l.r0 * ld_out + (long long)l.c * 4;
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
    for (int r = 0; r < l.nr; ++r, p += ld_in, o += ld_out) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
        bf16x4c b;
        b[0] = (__bf16)v.x; b[1] = (__bf16)v.y; b[2] = (__bf16)v.z; b[3] = (__bf16)v.w;
        *reinterpret_cast<bf16x4c*>(o) = b;
    }
    *reinterpret_cast<float4*>(part + (l.slab * f4_per_row + l.c) * 4) = sum;
}

// Round 6 (bf16 storage of the step's gradients): the producer - the attention backward, a GroupNorm backward - has already written the
// bfloat16 matrix; what is left of the statistics pass is the 64-row slab column sums (the bias gradients), read from the 2-byte rows: a
// third of cast_bf16_colsum_kernel's bytes.  A lane owns eight columns (16 bytes per row).
__global__ __launch_bounds__(256) void colsum_slabs_bf16_kernel(const unsigned short* __restrict__ in, float* __restrict__ scal, float* __restrict__ part,
                                                                long long rows, int c8_per_row, int ld_in) {
    const SlabLane l = bf16_slab_lane(scal, rows, c8_per_row);
    if (l.nr <= 0) return;
    const unsigned short* p = in + l.r0 * ld_in + (long long)l.c * 8;
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;  // columns 0-3 and 4-7
#pragma unroll 8
    for (int r = 0; r < l.nr; ++r, p += ld_in) {
        const uint4 w = *reinterpret_cast<const uint4*>(p);
        const float4 a = bf16x4_to_f32(make_uint2(w.x, w.y)), b = bf16x4_to_f32(make_uint2(w.z, w.w));
        lo.x += a.x; lo.y += a.y; lo.z += a.z; lo.w += a.w;
        hi.x += b.x; hi.y += b.y; hi.z += b.z; hi.w += b.w;
    }
    float* o = part + (l.slab * c8_per_row + l.c) * 8;
    *reinterpret_cast<float4*>(o) = lo;
    *reinterpret_cast<float4*>(o + 4) = hi;
}

// ---- the same pair of passes for a set of equally shaped matrices (the 12 * n_layers projection weights): blockIdx.z picks
//      the matrix, its scale pair sits at scal + 2 * z
constexpr int MULTI_MAX = 64;
struct MultiArgs {
    const float* in[MULTI_MAX];
    float* out[MULTI_MAX];
};
__global__ __launch_bounds__(256) void amax_multi_kernel(const MultiArgs a, unsigned* __restrict__ scal, long long n4) {
    const float* in = a.in[blockIdx.z];
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 v = *reinterpret_cast<const float4*>(in + i * 4);
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    block_amax_commit(m, scal + 2 * blockIdx.z);
}
__global__ __launch_bounds__(256) void cast_sp16_auto_multi_kernel(const MultiArgs a, float* __restrict__ scal, long long n8) {
    const float* in = a.in[blockIdx.z];
    float* out = a.out[blockIdx.z];
    float* sc = scal + 2 * blockIdx.z;
    const float scale = auto_scale(reinterpret_cast<const unsigned*>(sc)[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) sc[1] = 1.f / scale;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) cast_sp16_block(in + i * 8, scale, out + i * 8);
}

// ---- cast_sp16_kernel for a set of matrices of DIFFERENT shapes and pitches under one fixed scale (the conv weights): blockIdx.y
//      picks the job, its blocks stride over the job's 8-value groups (a small job's surplus blocks leave at once)
struct CastJobs {
    CastJob j[CAST_JOBS_MAX];
};
__global__ __launch_bounds__(256) void cast_sp16_multi_kernel(const CastJobs a, float scale) {
    const CastJob jb = a.j[blockIdx.y];
    const int blocks_per_row = jb.K / 8;
    const long long n = (long long)jb.rows * blocks_per_row;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long r = i / blocks_per_row;
        const int b = (int)(i - r * blocks_per_row);
        cast_sp16_block(jb.in + r * jb.ld_in + b * 8, scale, jb.out + r * jb.ld_out + b * 8);
    }
}

// ---- f32 -> plain f16 rows (the 16-bit storage mode): 8 values per thread, 16-byte stores --------------------------------
// eight scaled f32 values -> eight 16-bit values: f16, or (bf) bfloat16 - both round to nearest even; the bits travel as a half8
typedef __bf16 bf16x8c __attribute__((ext_vector_type(8)));
__device__ __forceinline__ half8 cvt16x8(const float* in8, float scale, int bf) {
    float x[8];
    load8_scaled(in8, scale, x);
    if (bf) {
        bf16x8c b;
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = (__bf16)x[j];
        return __builtin_bit_cast(half8, b);
    }
    half8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = (_Float16)x[j];
    return h;
}

// SCALED: the power-of-two scale comes from the amax slot (auto_scale), else from the argument
template <bool SCALED>
__global__ __launch_bounds__(256) void cast_f16_kernel(const float* __restrict__ in, _Float16* __restrict__ out, long long rows,
                                                       int blocks_per_row, int ld_in, int ld_out, float scale_arg, float* __restrict__ scal,
                                                       int target, float* __restrict__ scale_out, int bf) {
    float scale = scale_arg;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (SCALED) {
        // scale_arg > 0 caps the data-dependent scale (an output kept in the scaled units also carries scale * bias)
        scale = auto_scale(reinterpret_cast<const unsigned*>(scal)[0], target);
        if (scale_arg > 0.f) scale = fminf(scale, scale_arg);
        if (i == 0) {
            scal[1] = 1.f / scale;
            if (scale_out) *scale_out = scale;
        }
    }
    if (i >= rows * blocks_per_row) return;
    const long long r = i / blocks_per_row;
    const int b = (int)(i - r * blocks_per_row);
    *reinterpret_cast<half8*>(out + r * ld_out + b * 8) = cvt16x8(in + r * ld_in + b * 8, scale, bf);
}
__global__ __launch_bounds__(256) void cast_f16_auto_multi_kernel(const MultiArgs a, float* __restrict__ scal, long long n8, int bf) {
    const float* in = a.in[blockIdx.z];
    _Float16* out = reinterpret_cast<_Float16*>(a.out[blockIdx.z]);
    float* sc = scal + 2 * blockIdx.z;
    const float scale = auto_scale(reinterpret_cast<const unsigned*>(sc)[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) sc[1] = 1.f / scale;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256)
        *reinterpret_cast<half8*>(out + i * 8) = cvt16x8(in + i * 8, scale, bf);
}

// in [rows][cols] f32 (pitch ld_in) -> out [cols][ld_out] split-f16, out[c][8b..8b+7] = scale * in[8b..8b+7][c]; rows beyond
// `rows` up to ld_out are written as zeros.  Tile = 128 rows x 64 columns through LDS.
// With rowmap != null (ragged batches) row m reads source row rowmap[m].x + tap, zeros where bit `tap` of rowmap[m].y is clear.
// With conv_T_out > 0 the input is the implicit im2col of a channels-last conv for ONE tap: row m = (r, to) reads source row
// r * conv_T_in + to * conv_stride + conv_toff (tap - pad), zeros outside [0, conv_T_in).
// PURE: the output is plain _Float16 ([cols][ld_out halfs]) for the one-MFMA-per-product GEMM (GemmDesc::ab F16 / BF16); bf != 0: the
// 16-bit values are bfloat16 bit patterns instead.
// RMP: the format of the optional row-major copy (PURE = as the transposed output; false with PURE = true: the weight-gradient
// product takes plain f16 operands while the dX GEMM of the same gradient matrix keeps split-f16 ones - sola_tune "train_dw_f16")
template <bool PURE, bool RMP = PURE>
__global__ __launch_bounds__(256) void cast_sp16_t_kernel(const float* __restrict__ in, float* __restrict__ out, int rows, int cols,
                                                          int ld_in, long long ld_out, float* __restrict__ scal, int conv_T_in,
                                                          int conv_T_out, int conv_stride, int conv_toff, float* __restrict__ out_rm,
                                                          long long ld_rm, const int2* __restrict__ rowmap, int tap, int bf) {
    __shared__ float tile[128][65];
    const int t = threadIdx.x;
    const int r0 = blockIdx.x * 128, c0 = blockIdx.y * 64;
    float scale = 1.f;
    if (scal) {
        scale = auto_scale(reinterpret_cast<const unsigned*>(scal)[0]);
        if (blockIdx.x == 0 && blockIdx.y == 0 && t == 0) scal[1] = 1.f / scale;
    }
    {   // 16-byte loads when the pitch allows; LDS pitch 65: bank = (row + col) % 64, conflict-free for both phases
        const int c4 = (t & 15) * 4, rq = t >> 4;
        const bool vec = (ld_in & 3) == 0 && c0 + 64 <= cols;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = i * 16 + rq;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            long long src = r0 + r;
            bool ok = r0 + r < rows;
            if (rowmap && ok) {  // ragged batches: tap `tap` of output row m lives at source row rowmap[m].x + tap (GemmDesc::rowmap)
                const int2 rm = rowmap[r0 + r];
                ok = (rm.y >> tap) & 1;
                src = (long long)rm.x + tap;
            } else if (conv_T_out > 0 && ok) {
                const int m = r0 + r, rr = m / conv_T_out, tt = (m - rr * conv_T_out) * conv_stride + conv_toff;
                ok = (unsigned)tt < (unsigned)conv_T_in;
                src = (long long)rr * conv_T_in + tt;
            }
            if (ok) {
                const float* p = in + src * ld_in + c0 + c4;
                if (vec) {
                    const float4 q = *reinterpret_cast<const float4*>(p);
                    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c0 + c4 + e < cols) v[e] = p[e];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[r][c4 + e] = v[e] * scale;
            if (out_rm && r0 + r < rows) {  // the row-major cast of the same values (vec path guaranteed by the launcher)
                const long long col = c0 + c4;
                float sv[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) sv[e] = v[e] * scale;
                if (RMP) {
                    *reinterpret_cast<half4*>(reinterpret_cast<_Float16*>(out_rm) + (long long)(r0 + r) * ld_rm + col) = cvt16x4_out(sv, bf);
                } else {  // 8-value blocks [hi8 | lo8]: this thread owns half a block
                    store_sp16<4>(sv, reinterpret_cast<char*>(out_rm + (long long)(r0 + r) * ld_rm + (col & ~7ll)) + 8 * ((col >> 2) & 1));
                }
            }
        }
    }
    __syncthreads();
    // a lane owns (8-row block b, column cc) of an 8 x 8 patch: banks 8 b + cc + e are all different; 8 lanes write the 256
    // contiguous bytes of one output row
    const int lane = t & 63, wave = t >> 6;
    const int b8 = lane & 7, cc = lane >> 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = wave * 16 + cc + 8 * (j & 1), b = b8 + 8 * (j >> 1);
        if (c0 + c >= cols) continue;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = tile[8 * b + e][c];
        if (PURE) {
            half8 h;
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = cvt16(v[e], bf);
            *reinterpret_cast<half8*>(reinterpret_cast<_Float16*>(out) + (long long)(c0 + c) * ld_out + r0 + 8 * b) = h;
        } else {
            store_sp16<8>(v, out + (long long)(c0 + c) * ld_out + r0 + 8 * b);
        }
    }
}

// out row c (pitch ldo VALUES of format FMT) column col_off + r = in[r][c], 32x32 tiles through LDS.  F32: the plain transposition
// (W -> W^T), no scale.  Else the value is scaled and written straight in a GEMM operand format (SP16 = split-f16 pairs in 8-value
// blocks [hi8 | lo8]): one launch where the backward's dX GEMMs ran a transposition into an f32 buffer and a cast of that buffer (two
// launches per weight matrix and step).
template <Elem FMT>
__global__ __launch_bounds__(256) void transpose_cast_kernel(const float* __restrict__ in, void* __restrict__ out, int rows, int cols, int ldi,
                                                             int ldo, int col_off, float scale) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 8 * i, c = c0 + tx;
        if (r < rows && c < cols) tile[ty + 8 * i][tx] = in[(long long)r * ldi + c];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, r = r0 + tx;
        if (r >= rows || c >= cols) continue;
        const long long n = col_off + r;
        if (FMT == Elem::F32) {
            static_cast<float*>(out)[(long long)c * ldo + n] = tile[tx][ty + 8 * i];
            continue;
        }
        const float v = tile[tx][ty + 8 * i] * scale;
        if (FMT == Elem::SP16) {
            _Float16 hi, lo;
            split_f16(v, hi, lo);
            _Float16* blk = reinterpret_cast<_Float16*>(static_cast<float*>(out) + (long long)c * ldo + (n & ~7LL)) + (n & 7);
            blk[0] = hi;
            blk[8] = lo;
        } else if (FMT == Elem::F16) {
            static_cast<_Float16*>(out)[(long long)c * ldo + n] = (_Float16)v;
        } else {
            static_cast<__bf16*>(out)[(long long)c * ldo + n] = (__bf16)v;
        }
    }
}

// one block per GroupNorm: rms over the channels of sqrt(gamma^2 + beta^2) = the rms of that norm's output
constexpr int NORM_MAX = 32;
struct NormArgs {
    NormPair n[NORM_MAX];
};
__global__ __launch_bounds__(256) void norm_range_check_kernel(const NormArgs a, int* guard) {
    __shared__ float red[4];
    const NormPair np = a.n[blockIdx.x];
    float s = 0.f;
    for (int c = threadIdx.x; c < np.C; c += 256) s += np.gamma[c] * np.gamma[c] + np.beta[c] * np.beta[c];
    const float rms = sqrtf(block_sum_256(s, red) / (float)np.C);
    if (threadIdx.x == 0 && !(rms >= 0.015625f && rms <= 512.f)) atomicOr(guard, 2);
}


// what every row-major cast launcher asks of its matrices: whole 8-value blocks, 16-byte aligned rows
bool cast_args_ok(const void* in, const void* out, long long rows, int K, int ld_in, int ld_out) {
    return in && out && rows > 0 && K > 0 && K % 8 == 0 && ld_in % 4 == 0 && ld_out % 8 == 0;
}

// scal[0] = max(scal[0], max|in|), inside the caller's profiler scope.
// max|x| does not care about the matrix shape: contiguous rows narrower than 1024 values are re-cut into 1024-wide ones (amax_kernel
// gives a thread one float4 column of a 64-row slab, so a 256-wide matrix - the object tokens - kept 64 of a block's 256 threads busy:
// 74 us for 134 MB)
int amax_pass(const float* in, int ld, long long rows, int K, float* scal, hipStream_t s) {
    if (ld == K && K < 1024 && (rows * K) % 1024 == 0) {
        rows = rows * K / 1024;
        K = ld = 1024;
    }
    hipLaunchKernelGGL(amax_kernel<false>, dim3((unsigned)((K / 4 + 255) / 256), (unsigned)((rows + 63) / 64)), dim3(256), 0, s, in,
                       reinterpret_cast<unsigned*>(scal), (float*)nullptr, rows, K / 4, ld);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

// one launch of cast_sp16_kernel: the scale from the slot `scal` where there is one, else the argument
int cast_sp16_rows(const float* in, int ld_in, float* out, int ld_out, long long rows, int K, float scale, float* scal, void* side16, hipStream_t s) {
    const long long n = rows * (K / 8);
    hipLaunchKernelGGL(scal ? cast_sp16_kernel<true> : cast_sp16_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, rows, K / 8, ld_in,
                       ld_out, scale, scal, static_cast<_Float16*>(side16));
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int transpose_rows(const float* in, void* out, int rows, int cols, int ldi, int ldo, int col_off, float scale, Elem fmt, hipStream_t s) {
    const auto kernel = fmt == Elem::F32    ? transpose_cast_kernel<Elem::F32>
                        : fmt == Elem::SP16 ? transpose_cast_kernel<Elem::SP16>
                        : fmt == Elem::F16  ? transpose_cast_kernel<Elem::F16>
                                            : transpose_cast_kernel<Elem::BF16>;
    hipLaunchKernelGGL(kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0, s, in, out, rows, cols, ldi, ldo, col_off, scale);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

}  // namespace

int launch_cast_sp16_auto_multi(const float* const* in, float* const* out, int n, int rows, int K, float* scal, hipStream_t s) {
    SOLA_ARG(in && out && scal && n > 0 && rows > 0 && K > 0 && K % 8 == 0, "cast_sp16_auto_multi: n=%d rows=%d K=%d", n, rows, K);
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, 12.0 * n * rows * K);
    SOLA_HIP(hipMemsetAsync(scal, 0, (size_t)2 * n * sizeof(float), s));
    const long long elems = (long long)rows * K;
    const unsigned blocks = (unsigned)std::min<long long>(128, (elems / 8 + 255) / 256);
    for (int i0 = 0; i0 < n; i0 += MULTI_MAX) {
        const int nn = std::min(MULTI_MAX, n - i0);
        MultiArgs a;
        for (int i = 0; i < nn; ++i) { a.in[i] = in[i0 + i]; a.out[i] = out[i0 + i]; }
        for (int i = nn; i < MULTI_MAX; ++i) { a.in[i] = nullptr; a.out[i] = nullptr; }
        hipLaunchKernelGGL(amax_multi_kernel, dim3(blocks, 1, nn), dim3(256), 0, s, a, reinterpret_cast<unsigned*>(scal + 2 * i0), elems / 4);
        SOLA_LAUNCH_CHECK();
        hipLaunchKernelGGL(cast_sp16_auto_multi_kernel, dim3(blocks, 1, nn), dim3(256), 0, s, a, scal + 2 * i0, elems / 8);
        SOLA_LAUNCH_CHECK();
    }
    return SOLA_OK;
}

int launch_cast_f16(const float* in, int ld_in, void* out, int ld_out, long long rows, int K, float scale, float* scal, Elem fmt, hipStream_t s,
                    int target_exp, float* scale_out) {
    SOLA_ARG(cast_args_ok(in, out, rows, K, ld_in, ld_out) && is_row16(fmt), "cast_f16: K=%d ld_in=%d ld_out=%d (%s)", K, ld_in, ld_out, elem_name(fmt));
    const int bf16 = fmt == Elem::BF16;
    const long long n = rows * (K / 8);
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, (scal ? 10.0 : 6.0) * rows * K);
    if (scal) {
        SOLA_HIP(hipMemsetAsync(scal, 0, 2 * sizeof(float), s));
        // bfloat16 has f32's exponent range: no max|x| pass - the zeroed slot reads as "scale 1" (auto_scale(0)), the same bits as any
        // power-of-two scale would give, one read of the matrix less (round 6)
        if (!bf16) SOLA_TRY(amax_pass(in, ld_in, rows, K, scal, s));
        hipLaunchKernelGGL(cast_f16_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, static_cast<_Float16*>(out), rows, K / 8, ld_in, ld_out,
                           scale_out ? scale : 0.f, scal, target_exp, scale_out, bf16);
    } else {
        hipLaunchKernelGGL(cast_f16_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, static_cast<_Float16*>(out), rows, K / 8, ld_in, ld_out, scale, nullptr,
                           0, nullptr, bf16);
    }
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

// the cast half of launch_cast_f16 with a data-dependent scale: scal[0] already holds max|in| (launch_amax_colsum)
int launch_cast_f16_scaled(const float* in, int ld_in, void* out, int ld_out, long long rows, int K, float* scal, Elem fmt, hipStream_t s) {
    SOLA_ARG(cast_args_ok(in, out, rows, K, ld_in, ld_out) && scal && is_row16(fmt), "cast_f16_scaled: K=%d ld_in=%d ld_out=%d (%s)", K, ld_in, ld_out, elem_name(fmt));
    const int bf16 = fmt == Elem::BF16;
    const long long n = rows * (K / 8);
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, 6.0 * rows * K);
    hipLaunchKernelGGL(cast_f16_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, static_cast<_Float16*>(out), rows, K / 8, ld_in, ld_out,
                       0.f, scal, 13, nullptr, bf16);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_cast_f16_auto_multi(const float* const* in, void* const* out, int n, int rows, int K, float* scal, Elem fmt, hipStream_t s) {
    SOLA_ARG(in && out && scal && n > 0 && rows > 0 && K > 0 && K % 8 == 0 && is_row16(fmt), "cast_f16_auto_multi: n=%d rows=%d K=%d (%s)", n, rows, K, elem_name(fmt));
    const int bf16 = fmt == Elem::BF16;
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, 10.0 * n * rows * K);
    SOLA_HIP(hipMemsetAsync(scal, 0, (size_t)2 * n * sizeof(float), s));
    const long long elems = (long long)rows * K;
    const unsigned blocks = (unsigned)std::min<long long>(1024, (elems / 8 + 255) / 256);
    for (int i0 = 0; i0 < n; i0 += MULTI_MAX) {
        const int nn = std::min(MULTI_MAX, n - i0);
        MultiArgs a;
        for (int i = 0; i < MULTI_MAX; ++i) { a.in[i] = i < nn ? in[i0 + i] : nullptr; a.out[i] = i < nn ? static_cast<float*>(out[i0 + i]) : nullptr; }
        if (!bf16) {  // bfloat16: scale 1 (the zeroed slots), no max|x| pass over the matrices
            hipLaunchKernelGGL(amax_multi_kernel, dim3(blocks, 1, nn), dim3(256), 0, s, a, reinterpret_cast<unsigned*>(scal + 2 * i0), elems / 4);
            SOLA_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(cast_f16_auto_multi_kernel, dim3(blocks, 1, nn), dim3(256), 0, s, a, scal + 2 * i0, elems / 8, bf16);
        SOLA_LAUNCH_CHECK();
    }
    return SOLA_OK;
}

int launch_norm_range_check(const NormPair* norms, int n, int* guard, hipStream_t s) {
    SOLA_ARG(norms && guard && n > 0 && n <= NORM_MAX, "norm_range_check: n=%d (1..%d)", n, NORM_MAX);
    NormArgs a;
    for (int i = 0; i < NORM_MAX; ++i) a.n[i] = norms[i < n ? i : 0];
    hipLaunchKernelGGL(norm_range_check_kernel, dim3(n), dim3(256), 0, s, a, guard);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_amax_accumulate(const float* in, int ld_in, long long rows, int K, float* scal, hipStream_t s) {
    SOLA_ARG(in && scal && rows > 0 && K > 0 && K % 4 == 0 && ld_in % 4 == 0, "amax: K=%d ld_in=%d", K, ld_in);
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, 4.0 * rows * K);
    return amax_pass(in, ld_in, rows, K, scal, s);
}

int launch_amax_colsum(const float* in, int ld_in, long long rows, int K, float* scal, float* part, hipStream_t s) {
    SOLA_ARG(in && scal && part && rows > 0 && K > 0 && K % 4 == 0 && ld_in % 4 == 0, "amax_colsum: K=%d ld_in=%d", K, ld_in);
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, 4.0 * rows * K);
    hipLaunchKernelGGL(amax_kernel<true>, dim3((unsigned)((K / 4 + 255) / 256), (unsigned)((rows + 63) / 64)), dim3(256), 0, s, in,
                       reinterpret_cast<unsigned*>(scal), part, rows, K / 4, ld_in);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_cast_bf16_colsum(const float* in, int ld_in, void* out, int ld_out, long long rows, int K, float* scal, float* part, hipStream_t s) {
    SOLA_ARG(in && out && scal && part && rows > 0 && K > 0 && K % 4 == 0 && ld_in % 4 == 0 && ld_out % 4 == 0 && ld_out >= K,
             "cast_bf16_colsum: K=%d ld_in=%d ld_out=%d", K, ld_in, ld_out);
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, 6.0 * rows * K);
    const long long slabs = (rows + 63) / 64;
    hipLaunchKernelGGL(cast_bf16_colsum_kernel, dim3((unsigned)((K / 4 + 63) / 64), (unsigned)((slabs + 3) / 4)), dim3(256), 0, s, in,
                       reinterpret_cast<__bf16*>(out), scal, part, rows, K / 4, ld_in, ld_out);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_colsum_slabs_bf16(const void* in, int ld_in, long long rows, int K, float* scal, float* part, hipStream_t s) {
    SOLA_ARG(in && scal && part && rows > 0 && K > 0 && K % 8 == 0 && ld_in % 8 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0, "colsum_slabs_bf16: K=%d ld_in=%d", K, ld_in);
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, 2.0 * rows * K);
    const long long slabs = (rows + 63) / 64;
    hipLaunchKernelGGL(colsum_slabs_bf16_kernel, dim3((unsigned)((K / 8 + 63) / 64), (unsigned)((slabs + 3) / 4)), dim3(256), 0, s,
                       static_cast<const unsigned short*>(in), scal, part, rows, K / 8, ld_in);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_cast_sp16_scaled(const float* in, int ld_in, float* out, int ld_out, long long rows, int K, float* scal, hipStream_t s) {
    SOLA_ARG(cast_args_ok(in, out, rows, K, ld_in, ld_out) && scal, "cast_sp16_scaled: K=%d ld_in=%d ld_out=%d", K, ld_in, ld_out);
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, 8.0 * rows * K);
    return cast_sp16_rows(in, ld_in, out, ld_out, rows, K, 0.f, scal, nullptr, s);
}

int launch_cast_sp16_auto(const float* in, int ld_in, float* out, int ld_out, long long rows, int K, float* scal, hipStream_t s) {
    SOLA_ARG(cast_args_ok(in, out, rows, K, ld_in, ld_out) && scal, "cast_sp16_auto: K=%d ld_in=%d ld_out=%d", K, ld_in, ld_out);
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, 12.0 * rows * K);
    SOLA_HIP(hipMemsetAsync(scal, 0, 2 * sizeof(float), s));
    SOLA_TRY(amax_pass(in, ld_in, rows, K, scal, s));
    return cast_sp16_rows(in, ld_in, out, ld_out, rows, K, 0.f, scal, nullptr, s);
}

int launch_cast_sp16_multi(const CastJob* jobs, int n, float scale, hipStream_t s) {
    SOLA_ARG(jobs && n > 0 && n <= CAST_JOBS_MAX, "cast_sp16_multi: %d jobs (at most %d)", n, CAST_JOBS_MAX);
    CastJobs a;
    long long most = 0;
    double bytes = 0;
    for (int i = 0; i < n; ++i) {
        const CastJob& j = jobs[i];
        SOLA_ARG(cast_args_ok(j.in, j.out, j.rows, j.K, j.ld_in, j.ld_out), "cast_sp16_multi: job %d K=%d ld_in=%d ld_out=%d", i, j.K, j.ld_in, j.ld_out);
        a.j[i] = j;
        most = std::max(most, (long long)j.rows * (j.K / 8));
        bytes += 8.0 * j.rows * j.K;
    }
    for (int i = n; i < CAST_JOBS_MAX; ++i) a.j[i] = CastJob{nullptr, nullptr, 0, 8, 0, 0};
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, bytes);
    const unsigned blocks = (unsigned)std::min<long long>(2048, (most + 255) / 256);
    hipLaunchKernelGGL(cast_sp16_multi_kernel, dim3(blocks, (unsigned)n), dim3(256), 0, s, a, scale);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_cast_sp16(const float* in, int ld_in, float* out, int ld_out, long long rows, int K, float scale, hipStream_t s, void* side16) {
    SOLA_ARG(cast_args_ok(in, out, rows, K, ld_in, ld_out), "cast_sp16: K=%d ld_in=%d ld_out=%d", K, ld_in, ld_out);
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, (side16 ? 10.0 : 8.0) * rows * K);
    return cast_sp16_rows(in, ld_in, out, ld_out, rows, K, scale, nullptr, side16, s);
}

// ---- the transposing forms ---------------------------------------------------------------------------------------------------------
int cast_t(const CastTDesc& d, hipStream_t s) {
    const bool op16 = is_row16(d.ab);
    const bool rmp = op16 && d.rm_fmt != Elem::SP16;  // the row-major copy has the operands' 16-bit format
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, ((op16 ? 6.0 : 8.0) + (d.out_rm ? (rmp ? 2.0 : 4.0) : 0.0)) * d.rows * d.cols);
    const auto kernel = !op16 ? cast_sp16_t_kernel<false> : rmp ? cast_sp16_t_kernel<true> : cast_sp16_t_kernel<true, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(d.ld_out / 128), (unsigned)((d.cols + 63) / 64)), dim3(256), 0, s, d.in, d.out, d.rows, d.cols, d.ld_in, d.ld_out,
                       d.scal, d.conv_T_in, d.conv_T_out, d.conv_stride, d.conv_toff, d.out_rm, d.ld_rm, d.rowmap, d.tap, (int)(d.ab == Elem::BF16));
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_cast_sp16_t(const float* in, int ld_in, float* out, long long ld_out, int rows, int cols, float* scal, hipStream_t s) {
    SOLA_ARG(in && out && rows > 0 && cols > 0 && ld_out % 128 == 0 && ld_out >= rows, "cast_sp16_t: rows=%d ld_out=%lld", rows, ld_out);
    return cast_t(CastTDesc{Elem::SP16, in, ld_in, out, ld_out, rows, cols, scal}, s);
}

int launch_cast_f16_t(const float* in, int ld_in, void* out, long long ld_out, int rows, int cols, float* scal, Elem fmt, hipStream_t s) {
    SOLA_ARG(in && out && rows > 0 && cols > 0 && ld_out % 128 == 0 && ld_out >= rows && is_row16(fmt), "cast_f16_t: rows=%d ld_out=%lld (%s)", rows, ld_out, elem_name(fmt));
    return cast_t(CastTDesc{fmt, in, ld_in, static_cast<float*>(out), ld_out, rows, cols, scal}, s);
}

int launch_transpose(const float* in, float* out, int rows, int cols, int ldi, int ldo, int col_off, hipStream_t s) {
    SOLA_ARG(rows > 0 && cols > 0, "transpose: bad dims");
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, 8.0 * rows * cols);
    return transpose_rows(in, out, rows, cols, ldi, ldo, col_off, 1.f, Elem::F32, s);
}

int launch_transpose_cast(const float* in, void* out, int rows, int cols, int ldi, int ldo, int col_off, float scale, Elem fmt, hipStream_t s) {
    SOLA_ARG(in && out && rows > 0 && cols > 0 && fmt != Elem::F32 && (fmt != Elem::SP16 || ldo % 8 == 0), "transpose_cast: bad arguments (%s ldo %d)", elem_name(fmt), ldo);
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, (fmt == Elem::SP16 ? 8.0 : 6.0) * rows * cols);
    return transpose_rows(in, out, rows, cols, ldi, ldo, col_off, scale, fmt, s);
}
