// The fixed-order sums around the GEMMs (deterministic: no float atomics, every order of additions is written here once):
//   sum_slabs_kernel : C[n][k] = sum_s P[s][n][k], the split partial sums of gemm_tn.hip / gemm_tn_f32p.hip in index order
//   colsum_*_kernel  : out[seg][c] = sum_{r in segment} in[r][c]  (bias gradients, GroupNorm dgamma / dbeta, dlbar) - one launch for one
//                      matrix or a pair, for up to 16 pairs, for up to 48 jobs; all three sum a column in colsum_column()
//   col2im_*_kernel  : the scatter of a transposed conv as a gather over the taps, uniform or ragged batches
// HBM-bound streaming kernels.
#include <algorithm>
#include <utility>

#include "kernels.h"

namespace {

__global__ void sum_slabs_kernel(const float* __restrict__ P, float* __restrict__ C, long long n4, int splits) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 acc = reinterpret_cast<const float4*>(P)[i];
    for (int s = 1; s < splits; ++s) {
        const float4 v = reinterpret_cast<const float4*>(P)[i + (long long)s * n4];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    reinterpret_cast<float4*>(C)[i] = acc;
}

// One column of a block of 64 columns x 4 row lanes: lane rl sums rows r_begin + rl, + 4, ... < r_end of p[r * ld] (live = the column
// exists), the four lanes are folded through LDS; every thread returns its column's sum (the row lanes 0 write it).  The order is
// fixed - the bits of every bias and norm-parameter gradient are this function's.
// Eight independent partial sums, fixed combination order: a thread's loads pipeline instead of queueing behind one add chain (a
// [256][1024] bias pass took 16 us for 1 MB: 64 dependent load-add steps per thread; round 3: eight, not four - the 70 second-stage
// bias / norm-parameter reductions of a training step are ~200 dependent rows each)
__device__ __forceinline__ float colsum_column(const float* p, int ld, int r_begin, int r_end, int rl, bool live) {
    __shared__ float red[4][64];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f, s5 = 0.f, s6 = 0.f, s7 = 0.f;
    if (live) {
        int r = r_begin + rl;
        for (; r + 28 < r_end; r += 32) {
            s0 += p[(long long)r * ld]; s1 += p[(long long)(r + 4) * ld]; s2 += p[(long long)(r + 8) * ld]; s3 += p[(long long)(r + 12) * ld];
            s4 += p[(long long)(r + 16) * ld]; s5 += p[(long long)(r + 20) * ld]; s6 += p[(long long)(r + 24) * ld]; s7 += p[(long long)(r + 28) * ld];
        }
        for (; r < r_end; r += 4) s0 += p[(long long)r * ld];
    }
    const int cl = threadIdx.x & 63;
    red[rl][cl] = ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7));
    __syncthreads();
    return (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

// out[(chunk * segments + seg)][c] (+)= scale * sum_{r in chunk of segment} in[(seg * seg_rows + r)][c]
// grid.z splits long segments into row chunks (a second launch adds the chunks up)
// seg_stride: elements between the first rows of consecutive segments (seg_rows * ld for back-to-back segments).  out1 / split: output
// index >= split goes to out1[index - split] instead (two reductions with separate destinations in one launch: launch_colsum_pair).
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ in, float* __restrict__ out, int seg_rows,
                                                     int cols, int ld, int chunk_rows, float scale, int accumulate, long long seg_stride,
                                                     float* __restrict__ out1, long long split) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rl = threadIdx.x >> 6;
    const int seg = blockIdx.y;
    const int r_begin = blockIdx.z * chunk_rows;
    const float sum = colsum_column(in + (long long)seg * seg_stride + c, ld, r_begin, min(seg_rows, r_begin + chunk_rows), rl, c < cols);
    if (rl == 0 && c < cols) {
        const float v = sum * scale;
        const long long oi = ((long long)blockIdx.z * gridDim.y + seg) * cols + c;
        float* o = (out1 && oi >= split) ? out1 + (oi - split) : out + oi;
        *o = accumulate ? *o + v : v;
    }
}

// up to 16 (dgamma, dbeta) pairs of column sums in ONE launch (round 5, few-sample backward: the 11 GroupNorm backwards of a one-sample step
// each ended in a launch_colsum_pair of ~5 us; deferred - every norm keeps private partial buffers - they are one launch per bucket).
// One chunk per column: the bits of launch_colsum_pair on <= 256 rows.
constexpr int CSG_MAX = 16;
struct ColsumGroupArgs {
    const float* in0[CSG_MAX];
    const float* in1[CSG_MAX];
    float* out0[CSG_MAX];
    float* out1[CSG_MAX];
    int rows[CSG_MAX], cols[CSG_MAX], first_block[CSG_MAX + 1];
    int n;
};
__global__ __launch_bounds__(256) void colsum_pair_group_kernel(const ColsumGroupArgs a) {
    int e = 0;
    for (int j = 1; j < a.n; ++j)
        if ((int)blockIdx.x >= a.first_block[j]) e = j;
    const int lb = (int)blockIdx.x - a.first_block[e];
    const int cb = (a.cols[e] + 63) / 64;
    const int which = lb / cb;
    const int c = (lb - which * cb) * 64 + (threadIdx.x & 63);
    const int rl = threadIdx.x >> 6;
    const int cols = a.cols[e];
    const float sum = colsum_column((which ? a.in1[e] : a.in0[e]) + c, cols, 0, a.rows[e], rl, c < cols);
    if (rl == 0 && c < cols) (which ? a.out1[e] : a.out0[e])[c] = sum;
}

// Up to 48 single column sums in ONE launch (round 6: the ~30 bias gradients of a reduced-precision training step were one ~9-us launch each
// over the slab sums their statistics pass left; every statistics pass keeps its slab table now and a bucket's bias sums leave together).
// One chunk per column: the bits of launch_colsum without scratch.
constexpr int CSJ_MAX = 48;
struct ColsumJobsArgs {
    const float* in[CSJ_MAX];
    float* out[CSJ_MAX];
    int rows[CSJ_MAX], cols[CSJ_MAX], ld[CSJ_MAX], first_block[CSJ_MAX + 1];
    int n;
};
__global__ __launch_bounds__(256) void colsum_jobs_kernel(const ColsumJobsArgs a) {
    int lo = 0, hi = a.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.first_block[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const int e = lo;
    const int c = ((int)blockIdx.x - a.first_block[e]) * 64 + (threadIdx.x & 63);
    const int rl = threadIdx.x >> 6;
    const float sum = colsum_column(a.in[e] + c, a.ld[e], 0, a.rows[e], rl, c < a.cols[e]);
    if (rl == 0 && c < a.cols[e]) a.out[e][c] = sum;
}

// Transposed-conv scatter as a gather: z [R*T_out][k*cin] holds, for every output step, its contribution to each of the k
// input steps it touches (z = dY W, one GEMM); dx[(r, ti)][ci] = sum over the taps kk with (ti + pad - kk) = to * stride,
// 0 <= to < T_out, of z[(r, to)][kk*cin + ci].  One thread per float4 of dx; fixed tap order.
// ZB (round 6, bf16 steps): z is a bfloat16 matrix of the same shape (the GEMM that produced it wrote bfloat16 rows); the taps are summed in f32
// col2im_quad: quad i of dx (channels c4 * 4 ..) is step ti of a sequence whose output rows are row0 .. row0 + T_out - 1 of z
template <bool ZB>
__device__ __forceinline__ void col2im_quad(const float* __restrict__ z, float* __restrict__ dx, long long i, int c4, long long row0, int T_out,
                                            int ti, int cin4, int k, int stride, int pad) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int kk = 0; kk < k; ++kk) {
        const int u = ti + pad - kk;
        if (u < 0 || u % stride) continue;
        const int to = u / stride;
        if (to >= T_out) continue;
        const long long off = ((row0 + to) * k + kk) * (long long)(cin4 * 4) + c4 * 4;
        const float4 v = ZB ? bf16x4_to_f32(*reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(z) + off))
                            : *reinterpret_cast<const float4*>(z + off);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    *reinterpret_cast<float4*>(dx + i * 4) = acc;
}
template <bool ZB>
__global__ __launch_bounds__(256) void col2im_kernel(const float* __restrict__ z, float* __restrict__ dx, long long n4, int T_in, int T_out,
                                                     int cin4, int k, int stride, int pad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const long long rt = i / cin4;
    col2im_quad<ZB>(z, dx, i, (int)(i % cin4), rt / T_in * T_out, T_out, (int)(rt % T_in), cin4, k, stride, pad);
}
// ragged batches: input row i of the conv has imap[i] = (first output row of its sequence, T_out, step ti, -)
template <bool ZB>
__global__ __launch_bounds__(256) void col2im_ragged_kernel(const float* __restrict__ z, float* __restrict__ dx, long long n4,
                                                            const int4* __restrict__ imap, int cin4, int k, int stride, int pad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int4 im = imap[i / cin4];
    col2im_quad<ZB>(z, dx, i, (int)(i % cin4), im.x, im.y, im.z, cin4, k, stride, pad);
}

// launch_colsum and launch_colsum_pair: `segments` column sums whose first rows lie seg_stride elements apart, in one launch - or, over
// more than 256 rows with scratch at hand, row chunks into the scratch and a second launch that adds the chunks up
int colsum_segments(const float* in, float* out, int segments, int seg_rows, int cols, int ld, float scale, int accumulate, long long seg_stride,
                    float* out1, long long split, float* scratch, size_t scratch_bytes, hipStream_t s) {
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, 4.0 * segments * (double)seg_rows * cols);
    const size_t need = colsum_scratch_bytes(segments, seg_rows, cols);
    if (need == 0 || scratch == nullptr || scratch_bytes < need) {
        hipLaunchKernelGGL(colsum_kernel, dim3((cols + 63) / 64, segments, 1), dim3(256), 0, s, in, out, seg_rows, cols, ld, seg_rows, scale, accumulate,
                           seg_stride, out1, split);
        SOLA_LAUNCH_CHECK();
        return SOLA_OK;
    }
    const int chunks = (int)(need / ((size_t)segments * cols * sizeof(float)));
    const int chunk_rows = (seg_rows + chunks - 1) / chunks;
    hipLaunchKernelGGL(colsum_kernel, dim3((cols + 63) / 64, segments, chunks), dim3(256), 0, s, in, scratch, seg_rows, cols, ld, chunk_rows, 1.0f, 0,
                       seg_stride, (float*)nullptr, 0LL);
    SOLA_LAUNCH_CHECK();
    const int wide = segments * cols;  // second pass: [chunks][segments*cols] -> [segments*cols]
    hipLaunchKernelGGL(colsum_kernel, dim3((wide + 63) / 64, 1, 1), dim3(256), 0, s, scratch, out, chunks, wide, wide, chunks, scale, accumulate,
                       (long long)chunks * wide, out1, split);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

}  // namespace

int sum_slabs(const float* P, float* C, long long n4, int splits, hipStream_t s) {
    hipLaunchKernelGGL(sum_slabs_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, P, C, n4, splits);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

size_t colsum_scratch_bytes(int segments, int seg_rows, int cols) {
    if (seg_rows <= 256) return 0;
    const int chunks = min(64, (seg_rows + 127) / 128);
    return (size_t)chunks * segments * cols * sizeof(float);
}

int launch_colsum(const float* in, float* out, int segments, int seg_rows, int cols, int ld, float scale, int accumulate,
                  float* scratch, size_t scratch_bytes, hipStream_t s) {
    SOLA_ARG(segments > 0 && seg_rows > 0 && cols > 0 && segments <= 65535, "colsum: bad dims");
    return colsum_segments(in, out, segments, seg_rows, cols, ld, scale, accumulate, (long long)seg_rows * ld, nullptr, 0, scratch, scratch_bytes, s);
}

// Two column sums of equally shaped matrices with separate destinations (GroupNorm's dgamma / dbeta partials): two segments in1 - in0
// apart, the second one's sums to out1
int launch_colsum_pair(const float* in0, const float* in1, float* out0, float* out1, int seg_rows, int cols, int ld, float* scratch,
                       size_t scratch_bytes, hipStream_t s) {
    SOLA_ARG(in0 && in1 && out0 && out1 && seg_rows > 0 && cols > 0, "colsum_pair: bad arguments");
    if (in1 < in0) { std::swap(in0, in1); std::swap(out0, out1); }
    return colsum_segments(in0, out0, 2, seg_rows, cols, ld, 1.0f, 0, in1 - in0, out1, cols, scratch, scratch_bytes, s);
}

int launch_colsum_pair_group(const ColsumPairGroupDesc& d, hipStream_t s) {
    SOLA_ARG(d.n >= 1 && d.n <= CSG_MAX, "colsum_pair_group: %d pairs", d.n);
    ColsumGroupArgs a;
    a.n = d.n;
    int blocks = 0;
    double bytes = 0;
    for (int e = 0; e < d.n; ++e) {
        SOLA_ARG(d.in0[e] && d.in1[e] && d.out0[e] && d.out1[e] && d.rows[e] > 0 && d.rows[e] <= 256 && d.cols[e] > 0, "colsum_pair_group: pair %d (rows %d)", e, d.rows[e]);
        a.in0[e] = d.in0[e]; a.in1[e] = d.in1[e]; a.out0[e] = d.out0[e]; a.out1[e] = d.out1[e]; a.rows[e] = d.rows[e]; a.cols[e] = d.cols[e];
        a.first_block[e] = blocks;
        blocks += 2 * ((d.cols[e] + 63) / 64);
        bytes += 8.0 * d.rows[e] * d.cols[e];
    }
    a.first_block[d.n] = blocks;
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, bytes);
    hipLaunchKernelGGL(colsum_pair_group_kernel, dim3(blocks), dim3(256), 0, s, a);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_colsum_jobs(const ColsumJobsDesc& d, hipStream_t s) {
    SOLA_ARG(d.n >= 1 && d.n <= CSJ_MAX, "colsum_jobs: %d jobs", d.n);
    ColsumJobsArgs a;
    a.n = d.n;
    int blocks = 0;
    double bytes = 0;
    for (int e = 0; e < d.n; ++e) {
        SOLA_ARG(d.in[e] && d.out[e] && d.rows[e] > 0 && d.cols[e] > 0 && d.ld[e] >= d.cols[e], "colsum_jobs: job %d", e);
        a.in[e] = d.in[e]; a.out[e] = d.out[e]; a.rows[e] = d.rows[e]; a.cols[e] = d.cols[e]; a.ld[e] = d.ld[e];
        a.first_block[e] = blocks;
        blocks += (d.cols[e] + 63) / 64;
        bytes += 4.0 * d.rows[e] * d.cols[e];
    }
    a.first_block[d.n] = blocks;
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, bytes);
    hipLaunchKernelGGL(colsum_jobs_kernel, dim3(blocks), dim3(256), 0, s, a);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_col2im(const float* z, float* dx, long long R, int T_in, int T_out, int cin, int k, int stride, int pad, Elem z_fmt, hipStream_t s) {
    const bool z16 = z_fmt == Elem::BF16;
    SOLA_ARG(z && dx && cin % 4 == 0 && k >= 1 && stride >= 1 && (z16 || z_fmt == Elem::F32), "col2im: cin=%d k=%d stride=%d", cin, k, stride);
    const long long n4 = R * T_in * (cin / 4);
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, (z16 ? 2.0 : 4.0) * R * T_out * (double)k * cin + 4.0 * R * T_in * (double)cin);
    hipLaunchKernelGGL(z16 ? col2im_kernel<true> : col2im_kernel<false>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, z, dx, n4, T_in, T_out, cin / 4, k,
                       stride, pad);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_col2im_ragged(const float* z, float* dx, long long rows_in, const int4* imap, int cin, int k, int stride, int pad, Elem z_fmt, hipStream_t s) {
    const bool z16 = z_fmt == Elem::BF16;
    SOLA_ARG(z && dx && imap && cin % 4 == 0 && k >= 1 && stride >= 1 && rows_in > 0 && (z16 || z_fmt == Elem::F32), "col2im_ragged: cin=%d k=%d stride=%d", cin, k, stride);
    const long long n4 = rows_in * (cin / 4);
    SolaProfScope prof(SOLA_PROF_MISC, s, 0, (z16 ? 2.0 : 4.0) * rows_in * (double)k * cin / stride + 4.0 * rows_in * (double)cin);
    hipLaunchKernelGGL(z16 ? col2im_ragged_kernel<true> : col2im_ragged_kernel<false>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, z, dx, n4, imap,
                       cin / 4, k, stride, pad);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}
