// Weight gradients dW[n][k] = sum_m dY[m][n] X[m][k] on the split-f16 MFMA path (training, precision 1).
// The reduction runs over the ROWS of both operands, so each is first written transposed in the split-f16 format
// ([N][Mp] and [K][Mp], Mp = M rounded up and zero-filled) - one streaming pass that replaces the f32 kernel's strided
// staging - and the product is then the ordinary NT GEMM of gemm_glds.hip with the reduction dim = Mp.  dW has only
// (N/256) x (K/256) output tiles (16 for the 1024 x 1024 projections), so the reduction is cut into `ksplit` ranges,
// one persistent-kernel work item each, and gemm.hip's splitk_reduce_kernel folds the partial sums in a fixed order.
// dY is a gradient (entries ~1e-4..1e-9): it is scaled by a data-dependent power of two found on the device
// (cast.hip's amax pass; all problems of a launch share the scale), undone by the GEMM's out_scale_dev.  The transposing cast is
// cast.hip's cast_t; the col2im gather of the conv backward is reduce.hip's.
// Second route (round 3, the default for 16-bit operands - GemmTnSplitDesc::ab F16 / BF16 - when N and K are multiples of 256): NO transposed
// copies.  The operands are cast ROW-MAJOR (dY's cast is the dX GEMM's operand anyway, X's comes from the training forward's kept
// casts or one plain cast; convs: one cast of the conv input) and gemm_tn_tr.hip's gemm_tn_tr_kernel transposes them in its LDS reads.
#include <algorithm>

#include "kernels.h"

namespace {

void geometry(int M, int& ksplit, long long& Mp, bool op16 = false) {
    ksplit = M >= 8192 ? 16 : (M >= 2048 ? 8 : (M >= 512 ? 4 : 2));
    // every range at least two k-tiles (32 pairs or 64 halfs wide); a multiple of the 128-row cast tile
    const long long q = (op16 ? 128LL : 64LL) * ksplit;
    Mp = (M + q - 1) / q * q;
}

}  // namespace

bool gemm_tn_split_supported(int M, int N, int K) { return N % 8 == 0 && K % 8 == 0 && M >= 64; }

// the row-major copy is written by the 16-byte-load path of the cast only: whole 64-column tiles, aligned slices
bool gemm_tn_split_writes_rm(const GemmTnSplitDesc& d) {
    if (!d.a_rm || d.N % 64 != 0 || d.lda % 4 != 0 || d.a_rm_ld % 8 != 0) return false;
    for (int j = 0; j < d.nprob; ++j) {
        const long long off = d.A[j] - d.A[0];
        if (off < 0 || off % 8 != 0 || off + d.N > d.a_rm_ld) return false;
    }
    return true;
}

static long long conv_input_rows(const GemmTnSplitDesc& d) { return !d.conv ? 0 : (d.rowmap ? d.B_rows : (long long)d.M / d.T_out * d.T_in); }

bool gemm_tn_split_takes_tr(const GemmTnSplitDesc& d) {
    return is_row16(d.ab) && d.ldb % 4 == 0 && gemm_tn_tr_supported(d.M, d.N, d.K, 8, 8) &&
           (!d.conv || (d.Cin % 256 == 0 && d.ldb == d.Cin && conv_input_rows(d) > 0));
}

size_t gemm_tn_split_scratch_bytes(int M, int N, int K, int nprob) {
    int ks; long long Mp;
    geometry(M, ks, Mp, true);  // the f16-operand layout pads the rows further; sized for either
    const size_t el = (size_t)nprob * N * Mp + (size_t)nprob * K * Mp + (size_t)nprob * ks * N * K + 64;
    return el * sizeof(float);
}

int launch_gemm_tn_split(const GemmTnSplitDesc& d, hipStream_t s) {
    SOLA_ARG(d.nprob >= 1 && d.nprob <= 3 && d.scratch, "gemm_tn_split: nprob %d", d.nprob);
    SOLA_ARG(gemm_tn_split_supported(d.M, d.N, d.K) && d.lda % 4 == 0, "gemm_tn_split: M=%d N=%d K=%d lda=%d", d.M, d.N, d.K, d.lda);
    SOLA_ARG(!d.conv || (d.Cin > 0 && d.K % d.Cin == 0 && (d.rowmap || (d.T_out > 0 && d.M % d.T_out == 0))), "gemm_tn_split: conv geometry K=%d Cin=%d", d.K, d.Cin);
    SOLA_ARG(d.scratch_bytes >= gemm_tn_split_scratch_bytes(d.M, d.N, d.K, d.nprob), "gemm_tn_split: scratch too small");
    SOLA_ARG(gemm_tn_split_formats_ok(d.ab, d.rm_fmt, d.b16_fmt), "gemm_tn_split: %s operands with a %s row-major copy and %s kept rows", elem_name(d.ab),
             elem_name(d.rm_fmt), elem_name(d.b16_fmt));
    int ks; long long Mp;
    const bool op16 = is_row16(d.ab);
    const bool rm_sp = op16 && d.rm_fmt == Elem::SP16;  // the row-major copy stays split-f16 beside 16-bit operands
    const bool bf = d.ab == Elem::BF16;
    geometry(d.M, ks, Mp, op16);
    // transposed operands: rows of Mp split-f16 pairs (4 bytes per element) or Mp halfs (2 bytes); the buffers are sized for pairs
    const long long rowf = op16 ? Mp / 2 : Mp;  // floats per transposed row
    float* at = d.scratch;
    float* xt = at + (size_t)d.nprob * d.N * Mp;
    float* slabs = xt + (size_t)d.nprob * d.K * Mp;
    float* scal = d.scal ? d.scal : slabs + (size_t)d.nprob * ks * d.N * d.K;
    if (!d.scal) {  // one scale for all problems: the amax passes accumulate into the same slot
        SOLA_HIP(hipMemsetAsync(scal, 0, 2 * sizeof(float), s));
        for (int j = 0; j < d.nprob; ++j) SOLA_TRY(launch_amax_accumulate(d.A[j], d.lda, d.M, d.N, scal, s));
    }
    const bool rm = gemm_tn_split_writes_rm(d);
    const long long conv_rows_in = conv_input_rows(d);
    if (gemm_tn_split_takes_tr(d)) {
        // 16-bit operands, linear layers: NO transposed copies.  gemm_tn_tr.hip's gemm_tn_tr_kernel takes the ROW-MAJOR casts - dY's is the
        // dX GEMM's operand anyway - and transposes between LDS and the matrix pipe (ds_read_b64_tr_b16).
        GemmTnTrDesc t{};
        t.nprob = d.nprob; t.M = d.M; t.N = d.N; t.K = d.K;
        _Float16* a16 = reinterpret_cast<_Float16*>(at);
        _Float16* x16 = reinterpret_cast<_Float16*>(xt);
        const bool rm16 = rm && !rm_sp;  // the caller's row-major copy has the operand's format: cast once, into it
        // ... or it is the split-f16 copy (the dX GEMM of a split-f16 step): its hi halves ARE the plain f16 cast, the kernel fetches them
        const bool rmsp = rm && rm_sp && !bf;
        int n_x = 0;
        const bool b16_sp = d.b16_fmt == Elem::SP16;
        bool b_kept = !d.scal_b && !(b16_sp && bf);  // every problem's X comes from the forward's kept operand casts
        for (int j = 0; j < d.nprob; ++j) b_kept = b_kept && d.B16[j] != nullptr;
        for (int j = 0; j < d.nprob; ++j) {
            const long long off = d.A[j] - d.A[0];
            if (rm16) {
                _Float16* dst = reinterpret_cast<_Float16*>(d.a_rm) + off;
                if (!d.a_rm_ready) SOLA_TRY(launch_cast_f16_scaled(d.A[j], d.lda, dst, d.a_rm_ld, d.M, d.N, scal, d.ab, s));
                t.A[j] = dst;
            } else if (rmsp) {
                SOLA_TRY(launch_cast_sp16_scaled(d.A[j], d.lda, d.a_rm + off, d.a_rm_ld, d.M, d.N, scal, s));
                t.A[j] = d.a_rm + off;
            } else {
                _Float16* dst = a16 + (size_t)j * d.M * d.N;
                SOLA_TRY(launch_cast_f16_scaled(d.A[j], d.lda, dst, d.N, d.M, d.N, scal, d.ab, s));
                t.A[j] = dst;
                if (rm) SOLA_TRY(launch_cast_sp16_scaled(d.A[j], d.lda, d.a_rm + off, d.a_rm_ld, d.M, d.N, scal, s));  // the dX GEMM keeps split-f16 operands
            }
            t.B[j] = nullptr;
            for (int e = 0; e < j; ++e)
                if (d.B[e] == d.B[j]) t.B[j] = t.B[e];
            if (!t.B[j] && b_kept) t.B[j] = d.B16[j];  // the forward's operand cast of the same activation
            if (!t.B[j]) {
                // conv: ONE row-major cast of the conv input; the kernel gathers the taps (implicit im2col) in its DMA addresses
                const long long b_rows = d.conv ? conv_rows_in : d.M;
                const int b_cols = d.conv ? d.Cin : d.K;
                _Float16* dst = x16 + (size_t)n_x++ * b_rows * b_cols;
                if (d.scal_b) SOLA_TRY(launch_cast_f16_scaled(d.B[j], d.ldb, dst, b_cols, b_rows, b_cols, d.scal_b, d.ab, s));
                else SOLA_TRY(launch_cast_f16(d.B[j], d.ldb, dst, b_cols, b_rows, b_cols, 1.f, nullptr, d.ab, s));
                t.B[j] = dst;
            }
        }
        t.lda = (rm16 || rmsp) ? d.a_rm_ld : d.N;
        t.a_fmt = rmsp ? Elem::SP16 : d.ab;
        t.ldb = d.conv ? d.Cin : d.K;
        t.b_fmt = b_kept && b16_sp ? Elem::SP16 : d.ab;
        t.conv = d.conv; t.Cin = d.Cin; t.T_in = d.T_in; t.T_out = d.T_out; t.stride = d.stride; t.pad = d.pad; t.rowmap = d.rowmap;
        gemm_tn_tr_geometry(d.M, d.N, d.K, d.nprob, ks, t.ksplit, t.kper);
        t.part = slabs;
        // bf16 steps (train_bf16_store 3): the partial sums of the k ranges leave as bfloat16 slabs (half the bytes written by the 256 blocks
        // at once and read back by the fold); sixteen of them are summed in f32 - autocast's linear backward rounds the whole dW to bfloat16 once
        extern int g_train_bf16_store;
        t.part_fmt = (bf && g_train_bf16_store >= 3 && d.K % 4 == 0) ? Elem::BF16 : Elem::F32;
        SOLA_TRY(launch_gemm_tn_tr(t, s));
        if (t.part_fmt == Elem::BF16) return launch_splitk_reduce_bf16(slabs, t.ksplit, d.nprob, d.C, d.N, d.K, d.K, scal + 1, d.scal_b ? d.scal_b + 1 : nullptr, s);
        return launch_splitk_reduce(slabs, t.ksplit, d.nprob, d.C, d.N, d.K, d.K, scal + 1, d.scal_b ? d.scal_b + 1 : nullptr, s);
    }
    const float* xt_of[3] = {nullptr, nullptr, nullptr};
    int n_xt = 0;
    for (int j = 0; j < d.nprob; ++j) {
        CastTDesc ca{d.ab, d.A[j], d.lda, at + (size_t)j * d.N * rowf, Mp, d.M, d.N, scal};
        if (rm && !(d.a_rm_ready && op16 && !rm_sp)) {  // + the row-major cast of the same gradient matrix (the dX GEMM's operand): one read of dY for both
            const long long off = d.A[j] - d.A[0];
            ca.out_rm = (op16 && !rm_sp) ? reinterpret_cast<float*>(reinterpret_cast<_Float16*>(d.a_rm) + off) : d.a_rm + off;
            ca.ld_rm = d.a_rm_ld;
            ca.rm_fmt = d.rm_fmt;
        }
        SOLA_TRY(cast_t(ca, s));
        for (int e = 0; e < j; ++e)
            if (d.B[e] == d.B[j]) xt_of[j] = xt_of[e];
        if (!xt_of[j]) {
            float* dst = xt + (size_t)n_xt++ * d.K * rowf;
            CastTDesc cb{d.ab, d.B[j], d.ldb, dst, Mp, d.M, d.K, d.scal_b};
            if (d.conv) {  // rows [kk*Cin, (kk+1)*Cin) of X^T = tap kk of the implicit im2col
                cb.cols = d.Cin;
                cb.conv_T_in = d.T_in; cb.conv_T_out = d.T_out; cb.conv_stride = d.stride; cb.rowmap = d.rowmap;
                for (int kk = 0; kk < d.K / d.Cin; ++kk) {
                    cb.out = dst + (size_t)kk * d.Cin * rowf;
                    cb.conv_toff = kk - d.pad;
                    cb.tap = kk;
                    SOLA_TRY(cast_t(cb, s));
                }
            } else {
                SOLA_TRY(cast_t(cb, s));
            }
            xt_of[j] = dst;
        }
    }
    GemmDesc g{};
    g.nprob = d.nprob;
    for (int j = 0; j < d.nprob; ++j) g.p[j] = GemmProblem{at + (size_t)j * d.N * rowf, xt_of[j], nullptr, nullptr, d.C[j]};
    g.M = d.N; g.N = d.K; g.K = (int)Mp; g.lda = (int)Mp; g.ldr = 0; g.ldc = d.K;
    g.ab = d.ab; g.out_scale = 1.f; g.out_scale_dev = scal + 1;
    if (d.scal_b)  // the activations' own scale (the caller's tokens): every problem shares it
        for (int j = 0; j < d.nprob; ++j) g.p[j].scale_dev = d.scal_b + 1;
    g.ksplit = ks; g.splitk_ws = slabs; g.splitk_bytes = (size_t)d.nprob * ks * d.N * d.K * sizeof(float);
    return launch_gemm(g, s);
}
