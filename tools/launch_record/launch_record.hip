// Host-only launch recorder: the sequencing code of a build (forward.hip, forward_infer.hip, backward.hip, ragged.hip, api.hip) linked
// behind definitions that take the place of the launchers it calls and of the HIP runtime, so that a run prints what the device would have
// been handed - every descriptor field by field, device pointers as region+offset of fake address ranges, uploads as a hash of their
// bytes, workspace sizes, error codes and messages - without a GPU (nothing here initialises one: the HIP runtime is not even linked).
// Two builds whose records are equal line for line enqueue the same work.  `make -C tools/launch_record` builds it from build/obj;
// tools/README.md says how to compare a build against another.
//
// The predicates and size functions (gemm_tn_split_supported, attention_bwd_bf16_supported, scratch sizes, ...) are the library's own.
// A replaced launcher prints and succeeds; launch_attention reports the operand cast written and launch_group_norm the statistics kept
// (LAUNCH_RECORD_NOREPORT=1: neither), so the routes of the backward that depend on them are taken both ways.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../sola_amd/csrc/kernels.h"
#include "../../include/sola_hip.h"

// ---- fake device memory: region r is [r << 40, (r + 1) << 40) -----------------------------------------------------------------------------
static std::vector<std::string> g_regions = {"null"};
static char* fake(const char* name) {
    g_regions.push_back(name);
    return reinterpret_cast<char*>((uintptr_t)(g_regions.size() - 1) << 40);
}
static bool is_fake(const void* p) { return p && ((uintptr_t)p >> 40) < g_regions.size(); }
static std::string ptr_str(const void* p) {
    if (!p) return "null";
    if (!is_fake(p)) return "host";
    char b[64];
    snprintf(b, sizeof b, "%s+0x%llx", g_regions[(uintptr_t)p >> 40].c_str(), (unsigned long long)((uintptr_t)p & (((uintptr_t)1 << 40) - 1)));
    return b;
}
static unsigned long long fnv(const void* p, size_t n) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
    return h;
}

// ---- printing: __builtin_dump_struct hands every field to this printf, which renders pointers as regions and floats with all their digits
static int rec_printf(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    for (const char* f = fmt; *f;) {
        if (*f != '%') { fputc(*f++, stdout); continue; }
        const char* e = f + 1;
        while (*e && !strchr("diuxXpsfgecn%", *e)) ++e;
        const std::string spec(f, e + 1);
        const bool ll = spec.find("ll") != std::string::npos, l = !ll && spec.find('l') != std::string::npos;
        switch (*e) {
            case '%': fputc('%', stdout); break;
            case 'p': fputs(ptr_str(va_arg(ap, void*)).c_str(), stdout); break;
            case 's': printf(spec.c_str(), va_arg(ap, const char*)); break;
            case 'f': case 'g': case 'e': printf("%.9g", va_arg(ap, double)); break;
            case 'c': printf(spec.c_str(), va_arg(ap, int)); break;
            default:
                if (ll) printf(spec.c_str(), va_arg(ap, long long));
                else if (l) printf(spec.c_str(), va_arg(ap, long));
                else printf(spec.c_str(), va_arg(ap, int));
        }
        f = e + 1;
    }
    va_end(ap);
    return 0;
}
template <class T> void put(const T& v);
// the used entries of the array members, which the struct dump shows as an address only
template <class T> void put_arrays(const T&) {}
static void put_arrays(const GemmDesc& d) {
    for (int j = 0; j < d.nprob && j < 3; ++j) { put(d.p[j]); printf("  w_nn[%d] = %s\n", j, ptr_str(d.w_nn[j]).c_str()); }
}
static void put_arrays(const ConvFramePlan& d) { for (int j = 0; j < d.n; ++j) { put(d.l[j]); for (int i = 0; i < d.l[j].nprob; ++i) printf("  frame %d lo %d\n", d.l[j].frame[i], d.l[j].lo[i]); } }
static void put_arrays(const ConvTapWeights& d) { for (int j = 0; j < d.n; ++j) printf("  e[%d] = %d %d %s\n", j, d.e[j].lo, d.e[j].hi, ptr_str(d.e[j].w).c_str()); }
static void put_arrays(const GemmTnGroupDesc& d) { for (int j = 0; j < d.nprob; ++j) put(d.p[j]); }
static void put_arrays(const GemmTnSplitDesc& d) {
    for (int j = 0; j < d.nprob; ++j)
        printf("  [%d] A %s B %s C %s B16 %s\n", j, ptr_str(d.A[j]).c_str(), ptr_str(d.B[j]).c_str(), ptr_str(d.C[j]).c_str(), ptr_str(d.B16[j]).c_str());
}
static void put_arrays(const ColsumPairGroupDesc& d) {
    for (int j = 0; j < d.n; ++j)
        printf("  [%d] %s %s %s %s %d %d\n", j, ptr_str(d.in0[j]).c_str(), ptr_str(d.in1[j]).c_str(), ptr_str(d.out0[j]).c_str(), ptr_str(d.out1[j]).c_str(), d.rows[j], d.cols[j]);
}
static void put_arrays(const ColsumJobsDesc& d) {
    for (int j = 0; j < d.n; ++j) printf("  [%d] %s %s %d %d %d\n", j, ptr_str(d.in[j]).c_str(), ptr_str(d.out[j]).c_str(), d.rows[j], d.cols[j], d.ld[j]);
}
// the element formats a descriptor or a launcher call carries, as one canonical line behind it (the struct dump shows Elem fields as integers)
static int fmt_line(const char* k0, Elem e0, const char* k1 = nullptr, Elem e1 = Elem::F32, const char* k2 = nullptr, Elem e2 = Elem::F32) {
    printf("fmt %s=%s", k0, elem_name(e0));
    if (k1) printf(" %s=%s", k1, elem_name(e1));
    if (k2) printf(" %s=%s", k2, elem_name(e2));
    fputc('\n', stdout);
    return SOLA_OK;
}
template <class T> void put_formats(const T&) {}
static void put_formats(const GemmDesc& d) { fmt_line("ab", d.ab, "r", d.r, "c", d.c); }
static void put_formats(const GemmTnSplitDesc& d) { fmt_line("ab", d.ab, "rm", d.rm_fmt, "b16", d.b16_fmt); }
static void put_formats(const AttnDesc& d) { fmt_line("in", d.in, "out", d.out, "cast", d.cast); }
static void put_formats(const AttnBwdDesc& d) { fmt_line("io", d.io_fmt, "dout", d.dout_fmt, "o", d.o_fmt); }
static void put_formats(const GroupNormDesc& d) { fmt_line("in", d.in, "out", d.out, "cast", d.cast); }
static void put_formats(const GroupNormBwdDesc& d) { fmt_line("x", d.x_fmt, "dy2", d.dy2_fmt); }
template <class T> void put(const T& v) {
    if constexpr (std::is_pointer<T>::value) printf(" %s", ptr_str(reinterpret_cast<const void*>(v)).c_str());
    else if constexpr (std::is_floating_point<T>::value) printf(" %.9g", (double)v);
    else if constexpr (std::is_arithmetic<T>::value) printf(" %lld", (long long)v);
    else {
        fputc('\n', stdout);
        __builtin_dump_struct(&v, rec_printf);
        put_arrays(v);
        put_formats(v);
    }
}
template <class... A> int rec(const char* name, const A&... a) {
    fputs(name, stdout);
    (put(a), ...);
    fputc('\n', stdout);
    return SOLA_OK;
}
template <class T> void put_list(const T* v, int n) { for (int i = 0; i < n; ++i) put(v[i]); }

// ---- the launchers the sequences call ------------------------------------------------------------------------------------------------------
static bool g_report = true;
int launch_amax_colsum(float const* a0, int a1, long long a2, int a3, float* a4, float* a5, hipStream_t a6) { return rec("launch_amax_colsum",  a0, a1, a2, a3, a4, a5, a6); }
int launch_attention(AttnDesc const& a0, hipStream_t a1) { int r = rec("launch_attention", a0,a1); if (g_report && a0.o_cast && a0.o_cast_done) *a0.o_cast_done = true; return r; }
int launch_attention_bwd(AttnBwdDesc const& a0, hipStream_t a1) { return rec("launch_attention_bwd",  a0, a1); }
int launch_attention_f16(AttnDesc const& a0, hipStream_t a1) { return rec("launch_attention_f16",  a0, a1); }
int launch_cast_bf16_colsum(float const* a0, int a1, void* a2, int a3, long long a4, int a5, float* a6, float* a7, hipStream_t a8) { return rec("launch_cast_bf16_colsum",  a0, a1, a2, a3, a4, a5, a6, a7, a8); }
int launch_cast_f16(float const* a0, int a1, void* a2, int a3, long long a4, int a5, float a6, float* a7, Elem fmt, hipStream_t a8, int a9, float* a10) { rec("launch_cast_f16",  a0, a1, a2, a3, a4, a5, a6, a7, a8, a9, a10); return fmt_line("out", fmt); }
int launch_cast_f16_auto_multi(float const* const* a0, void* const* a1, int a2, int a3, int a4, float* a5, Elem fmt, hipStream_t a6) { rec("launch_cast_f16_auto_multi", a2,a3,a4,a5,a6); put_list(a0, a2); put_list(a1, a2); fputc(10, stdout); return fmt_line("out", fmt); }
int launch_cast_f16_scaled(float const* a0, int a1, void* a2, int a3, long long a4, int a5, float* a6, Elem fmt, hipStream_t a7) { rec("launch_cast_f16_scaled",  a0, a1, a2, a3, a4, a5, a6, a7); return fmt_line("out", fmt); }
int launch_cast_f16_t(float const* a0, int a1, void* a2, long long a3, int a4, int a5, float* a6, Elem fmt, hipStream_t a7) { rec("launch_cast_f16_t",  a0, a1, a2, a3, a4, a5, a6, a7); return fmt_line("out", fmt); }
int launch_cast_sp16(float const* a0, int a1, float* a2, int a3, long long a4, int a5, float a6, hipStream_t a7, void* a8) { return rec("launch_cast_sp16",  a0, a1, a2, a3, a4, a5, a6, a7, a8); }
int launch_cast_sp16_auto(float const* a0, int a1, float* a2, int a3, long long a4, int a5, float* a6, hipStream_t a7) { return rec("launch_cast_sp16_auto",  a0, a1, a2, a3, a4, a5, a6, a7); }
int launch_cast_sp16_auto_multi(float const* const* a0, float* const* a1, int a2, int a3, int a4, float* a5, hipStream_t a6) { rec("launch_cast_sp16_auto_multi", a2,a3,a4,a5,a6); put_list(a0, a2); put_list(a1, a2); fputc(10, stdout); return SOLA_OK; }
int launch_cast_sp16_multi(CastJob const* a0, int a1, float a2, hipStream_t a3) { rec("launch_cast_sp16_multi", a1,a2,a3); put_list(a0, a1); return SOLA_OK; }
int launch_cast_sp16_scaled(float const* a0, int a1, float* a2, int a3, long long a4, int a5, float* a6, hipStream_t a7) { return rec("launch_cast_sp16_scaled",  a0, a1, a2, a3, a4, a5, a6, a7); }
int launch_cast_sp16_t(float const* a0, int a1, float* a2, long long a3, int a4, int a5, float* a6, hipStream_t a7) { return rec("launch_cast_sp16_t",  a0, a1, a2, a3, a4, a5, a6, a7); }
int launch_col2im(float const* a0, float* a1, long long a2, int a3, int a4, int a5, int a6, int a7, int a8, Elem z_fmt, hipStream_t a9) { rec("launch_col2im",  a0, a1, a2, a3, a4, a5, a6, a7, a8, a9); return fmt_line("z", z_fmt); }
int launch_col2im_ragged(float const* a0, float* a1, long long a2, int4 const* a3, int a4, int a5, int a6, int a7, Elem z_fmt, hipStream_t a8) { rec("launch_col2im_ragged",  a0, a1, a2, a3, a4, a5, a6, a7, a8); return fmt_line("z", z_fmt); }
int launch_colsum(float const* a0, float* a1, int a2, int a3, int a4, int a5, float a6, int a7, float* a8, size_t a9, hipStream_t a10) { return rec("launch_colsum",  a0, a1, a2, a3, a4, a5, a6, a7, a8, a9, a10); }
int launch_colsum_jobs(ColsumJobsDesc const& a0, hipStream_t a1) { return rec("launch_colsum_jobs",  a0, a1); }
int launch_colsum_pair(float const* a0, float const* a1, float* a2, float* a3, int a4, int a5, int a6, float* a7, size_t a8, hipStream_t a9) { return rec("launch_colsum_pair",  a0, a1, a2, a3, a4, a5, a6, a7, a8, a9); }
int launch_colsum_pair_group(ColsumPairGroupDesc const& a0, hipStream_t a1) { return rec("launch_colsum_pair_group",  a0, a1); }
int launch_colsum_slabs_bf16(void const* a0, int a1, long long a2, int a3, float* a4, float* a5, hipStream_t a6) { return rec("launch_colsum_slabs_bf16",  a0, a1, a2, a3, a4, a5, a6); }
int launch_conv_frames(GemmDesc const& a0, ConvFramePlan const& a1, ConvTapWeights const& a2, hipStream_t a3) { return rec("launch_conv_frames",  a0, a1, a2, a3); }
int launch_gather_rows(float const* a0, float* a1, int4 const* a2, int a3, int a4, long long a5, hipStream_t a6) { return rec("launch_gather_rows",  a0, a1, a2, a3, a4, a5, a6); }
int launch_gemm(GemmDesc const& a0, hipStream_t a1) { return rec("launch_gemm",  a0, a1); }
int launch_gemm_tn(GemmTnDesc const& a0, hipStream_t a1) { return rec("launch_gemm_tn",  a0, a1); }
int launch_gemm_tn_group(GemmTnGroupDesc const& a0, hipStream_t a1) { return rec("launch_gemm_tn_group",  a0, a1); }
int launch_gemm_tn_split(GemmTnSplitDesc const& a0, hipStream_t a1) { return rec("launch_gemm_tn_split",  a0, a1); }
int launch_group_norm(GroupNormDesc const& a0, hipStream_t a1) { int r = rec("launch_group_norm", a0,a1); if (g_report && a0.stats_out && a0.stats_written) *a0.stats_written = 1; return r; }
int launch_group_norm_bwd(GroupNormBwdDesc const& a0, hipStream_t a1) { return rec("launch_group_norm_bwd",  a0, a1); }
int launch_lang_concat(float const* a0, float const* a1, float* a2, float* a3, int a4, int a5, int a6, int a7, hipStream_t a8) { return rec("launch_lang_concat",  a0, a1, a2, a3, a4, a5, a6, a7, a8); }
int launch_lang_concat_ragged(float const* a0, float const* a1, float* a2, float* a3, int a4, int4 const* a5, int a6, int a7, hipStream_t a8) { return rec("launch_lang_concat_ragged",  a0, a1, a2, a3, a4, a5, a6, a7, a8); }
int launch_lang_concat_shared(float const* a0, float const* a1, float* a2, float* a3, int a4, int a5, int a6, int a7, hipStream_t a8) { return rec("launch_lang_concat_shared",  a0, a1, a2, a3, a4, a5, a6, a7, a8); }
int launch_neg_token_grad(float const* a0, float const* a1, float const* a2, float* a3, int a4, int a5, int a6, int a7, hipStream_t a8, int4 const* a9) { return rec("launch_neg_token_grad",  a0, a1, a2, a3, a4, a5, a6, a7, a8, a9); }
int launch_norm_range_check(NormPair const* a0, int a1, int* a2, hipStream_t a3) { rec("launch_norm_range_check", a1,a2,a3); put_list(a0, a1); return SOLA_OK; }
int launch_pos_encoding(float const* a0, int a1, int a2, int a3, float* a4, hipStream_t a5) { return rec("launch_pos_encoding",  a0, a1, a2, a3, a4, a5); }
int launch_score_head(HeadDesc const& a0, hipStream_t a1) { return rec("launch_score_head",  a0, a1); }
int launch_score_head_bwd(HeadBwdDesc const& a0, hipStream_t a1) { return rec("launch_score_head_bwd",  a0, a1); }
int launch_segsum_rows(float const* a0, float* a1, int const* a2, int a3, int a4, hipStream_t a5) { return rec("launch_segsum_rows",  a0, a1, a2, a3, a4, a5); }
int launch_transpose(float const* a0, float* a1, int a2, int a3, int a4, int a5, int a6, hipStream_t a7) { return rec("launch_transpose",  a0, a1, a2, a3, a4, a5, a6, a7); }
int launch_transpose_cast(float const* a0, void* a1, int a2, int a3, int a4, int a5, int a6, float a7, Elem fmt, hipStream_t a9) { rec("launch_transpose_cast",  a0, a1, a2, a3, a4, a5, a6, a7, a9); return fmt_line("out", fmt); }
int launch_ws_backward(WsBwdLayer const* a0, int a1, hipStream_t a2) { rec("launch_ws_backward", a1,a2); put_list(a0, a1); return SOLA_OK; }
int launch_ws_standardize(WsLayer const* a0, int a1, hipStream_t a2) { rec("launch_ws_standardize", a1,a2); put_list(a0, a1); return SOLA_OK; }

// ---- the HIP runtime the sequences call themselves ----------------------------------------------------------------------------------------
static std::vector<std::pair<const void*, std::string>> g_kernels;
static struct { dim3 grid, block; size_t shmem; hipStream_t s; } g_cfg;
static char *g_dev = nullptr, *g_ev = nullptr, *g_st = nullptr;
static char* bump(char*& at, const char* region, size_t bytes) {
    if (!at) at = fake(region);
    char* p = at;
    at += (bytes + 255) & ~(size_t)255;
    return p;
}
static void copy_rec(const char* what, void* dst, const void* src, size_t n, hipStream_t s) {
    printf("%s %s <- %s %zu", what, ptr_str(dst).c_str(), ptr_str(src).c_str(), n);
    if (!is_fake(src)) printf(" bytes %016llx", fnv(src, n));
    if (!is_fake(dst)) {
        if (is_fake(src)) memset(dst, 0, n);  // what comes back from the device: zeros (guard words clear)
        else memcpy(dst, src, n);
    }
    printf(" stream %s\n", ptr_str(s).c_str());
}
extern "C" {
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "no error"; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600* p, int) {
    memset(p, 0, sizeof *p);
    p->multiProcessorCount = 256;
    return hipSuccess;
}
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipMalloc(void** p, size_t n) { *p = bump(g_dev, "dev", n); printf("hipMalloc %zu -> %s\n", n, ptr_str(*p).c_str()); return hipSuccess; }
hipError_t hipFree(void* p) { printf("hipFree %s\n", ptr_str(p).c_str()); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = calloc(1, n); return hipSuccess; }
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
hipError_t hipMemset(void* p, int v, size_t n) { printf("hipMemset %s %d %zu\n", ptr_str(p).c_str(), v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t s) { printf("hipMemsetAsync %s %d %zu stream %s\n", ptr_str(p).c_str(), v, n, ptr_str(s).c_str()); return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { copy_rec("hipMemcpy", d, s, n, nullptr); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t st) { copy_rec("hipMemcpyAsync", d, s, n, st); return hipSuccess; }
hipError_t hipMemcpy2DAsync(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, hipMemcpyKind, hipStream_t st) {
    printf("hipMemcpy2DAsync %s %zu <- %s %zu, %zu x %zu stream %s\n", ptr_str(d).c_str(), dp, ptr_str(s).c_str(), sp, w, h, ptr_str(st).c_str());
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { *e = reinterpret_cast<hipEvent_t>(bump(g_ev, "event", 1)); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { printf("hipEventRecord %s stream %s\n", ptr_str(e).c_str(), ptr_str(s).c_str()); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { printf("hipEventSynchronize %s\n", ptr_str(e).c_str()); return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = reinterpret_cast<hipStream_t>(bump(g_st, "stream", 1)); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { printf("hipStreamSynchronize %s\n", ptr_str(s).c_str()); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { printf("hipStreamWaitEvent stream %s %s\n", ptr_str(s).c_str(), ptr_str(e).c_str()); return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* st) { *st = hipStreamCaptureStatusNone; return hipSuccess; }
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void**, size_t shmem, hipStream_t s) {
    const char* name = "?";
    for (const auto& k : g_kernels)
        if (k.first == f) name = k.second.c_str();
    printf("hipLaunchKernel %s grid %u %u %u block %u %u %u lds %zu stream %s\n", name, grid.x, grid.y, grid.z, block.x, block.y, block.z, shmem, ptr_str(s).c_str());
    return hipSuccess;
}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t s) { g_cfg = {grid, block, shmem, s}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, hipStream_t* s) {
    *grid = g_cfg.grid; *block = g_cfg.block; *shmem = g_cfg.shmem; *s = g_cfg.s;
    return hipSuccess;
}
void** __hipRegisterFatBinary(const void*) { static void* h = nullptr; return &h; }
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* name, unsigned, void*, void*, void*, void*, int*) { g_kernels.emplace_back(host_fn, name); }
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void**) {}
}

// ---- cases ----------------------------------------------------------------------------------------------------------------------------------
static const SolaConfig kFull = {256, 1024, 2, 100, 32, 8, 8, 8}, kSmall = {32, 128, 2, 100, 4, 8, 8, 8},
                        kDeep = {256, 1024, 11, 100, 32, 8, 8, 8};
static char *g_obj, *g_lang, *g_sm, *g_st_out, *g_ws, *g_scratch, *g_dsm, *g_dst, *g_w, *g_g, *g_arena;

static SolaCtx* make_ctx(const SolaConfig& cfg, int precision, bool grads, bool arena) {
    SolaCtx* c = nullptr;
    printf("ctx_create -> %d\n", sola_ctx_create(&cfg, 0, &c));
    size_t at = 0;
    for (int i = 0; i < sola_num_weights(c); ++i) {
        const char* name; int64_t numel;
        sola_weight_info(c, i, &name, &numel);
        sola_set_weight(c, name, g_w + at, numel);
        if (grads) sola_set_grad(c, name, g_g + at, numel);
        at += ((size_t)numel * 4 + 255) & ~(size_t)255;
    }
    printf("set_precision %d -> %d\n", precision, sola_set_precision(c, precision));
    if (arena) sola_set_x16_arena(c, g_arena, (size_t)1 << 36);
    return c;
}
static void status(const char* what, int r) { printf("%s -> %d%s%s\n", what, r, r ? " : " : "", r ? sola_last_error() : ""); }

struct Rag { std::vector<int32_t> vn, vt, sv, sl; SolaRaggedBatch b; };
static Rag rag(std::vector<int32_t> vn, std::vector<int32_t> vt, std::vector<int32_t> sv, std::vector<int32_t> sl) {
    Rag r{std::move(vn), std::move(vt), std::move(sv), std::move(sl), {}};
    return r;
}
static const SolaRaggedBatch* batch(Rag& r) {
    r.b = SolaRaggedBatch{(int32_t)r.vn.size(), r.vn.data(), r.vt.data(), (int32_t)r.sv.size(), r.sv.data(), r.sl.data()};
    return &r.b;
}
static std::vector<Rag> ragged_cases(bool train) {
    std::vector<Rag> v;
    const std::vector<int32_t> id6 = {0, 1, 2, 3, 4, 5};
    v.push_back(rag({5, 9, 12, 7, 16, 3}, {20, 33, 40, 64, 25, 150}, id6, {5, 7, 3, 11, 16, 1}));
    v.push_back(rag({20, 36, 48, 100, 64, 12}, {20, 33, 40, 64, 25, 150}, id6, {5, 7, 3, 11, 16, 1}));
    if (train) v.push_back(rag(std::vector<int32_t>(10, 64), std::vector<int32_t>(10, 32), {0, 1, 2, 3, 4, 5, 6, 7, 8, 9}, std::vector<int32_t>(10, 16)));
    else {
        v.push_back(rag({9, 20, 64, 130, 2, 1}, {24, 40, 32, 900, 8, 8}, id6, {5, 7, 3, 100, 16, 1}));
        v.push_back(rag({5, 9, 12}, {20, 33, 40}, {0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2}, {5, 7, 3, 11, 16, 1, 2, 9, 4, 4, 8, 6}));
    }
    return v;
}
struct Uni { int B, N, T, L; };

static void infer_cases() {
    const Uni shapes[] = {{1, 4, 32, 5}, {8, 24, 32, 7}, {64, 8, 32, 16}, {256, 64, 32, 16}, {2, 128, 32, 100}, {4, 100, 1000, 20}, {3, 7, 9, 1}};
    for (int prec = 0; prec <= 2; ++prec) {
        SolaCtx* c = make_ctx(kFull, prec, false, false);
        for (const Uni& u : shapes) {
            const size_t need = sola_workspace_bytes(c, u.B, u.N, u.T, u.L);
            printf("== infer precision %d uniform %d %d %d %d workspace %zu\n", prec, u.B, u.N, u.T, u.L, need);
            status("forward", sola_forward(c, (float*)g_obj, (float*)g_lang, u.B, u.N, u.T, u.L, (float*)g_sm, (float*)g_st_out, g_ws, need, nullptr));
        }
        int i = 0;
        for (Rag& r : ragged_cases(false)) {
            const size_t need = sola_ragged_workspace_bytes(c, batch(r));
            printf("== infer precision %d ragged %d workspace %zu\n", prec, i++, need);
            status("forward_ragged", sola_forward_ragged(c, (float*)g_obj, (float*)g_lang, batch(r), (float*)g_sm, (float*)g_st_out, g_ws, need, nullptr));
        }
        sola_ctx_destroy(c);
    }
    printf("== infer error paths\n");
    SolaCtx* c = make_ctx(kSmall, 2, false, false);
    status("forward (small model, 16-bit storage)", sola_forward(c, (float*)g_obj, (float*)g_lang, 1, 4, 32, 5, (float*)g_sm, (float*)g_st_out, g_ws, (size_t)1 << 30, nullptr));
    sola_set_precision(c, 0);
    status("forward (null)", sola_forward(c, nullptr, (float*)g_lang, 1, 4, 32, 5, (float*)g_sm, (float*)g_st_out, g_ws, (size_t)1 << 30, nullptr));
    status("forward (workspace)", sola_forward(c, (float*)g_obj, (float*)g_lang, 1, 4, 32, 5, (float*)g_sm, (float*)g_st_out, g_ws, sola_workspace_bytes(c, 1, 4, 32, 5) - 256, nullptr));
    status("forward (B = 0)", sola_forward(c, (float*)g_obj, (float*)g_lang, 0, 4, 32, 5, (float*)g_sm, (float*)g_st_out, g_ws, (size_t)1 << 30, nullptr));
    Rag bad = rag({5, 9}, {20, 0}, {0, 1}, {5, 7});
    status("forward_ragged (T = 0)", sola_forward_ragged(c, (float*)g_obj, (float*)g_lang, batch(bad), (float*)g_sm, (float*)g_st_out, g_ws, (size_t)1 << 30, nullptr));
    sola_ctx_destroy(c);
}

// one training step: forward, backward, every bucket waited for.  rg = null: the uniform shape u
static void train_step(SolaCtx* c, const Uni& u, Rag* rg, long long scratch_short = 0) {
    const size_t need = rg ? sola_train_ragged_workspace_bytes(c, batch(*rg)) : sola_train_workspace_bytes(c, u.B, u.N, u.T, u.L);
    const size_t bneed = rg ? sola_backward_ragged_workspace_bytes(c, batch(*rg)) : sola_backward_workspace_bytes(c, u.B, u.N, u.T, u.L);
    printf("workspace %zu scratch %zu\n", need, bneed);
    if (rg) status("forward_train_ragged", sola_forward_train_ragged(c, (float*)g_obj, (float*)g_lang, batch(*rg), (float*)g_sm, (float*)g_st_out, g_ws, need, nullptr));
    else status("forward_train", sola_forward_train(c, (float*)g_obj, (float*)g_lang, u.B, u.N, u.T, u.L, (float*)g_sm, (float*)g_st_out, g_ws, need, nullptr));
    size_t an, ac, au;
    sola_x16_arena_info(c, &an, &ac, &au);
    printf("x16 arena need %zu used %zu\n", an, au);
    if (rg) status("backward_ragged", sola_backward_ragged(c, (float*)g_dsm, (float*)g_dst, g_ws, g_scratch, bneed - scratch_short, nullptr));
    else status("backward", sola_backward(c, (float*)g_dsm, (float*)g_dst, g_ws, g_scratch, bneed - scratch_short, nullptr));
    for (int b = 0; b < sola_grad_bucket_count(c); ++b) sola_backward_wait_bucket(c, b, nullptr);
}

static void train_cases() {
    const Uni shapes[] = {{1, 64, 32, 16}, {3, 64, 32, 7}, {5, 64, 32, 7}, {9, 64, 32, 5}, {36, 64, 32, 16}, {3, 7, 9, 1}, {2, 10, 1000, 20}};
    std::vector<Rag> rags = ragged_cases(true);
    const struct { const char* key; int value; } switches[] = {
        {"bwd_group_rows", 0}, {"bwd_group_rows", 100000}, {"bwd_side_rows", 4096}, {"train_dw_f16", 0}, {"bwd_dual_cast", 0}, {"bwd_fused_bf16_cast", 0},
        {"train_x16_keep", 0}, {"train_bf16_store", 0}, {"train_bf16_store", 1}, {"train_bf16_store", 2}, {"train_split_min_rows", 0}, {"train_gn_stats", 0},
        {"train_attn_cast", 0}};
    for (int prec = 0; prec <= 3; ++prec) {
        SolaCtx* c = make_ctx(kFull, prec, true, true);
        for (const Uni& u : shapes) {
            printf("== train precision %d uniform %d %d %d %d\n", prec, u.B, u.N, u.T, u.L);
            train_step(c, u, nullptr);
        }
        for (size_t i = 0; i < rags.size(); ++i) {
            printf("== train precision %d ragged %zu\n", prec, i);
            train_step(c, Uni{}, &rags[i]);
        }
        for (const auto& sw : switches) {
            int was = 0, dflt = 0;
            sola_tune_query(sw.key, &was, &dflt);
            sola_tune(sw.key, sw.value);
            for (int k = 0; k < 4; ++k) {
                printf("== train precision %d %s %d case %d\n", prec, sw.key, sw.value, k);
                if (k < 2) train_step(c, shapes[k == 0 ? 0 : 3], nullptr);
                else train_step(c, Uni{}, &rags[k - 2]);
            }
            sola_tune(sw.key, was);
        }
        printf("== train precision %d dropout\n", prec);
        sola_set_dropout(c, 0.2f, 0.1f, 1234);
        train_step(c, shapes[3], nullptr);
        train_step(c, Uni{}, &rags[0]);
        sola_set_dropout(c, 0.f, 0.f, 0);
        printf("== train precision %d no operand arena\n", prec);
        sola_set_x16_arena(c, nullptr, 0);
        train_step(c, shapes[2], nullptr);
        train_step(c, Uni{}, &rags[1]);
        sola_ctx_destroy(c);
    }
    printf("== train state errors\n");
    {
        SolaCtx* c = make_ctx(kFull, 0, true, true);
        status("backward (no forward)", sola_backward(c, (float*)g_dsm, (float*)g_dst, g_ws, g_scratch, (size_t)1 << 36, nullptr));
        const size_t need = sola_train_ragged_workspace_bytes(c, batch(rags[0]));
        status("forward_train_ragged", sola_forward_train_ragged(c, (float*)g_obj, (float*)g_lang, batch(rags[0]), (float*)g_sm, (float*)g_st_out, g_ws, need, nullptr));
        status("backward (after a ragged forward)", sola_backward(c, (float*)g_dsm, (float*)g_dst, g_ws, g_scratch, (size_t)1 << 36, nullptr));
        status("backward_ragged (another workspace)", sola_backward_ragged(c, (float*)g_dsm, (float*)g_dst, g_ws + 4096, g_scratch, (size_t)1 << 36, nullptr));
        train_step(c, shapes[0], nullptr, 256);
        train_step(c, Uni{}, &rags[0], 256);
        sola_ctx_destroy(c);
        c = make_ctx(kFull, 0, false, true);
        train_step(c, shapes[0], nullptr);  // a gradient buffer missing
        sola_ctx_destroy(c);
        c = make_ctx(kFull, 3, true, true);
        const Uni u = shapes[2];
        const size_t n2 = sola_train_workspace_bytes(c, u.B, u.N, u.T, u.L);
        status("forward_train", sola_forward_train(c, (float*)g_obj, (float*)g_lang, u.B, u.N, u.T, u.L, (float*)g_sm, (float*)g_st_out, g_ws, n2, nullptr));
        sola_tune("train_bf16_store", 2);
        status("backward (train_bf16_store changed)", sola_backward(c, (float*)g_dsm, (float*)g_dst, g_ws, g_scratch, (size_t)1 << 36, nullptr));
        sola_tune("train_bf16_store", 3);
        sola_ctx_destroy(c);
    }
    // more than ten layers, the reduced-precision steps: every layer's projections read their own 16-bit copies and scales (ctx.h: lin16_weight)
    for (int prec = 1; prec <= 3; ++prec) {
        SolaCtx* c = make_ctx(kDeep, prec, true, true);
        printf("== train deep precision %d uniform %d %d %d %d\n", prec, shapes[4].B, shapes[4].N, shapes[4].T, shapes[4].L);
        train_step(c, shapes[4], nullptr);
        printf("== train deep precision %d ragged 0\n", prec);
        train_step(c, Uni{}, &rags[0]);
        sola_ctx_destroy(c);
    }
}

int main(int argc, char** argv) {
    g_report = !getenv("LAUNCH_RECORD_NOREPORT");
    g_obj = fake("obj"); g_lang = fake("lang"); g_sm = fake("score_map"); g_st_out = fake("score_tokens"); g_ws = fake("ws");
    g_scratch = fake("scratch"); g_dsm = fake("d_score_map"); g_dst = fake("d_score_tokens"); g_w = fake("w"); g_g = fake("g"); g_arena = fake("arena");
    const std::string what = argc > 1 ? argv[1] : "all";
    if (what == "infer" || what == "all") infer_cases();
    if (what == "train" || what == "all") train_cases();
    return 0;
}
