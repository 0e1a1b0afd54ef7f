// Ragged batches (ragged.h): what the ragged inference forward (forward_infer.hip) and the ragged training step (forward.hip /
// backward.hip) share - the host-side shape bookkeeping (rag_shape), the device plan kernel that turns the uploaded (N, T, L)
// arrays into the unit tables every shape-dependent kernel reads, the table layout, the pinned staging ring of the upload and
// the scratch size of the sliced GroupNorm shape.
#include <string.h>

#include <algorithm>

#include "ragged.h"

namespace {

// ---- device-side plan: unit tables from the compact per-video / per-sample descriptors ---------------------------
struct RagDev {
    // uploaded descriptor arrays (ints)
    const int *vN, *vT /* [7][V] */, *vRow0 /* [7][V+1] */, *vTrk0 /* [V+1] */, *vTp0 /* [V+1] */;
    const int *sVid, *sL, *sLin0, *sLrow0, *sTrk0, *sRow0, *sTp0;  // [S] / [S+1]
    int V, S, NT /* video tracks */, n_neg;
    int stride[5], pad[5], k[5];
    // tables to build
    int4* u_lvl[7];   // [NT] per level: (first row, 1, T_level, video)
    int2* rowmap[5];  // [rows of level l+1]
    int4* u_vt;       // [sum T'_v]  (first row, T'_v, N_v, t')
    int4* u_st;       // [sum T'_i]
    int4* u_strk;     // [sum N_i]   (first row, 1, T', sample)
    int4* u_smp;      // [S]         (first row, 1, N*T', sample)
    int4* u_lang;     // [S]         (first input text row, L, first lang_cat row, W)
    int4* u_langk;    // [S]         (first lang_cat row, 1, W, 0)
    int4* u_gather;   // [S]         (first sample row, first video row at T', rows, 0)
    int4* imap[5];    // training: [rows of level l + 1] (first output row of the sequence under conv l + 1, T_out, ti, 0); null = not built
};

// largest i in [0, n) with pre[i] <= x (pre ascending, pre[0] = 0)
__device__ __forceinline__ int seg_of(const int* pre, int n, int x) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// blockIdx.y = section: 0..6 level tables, 7..11 row maps, 12 (video, t') units, 13 (sample, t') units, 14 sample tracks, 15 samples,
// 16..20 (training) input-row maps of convs 1..5
__global__ __launch_bounds__(256) void ragged_plan_kernel(const RagDev p) {
    const int sec = blockIdx.y;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x;; i += (long long)gridDim.x * 256) {
        if (sec < 7) {
            if (i >= p.NT) return;
            const int v = seg_of(p.vTrk0, p.V, (int)i);
            const int T = p.vT[sec * p.V + v];
            p.u_lvl[sec][i] = make_int4(p.vRow0[sec * (p.V + 1) + v] + ((int)i - p.vTrk0[v]) * T, 1, T, v);
        } else if (sec < 12) {
            const int l = sec - 7;  // conv l: level l -> level l + 1
            const int* pre = p.vRow0 + (l + 1) * (p.V + 1);
            if (i >= pre[p.V]) return;
            const int v = seg_of(pre, p.V, (int)i);
            const int local = (int)i - pre[v];
            const int T_out = p.vT[(l + 1) * p.V + v], T_in = p.vT[l * p.V + v];
            const int n = local / T_out, to = local - n * T_out;
            const int t0 = to * p.stride[l] - p.pad[l];
            int bits = 0;
            for (int kk = 0; kk < p.k[l]; ++kk) bits |= ((unsigned)(t0 + kk) < (unsigned)T_in) ? (1 << kk) : 0;
            p.rowmap[l][i] = make_int2(p.vRow0[l * (p.V + 1) + v] + n * T_in + t0, bits);
        } else if (sec == 12) {
            if (i >= p.vTp0[p.V]) return;
            const int v = seg_of(p.vTp0, p.V, (int)i);
            const int t = (int)i - p.vTp0[v];
            p.u_vt[i] = make_int4(p.vRow0[6 * (p.V + 1) + v] + t, p.vT[6 * p.V + v], p.vN[v], t);
        } else if (sec == 13) {
            if (i >= p.sTp0[p.S]) return;
            const int sidx = seg_of(p.sTp0, p.S, (int)i);
            const int t = (int)i - p.sTp0[sidx];
            const int v = p.sVid[sidx];
            p.u_st[i] = make_int4(p.sRow0[sidx] + t, p.vT[6 * p.V + v], p.vN[v], t);
        } else if (sec == 14) {
            if (i >= p.sTrk0[p.S]) return;
            const int sidx = seg_of(p.sTrk0, p.S, (int)i);
            const int v = p.sVid[sidx];
            const int Tp = p.vT[6 * p.V + v];
            p.u_strk[i] = make_int4(p.sRow0[sidx] + ((int)i - p.sTrk0[sidx]) * Tp, 1, Tp, sidx);
        } else if (sec >= 16) {
            const int l = sec - 16 + 1;  // conv l reads level l and writes level l + 1: this is the table of its INPUT rows
            if (!p.imap[l - 1]) return;
            const int* pre = p.vRow0 + l * (p.V + 1);
            if (i >= pre[p.V]) return;
            const int v = seg_of(pre, p.V, (int)i);
            const int local = (int)i - pre[v];
            const int T_in = p.vT[l * p.V + v], T_out = p.vT[(l + 1) * p.V + v];
            const int n = local / T_in, ti = local - n * T_in;
            p.imap[l - 1][i] = make_int4(p.vRow0[(l + 1) * (p.V + 1) + v] + n * T_out, T_out, ti, 0);
        } else {
            if (i >= p.S) return;
            const int v = p.sVid[i];
            const int rows = p.vN[v] * p.vT[6 * p.V + v];
            const int W = p.sL[i] + p.n_neg;
            p.u_smp[i] = make_int4(p.sRow0[i], 1, rows, (int)i);
            p.u_lang[i] = make_int4(p.sLin0[i], p.sL[i], p.sLrow0[i], W);
            p.u_langk[i] = make_int4(p.sLrow0[i], 1, W, 0);
            p.u_gather[i] = make_int4(p.sRow0[i], p.vRow0[6 * (p.V + 1) + v], rows, 0);
        }
    }
}

}  // namespace

// ---- host-side shape bookkeeping ---------------------------------------------------------------------------------
int rag_shape(const SolaCtx* c, const SolaRaggedBatch* b, RagShape& r) {
    SOLA_ARG(b && b->n_videos > 0 && b->n_samples > 0 && b->video_tracks && b->video_frames && b->sample_video && b->sample_text_len,
             "ragged batch: null or empty descriptor");
    r.V = b->n_videos; r.S = b->n_samples;
    for (int j = 0; j < 7; ++j) { r.vT[j].resize(r.V); r.vRow0[j].assign(r.V + 1, 0); }
    r.vN.resize(r.V); r.vTrk0.assign(r.V + 1, 0); r.vTp0.assign(r.V + 1, 0);
    for (int v = 0; v < r.V; ++v) {
        const int N = b->video_tracks[v], T = b->video_frames[v];
        SOLA_ARG(N >= 1 && T >= 1, "ragged batch: video %d has N=%d T=%d", v, N, T);
        r.vN[v] = N;
        int t = T;
        r.vT[0][v] = t;
        for (int i = 0; i < 6; ++i) {
            t = (t + 2 * c->conv[i].pad - c->conv[i].k) / c->conv[i].stride + 1;
            SOLA_ARG(t >= 1, "ragged batch: video %d (T=%d) is shorter than the encoder's receptive field", v, T);
            r.vT[i + 1][v] = t;
        }
        for (int j = 0; j < 7; ++j) {
            const long long next = (long long)r.vRow0[j][v] + (long long)N * r.vT[j][v];
            SOLA_ARG(next < (1ll << 31), "ragged batch: more than 2^31 token rows");
            r.vRow0[j][v + 1] = (int)next;
            r.maxT[j] = std::max(r.maxT[j], r.vT[j][v]);
        }
        r.vTrk0[v + 1] = r.vTrk0[v] + N;
        r.vTp0[v + 1] = r.vTp0[v] + r.vT[6][v];
        r.maxN = std::max(r.maxN, N);
    }
    for (int j = 0; j < 7; ++j) r.rows[j] = r.vRow0[j][r.V];
    r.NT = r.vTrk0[r.V]; r.Mv = r.rows[6]; r.sumTpV = r.vTp0[r.V];
    r.sVid.resize(r.S); r.sL.resize(r.S);
    r.sLin0.assign(r.S + 1, 0); r.sLrow0.assign(r.S + 1, 0); r.sTrk0.assign(r.S + 1, 0); r.sRow0.assign(r.S + 1, 0); r.sTp0.assign(r.S + 1, 0);
    r.identity = r.S == r.V;
    for (int i = 0; i < r.S; ++i) {
        const int v = b->sample_video[i], L = b->sample_text_len[i];
        SOLA_ARG(v >= 0 && v < r.V && L >= 1, "ragged batch: sample %d has video=%d L=%d", i, v, L);
        r.sVid[i] = v; r.sL[i] = L;
        const int W = L + c->cfg.n_negative;
        const int rows = r.vN[v] * r.vT[6][v];
        const long long next = (long long)r.sRow0[i] + rows;
        SOLA_ARG(next < (1ll << 31), "ragged batch: more than 2^31 token rows");
        r.sLin0[i + 1] = r.sLin0[i] + L;
        r.sLrow0[i + 1] = r.sLrow0[i] + W;
        r.sTrk0[i + 1] = r.sTrk0[i] + r.vN[v];
        r.sRow0[i + 1] = (int)next;
        r.sTp0[i + 1] = r.sTp0[i] + r.vT[6][v];
        r.maxW = std::max(r.maxW, W);
        r.maxRowsSample = std::max(r.maxRowsSample, rows);
        if (v != i) r.identity = false;
    }
    r.Ms = r.sRow0[r.S]; r.LW = r.sLrow0[r.S]; r.Lin = r.sLin0[r.S];
    r.sumTpS = r.sTp0[r.S]; r.sumNS = r.sTrk0[r.S];
    return SOLA_OK;
}

// slots of the sliced GroupNorm shape: a launch has (instances x 8 groups x slices of the LONGEST unit) blocks of 8 bytes; the
// object->language norm has one instance per sample (up to maxRowsSample tokens), the encoder norms one per track (up to
// maxT[1] tokens); slices are at least 128 tokens
size_t rag_gn_slots_bytes(const RagShape& r) {
    const size_t a = (size_t)r.S * ((size_t)r.maxRowsSample / 128 + 1);
    const size_t b = (size_t)r.NT * ((size_t)r.maxT[1] / 128 + 1);
    const size_t t = (size_t)std::max(r.sumTpV, r.sumTpS) * ((size_t)r.maxN / 128 + 1);  // inter-object norm: one instance per (sample, t')
    return 8 * 8 * std::max(a, std::max(b, t)) + 4096;
}

namespace {

size_t blob_ints(const RagShape& r) { return (size_t)r.V * 8 + (size_t)(r.V + 1) * 9 + (size_t)r.S * 2 + (size_t)(r.S + 1) * 5; }

// pinned staging for the descriptor upload: a small ring, a slot is reused only after the copy that read it has completed
struct RagStage {
    static constexpr int SLOTS = 4;
    int* host[SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev[SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    bool used[SLOTS] = {false, false, false, false};
    size_t cap = 0;
    int next = 0;
};

}  // namespace

struct SolaRagStage : RagStage {};

void sola_rag_stage_free(SolaRagStage* st) {
    if (!st) return;
    for (int i = 0; i < RagStage::SLOTS; ++i) {
        if (st->host[i]) (void)hipHostFree(st->host[i]);
        if (st->ev[i]) (void)hipEventDestroy(st->ev[i]);
    }
    delete st;
}

static int stage_slot(SolaCtx* c, size_t ints, int** host, hipEvent_t* ev) {
    if (!c->rag_stage) c->rag_stage = new SolaRagStage();
    RagStage* st = c->rag_stage;
    if (ints > st->cap) {
        for (int i = 0; i < RagStage::SLOTS; ++i) {
            if (st->used[i]) SOLA_HIP(hipEventSynchronize(st->ev[i]));
            if (st->host[i]) SOLA_HIP(hipHostFree(st->host[i]));
            st->host[i] = nullptr;
            st->used[i] = false;
        }
        st->cap = std::max<size_t>(ints * 2, 16384);
        for (int i = 0; i < RagStage::SLOTS; ++i) SOLA_HIP(hipHostMalloc(reinterpret_cast<void**>(&st->host[i]), st->cap * sizeof(int), hipHostMallocDefault));
    }
    const int i = st->next;
    st->next = (st->next + 1) % RagStage::SLOTS;
    if (!st->ev[i]) SOLA_HIP(hipEventCreateWithFlags(&st->ev[i], hipEventDisableTiming));
    if (st->used[i]) SOLA_HIP(hipEventSynchronize(st->ev[i]));
    st->used[i] = true;
    *host = st->host[i];
    *ev = st->ev[i];
    return SOLA_OK;
}

namespace {
size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
// walks the table region in a fixed order; `visit(name index, bytes)` returns nothing, offsets accumulate
struct TableLayout {
    size_t blob, u_lvl[7], rowmap[5], imap[5], u_vt, u_st, u_strk, u_smp, u_lang, u_langk, u_gather, total;
};
TableLayout table_layout(const RagShape& r, bool train) {
    TableLayout t{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += al256(bytes); return at; };
    t.blob = take(blob_ints(r) * sizeof(int));
    for (int j = 0; j < 7; ++j) t.u_lvl[j] = take((size_t)r.NT * sizeof(int4));
    for (int l = 0; l < 5; ++l) t.rowmap[l] = take((size_t)r.rows[l + 1] * sizeof(int2));
    for (int l = 0; l < 5; ++l) t.imap[l] = train ? take((size_t)r.rows[l + 1] * sizeof(int4)) : 0;
    t.u_vt = take((size_t)r.sumTpV * sizeof(int4));
    t.u_st = take((size_t)r.sumTpS * sizeof(int4));
    t.u_strk = take((size_t)r.sumNS * sizeof(int4));
    t.u_smp = take((size_t)r.S * sizeof(int4));
    t.u_lang = take((size_t)r.S * sizeof(int4));
    t.u_langk = take((size_t)r.S * sizeof(int4));
    t.u_gather = take((size_t)r.S * sizeof(int4));
    t.total = o;
    return t;
}
}  // namespace

size_t rag_tables_bytes(const RagShape& r, bool train) { return table_layout(r, train).total; }

int rag_build_tables(SolaCtx* c, const RagShape& r, char* base, bool train, RagTables* out, hipStream_t s) {
    SOLA_ARG(c && base && out && (reinterpret_cast<uintptr_t>(base) & 255) == 0, "ragged tables: bad arguments");
    const TableLayout t = table_layout(r, train);
    int* host;
    hipEvent_t ev;
    SOLA_TRY(stage_slot(c, blob_ints(r), &host, &ev));
    int* w = host;
    int* const blob = reinterpret_cast<int*>(base + t.blob);
    auto put = [&](const std::vector<int>& v) { const int* at = blob + (w - host); memcpy(w, v.data(), v.size() * sizeof(int)); w += v.size(); return at; };
    RagDev dv{};
    dv.vN = put(r.vN);
    dv.vT = blob + (w - host);
    for (int j = 0; j < 7; ++j) put(r.vT[j]);
    dv.vRow0 = blob + (w - host);
    for (int j = 0; j < 7; ++j) put(r.vRow0[j]);
    dv.vTrk0 = put(r.vTrk0); dv.vTp0 = put(r.vTp0);
    dv.sVid = put(r.sVid); dv.sL = put(r.sL); dv.sLin0 = put(r.sLin0); dv.sLrow0 = put(r.sLrow0);
    dv.sTrk0 = put(r.sTrk0); dv.sRow0 = put(r.sRow0); dv.sTp0 = put(r.sTp0);
    SOLA_HIP(hipMemcpyAsync(blob, host, (size_t)(w - host) * sizeof(int), hipMemcpyHostToDevice, s));
    SOLA_HIP(hipEventRecord(ev, s));
    dv.V = r.V; dv.S = r.S; dv.NT = r.NT; dv.n_neg = c->cfg.n_negative;
    for (int l = 0; l < 5; ++l) { dv.stride[l] = c->conv[l].stride; dv.pad[l] = c->conv[l].pad; dv.k[l] = c->conv[l].k; }
    auto t4 = [&](size_t off) { return reinterpret_cast<int4*>(base + off); };
    for (int j = 0; j < 7; ++j) dv.u_lvl[j] = t4(t.u_lvl[j]);
    for (int l = 0; l < 5; ++l) dv.rowmap[l] = reinterpret_cast<int2*>(base + t.rowmap[l]);
    for (int l = 0; l < 5; ++l) dv.imap[l] = train ? t4(t.imap[l]) : nullptr;
    dv.u_vt = t4(t.u_vt); dv.u_st = t4(t.u_st); dv.u_strk = t4(t.u_strk); dv.u_smp = t4(t.u_smp);
    dv.u_lang = t4(t.u_lang); dv.u_langk = t4(t.u_langk); dv.u_gather = t4(t.u_gather);
    long long biggest = std::max<long long>(r.NT, r.rows[1]);
    biggest = std::max<long long>(biggest, std::max<long long>(r.sumNS, std::max(r.sumTpS, r.sumTpV)));
    const unsigned bx = (unsigned)std::min<long long>(2048, (biggest + 255) / 256);
    {
        SolaProfScope prof(SOLA_PROF_MISC, s, 0, 0);
        hipLaunchKernelGGL(ragged_plan_kernel, dim3(bx, train ? 21 : 16), dim3(256), 0, s, dv);
        SOLA_LAUNCH_CHECK();
    }
    RagTables& o = *out;
    for (int j = 0; j < 7; ++j) o.u_lvl[j] = dv.u_lvl[j];
    for (int l = 0; l < 5; ++l) { o.rowmap[l] = dv.rowmap[l]; o.imap[l] = dv.imap[l]; }
    o.u_vt = dv.u_vt; o.u_st = dv.u_st; o.u_strk = dv.u_strk; o.u_smp = dv.u_smp;
    o.u_lang = dv.u_lang; o.u_langk = dv.u_langk; o.u_gather = dv.u_gather;
    o.trk_off = dv.sTrk0;
    o.V = r.V; o.S = r.S; o.NT = r.NT; o.sumNS = r.sumNS; o.sumTpV = r.sumTpV; o.sumTpS = r.sumTpS;
    o.maxN = r.maxN; o.maxW = r.maxW; o.maxRowsSample = r.maxRowsSample;
    for (int j = 0; j < 7; ++j) { o.maxT[j] = r.maxT[j]; o.rows[j] = r.rows[j]; }
    o.Mv = r.Mv; o.Ms = r.Ms; o.LW = r.LW; o.Lin = r.Lin; o.identity = r.identity;
    return SOLA_OK;
}

