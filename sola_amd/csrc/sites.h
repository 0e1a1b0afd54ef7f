// The three sites of an alignment layer (module/module.py:22-52) - 0: inter-object attention over the N tracks of each (sample, t'),
// 1: motion attention over the T' steps of each track, 2: object -> language attention of a sample's N * T' rows over its text ++
// negative rows - and their unit geometry, stated once for the training forward (forward.hip), both inference forwards
// (forward_infer.hip) and the backward (backward.hip).  A site is projection GEMM -> attention -> out-projection (+ residual) ->
// GroupNorm; the attention's query units and the norm's instances are the SAME family of row sets, which the attention backward, the
// norm backward and - for the track family - the score head walk too: strided over the one [B, N, T', D] layout, or a unit table of
// ragged.hip.  Under a table the strides are dead (attn_common.h: attn_unit, gn_common.h: gn_unit take first row,
// row stride and length from the entry; the host predicates test the table first) and every caller gets inner 1, row stride 1, rest 0.
#pragma once
#include <type_traits>

#include "ctx.h"

// n row sets; set g holds the rows first(g) + i * row_stride, i < len, first(g) = (g / inner) * outer + (g % inner) * inner_stride -
// or, with units, what units[g] = (first row, row stride, length, -) says, len then being the LONGEST length (it selects kernel shapes)
struct RowFamily {
    int n = 0, inner = 1;
    long long outer = 0, inner_stride = 0, row_stride = 1;
    int len = 0;
    const int4* units = nullptr;
};

// Where the families come from: a uniform batch, the samples of a ragged batch, or its videos (sites 0 and 1 only: what layer 0
// computes once per video in front of the gather).  B / N are the head's [B, N] (ragged: 1 x all tracks).
struct SiteShape {
    RowFamily fam[3], keys;  // query family per site; key family of site 2 (sites 0 and 1 attend their own rows)
    int k_private = 0;       // AttnDesc::k_private / k_shared_row: the negatives' key rows stored once behind all samples' text rows
    long long k_shared_row = 0;
    int B = 0, N = 0;
};

inline RowFamily site_table(int n, int longest, const int4* units) { return RowFamily{n, 1, 0, 0, 1, longest, units}; }
// the track family at an encoder level - R tracks of T consecutive tokens, or the ragged batch's tracks at `level` (0 = the object tokens):
// the encoder norms' instances, and at level 6 (T') the units of site 1
inline RowFamily site_tracks(int R, int T) { return RowFamily{R, 1, T, 0, 1, T, nullptr}; }
inline RowFamily site_tracks(const RagTables& t, int level) { return site_table(t.NT, t.maxT[level], t.u_lvl[level]); }
// shared_L > 0: the text rows are [B * L own | n_negative shared] (uniform inference, launch_lang_concat_shared)
inline SiteShape site_shape_uniform(int B, int N, int Tp, int W, int shared_L = 0) {
    SiteShape z;
    const long long NT = (long long)N * Tp;
    z.fam[0] = RowFamily{B * Tp, Tp, NT, 1, Tp, N, nullptr};
    z.fam[1] = site_tracks(B * N, Tp);
    z.fam[2] = RowFamily{B, 1, NT, 0, 1, N * Tp, nullptr};
    z.keys = RowFamily{B, 1, shared_L ? shared_L : W, 0, 1, W, nullptr};
    if (shared_L) { z.k_private = shared_L; z.k_shared_row = (long long)B * shared_L; }
    z.B = B; z.N = N;
    return z;
}
inline SiteShape site_shape_samples(const RagTables& t) {
    SiteShape z;
    z.fam[0] = site_table(t.sumTpS, t.maxN, t.u_st);
    z.fam[1] = site_table(t.sumNS, t.maxT[6], t.u_strk);
    z.fam[2] = site_table(t.S, t.maxRowsSample, t.u_smp);
    z.keys = site_table(t.S, t.maxW, t.u_langk);
    z.B = 1; z.N = t.sumNS;
    return z;
}
inline SiteShape site_shape_videos(const RagTables& t) {
    SiteShape z;
    z.fam[0] = site_table(t.sumTpV, t.maxN, t.u_vt);
    z.fam[1] = site_tracks(t, 6);
    return z;
}

struct SiteGeom { RowFamily q, k; int k_private; long long k_shared_row; };  // k is q at sites 0 and 1
inline SiteGeom site_geom(const SiteShape& z, int a) {
    return a == 2 ? SiteGeom{z.fam[2], z.keys, z.k_private, z.k_shared_row} : SiteGeom{z.fam[a], z.fam[a], 0, 0};
}

// ---- the descriptors' geometry members, by their shared names (in the manner of attn_fill_common) -----------------------------
template <class D>  // AttnDesc / AttnBwdDesc
void site_fill_attn(D& d, const SiteGeom& g) {
    d.G = g.q.n; d.Sq = g.q.len; d.Sk = g.k.len; d.inner = g.q.inner;
    d.q_outer = g.q.outer; d.q_inner = g.q.inner_stride; d.q_rs = g.q.row_stride;
    d.k_outer = g.k.outer; d.k_inner = g.k.inner_stride; d.k_rs = g.k.row_stride;
    d.q_units = g.q.units; d.k_units = g.k.units == g.q.units ? nullptr : g.k.units;  // self-attention: attn_fill_common's fallback
    if constexpr (std::is_same<D, AttnDesc>::value) { d.k_private = g.k_private; d.k_shared_row = g.k_shared_row; }
}
template <class D>  // GroupNormDesc / GroupNormBwdDesc
void site_fill_norm(D& d, const RowFamily& f) {
    d.n_inst = f.n; d.inner = f.inner; d.outer_stride = f.outer; d.inner_stride = f.inner_stride; d.tok_stride = f.row_stride;
    d.ntok = f.len; d.units = f.units;
}
template <class D>  // HeadDesc / HeadBwdDesc: the track family
void site_fill_head(D& d, const SiteShape& z) { d.B = z.B; d.N = z.N; d.Tp = z.fam[1].len; d.units = z.fam[1].units; }
