// The sola_tune keys of the library, one line per key: api.hip makes the `extern int` declarations and the table that sola_tune,
// sola_tune_query and sola_tune_key scan from these lists and from nothing else.  What a key's values mean is in docs/tune_keys.md.
//
//   P(key)                  plain: sola_tune assigns the argument to the global `int g_<key>`.  That global is DEFINED in the file
//                           that reads it, with its default and its comment - the only place the default is written.
//   S(key, setter, report)  the setter clamps the argument or writes two globals; `report` is the argument that, handed back to
//                           sola_tune, leaves the library as it is now (sola_tune_query's `value`).
//
// "gemm_splitk" reports `on ? tiles : 0`: 0 switches the split off and keeps the tile threshold, an argument above 1 switches it on and
// is the threshold, so set(8), set(0), set(what the query gave before each) walks back through (on, 8) to the first state.  While the
// split is off nothing reads the threshold, and a borrower that found it off hands it back off with whatever threshold it set itself.
#pragma once

void sola_attn_set_spin(int);            // attn_simple.hip
void sola_gemm_set_splitk(int);          // gemm.hip
void sola_gemm_set_splitk_max(int);      // gemm.hip
void sola_attn_set_f16_qpb(int);         // attn_f16.hip
void sola_attn_set_res_tiles(int);       // attn_res.hip
void sola_attn_set_ring_blocks(int);     // lab/attn_ring.hip (EXPERIMENTS)
extern int g_attn_spin, g_attn_spin_db, g_gemm_splitk, g_gemm_splitk_tiles, g_gemm_splitk_max, g_attn_f16_qpb, g_attn_res_tiles,
    g_attn_ring_blocks;
// "attn_stage_split_math" is a static of api.hip, defined there in front of the table

#define SOLA_TUNE_KEYS(P, S) \
    S(attn_stage_split_math, sola_set_stage_split_math, g_stage_split_math) \
    P(gemm_variant) \
    P(gemm_glds) \
    P(bwd_side_rows) \
    P(bwd_group_rows) \
    P(lang_shared_neg) \
    P(train_tn_tr) \
    P(train_x16_keep) \
    P(train_attn_cast) \
    S(gemm_splitk, sola_gemm_set_splitk, g_gemm_splitk ? g_gemm_splitk_tiles : 0) \
    S(gemm_splitk_max, sola_gemm_set_splitk_max, g_gemm_splitk_max) \
    P(gemm_small_rows) \
    P(infer_f32_rows) \
    P(gemm_small_nw8) \
    P(gemm_f32_nw8) \
    P(gemm_f32_persist) \
    P(gemm_tn_nw8) \
    P(gemm_tn_persist) \
    P(gemm_glds_force) \
    P(train_split_min_rows) \
    P(gemm_persist) \
    P(gn_variant) \
    P(bilinear_staged) \
    P(attn_variant) \
    P(attn_target_blocks) \
    P(iou_fused) \
    P(iou_shape) \
    P(train_bf16_store) \
    P(attn_bf16_mfma) \
    P(attn_bwd_bf16_mfma) \
    P(train_gn_stats) \
    P(gemm_slack_stagger) \
    P(iou_packed) \
    P(attn_split_min_keys) \
    P(attn_splitm) \
    P(attn_reg) \
    P(attn_res) \
    S(attn_res_tiles, sola_attn_set_res_tiles, g_attn_res_tiles) \
    P(attn_res_shape) \
    P(attn_bwd_small) \
    P(attn_bwd_blk) \
    P(attn_bwd_rag_wave) \
    P(attn_bwd_fused) \
    P(attn_f16_small) \
    P(gn_h8) \
    S(attn_spin, sola_attn_set_spin, !g_attn_spin ? 0 : g_attn_spin_db ? 1 : 2) \
    P(train_dw_f16) \
    P(train_gn_cast) \
    P(attn_simple_train) \
    P(gn_bwd_reg) \
    P(gn_slices) \
    P(gn_wide) \
    P(bwd_dual_cast) \
    S(attn_f16_qpb, sola_attn_set_f16_qpb, g_attn_f16_qpb) \
    P(bwd_fused_bf16_cast) \
    P(attn_simple_remap) \
    P(attn_simple_db) \
    P(pack_resample_lds)

// closed experiments and measurement switches: EXPERIMENTS=1 builds only (make -C sola_amd/csrc EXPERIMENTS=1)
#define SOLA_TUNE_EXPERIMENT_KEYS(P, S) \
    P(gemm_f32p_ablate) \
    P(gemm_pp) \
    P(gemm_nw4) \
    P(gemm_k16) \
    P(gemm_stagger) \
    P(gemm_order) \
    P(gemm_trace) \
    P(gemm_ld) \
    P(gemm_ablate) \
    P(attn_reg_minw) \
    P(attn_res_splitm) \
    P(attn_ring) \
    S(attn_ring_blocks, sola_attn_set_ring_blocks, g_attn_ring_blocks) \
    P(attn_ring_remap) \
    P(attn_ring_ablate) \
    P(attn_bwd_ablate) \
    P(gemm_gn_fuse)
