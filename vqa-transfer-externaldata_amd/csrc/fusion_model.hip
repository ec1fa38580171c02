// Host-side composition of the fusion model's forward and backward passes:
// one call enqueues every kernel of a step on the caller's stream.
//
// Forward  = vqa/model_vlmap_answer.py:102-288 (model_standard.py:193-374):
//   feature gather -> v_linear_v -> embedding -> GRU -> q_linear_v -> Hadamard
//   attention + pooling -> pooled_linear_l / q_linear_l -> joint_fc (+dropout) ->
//   answer head -> sigmoid-CE loss, argmax, report.
// Backward = the autodiff that tf.contrib.layers.optimize_loss builds
//   (vqa/trainer.py:106-114), hand-derived; frozen variables of model_vlmap_answer
//   (filter_train_vars, model_vlmap_answer.py:81-89) still propagate dX.
//
// Workspace layout is computed from the dims alone, so the host can view named
// intermediates (mid_result / output of the reference Model) without copies.
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "gemm_args.h"
#include "gru_encoder.h"
#include "keep_launch.h"

namespace {

// properties that several model types share (include/vqa_hot.h: VQA_MODEL_*)
inline bool has_tuned_head(int mt) { return mt == VQA_MODEL_VQA_ALL2 || mt == VQA_MODEL_VQA_ALL; }      // a second, trainable head on `joint`
inline bool train_loss_masked(int mt) { return mt != VQA_MODEL_STANDARD; }      // train loss masked by the train-answer mask
inline bool bf16_routed(int mt) { return mt == VQA_MODEL_VLMAP_ANSWER || mt == VQA_MODEL_STANDARD; }      // every dense product on VQA_FLAG_BF16_GEMM's routed list
inline bool feat16(const vqa_dims_t& d) { return (d.flags & VQA_FLAG_BF16_FEATURES) != 0; }      // table and V_ft are bf16 patterns
inline bool enc16(const vqa_dims_t& d) { return (d.flags & VQA_FLAG_BF16_ENCODER_GEMMS) != 0; }      // the encoder's five single products are routed

void legacy_vqa_layout(Layout& L, const vqa_dims_t& d, int64_t& gw);      // csrc/legacy_vqa.inc (model_type 13)

Layout make_layout(const vqa_dims_t& d) {
    Layout L;
    const int64_t B = d.B, R = d.R, D = d.D, H = d.H, T = d.T, W = d.W, A = d.A;
    L.add("V_ft", B * R * D, feat16(d) ? 2 : 4);
    L.add("num_V_ft", B);
    L.add("pre_v", B * R * H);
    L.add("v_linear_v", B * R * H);
    L.add("mean_v", B); L.add("rstd_v", B);
    const int64_t Wp = x_stride(W);
    L.add("x_tm", T * B * Wp);
    L.add("xp", T * B * 3 * H);
    L.add("wx_cat", W * 3 * H); L.add("bx_cat", 3 * H); L.add("dwx_cat", Wp * 3 * H);
    L.add("hs", (T + 1) * B * H);
    L.add("gru_r", T * B * H); L.add("gru_u", T * B * H); L.add("gru_c", T * B * H); L.add("gru_rh", T * B * H);
    // hand-off buffers and flags of the weight-stationary recurrence (csrc/gru_ws.hip), where its shape limits hold
    if (H == 1024 && B <= 512) L.add("gru_ws", vqa_gru_ws_workspace_bytes((int)T) / 4);
    L.add("pre_qv", B * H); L.add("q_linear_v", B * H); L.add("mean_qv", B); L.add("rstd_qv", B);
    L.add("att_score", B * R);
    const int64_t Dp = d.model_type == VQA_MODEL_ADAPT ? H : D;      // width of what the attention pools (pooled_dim)
    L.add("pooled_V_ft", B * Dp);
    L.add("pre_pl", B * H); L.add("pooled_linear_l", B * H); L.add("mean_pl", B); L.add("rstd_pl", B);
    L.add("pre_ll", B * H); L.add("l_linear_l", B * H); L.add("mean_ll", B); L.add("rstd_ll", B);
    L.add("joint_in", B * H);
    L.add("pre_j", B * 2 * H); L.add("joint", B * 2 * H); L.add("mean_j", B); L.add("rstd_j", B);
    L.add("joint2", B * W);      // standard_word2vec: classifier output in the 300-d word space
    L.add("logit", B * A);
    if (d.model_type == VQA_MODEL_NOC) {     // vlmap_answer_noc: the l_joint branch ("joint" is v_joint)
        L.add("pre_jl", B * 2 * H); L.add("l_joint", B * 2 * H); L.add("mean_jl", B); L.add("rstd_jl", B);
        L.add("d_ljoint", B * 2 * H); L.add("d_pre_jl", B * 2 * H);
    }
    if (has_tuned_head(d.model_type)) {     // vlmap_answer_vqa_all2 / _vqa_all: the two heads' logits ("logit" = their sum), the tuned head's dz
        L.add("logit_fixed", B * A); L.add("logit_tuned", B * A); L.add("dlogit_tuned", B * A);
    }
    if (d.model_type == VQA_MODEL_VQA_ALL) { L.add("logit_raw", B * A); L.add("rowmin", B); }      // before the row-minimum substitution
    // the five older ablations (vqa_hot.h: VQA_MODEL_*)
    if (d.model_type == VQA_MODEL_ANSWER2) {
        L.add("pre_ft2", B * H); L.add("q_L_ft2", B * H); L.add("mean_ft2", B); L.add("rstd_ft2", B);
        L.add("d_ft2", B * H); L.add("d_pre_ft2", B * H);
    }
    if (d.model_type == VQA_MODEL_NO_NOISE || d.model_type == VQA_MODEL_FULL) { L.add("q_L_mean", B * H); L.add("d_qm", B * H); }
    if (d.model_type == VQA_MODEL_FULL) {
        L.add("q_L_log_sigma_sq", B * H); L.add("q_L_mean_noise", B * H); L.add("d_qs", B * H); L.add("d_lin", B * H);
    }
    if (d.model_type == VQA_MODEL_FULL || d.model_type == VQA_MODEL_ENT) L.add("extra_row", B);
    if (d.model_type == VQA_MODEL_ADAPT) {
        L.add("pre_va", B * R * H); L.add("v_adapt", B * R * H); L.add("mean_va", B); L.add("rstd_va", B);
        L.add("d_va", B * R * H); L.add("d_pre_va", B * R * H);
    }
    if (d.model_type == VQA_MODEL_BI) {
        // bi-directional question encoder + question self-attention (the forward cell reuses x_tm / xp / hs / gru_* / dxp /
        // wx_cat / bx_cat / dwx_cat above with h = H / 2 columns; the backward cell gets its own)
        const int64_t h = H / 2, Wq = x_stride(W);
        L.add("q_rev", B * T);
        L.add("x_tm_bw", T * B * Wq); L.add("xp_bw", T * B * 3 * h);
        L.add("wx_cat_bw", W * 3 * h); L.add("bx_cat_bw", 3 * h); L.add("dwx_cat_bw", Wq * 3 * h);
        L.add("hs_bw", (T + 1) * B * h);
        L.add("gru_r_bw", T * B * h); L.add("gru_u_bw", T * B * h); L.add("gru_c_bw", T * B * h); L.add("gru_rh_bw", T * B * h);
        L.add("q_L_map", B * T * H); L.add("q_L_ft", B * H);
        L.add("pre_key", B * T * H); L.add("q_att_key", B * T * H); L.add("mean_key", B); L.add("rstd_key", B);
        L.add("pre_query", B * H); L.add("q_att_query", B * H); L.add("mean_query", B); L.add("rstd_query", B);
        L.add("w_att_score", B * T);
        L.add("e2", B * T * W); L.add("pre_vw", B * T * H); L.add("q_v_ft", B * T * H); L.add("mean_vw", B); L.add("rstd_vw", B);
        L.add("pooled_q_v", B * H);
        L.add("d_pooled_qv", B * H); L.add("d_key", B * T * H); L.add("d_pre_key", B * T * H);
        L.add("d_query", B * H); L.add("d_pre_query", B * H);
        L.add("d_qvft", B * T * H); L.add("d_pre_vw", B * T * H); L.add("d_e2", B * T * W); L.add("sq_e2", 4);
        L.add("d_qmap", B * T * H);
        L.add("dout_fw", T * B * h); L.add("dout_bw", T * B * h);
        L.add("dhT_fw", B * h); L.add("dhT_bw", B * h); L.add("dhS_fw", B * h); L.add("dhS_bw", B * h);
        L.add("dxp_bw", T * B * 3 * h); L.add("dx_fw", T * B * W); L.add("dx_bw", T * B * W);
        L.add("part_wdw", B * H); L.add("part_wdb", B);
    }
    if (d.model_type == VQA_MODEL_ENT) {
        const int64_t M = d.num_marginal, C = d.ent_cols;
        L.add("tile_in", B * M * H); L.add("pre_tj", B * M * 2 * H); L.add("tile_joint", B * M * 2 * H);
        L.add("mean_tj", B); L.add("rstd_tj", B);
        L.add("tile_z", B * M * C); L.add("marginal_prob", B * C);
        L.add("d_tile_joint", B * M * 2 * H); L.add("d_pre_tj", B * M * 2 * H); L.add("d_tile_in", B * M * H);
    }
    L.add("stats", B * VQA_STAT_COUNT);
    L.add("pred", B);
    L.add("report", 16);
    L.add("dlogit", B * A);
    // backward scratch
    L.add("d_joint2", B * W);
    L.add("d_joint", B * 2 * H); L.add("d_pre_j", B * 2 * H);
    L.add("d_joint_in", B * H);
    L.add("d_pl", B * H); L.add("d_ll", B * H); L.add("d_pre_pl", B * H); L.add("d_pre_ll", B * H);
    L.add("d_pooled", B * Dp);
    L.add("d_h0", B * H); L.add("d_h1", B * H);
    L.add("d_v", B * R * H); L.add("d_pre_v", B * R * H);
    L.add("d_qv", B * H); L.add("d_pre_qv", B * H);
    L.add("part_a", B * 2 * H); L.add("part_b", B * 2 * H); L.add("part_c", B * 2 * H);
    L.add("part_dw", B * H); L.add("part_db", B);
    L.add("ds", B * R);          // gradient of the raw attention scores (the fused v_linear_v chain, vtail_mode)
    L.add("dxp", T * B * 3 * H);
    L.add("d_rh", B * H);
    L.add("dx_embed", T * B * W);
    // shared scratch: split-k slabs, colsum partials, sumsq partials
    int64_t gw = 0;
    auto g = [&](int tA, int tB, int64_t M, int64_t N, int64_t K) {
        gw = max64(gw, vqa_gemm_workspace_floats(tA, tB, (int)M, (int)N, (int)K, 0));
        if (d.flags & VQA_FLAG_BF16_GEMM) gw = max64(gw, vqa_gemm_bf16_workspace_floats((int)M, (int)N, (int)K, 0));
    };
    g(0, 0, B * R, H, D); g(0, 0, T * B, 2 * H, W); g(0, 0, T * B, H, W); g(0, 0, B, H, H); g(0, 0, B, H, D);
    g(0, 0, B, 2 * H, H); g(0, 0, B, A, 2 * H);                                   // forward
    g(0, 1, B, 2 * H, A); g(1, 0, 2 * H, A, B); g(0, 1, B, H, 2 * H); g(1, 0, H, 2 * H, B); g(0, 1, B, D, H);
    g(1, 0, D, H, B); g(1, 0, H, H, B); g(0, 1, B, H, H); g(1, 0, D, H, B * R); g(1, 0, W, 2 * H, T * B);
    g(1, 0, H, 2 * H, T * B); g(1, 0, W, H, T * B); g(1, 0, H, H, T * B); g(0, 1, T * B, W, 2 * H);
    g(0, 1, T * B, W, H);                                                         // backward
    g(0, 0, T * B, 3 * H, W); g(0, 1, T * B, W, 3 * H); g(1, 0, W, 3 * H, T * B);  // packed x-projection
    g(1, 0, Wp, 3 * H, T * B);
    g(0, 0, B, W, 2 * H); g(0, 0, B, A, W); g(0, 1, B, W, A); g(1, 0, 2 * H, W, B); g(0, 1, B, 2 * H, W);  // word2vec head
    if (d.model_type == VQA_MODEL_BI) {
        const int64_t h = H / 2;
        g(0, 0, T * B, 3 * h, W); g(0, 1, T * B, W, 3 * h); g(1, 0, Wp, 3 * h, T * B); g(1, 0, h, 2 * h, T * B); g(1, 0, h, h, T * B);
        g(0, 0, B * T, H, H); g(0, 1, B * T, H, H); g(1, 0, H, H, B * T);
        g(0, 0, B * T, H, W); g(0, 1, B * T, W, H); g(1, 0, W, H, B * T);
    }
    if (d.model_type == VQA_MODEL_ENT) {
        const int64_t M = d.num_marginal, C = d.ent_cols;
        g(0, 0, B * M, 2 * H, H); g(0, 0, B * M, C, 2 * H); g(0, 1, B * M, 2 * H, C); g(0, 1, B * M, H, 2 * H);
    }
    if (d.model_type == VQA_MODEL_LEGACY_VQA) legacy_vqa_layout(L, d, gw);
    L.add("gemm_ws", max64(gw, 4));
    L.add("gemm_ws1", max64(gw, 4));            // scratch of the side stream (v_linear_v branch)
    int64_t cw = 0;
    cw = max64(cw, vqa_colsum_workspace_floats((int)B, (int)(2 * H)));
    cw = max64(cw, vqa_colsum_workspace_floats((int)(T * B), (int)(3 * H)));
    cw = max64(cw, vqa_colsum_workspace_floats((int)B, (int)A));
    cw = max64(cw, vqa_colsum_workspace_floats((int)B, (int)W));
    cw = max64(cw, vqa_colsum_workspace_floats((int)(B * T), (int)H));
    cw = max64(cw, (vqa_colsum_vtail_workspace_floats((int)B, (int)H) + 2) / 3);
    if (d.model_type == VQA_MODEL_LEGACY_VQA)
        cw = max64(cw, max64(max64(vqa_colsum_workspace_floats((int)(T * B), (int)(4 * H)), vqa_colsum_workspace_floats((int)(d.La * A), (int)(4 * H))),
                             vqa_colsum_workspace_floats((int)A, 1)));
    L.add("colsum_ws", max64(3 * cw, 4));    // x3: vqa_colsum3 reduces three partial matrices per launch
    L.add("colsum_ws1", max64(3 * cw, 4));
    L.add("part_a1", B * H); L.add("part_b1", B * H); L.add("part_c1", B * H);
    L.add("sumsq_ws", max64(vqa_sumsq_workspace_floats(T * B * W), 4));
    L.add("sumsq_ws2", max64(vqa_sumsq_workspace_floats(T * B * W), 4));
    return L;
}

struct Ctx : Workspace {
    const vqa_dims_t& d;
    hipStream_t st;
    int lane;   // 0 = caller's stream, 1 = side stream (own scratch so the two never share a buffer)
    float* gemm_ws() const { return f(lane ? "gemm_ws1" : "gemm_ws"); }
    float* colsum_ws() const { return f(lane ? "colsum_ws1" : "colsum_ws"); }
    float* part(int i) const {
        static const char* const n0[3] = {"part_a", "part_b", "part_c"};
        static const char* const n1[3] = {"part_a1", "part_b1", "part_c1"};
        return f(lane ? n1[i] : n0[i]);
    }
    int64_t gemm_ws_floats() const { return count("gemm_ws"); }
    int64_t colsum_ws_floats() const { return count("colsum_ws"); }
};

// ---- The VQA_HOT_* switches of this file.  Each is read from the environment once per process, at its first use (never
// at load time), and exists for same-box A/B runs: the default is the measured best.
//   VQA_HOT_XCAT=0          question encoder's x-projection, dx and dW as two GEMMs per direction instead of the packed one
//   VQA_HOT_REPACK=1        the backward packs wx_cat again instead of reusing the forward's copy
//   VQA_HOT_GRU_WS=0        never the weight-stationary recurrence: the per-step kernels (gru_form)
//   VQA_HOT_GRU_CHAINS=n    row chains of the per-step recurrence (default 2; 1 = one chain on the caller's stream), and
//   VQA_HOT_GRU_CHAIN_DELAY_US  their anti-phase delay (default 3)                                    -- gru_chains()
//   VQA_HOT_VISUAL_LATE=0   the visual branch in front of the question branch (the round-1 order)
//   VQA_HOT_OVERLAP=1       the visual branch / v_linear_v's backward on a side stream                -- side_stream()
//   VQA_HOT_SIDE_BLOCKS=n   workgroup cap of the side stream's GEMMs (default 0 = none)
//   VQA_HOT_GATHER=fused    the feature gather inside v_linear_v's GEMM (anything else: a pass of its own; unset: the flag)
//   VQA_HOT_LN_PAIR=0       pooled_linear_l and q_linear_l as two LayerNorm launches plus the element-wise product
//   VQA_HOT_VTAIL=0         v_linear_v's LayerNorm backward and the score gradient as separate calls (vqa_vtail_set_mode)
//   VQA_HOT_GRU_H0SKIP=n    what the question GRU's zero initial state saves (default 1; vqa_gru_h0skip_set_mode): bit 0 the
//                           matrix streams of step 0 in the weight-stationary recurrence (same results), bit 1 the rows of
//                           step 0 in the two recurrent weight-gradient GEMMs (opt-in: another split-k boundary, so those
//                           two gradients and with them a training run's numbers move at rounding level)
inline bool env_on(const char* name, bool dflt) {
    const char* e = getenv(name);
    return e == nullptr ? dflt : atoi(e) != 0;
}
inline bool xcat_enabled() { static const bool v = env_on("VQA_HOT_XCAT", true); return v; }
inline bool repack_enabled() { static const bool v = env_on("VQA_HOT_REPACK", false); return v; }
inline bool gru_ws_on() { static const bool v = env_on("VQA_HOT_GRU_WS", true); return v; }
inline bool visual_late_enabled() { static const bool v = env_on("VQA_HOT_VISUAL_LATE", true); return v; }
// pooled_linear_l and q_linear_l finish in one launch that also forms their product (vqa_ln_pair_mul_*): two LayerNorm
// launches and the element-wise one less per direction
inline bool ln_pair_enabled() { static const bool v = env_on("VQA_HOT_LN_PAIR", true); return v; }
// The backward of v_linear_v's LayerNorm and of the attention score as one chain (vqa_attn_pool_bwd_ds ->
// vqa_ln_relu_att_bwd -> vqa_colsum_vtail) where it applies (vtail_ok); 0 = the separate calls.  vqa_vtail_set_mode
// overrides the environment, and a negative mode has it read again.
int g_vtail_mode = -1;
inline int vtail_mode() {
    if (g_vtail_mode < 0) g_vtail_mode = env_on("VQA_HOT_VTAIL", true) ? 1 : 0;
    return g_vtail_mode;
}
// fwd_question clears hs[0] itself (dynamic_rnn without an initial state), so h_0 W_g, (r h_0) W_c and the rows of t = 0
// in hs[0..T-1]^T dxp and gru_rh^T dxp_c are zero by construction.  Bit 0: the weight-stationary recurrence is told so
// (vqa_gru_seq_fwd_ws_ex / _bwd_ws_ex, h0_zero); bit 1: the two gru.dwh_gemm calls start at row B of their operands.
// Bit 0 is on by default: it leaves every result as it was.  Bit 1 is measured faster (profiles/r14_h0skip_ab.txt) but sums the
// two gradients in another order, and a training run must compute what it computed: opt-in.
// vqa_gru_h0skip_set_mode overrides the environment, and a negative mode has it read again.
int g_h0skip_mode = -1;
inline int h0skip_mode() {
    if (g_h0skip_mode < 0) {
        const char* e = getenv("VQA_HOT_GRU_H0SKIP");
        g_h0skip_mode = e == nullptr ? 1 : (atoi(e) & 3);
    }
    return g_h0skip_mode;
}
int side_max_blocks() {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("VQA_HOT_SIDE_BLOCKS");
        v = e ? atoi(e) : 0;
    }
    return v;
}
// how V_ft = features[image_idx] is produced: 0 = a gather pass in front of v_linear_v's GEMM, 1 = fused into that GEMM's
// operand load whatever the shape (VQA_FLAG_FUSED_GATHER or VQA_HOT_GATHER=fused), 2 = automatic (the variable unset, the
// flag clear): fused exactly where vqa_gemm_gather_matches_plain() holds, i.e. where the plain product would run the
// tall tile the fused kernel is built on (M >= 2048, N >= 512, K >= 2048, at least 1024 tiles: the same tile and k order,
// so pre_v and everything behind it keep their bits) and the table fits the 32-bit offsets of a buffer descriptor; a pass
// everywhere else.  Any other value of VQA_HOT_GATHER forces the pass.
// Measured at the bench shape (profiles/r22_gather_gemm.txt): plain GEMM 536 us, pass + GEMM 583, fused through offsets
// with the by-product 552 -- the gathered load itself is free (539 without the by-product code), on a cache-resident table
// as on the 2.4 GB one, so lookahead for a cold operand was not built.  What the earlier fused kernel lost against the
// plain one was not Infinity-Cache residency of V_ft: it ran without the SIMD-partner stagger and with a workgroup-
// uniform test around the by-product stores inside its loop.
// A table of 4 GiB or more needs per-lane 64-bit pointers; that form measures 584 us, no better than pass + GEMM, so
// the automatic mode never selects it.  A third form, the gather on a helper stream beside the question branch's
// projection GEMMs, lost 0.13 ms to the cross-stream fork / join (profiles/r2_gather_mode_ab.txt).
int gather_mode(const vqa_dims_t* dims) {
    static int env = -2;
    if (env == -2) {
        const char* e = getenv("VQA_HOT_GATHER");
        env = e == nullptr ? -1 : (strcmp(e, "fused") == 0 ? 1 : 0);
    }
    if (env >= 0) return env;
    return (dims->flags & VQA_FLAG_FUSED_GATHER) ? 1 : 2;
}

// ---- side stream: the v_linear_v branch (one big GEMM) runs beside the latency-bound GRU
// recurrence so its workgroups fill the CUs the small per-step GEMMs leave idle.  Fork/join
// with events keeps everything ordered with respect to the caller's stream (capture-safe).
struct Side {
    hipStream_t s = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    bool ok = false, tried = false;
};
Side& side_stream() {
    static Side sd[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    Side& x = sd[dev & 63];
    if (!x.tried) {
        x.tried = true;
        // Off by default: measured on MI355X the overlap is worth ~1-2 % of the step (both sides are
        // MFMA-bound) while it inflates each overlapped kernel's own duration; VQA_HOT_OVERLAP=1 enables it.
        const char* env = getenv("VQA_HOT_OVERLAP");
        if (env != nullptr && env[0] == '1') {
            x.ok = hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking) == hipSuccess &&
                   hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) == hipSuccess &&
                   hipEventCreateWithFlags(&x.join, hipEventDisableTiming) == hipSuccess;
        }
    }
    return x;
}
// The recurrence is latency-bound (M = batch rows only): every one of its 2 T dependent step kernels pays ~7 us that
// is not matrix work (drain, launch gap, kernel arguments, first tile, fused epilogue) against 7-14 us that is
// (profiles/r3_gru_loop_variants.txt).  The rows of a batch are independent sequences, so the batch is cut into CHAINS
// of rows that run on their own streams with small co-resident workgroups (32x32 tiles, 4 waves: several workgroups
// of different chains share a CU) and -- the point -- in ANTI-PHASE: chain i starts i * delay later, so one chain's
// boundary falls into the other chain's matrix work.  In phase (no delay) both chains compute at half rate and wait
// together, and nothing is gained (profiles/r3_gru_split2.txt: one chain 558 us, two chains in phase 511-540, two chains
// 8-16 us apart 491).  Inside the step the second chain starts behind a cross-stream event anyway, and a small explicit
// delay is enough (profiles/r3_gru_chains.txt: 0 / 3 us 3.592 ms per step, 6 / 10 us 3.602-3.604).
// VQA_HOT_GRU_CHAINS (default 2; 1 = one chain on the caller's stream), VQA_HOT_GRU_CHAIN_DELAY_US (default 3).
struct Chains {
    static constexpr int MAXC = 4;
    hipStream_t s[MAXC] = {};
    hipEvent_t fork = nullptr, join[MAXC] = {};
    int n = 1;
    float delay_us = 3.f;
    bool tried = false;
};
Chains& gru_chains() {
    static Chains ch[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    Chains& x = ch[dev & 63];
    if (!x.tried) {
        x.tried = true;
        const char* e = getenv("VQA_HOT_GRU_CHAINS");
        int want = e ? atoi(e) : 2;
        if (want > Chains::MAXC) want = Chains::MAXC;
        const char* d = getenv("VQA_HOT_GRU_CHAIN_DELAY_US");
        if (d != nullptr) x.delay_us = (float)atof(d);
        bool ok = want > 1 && hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 1; ok && i < want; ++i)
            ok = hipStreamCreateWithFlags(&x.s[i], hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&x.join[i], hipEventDisableTiming) == hipSuccess;
        x.n = ok ? want : 1;
    }
    return x;
}
// rows [lo, hi) of chain i of n over B rows: boundaries on multiples of 32 (the step kernels' row tile)
inline void chain_rows(int64_t B, int n, int i, int64_t* lo, int64_t* hi) {
    const int64_t tiles = (B + 31) / 32;
    const int64_t q = tiles / n, r = tiles % n;
    const int64_t t0 = i * q + (i < r ? i : r), t1 = t0 + q + (i < r ? 1 : 0);
    *lo = t0 * 32 < B ? t0 * 32 : B;
    *hi = t1 * 32 < B ? t1 * 32 : B;
}
// runs fn(chain, row0, rows, stream) for every chain: chain 0 on the caller's stream, chain i > 0 on its own stream behind
// a fork event and a delay of i * delay_us; the caller's stream waits for all of them at the end
template <typename Fn>
int run_chains(const Ctx& c, int64_t B, Fn fn) {
    Chains& ch = gru_chains();
    int n = ch.n;
    while (n > 1 && B < 64 * (int64_t)n) --n;         // at least two row tiles per chain
    if (n <= 1) return fn(0, (int64_t)0, B, c.st);
    if (hipEventRecord(ch.fork, c.st) != hipSuccess) return VQA_ERR_LAUNCH;
    // Whatever fails after the fork, the caller's stream is still ordered behind every side stream that may have work
    // in flight before the error code goes back: the caller owns the workspace and may free or reuse it on return.
    int rc = VQA_OK, launched = 0;
    for (int i = 1; i < n && rc == VQA_OK; ++i) {
        int64_t lo, hi;
        chain_rows(B, n, i, &lo, &hi);
        if (hipStreamWaitEvent(ch.s[i], ch.fork, 0) != hipSuccess) { rc = VQA_ERR_LAUNCH; break; }
        launched = i;
        if (ch.delay_us > 0.f) rc = vqa_stream_delay_us(ch.delay_us * (float)i, ch.s[i]);
        if (rc == VQA_OK) rc = fn(i, lo, hi - lo, ch.s[i]);
    }
    if (rc == VQA_OK) {
        int64_t lo, hi;
        chain_rows(B, n, 0, &lo, &hi);
        rc = fn(0, lo, hi - lo, c.st);
    }
    for (int i = 1; i <= launched; ++i)
        if (hipEventRecord(ch.join[i], ch.s[i]) != hipSuccess || hipStreamWaitEvent(c.st, ch.join[i], 0) != hipSuccess)
            rc = rc == VQA_OK ? VQA_ERR_LAUNCH : rc;
    return rc;
}
bool fork_side(const Ctx& c, Side& sd) {
    if (!sd.ok) return false;
    return hipEventRecord(sd.fork, c.st) == hipSuccess && hipStreamWaitEvent(sd.s, sd.fork, 0) == hipSuccess;
}
bool join_side_record(Side& sd) { return hipEventRecord(sd.join, sd.s) == hipSuccess; }


// The f32 MFMA product, whatever the flags say: without VQA_FLAG_BF16_ENCODER_GEMMS the question encoder's sites
// (x-projection, dx, dwx, dwh) call this one (include/vqa_hot.h, VQA_FLAG_BF16_GEMM: the unrouted list).
int gemm_f32(const Ctx& c, int tA, int tB, int64_t M, int64_t N, int64_t K, const float* A, int lda, const float* B,
             int ldb, float* C, int ldc, const float* bias = nullptr, const float* D = nullptr, int ldd = 0) {
    // side-stream GEMMs: one workgroup per CU (persistent), so the recurrence on the caller's
    // stream keeps finding free LDS / wave slots on every CU
    return vqa_gemm_f32_ex(tA, tB, (int)M, (int)N, (int)K, A, lda, B, ldb, C, ldc, bias, D, ldd, 0, c.gemm_ws(),
                           c.gemm_ws_floats(), c.lane ? side_max_blocks() : 0, c.st);
}
// The dense layers' products (forward, dW, dx): bf16 operands in the matrix unit under VQA_FLAG_BF16_GEMM, else f32.  A
// shape the bf16 kernel refused would be an error, never a silent f32 product.
int gemm(const Ctx& c, int tA, int tB, int64_t M, int64_t N, int64_t K, const float* A, int lda, const float* B,
         int ldb, float* C, int ldc, const float* bias = nullptr, const float* D = nullptr, int ldd = 0) {
    if (c.d.flags & VQA_FLAG_BF16_GEMM)
        return vqa_gemm_bf16(tA, tB, (int)M, (int)N, (int)K, A, lda, B, ldb, C, ldc, bias, D, ldd, 0, c.gemm_ws(),
                             c.gemm_ws_floats(), c.lane ? side_max_blocks() : 0, c.st);
    return gemm_f32(c, tA, tB, M, N, K, A, lda, B, ldb, C, ldc, bias, D, ldd);
}
// A dense layer's product whose LEFT operand is the layer's input x (forward, dW).  Under VQA_FLAG_BF16_FEATURES the
// workspace's V_ft holds bf16 patterns, and the two products that read it (v_linear_v's forward and dW) take the GEMM whose
// left operand is bf16 in HBM; every other x is f32.
int gemm_x(const Ctx& c, int tA, int64_t M, int64_t N, int64_t K, const float* x, int ldx, const float* B, int ldb, float* C,
           int ldc, const float* bias = nullptr) {
    if (feat16(c.d) && x == c.f("V_ft"))
        return vqa_gemm_bf16_a16(tA, 0, (int)M, (int)N, (int)K, c.u16("V_ft"), ldx, B, ldb, C, ldc, bias, nullptr, 0, 0,
                                 c.gemm_ws(), c.gemm_ws_floats(), c.lane ? side_max_blocks() : 0, c.st);
    return gemm(c, tA, 0, M, N, K, x, ldx, B, ldb, C, ldc, bias);
}
int colsum(const Ctx& c, const float* X, int64_t M, int64_t N, int ldx, float* out) {
    return vqa_colsum(X, (int)M, (int)N, ldx, out, c.colsum_ws(), c.colsum_ws_floats(), c.st);
}
// The question encoder's single products (x-projection, dx, dwx, both dwh; never the recurrence): the dense layers' routed
// product under VQA_FLAG_BF16_ENCODER_GEMMS (which implies VQA_FLAG_BF16_GEMM, dims_ok: lane scratch and the side
// stream's max_blocks as for them), else the f32 product, launch for launch what it was.
int gemm_enc(const Ctx& c, int tA, int tB, int64_t M, int64_t N, int64_t K, const float* A, int lda, const float* B,
             int ldb, float* C, int ldc, const float* bias = nullptr, const float* D = nullptr, int ldd = 0) {
    return enc16(c.d) ? gemm(c, tA, tB, M, N, K, A, lda, B, ldb, C, ldc, bias, D, ldd)
                      : gemm_f32(c, tA, tB, M, N, K, A, lda, B, ldb, C, ldc, bias, D, ldd);
}
auto f32(const Ctx& c) { return [&c](auto... a) { return gemm_f32(c, a...); }; }      // gemm_f32 on c as a callable (gru_encoder.h)
auto enc(const Ctx& c) { return [&c](auto... a) { return gemm_enc(c, a...); }; }      // gemm_enc likewise: the question encoder's sites
GruCell fw_cell(const vqa_params_t* p) { return {p->gru_wg, p->gru_bg, p->gru_wc, p->gru_bc}; }
GruCell bw_cell(const vqa_params_t* p) { return {p->gru_bw_wg, p->gru_bw_bg, p->gru_bw_wc, p->gru_bw_bc}; }      // model_type 12

bool dims_ok(const vqa_dims_t* d) {
    if (!(d && d->B > 0 && d->R > 0 && d->D > 0 && d->H > 0 && d->T > 0 && d->W > 0 && d->A > 0 && d->Vq > 0 &&
          d->N_img > 0 && d->model_type >= VQA_MODEL_VLMAP_ANSWER && d->model_type <= VQA_MODEL_LEGACY_VQA))
        return false;
    // bf16 mode: the two model types whose every dense product is on the routed list, and no gather-fused GEMM
    if ((d->flags & VQA_FLAG_BF16_GEMM) && (!bf16_routed(d->model_type) || (d->flags & VQA_FLAG_FUSED_GATHER))) return false;
    // a bf16 table: only inside the bf16 mode (which brings the two conditions above with it)
    if ((d->flags & VQA_FLAG_BF16_FEATURES) && !(d->flags & VQA_FLAG_BF16_GEMM)) return false;
    // the bf16 sequence encoder is the pre-training steps' (this step's recurrence is the weight-stationary launch)
    if (d->flags & VQA_PT_FLAG_BF16_ENCODER) return false;
    // this step's switch for the encoder's single products: only inside the bf16 mode, like the bf16 table
    if (enc16(*d) && !(d->flags & VQA_FLAG_BF16_GEMM)) return false;
    if (d->model_type == VQA_MODEL_LEGACY_VQA)      // 16-byte rows everywhere; the scoring kernel keeps one H-row in LDS
        return d->map_dim > 0 && d->La > 0 && d->H % 4 == 0 && d->D % 4 == 0 && d->map_dim % 4 == 0 && d->W % 4 == 0 && d->H <= 1024 && d->Vq > 3;
    if (d->model_type == VQA_MODEL_BI) return d->H % 8 == 0;      // two cells of H / 2 units, 16-byte rows each
    if (d->model_type == VQA_MODEL_ENT)       // the pairings' tensors are addressed with 32-bit element counts
        return d->num_marginal > 0 && d->ent_cols > 0 && d->ent_cols <= d->A && d->ent_cols <= 4096 &&
               (int64_t)d->B * d->num_marginal * (2 * (int64_t)d->H > d->ent_cols ? 2 * (int64_t)d->H : d->ent_cols) < (1ll << 30);
    return true;
}
// K of pooled_linear_l = width of what the attention pools: v_adapt [R,H] for vlmap_answer_adapt, V_ft [R,D] otherwise
inline int64_t pooled_dim(const vqa_dims_t& d) { return d.model_type == VQA_MODEL_ADAPT ? d.H : d.D; }

// One dropout site of the step (VQA_KEEP_SITE_*): the explicit mask of the batch (or NULL: no dropout), or, where the
// site's bit of vqa_batch_t.keep_seeded is set, the stream position its bits are drawn from inside the consuming kernels.
// Every mask site of the forward and the backward resolves through keep_site() and hands src() to the op's launch function
// (keep_launch.h), which picks the kernel; the batch struct carries everything, nothing is remembered here.
struct KeepSite {
    const uint8_t* mask;
    bool seeded;
    uint64_t seed, off;
    // the keep source of an op on this site whose rows are row_len long
    KeepSrc src(float keep_prob, int64_t row_len) const {
        return seeded ? KeepSrc::seeded(seed, off, row_len, keep_prob) : KeepSrc::bytes(mask, keep_prob);
    }
};
const KeepSite NO_KEEP = {nullptr, false, 0, 0};      // a layer without dropout

KeepSite keep_site(const vqa_batch_t* bt, int site) {
    const bool sd = (bt->keep_seeded & site) != 0;
    switch (site) {
        case VQA_KEEP_SITE_ATT: return {bt->keep_att, sd, bt->keep_seed, bt->keep_att_off};
        case VQA_KEEP_SITE_JOINT: return {bt->keep_joint, sd, bt->keep_seed, bt->keep_joint_off};
        case VQA_KEEP_SITE_JOINT2: return {bt->keep_joint2, sd, bt->keep_seed, bt->keep_joint2_off};
        case VQA_KEEP_SITE_TILE: return {bt->keep_tile, sd, bt->keep_seed, bt->keep_tile_off};
        default: return {bt->keep_word, sd, bt->keep_seed, bt->keep_word_off};
    }
}
// a seeded site has no mask buffer, and no bit beyond the five sites is set
bool keep_sites_ok(const vqa_batch_t* bt) {
    if (bt->keep_seeded & ~31) return false;
    for (int site = 1; site <= VQA_KEEP_SITE_WORD; site <<= 1) {
        const KeepSite k = keep_site(bt, site);
        if (k.seeded && k.mask != nullptr) return false;
    }
    return true;
}

// FC + LN + ReLU forward (modules.fc_layer, vlmap/modules.py:630-650)
int fc_ln_relu_fwd(const Ctx& c, const float* x, int64_t M, int64_t K, int64_t N, const vqa_fc_t& p, int rows,
                   const char* pre, const char* y, const char* mean, const char* rstd, const KeepSite& keep,
                   float keep_prob) {
    {
        ProbeScope ps(rows > 1 ? "v_linear_v.fwd_gemm" : "fc.fwd_gemm", c.st);
        TRY(gemm_x(c, 0, M, N, K, x, (int)K, p.w, (int)N, c.f(pre), (int)N, p.b));
    }
    ProbeScope ps(rows > 1 ? "v_linear_v.ln_fwd" : "fc.ln_fwd", c.st);
    return vqa_ln_act_fwd_run(c.f(pre), p.gamma, p.beta, keep.src(keep_prob, N), c.f(y), c.f(mean), c.f(rstd), (int)(M / rows), rows,
                              (int)N, 0, c.st);
}

// the FC half of the backward once d_pre is known: parameter gradients from the per-group partials (g.w == NULL => frozen
// layer) and the optional dx = d_pre * W^T (+ dx)
int fc_bwd_tail(const Ctx& c, const float* x, int64_t M, int64_t K, int64_t N, const vqa_fc_t& p, const vqa_fc_t* g, int rows,
                const float* d_pre, const float* pa, const float* pb, const float* pc, float* dx, bool dx_accumulate) {
    const bool train = g != nullptr && g->w != nullptr;
    const int64_t G = M / rows;
    if (train) {
        {
            ProbeScope ps(rows > 1 ? "v_linear_v.ln_bwd" : "fc.ln_bwd", c.st);
            TRY(vqa_colsum3(pa, pb, pc, (int)G, (int)N, (int)N, g->gamma, g->beta, g->b, c.colsum_ws(), c.colsum_ws_floats(), c.st));
        }
        ProbeScope ps(rows > 1 ? "v_linear_v.dw_gemm" : "fc.dw_gemm", c.st);
        TRY(gemm_x(c, 1, K, N, M, x, (int)K, d_pre, (int)N, g->w, (int)N));  // dW = x^T * d_pre
    }
    if (dx != nullptr) {
        ProbeScope ps("fc.dx_gemm", c.st);
        TRY(gemm(c, 0, 1, M, K, N, d_pre, (int)N, p.w, (int)N, dx, (int)K, nullptr, dx_accumulate ? dx : nullptr, (int)K));
    }
    return VQA_OK;
}

// backward of the same block.  dy -> d_pre (named buffer); optional parameter
// grads (g.w == NULL => frozen layer); optional dx = d_pre * W^T (+ dx_add).
int fc_ln_relu_bwd(const Ctx& c, const float* dy, const float* x, int64_t M, int64_t K, int64_t N, const vqa_fc_t& p,
                   const vqa_fc_t* g, int rows, const char* pre, const char* mean, const char* rstd,
                   const KeepSite& keep, float keep_prob, const char* d_pre, float* dx, bool dx_accumulate) {
    const bool train = g != nullptr && g->w != nullptr;
    const int64_t G = M / rows;
    {
        ProbeScope ps(rows > 1 ? "v_linear_v.ln_bwd" : "fc.ln_bwd", c.st);
        TRY(vqa_ln_act_bwd_run(dy, c.f(pre), c.f(mean), c.f(rstd), p.gamma, p.beta, keep.src(keep_prob, N), c.f(d_pre),
                               train ? c.part(0) : nullptr, train ? c.part(1) : nullptr,
                               train ? c.part(2) : nullptr, (int)G, rows, (int)N, 0, c.st));
    }
    return fc_bwd_tail(c, x, M, K, N, p, g, rows, c.f(d_pre), c.part(0), c.part(1), c.part(2), dx, dx_accumulate);
}

// whether the paired launch runs: not for vlmap_answer_noc, and only on 16-byte rows
bool ln_pair_ok(const vqa_dims_t& d, const vqa_params_t* P) {
    if (!ln_pair_enabled() || d.model_type == VQA_MODEL_NOC) return false;       // vlmap_answer_noc has no product
    const void* ptrs[4] = {P->pooled_linear_l.gamma, P->pooled_linear_l.beta, P->q_linear_l.gamma, P->q_linear_l.beta};
    return vqa_ln_pair_mul_supported(d.H, ptrs, 4) != 0;
}

#include "legacy_vqa.inc"

// ---- model_type 12: bi-directional question encoder + question self-attention (vqa/model_vlmap_finetune.py:119-150) ----
// bi[0] / bi[1]: the forward / backward cell's encoder (Step::enc)
int bi_question_fwd(const Ctx& c, const vqa_params_t* P, const vqa_batch_t* bt, const GruTape* bi) {
    const vqa_dims_t& d = c.d;
    const int64_t B = d.B, H = d.H, T = d.T, W = d.W, h = H / 2;
    VQA_REQUIRE(P->embed2 && P->gru_bw_wg && P->gru_bw_bg && P->gru_bw_wc && P->gru_bw_bc && P->q_att_key.w &&
                    P->q_att_key.gamma && P->q_att_query.w && P->q_att_query.gamma && P->word_score.w && P->word_score.b &&
                    P->v_word_fc.w && P->v_word_fc.gamma,
                VQA_ERR_ARG);
    int32_t* q_rev = c.i32("q_rev");
    {
        ProbeScope ps("embed.fwd", c.st);
        TRY(vqa_reverse_tokens(bt->q_intseq, bt->q_intseq_len, q_rev, (int)B, (int)T, c.st));
        TRY(vqa_embed_fwd_ld(P->embed, bt->q_intseq, bi[0].x_tm, (int)B, (int)T, (int)W, d.Vq, bi[0].ldx(), c.st));
        TRY(vqa_embed_fwd_ld(P->embed, q_rev, bi[1].x_tm, (int)B, (int)T, (int)W, d.Vq, bi[1].ldx(), c.st));
        // the second embedding, batch-major rows (b, t): one "sequence" per token
        TRY(vqa_embed_fwd_ld(P->embed2, bt->q_intseq, c.f("e2"), (int)(B * T), 1, (int)W, d.Vq, (int)W, c.st));
    }
    for (int k = 0; k < 2; ++k) {
        const GruTape& t = bi[k];
        {
            ProbeScope ps("gru.xp_gemm", c.st);
            TRY(t.pack_wx());
            TRY(t.project(f32(c)));
        }
        TRY(t.clear_h0());
        ProbeScope ps("gru.fwd", c.st);
        TRY(vqa_gru_seq_fwd_rows(t.xp, t.Wg_h(), t.Wc_h(), bt->q_intseq_len, t.hs, t.gru_r, t.gru_u, t.gru_c, t.gru_rh, (int)T,
                                 (int)B, (int)h, 0, (int)B, c.st));
    }
    TRY(vqa_bi_outputs_fwd(bi[0].hs, bi[1].hs, bt->q_intseq_len, c.f("q_L_map"), c.f("q_L_ft"), (int)B, (int)T, (int)h, c.st));
    // keys: fc_layer on [B,T,H] -- LayerNorm over the whole [T,H] block of a question, padded positions included
    TRY(fc_ln_relu_fwd(c, c.f("q_L_map"), B * T, H, H, P->q_att_key, (int)T, "pre_key", "q_att_key", "mean_key", "rstd_key",
                       NO_KEEP, 1.f));
    TRY(fc_ln_relu_fwd(c, c.f("q_L_ft"), B, H, H, P->q_att_query, 1, "pre_query", "q_att_query", "mean_query", "rstd_query",
                       NO_KEEP, 1.f));
    TRY(fc_ln_relu_fwd(c, c.f("e2"), B * T, W, H, P->v_word_fc, (int)T, "pre_vw", "q_v_ft", "mean_vw", "rstd_vw", NO_KEEP, 1.f));
    ProbeScope ps("attn_pool.fwd", c.st);
    return vqa_attn_fwd_run(c.f("q_att_key"), c.f("q_att_query"), c.f("q_v_ft"), false, bt->q_intseq_len, P->word_score.w,
                            P->word_score.b, keep_site(bt, VQA_KEEP_SITE_WORD).src(d.keep_att, H), c.f("w_att_score"),
                            c.f("pooled_q_v"), (int)B, 1, (int)T, (int)H, (int)H, c.st);
}

// everything between d(pooled_q_v) / d(q_L_ft) and the two recurrences' inputs: word attention, v_word_fc (+ the second
// embedding's slices), q_att_query, q_att_key.  dh = gradient wrt q_L_ft so far (q_linear_l's share), accumulated into.
int bi_question_bwd_head(const Ctx& c, const vqa_params_t* P, const vqa_params_t* G, const vqa_batch_t* bt, float* dh) {
    const vqa_dims_t& d = c.d;
    const int64_t B = d.B, H = d.H, T = d.T, W = d.W;
    {
        ProbeScope ps("attn_pool.bwd", c.st);
        TRY(vqa_attn_bwd_run(c.f("d_pooled_qv"), c.f("q_att_key"), c.f("q_att_query"), c.f("q_v_ft"), false, c.f("w_att_score"),
                             P->word_score.w, keep_site(bt, VQA_KEEP_SITE_WORD).src(d.keep_att, H), c.f("d_key"), c.f("d_query"),
                             c.f("part_wdw"), c.f("part_wdb"), (int)B, 1, (int)T, (int)H, (int)H, c.st));
        if (G->word_score.w != nullptr) {
            TRY(colsum(c, c.f("part_wdw"), B, H, (int)H, G->word_score.w));
            TRY(colsum(c, c.f("part_wdb"), B, 1, 1, G->word_score.b));
        }
        // the pooled memory is a trainable layer's output here: d q_v_ft = w_att (x) d pooled_q_v
        TRY(vqa_outer_rows(c.f("w_att_score"), c.f("d_pooled_qv"), c.f("d_qvft"), (int)B, (int)T, (int)H, c.st));
    }
    const bool e2_train = G->embed2 != nullptr;
    if (G->v_word_fc.w != nullptr || e2_train)
        TRY(fc_ln_relu_bwd(c, c.f("d_qvft"), c.f("e2"), B * T, W, H, P->v_word_fc, &G->v_word_fc, (int)T, "pre_vw", "mean_vw",
                           "rstd_vw", NO_KEEP, 1.f, "d_pre_vw", e2_train ? c.f("d_e2") : nullptr, false));
    if (e2_train) {      // V_WordMap: scatter-add of the batch-major slices (every position, padding included) + their norm
        ProbeScope ps("embed.bwd", c.st);
        TRY(vqa_embed_bwd_len_det(c.f("d_e2"), bt->q_intseq, nullptr, G->embed2, (int)(B * T), 1, (int)W, d.Vq,
                                  (d.flags & VQA_FLAG_DETERMINISTIC) ? 1 : 0, c.st));
        TRY(vqa_sumsq(c.f("d_e2"), B * T * W, nullptr, c.f("sq_e2"), c.f("sumsq_ws2"), c.count("sumsq_ws2"), c.st));
    }
    TRY(fc_ln_relu_bwd(c, c.f("d_query"), c.f("q_L_ft"), B, H, H, P->q_att_query, &G->q_att_query, 1, "pre_query", "mean_query",
                       "rstd_query", NO_KEEP, 1.f, "d_pre_query", dh, true));
    return fc_ln_relu_bwd(c, c.f("d_key"), c.f("q_L_map"), B * T, H, H, P->q_att_key, &G->q_att_key, (int)T, "pre_key", "mean_key",
                          "rstd_key", NO_KEEP, 1.f, "d_pre_key", c.f("d_qmap"), false);
}

// phase 2: both BPTTs, the gradient wrt the looked-up embeddings, LearnGloVe's scatter-add and the slice norm
int bi_question_bwd_bptt(const Ctx& c, const vqa_params_t* G, const vqa_batch_t* bt, const GruTape* bi, const float* dh,
                         float* embed_slice_sq) {
    const vqa_dims_t& d = c.d;
    const int64_t B = d.B, H = d.H, T = d.T, W = d.W, h = H / 2;
    const std::string dir[2] = {"_fw", "_bw"};      // the bi-directional model's own per-cell buffers
    TRY(vqa_bi_outputs_bwd(c.f("d_qmap"), dh, bt->q_intseq_len, c.f("dout_fw"), c.f("dout_bw"), c.f("dhT_fw"), c.f("dhT_bw"),
                           (int)B, (int)T, (int)h, c.st));
    {
        ProbeScope ps("gru.bwd", c.st);
        for (int k = 0; k < 2; ++k) {
            const GruTape& t = bi[k];
            TRY(vqa_gru_seq_bwd_outs(c.f("dhT" + dir[k]), t.Wg_h(), t.Wc_h(), bt->q_intseq_len, t.hs, t.gru_r,
                                     t.gru_u, t.gru_c, c.f("dout" + dir[k]), t.dxp, c.f("dhS" + dir[k]), (int)T, (int)B, (int)h, c.st));
        }
    }
    {
        ProbeScope ps("gru.dx_gemm", c.st);
        for (int k = 0; k < 2; ++k) {
            TRY(bi[k].pack_wx());
            TRY(bi[k].dx(f32(c), c.f("dx" + dir[k])));
        }
        TRY(vqa_bi_dx_combine(c.f("dx_fw"), c.f("dx_bw"), bt->q_intseq_len, c.f("dx_embed"), (int)B, (int)T, (int)W, c.st));
    }
    ProbeScope ps("embed.bwd", c.st);
    if (G->embed != nullptr)
        TRY(vqa_embed_bwd_len_det(c.f("dx_embed"), bt->q_intseq, bt->q_intseq_len, G->embed, (int)B, (int)T, (int)W, d.Vq,
                                  (d.flags & VQA_FLAG_DETERMINISTIC) ? 1 : 0, c.st));
    if (embed_slice_sq != nullptr)
        TRY(vqa_sumsq(c.f("dx_embed"), T * B * W, G->embed2 != nullptr ? c.f("sq_e2") : nullptr, embed_slice_sq, c.f("sumsq_ws"),
                      c.count("sumsq_ws"), c.st));
    return VQA_OK;
}

}  // namespace

extern "C" int64_t vqa_fusion_workspace_bytes(const vqa_dims_t* dims) {
    if (!dims_ok(dims)) return VQA_ERR_ARG;
    return make_layout(*dims).total;
}

extern "C" int vqa_fusion_tensor(const vqa_dims_t* dims, const char* name, int64_t* offset_bytes, int64_t* n_elems) {
    if (!dims_ok(dims) || name == nullptr) return VQA_ERR_ARG;
    const Layout L = make_layout(*dims);
    const char* key = name;
    if (strcmp(name, "condition") == 0 && dims->model_type == VQA_MODEL_ANSWER2) key = "q_L_ft2";   // model_vlmap_answer2.py:131
    else if (strcmp(name, "condition") == 0 && dims->model_type == VQA_MODEL_BI) key = "q_L_ft";  // concat of the two final states
    else if (dims->model_type == VQA_MODEL_LEGACY_VQA && (strcmp(name, "q_L_ft") == 0 || strcmp(name, "answer_ft") == 0)) {
        // final LSTM states: the last [N,H] block of the time-major state tapes
        const bool q = name[0] == 'q';
        const auto* hsn = L.find(q ? "lv_hsq" : "lv_hsa");
        const int64_t N = q ? dims->B : dims->A, Tn = q ? dims->T : dims->La;
        if (offset_bytes) *offset_bytes = hsn->off + Tn * N * dims->H * 4;
        if (n_elems) *n_elems = N * dims->H;
        return VQA_OK;
    }
    else if (strcmp(name, "condition") == 0) {  // heavy_output['condition'] = final GRU state = hs[T]
        const auto* h = L.find("hs");
        if (offset_bytes) *offset_bytes = h->off + (int64_t)dims->T * dims->B * dims->H * 4;
        if (n_elems) *n_elems = (int64_t)dims->B * dims->H;
        return VQA_OK;
    }
    const auto* e = L.find(key);
    if (e == nullptr) return VQA_ERR_ARG;
    if (offset_bytes) *offset_bytes = e->off;
    if (n_elems) *n_elems = e->n;
    return VQA_OK;
}

extern "C" int vqa_vtail_set_mode(int mode) {
    g_vtail_mode = mode < 0 ? -1 : (mode ? 1 : 0);
    return vtail_mode();
}

extern "C" int vqa_gru_h0skip_set_mode(int mode) {
    g_h0skip_mode = mode < 0 ? -1 : (mode & 3);
    return h0skip_mode();
}

namespace {

// Everything one forward or backward call derives from its arguments, computed once and handed to every stage.  The
// second half holds what a stage decides for the stages behind it.  Of the VQA_HOT_* switches it holds the ones a later
// stage depends on (pair, visual_late, fuse_gather, forked); xcat, repack, gru_ws, vtail_mode and the gather mode stay
// calls of their once-per-process readers at the place of use, so that none is read from the environment before the
// first step that needs it (vqa_vtail_set_mode(-1) must still take effect between a forward and its backward).
struct Step {
    const vqa_dims_t& d;
    const vqa_params_t* const P;
    const vqa_params_t* const G;       // where the gradients go (backward); NULL in a forward call
    const vqa_batch_t* const bt;
    const Layout L;
    const Ctx c;                       // the caller's stream
    const int mt;
    const int64_t B, R, D, H, T, W, A;
    const int64_t Dp;                  // width of what the attention pools
    GruTape enc[2];                    // [0] the question encoder; model_type 12: the forward and [1] the backward cell, H / 2 units each
    // side stream (VQA_HOT_OVERLAP=1): set where the visual branch (forward) or v_linear_v's backward forks
    Side* sd = nullptr;
    bool forked = false;
    // forward: the visual branch's plan, and what the question branch hands on
    bool fuse_gather = false, visual_late = false;
    const float* q_ft = nullptr;       // the question code q_L_ft [B,H]
    const float* qv_in = nullptr;      // what q_linear_v reads
    const float* lin_in = nullptr;     // what q_linear_l reads: the question code, or one of the ablations' layers on top of it
    // both directions: pooled_linear_l and q_linear_l finish in the paired LayerNorm launch (ln_pair_ok)
    bool pair = false;

    Step(const vqa_dims_t* dims, const vqa_params_t* P_, const vqa_params_t* G_, const vqa_batch_t* bt_, void* workspace,
         void* stream)
        : d(*dims), P(P_), G(G_), bt(bt_), L(make_layout(*dims)),
          c{{L, static_cast<char*>(workspace)}, *dims, static_cast<hipStream_t>(stream), 0}, mt(dims->model_type),
          B(dims->B), R(dims->R), D(dims->D), H(dims->H), T(dims->T), W(dims->W), A(dims->A),
          Dp(pooled_dim(*dims)) {
        if (mt == VQA_MODEL_LEGACY_VQA) return;      // LSTM encoders (legacy_vqa.inc)
        const int64_t Hc = mt == VQA_MODEL_BI ? H / 2 : H;
        enc[0] = GruTape(c, "", "", "", T, B, Hc, W, fw_cell(P), c.st);
        if (mt == VQA_MODEL_BI) enc[1] = GruTape(c, "", "", "_bw", T, B, Hc, W, bw_cell(P), c.st);
    }
    Step(const Step&) = delete;
    Step& operator=(const Step&) = delete;

    // the context of what may run beside the caller's stream (the visual branch; v_linear_v's backward): the side stream
    // and its own scratch when forked, else the caller's
    Ctx side_ctx() const { return Ctx{{L, c.ws}, d, forked ? sd->s : c.st, forked ? 1 : 0}; }
    float* const dh = c.f("d_h0");     // backward: gradient wrt the question code
};

// the two halves of the side stream's join: its work is recorded, the caller's stream waits for the record
int side_record(const Step& s) { return !s.forked || join_side_record(*s.sd) ? VQA_OK : VQA_ERR_LAUNCH; }
int side_wait(const Step& s) {
    return !s.forked || hipStreamWaitEvent(s.c.st, s.sd->join, 0) == hipSuccess ? VQA_OK : VQA_ERR_LAUNCH;
}

// Which form of the recurrence runs: one decision for the forward and the backward of a step.
//   GRU_WS      one launch, recurrent weights resident in registers and LDS, eight XCD-local chains (csrc/gru_ws.hip)
//   GRU_LIVE    rows sorted by length: per-step kernels that skip finished sequences
//   GRU_CHAINS  per-step kernels on independent row chains in anti-phase (gru_chains)
// (A length-sorted batch whose longest row runs to T: the weight-stationary launch computes every row of every step under
// its length mask -- same results -- and is faster than the shrinking per-step kernels at these sizes.)
enum GruForm { GRU_WS, GRU_LIVE, GRU_CHAINS };
enum GruDir { GRU_FWD, GRU_BWD };
GruForm gru_form(GruDir dir, int64_t T, int64_t B, int64_t H, const int32_t* live_rows) {
    const bool ws_ok = gru_ws_on() && (live_rows == nullptr || (T > 0 && live_rows[T - 1] > 0));
    if (ws_ok && (dir == GRU_FWD ? vqa_gru_ws_supported((int)T, (int)B, (int)H) : vqa_gru_ws_bwd_supported((int)T, (int)B, (int)H)) == 1)
        return GRU_WS;
    return live_rows != nullptr ? GRU_LIVE : GRU_CHAINS;
}

// ---------------------------------------------------------------- forward stages, in launch order

// Where the visual branch runs.  With the side stream it is launched first and overlaps the recurrence; on one stream it
// runs AFTER the question branch, right before the attention that consumes it: V_ft (151 MB) and v_linear_v (75 MB) are
// then still in the 256 MB Infinity Cache when the attention kernel reads them, instead of having been pushed out by the
// recurrence's traffic.
void fwd_visual_plan(Step& s) {
    s.sd = &side_stream();
    s.forked = fork_side(s.c, *s.sd);
    // (dims_ok refuses the FLAG pair; VQA_HOT_GATHER=fused in the environment must not bring the f32 gather GEMM into a bf16 step either)
    const int gm = gather_mode(&s.d);
    const bool same_kernel = gm == 2 && side_max_blocks() == 0 &&
                             vqa_gemm_gather_matches_plain((int)(s.B * s.R), (int)s.H, (int)s.D, (int)s.D, (int)s.R, s.d.N_img);
    s.fuse_gather = !(s.d.flags & VQA_FLAG_BF16_GEMM) && (gm == 1 || same_kernel) && (s.D % 32 == 0) && (s.H % 4 == 0) &&
                    vqa_aligned16(s.bt->table);
    s.visual_late = !s.forked && visual_late_enabled();
}

// a1 + a2: feature gather, v_linear_v and (vlmap_answer_adapt) v_adapt
int fwd_visual(const Step& s) {
    const Ctx cv = s.side_ctx();
    const vqa_params_t* P = s.P;
    const vqa_batch_t* bt = s.bt;
    const int64_t B = s.B, R = s.R, D = s.D, H = s.H;
    // a1: V_ft = features[image_idx] (a pass of its own, or inside the GEMM below), num_V_ft = num_boxes[image_idx]
    {
        ProbeScope ps("gather", cv.st);
        if (feat16(s.d))      // (never fused: dims_ok)
            TRY(vqa_gather_features_bf16(reinterpret_cast<const uint16_t*>(bt->table), bt->nbox_table, bt->image_idx,
                                         cv.u16("V_ft"), cv.i32("num_V_ft"), (int)B, (int)R, (int)D, s.d.N_img, cv.st));
        else
            TRY(vqa_gather_features(bt->table, bt->nbox_table, bt->image_idx, s.fuse_gather ? nullptr : cv.f("V_ft"),
                                    cv.i32("num_V_ft"), (int)B, (int)R, (int)D, s.d.N_img, cv.st));
    }
    // a2: v_linear_v, LN statistics over the whole [R,H] block of a sample
    if (s.fuse_gather) {
        {
            ProbeScope ps("v_linear_v.fwd_gemm", cv.st);
            TRY(vqa_gemm_f32_gather((int)(B * R), (int)H, (int)D, bt->table, (int)D, bt->image_idx, (int)R, s.d.N_img,
                                    P->v_linear_v.w, (int)H, cv.f("pre_v"), (int)H, P->v_linear_v.b, cv.f("V_ft"), (int)D,
                                    cv.st));
        }
        ProbeScope ps("v_linear_v.ln_fwd", cv.st);
        TRY(vqa_ln_relu_fwd(cv.f("pre_v"), P->v_linear_v.gamma, P->v_linear_v.beta, nullptr, 1.f, cv.f("v_linear_v"),
                            cv.f("mean_v"), cv.f("rstd_v"), (int)B, (int)R, (int)H, cv.st));
    } else {
        TRY(fc_ln_relu_fwd(cv, cv.f("V_ft"), B * R, D, H, P->v_linear_v, (int)R, "pre_v", "v_linear_v", "mean_v", "rstd_v",
                           NO_KEEP, 1.f));
    }
    if (s.mt == VQA_MODEL_ADAPT) {     // v_adapt: a second FC + LN[R,H] + ReLU on the same V_ft (:132-135)
        VQA_REQUIRE(P->v_adapt.w != nullptr && P->v_adapt.gamma != nullptr, VQA_ERR_ARG);
        TRY(fc_ln_relu_fwd(cv, cv.f("V_ft"), B * R, D, H, P->v_adapt, (int)R, "pre_va", "v_adapt", "mean_va", "rstd_va",
                           NO_KEEP, 1.f));
    }
    return VQA_OK;
}

// a3 + a4: embedding lookup, x-projection of all steps, recurrence.  Leaves the question code in s.q_ft / s.qv_in.
int fwd_question(Step& s) {
    const Ctx& c = s.c;
    const vqa_params_t* P = s.P;
    const vqa_batch_t* bt = s.bt;
    const int64_t B = s.B, H = s.H, T = s.T, W = s.W;
    if (s.mt == VQA_MODEL_BI) {
        TRY(bi_question_fwd(c, P, bt, s.enc));
        s.q_ft = c.f("q_L_ft");
        s.qv_in = c.f("pooled_q_v");
        return VQA_OK;
    }
    const GruTape& e = s.enc[0];
    // a3: embedding lookup, time-major
    // x_tm rows carry the constant 1 after the W inputs (vqa_embed_fwd_ld): the x-part weight-gradient GEMM then also
    // delivers the bias gradients, and the two passes over dxp that summed its columns are gone
    {
        ProbeScope ps("embed.fwd", c.st);
        TRY(vqa_embed_fwd_ld(P->embed, bt->q_intseq, e.x_tm, (int)B, (int)T, (int)W, s.d.Vq, e.ldx(), c.st));
    }
    // a4: GRU.  Input projections of all steps as one packed GEMM (or the two-GEMM form) ...
    {
        ProbeScope ps("gru.xp_gemm", c.st);
        if (xcat_enabled()) {
            TRY(e.pack_wx());
            TRY(e.project(enc(c)));
        } else {
            TRY(gemm_enc(c, 0, 0, T * B, 2 * H, W, e.x_tm, e.ldx(), P->gru_wg, (int)(2 * H), e.xp, (int)(3 * H), P->gru_bg));
            TRY(gemm_enc(c, 0, 0, T * B, H, W, e.x_tm, e.ldx(), P->gru_wc, (int)H, e.xp + 2 * H, (int)(3 * H), P->gru_bc));
        }
    }
    // ... then the recurrence
    TRY(e.clear_h0());
    const float *Wg_h = e.Wg_h(), *Wc_h = e.Wc_h();
    {
        ProbeScope ps("gru.fwd", c.st);
        switch (gru_form(GRU_FWD, T, B, H, bt->live_rows)) {
            case GRU_WS:
                TRY(vqa_gru_seq_fwd_ws_ex(e.xp, Wg_h, Wc_h, bt->q_intseq_len, e.hs, e.gru_r, e.gru_u, e.gru_c, e.gru_rh, (int)T, (int)B,
                                          (int)H, h0skip_mode() & 1, c.find_f("gru_ws"), c.st));      // hs[0]: cleared above
                break;
            case GRU_LIVE:
                TRY(vqa_gru_seq_fwd_live(e.xp, Wg_h, Wc_h, bt->q_intseq_len, bt->live_rows, e.hs, e.gru_r, e.gru_u, e.gru_c, e.gru_rh,
                                         (int)T, (int)B, (int)H, c.st));
                break;
            case GRU_CHAINS:
                TRY(run_chains(c, B, [&](int, int64_t row0, int64_t rows, hipStream_t st) {
                    return vqa_gru_seq_fwd_rows(e.xp, Wg_h, Wc_h, bt->q_intseq_len, e.hs, e.gru_r, e.gru_u, e.gru_c, e.gru_rh, (int)T,
                                                (int)B, (int)H, (int)row0, (int)rows, st);
                }));
                break;
        }
    }
    s.q_ft = e.h_final();
    s.qv_in = s.q_ft;
    return VQA_OK;
}

// the ablations' layer between the question code and q_linear_l; leaves what q_linear_l reads in s.lin_in
int fwd_question_code(Step& s) {
    const Ctx& c = s.c;
    const vqa_params_t* P = s.P;
    const int64_t B = s.B, H = s.H;
    const float* h = s.q_ft;
    s.lin_in = h;
    if (s.mt == VQA_MODEL_ANSWER2) {           // q_L_ft2 = tanh(LN(fc(q_L_ft)))   (vqa/model_vlmap_answer2.py:127-130)
        VQA_REQUIRE(P->q_L_ft2.w != nullptr && P->q_L_ft2.gamma != nullptr, VQA_ERR_ARG);
        ProbeScope ps("fc.fwd_gemm", c.st);
        TRY(gemm(c, 0, 0, B, H, H, h, (int)H, P->q_L_ft2.w, (int)H, c.f("pre_ft2"), (int)H, P->q_L_ft2.b));
        TRY(vqa_ln_act_fwd(c.f("pre_ft2"), P->q_L_ft2.gamma, P->q_L_ft2.beta, nullptr, 1.f, c.f("q_L_ft2"), c.f("mean_ft2"),
                           c.f("rstd_ft2"), (int)B, 1, (int)H, 1, c.st));
        s.lin_in = c.f("q_L_ft2");
    } else if (s.mt == VQA_MODEL_NO_NOISE || s.mt == VQA_MODEL_FULL) {     // q_L_mean: a plain linear layer (:122-125)
        VQA_REQUIRE(P->q_L_mean.w != nullptr, VQA_ERR_ARG);
        ProbeScope ps("fc.fwd_gemm", c.st);
        TRY(gemm(c, 0, 0, B, H, H, h, (int)H, P->q_L_mean.w, (int)H, c.f("q_L_mean"), (int)H, P->q_L_mean.b));
        s.lin_in = c.f("q_L_mean");
        if (s.mt == VQA_MODEL_FULL) {          // reparameterisation (vqa/model_vlmap_answer_full.py:128-134)
            VQA_REQUIRE(P->q_L_log_sigma_sq.w != nullptr && s.bt->noise != nullptr, VQA_ERR_ARG);
            TRY(gemm(c, 0, 0, B, H, H, h, (int)H, P->q_L_log_sigma_sq.w, (int)H, c.f("q_L_log_sigma_sq"), (int)H,
                     P->q_L_log_sigma_sq.b));
            TRY(vqa_reparam_fwd(c.f("q_L_mean"), c.f("q_L_log_sigma_sq"), s.bt->noise, c.f("q_L_mean_noise"), c.f("extra_row"),
                                (int)B, (int)H, c.st));
            s.lin_in = c.f("q_L_mean_noise");
        }
    }
    return VQA_OK;
}

// a5
int fwd_q_linear_v(const Step& s) {
    return fc_ln_relu_fwd(s.c, s.qv_in, s.B, s.H, s.H, s.P->q_linear_v, 1, "pre_qv", "q_linear_v", "mean_qv", "rstd_qv", NO_KEEP, 1.f);
}

// a6 + a7: Hadamard attention and pooling (vlmap_answer_adapt pools v_adapt [R,H] instead of V_ft [R,D])
int fwd_attention(const Step& s) {
    const Ctx& c = s.c;
    ProbeScope ps("attn_pool.fwd", c.st);
    const bool v16 = feat16(s.d);
    const void* V = v16 ? (const void*)c.u16("V_ft") : (const void*)c.f(s.mt == VQA_MODEL_ADAPT ? "v_adapt" : "V_ft");
    return vqa_attn_fwd_run(c.f("v_linear_v"), c.f("q_linear_v"), V, v16, c.i32("num_V_ft"), s.P->score.w, s.P->score.b,
                            keep_site(s.bt, VQA_KEEP_SITE_ATT).src(s.d.keep_att, s.H), c.f("att_score"), c.f("pooled_V_ft"),
                            (int)s.B, 1, (int)s.R, (int)s.H, (int)s.Dp, c.st);
}

// a8: pooled_linear_l and q_linear_l; the paired form also leaves their product in joint_in
int fwd_linear_l(Step& s) {
    const Ctx& c = s.c;
    const vqa_params_t* P = s.P;
    const int64_t B = s.B, H = s.H, Dp = s.Dp;
    s.pair = ln_pair_ok(s.d, P);
    if (!s.pair) {
        TRY(fc_ln_relu_fwd(c, c.f("pooled_V_ft"), B, Dp, H, P->pooled_linear_l, 1, "pre_pl", "pooled_linear_l", "mean_pl",
                           "rstd_pl", NO_KEEP, 1.f));
        return fc_ln_relu_fwd(c, s.lin_in, B, H, H, P->q_linear_l, 1, "pre_ll", "l_linear_l", "mean_ll", "rstd_ll", NO_KEEP, 1.f);
    }
    {
        ProbeScope ps("fc.fwd_gemm", c.st);
        TRY(gemm(c, 0, 0, B, H, Dp, c.f("pooled_V_ft"), (int)Dp, P->pooled_linear_l.w, (int)H, c.f("pre_pl"), (int)H,
                 P->pooled_linear_l.b));
        TRY(gemm(c, 0, 0, B, H, H, s.lin_in, (int)H, P->q_linear_l.w, (int)H, c.f("pre_ll"), (int)H, P->q_linear_l.b));
    }
    ProbeScope ps("fc.ln_fwd", c.st);
    return vqa_ln_pair_mul_fwd(c.f("pre_pl"), c.f("pre_ll"), P->pooled_linear_l.gamma, P->pooled_linear_l.beta, P->q_linear_l.gamma,
                               P->q_linear_l.beta, c.f("pooled_linear_l"), c.f("l_linear_l"), c.f("joint_in"), c.f("mean_pl"),
                               c.f("rstd_pl"), c.f("mean_ll"), c.f("rstd_ll"), (int)B, (int)H, c.st);
}

// a9: the joint layer on the product of the two branches (dropout .5); vlmap_answer_noc keeps the branches apart
int fwd_joint(const Step& s) {
    const Ctx& c = s.c;
    const vqa_params_t* P = s.P;
    const vqa_batch_t* bt = s.bt;
    const int64_t B = s.B, H = s.H;
    if (s.mt == VQA_MODEL_NOC) {
        // vlmap_answer_noc (vqa/model_vlmap_answer_noc.py:177-188): no composition -- joint_v on pooled_linear_l and joint_l
        // on l_linear_l, each FC + LN + ReLU + dropout .5 ("joint" holds v_joint)
        VQA_REQUIRE(P->joint2.w != nullptr && P->head2.w != nullptr, VQA_ERR_ARG);
        TRY(fc_ln_relu_fwd(c, c.f("pooled_linear_l"), B, H, 2 * H, P->joint_fc, 1, "pre_j", "joint", "mean_j", "rstd_j",
                           keep_site(bt, VQA_KEEP_SITE_JOINT), s.d.keep_joint));
        return fc_ln_relu_fwd(c, c.f("l_linear_l"), B, H, 2 * H, P->joint2, 1, "pre_jl", "l_joint", "mean_jl", "rstd_jl",
                              keep_site(bt, VQA_KEEP_SITE_JOINT2), s.d.keep_joint);
    }
    if (!s.pair) {
        ProbeScope ps("eltwise", c.st);
        TRY(vqa_mul(c.f("pooled_linear_l"), c.f("l_linear_l"), c.f("joint_in"), B * H, c.st));
    }
    return fc_ln_relu_fwd(c, c.f("joint_in"), B, H, 2 * H, P->joint_fc, 1, "pre_j", "joint", "mean_j", "rstd_j",
                          keep_site(bt, VQA_KEEP_SITE_JOINT), s.d.keep_joint);
}

// a10: the answer head
int fwd_head(const Step& s) {
    const Ctx& c = s.c;
    const vqa_params_t* P = s.P;
    const int64_t B = s.B, H = s.H, W = s.W, A = s.A;
    if (s.mt == VQA_MODEL_WORD2VEC) {
        // standard_word2vec (vqa/model_standard_word2vec.py:180-188): classifier FC into the 300-d word space, then
        // logits = joint2 x the constant [W, A] GloVe matrix of the answers
        VQA_REQUIRE(P->answer_glove != nullptr, VQA_ERR_ARG);
        ProbeScope ps("head.fwd_gemm", c.st);
        TRY(gemm(c, 0, 0, B, W, 2 * H, c.f("joint"), (int)(2 * H), P->head.w, (int)W, c.f("joint2"), (int)W, P->head.b));
        TRY(gemm(c, 0, 0, B, A, W, c.f("joint2"), (int)W, P->answer_glove, (int)A, c.f("logit"), (int)A));
    } else if (s.mt == VQA_MODEL_NOC) {
        // logit = WordWeightAnswerV(v_joint) + WordWeightAnswerL(l_joint)   (:190-204): the second GEMM adds onto the first
        ProbeScope ps("head.fwd_gemm", c.st);
        TRY(gemm(c, 0, 0, B, A, 2 * H, c.f("joint"), (int)(2 * H), P->head.w, (int)A, c.f("logit"), (int)A, P->head.b));
        TRY(gemm(c, 0, 0, B, A, 2 * H, c.f("l_joint"), (int)(2 * H), P->head2.w, (int)A, c.f("logit"), (int)A, P->head2.b,
                 c.f("logit"), (int)A));
    } else if (has_tuned_head(s.mt)) {
        // vlmap_answer_vqa_all2 (vqa/model_vlmap_answer_vqa_all2.py:196-227): the fixed WordWeightAnswer head and the
        // trainable TunedWordWeightAnswer head, BOTH on `joint` (the reference's tuned head reads `joint`, :216-217);
        // _vqa_all: the same with the fixed logits of unknown answers moved to the row minimum (:192-194)
        VQA_REQUIRE(P->head2.w != nullptr && P->head2.b != nullptr, VQA_ERR_ARG);
        ProbeScope ps("head.fwd_gemm", c.st);
        TRY(gemm(c, 0, 0, B, A, 2 * H, c.f("joint"), (int)(2 * H), P->head.w, (int)A,
                 c.f(s.mt == VQA_MODEL_VQA_ALL ? "logit_raw" : "logit_fixed"), (int)A, P->head.b));
        if (s.mt == VQA_MODEL_VQA_ALL)
            TRY(vqa_rowmin_mask_fwd(c.f("logit_raw"), s.bt->exist_mask, c.f("logit_fixed"), c.f("rowmin"), (int)B, (int)A, c.st));
        TRY(gemm(c, 0, 0, B, A, 2 * H, c.f("joint"), (int)(2 * H), P->head2.w, (int)A, c.f("logit_tuned"), (int)A, P->head2.b));
    } else {
        ProbeScope ps("head.fwd_gemm", c.st);
        TRY(gemm(c, 0, 0, B, A, 2 * H, c.f("joint"), (int)(2 * H), P->head.w, (int)A, c.f("logit"), (int)A, P->head.b));
    }
    return VQA_OK;
}

// a11: loss, argmax and report; the entropy regulariser's forward and the extra report ride in the same scope
int fwd_loss(const Step& s, int want_dz) {
    const Ctx& c = s.c;
    const vqa_params_t* P = s.P;
    const vqa_batch_t* bt = s.bt;
    const int64_t B = s.B, H = s.H, A = s.A;
    ProbeScope ps("loss.fwd", c.st);
    if (has_tuned_head(s.mt))
        TRY(vqa_loss2_fwd(c.f("logit_fixed"), c.f("logit_tuned"), bt->answer_target, bt->train_mask, bt->obj_mask,
                          bt->attr_mask, bt->exist_mask, s.d.inv_global_batch, c.f("stats"), c.i32("pred"),
                          want_dz ? c.f("dlogit") : nullptr, want_dz ? c.f("dlogit_tuned") : nullptr, c.f("logit"),
                          s.mt == VQA_MODEL_VQA_ALL ? 1 : 0, (int)B, (int)A, c.st));
    else
        TRY(vqa_loss_fwd(c.f("logit"), bt->answer_target, bt->train_mask, bt->obj_mask, bt->attr_mask, bt->exist_mask,
                         train_loss_masked(s.mt) ? 1 : 0, s.d.inv_global_batch, c.f("stats"), c.i32("pred"),
                         want_dz ? c.f("dlogit") : nullptr, (int)B, (int)A, c.st));
    TRY(vqa_report_reduce(c.f("stats"), (int)B, c.f("report"), c.st));
    if (s.mt == VQA_MODEL_ENT) {
        // Maximum entropy regularisation (vqa/model_vlmap_answer_ent.py:191-211, 281-292): joint_fc (+ its own dropout)
        // and the head's first ent_cols columns on num_marginal pairings of every question; tile_z ends up holding
        // d loss / d logit of the pairings (want_dz) or their probabilities
        ProbeScope ps_ent("ent.fwd", c.st);
        const int64_t M = s.d.num_marginal, C = s.d.ent_cols;
        TRY(vqa_tile_mul_fwd(c.f("pooled_linear_l"), c.f("l_linear_l"), c.f("tile_in"), (int)B, (int)M, (int)H, c.st));
        TRY(gemm(c, 0, 0, B * M, 2 * H, H, c.f("tile_in"), (int)H, P->joint_fc.w, (int)(2 * H), c.f("pre_tj"), (int)(2 * H),
                 P->joint_fc.b));
        TRY(vqa_ln_act_fwd_run(c.f("pre_tj"), P->joint_fc.gamma, P->joint_fc.beta,
                               keep_site(bt, VQA_KEEP_SITE_TILE).src(s.d.keep_joint, 2 * H), c.f("tile_joint"), c.f("mean_tj"),
                               c.f("rstd_tj"), (int)B, (int)M, (int)(2 * H), 0, c.st));
        TRY(gemm(c, 0, 0, B * M, C, 2 * H, c.f("tile_joint"), (int)(2 * H), P->head.w, (int)A, c.f("tile_z"), (int)C, P->head.b));
        TRY(vqa_marginal_entropy(c.f("tile_z"), bt->train_mask, bt->exist_mask, s.d.extra_weight * s.d.inv_global_batch,
                                 c.f("marginal_prob"), c.f("extra_row"), (int)B, (int)M, (int)C, (int)C, want_dz, c.st));
    }
    if (s.mt == VQA_MODEL_FULL || s.mt == VQA_MODEL_ENT)      // latent_loss | entropy, its weighted form and the total loss
        TRY(vqa_extra_report(c.f("extra_row"), c.f("stats"), (int)B, s.d.extra_weight, c.f("report"), c.st));
    return VQA_OK;
}

}  // namespace

extern "C" int vqa_fusion_forward(const vqa_dims_t* dims, const vqa_params_t* P, const vqa_batch_t* bt,
                                  void* workspace, int64_t workspace_bytes, int want_dz, void* stream) {
    VQA_REQUIRE(dims_ok(dims) && P && bt && workspace, VQA_ERR_ARG);
    VQA_REQUIRE(keep_sites_ok(bt), VQA_ERR_ARG);
    Step s(dims, P, nullptr, bt, workspace, stream);
    VQA_REQUIRE(workspace_bytes >= s.L.total, VQA_ERR_WORKSPACE);
    VQA_REQUIRE(vqa_aligned16(workspace), VQA_ERR_ALIGN);
    ProbeScope ps_all("forward", s.c.st);
    if (s.mt == VQA_MODEL_LEGACY_VQA) return legacy_vqa_forward(s.c, P, bt, want_dz);

    // visual branch (a1 + a2) on the side stream (VQA_HOT_OVERLAP=1 only), question branch (a3-a5) on the caller's
    fwd_visual_plan(s);
    if (!s.visual_late) TRY(fwd_visual(s));
    TRY(side_record(s));
    TRY(fwd_question(s));
    TRY(fwd_question_code(s));
    TRY(fwd_q_linear_v(s));
    TRY(side_wait(s));
    if (s.visual_late) TRY(fwd_visual(s));
    TRY(fwd_attention(s));
    TRY(fwd_linear_l(s));
    TRY(fwd_joint(s));
    TRY(fwd_head(s));
    return fwd_loss(s, want_dz);
}

// Which recurrence a step of these dims and this batch's live_rows runs: gru_form's answer (0 GRU_WS, 1 GRU_LIVE,
// 2 GRU_CHAINS), for tests that pin the routing.  Host only.  The bi-directional and the legacy model do not ask gru_form.
extern "C" int vqa_fusion_gru_form(const vqa_dims_t* dims, const int32_t* live_rows_host, int backward) {
    VQA_REQUIRE(dims_ok(dims) && (backward == 0 || backward == 1), VQA_ERR_ARG);
    VQA_REQUIRE(dims->model_type != VQA_MODEL_BI && dims->model_type != VQA_MODEL_LEGACY_VQA, VQA_ERR_UNSUPPORTED);
    return (int)gru_form(backward ? GRU_BWD : GRU_FWD, dims->T, dims->B, dims->H, live_rows_host);
}

extern "C" int vqa_fusion_backward(const vqa_dims_t* dims, const vqa_params_t* P, const vqa_params_t* G,
                                   const vqa_batch_t* bt, void* workspace, int64_t workspace_bytes,
                                   float* embed_slice_sq, void* stream) {
    return vqa_fusion_backward_phases(dims, P, G, bt, workspace, workspace_bytes, embed_slice_sq, 15, stream);
}

namespace {

// ---------------------------------------------------------------- backward stages: phase 1 in launch order, then 2, 4, 8

// the answer head: dlogit -> the head's gradients and d_joint
int bwd_head(const Step& s) {
    const Ctx& c = s.c;
    const vqa_params_t* P = s.P;
    const vqa_params_t* G = s.G;
    const int64_t B = s.B, H = s.H, W = s.W, A = s.A;
    ProbeScope ps_head("head.bwd_gemm", c.st);
    if (s.mt == VQA_MODEL_WORD2VEC) {
        // word2vec head: d_joint2 = dlogit * G^T (the GloVe matrix is a constant), then the classifier FC
        VQA_REQUIRE(P->answer_glove != nullptr, VQA_ERR_ARG);
        TRY(gemm(c, 0, 1, B, W, A, c.f("dlogit"), (int)A, P->answer_glove, (int)A, c.f("d_joint2"), (int)W));
        if (G->head.w != nullptr) {
            TRY(gemm(c, 1, 0, 2 * H, W, B, c.f("joint"), (int)(2 * H), c.f("d_joint2"), (int)W, G->head.w, (int)W));
            TRY(colsum(c, c.f("d_joint2"), B, W, (int)W, G->head.b));
        }
        return gemm(c, 0, 1, B, 2 * H, W, c.f("d_joint2"), (int)W, P->head.w, (int)W, c.f("d_joint"), (int)(2 * H));
    }
    if (s.mt == VQA_MODEL_VQA_ALL)       // back through the row-minimum substitution, in place (dlogit was taken wrt the masked logits)
        TRY(vqa_rowmin_mask_bwd(c.f("dlogit"), c.f("logit_raw"), c.f("rowmin"), s.bt->exist_mask, (int)B, (int)A, c.st));
    // head: logit = joint*W + b
    if (G->head.w != nullptr) {
        TRY(gemm(c, 1, 0, 2 * H, A, B, c.f("joint"), (int)(2 * H), c.f("dlogit"), (int)A, G->head.w, (int)A));
        TRY(colsum(c, c.f("dlogit"), B, A, (int)A, G->head.b));
    }
    TRY(gemm(c, 0, 1, B, 2 * H, A, c.f("dlogit"), (int)A, P->head.w, (int)A, c.f("d_joint"), (int)(2 * H)));
    if (has_tuned_head(s.mt)) {     // the tuned head: its own weights train, and its dz joins d_joint (unmasked term of the loss)
        VQA_REQUIRE(P->head2.w != nullptr, VQA_ERR_ARG);
        if (G->head2.w != nullptr) {
            TRY(gemm(c, 1, 0, 2 * H, A, B, c.f("joint"), (int)(2 * H), c.f("dlogit_tuned"), (int)A, G->head2.w, (int)A));
            TRY(colsum(c, c.f("dlogit_tuned"), B, A, (int)A, G->head2.b));
        }
        TRY(gemm(c, 0, 1, B, 2 * H, A, c.f("dlogit_tuned"), (int)A, P->head2.w, (int)A, c.f("d_joint"), (int)(2 * H), nullptr,
                 c.f("d_joint"), (int)(2 * H)));
    }
    return VQA_OK;
}

// the joint layer: d_joint -> d_pl / d_ll (d_joint_in under the paired LayerNorm, whose backward differentiates the product)
int bwd_joint(const Step& s) {
    const Ctx& c = s.c;
    const vqa_params_t* P = s.P;
    const vqa_params_t* G = s.G;
    const vqa_batch_t* bt = s.bt;
    const int64_t B = s.B, H = s.H, A = s.A;
    if (s.mt == VQA_MODEL_NOC) {
        // vlmap_answer_noc: the two branches separately, straight into d_pl / d_ll (no product to differentiate); the
        // l_joint branch's head first
        if (G->head2.w != nullptr) {
            TRY(gemm(c, 1, 0, 2 * H, A, B, c.f("l_joint"), (int)(2 * H), c.f("dlogit"), (int)A, G->head2.w, (int)A));
            TRY(colsum(c, c.f("dlogit"), B, A, (int)A, G->head2.b));
        }
        TRY(gemm(c, 0, 1, B, 2 * H, A, c.f("dlogit"), (int)A, P->head2.w, (int)A, c.f("d_ljoint"), (int)(2 * H)));
        TRY(fc_ln_relu_bwd(c, c.f("d_joint"), c.f("pooled_linear_l"), B, H, 2 * H, P->joint_fc, &G->joint_fc, 1, "pre_j",
                           "mean_j", "rstd_j", keep_site(bt, VQA_KEEP_SITE_JOINT), s.d.keep_joint, "d_pre_j", c.f("d_pl"), false));
        return fc_ln_relu_bwd(c, c.f("d_ljoint"), c.f("l_linear_l"), B, H, 2 * H, P->joint2, &G->joint2, 1, "pre_jl", "mean_jl",
                              "rstd_jl", keep_site(bt, VQA_KEEP_SITE_JOINT2), s.d.keep_joint, "d_pre_jl", c.f("d_ll"), false);
    }
    // joint_fc (dropout mask folded into the LN/ReLU backward)
    TRY(fc_ln_relu_bwd(c, c.f("d_joint"), c.f("joint_in"), B, H, 2 * H, P->joint_fc, &G->joint_fc, 1, "pre_j", "mean_j",
                       "rstd_j", keep_site(bt, VQA_KEEP_SITE_JOINT), s.d.keep_joint, "d_pre_j", c.f("d_joint_in"), false));
    if (!s.pair) {
        ProbeScope ps("eltwise", c.st);
        TRY(vqa_mul_bwd(c.f("d_joint_in"), c.f("pooled_linear_l"), c.f("l_linear_l"), c.f("d_pl"), c.f("d_ll"), B * H,
                        c.st));
    }
    return VQA_OK;
}

// vlmap_answer_ent: the regulariser's path back to l_linear_l (pooled_linear_l is behind tf.stop_gradient, :197): tile_z
// holds d loss / d logit; head and joint_fc are frozen (filter_train_vars :86-94), so only dX products run
int bwd_entropy(const Step& s) {
    const Ctx& c = s.c;
    const vqa_params_t* P = s.P;
    const int64_t B = s.B, H = s.H, A = s.A;
    ProbeScope ps("ent.bwd", c.st);
    const int64_t M = s.d.num_marginal, C = s.d.ent_cols;
    TRY(gemm(c, 0, 1, B * M, 2 * H, C, c.f("tile_z"), (int)C, P->head.w, (int)A, c.f("d_tile_joint"), (int)(2 * H)));
    TRY(vqa_ln_act_bwd_run(c.f("d_tile_joint"), c.f("pre_tj"), c.f("mean_tj"), c.f("rstd_tj"), P->joint_fc.gamma, P->joint_fc.beta,
                           keep_site(s.bt, VQA_KEEP_SITE_TILE).src(s.d.keep_joint, 2 * H), c.f("d_pre_tj"), nullptr, nullptr, nullptr,
                           (int)B, (int)M, (int)(2 * H), 0, c.st));
    TRY(gemm(c, 0, 1, B * M, H, 2 * H, c.f("d_pre_tj"), (int)(2 * H), P->joint_fc.w, (int)(2 * H), c.f("d_tile_in"), (int)H));
    // (paired LayerNorm backward: d_ll holds only this extra gradient and is added inside that kernel)
    return vqa_tile_mul_bwd(c.f("d_tile_in"), c.f("pooled_linear_l"), c.f("d_ll"), (int)B, (int)M, (int)H, s.pair ? 0 : 1, c.st);
}

// pooled_linear_l, and q_linear_l's LayerNorm where the two are paired: LayerNorm backward (paired with the product's, or
// on its own), then pooled_linear_l's FC half
int bwd_linear_l(const Step& s) {
    const Ctx& c = s.c;
    const vqa_params_t* P = s.P;
    const vqa_params_t* G = s.G;
    const int64_t B = s.B, H = s.H, Dp = s.Dp;
    if (!s.pair)
        return fc_ln_relu_bwd(c, c.f("d_pl"), c.f("pooled_V_ft"), B, Dp, H, P->pooled_linear_l, &G->pooled_linear_l, 1, "pre_pl",
                              "mean_pl", "rstd_pl", NO_KEEP, 1.f, "d_pre_pl", c.f("d_pooled"), false);
    const bool tr_pl = G->pooled_linear_l.w != nullptr, tr_ll = G->q_linear_l.w != nullptr;
    ProbeScope ps("fc.ln_bwd", c.st);
    TRY(vqa_ln_pair_mul_bwd(c.f("d_joint_in"), s.mt == VQA_MODEL_ENT ? c.f("d_ll") : nullptr, c.f("pre_pl"), c.f("pre_ll"),
                            c.f("mean_pl"), c.f("rstd_pl"), c.f("mean_ll"), c.f("rstd_ll"), P->pooled_linear_l.gamma,
                            P->pooled_linear_l.beta, P->q_linear_l.gamma, P->q_linear_l.beta, c.f("d_pre_pl"), c.f("d_pre_ll"),
                            tr_pl ? c.part(0) : nullptr, tr_pl ? c.part(1) : nullptr, tr_pl ? c.part(2) : nullptr,
                            tr_ll ? c.f("part_a1") : nullptr, tr_ll ? c.f("part_b1") : nullptr, tr_ll ? c.f("part_c1") : nullptr,
                            (int)B, (int)H, c.st));
    return fc_bwd_tail(c, c.f("pooled_V_ft"), B, Dp, H, P->pooled_linear_l, &G->pooled_linear_l, 1, c.f("d_pre_pl"), c.part(0),
                       c.part(1), c.part(2), c.f("d_pooled"), false);
}

// q_linear_l's FC half (after its LayerNorm backward, unless the paired kernel did it): x = what the layer read
int q_linear_l_bwd(const Step& s, const float* x, float* dx) {
    const Ctx& c = s.c;
    const int64_t B = s.B, H = s.H;
    if (s.pair)
        return fc_bwd_tail(c, x, B, H, H, s.P->q_linear_l, &s.G->q_linear_l, 1, c.f("d_pre_ll"), c.f("part_a1"), c.f("part_b1"),
                           c.f("part_c1"), dx, false);
    return fc_ln_relu_bwd(c, c.f("d_ll"), x, B, H, H, s.P->q_linear_l, &s.G->q_linear_l, 1, "pre_ll", "mean_ll", "rstd_ll", NO_KEEP,
                          1.f, "d_pre_ll", dx, false);
}

// q_linear_l and the ablations' layer under it: d_ll -> dh, the gradient wrt the question code
int bwd_question_code(const Step& s) {
    const Ctx& c = s.c;
    const vqa_params_t* P = s.P;
    const vqa_params_t* G = s.G;
    const int64_t B = s.B, H = s.H;
    const float* h = s.enc[0].h_final();      // the final GRU state hs[T]
    float* dh = s.dh;
    if (s.mt == VQA_MODEL_ANSWER2) {
        // q_linear_l read q_L_ft2: back through it, then through tanh + LN + FC (trainable) into dh
        TRY(q_linear_l_bwd(s, c.f("q_L_ft2"), c.f("d_ft2")));
        const bool train = G->q_L_ft2.w != nullptr;
        TRY(vqa_ln_act_bwd(c.f("d_ft2"), c.f("pre_ft2"), c.f("mean_ft2"), c.f("rstd_ft2"), P->q_L_ft2.gamma, P->q_L_ft2.beta,
                           nullptr, 1.f, c.f("d_pre_ft2"), train ? c.part(0) : nullptr, train ? c.part(1) : nullptr,
                           train ? c.part(2) : nullptr, (int)B, 1, (int)H, 1, c.st));
        if (train) {
            TRY(vqa_colsum3(c.part(0), c.part(1), c.part(2), (int)B, (int)H, (int)H, G->q_L_ft2.gamma, G->q_L_ft2.beta,
                            G->q_L_ft2.b, c.colsum_ws(), c.colsum_ws_floats(), c.st));
            TRY(gemm(c, 1, 0, H, H, B, h, (int)H, c.f("d_pre_ft2"), (int)H, G->q_L_ft2.w, (int)H));
        }
        return gemm(c, 0, 1, B, H, H, c.f("d_pre_ft2"), (int)H, P->q_L_ft2.w, (int)H, dh, (int)H);
    }
    if (s.mt == VQA_MODEL_NO_NOISE || s.mt == VQA_MODEL_FULL) {
        // q_linear_l read q_L_mean (+ noise * sigma): linear layers on the GRU state
        const bool full = s.mt == VQA_MODEL_FULL;
        float* d_in = c.f(full ? "d_lin" : "d_qm");
        TRY(q_linear_l_bwd(s, c.f(full ? "q_L_mean_noise" : "q_L_mean"), d_in));
        if (full)      // through x = mean + noise * sigma, plus the KL term's own gradient (weight / global batch)
            TRY(vqa_reparam_bwd(d_in, c.f("q_L_mean"), c.f("q_L_log_sigma_sq"), s.bt->noise,
                                s.d.extra_weight * s.d.inv_global_batch, c.f("d_qm"), c.f("d_qs"), B * H, c.st));
        if (G->q_L_mean.w != nullptr) {
            TRY(gemm(c, 1, 0, H, H, B, h, (int)H, c.f("d_qm"), (int)H, G->q_L_mean.w, (int)H));
            TRY(colsum(c, c.f("d_qm"), B, H, (int)H, G->q_L_mean.b));
        }
        TRY(gemm(c, 0, 1, B, H, H, c.f("d_qm"), (int)H, P->q_L_mean.w, (int)H, dh, (int)H));
        if (full) {
            if (G->q_L_log_sigma_sq.w != nullptr) {
                TRY(gemm(c, 1, 0, H, H, B, h, (int)H, c.f("d_qs"), (int)H, G->q_L_log_sigma_sq.w, (int)H));
                TRY(colsum(c, c.f("d_qs"), B, H, (int)H, G->q_L_log_sigma_sq.b));
            }
            TRY(gemm(c, 0, 1, B, H, H, c.f("d_qs"), (int)H, P->q_L_log_sigma_sq.w, (int)H, dh, (int)H, nullptr, dh, (int)H));
        }
        return VQA_OK;
    }
    return q_linear_l_bwd(s, s.mt == VQA_MODEL_BI ? c.f("q_L_ft") : h, dh);
}

// Whether the backward of v_linear_v's LayerNorm and of the attention score runs as one chain ("The fused
// v_linear_v chain"): on one stream, one query per memory, v_linear_v and the score trainable, 16-byte rows.  The separate
// calls stay for the side stream (VQA_HOT_OVERLAP=1), for vlmap_answer_adapt (a second consumer of att_score and a
// 1024-wide memory), for frozen layers and for every other shape.
bool vtail_ok(const Step& s, const Side& sd) {
    const Ctx& c = s.c;
    const vqa_params_t* P = s.P;
    const vqa_params_t* G = s.G;
    const vqa_batch_t* bt = s.bt;
    return vtail_mode() != 0 && !sd.ok && s.mt != VQA_MODEL_ADAPT && vqa_vtail_supported(1, (int)s.R, (int)s.H, (int)s.Dp) == 1 &&
           G->v_linear_v.w != nullptr && G->v_linear_v.gamma != nullptr && G->v_linear_v.beta != nullptr &&
           G->v_linear_v.b != nullptr && G->score.w != nullptr && G->score.b != nullptr && vqa_aligned16(c.f("d_pooled")) &&
           vqa_aligned16(P->score.w) && vqa_aligned16(P->v_linear_v.gamma) && vqa_aligned16(P->v_linear_v.beta) &&
           (bt->keep_att == nullptr || (reinterpret_cast<uintptr_t>(bt->keep_att) & 3u) == 0) &&
           vqa_aligned16(G->v_linear_v.gamma) && vqa_aligned16(G->v_linear_v.beta) && vqa_aligned16(G->v_linear_v.b) &&
           vqa_aligned16(G->score.w);
}

// attention + pooling, and v_linear_v behind it.  With one query per memory d_v is rank one per region, so the fused chain
// stops the attention backward at the score gradient ds, v_linear_v's LayerNorm backward forms d_v in registers and delivers
// d_qv and the score's weight partials, and one pair of launches reduces the five parameter gradients; d_v is not written on
// that path.  Otherwise: the attention backward, v_adapt, the score's gradients, then v_linear_v's backward -- on the side
// stream where there is one (its join is recorded here; side_wait follows q_linear_v).
int bwd_attention(Step& s) {
    const Ctx& c = s.c;
    const vqa_params_t* P = s.P;
    const vqa_params_t* G = s.G;
    const vqa_batch_t* bt = s.bt;
    const int64_t B = s.B, R = s.R, D = s.D, H = s.H, Dp = s.Dp;
    s.sd = &side_stream();
    if (vtail_ok(s, *s.sd)) {
        {
            ProbeScope ps("attn_pool.bwd", c.st);
            if (feat16(s.d))
                TRY(vqa_attn_pool_bwd_ds_v16(c.f("d_pooled"), c.u16("V_ft"), c.f("att_score"), c.f("ds"), c.f("part_db"), (int)B,
                                             1, (int)R, (int)H, (int)D, c.st));
            else
                TRY(vqa_attn_pool_bwd_ds(c.f("d_pooled"), c.f("V_ft"), c.f("att_score"), c.f("ds"), c.f("part_db"), (int)B, 1,
                                         (int)R, (int)H, (int)D, c.st));
        }
        {
            ProbeScope ps("v_linear_v.ln_bwd", c.st);
            TRY(vqa_ln_relu_att_bwd_run(c.f("ds"), c.f("q_linear_v"), P->score.w, keep_site(bt, VQA_KEEP_SITE_ATT).src(s.d.keep_att, H),
                                        c.f("pre_v"), c.f("mean_v"), c.f("rstd_v"), P->v_linear_v.gamma, P->v_linear_v.beta,
                                        c.f("d_pre_v"), c.part(0), c.part(1), c.part(2), c.f("d_qv"), c.f("part_dw"), (int)B, 1, (int)R,
                                        (int)H, (int)D, c.st));
            TRY(vqa_colsum_vtail(c.part(0), c.part(1), c.part(2), c.f("part_dw"), c.f("part_db"), (int)B, (int)H,
                                 G->v_linear_v.gamma, G->v_linear_v.beta, G->v_linear_v.b, G->score.w, G->score.b, c.colsum_ws(),
                                 c.colsum_ws_floats(), c.st));
        }
        ProbeScope ps("v_linear_v.dw_gemm", c.st);
        return gemm_x(c, 1, D, H, B * R, c.f("V_ft"), (int)D, c.f("d_pre_v"), (int)H, G->v_linear_v.w, (int)H);  // dW = x^T * d_pre
    }
    {
        ProbeScope ps("attn_pool.bwd", c.st);
        const bool v16 = feat16(s.d);
        const void* V = v16 ? (const void*)c.u16("V_ft") : (const void*)c.f(s.mt == VQA_MODEL_ADAPT ? "v_adapt" : "V_ft");
        TRY(vqa_attn_bwd_run(c.f("d_pooled"), c.f("v_linear_v"), c.f("q_linear_v"), V, v16, c.f("att_score"), P->score.w,
                             keep_site(bt, VQA_KEEP_SITE_ATT).src(s.d.keep_att, H), c.f("d_v"), c.f("d_qv"), c.f("part_dw"),
                             c.f("part_db"), (int)B, 1, (int)R, (int)H, (int)Dp, c.st));
    }
    if (s.mt == VQA_MODEL_ADAPT) {
        // the pooled memory is trainable here: d v_adapt = att (x) d pooled, then LN[R,H] + ReLU + FC backward (V_ft is an
        // input: parameters only), like v_linear_v's
        TRY(vqa_outer_rows(c.f("att_score"), c.f("d_pooled"), c.f("d_va"), (int)B, (int)R, (int)H, c.st));
        TRY(fc_ln_relu_bwd(c, c.f("d_va"), c.f("V_ft"), B * R, D, H, P->v_adapt, &G->v_adapt, (int)R, "pre_va", "mean_va",
                           "rstd_va", NO_KEEP, 1.f, "d_pre_va", nullptr, false));
    }
    if (G->score.w != nullptr) {
        ProbeScope ps("attn_pool.bwd", c.st);
        TRY(colsum(c, c.f("part_dw"), B, H, (int)H, G->score.w));
        TRY(colsum(c, c.f("part_db"), B, 1, 1, G->score.b));
    }
    // v_linear_v: parameters only (V_ft is an input).  77 GFLOP of dW on the side stream, beside
    // the latency-bound back-propagation through time below.
    s.forked = fork_side(c, *s.sd);
    const Ctx cv = s.side_ctx();
    TRY(fc_ln_relu_bwd(cv, cv.f("d_v"), cv.f("V_ft"), B * R, D, H, P->v_linear_v, &G->v_linear_v, (int)R, "pre_v",
                       "mean_v", "rstd_v", NO_KEEP, 1.f, "d_pre_v", nullptr, false));
    return side_record(s);
}

// q_linear_v: d_qv -> dh (accumulated); the bi-directional models go on through the question self-attention
int bwd_q_linear_v(const Step& s) {
    const Ctx& c = s.c;
    const int64_t B = s.B, H = s.H;
    if (s.mt == VQA_MODEL_BI) {
        // q_linear_v read pooled_q_v; from there back through the question self-attention into d q_L_ft (dh) / d q_L_map
        TRY(fc_ln_relu_bwd(c, c.f("d_qv"), c.f("pooled_q_v"), B, H, H, s.P->q_linear_v, &s.G->q_linear_v, 1, "pre_qv", "mean_qv",
                           "rstd_qv", NO_KEEP, 1.f, "d_pre_qv", c.f("d_pooled_qv"), false));
        return bi_question_bwd_head(c, s.P, s.G, s.bt, s.dh);
    }
    // q_linear_v: dh += ...
    return fc_ln_relu_bwd(c, c.f("d_qv"), s.enc[0].h_final(), B, H, H, s.P->q_linear_v, &s.G->q_linear_v, 1, "pre_qv", "mean_qv",
                          "rstd_qv", NO_KEEP, 1.f, "d_pre_qv", s.dh, true);
}

// phase 2: GRU back-propagation through time (gate math fused into the GEMM epilogues), dx, embedding scatter-add, slice
// sum of squares
int bwd_bptt(const Step& s, float* embed_slice_sq) {
    const Ctx& c = s.c;
    const vqa_params_t* P = s.P;
    const vqa_batch_t* bt = s.bt;
    const int64_t B = s.B, H = s.H, T = s.T, W = s.W;
    const GruTape& e = s.enc[0];
    float* dh = s.dh;
    const float *Wg_h = e.Wg_h(), *Wc_h = e.Wc_h();
    {
        ProbeScope ps("gru.bwd", c.st);
        switch (gru_form(GRU_BWD, T, B, H, bt->live_rows)) {
            case GRU_WS:
                // (hs[0] of this tape: fwd_question's zeros)
                TRY(vqa_gru_seq_bwd_ws_ex(dh, nullptr, Wg_h, Wc_h, bt->q_intseq_len, e.hs, e.gru_r, e.gru_u, e.gru_c, e.dxp, (int)T, (int)B,
                                          (int)H, h0skip_mode() & 1, c.find_f("gru_ws"), c.st));
                break;
            case GRU_LIVE:
                TRY(vqa_gru_seq_bwd_live(dh, Wg_h, Wc_h, bt->q_intseq_len, bt->live_rows, e.hs, e.gru_r, e.gru_u, e.gru_c, e.dxp,
                                         c.f("d_h1"), (int)T, (int)B, (int)H, c.st));
                break;
            case GRU_CHAINS: {
                float* dh1 = c.f("d_h1");
                TRY(run_chains(c, B, [&](int, int64_t row0, int64_t rows, hipStream_t st) {
                    return vqa_gru_seq_bwd_rows(dh, Wg_h, Wc_h, bt->q_intseq_len, e.hs, e.gru_r, e.gru_u, e.gru_c, e.dxp, dh1, (int)T,
                                                (int)B, (int)H, (int)row0, (int)rows, st);
                }));
                break;
            }
        }
    }
    // embedding: un-aggregated slices dx [T,B,W], then scatter-add
    float* dx = c.f("dx_embed");
    {
        ProbeScope ps("gru.dx_gemm", c.st);
        if (xcat_enabled()) {
            // wx_cat: the forward's packed copy of the x rows still sits in the workspace (backward follows the forward of the
            // same step on the same weights: every gradient here is meaningless otherwise); VQA_HOT_REPACK=1 packs it again
            if (repack_enabled()) TRY(e.pack_wx());
            TRY(e.dx(enc(c), dx));
        } else {
            TRY(gemm_enc(c, 0, 1, T * B, W, 2 * H, e.dxp, (int)(3 * H), P->gru_wg, (int)(2 * H), dx, (int)W));
            TRY(gemm_enc(c, 0, 1, T * B, W, H, e.dxp + 2 * H, (int)(3 * H), P->gru_wc, (int)H, dx, (int)W, nullptr, dx, (int)W));
        }
    }
    ProbeScope ps_embed("embed.bwd", c.st);
    if (s.G->embed != nullptr)
        TRY(vqa_embed_bwd_len_det(dx, bt->q_intseq, bt->q_intseq_len, s.G->embed, (int)B, (int)T, (int)W, s.d.Vq,
                                  (s.d.flags & VQA_FLAG_DETERMINISTIC) ? 1 : 0, c.st));
    if (embed_slice_sq != nullptr)
        TRY(vqa_sumsq(dx, T * B * W, nullptr, embed_slice_sq, c.f("sumsq_ws"), c.count("sumsq_ws"), c.st));
    return VQA_OK;
}

// Phases 4 and 8 of one cell e with gradients g (frozen: nothing).  packed: the x rows and biases of both kernels come out of
// one GEMM into dwx_cat; else fusion's two-GEMM form (VQA_HOT_XCAT=0).  The recurrent weight gradients (gru.dwh_gemm) start
// at the tape's rows of step t0: those of t = 0 are h_0 (gate kernel) or r * h_0 (candidate kernel), zeros since the forward
// cleared hs[0], and bit 1 of h0skip_mode() leaves them out for the question encoder.  Every product here is the
// encoder's (enc(c)): bf16 operands under VQA_FLAG_BF16_ENCODER_GEMMS, which the bi-directional model never carries.
int bwd_gru_weights(const Ctx& c, const GruTape& e, const GruCell& g, int phases, bool packed, int t0) {
    const int64_t TB = e.T * e.B, H = e.H, W = e.W;
    const int ld3 = (int)(3 * H);
    if (g.wg == nullptr) return VQA_OK;
    // phase 4: the gate kernel's weight and bias gradients; in the packed form the x rows and biases of BOTH kernels (the
    // candidate's bucket is reduced after phase 4)
    if (phases & 4) {
        {
            ProbeScope ps("gru.dwx_gemm", c.st);
            if (packed) {
                TRY(e.dwx(enc(c)));
                TRY(e.unpack_dwx(g));
            } else {
                TRY(gemm_enc(c, 1, 0, W, 2 * H, TB, e.x_tm, e.ldx(), e.dxp, ld3, g.wg, (int)(2 * H)));
                TRY(colsum(c, e.dxp, TB, 2 * H, ld3, g.bg));
            }
        }
        ProbeScope ps("gru.dwh_gemm", c.st);
        TRY(e.dwh(enc(c), g, false, t0));
    }
    // phase 8: the candidate kernel's weight and bias gradients (its x rows and bias only in the two-GEMM form)
    if (phases & 8) {
        if (!packed) {
            ProbeScope ps("gru.dwx_gemm", c.st);
            TRY(gemm_enc(c, 1, 0, W, H, TB, e.x_tm, e.ldx(), e.dxp + 2 * H, ld3, g.wc, (int)H));
            TRY(colsum(c, e.dxp + 2 * H, TB, H, ld3, g.bc));
        }
        ProbeScope ps("gru.dwh_gemm", c.st);
        TRY(e.dwh(enc(c), g, true, t0));
    }
    return VQA_OK;
}

}  // namespace

// phases (bit mask), in dependency order:
//   1  head .. attention .. v_linear_v / q_linear_v / score gradients      (complete after this phase)
//   2  GRU back-propagation through time, dx, embedding scatter-add, slice sum of squares
//   4  GRU gate weight / bias gradients (the larger half, 10.8 MB at H 1024)
//   8  GRU candidate weight / bias gradients (5.4 MB) -- the only all-reduce nothing is left to overlap with
// so a data-parallel caller can start all-reducing each gradient bucket while the next phase runs.
extern "C" int vqa_fusion_backward_phases(const vqa_dims_t* dims, const vqa_params_t* P, const vqa_params_t* G,
                                          const vqa_batch_t* bt, void* workspace, int64_t workspace_bytes,
                                          float* embed_slice_sq, int phases, void* stream) {
    VQA_REQUIRE(dims_ok(dims) && P && G && bt && workspace, VQA_ERR_ARG);
    VQA_REQUIRE(keep_sites_ok(bt), VQA_ERR_ARG);
    Step s(dims, P, G, bt, workspace, stream);
    VQA_REQUIRE(workspace_bytes >= s.L.total, VQA_ERR_WORKSPACE);
    ProbeScope ps_all("backward", s.c.st);
    if (s.mt == VQA_MODEL_LEGACY_VQA) return (phases & 1) ? legacy_vqa_backward(s.c, P, G, bt, embed_slice_sq) : VQA_OK;
    s.pair = ln_pair_ok(s.d, P);

    if (phases & 1) {
        TRY(bwd_head(s));
        TRY(bwd_joint(s));
        if (s.mt == VQA_MODEL_ENT) TRY(bwd_entropy(s));
        TRY(bwd_linear_l(s));
        TRY(bwd_question_code(s));
        TRY(bwd_attention(s));
        TRY(bwd_q_linear_v(s));
        TRY(side_wait(s));
    }
    if (s.mt == VQA_MODEL_BI) {
        if (phases & 2) TRY(bi_question_bwd_bptt(s.c, G, bt, s.enc, s.dh, embed_slice_sq));
        TRY(bwd_gru_weights(s.c, s.enc[0], fw_cell(G), phases, true, 0));
        return bwd_gru_weights(s.c, s.enc[1], bw_cell(G), phases, true, 0);
    }
    if (phases & 2) TRY(bwd_bptt(s, embed_slice_sq));
    return (phases & 12) ? bwd_gru_weights(s.c, s.enc[0], fw_cell(G), phases, xcat_enabled(), (h0skip_mode() >> 1) & 1) : VQA_OK;
}

extern "C" int vqa_hot_version(void) { return VQA_HOT_ABI_VERSION; }

extern "C" const char* vqa_hot_error_string(int code) {
    switch (code) {
        case VQA_OK: return "ok";
        case VQA_ERR_ARG: return "bad argument (size or null pointer)";
        case VQA_ERR_ALIGN: return "pointer / leading dimension not aligned";
        case VQA_ERR_LAUNCH: return "kernel launch failed";
        case VQA_ERR_UNSUPPORTED: return "unsupported configuration";
        case VQA_ERR_WORKSPACE: return "workspace too small";
        default: return "unknown error";
    }
}
