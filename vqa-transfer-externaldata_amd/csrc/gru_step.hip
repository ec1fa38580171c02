// Per-step GRU recurrence: tf.contrib.rnn.GRUCell + tf.nn.dynamic_rnn(sequence_length) (vlmap/modules.py:124-140) as
// two fused GEMM launches per time step, with the gate math in their epilogues.  Host code only: the kernels are the
// step GEMMs of gemm_f32.hip (vqa_gru_step_launch) and the row kernels of rowops.hip.  Every shape that the
// weight-stationary launch (gru_ws.hip) does not take runs here.  Tapes are time-major: xp / dxp [T,B,3H] (r | u | c),
// hs [T+1,B,H] (hs[0] = the initial state), r, u, c, rh [T,B,H].  The forward and the backward step are written once
// (fwd_step, bwd_step) on rows [row0, row0 + rows); the entry points differ in which rows they hand to each step.
// Every driver exists once, as a C++ function that takes the FORM of the step GEMMs (gru_step.h: f32, or the bf16 matrix
// unit of gru_step_bf16.hip); the extern "C" entry points forward the process-wide setting (GRU-step id GRU_CFG_BF16 =
// the bf16 form), a train step hands in its own.

#include "vqa_common.h"
#include "gemm_args.h"
#include "gemm_tiles.h"
#include "gru_step.h"

namespace {

// Tile config of the fused GRU-step GEMMs: many waves with small per-wave tiles (32x32), in-block split-k and two
// tiles of register prefetch hide the per-tile barrier and load latency better than 4 waves of 64x32 per CU, and
// every k group finishes its share of the rows in the epilogue (recurrence at B 512, H 1024, T 14: 622 -> 523 us
// forward, 607 -> 487 us backward).  Default: one 16-wave workgroup per CU (cfg 18), 32x32 tiles / 4 waves
// (cfg 16) once the live prefix is down to 256 rows, plain 4-wave tiles for tall batches.
// vqa_gemm_set_gru_config(cfg) forces one config on both directions (tests, tuning); -1 = defaults.
int g_gru_cfg = -1;
// Tall batches (the pre-training model runs 2560 rows per step) fill the chip with plain 4-wave tiles.
// (2560 rows, T 10: forward 1637 us with 64x64 BK 64, 1550 with BK 32 -- profiles/r2_gru_tune_b2560.txt)
// Between 512 and 2048 rows (the live prefix of the pre-training model's 2560-row recurrence passes through all of
// them) one 16-wave workgroup per CU is no longer the best form: 32x64 / 4-wave tiles forward (768 rows: 693 -> 565 us,
// 1536 rows: 1072 -> 961 us per 10 steps) and 64x32 tiles of 8 waves backward (632 -> 559, 995 -> 869);
// profiles/r2_gru_tune_rows.txt.
inline int gru_cfg_by_rows(int rows, int mid, int tall) {
    // (GRU_CFG_BF16 names a form, not a tile of the f32 kernels: an f32 recurrence under it runs the defaults)
    return (g_gru_cfg >= 0 && g_gru_cfg != GRU_CFG_BF16) ? g_gru_cfg : (rows >= 2048 ? tall : rows > 512 ? mid : rows > 256 ? 18 : 16);
}
inline int gru_cfg_fwd(int rows) {
    static const int mid = vqa_env_int("VQA_HOT_GRU_MID_FWD", 9), tall = vqa_env_int("VQA_HOT_GRU_TALL_FWD", 12);
    return gru_cfg_by_rows(rows, mid, tall);
}
// The H-wide candidate kernel of a tall batch takes 32x64 tiles: at 2560 rows x 1024 columns the 64x64 tile gives 640
// tiles (2.5 per CU, a half-empty last round), 32x64 gives 1280 (5 per CU): forward recurrence 1548 -> 1489 us at
// 2560 rows, T 10.  VQA_HOT_GRU_NARROW_CFG overrides (tuning; -1 = the same config as the gate kernel).
inline int gru_cfg_fwd_cand(int rows) {
    static const int narrow = vqa_env_int("VQA_HOT_GRU_NARROW_CFG", 9);
    return ((g_gru_cfg < 0 || g_gru_cfg == GRU_CFG_BF16) && rows >= 2048 && narrow >= 0) ? narrow : gru_cfg_fwd(rows);
}
inline int gru_cfg_bwd(int rows) {
    static const int mid = vqa_env_int("VQA_HOT_GRU_MID_BWD", 17), tall = vqa_env_int("VQA_HOT_GRU_TALL_BWD", 13);
    return gru_cfg_by_rows(rows, mid, tall);
}

// what every step of one recurrence shares (the entry points' own arguments)
struct FwdTape {
    float* xp; const float *Wg_h, *Wc_h; const int32_t* len; float *hs, *r, *u, *c, *rh;
    int B, H; hipStream_t st;
    int form;              // GRU_FORM_*
};
struct BwdTape {
    const float *Wg_h, *Wc_h; const int32_t* len; const float *hs, *r, *u, *c;
    const float* d_outs;   // gradient wrt every step's output [T,B,H], or null
    float* dxp; int B, H; hipStream_t st;
    int form;
};

// one fused step GEMM in the tape's form; `cfg`: the f32 form's tile (the bf16 form chooses its own by rows)
inline int step_launch(int form, int epi, int cfg, const GemmArgs& a, const EpiArgs& ep, hipStream_t st) {
    return form == GRU_FORM_BF16 ? vqa_gru_step_launch_bf16(epi, a, ep, st) : vqa_gru_step_launch(epi, cfg, a, ep, st);
}

// Forward step t on rows [row0, row0 + rows): gates (r, u, rh = r * h_prev), then candidate and the new state.
int fwd_step(const FwdTape& p, int t, int row0, int rows) {
    const int H = p.H;
    const int64_t BH = (int64_t)p.B * H, s = t * BH + (int64_t)row0 * H;   // the rows of step t in a [T,B,H] tape
    float* xpt = p.xp + s * 3;
    const float* hp = p.hs + s;
    EpiArgs eg{};
    eg.H = H; eg.h_prev = hp; eg.o0 = p.r + s; eg.o1 = p.u + s; eg.o2 = p.rh + s;
    GemmArgs ag = vqa_gemm_make_args(rows, 2 * H, H, hp, H, p.Wg_h, 2 * H, nullptr, 0, nullptr, xpt, 3 * H);
    int rc = step_launch(p.form, EPI_GATES, gru_cfg_fwd(rows), ag, eg, p.st);
    if (rc != VQA_OK) return rc;
    EpiArgs ec{};
    ec.H = H; ec.t = t; ec.len = p.len + row0; ec.h_prev = hp; ec.i0 = p.u + s; ec.o0 = p.c + s; ec.o1 = p.hs + s + BH;
    GemmArgs ac = vqa_gemm_make_args(rows, H, H, p.rh + s, H, p.Wc_h, H, nullptr, 0, nullptr, xpt + 2 * H, 3 * H);
    return step_launch(p.form, EPI_CAND, gru_cfg_fwd_cand(rows), ac, ec, p.st);
}

// Second half of backward step t on rows [row0, row0 + rows), whose first half (vqa_gru_bwd_a: dc_pre, du_pre, dh_acc)
// is done: `cur` holds these rows' running dL/dh_{t-1} (partial).
//   drh = dc_pre * Wc_h^T ; epilogue: dr_pre, cur += drh * r
//   t > 0: (+ d_outs of step t-1) ; dh_{t-1} = (dr_pre | du_pre) * Wg_h^T + cur ; epilogue: first half of step t-1,
//          whose dh_acc goes to `other`; the two buffers then change roles
int bwd_step(const BwdTape& p, int t, int row0, int rows, float*& cur, float*& other) {
    const int H = p.H, ld = 3 * H;
    const int64_t BH = (int64_t)p.B * H, s = t * BH + (int64_t)row0 * H;
    float* dxpt = p.dxp + s * 3;
    EpiArgs e1{};
    e1.H = H; e1.ldo = ld; e1.h_prev = p.hs + s; e1.i0 = p.r + s; e1.o0 = dxpt; e1.o1 = cur;
    GemmArgs a1 = vqa_gemm_make_args(rows, H, H, dxpt + 2 * H, ld, p.Wc_h, H, nullptr, 0, nullptr, nullptr, 0);
    int rc = step_launch(p.form, EPI_BWD_RH, gru_cfg_bwd(rows), a1, e1, p.st);
    if (rc != VQA_OK || t == 0) return rc;
    const int64_t sp = s - BH;   // step t-1
    if (p.d_outs) {
        rc = vqa_add_inplace(cur, p.d_outs + sp, (int64_t)rows * H, p.st);     // + dL/d(output of step t-1)
        if (rc != VQA_OK) return rc;
    }
    float* dxpp = p.dxp + sp * 3;
    EpiArgs e2{};
    e2.H = H; e2.t = t - 1; e2.ldo = ld; e2.len = p.len + row0; e2.h_prev = p.hs + sp;
    e2.i0 = p.u + sp; e2.i1 = p.c + sp; e2.o0 = dxpp + 2 * H; e2.o1 = dxpp + H; e2.o2 = other;
    GemmArgs a2 = vqa_gemm_make_args(rows, H, 2 * H, dxpt, ld, p.Wg_h, 2 * H, nullptr, 0, nullptr, cur, H);
    rc = step_launch(p.form, EPI_BWD_DH, gru_cfg_bwd(rows), a2, e2, p.st);
    float* x = cur; cur = other; other = x;
    return rc;
}

// Backward over all T steps of the row window [row0, row0 + rows): the first half of step T-1 from dh_T (+ d_outs),
// then every step.  The running gradient starts in dh_scratch and alternates with dh_T.
int bwd_window(const BwdTape& p, float* dh_T, float* dh_scratch, int T, int row0, int rows) {
    if (T == 0 || rows == 0) return VQA_OK;
    const int H = p.H, ld = 3 * H;
    const int64_t o = (int64_t)row0 * H, s = (int64_t)(T - 1) * p.B * H + o;
    float *other = dh_T + o, *cur = dh_scratch + o;
    float* dxpt = p.dxp + s * 3;
    int rc = p.d_outs ? vqa_add_inplace(other, p.d_outs + s, (int64_t)rows * H, p.st) : VQA_OK;
    if (rc != VQA_OK) return rc;
    rc = vqa_gru_bwd_a(other, p.hs + s, p.u + s, p.c + s, p.len + row0, T - 1, dxpt + 2 * H, ld, dxpt + H, ld, cur, rows, H,
                       p.st);
    for (int t = T - 1; t >= 0 && rc == VQA_OK; --t) rc = bwd_step(p, t, row0, rows, cur, other);
    return rc;
}

inline int global_form() { return g_gru_cfg == GRU_CFG_BF16 ? GRU_FORM_BF16 : GRU_FORM_F32; }
inline bool form_ok(int form) { return form == GRU_FORM_F32 || form == GRU_FORM_BF16; }

}  // namespace

extern "C" int vqa_gemm_set_gru_config(int cfg) {
    VQA_REQUIRE(cfg == -1 || cfg == GRU_CFG_BF16 || vqa_gru_cfg_known(cfg), VQA_ERR_ARG);
    g_gru_cfg = cfg;   // -1 restores the defaults
    return VQA_OK;
}

extern "C" int vqa_gru_seq_fwd(float* xp, const float* Wg_h, const float* Wc_h, const int32_t* len, float* hs,
                               float* r, float* u, float* c, float* rh, int T, int B, int H, void* stream) {
    return gru_seq_fwd_rows_form(global_form(), xp, Wg_h, Wc_h, len, hs, r, u, c, rh, T, B, H, 0, B, stream);
}

// rows [row0, row0 + rows) of the batch only (independent chains: one per stream)
extern "C" int vqa_gru_seq_fwd_rows(float* xp, const float* Wg_h, const float* Wc_h, const int32_t* len, float* hs,
                                    float* r, float* u, float* c, float* rh, int T, int B, int H, int row0, int rows,
                                    void* stream) {
    return gru_seq_fwd_rows_form(global_form(), xp, Wg_h, Wc_h, len, hs, r, u, c, rh, T, B, H, row0, rows, stream);
}
int gru_seq_fwd_rows_form(int form, float* xp, const float* Wg_h, const float* Wc_h, const int32_t* len, float* hs, float* r,
                          float* u, float* c, float* rh, int T, int B, int H, int row0, int rows, void* stream) {
    VQA_REQUIRE(form_ok(form), VQA_ERR_ARG);
    VQA_REQUIRE(xp && Wg_h && Wc_h && len && hs && r && u && c && rh && T >= 0 && B > 0 && H > 0, VQA_ERR_ARG);
    VQA_REQUIRE(row0 >= 0 && rows >= 0 && row0 + rows <= B, VQA_ERR_ARG);
    VQA_REQUIRE(H % 4 == 0, VQA_ERR_ALIGN);
    if (rows == 0) return VQA_OK;
    const FwdTape p{xp, Wg_h, Wc_h, len, hs, r, u, c, rh, B, H, static_cast<hipStream_t>(stream), form};
    int rc = VQA_OK;
    for (int t = 0; t < T && rc == VQA_OK; ++t) rc = fwd_step(p, t, row0, rows);
    return rc;
}

// Recurrence over the LIVE prefix only.  Contract: the batch rows are sorted by length, longest first, and
// live_rows[t] (HOST array of T ints) = number of rows with len > t.  Step t then runs on rows [0, live_rows[t])
// -- the gate / candidate GEMMs shrink with the sequences that are still running (real questions average ~6 of
// 14 tokens) -- and finished rows are filled in afterwards exactly as the masked recurrence leaves them.
extern "C" int vqa_gru_seq_fwd_live(float* xp, const float* Wg_h, const float* Wc_h, const int32_t* len,
                                    const int32_t* live_rows, float* hs, float* r, float* u, float* c, float* rh,
                                    int T, int B, int H, void* stream) {
    return gru_seq_fwd_live_form(global_form(), xp, Wg_h, Wc_h, len, live_rows, hs, r, u, c, rh, T, B, H, stream);
}
int gru_seq_fwd_live_form(int form, float* xp, const float* Wg_h, const float* Wc_h, const int32_t* len,
                          const int32_t* live_rows, float* hs, float* r, float* u, float* c, float* rh, int T, int B, int H,
                          void* stream) {
    VQA_REQUIRE(form_ok(form), VQA_ERR_ARG);
    VQA_REQUIRE(xp && Wg_h && Wc_h && len && live_rows && hs && r && u && c && rh && T >= 0 && B > 0 && H > 0, VQA_ERR_ARG);
    VQA_REQUIRE(H % 4 == 0, VQA_ERR_ALIGN);
    const FwdTape p{xp, Wg_h, Wc_h, len, hs, r, u, c, rh, B, H, static_cast<hipStream_t>(stream), form};
    int prev = B;
    for (int t = 0; t < T; ++t) {
        const int rows = live_rows[t];
        VQA_REQUIRE(rows >= 0 && rows <= prev, VQA_ERR_ARG);      // non-increasing
        prev = rows;
        if (rows == 0) break;
        const int rc = fwd_step(p, t, 0, rows);
        if (rc != VQA_OK) return rc;
    }
    return vqa_gru_fill_finished(hs, rh, len, T, B, H, stream);
}

// Back-propagation through time.  dh_T [B,H] is the gradient wrt the final state (consumed: used as scratch, it and
// dh_scratch [B,H] alternate as the running state gradient); dxp [T,B,3H] receives (dr_pre | du_pre | dc_pre) per
// step, exactly 0 for t >= len[b].  The gradient wrt the initial state hs[0] (zeros, not trained) is not formed: step 0
// stops after dr_pre.
extern "C" int vqa_gru_seq_bwd(float* dh_T, const float* Wg_h, const float* Wc_h, const int32_t* len,
                               const float* hs, const float* r, const float* u, const float* c, float* dxp,
                               float* dh_scratch, int T, int B, int H, void* stream) {
    return gru_seq_bwd_rows_form(global_form(), dh_T, Wg_h, Wc_h, len, hs, r, u, c, dxp, dh_scratch, T, B, H, 0, B, stream);
}

extern "C" int vqa_gru_seq_bwd_rows(float* dh_T, const float* Wg_h, const float* Wc_h, const int32_t* len,
                                    const float* hs, const float* r, const float* u, const float* c, float* dxp,
                                    float* dh_scratch, int T, int B, int H, int row0, int rows, void* stream) {
    return gru_seq_bwd_rows_form(global_form(), dh_T, Wg_h, Wc_h, len, hs, r, u, c, dxp, dh_scratch, T, B, H, row0, rows,
                                 stream);
}
int gru_seq_bwd_rows_form(int form, float* dh_T, const float* Wg_h, const float* Wc_h, const int32_t* len, const float* hs,
                          const float* r, const float* u, const float* c, float* dxp, float* dh_scratch, int T, int B, int H,
                          int row0, int rows, void* stream) {
    VQA_REQUIRE(form_ok(form), VQA_ERR_ARG);
    VQA_REQUIRE(dh_T && Wg_h && Wc_h && len && hs && r && u && c && dxp && dh_scratch && T >= 0 && B > 0 && H > 0,
                VQA_ERR_ARG);
    VQA_REQUIRE(row0 >= 0 && rows >= 0 && row0 + rows <= B, VQA_ERR_ARG);
    VQA_REQUIRE(H % 4 == 0, VQA_ERR_ALIGN);
    const BwdTape p{Wg_h, Wc_h, len, hs, r, u, c, nullptr, dxp, B, H, static_cast<hipStream_t>(stream), form};
    return bwd_window(p, dh_T, dh_scratch, T, row0, rows);
}

// BPTT of a recurrence whose per-step OUTPUTS are consumed too (the bi-directional encoder of vqa/model_vlmap_finetune.py:
// q_L_map = every step's state): d_outs [T,B,H], the gradient wrt the output of step t (zero where t >= len, as
// dynamic_rnn zeroes those outputs), joins the running state gradient before step t is differentiated -- one small add
// per step in front of the same two fused launches as vqa_gru_seq_bwd.
extern "C" int vqa_gru_seq_bwd_outs(float* dh_T, const float* Wg_h, const float* Wc_h, const int32_t* len, const float* hs,
                                    const float* r, const float* u, const float* c, const float* d_outs, float* dxp,
                                    float* dh_scratch, int T, int B, int H, void* stream) {
    VQA_REQUIRE(dh_T && Wg_h && Wc_h && len && hs && r && u && c && d_outs && dxp && dh_scratch && T >= 0 && B > 0 && H > 0,
                VQA_ERR_ARG);
    VQA_REQUIRE(H % 4 == 0, VQA_ERR_ALIGN);
    const BwdTape p{Wg_h, Wc_h, len, hs, r, u, c, d_outs, dxp, B, H, static_cast<hipStream_t>(stream), global_form()};
    return bwd_window(p, dh_T, dh_scratch, T, 0, B);
}

// The live-prefix form of vqa_gru_seq_fwd_live (same contract for live_rows): a row enters the recurrence at its own
// last step, from dL/dh_final, and step t runs on rows [0, live_rows[t]); dxp of finished steps is zero.
extern "C" int vqa_gru_seq_bwd_live(float* dh_T, const float* Wg_h, const float* Wc_h, const int32_t* len,
                                    const int32_t* live_rows, const float* hs, const float* r, const float* u,
                                    const float* c, float* dxp, float* dh_scratch, int T, int B, int H, void* stream) {
    return gru_seq_bwd_live_form(global_form(), dh_T, Wg_h, Wc_h, len, live_rows, hs, r, u, c, dxp, dh_scratch, T, B, H,
                                 stream);
}
int gru_seq_bwd_live_form(int form, float* dh_T, const float* Wg_h, const float* Wc_h, const int32_t* len,
                          const int32_t* live_rows, const float* hs, const float* r, const float* u, const float* c,
                          float* dxp, float* dh_scratch, int T, int B, int H, void* stream) {
    VQA_REQUIRE(form_ok(form), VQA_ERR_ARG);
    VQA_REQUIRE(dh_T && Wg_h && Wc_h && len && live_rows && hs && r && u && c && dxp && dh_scratch, VQA_ERR_ARG);
    VQA_REQUIRE(T >= 0 && B > 0 && H > 0, VQA_ERR_ARG);
    VQA_REQUIRE(H % 4 == 0, VQA_ERR_ALIGN);
    if (T == 0) return VQA_OK;
    const BwdTape p{Wg_h, Wc_h, len, hs, r, u, c, nullptr, dxp, B, H, static_cast<hipStream_t>(stream), form};
    const int64_t BH = (int64_t)B * H;
    const int ld = 3 * H;
    // both state-gradient buffers start as dL/dh_final: a row is first touched at its own last step
    if (hipMemcpyAsync(dh_scratch, dh_T, (size_t)BH * sizeof(float), hipMemcpyDeviceToDevice, p.st) != hipSuccess)
        return VQA_ERR_LAUNCH;
    int rc = vqa_gru_zero_finished(dxp, len, T, B, H, stream);
    if (rc != VQA_OK) return rc;
    float *cur = dh_T, *other = dh_scratch;
    int entered = 0;   // rows [0, entered) already carry a running dh_acc in `cur`
    for (int t = T - 1; t >= 0; --t) {
        const int rows = live_rows[t];
        VQA_REQUIRE(rows >= entered && rows <= B, VQA_ERR_ARG);
        if (rows > entered) {   // rows whose LAST step is t: first half of the step from dL/dh_final, in place
            const int64_t o = (int64_t)entered * H, s = t * BH + o;
            float* dxpt = dxp + s * 3;
            rc = vqa_gru_bwd_a(cur + o, hs + s, u + s, c + s, len + entered, t, dxpt + 2 * H, ld, dxpt + H, ld, cur + o,
                               rows - entered, H, stream);
            if (rc != VQA_OK) return rc;
            entered = rows;
        }
        if (rows == 0) continue;
        rc = bwd_step(p, t, 0, rows, cur, other);
        if (rc != VQA_OK) return rc;
    }
    return VQA_OK;
}
