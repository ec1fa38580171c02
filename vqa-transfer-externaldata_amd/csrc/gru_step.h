// The per-step GRU recurrence drivers of gru_step.hip with the form of their step GEMMs as an argument.  The extern "C"
// entry points of the same names (vqa_gru_seq_*) forward the process-wide setting of vqa_gemm_set_gru_config; a train
// step that owns a flag for the form (VQA_PT_FLAG_BF16_ENCODER) calls these, so two engines in one process do not share it.
// Arguments after `form`: those of the entry point.  Internal: not part of the C ABI.
#pragma once
#include <stdint.h>

enum { GRU_FORM_F32 = 0, GRU_FORM_BF16 = 1 };      // f32 step kernels (gemm_f32.hip) / bf16 operands (gru_step_bf16.hip)

int gru_seq_fwd_rows_form(int form, float* xp, const float* Wg_h, const float* Wc_h, const int32_t* len, float* hs, float* r,
                          float* u, float* c, float* rh, int T, int B, int H, int row0, int rows, void* stream);
int gru_seq_fwd_live_form(int form, float* xp, const float* Wg_h, const float* Wc_h, const int32_t* len,
                          const int32_t* live_rows, float* hs, float* r, float* u, float* c, float* rh, int T, int B, int H,
                          void* stream);
int gru_seq_bwd_rows_form(int form, float* dh_T, const float* Wg_h, const float* Wc_h, const int32_t* len, const float* hs,
                          const float* r, const float* u, const float* c, float* dxp, float* dh_scratch, int T, int B, int H,
                          int row0, int rows, void* stream);
int gru_seq_bwd_live_form(int form, float* dh_T, const float* Wg_h, const float* Wc_h, const int32_t* len,
                          const int32_t* live_rows, const float* hs, const float* r, const float* u, const float* c,
                          float* dxp, float* dh_scratch, int T, int B, int H, void* stream);
