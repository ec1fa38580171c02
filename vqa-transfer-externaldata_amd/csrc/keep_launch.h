// Launch functions of the kernels that have a dropout site (layernorm.hip, attention.hip), with the site's keep source
// as a KeepSrc: what the explicit-mask and the *_seeded entry points of the C ABI wrap, and what the fusion step and the
// pre-training steps call directly (fusion_model.hip, pretrain_model.hip).  Same checks and return codes as the entry points; a combination of keep source, queries
// per memory and memory type that has no kernel is refused here.  Internal: nothing here is part of the C ABI.
#pragma once
#include "vqa_common.h"

// layernorm.hip.  act: 0 ReLU, 1 tanh.  Seeded: the 16-byte route only (VQA_ERR_ALIGN on the route of single columns)
int vqa_ln_act_fwd_run(const float* pre, const float* gamma, const float* beta, const KeepSrc& keep, float* y, float* mean,
                       float* rstd, int G, int rows, int N, int act, void* stream);
int vqa_ln_act_bwd_run(const float* dy, const float* pre, const float* mean, const float* rstd, const float* gamma,
                       const float* beta, const KeepSrc& keep, float* dpre, float* part_dgamma, float* part_dbeta,
                       float* part_dbias, int G, int rows, int N, int act, void* stream);
int vqa_ln_relu_att_bwd_run(const float* ds, const float* qv, const float* w, const KeepSrc& keep, const float* pre,
                            const float* mean, const float* rstd, const float* gamma, const float* beta, float* dpre,
                            float* part_dgamma, float* part_dbeta, float* part_dbias, float* dqv, float* part_dw, int B, int rep,
                            int R, int H, int D, void* stream);

// attention.hip.  V: float, or raw bf16 patterns (v_bf16).  rep queries per memory, 1..8, with any keep source (the mask
// of query q = m * rep + j: rows q * R .. of the [B * rep, R, H] mask or stream), for either memory type (the bf16
// pre-training steps run rep 5 over a bf16 memory; the C ABI's bf16 entry points are one query per memory).
// seeded_one_query: the contract of vqa_attn_pool_fwd_seeded / _bwd_seeded, which refuse a seeded source with rep != 1
// (VQA_ERR_UNSUPPORTED, where they always checked it)
int vqa_attn_fwd_run(const float* v, const float* qv, const void* V, bool v_bf16, const int32_t* nb, const float* w,
                     const float* bias, const KeepSrc& keep, float* att, float* pooled, int B, int rep, int R, int H, int D,
                     void* stream, bool seeded_one_query = false);
int vqa_attn_bwd_run(const float* dpooled, const float* v, const float* qv, const void* V, bool v_bf16, const float* att,
                     const float* w, const KeepSrc& keep, float* dv, float* dqv, float* part_dw, float* part_db, int B, int rep,
                     int R, int H, int D, void* stream, bool seeded_one_query = false);
