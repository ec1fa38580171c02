// The sequence encoder around the GRU recurrence, for the host-composed steps (fusion_model.hip: the question encoder and
// the two cells of the bi-directional model; pretrain_model.hip: the caption and the context batch).  The one place that
// knows the format of the packed x-projection:
//   wx_cat [W,3H], bx_cat [3H]   the x rows and biases of the gate kernel [W+H,2H] and the candidate kernel [W+H,H] side
//                                by side (vqa_gru_pack_wx), so all steps are projected by one GEMM
//   x_tm [T,B,x_stride(W)]       the inputs, time-major, with the constant 1 in column W
//   xp, dxp [T,B,3H]             projection and its gradient as r | u | c, leading dimension 3H: candidate part at + 2H
//   dwx_cat [x_stride(W),3H]     x_tm^T dxp; row W (the constant input) holds both bias gradients (vqa_gru_unpack_dwx_bias)
//   hs [T+1,B,H]                 the state tape; hs[0] is the initial state, cleared by clear_h0
//   gru_r, gru_u, gru_c, gru_rh [T,B,H]   the gates' tape; gru_rh = r * h_{t-1}, the left operand of the candidate kernel
// Each user calls the steps in its own order, picks the form of the recurrence itself (the vqa_gru_seq_* calls take their
// pointers from the tape) and hands in its own product as `gemm(tA, tB, M, N, K, A, lda, B, ldb, C, ldc, bias)`.
// Internal: not part of the C ABI.
#pragma once
#include "step_workspace.h"
#include "vqa_common.h"

struct GruCell { float *wg, *bg, *wc, *bc; };      // gate / candidate kernel and bias of one cell, or their gradients

struct GruTape {
    float *x_tm, *xp, *wx_cat, *bx_cat, *dwx_cat, *hs, *gru_r, *gru_u, *gru_c, *gru_rh, *dxp;
    int64_t T, B, H, W;
    GruCell p;      // the cell's variables
    hipStream_t st;
    GruTape() = default;
    // the buffers <tape><name><suffix> (inputs and forward tape) and <scratch><name><suffix> (packed x rows, backward)
    GruTape(const Workspace& w, const std::string& tape, const std::string& scratch, const std::string& suffix, int64_t T_,
            int64_t B_, int64_t H_, int64_t W_, const GruCell& p_, hipStream_t st_)
        : T(T_), B(B_), H(H_), W(W_), p(p_), st(st_) {
        auto in = [&](const char* n) { return w.f(tape + n + suffix); };
        auto scr = [&](const char* n) { return w.f(scratch + n + suffix); };
        x_tm = in("x_tm"); xp = in("xp"); hs = in("hs");
        gru_r = in("gru_r"); gru_u = in("gru_u"); gru_c = in("gru_c"); gru_rh = in("gru_rh");
        wx_cat = scr("wx_cat"); bx_cat = scr("bx_cat"); dwx_cat = scr("dwx_cat"); dxp = scr("dxp");
    }
    int ldx() const { return (int)x_stride(W); }
    const float* Wg_h() const { return p.wg + W * 2 * H; }      // the recurrent rows of the two kernels
    const float* Wc_h() const { return p.wc + W * H; }
    float* h_final() const { return hs + T * B * H; }      // hs[T]

    int pack_wx() const { return vqa_gru_pack_wx(p.wg, p.wc, p.bg, p.bc, wx_cat, bx_cat, (int)W, (int)H, st); }
    template <class Gemm>
    int project(Gemm&& gemm) const {      // xp = x_tm wx_cat + bx_cat, all steps
        return gemm(0, 0, T * B, 3 * H, W, x_tm, ldx(), wx_cat, (int)(3 * H), xp, (int)(3 * H), bx_cat);
    }
    int clear_h0() const { return hipMemsetAsync(hs, 0, (size_t)(B * H) * 4, st) == hipSuccess ? VQA_OK : VQA_ERR_LAUNCH; }
    template <class Gemm>
    int dx(Gemm&& gemm, float* dx_out) const {      // dx [T,B,W] = dxp wx_cat^T
        return gemm(0, 1, T * B, W, 3 * H, dxp, (int)(3 * H), wx_cat, (int)(3 * H), dx_out, (int)W, nullptr);
    }
    template <class Gemm>
    int dwx(Gemm&& gemm) const {
        return gemm(1, 0, x_stride(W), 3 * H, T * B, x_tm, ldx(), dxp, (int)(3 * H), dwx_cat, (int)(3 * H), nullptr);
    }
    int unpack_dwx(const GruCell& g) const { return vqa_gru_unpack_dwx_bias(dwx_cat, g.wg, g.wc, g.bg, g.bc, (int)W, (int)H, st); }
    // A recurrent weight gradient of g: the gate kernel's rows W.. = hs[t0..T-1]^T dxp_{r|u}, or (cand) the candidate kernel's
    // = gru_rh[t0..T-1]^T dxp_c.  t0 = 1 where the caller knows the rows of step 0 to be zero (hs[0] cleared: h_0 and r * h_0);
    // with no step left the block, which the GEMM overwrites, is cleared (rows W.. of a [W+H,N] gradient: contiguous).
    template <class Gemm>
    int dwh(Gemm&& gemm, const GruCell& g, bool cand, int t0) const {
        const int64_t N = cand ? H : 2 * H, row0 = t0 * B;
        float* dW = cand ? g.wc + W * H : g.wg + W * 2 * H;
        if (t0 >= T) return hipMemsetAsync(dW, 0, (size_t)(H * N) * 4, st) == hipSuccess ? VQA_OK : VQA_ERR_LAUNCH;
        return gemm(1, 0, H, N, (T - t0) * B, (cand ? gru_rh : hs) + row0 * H, (int)H, dxp + row0 * 3 * H + (cand ? 2 * H : 0),
                    (int)(3 * H), dW, (int)N, nullptr);
    }
};
