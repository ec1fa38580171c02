// Host-side composition of the pre-training models: one call enqueues the whole forward (or backward)
// pass on the caller's stream -- the counterpart of vqa_fusion_forward / vqa_fusion_backward for the fusion model.
// ONE model description, ONE prologue, ONE forward and ONE backward serve every model: a model is a head set on one of
// three architectures (Model), and each public family only adapts its structs to the internal views (Params, Batch):
//   vqa_pretrain_*        cfg 5, vlmap_memft/model_vlmap_bf_or_wordset_withatt_sp.py: heads bf | ws, standard
//   vqa_pretrain_ext_*    model_vlmap_bf_or_wordset_enwiki_withatt_sp.py (bf | ws | ew), model_vlmap_bf_enwiki_withatt_sp.py
//                         (bf | ew), and bf | ws = cfg 5 bit for bit; standard
//   vqa_pretrain_noc_*    the "no composition" heads on the same trunk (noc_heads_fwd / noc_heads_bwd)
//   vqa_pretrain_adapt_*  the v_adapt layer between the features and the attention pooling (v_adapt_fwd / v_adapt_bwd)
// No family calls another family's entry points.
//
// Per category k in {object, attribute} (reference lines relative to the cfg-5 file):
//   build_*_V_ft      :323-364, :414-455   6-d box -> FC 1024 + LN + ReLU for the 36 regions (once per image) and the
//                                          n = 5 key boxes, Hadamard attention + pooling over the raw features with the
//                                          x5 tile of V_ft never materialised (attn_pool_*_rep)
//   build_*_blank_fill:505-609             L_GloVe embedding -> GRU over the caption with a blank (length-sorted live
//                                          prefix) -> fusion MLP -> classifier -> masked softmax-CE, top-1 / top-5
//   build_*_wordset   :366-412, :457-503   tanh(word-set embedding) -> FC + LN + tanh -> the same fusion MLP
//   build_*_enwiki    (enwiki file :519-624) enwiki_map embedding of the answer's Wikipedia context -> a second GRU
//                                          (encode_L_enwiki, shared by both categories) -> the same fusion MLP and
//                                          classifier -> masked softmax-CE over the blank-fill fills
//   n_way_classification_loss :675-706
// Head h = 2 r + k for the type of rank r among the enabled ones (bf < ws < ew) and category k; the heads share
// pooled_linear_l, q_linear_l, joint_fc and the classifier, so their rows are stacked and every shared FC is ONE GEMM
// over NH Bn rows (2 Bn for pooled_linear_l): for cfg 5, M = 2560 leaves the last round of tiles half empty (1260 tiles of
// 128x64 on 512 workgroup slots = 2.46 rounds), M = 10240 does not (9.84).  LayerNorm and the loss run per slice.
// LayerNorm variables of an fc_layer scope entered by several call sites: with VQA_FLAG_SHARED_LN (what TF 1.x builds:
// leaving the string-named scope zeroes its sub-scope counts, so the un-scoped layers.layer_norm gets the un-suffixed
// name again and AUTO_REUSE shares it -- oracle/pretrain_oracle.py) every call site uses slot 0 and the
// call sites' d_gamma / d_beta are accumulated; without the flag each call site owns slot [k] (V_ft / blank-fill /
// wordset_ft) or [h] (the heads of the shared fusion MLP) in TF graph build order.
//
// The workspace layout is a function of the dims alone, so the host views named intermediates without copies.
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "gru_encoder.h"
#include "gru_step.h"
#include "keep_launch.h"

namespace {

// ---------------------------------------------------------------- small kernels of this model
// key6 = (y1, x1, y2, x2, y2 - y1, x2 - x1)   (:330-333)
__global__ __launch_bounds__(256) void box6_kernel(const float* __restrict__ key, float* __restrict__ key6, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 b = reinterpret_cast<const float4*>(key)[i];
    float* o = key6 + (int64_t)i * 6;
    o[0] = b.x; o[1] = b.y; o[2] = b.z; o[3] = b.w; o[4] = b.z - b.x; o[5] = b.w - b.y;
}

// valid[b, j] = j < num[b] ; inv_valid = 1 / sum(valid)     (tf.sequence_mask + reduce_sum, :675-706); under data
// parallelism the sum runs over the GLOBAL batch and is handed in (global_valid > 0)
__global__ __launch_bounds__(256) void valid_kernel(const int32_t* __restrict__ num, float* __restrict__ valid,
                                                    float* __restrict__ inv_valid, int B, int n, float global_valid) {
    __shared__ float red[16];
    float tot = 0.f;
    for (int i = threadIdx.x; i < B * n; i += 256) {
        const float v = (i % n) < num[i / n] ? 1.f : 0.f;
        valid[i] = v;
        tot += v;
    }
    tot = block_sum(tot, red);
    if (threadIdx.x == 0) inv_valid[0] = 1.f / (global_valid > 0.f ? global_valid : tot);
}

// out[i, :] = in[index[i], :]   (rows of `cols` 4-byte words; index == NULL copies)
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint32_t* __restrict__ in, const int32_t* __restrict__ index,
                                                          uint32_t* __restrict__ out, int rows, int cols) {
    const int64_t total = (int64_t)rows * cols;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int r = (int)(i / cols), c = (int)(i - (int64_t)r * cols);
        out[i] = in[(int64_t)(index ? index[r] : r) * cols + c];
    }
}

// out[i, :] = (in0 ++ in1)[index[i], :]: rows 0..rows0-1 of the virtual concatenation live in in0, the rest in in1
// (the captions of the two categories arrive as two arrays and are encoded as ONE batch)
__global__ __launch_bounds__(256) void gather_rows2_kernel(const uint32_t* __restrict__ in0, const uint32_t* __restrict__ in1,
                                                           const int32_t* __restrict__ index, uint32_t* __restrict__ out,
                                                           int rows, int cols, int rows0) {
    const int64_t total = (int64_t)rows * cols;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int r = (int)(i / cols), c = (int)(i - (int64_t)r * cols);
        int s = index ? index[r] : r;
        s = min(max(s, 0), rows - 1);
        out[i] = s < rows0 ? in0[(int64_t)s * cols + c] : in1[(int64_t)(s - rows0) * cols + c];
    }
}

// ---------------------------------------------------------------- workspace layout (step_workspace.h)
const char* const KIND[2] = {"obj", "attr"};
const char* const HEAD[3] = {"bf", "ws", "ew"};      // blank fill, word set, enwiki context
const char* const TASK[3] = {"blank_fill", "wordset", "enwiki"};

inline bool feat16(const vqa_pretrain_dims_t& d) { return (d.flags & VQA_FLAG_BF16_FEATURES) != 0; }      // image_ft is bf16 patterns
inline bool enc16(const vqa_pretrain_dims_t& d) { return (d.flags & VQA_PT_FLAG_BF16_ENCODER) != 0; }       // both encoders are routed

// (bf16 features and the bf16 encoder only on top of the bf16 GEMMs: every query and every pass of every family goes
// through here, so either flag alone is VQA_ERR_ARG before anything is launched)
bool dims_ok(const vqa_pretrain_dims_t* d) {
    return d && d->B > 0 && d->n > 0 && d->n <= 8 && d->R > 0 && d->D > 0 && d->H > 0 && d->W > 0 && d->A > 0 &&
           d->Vq > 0 && d->n_ws > 0 && d->L > 0 && d->H % 4 == 0 && d->D % 4 == 0 &&
           (!(feat16(*d) || enc16(*d)) || (d->flags & VQA_FLAG_BF16_GEMM)) &&
           !(d->flags & VQA_FLAG_BF16_ENCODER_GEMMS);      // the VQA step's switch: these steps' is VQA_PT_FLAG_BF16_ENCODER
}

struct Ctx : Workspace {
    const vqa_pretrain_dims_t& d;
    hipStream_t st;
    const vqa_pretrain_keep_t* keep = nullptr;      // the *_ex entry points' seeded sites; NULL: every site reads its mask
    // The keep source of one dropout site: `bit` = its VQA_PT_KEEP_SITE_* bit, `mask` = its mask pointer of the batch, `off`
    // = its stream offset of the keep struct, row_len = the row length of the op that consumes it.  Every mask site of
    // the forward and the backward resolves through here and hands the result to the op's launch function (keep_launch.h).
    KeepSrc site(int bit, const uint8_t* mask, uint64_t off, float keep_prob, int64_t row_len) const {
        if (keep != nullptr && (keep->seeded & bit)) return KeepSrc::seeded(keep->keep_seed, off, row_len, keep_prob);
        return KeepSrc::bytes(mask, keep_prob);
    }
    // LayerNorm slot of call site `site` of an fc_layer scope: slot 0 for every site under VQA_FLAG_SHARED_LN
    int li(int site) const { return (d.flags & VQA_FLAG_SHARED_LN) ? 0 : site; }
    // The f32 MFMA product, whatever the flags say: wordset_ft, the K = 6 box layers and -- without
    // VQA_PT_FLAG_BF16_ENCODER -- both encoders (x-projection, dx, dwx, dwh) call this one (include/vqa_hot.h,
    // VQA_FLAG_BF16_GEMM: the unrouted list).
    int gemm_f32(int tA, int tB, int64_t M, int64_t N, int64_t K, const float* A, int lda, const float* B, int ldb, float* C,
                 int ldc, const float* bias = nullptr, const float* D = nullptr, int ldd = 0) const {
        return vqa_gemm_f32(tA, tB, (int)M, (int)N, (int)K, A, lda, B, ldb, C, ldc, bias, D, ldd, 0, f("gemm_ws"),
                            count("gemm_ws"), st);
    }
    auto f32() const { return [this](auto... a) { return gemm_f32(a...); }; }      // as a callable (gru_encoder.h)
    auto routed() const { return [this](auto... a) { return gemm_routed(a...); }; }
    // what the encoders run: the routed product and the bf16 recurrence under VQA_PT_FLAG_BF16_ENCODER (which implies
    // VQA_FLAG_BF16_GEMM, dims_ok), else the f32 product and the recurrence's entry points as they always were
    bool enc_routed() const { return enc16(d); }
    // The routed layers' products (forward, dW, dx): bf16 operands in the matrix unit under VQA_FLAG_BF16_GEMM, else f32.
    // A shape the bf16 kernel refuses is its error return, never a silent f32 product.  Every call site names one of the
    // two wrappers: there is no default a new site could pick up by accident.
    // a16: the left operand is the features under VQA_FLAG_BF16_FEATURES -- raw bf16 patterns behind the float pointer, lda
    // in elements; the flag implies VQA_FLAG_BF16_GEMM (dims_ok), so there is no f32 form of it.
    int gemm_routed(int tA, int tB, int64_t M, int64_t N, int64_t K, const float* A, int lda, const float* B, int ldb,
                    float* C, int ldc, const float* bias = nullptr, const float* D = nullptr, int ldd = 0,
                    bool a16 = false) const {
        if (a16)
            return vqa_gemm_bf16_a16(tA, tB, (int)M, (int)N, (int)K, reinterpret_cast<const uint16_t*>(A), lda, B, ldb, C, ldc,
                                     bias, D, ldd, 0, f("gemm_ws"), count("gemm_ws"), 0, st);
        if (d.flags & VQA_FLAG_BF16_GEMM)
            return vqa_gemm_bf16(tA, tB, (int)M, (int)N, (int)K, A, lda, B, ldb, C, ldc, bias, D, ldd, 0, f("gemm_ws"),
                                 count("gemm_ws"), 0, st);
        return gemm_f32(tA, tB, M, N, K, A, lda, B, ldb, C, ldc, bias, D, ldd);
    }
};
enum Prec { PREC_F32, PREC_ROUTED };      // which of the two a helper shared by routed and unrouted layers uses

// modules.fc_layer forward: FC on the last axis, layer_norm over groups of `rows` rows, activation (0 relu, 1 tanh).
// Its users are the unrouted layers (K = 6 box layers, wordset_ft): the product is f32 in every mode.
int fc_ln_fwd(const Ctx& c, const float* x, int64_t M, int64_t K, int64_t N, const vqa_pt_fc6_t& p, int ln, int rows,
              int act, const std::string& pre, const std::string& y, const std::string& mean, const std::string& rstd,
              const KeepSrc& keep) {
    TRY(c.gemm_f32(0, 0, M, N, K, x, (int)K, p.w, (int)N, c.f(pre), (int)N, p.b));
    return vqa_ln_act_fwd_run(c.f(pre), p.gamma[ln], p.beta[ln], keep, c.f(y), c.f(mean), c.f(rstd), (int)(M / rows), rows,
                              (int)N, act, c.st);
}
const KeepSrc NO_KEEP;      // a layer without dropout

// Gradient accumulation over the call sites that share a variable: the first contribution overwrites (gradient
// buffers are not cleared between steps), later ones add.
struct Acc {
    const Ctx& c;
    std::set<const float*> touched;
    int vec(float* grad, const float* value, int64_t n) {      // value already computed somewhere else
        if (touched.insert(grad).second)
            return hipMemcpyAsync(grad, value, (size_t)n * 4, hipMemcpyDeviceToDevice, c.st) == hipSuccess ? VQA_OK : VQA_ERR_LAUNCH;
        return vqa_add_inplace(grad, value, n, c.st);
    }
    // dW (+)= x^T * dpre, through the wrapper the call site names; the in-place addend of a second touch goes through
    // the same kernel's D == C form.  No model touches a ROUTED weight twice today (every routed layer is one stacked
    // product; the second touches are wordset_ft and the box layers, f32), so no step-level test runs the bf16 kernel's
    // D == C form: it is covered by the op tests of vqa_gemm_bf16 only (tests/test_gpu_bf16.py, in-place addend).
    // x16: x is the features under VQA_FLAG_BF16_FEATURES (Ctx::gemm_routed's a16; a routed layer's only)
    int weight(Prec prec, float* gw, const float* x, int ldx, const float* dpre, int ldp, int64_t K, int64_t N, int64_t M,
               bool x16 = false) {
        const bool first = touched.insert(gw).second;
        const float* add = first ? nullptr : gw;
        if (prec == PREC_ROUTED) return c.gemm_routed(1, 0, K, N, M, x, ldx, dpre, ldp, gw, (int)N, nullptr, add, (int)N, x16);
        return c.gemm_f32(1, 0, K, N, M, x, ldx, dpre, ldp, gw, (int)N, nullptr, add, (int)N);
    }
    auto as_gemm(Prec prec) {      // weight(prec, ...) in the argument order of a GEMM call with tA = 1, tB = 0 (gru_encoder.h)
        return [this, prec](int, int, int64_t K, int64_t N, int64_t M, const float* x, int ldx, const float* dy, int ldy, float* gw,
                            int, const float*) { return weight(prec, gw, x, ldx, dy, ldy, K, N, M); };
    }
    // three column sums (d_gamma, d_beta, d_bias partials [G, N]) into their gradients: first touch overwrites, later
    // ones add inside the reduction's last pass (no temporaries, no add kernels)
    int colsum3(const float* p0, const float* p1, const float* p2, int64_t G, int64_t N, float* g0, float* g1, float* g2) {
        const int mask = (touched.count(g0) ? 1 : 0) | (touched.count(g1) ? 2 : 0) | (touched.count(g2) ? 4 : 0);
        TRY(vqa_colsum3_acc(p0, p1, p2, (int)G, (int)N, (int)N, g0, g1, g2, mask, c.f("colsum_ws"), c.count("colsum_ws"),
                            c.st));
        touched.insert(g0); touched.insert(g1); touched.insert(g2);
        return VQA_OK;
    }
    int colsum(const float* X, int64_t M, int64_t N, int ldx, float* grad) {
        const bool first = touched.insert(grad).second;
        return vqa_colsum_acc(X, (int)M, (int)N, ldx, grad, first ? 0 : 1, c.f("colsum_ws"), c.count("colsum_ws"), c.st);
    }
};

// backward of the LayerNorm / activation half of fc_ln_fwd on pointers (the stacked heads hand in their slices):
// dy -> d_pre; gamma, beta and bias gradients accumulated
int ln_bwd(const Ctx& c, Acc& acc, const float* dy, int64_t M, int64_t N, const vqa_pt_fc6_t& p, const vqa_pt_fc6_t& g, int ln,
           int rows, int act, const float* pre, const float* mean, const float* rstd, const KeepSrc& keep, float* d_pre) {
    const int64_t G = M / rows;
    TRY(vqa_ln_act_bwd_run(dy, pre, mean, rstd, p.gamma[ln], p.beta[ln], keep, d_pre, c.f("part_a"), c.f("part_b"),
                           c.f("part_c"), (int)G, rows, (int)N, act, c.st));
    return acc.colsum3(c.f("part_a"), c.f("part_b"), c.f("part_c"), G, N, g.gamma[ln], g.beta[ln], g.b);
}

// backward of the FC half: dW (+)= x^T d_pre, optional dx = d_pre * W^T
int fc_bwd(const Ctx& c, Acc& acc, Prec prec, const std::string& d_pre, const float* x, int64_t M, int64_t K, int64_t N,
           const vqa_pt_fc6_t& p, const vqa_pt_fc6_t& g, float* dx) {
    TRY(acc.weight(prec, g.w, x, (int)K, c.f(d_pre), (int)N, K, N, M));
    if (dx == nullptr) return VQA_OK;
    if (prec == PREC_ROUTED) return c.gemm_routed(0, 1, M, K, N, c.f(d_pre), (int)N, p.w, (int)N, dx, (int)K);
    return c.gemm_f32(0, 1, M, K, N, c.f(d_pre), (int)N, p.w, (int)N, dx, (int)K);
}

// backward of fc_ln_fwd (the unrouted layers: f32 products)
int fc_ln_bwd(const Ctx& c, Acc& acc, const float* dy, const float* x, int64_t M, int64_t K, int64_t N, const vqa_pt_fc6_t& p,
              const vqa_pt_fc6_t& g, int ln, int rows, int act, const std::string& pre, const std::string& mean,
              const std::string& rstd, const KeepSrc& keep, const std::string& d_pre, float* dx) {
    TRY(ln_bwd(c, acc, dy, M, N, p, g, ln, rows, act, c.f(pre), c.f(mean), c.f(rstd), keep, c.f(d_pre)));
    return fc_bwd(c, acc, PREC_F32, d_pre, x, M, K, N, p, g, dx);
}

int gather_rows(const void* in, const int32_t* index, void* out, int64_t rows, int64_t cols, hipStream_t st) {
    if (rows * cols == 0) return VQA_OK;
    const int grid = (int)std::min<int64_t>((rows * cols + 255) / 256, 4096);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid), dim3(256), 0, st, static_cast<const uint32_t*>(in), index,
                       static_cast<uint32_t*>(out), (int)rows, (int)cols);
    VQA_CHECK_LAUNCH();
    return VQA_OK;
}

int gather_rows2(const void* in0, const void* in1, const int32_t* index, void* out, int64_t rows, int64_t cols,
                 int64_t rows0, hipStream_t st) {
    if (rows * cols == 0) return VQA_OK;
    const int grid = (int)std::min<int64_t>((rows * cols + 255) / 256, 4096);
    hipLaunchKernelGGL(gather_rows2_kernel, dim3(grid), dim3(256), 0, st, static_cast<const uint32_t*>(in0),
                       static_cast<const uint32_t*>(in1), index, static_cast<uint32_t*>(out), (int)rows, (int)cols, (int)rows0);
    VQA_CHECK_LAUNCH();
    return VQA_OK;
}

struct HeadSet {
    int type[3] = {0, 0, 0};      // type of rank r (0 blank fill, 1 word set, 2 enwiki)
    int rank[3] = {-1, -1, -1};   // rank of type t, -1 = not enabled
    int nt = 0;
    explicit HeadSet(int mask) {
        for (int t = 0; t < 3; ++t)
            if (mask & (1 << t)) { rank[t] = nt; type[nt++] = t; }
    }
    int nh() const { return 2 * nt; }
    // workspace prefix of head h = 2 r + k: "<obj|attr>/<bf|ws|ew>/"
    std::string name(int h) const { return std::string(KIND[h & 1]) + "/" + HEAD[type[h >> 1]] + "/"; }
};

// The architecture of a model: what sits between the features and the attention pooling, and which head block follows
// the shared head inputs.  noc: the "no composition" heads (two joint branches and two logit blocks per head instead of
// jin / joint_fc / classifier); adapt: the attention pools the adapted memory v_adapt [B,R,H], so the pooled width is H
enum Arch { ARCH_STANDARD, ARCH_NOC, ARCH_ADAPT };

// the head sets an architecture has a model for
bool heads_ok(Arch arch, int heads) {
    if (!(heads & VQA_PT_HEAD_BF) || (heads & ~(VQA_PT_HEAD_BF | VQA_PT_HEAD_WS | VQA_PT_HEAD_EW))) return false;
    if (arch == ARCH_NOC) return heads == (VQA_PT_HEAD_BF | VQA_PT_HEAD_WS) || heads == (VQA_PT_HEAD_BF | VQA_PT_HEAD_EW);
    return arch == ARCH_STANDARD || heads == (VQA_PT_HEAD_BF | VQA_PT_HEAD_WS);
}

bool noc_split(int type) { return type != 0; }      // noc: blank fill SUM, word set / enwiki SPLIT

// report[3 i + j] (i = k * nt + r: the key order of vqa_pretrain_ext_report_key), report[3 nh] = sum of the losses
struct ReportExtArgs { const float* stats[6]; const float* inv[6]; int rows, nh; };
__global__ __launch_bounds__(256) void pretrain_ext_report_kernel(ReportExtArgs a, float* __restrict__ report) {
    __shared__ float red[16];
    __shared__ float loss[6];
    for (int h = 0; h < a.nh; ++h) {
        for (int j = 0; j < 3; ++j) {
            float s = 0.f;
            for (int i = threadIdx.x; i < a.rows; i += 256) s += a.stats[h][(int64_t)i * 4 + j];
            s = block_sum(s, red);
            if (threadIdx.x == 0) {
                const float v = s * a.inv[h][0];
                report[3 * h + j] = v;
                if (j == 0) loss[h] = v;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = loss[0];
        for (int h = 1; h < a.nh; ++h) t += loss[h];
        report[3 * a.nh] = t;
    }
}

Layout make_layout_ext(const vqa_pretrain_ext_dims_t& dx, bool noc, bool adapt) {
    const vqa_pretrain_dims_t& d = dx.base;
    const HeadSet hs(dx.heads);
    Layout L;
    const int64_t B = d.B, n = d.n, R = d.R, H = d.H, W = d.W, A = d.A, T = d.L, Bn = B * n, NH = hs.nh();
    const int64_t D = adapt ? d.H : d.D;      // width of the pooled memory
    const int64_t Tc = hs.rank[2] >= 0 ? dx.Lc : 0;
    L.add("S/pooled", 2 * Bn * D); L.add("S/vl_pre", 2 * Bn * H); L.add("S/lft", NH * Bn * H);
    L.add("S/vl", NH * Bn * H); L.add("S/ll_pre", NH * Bn * H); L.add("S/ll", NH * Bn * H);
    if (noc) {
        L.add("S/jv_pre", NH * Bn * 2 * H); L.add("S/jv", NH * Bn * 2 * H);
        L.add("S/jl_pre", NH * Bn * 2 * H); L.add("S/jl", NH * Bn * 2 * H);
        L.add("S/zv", NH * Bn * A); L.add("S/zl", NH * Bn * A); L.add("S/dzv", NH * Bn * A); L.add("S/dzl", NH * Bn * A);
        L.add("S/stats", NH * Bn * 4); L.add("S/stats_l", NH * Bn * 4);
    } else {
        L.add("S/jin", NH * Bn * H);
        L.add("S/j_pre", NH * Bn * 2 * H); L.add("S/j", NH * Bn * 2 * H);
        L.add("S/z", NH * Bn * A); L.add("S/dz", NH * Bn * A); L.add("S/stats", NH * Bn * 4);
    }
    for (int k = 0; k < 2; ++k) {
        const std::string p = std::string(KIND[k]) + "/";
        L.add(p + "key6", Bn * 6);
        L.add(p + "v_pre", B * R * H); L.add(p + "v", B * R * H); L.add(p + "v_mean", B); L.add(p + "v_rstd", B);
        L.add(p + "qv_pre", Bn * H); L.add(p + "qv", Bn * H); L.add(p + "qv_mean", B); L.add(p + "qv_rstd", B);
        L.add(p + "att", Bn * R);
        L.alias(p + "pooled", "S/pooled", k * Bn * D, Bn * D); L.alias(p + "vl_pre", "S/vl_pre", k * Bn * H, Bn * H);
        L.add(p + "valid", Bn); L.add(p + "inv_valid", 4);
        L.alias(p + "bf_state", "S/lft", k * Bn * H, Bn * H);
        if (hs.rank[1] >= 0) {
            L.add(p + "wse", Bn * W); L.add(p + "ws", Bn * W);
            L.add(p + "wf_pre", Bn * H); L.alias(p + "wf", "S/lft", (2 * hs.rank[1] + k) * Bn * H, Bn * H);
            L.add(p + "wf_mean", B); L.add(p + "wf_rstd", B);
        }
        if (hs.rank[2] >= 0) L.alias(p + "ew_state", "S/lft", (2 * hs.rank[2] + k) * Bn * H, Bn * H);
        for (int r = 0; r < hs.nt; ++r) {
            const std::string q = p + HEAD[hs.type[r]] + "/";
            const int64_t h = 2 * r + k;
            L.alias(q + "vl", "S/vl", h * Bn * H, Bn * H); L.add(q + "vl_mean", B); L.add(q + "vl_rstd", B);
            L.alias(q + "ll_pre", "S/ll_pre", h * Bn * H, Bn * H); L.alias(q + "ll", "S/ll", h * Bn * H, Bn * H);
            L.add(q + "ll_mean", B); L.add(q + "ll_rstd", B);
            if (noc) {
                for (const char* br : {"v", "l"}) {
                    const std::string b = br;
                    L.alias(q + "j" + b + "_pre", "S/j" + b + "_pre", h * Bn * 2 * H, Bn * 2 * H);
                    L.alias(q + "j" + b, "S/j" + b, h * Bn * 2 * H, Bn * 2 * H);
                    L.add(q + "j" + b + "_mean", B); L.add(q + "j" + b + "_rstd", B);
                    L.alias(q + "z" + b, "S/z" + b, h * Bn * A, Bn * A); L.alias(q + "dz" + b, "S/dz" + b, h * Bn * A, Bn * A);
                }
                L.alias(q + "stats", "S/stats", h * Bn * 4, Bn * 4); L.alias(q + "stats_l", "S/stats_l", h * Bn * 4, Bn * 4);
                continue;
            }
            L.alias(q + "jin", "S/jin", h * Bn * H, Bn * H);
            L.alias(q + "j_pre", "S/j_pre", h * Bn * 2 * H, Bn * 2 * H); L.alias(q + "j", "S/j", h * Bn * 2 * H, Bn * 2 * H);
            L.add(q + "j_mean", B); L.add(q + "j_rstd", B);
            L.alias(q + "z", "S/z", h * Bn * A, Bn * A); L.alias(q + "dz", "S/dz", h * Bn * A, Bn * A);
            L.alias(q + "stats", "S/stats", h * Bn * 4, Bn * 4);
        }
    }
    // captions (J/) and enwiki contexts (E/) of both categories, each one batch of 2 Bn rows, time-major
    L.add("J/blanks_s", 2 * Bn * T); L.add("J/lens_s", 2 * Bn);
    L.add("J/x_tm", T * 2 * Bn * x_stride(W)); L.add("J/xp", T * 2 * Bn * 3 * H); L.add("J/hs", (T + 1) * 2 * Bn * H);
    L.add("J/gru_r", T * 2 * Bn * H); L.add("J/gru_u", T * 2 * Bn * H); L.add("J/gru_c", T * 2 * Bn * H);
    L.add("J/gru_rh", T * 2 * Bn * H);
    L.add("wx_cat", W * 3 * H); L.add("bx_cat", 3 * H); L.add("dwx_cat", x_stride(W) * 3 * H);
    if (Tc > 0) {
        L.add("E/ctx_s", 2 * Bn * Tc); L.add("E/lens_s", 2 * Bn);
        L.add("E/x_tm", Tc * 2 * Bn * x_stride(W)); L.add("E/xp", Tc * 2 * Bn * 3 * H); L.add("E/hs", (Tc + 1) * 2 * Bn * H);
        L.add("E/gru_r", Tc * 2 * Bn * H); L.add("E/gru_u", Tc * 2 * Bn * H); L.add("E/gru_c", Tc * 2 * Bn * H);
        L.add("E/gru_rh", Tc * 2 * Bn * H);
        L.add("E/wx_cat", W * 3 * H); L.add("E/bx_cat", 3 * H); L.add("E/dwx_cat", x_stride(W) * 3 * H);
        L.add("E/d_state_s", 2 * Bn * H); L.add("E/dxp", Tc * 2 * Bn * 3 * H); L.add("E/dx", Tc * 2 * Bn * W);
    }
    L.add("report", 32);
    if (noc) {
        L.add("d_jv", NH * Bn * 2 * H); L.add("d_jvpre", NH * Bn * 2 * H);
        L.add("d_jl", NH * Bn * 2 * H); L.add("d_jlpre", NH * Bn * 2 * H);
    } else {
        L.add("d_j", NH * Bn * 2 * H); L.add("d_jpre", NH * Bn * 2 * H); L.add("d_jin", NH * Bn * H);
    }
    L.add("d_vl", NH * Bn * H); L.add("d_ll", NH * Bn * H); L.add("d_vlpre", NH * Bn * H); L.add("d_llpre", NH * Bn * H);
    L.add("d_lft", NH * Bn * H); L.add("d_pooled", 2 * Bn * D);
    L.add("d_state_s", 2 * Bn * H); L.add("d_hscratch", 2 * Bn * H);
    L.add("dxp", T * 2 * Bn * 3 * H); L.add("dx", T * 2 * Bn * W);
    L.add("d_wfpre", Bn * H); L.add("d_ws", Bn * W); L.add("d_wse", Bn * W);
    L.add("d_v", B * R * H); L.add("d_vpre", B * R * H); L.add("d_qv", Bn * H); L.add("d_qvpre", Bn * H);
    L.add("part_a", B * 2 * H); L.add("part_b", B * 2 * H); L.add("part_c", B * 2 * H);
    L.add("part_dw", Bn * H); L.add("part_db", Bn);
    L.add("sq", 16);
    int64_t gw = 4;
    auto g = [&](int tA, int tB, int64_t M, int64_t N, int64_t K) {
        gw = max64(gw, vqa_gemm_workspace_floats(tA, tB, (int)M, (int)N, (int)K, 0));
    };
    // a routed product: under VQA_FLAG_BF16_GEMM also what the bf16 kernel's shape-chosen split k needs
    auto gr = [&](int tA, int tB, int64_t M, int64_t N, int64_t K) {
        g(tA, tB, M, N, K);
        if (d.flags & VQA_FLAG_BF16_GEMM) gw = max64(gw, vqa_gemm_bf16_workspace_floats((int)M, (int)N, (int)K, 0));
    };
    if (adapt) {
        // v_adapt: ONE pre-activation per image (the x n tile and the second category repeat it), one output per
        // LayerNorm: shared -> "obj/va" and "attr/va" name the same buffer
        const int64_t S = B * R * H;
        const bool ln_shared = (d.flags & VQA_FLAG_SHARED_LN) != 0;
        L.add("va_pre", S);
        if (ln_shared) {
            L.add("va", S); L.add("va_mean", B); L.add("va_rstd", B);
        }
        for (int k = 0; k < 2; ++k) {
            const std::string p = std::string(KIND[k]) + "/";
            if (ln_shared) {
                L.alias(p + "va", "va", 0, S); L.alias(p + "va_mean", "va_mean", 0, B); L.alias(p + "va_rstd", "va_rstd", 0, B);
            } else {
                L.add(p + "va", S); L.add(p + "va_mean", B); L.add(p + "va_rstd", B);
            }
        }
        L.add("d_va", S); L.add("d_vapre", S);
        if (!ln_shared) L.add("d_vapre1", S);      // the attribute call site's d_pre before the two meet
        gr(0, 0, B * R, H, d.D); gr(1, 0, d.D, H, B * R);
    }
    g(0, 0, B * R, H, 6); g(0, 0, Bn, H, 6); g(0, 0, Bn, H, W);
    g(1, 0, 6, H, B * R); g(1, 0, 6, H, Bn); g(1, 0, W, H, Bn); g(0, 1, Bn, W, H);
    for (const int64_t S : {T, Tc}) {        // the two recurrences' x-projection, its dW / dx and the h-row dW
        if (S == 0) continue;
        // (routed under VQA_PT_FLAG_BF16_ENCODER only: without it the sizing is what it was)
        auto ge = [&](int tA, int tB, int64_t M, int64_t N, int64_t K) { enc16(d) ? gr(tA, tB, M, N, K) : g(tA, tB, M, N, K); };
        ge(0, 0, S * 2 * Bn, 3 * H, W); ge(1, 0, x_stride(W), 3 * H, S * 2 * Bn); ge(0, 1, S * 2 * Bn, W, 3 * H);
        ge(1, 0, H, 2 * H, S * 2 * Bn); ge(1, 0, H, H, S * 2 * Bn);
    }
    // the routed layers: pooled_linear_l, q_linear_l, the joint layer(s) and the classifier(s), forward / dW / dx
    gr(0, 0, 2 * Bn, H, D); gr(0, 0, NH * Bn, H, H); gr(0, 0, NH * Bn, 2 * H, H); gr(0, 0, NH * Bn, A, 2 * H);
    gr(1, 0, 2 * H, A, NH * Bn); gr(0, 1, NH * Bn, 2 * H, A); gr(1, 0, H, 2 * H, NH * Bn); gr(0, 1, NH * Bn, H, 2 * H);
    gr(1, 0, D, H, 2 * Bn); gr(0, 1, 2 * Bn, D, H); gr(1, 0, H, H, NH * Bn); gr(0, 1, NH * Bn, H, H);
    L.add("gemm_ws", gw);
    int64_t cw = 4;
    cw = max64(cw, vqa_colsum_workspace_floats((int)B, (int)(2 * H)));
    cw = max64(cw, vqa_colsum_workspace_floats((int)(NH * Bn), (int)A));
    cw = max64(cw, vqa_colsum_workspace_floats((int)Bn, (int)H));
    cw = max64(cw, vqa_colsum_workspace_floats((int)B, (int)H));
    cw = max64(cw, vqa_colsum_workspace_floats((int)Bn, 1));
    L.add("colsum_ws", 3 * cw);
    L.add("sumsq_ws", max64(max64(vqa_sumsq_workspace_floats(2 * T * Bn * W), vqa_sumsq_workspace_floats(2 * Tc * Bn * W)),
                            max64(vqa_sumsq_workspace_floats(Bn * W), 4)));
    return L;
}

// ---------------------------------------------------------------- the normalised view of a call
// Every public family (vqa_pretrain_*, _ext_*, _noc_*, _adapt_*) hands its structs to an adapter (Model::cfg5 / Model::of,
// view()) and runs the ONE prologue, forward and backward below on the result.  The views hold pointers only.

// report keys of a head set in report order: per category, per enabled type <kind>_<task>_{loss,acc,top_5_acc} (a SPLIT
// head of a noc model: <kind>_<task>_v_{...} then <kind>_<task>_l_{...}); then total_loss
std::vector<std::string> report_keys(Arch arch, int heads) {
    const HeadSet hs(heads);
    std::vector<std::string> keys;
    for (int k = 0; k < 2; ++k)
        for (int r = 0; r < hs.nt; ++r) {
            const std::string base = std::string(KIND[k]) + "_" + TASK[hs.type[r]];
            const bool split = arch == ARCH_NOC && noc_split(hs.type[r]);
            for (const char* br : split ? std::vector<const char*>{"_v", "_l"} : std::vector<const char*>{""})
                for (const char* suf : {"_loss", "_acc", "_top_5_acc"}) keys.push_back(base + br + suf);
        }
    keys.push_back("total_loss");
    return keys;
}

// vqa_pretrain_*_report_key of every family; NULL past the last key or for a head set the architecture has no model for
const char* report_key(Arch arch, int heads, int i) {
    static std::vector<std::string> keys[3][8];        // built once; the pointers stay valid
    static const int init = [] {
        for (const Arch a : {ARCH_STANDARD, ARCH_NOC, ARCH_ADAPT})
            for (int m = 0; m < 8; ++m)
                if (heads_ok(a, m)) keys[a][m] = report_keys(a, m);
        return 0;
    }();
    (void)init;
    if (heads < 0 || heads >= 8 || i < 0 || i >= (int)keys[arch][heads].size()) return nullptr;
    return keys[arch][heads][i].c_str();
}

// The model of a call: the dims of the variable head set plus the architecture.  The one place that maps a family to its
// dims check, its layout and its probe labels.
struct Model {
    vqa_pretrain_ext_dims_t dims{};
    Arch arch = ARCH_STANDARD;
    bool ok = false;      // the family's dims check
    // vqa_pretrain_*: heads bf | ws, no context batch
    static Model cfg5(const vqa_pretrain_dims_t* d) {
        Model m;
        if ((m.ok = dims_ok(d))) m.dims = vqa_pretrain_ext_dims_t{*d, VQA_PT_HEAD_BF | VQA_PT_HEAD_WS, 0, 0};
        return m;
    }
    static Model of(const vqa_pretrain_ext_dims_t* d, Arch arch) {
        Model m;
        m.arch = arch;
        m.ok = d != nullptr && dims_ok(&d->base) && heads_ok(arch, d->heads) &&
               (!(d->heads & VQA_PT_HEAD_EW) || (d->Lc > 0 && d->n_ctx > 0));
        if (m.ok) m.dims = *d;
        return m;
    }
    Layout layout() const { return make_layout_ext(dims, arch == ARCH_NOC, arch == ARCH_ADAPT); }
    bool ln_shared() const { return (dims.base.flags & VQA_FLAG_SHARED_LN) != 0; }
    const char* fwd_label() const { return arch == ARCH_NOC ? "pretrain_noc.forward" : "pretrain_ext.forward"; }
    const char* bwd_label() const { return arch == ARCH_NOC ? "pretrain_noc.backward" : "pretrain_ext.backward"; }
};

int64_t layout_bytes(const Model& m) { return m.ok ? m.layout().total : VQA_ERR_ARG; }

// vqa_pretrain_*_tensor of every family: a name of the layout -> byte offset and element count
int layout_tensor(const Model& m, const char* name, int64_t* offset_bytes, int64_t* n_elems) {
    if (!m.ok || name == nullptr) return VQA_ERR_ARG;
    const Layout L = m.layout();
    const auto* e = L.find(name);
    if (e == nullptr) return VQA_ERR_ARG;
    if (offset_bytes) *offset_bytes = e->off;
    if (n_elems) *n_elems = e->n;
    return VQA_OK;
}

// The variables (or their gradients) of a call, whichever public struct they came in: the trunk, up to two joint /
// classifier blocks (standard, adapt: [0] = joint_fc / classifier; noc: [0] = joint_v / classifier_v, [1] = joint_l /
// classifier_l) and v_adapt.  Members the model does not have stay NULL.
struct Params {
    bool present;      // the caller's pointer was non-NULL
    float *wordset_map, *l_glove, *enwiki_map;
    vqa_pt_fc6_t spat_v_linear_v, spat_q_linear_v, spat_att_score;
    GruCell gru, egru;
    vqa_pt_fc6_t pooled_linear_l, q_linear_l, wordset_ft, joint[2], classifier[2], v_adapt;
};

// the widening of a cfg-5 fc_layer scope from 4 to 6 LayerNorm slots (4 and 5 NULL: four heads never index them)
vqa_pt_fc6_t fc6(const vqa_pt_fc_t& f) {
    vqa_pt_fc6_t o{};
    o.w = f.w; o.b = f.b;
    for (int i = 0; i < 4; ++i) { o.beta[i] = f.beta[i]; o.gamma[i] = f.gamma[i]; }
    return o;
}
const vqa_pt_fc6_t& fc6(const vqa_pt_fc6_t& f) { return f; }

// the members every public params struct has under the same names
template <class T>
void view_trunk(const T& p, Params* v) {
    v->present = true;
    v->wordset_map = p.wordset_map; v->l_glove = p.l_glove;
    v->spat_v_linear_v = fc6(p.spat_v_linear_v); v->spat_q_linear_v = fc6(p.spat_q_linear_v);
    v->spat_att_score = fc6(p.spat_att_score);
    v->gru = {p.gru_wg, p.gru_bg, p.gru_wc, p.gru_bc};
    v->pooled_linear_l = fc6(p.pooled_linear_l); v->q_linear_l = fc6(p.q_linear_l); v->wordset_ft = fc6(p.wordset_ft);
}
template <class T>
void view_enwiki(const T& p, Params* v) {
    v->enwiki_map = p.enwiki_map;
    v->egru = {p.egru_wg, p.egru_bg, p.egru_wc, p.egru_bc};
}

Params view(const vqa_pretrain_params_t* p) {
    Params v{};
    if (p == nullptr) return v;
    view_trunk(*p, &v);
    v.joint[0] = fc6(p->joint_fc); v.classifier[0] = fc6(p->classifier);
    return v;
}
Params view(const vqa_pretrain_ext_params_t* p) {
    Params v{};
    if (p == nullptr) return v;
    view_trunk(*p, &v); view_enwiki(*p, &v);
    v.joint[0] = p->joint_fc; v.classifier[0] = p->classifier;
    return v;
}
Params view(const vqa_pretrain_noc_params_t* p) {
    Params v{};
    if (p == nullptr) return v;
    view_trunk(*p, &v); view_enwiki(*p, &v);
    v.joint[0] = p->joint_v; v.joint[1] = p->joint_l; v.classifier[0] = p->classifier_v; v.classifier[1] = p->classifier_l;
    return v;
}
Params view(const vqa_pretrain_adapt_params_t* p) {
    Params v = view(p ? &p->ext : nullptr);
    if (p != nullptr) v.v_adapt = p->v_adapt;
    return v;
}

// The batch of a call: the ext batch (cfg-5: no contexts) plus the l branch's masks of a noc batch (else NULL)
struct Batch {
    bool present;
    vqa_pretrain_ext_batch_t x;
    const vqa_pretrain_noc_kind_t* l;
};
Batch view(const vqa_pretrain_ext_batch_t* b) {
    Batch v{};
    if ((v.present = b != nullptr)) v.x = *b;
    return v;
}
Batch view(const vqa_pretrain_batch_t* b) {
    Batch v{};
    if ((v.present = b != nullptr)) v.x.base = *b;
    return v;
}
Batch view(const vqa_pretrain_noc_batch_t* b) {
    Batch v = view(b ? &b->base : nullptr);
    if (b != nullptr) v.l = b->l;
    return v;
}

// the memory the spatial attention pools: one [B,R,width] block per category; bf16: raw bf16 patterns behind the pointers
// (the features under VQA_FLAG_BF16_FEATURES; the adapted memory is an f32 activation in every mode)
struct PoolMem { const float* mem[2]; int64_t width; bool bf16; };

// the keep struct's offsets, or zeros without one
const vqa_pretrain_keep_t NO_SEEDED_SITES = {};
const vqa_pretrain_keep_t& keep_of(const Ctx& c) { return c.keep ? *c.keep : NO_SEEDED_SITES; }

// dropout of the attention score, category k: [B*n, R, H]
KeepSrc att_keep(const Ctx& c, const Batch& b, int k) {
    return c.site(VQA_PT_KEEP_SITE_ATT, b.x.base.kind[k].keep_att, keep_of(c).att_off[k], c.d.keep_att, c.d.H);
}

// joint_fc dropout (noc: the v branch's) of the head of type t, category k: [B*n, 2H]
KeepSrc joint_keep(const Ctx& c, const Batch& b, int k, int t) {
    const vqa_pretrain_keep_t& o = keep_of(c);
    const vqa_pretrain_kind_t& kb = b.x.base.kind[k];
    const int64_t N = 2 * (int64_t)c.d.H;
    if (t == 0) return c.site(VQA_PT_KEEP_SITE_BF_JOINT, kb.keep_bf_joint, o.bf_joint_off[k], c.d.keep_joint, N);
    if (t == 1) return c.site(VQA_PT_KEEP_SITE_WS_JOINT, kb.keep_ws_joint, o.ws_joint_off[k], c.d.keep_joint, N);
    return c.site(VQA_PT_KEEP_SITE_EW_JOINT, b.x.ctx[k].keep_ew_joint, o.ew_joint_off[k], c.d.keep_joint, N);
}

// dropout of the l joint branch of a noc head of type t, category k
KeepSrc noc_lmask(const Ctx& c, const Batch& b, int k, int t) {
    const vqa_pretrain_noc_kind_t& l = b.l[k];
    return c.site(VQA_PT_KEEP_SITE_L_JOINT, t == 0 ? l.keep_bf_l_joint : t == 1 ? l.keep_ws_l_joint : l.keep_ew_l_joint,
                  keep_of(c).l_joint_off[k][t], c.d.keep_joint, 2 * (int64_t)c.d.H);
}

// a seeded site must not also carry a mask; unknown site bits are refused
int keep_sites_ok(const vqa_pretrain_keep_t* ks, const Batch& b) {
    if (ks == nullptr) return VQA_OK;
    VQA_REQUIRE((ks->seeded & ~VQA_PT_KEEP_SITE_ALL) == 0, VQA_ERR_ARG);
    for (int k = 0; k < 2; ++k) {
        const vqa_pretrain_kind_t& kb = b.x.base.kind[k];
        VQA_REQUIRE(!(ks->seeded & VQA_PT_KEEP_SITE_ATT) || kb.keep_att == nullptr, VQA_ERR_ARG);
        VQA_REQUIRE(!(ks->seeded & VQA_PT_KEEP_SITE_BF_JOINT) || kb.keep_bf_joint == nullptr, VQA_ERR_ARG);
        VQA_REQUIRE(!(ks->seeded & VQA_PT_KEEP_SITE_WS_JOINT) || kb.keep_ws_joint == nullptr, VQA_ERR_ARG);
        VQA_REQUIRE(!(ks->seeded & VQA_PT_KEEP_SITE_EW_JOINT) || b.x.ctx[k].keep_ew_joint == nullptr, VQA_ERR_ARG);
        if (b.l != nullptr)
            VQA_REQUIRE(!(ks->seeded & VQA_PT_KEEP_SITE_L_JOINT) ||
                        (!b.l[k].keep_bf_l_joint && !b.l[k].keep_ws_l_joint && !b.l[k].keep_ew_l_joint), VQA_ERR_ARG);
    }
    return VQA_OK;
}

// what the trunk dereferences
int trunk_inputs_ok(const HeadSet& hs, const Params& P, const Batch& b) {
    const vqa_pretrain_batch_t* bt = &b.x.base;
    VQA_REQUIRE(bt->image_ft && bt->spatial_ft && bt->num_boxes, VQA_ERR_ARG);
    VQA_REQUIRE((bt->perm == nullptr) == (bt->inv == nullptr) && (bt->perm == nullptr) == (bt->live_rows == nullptr), VQA_ERR_ARG);
    VQA_REQUIRE((b.x.ctx_perm == nullptr) == (b.x.ctx_inv == nullptr) &&
                (b.x.ctx_perm == nullptr) == (b.x.ctx_live_rows == nullptr), VQA_ERR_ARG);
    for (const vqa_pretrain_kind_t& kb : bt->kind)
        VQA_REQUIRE(kb.normal_boxes && kb.fills && kb.blanks && kb.blanks_len && kb.num && (hs.rank[1] < 0 || kb.wordsets),
                    VQA_ERR_ARG);
    VQA_REQUIRE(P.wordset_map && P.l_glove && P.gru.wg && P.gru.bg && P.gru.wc && P.gru.bc, VQA_ERR_ARG);
    if (hs.rank[1] >= 0) VQA_REQUIRE(P.wordset_ft.w && P.wordset_ft.b, VQA_ERR_ARG);
    if (hs.rank[2] >= 0)
        VQA_REQUIRE(P.enwiki_map && P.egru.wg && P.egru.bg && P.egru.wc && P.egru.bc && b.x.ctx[0].context &&
                    b.x.ctx[0].context_len && b.x.ctx[1].context && b.x.ctx[1].context_len, VQA_ERR_ARG);
    return VQA_OK;
}

// The ONE prologue of every forward (G == NULL) and backward of every family.  The order of the checks is part of the
// ABI -- a call that fails several of them returns the first one's code -- and it is not the same for every call.  The
// differences found in the per-family prologues this one replaced, each kept as it was:
//   - forwards only: the workspace's 16-byte alignment (VQA_ERR_ALIGN), after the workspace size; the backwards run on
//     the workspace a forward accepted and do not look again
//   - forwards only: the trunk's inputs (trunk_inputs_ok), after the workspace checks; the backwards never had the check
//   - backwards only: the phase range, after the keep sites and before everything below
//   - noc forward only: the six head weights, after the trunk's inputs (no other architecture checks its head weights)
//   - adapt only: v_adapt's pointers (with the LayerNorm slots in use), BEFORE the layout and the workspace size.  The
//     forward checks the parameters' v_adapt, the backward the GRADIENTS' and not the parameters'
//   - cfg 5 is judged by dims_ok alone (Model::cfg5); its head set cannot be wrong
const int ALL_PHASES = 15;
int prologue(const Model& m, const Params& P, const Params* G, const Batch& b, const void* workspace,
             int64_t workspace_bytes, int phases, const vqa_pretrain_keep_t* keep, Layout* L) {
    const bool fwd = G == nullptr;
    VQA_REQUIRE(m.ok && P.present && (fwd || G->present) && b.present && workspace, VQA_ERR_ARG);
    TRY(keep_sites_ok(keep, b));
    if (!fwd) VQA_REQUIRE(phases > 0 && phases < 16, VQA_ERR_ARG);
    if (m.arch == ARCH_ADAPT) {
        const vqa_pt_fc6_t& va = fwd ? P.v_adapt : G->v_adapt;
        VQA_REQUIRE(va.w && va.b && va.gamma[0] && va.beta[0] && (m.ln_shared() || (va.gamma[1] && va.beta[1])), VQA_ERR_ARG);
    }
    *L = m.layout();
    VQA_REQUIRE(workspace_bytes >= L->total, VQA_ERR_WORKSPACE);
    if (!fwd) return VQA_OK;
    VQA_REQUIRE(vqa_aligned16(workspace), VQA_ERR_ALIGN);
    TRY(trunk_inputs_ok(HeadSet(m.dims.heads), P, b));
    if (m.arch == ARCH_NOC)
        VQA_REQUIRE(P.pooled_linear_l.w && P.q_linear_l.w && P.joint[0].w && P.joint[1].w && P.classifier[0].w &&
                    P.classifier[1].w, VQA_ERR_ARG);
    return VQA_OK;
}

// ---------------------------------------------------------------- the sequence encoder
// A token batch of BOTH categories as one batch of 2 Bn rows (object rows first), time-major: embedding -> GRU -> final
// states into two Bn-row head slices of "S/lft".  The embedding and the GRU are shared by the categories, so one
// recurrence over 5120 rows replaces two over 2560 (half the step launches, tiles that fill the chip).  Rows in length
// order when the host sorted them (perm / inv / live_rows: the recurrence runs on the live prefix).  Two users: the
// blank-fill captions (L_GloVe, encode_L_blank, "J/...") and the enwiki contexts (enwiki_map, encode_L_enwiki, "E/...").
struct Seq {
    // workspace names: in + {tok, "lens_s", "x_tm", "xp", "hs", "gru_r", "gru_u", "gru_c", "gru_rh"} hold the sorted
    // batch and the forward tape, scr + {"wx_cat", "bx_cat", "dwx_cat", "d_state_s", "dxp", "dx"} the packed x rows
    // and the backward scratch
    std::string in, tok, scr;
    const char *fwd_label, *bptt_label, *embed_label;      // probe scopes
    const int32_t *tokens[2], *len[2];                     // per category: tokens [Bn,T] zero padded, lengths [Bn]
    const int32_t *perm, *inv, *live_rows;
    float *table, *g_table;                                // embedding table [vocab,W] and its gradient
    int vocab;
    GruCell G;                                             // the gradients of the recurrence's variables
    int64_t T, head;                                       // padded length; "S/lft" / "d_lft" slices head, head + 1
    GruTape t;                                             // the encoder's buffers (gru_encoder.h) with the variables P
};
struct SeqSet { Seq s[2]; int n; };

// the token batches of the head set: the captions, then the contexts when the enwiki head is on (G NULL in the forward:
// the gradient members stay NULL)
SeqSet make_seqs(const Ctx& c, const vqa_pretrain_ext_dims_t& dims, const Params& P, const Params* G, const Batch& b, const HeadSet& hs) {
    const vqa_pretrain_ext_batch_t* bx = &b.x;
    const vqa_pretrain_batch_t& bt = bx->base;
    SeqSet q{};
    Seq& j = q.s[0];
    j.in = "J/"; j.tok = "blanks_s"; j.scr = "";
    j.fwd_label = "pt.caption_gru.fwd"; j.bptt_label = "pt.caption_gru.bwd"; j.embed_label = "pt.caption_embed.bwd";
    for (int k = 0; k < 2; ++k) { j.tokens[k] = bt.kind[k].blanks; j.len[k] = bt.kind[k].blanks_len; }
    j.perm = bt.perm; j.inv = bt.inv; j.live_rows = bt.live_rows;
    j.table = P.l_glove; j.vocab = dims.base.Vq; j.T = dims.base.L; j.head = 0;
    j.t = GruTape(c, j.in, j.scr, "", j.T, 2 * (int64_t)c.d.B * c.d.n, c.d.H, c.d.W, P.gru, c.st);
    if (G != nullptr) { j.g_table = G->l_glove; j.G = G->gru; }
    q.n = 1;
    if (hs.rank[2] < 0) return q;
    Seq& e = q.s[1];
    e.in = "E/"; e.tok = "ctx_s"; e.scr = "E/";
    e.fwd_label = "pt.enwiki_gru.fwd"; e.bptt_label = "pt.enwiki_gru.bwd"; e.embed_label = "pt.enwiki_embed.bwd";
    for (int k = 0; k < 2; ++k) { e.tokens[k] = bx->ctx[k].context; e.len[k] = bx->ctx[k].context_len; }
    e.perm = bx->ctx_perm; e.inv = bx->ctx_inv; e.live_rows = bx->ctx_live_rows;
    e.table = P.enwiki_map; e.vocab = dims.n_ctx; e.T = dims.Lc; e.head = 2 * hs.rank[2];
    e.t = GruTape(c, e.in, e.scr, "", e.T, 2 * (int64_t)c.d.B * c.d.n, c.d.H, c.d.W, P.egru, c.st);
    if (G != nullptr) { e.g_table = G->enwiki_map; e.G = G->egru; }
    q.n = 2;
    return q;
}

// pack_wx false: the caller has packed the x rows already (the caption batch: the step's first launch)
int seq_fwd(const Ctx& c, const Seq& s, bool pack_wx) {
    const int64_t H = c.d.H, W = c.d.W, Bn = (int64_t)c.d.B * c.d.n, B2 = 2 * Bn, T = s.T;
    ProbeScope ps(s.fwd_label, c.st);
    const GruTape& t = s.t;
    if (pack_wx) TRY(t.pack_wx());
    int32_t *tok = c.i32(s.in + s.tok), *lens = c.i32(s.in + "lens_s");
    TRY(gather_rows2(s.tokens[0], s.tokens[1], s.perm, tok, B2, T, Bn, c.st));
    TRY(gather_rows2(s.len[0], s.len[1], s.perm, lens, B2, 1, Bn, c.st));
    TRY(vqa_embed_fwd_ld(s.table, tok, t.x_tm, (int)B2, (int)T, (int)W, s.vocab, t.ldx(), c.st));
    TRY(c.enc_routed() ? t.project(c.routed()) : t.project(c.f32()));
    TRY(t.clear_h0());
    if (c.enc_routed()) {      // the bf16 form of the same two drivers, per call (gru_step.h)
        if (s.live_rows != nullptr)
            TRY(gru_seq_fwd_live_form(GRU_FORM_BF16, t.xp, t.Wg_h(), t.Wc_h(), lens, s.live_rows, t.hs, t.gru_r, t.gru_u, t.gru_c,
                                      t.gru_rh, (int)T, (int)B2, (int)H, c.st));
        else
            TRY(gru_seq_fwd_rows_form(GRU_FORM_BF16, t.xp, t.Wg_h(), t.Wc_h(), lens, t.hs, t.gru_r, t.gru_u, t.gru_c, t.gru_rh,
                                      (int)T, (int)B2, (int)H, 0, (int)B2, c.st));
    } else if (s.live_rows != nullptr)
        TRY(vqa_gru_seq_fwd_live(t.xp, t.Wg_h(), t.Wc_h(), lens, s.live_rows, t.hs, t.gru_r, t.gru_u, t.gru_c, t.gru_rh, (int)T,
                                 (int)B2, (int)H, c.st));
    else
        TRY(vqa_gru_seq_fwd(t.xp, t.Wg_h(), t.Wc_h(), lens, t.hs, t.gru_r, t.gru_u, t.gru_c, t.gru_rh, (int)T, (int)B2, (int)H,
                            c.st));
    return gather_rows(t.h_final(), s.inv, c.f("S/lft") + s.head * Bn * H, B2, H, c.st);      // back to the given order
}

// phase 2: back-propagation through time from the two "d_lft" slices, the GRU kernels' and biases' gradients (the x rows
// and biases unpacked after the two recurrent blocks)
int seq_bptt(const Ctx& c, Acc& acc, const Seq& s) {
    const int64_t H = c.d.H, Bn = (int64_t)c.d.B * c.d.n, B2 = 2 * Bn, T = s.T;
    ProbeScope ps(s.bptt_label, c.st);
    const GruTape& t = s.t;
    const int32_t* lens = c.i32(s.in + "lens_s");
    float* d_state = c.f(s.scr + "d_state_s");
    TRY(gather_rows(c.f("d_lft") + s.head * Bn * H, s.perm, d_state, B2, H, c.st));      // into the sorted order
    if (c.enc_routed()) {
        if (s.live_rows != nullptr)
            TRY(gru_seq_bwd_live_form(GRU_FORM_BF16, d_state, t.Wg_h(), t.Wc_h(), lens, s.live_rows, t.hs, t.gru_r, t.gru_u,
                                      t.gru_c, t.dxp, c.f("d_hscratch"), (int)T, (int)B2, (int)H, c.st));
        else
            TRY(gru_seq_bwd_rows_form(GRU_FORM_BF16, d_state, t.Wg_h(), t.Wc_h(), lens, t.hs, t.gru_r, t.gru_u, t.gru_c, t.dxp,
                                      c.f("d_hscratch"), (int)T, (int)B2, (int)H, 0, (int)B2, c.st));
    } else if (s.live_rows != nullptr)
        TRY(vqa_gru_seq_bwd_live(d_state, t.Wg_h(), t.Wc_h(), lens, s.live_rows, t.hs, t.gru_r, t.gru_u, t.gru_c, t.dxp,
                                 c.f("d_hscratch"), (int)T, (int)B2, (int)H, c.st));
    else
        TRY(vqa_gru_seq_bwd(d_state, t.Wg_h(), t.Wc_h(), lens, t.hs, t.gru_r, t.gru_u, t.gru_c, t.dxp, c.f("d_hscratch"), (int)T,
                            (int)B2, (int)H, c.st));
    const Prec prec = c.enc_routed() ? PREC_ROUTED : PREC_F32;
    TRY(t.dwx(acc.as_gemm(prec)));
    TRY(t.dwh(acc.as_gemm(prec), s.G, false, 0));
    TRY(t.dwh(acc.as_gemm(prec), s.G, true, 0));
    return t.unpack_dwx(s.G);
}

// running sum of squares of the un-aggregated embedding slices
struct SliceSq {
    const Ctx& c;
    const float* prev;
    int add(const float* g, int64_t cnt) {
        TRY(vqa_sumsq(g, cnt, prev, c.f("sq"), c.f("sumsq_ws"), c.count("sumsq_ws"), c.st));
        prev = c.f("sq");
        return VQA_OK;
    }
};

// phase 4: dx of the packed x-projection -> scatter-add into the (cleared) embedding gradient, slice sum of squares
int seq_embed_bwd(const Ctx& c, const Seq& s, SliceSq& sq) {
    const int64_t W = c.d.W, B2 = 2 * (int64_t)c.d.B * c.d.n, T = s.T;
    ProbeScope ps(s.embed_label, c.st);
    if (hipMemsetAsync(s.g_table, 0, (size_t)s.vocab * W * 4, c.st) != hipSuccess) return VQA_ERR_LAUNCH;
    float* dx = c.f(s.scr + "dx");
    const GruTape& t = s.t;
    // packed again here (one small kernel): no hidden dependence on the forward's copy of the weights
    TRY(t.pack_wx());
    TRY(c.enc_routed() ? t.dx(c.routed(), dx) : t.dx(c.f32(), dx));
    TRY(vqa_embed_bwd_len_det(dx, c.i32(s.in + s.tok), c.i32(s.in + "lens_s"), s.g_table, (int)B2, (int)T, (int)W, s.vocab,
                              (c.d.flags & VQA_FLAG_DETERMINISTIC) ? 1 : 0, c.st));
    return sq.add(dx, T * B2 * W);
}

// The trunk of every model of this file: spatial attention and pooling over the memory pm, word sets, the caption batch
// and the context batch, up to the stacked "S/pooled" and "S/lft" blocks the heads read
int trunk_fwd(const Ctx& c, const Model& m, const Params& P, const Batch& b, const HeadSet& hs, const PoolMem& pm) {
    const vqa_pretrain_dims_t* d = &m.dims.base;
    const vqa_pretrain_batch_t* bt = &b.x.base;
    const int64_t B = d->B, n = d->n, R = d->R, D = pm.width, H = d->H, W = d->W, Bn = B * n;
    const SeqSet q = make_seqs(c, m.dims, P, nullptr, b, hs);
    TRY(q.s[0].t.pack_wx());
    for (int k = 0; k < 2; ++k) {
        const vqa_pretrain_kind_t& kb = bt->kind[k];
        const std::string p = std::string(KIND[k]) + "/";
        // ---- build_*_V_ft: spatial attention over the regions
        ProbeScope ps_sp("pt.spatial_wordset.fwd", c.st);
        hipLaunchKernelGGL(box6_kernel, dim3((unsigned)((Bn + 255) / 256)), dim3(256), 0, c.st, kb.normal_boxes,
                           c.f(p + "key6"), (int)Bn);
        VQA_CHECK_LAUNCH();
        TRY(fc_ln_fwd(c, bt->spatial_ft, B * R, 6, H, P.spat_v_linear_v, c.li(k), (int)R, 0, p + "v_pre", p + "v",
                      p + "v_mean", p + "v_rstd", NO_KEEP));
        TRY(fc_ln_fwd(c, c.f(p + "key6"), Bn, 6, H, P.spat_q_linear_v, c.li(k), (int)n, 0, p + "qv_pre", p + "qv",
                      p + "qv_mean", p + "qv_rstd", NO_KEEP));
        TRY(vqa_attn_fwd_run(c.f(p + "v"), c.f(p + "qv"), pm.mem[k], pm.bf16, bt->num_boxes,
                             P.spat_att_score.w, P.spat_att_score.b, att_keep(c, b, k), c.f(p + "att"), c.f(p + "pooled"),
                             (int)B, (int)n, (int)R, (int)H, (int)D, c.st));
        hipLaunchKernelGGL(valid_kernel, dim3(1), dim3(256), 0, c.st, kb.num, c.f(p + "valid"), c.f(p + "inv_valid"),
                           (int)B, (int)n, d->global_valid[k]);
        VQA_CHECK_LAUNCH();
        if (hs.rank[1] >= 0) {      // ---- build_*_wordset
            TRY(vqa_embed_fwd(P.wordset_map, kb.wordsets, c.f(p + "wse"), (int)Bn, 1, (int)W, d->n_ws, c.st));
            TRY(vqa_tanh_fwd(c.f(p + "wse"), c.f(p + "ws"), Bn * W, c.st));
            TRY(fc_ln_fwd(c, c.f(p + "ws"), Bn, W, H, P.wordset_ft, c.li(k), (int)n, 1, p + "wf_pre", p + "wf", p + "wf_mean",
                          p + "wf_rstd", NO_KEEP));
        }
    }
    // ---- build_*_blank_fill -> heads 0 / 1 of "S/lft", build_*_enwiki -> heads 2 r_ew + k
    for (int i = 0; i < q.n; ++i) TRY(seq_fwd(c, q.s[i], i > 0));
    return VQA_OK;
}

// Phases 2, 4 and 8 of the backward (everything below the heads)
int trunk_bwd(const Ctx& c, Acc& acc, const Model& m, const Params& P, const Params& G, const Batch& b, const HeadSet& hs,
              float* slice_sq, int phases, const PoolMem& pm) {
    const vqa_pretrain_dims_t* d = &m.dims.base;
    const vqa_pretrain_batch_t* bt = &b.x.base;
    const int64_t B = d->B, n = d->n, R = d->R, D = pm.width, H = d->H, W = d->W, Bn = B * n;
    const int det = (d->flags & VQA_FLAG_DETERMINISTIC) ? 1 : 0;
    // the embedding tables are scatter-added: cleared in their phase; every other gradient is overwritten on first touch
    SliceSq sq{c, nullptr};
    const SeqSet q = make_seqs(c, m.dims, P, &G, b, hs);
    for (int i = 0; i < q.n && (phases & 2); ++i) TRY(seq_bptt(c, acc, q.s[i]));
    for (int i = 0; i < q.n && (phases & 4); ++i) TRY(seq_embed_bwd(c, q.s[i], sq));
    if (phases & 8) {
        if (hipMemsetAsync(G.wordset_map, 0, (size_t)d->n_ws * W * 4, c.st) != hipSuccess) return VQA_ERR_LAUNCH;
        if (!(phases & 4)) sq.prev = c.f("sq");      // phase 4 of this step left the sequences' slice sum of squares there
    }
    for (int k = 0; k < 2 && (phases & 8); ++k) {
        ProbeScope ps_sp("pt.spatial_wordset.bwd", c.st);
        const vqa_pretrain_kind_t& kb = bt->kind[k];
        const std::string p = std::string(KIND[k]) + "/";
        if (hs.rank[1] >= 0) {      // ---- word set -> wordset_ft -> tanh -> wordset_map
            TRY(fc_ln_bwd(c, acc, c.f("d_lft") + (2 * hs.rank[1] + k) * Bn * H, c.f(p + "ws"), Bn, W, H, P.wordset_ft,
                          G.wordset_ft, c.li(k), (int)n, 1, p + "wf_pre", p + "wf_mean", p + "wf_rstd", NO_KEEP, "d_wfpre",
                          c.f("d_ws")));
            TRY(vqa_tanh_bwd(c.f("d_ws"), c.f(p + "ws"), c.f("d_wse"), Bn * W, c.st));
            TRY(vqa_embed_bwd_len_det(c.f("d_wse"), kb.wordsets, nullptr, G.wordset_map, (int)Bn, 1, (int)W, d->n_ws, det,
                                      c.st));
            TRY(sq.add(c.f("d_wse"), Bn * W));
        }
        // ---- spatial attention
        TRY(vqa_attn_bwd_run(c.f("d_pooled") + k * Bn * D, c.f(p + "v"), c.f(p + "qv"), pm.mem[k], pm.bf16,
                             c.f(p + "att"), P.spat_att_score.w, att_keep(c, b, k), c.f("d_v"), c.f("d_qv"),
                             c.f("part_dw"), c.f("part_db"), (int)B, (int)n, (int)R, (int)H, (int)D, c.st));
        TRY(acc.colsum(c.f("part_dw"), Bn, H, (int)H, G.spat_att_score.w));
        TRY(acc.colsum(c.f("part_db"), Bn, 1, 1, G.spat_att_score.b));
        TRY(fc_ln_bwd(c, acc, c.f("d_v"), bt->spatial_ft, B * R, 6, H, P.spat_v_linear_v, G.spat_v_linear_v, c.li(k), (int)R,
                      0, p + "v_pre", p + "v_mean", p + "v_rstd", NO_KEEP, "d_vpre", nullptr));
        TRY(fc_ln_bwd(c, acc, c.f("d_qv"), c.f(p + "key6"), Bn, 6, H, P.spat_q_linear_v, G.spat_q_linear_v, c.li(k), (int)n,
                      0, p + "qv_pre", p + "qv_mean", p + "qv_rstd", NO_KEEP, "d_qvpre", nullptr));
    }
    if ((phases & 8) && slice_sq != nullptr && sq.prev != nullptr)
        if (hipMemcpyAsync(slice_sq, sq.prev, sizeof(float), hipMemcpyDeviceToDevice, c.st) != hipSuccess)
            return VQA_ERR_LAUNCH;
    return VQA_OK;
}

// pooled_linear_l over the 2 Bn pooled rows and q_linear_l over the NH Bn stacked language rows ("S/lft"), then each
// head's LayerNorm + ReLU of both into its slices of "S/vl" / "S/ll" (v_linear_l / l_linear_l of the reference)
// (D: the width of the pooled memory = K of pooled_linear_l)
int heads_in_fwd(const Ctx& c, const HeadSet& hs, const vqa_pt_fc6_t& pooled, const vqa_pt_fc6_t& qlin, int64_t D) {
    const vqa_pretrain_dims_t& d = c.d;
    const int64_t B = d.B, n = d.n, H = d.H, Bn = B * n, NH = hs.nh(), SH = Bn * H;
    TRY(c.gemm_routed(0, 0, 2 * Bn, H, D, c.f("S/pooled"), (int)D, pooled.w, (int)H, c.f("S/vl_pre"), (int)H, pooled.b));
    TRY(c.gemm_routed(0, 0, NH * Bn, H, H, c.f("S/lft"), (int)H, qlin.w, (int)H, c.f("S/ll_pre"), (int)H, qlin.b));
    for (int h = 0; h < NH; ++h) {
        const std::string q = hs.name(h);
        TRY(vqa_ln_act_fwd_run(c.f("S/vl_pre") + (h & 1) * SH, pooled.gamma[c.li(h)], pooled.beta[c.li(h)], NO_KEEP,
                               c.f("S/vl") + h * SH, c.f(q + "vl_mean"), c.f(q + "vl_rstd"), (int)B, (int)n, (int)H, 0, c.st));
        TRY(vqa_ln_act_fwd_run(c.f("S/ll_pre") + h * SH, qlin.gamma[c.li(h)], qlin.beta[c.li(h)], NO_KEEP, c.f("S/ll") + h * SH,
                               c.f(q + "ll_mean"), c.f(q + "ll_rstd"), (int)B, (int)n, (int)H, 0, c.st));
    }
    return VQA_OK;
}

// its backward from "d_vl" / "d_ll": LayerNorms, pooled_linear_l (dW, d_pooled) and q_linear_l (dW, d_lft)
int heads_in_bwd(const Ctx& c, Acc& acc, const HeadSet& hs, const vqa_pt_fc6_t& pooled, const vqa_pt_fc6_t& qlin,
                 const vqa_pt_fc6_t& g_pooled, const vqa_pt_fc6_t& g_qlin, int64_t D) {
    const vqa_pretrain_dims_t& d = c.d;
    const int64_t B = d.B, n = d.n, H = d.H, Bn = B * n, NH = hs.nh(), SH = Bn * H;
    for (int h = 0; h < NH; ++h) {
        const std::string q = hs.name(h);
        TRY(ln_bwd(c, acc, c.f("d_vl") + h * SH, Bn, H, pooled, g_pooled, c.li(h), (int)n, 0, c.f("S/vl_pre") + (h & 1) * SH,
                   c.f(q + "vl_mean"), c.f(q + "vl_rstd"), NO_KEEP, c.f("d_vlpre") + h * SH));
        TRY(ln_bwd(c, acc, c.f("d_ll") + h * SH, Bn, H, qlin, g_qlin, c.li(h), (int)n, 0, c.f("S/ll_pre") + h * SH,
                   c.f(q + "ll_mean"), c.f(q + "ll_rstd"), NO_KEEP, c.f("d_llpre") + h * SH));
    }
    // every head of a category applies pooled_linear_l to the same pooled rows: their d_pre meet before one dW / dx
    for (int r = 1; r < hs.nt; ++r) TRY(vqa_add_inplace(c.f("d_vlpre"), c.f("d_vlpre") + 2 * r * SH, 2 * SH, c.st));
    TRY(acc.weight(PREC_ROUTED, g_pooled.w, c.f("S/pooled"), (int)D, c.f("d_vlpre"), (int)H, D, H, 2 * Bn));
    TRY(c.gemm_routed(0, 1, 2 * Bn, D, H, c.f("d_vlpre"), (int)H, pooled.w, (int)H, c.f("d_pooled"), (int)D));
    return fc_bwd(c, acc, PREC_ROUTED, "d_llpre", c.f("S/lft"), NH * Bn, H, H, qlin, g_qlin, c.f("d_lft"));
}

// the v_adapt layer of the adapt architecture: image_ft [B R, D] -> FC -> LayerNorm over each image's [R,H] block + ReLU,
// one pre-activation, one output per LayerNorm slot in use ("attr/va" names "obj/va" when the slot is shared)
int v_adapt_fwd(const Ctx& c, const vqa_pretrain_batch_t* bt, const vqa_pt_fc6_t& va) {
    const vqa_pretrain_dims_t& d = c.d;
    const int64_t B = d.B, R = d.R, D = d.D, H = d.H;
    const bool ln_shared = (d.flags & VQA_FLAG_SHARED_LN) != 0;
    ProbeScope ps("pt.v_adapt.fwd", c.st);
    TRY(c.gemm_routed(0, 0, B * R, H, D, bt->image_ft, (int)D, va.w, (int)H, c.f("va_pre"), (int)H, va.b, nullptr, 0,
                      feat16(d)));
    for (int k = 0; k < (ln_shared ? 1 : 2); ++k) {
        const std::string p = std::string(KIND[k]) + "/";
        TRY(vqa_ln_act_fwd_run(c.f("va_pre"), va.gamma[k], va.beta[k], NO_KEEP, c.f(p + "va"), c.f(p + "va_mean"),
                               c.f(p + "va_rstd"), (int)B, (int)R, (int)H, 0, c.st));
    }
    return VQA_OK;
}

// its backward (phase 8, after the attention backward of both categories): d v_adapt from the attention weights and
// d pooled of the n queries -- shared LayerNorm: both categories pooled the same memory, one launch writes the sum --
// then the LayerNorm backward per slot, ONE dW over the sum of the call sites' d_pre, no dx (the features are an input)
int v_adapt_bwd(const Ctx& c, Acc& acc, const vqa_pretrain_batch_t* bt, const vqa_pt_fc6_t& va, const vqa_pt_fc6_t& g_va) {
    const vqa_pretrain_dims_t& d = c.d;
    const int64_t B = d.B, n = d.n, R = d.R, D = d.D, H = d.H, Bn = B * n;
    const bool ln_shared = (d.flags & VQA_FLAG_SHARED_LN) != 0;
    ProbeScope ps("pt.v_adapt.bwd", c.st);
    const float* dp[2] = {c.f("d_pooled"), c.f("d_pooled") + Bn * H};
    if (ln_shared) {
        TRY(vqa_outer_rows_rep(c.f("obj/att"), dp[0], c.f("attr/att"), dp[1], c.f("d_va"), (int)B, (int)n, (int)R, (int)H, c.st));
        TRY(ln_bwd(c, acc, c.f("d_va"), B * R, H, va, g_va, 0, (int)R, 0, c.f("va_pre"), c.f("va_mean"), c.f("va_rstd"),
                   NO_KEEP, c.f("d_vapre")));
    } else {
        for (int k = 0; k < 2; ++k) {
            const std::string p = std::string(KIND[k]) + "/";
            TRY(vqa_outer_rows_rep(c.f(p + "att"), dp[k], nullptr, nullptr, c.f("d_va"), (int)B, (int)n, (int)R, (int)H, c.st));
            TRY(ln_bwd(c, acc, c.f("d_va"), B * R, H, va, g_va, k, (int)R, 0, c.f("va_pre"), c.f(p + "va_mean"),
                       c.f(p + "va_rstd"), NO_KEEP, c.f(k == 0 ? "d_vapre" : "d_vapre1")));
        }
        TRY(vqa_add_inplace(c.f("d_vapre"), c.f("d_vapre1"), B * R * H, c.st));
    }
    return acc.weight(PREC_ROUTED, g_va.w, bt->image_ft, (int)D, c.f("d_vapre"), (int)H, D, H, B * R, feat16(d));
}

// the memory the model's attention pools: the features, or v_adapt per LayerNorm slot
PoolMem pool_mem(const Ctx& c, const Model& m, const Batch& b) {
    if (m.arch == ARCH_ADAPT) return {{c.f("obj/va"), c.f("attr/va")}, c.d.H, false};
    return {{b.x.base.image_ft, b.x.base.image_ft}, c.d.D, feat16(c.d)};
}

// ---------------------------------------------------------------- the head blocks
// What follows "S/vl" / "S/ll" (heads_in_fwd), per architecture: the logits and losses of the NH stacked heads, and the
// stats blocks the report reads, in key order.  The backward counterparts run from the dz blocks to "d_vl" / "d_ll".

// standard and adapt: joint_fc(v_linear_l * l_linear_l) -> classifier -> masked softmax-CE per head
int std_heads_fwd(const Ctx& c, const HeadSet& hs, const Params& P, const Batch& b, int want_dz, ReportExtArgs* ra) {
    const vqa_pretrain_dims_t& d = c.d;
    const int64_t B = d.B, n = d.n, H = d.H, A = d.A, Bn = B * n, NH = hs.nh(), SH = Bn * H, SJ = Bn * 2 * H, SA = Bn * A;
    const vqa_pt_fc6_t &joint = P.joint[0], &cls = P.classifier[0];
    TRY(vqa_mul(c.f("S/vl"), c.f("S/ll"), c.f("S/jin"), NH * SH, c.st));
    TRY(c.gemm_routed(0, 0, NH * Bn, 2 * H, H, c.f("S/jin"), (int)H, joint.w, (int)(2 * H), c.f("S/j_pre"), (int)(2 * H),
                      joint.b));
    for (int h = 0; h < NH; ++h) {
        const std::string q = hs.name(h);
        TRY(vqa_ln_act_fwd_run(c.f("S/j_pre") + h * SJ, joint.gamma[c.li(h)], joint.beta[c.li(h)],
                               joint_keep(c, b, h & 1, hs.type[h >> 1]), c.f("S/j") + h * SJ, c.f(q + "j_mean"),
                               c.f(q + "j_rstd"), (int)B, (int)n, (int)(2 * H), 0, c.st));
    }
    TRY(c.gemm_routed(0, 0, NH * Bn, A, 2 * H, c.f("S/j"), (int)(2 * H), cls.w, (int)A, c.f("S/z"), (int)A, cls.b));
    for (int h = 0; h < NH; ++h) {
        const int k = h & 1, r = h >> 1;
        const std::string p = std::string(KIND[k]) + "/";
        TRY(vqa_softmax_ce_fwd(c.f("S/z") + h * SA, b.x.base.kind[k].fills, c.f(p + "valid"), 5, c.f(p + "inv_valid"),
                               c.f("S/stats") + h * Bn * 4, want_dz ? c.f("S/dz") + h * SA : nullptr, (int)Bn, (int)A, c.st));
        ra->stats[k * hs.nt + r] = c.f("S/stats") + h * Bn * 4;
        ra->inv[k * hs.nt + r] = c.f(p + "inv_valid");
    }
    ra->nh = (int)NH;
    return VQA_OK;
}

int std_heads_bwd(const Ctx& c, Acc& acc, const HeadSet& hs, const Params& P, const Params& G, const Batch& b) {
    const vqa_pretrain_dims_t& d = c.d;
    const int64_t B = d.B, n = d.n, H = d.H, A = d.A, Bn = B * n, NH = hs.nh(), SH = Bn * H, SJ = Bn * 2 * H;
    const vqa_pt_fc6_t &joint = P.joint[0], &g_joint = G.joint[0];
    TRY(acc.weight(PREC_ROUTED, G.classifier[0].w, c.f("S/j"), (int)(2 * H), c.f("S/dz"), (int)A, 2 * H, A, NH * Bn));
    TRY(acc.colsum(c.f("S/dz"), NH * Bn, A, (int)A, G.classifier[0].b));
    TRY(c.gemm_routed(0, 1, NH * Bn, 2 * H, A, c.f("S/dz"), (int)A, P.classifier[0].w, (int)A, c.f("d_j"), (int)(2 * H)));
    for (int h = 0; h < NH; ++h) {
        const std::string q = hs.name(h);
        TRY(ln_bwd(c, acc, c.f("d_j") + h * SJ, Bn, 2 * H, joint, g_joint, c.li(h), (int)n, 0, c.f("S/j_pre") + h * SJ,
                   c.f(q + "j_mean"), c.f(q + "j_rstd"), joint_keep(c, b, h & 1, hs.type[h >> 1]), c.f("d_jpre") + h * SJ));
    }
    TRY(fc_bwd(c, acc, PREC_ROUTED, "d_jpre", c.f("S/jin"), NH * Bn, H, 2 * H, joint, g_joint, c.f("d_jin")));
    return vqa_mul_bwd(c.f("d_jin"), c.f("S/vl"), c.f("S/ll"), c.f("d_vl"), c.f("d_ll"), NH * SH, c.st);
}

// noc (vlmap_memft/model_vlmap_noc_bf_or_wordset_withatt_sp.py = model_vlmap_nocarch_bf_or_wordset_withatt_sp.py, bf | ws;
// model_vlmap_noc_bf_or_enwiki_withatt_sp.py, bf | ew): per head two branches instead of the product,
//   v_joint = dropout(relu(LN(v_linear_l joint_v)), 0.5) -> classifier_v,  l_joint = the same on l_linear_l -> classifier_l
// Blank fill is a SUM head (one CE of v_logit + l_logit), word set and enwiki are SPLIT heads (a CE per branch).  Both
// branches' joint and classifier GEMMs run over the whole stacked NH Bn block, forward and backward, whatever the
// head's loss; vqa_softmax_ce_pair_fwd writes every head's stats and dz in one launch.
int noc_heads_fwd(const Ctx& c, const HeadSet& hs, const Params& P, const Batch& b, int want_dz, ReportExtArgs* ra) {
    const vqa_pretrain_dims_t& d = c.d;
    const int64_t B = d.B, n = d.n, H = d.H, A = d.A, Bn = B * n, NH = hs.nh(), SJ = Bn * 2 * H, SA = Bn * A;
    TRY(c.gemm_routed(0, 0, NH * Bn, 2 * H, H, c.f("S/vl"), (int)H, P.joint[0].w, (int)(2 * H), c.f("S/jv_pre"), (int)(2 * H),
                      P.joint[0].b));
    TRY(c.gemm_routed(0, 0, NH * Bn, 2 * H, H, c.f("S/ll"), (int)H, P.joint[1].w, (int)(2 * H), c.f("S/jl_pre"), (int)(2 * H),
                      P.joint[1].b));
    for (int h = 0; h < NH; ++h) {
        const int k = h & 1, t = hs.type[h >> 1];
        const std::string q = hs.name(h);
        TRY(vqa_ln_act_fwd_run(c.f("S/jv_pre") + h * SJ, P.joint[0].gamma[c.li(h)], P.joint[0].beta[c.li(h)],
                               joint_keep(c, b, k, t), c.f("S/jv") + h * SJ, c.f(q + "jv_mean"), c.f(q + "jv_rstd"), (int)B,
                               (int)n, (int)(2 * H), 0, c.st));
        TRY(vqa_ln_act_fwd_run(c.f("S/jl_pre") + h * SJ, P.joint[1].gamma[c.li(h)], P.joint[1].beta[c.li(h)],
                               noc_lmask(c, b, k, t), c.f("S/jl") + h * SJ, c.f(q + "jl_mean"), c.f(q + "jl_rstd"), (int)B,
                               (int)n, (int)(2 * H), 0, c.st));
    }
    TRY(c.gemm_routed(0, 0, NH * Bn, A, 2 * H, c.f("S/jv"), (int)(2 * H), P.classifier[0].w, (int)A, c.f("S/zv"), (int)A,
                      P.classifier[0].b));
    TRY(c.gemm_routed(0, 0, NH * Bn, A, 2 * H, c.f("S/jl"), (int)(2 * H), P.classifier[1].w, (int)A, c.f("S/zl"), (int)A,
                      P.classifier[1].b));
    // every head's loss in one launch; the report reads the stats blocks in key order
    vqa_softmax_pair_t pr[VQA_SOFTMAX_PAIR_MAX] = {};
    const float* st_by_key[2][3][2] = {};
    for (int h = 0; h < NH; ++h) {
        const int k = h & 1, r = h >> 1;
        const std::string p = std::string(KIND[k]) + "/";
        vqa_softmax_pair_t& e = pr[h];
        e.zv = c.f("S/zv") + h * SA; e.zl = c.f("S/zl") + h * SA;
        e.label = b.x.base.kind[k].fills; e.valid = c.f(p + "valid"); e.inv_valid_sum = c.f(p + "inv_valid");
        e.split = noc_split(hs.type[r]) ? 1 : 0;
        e.stats_v = c.f("S/stats") + h * Bn * 4; e.stats_l = c.f("S/stats_l") + h * Bn * 4;
        e.dzv = want_dz ? c.f("S/dzv") + h * SA : nullptr; e.dzl = want_dz ? c.f("S/dzl") + h * SA : nullptr;
        st_by_key[k][r][0] = e.stats_v;
        st_by_key[k][r][1] = e.split ? e.stats_l : nullptr;
    }
    TRY(vqa_softmax_ce_pair_fwd(pr, (int)NH, 5, (int)Bn, (int)A, c.st));
    for (int k = 0; k < 2; ++k)
        for (int r = 0; r < hs.nt; ++r)
            for (int br = 0; br < 2; ++br)
                if (st_by_key[k][r][br] != nullptr) {
                    ra->stats[ra->nh] = st_by_key[k][r][br];
                    ra->inv[ra->nh++] = c.f(std::string(KIND[k]) + "/inv_valid");
                }
    return VQA_OK;
}

// per branch: classifier dW / db / dx, each head's joint LayerNorm, the joint dW / db and dx into d_vl / d_ll
int noc_heads_bwd(const Ctx& c, Acc& acc, const HeadSet& hs, const Params& P, const Params& G, const Batch& b) {
    const vqa_pretrain_dims_t& d = c.d;
    const int64_t n = d.n, H = d.H, A = d.A, Bn = (int64_t)d.B * n, NH = hs.nh(), SJ = Bn * 2 * H;
    struct Branch { const char *j, *dz, *dj, *jpre, *djpre, *in, *din, *tag; };
    const Branch br[2] = {{"S/jv", "S/dzv", "d_jv", "S/jv_pre", "d_jvpre", "S/vl", "d_vl", "jv"},
                          {"S/jl", "S/dzl", "d_jl", "S/jl_pre", "d_jlpre", "S/ll", "d_ll", "jl"}};
    for (int v = 0; v < 2; ++v) {
        const Branch& x = br[v];
        TRY(acc.weight(PREC_ROUTED, G.classifier[v].w, c.f(x.j), (int)(2 * H), c.f(x.dz), (int)A, 2 * H, A, NH * Bn));
        TRY(acc.colsum(c.f(x.dz), NH * Bn, A, (int)A, G.classifier[v].b));
        TRY(c.gemm_routed(0, 1, NH * Bn, 2 * H, A, c.f(x.dz), (int)A, P.classifier[v].w, (int)A, c.f(x.dj), (int)(2 * H)));
        for (int h = 0; h < NH; ++h) {
            const int k = h & 1, t = hs.type[h >> 1];
            const std::string q = hs.name(h) + x.tag;
            TRY(ln_bwd(c, acc, c.f(x.dj) + h * SJ, Bn, 2 * H, P.joint[v], G.joint[v], c.li(h), (int)n, 0, c.f(x.jpre) + h * SJ,
                       c.f(q + "_mean"), c.f(q + "_rstd"), v == 0 ? joint_keep(c, b, k, t) : noc_lmask(c, b, k, t),
                       c.f(x.djpre) + h * SJ));
        }
        TRY(fc_bwd(c, acc, PREC_ROUTED, x.djpre, c.f(x.in), NH * Bn, H, 2 * H, P.joint[v], G.joint[v], c.f(x.din)));
    }
    return VQA_OK;
}

// ---------------------------------------------------------------- the forward and the backward of every model
int forward(const Model& m, const Params& P, const Batch& b, void* workspace, int64_t workspace_bytes, int want_dz,
            void* stream, const vqa_pretrain_keep_t* keep) {
    Layout L;
    TRY(prologue(m, P, nullptr, b, workspace, workspace_bytes, ALL_PHASES, keep, &L));      // a forward has no phases
    const HeadSet hs(m.dims.heads);
    const Ctx c{{L, static_cast<char*>(workspace)}, m.dims.base, static_cast<hipStream_t>(stream), keep};
    ReportExtArgs ra{};
    ra.rows = c.d.B * c.d.n;
    ProbeScope ps_all(m.fwd_label(), c.st);
    if (m.arch == ARCH_ADAPT) TRY(v_adapt_fwd(c, &b.x.base, P.v_adapt));
    const PoolMem pm = pool_mem(c, m, b);
    TRY(trunk_fwd(c, m, P, b, hs, pm));
    {   // the NH heads, stacked
        ProbeScope ps_h("pt.heads.fwd", c.st);
        TRY(heads_in_fwd(c, hs, P.pooled_linear_l, P.q_linear_l, pm.width));
        TRY((m.arch == ARCH_NOC ? noc_heads_fwd : std_heads_fwd)(c, hs, P, b, want_dz, &ra));
    }
    hipLaunchKernelGGL(pretrain_ext_report_kernel, dim3(1), dim3(256), 0, c.st, ra, c.f("report"));
    VQA_CHECK_LAUNCH();
    return VQA_OK;
}

// The backward in dependency-ordered phases (bit mask, ascending within a step):
//   1  the NH stacked heads: the architecture's head block, then pooled_linear_l and q_linear_l
//   2  BPTT of the caption batch, then of the enwiki context batch (encode_L_blank and encode_L_enwiki gradients)
//   4  L_GloVe scatter-add, then enwiki_map scatter-add (both slice sums of squares)
//   8  per category: wordset_ft / wordset_map (cleared even without the word-set head), spatial attention (writes
//      slice_sq); adapt: then the v_adapt gradients, which need the attention backward of both categories
int backward(const Model& m, const Params& P, const Params& G, const Batch& b, void* workspace, int64_t workspace_bytes,
             float* slice_sq, int phases, void* stream, const vqa_pretrain_keep_t* keep) {
    Layout L;
    TRY(prologue(m, P, &G, b, workspace, workspace_bytes, phases, keep, &L));
    const HeadSet hs(m.dims.heads);
    const Ctx c{{L, static_cast<char*>(workspace)}, m.dims.base, static_cast<hipStream_t>(stream), keep};
    ProbeScope ps_all(m.bwd_label(), c.st);
    Acc acc{c, {}};
    const PoolMem pm = pool_mem(c, m, b);
    if (phases & 1) {
        ProbeScope ps_h("pt.heads.bwd", c.st);
        TRY((m.arch == ARCH_NOC ? noc_heads_bwd : std_heads_bwd)(c, acc, hs, P, G, b));
        TRY(heads_in_bwd(c, acc, hs, P.pooled_linear_l, P.q_linear_l, G.pooled_linear_l, G.q_linear_l, pm.width));
    }
    TRY(trunk_bwd(c, acc, m, P, G, b, hs, slice_sq, phases, pm));
    return (m.arch == ARCH_ADAPT && (phases & 8)) ? v_adapt_bwd(c, acc, &b.x.base, P.v_adapt, G.v_adapt) : VQA_OK;
}

}  // namespace

// ================================================================ the entry points
// Every family: an adapter from its public structs to (Model, Params, Batch), then the one function above.  The calls
// without _ex are the _ex calls with keep = NULL, *_backward is *_backward_phases with phases = 15.

// ---- vqa_pretrain_*: cfg 5 = heads bf | ws on the standard architecture, structs with 4 LayerNorm slots and no contexts
extern "C" const char* vqa_pretrain_report_key(int i) {
    return report_key(ARCH_STANDARD, VQA_PT_HEAD_BF | VQA_PT_HEAD_WS, i);
}

extern "C" int64_t vqa_pretrain_workspace_bytes(const vqa_pretrain_dims_t* dims) { return layout_bytes(Model::cfg5(dims)); }

extern "C" int vqa_pretrain_tensor(const vqa_pretrain_dims_t* dims, const char* name, int64_t* offset_bytes,
                                   int64_t* n_elems) {
    return layout_tensor(Model::cfg5(dims), name, offset_bytes, n_elems);
}

extern "C" int vqa_pretrain_forward_ex(const vqa_pretrain_dims_t* dims, const vqa_pretrain_params_t* P,
                                       const vqa_pretrain_batch_t* bt, void* workspace, int64_t workspace_bytes,
                                       int want_dz, void* stream, const vqa_pretrain_keep_t* keep) {
    return forward(Model::cfg5(dims), view(P), view(bt), workspace, workspace_bytes, want_dz, stream, keep);
}

extern "C" int vqa_pretrain_forward(const vqa_pretrain_dims_t* dims, const vqa_pretrain_params_t* P,
                                    const vqa_pretrain_batch_t* bt, void* workspace, int64_t workspace_bytes,
                                    int want_dz, void* stream) {
    return vqa_pretrain_forward_ex(dims, P, bt, workspace, workspace_bytes, want_dz, stream, nullptr);
}

extern "C" int vqa_pretrain_backward_phases_ex(const vqa_pretrain_dims_t* dims, const vqa_pretrain_params_t* P,
                                               const vqa_pretrain_params_t* G, const vqa_pretrain_batch_t* bt,
                                               void* workspace, int64_t workspace_bytes, float* slice_sq, int phases,
                                               void* stream, const vqa_pretrain_keep_t* keep) {
    return backward(Model::cfg5(dims), view(P), view(G), view(bt), workspace, workspace_bytes, slice_sq, phases, stream, keep);
}

extern "C" int vqa_pretrain_backward_phases(const vqa_pretrain_dims_t* dims, const vqa_pretrain_params_t* P,
                                            const vqa_pretrain_params_t* G, const vqa_pretrain_batch_t* bt,
                                            void* workspace, int64_t workspace_bytes, float* slice_sq, int phases,
                                            void* stream) {
    return vqa_pretrain_backward_phases_ex(dims, P, G, bt, workspace, workspace_bytes, slice_sq, phases, stream, nullptr);
}

extern "C" int vqa_pretrain_backward(const vqa_pretrain_dims_t* dims, const vqa_pretrain_params_t* P,
                                     const vqa_pretrain_params_t* G, const vqa_pretrain_batch_t* bt, void* workspace,
                                     int64_t workspace_bytes, float* slice_sq, void* stream) {
    return vqa_pretrain_backward_phases(dims, P, G, bt, workspace, workspace_bytes, slice_sq, 15, stream);
}

// ---- vqa_pretrain_ext_*: the variable head set on the standard architecture
extern "C" const char* vqa_pretrain_ext_report_key(int heads, int i) { return report_key(ARCH_STANDARD, heads, i); }

extern "C" int64_t vqa_pretrain_ext_workspace_bytes(const vqa_pretrain_ext_dims_t* dims) {
    return layout_bytes(Model::of(dims, ARCH_STANDARD));
}

extern "C" int vqa_pretrain_ext_tensor(const vqa_pretrain_ext_dims_t* dims, const char* name, int64_t* offset_bytes,
                                       int64_t* n_elems) {
    return layout_tensor(Model::of(dims, ARCH_STANDARD), name, offset_bytes, n_elems);
}

extern "C" int vqa_pretrain_ext_forward_ex(const vqa_pretrain_ext_dims_t* dims, const vqa_pretrain_ext_params_t* P,
                                           const vqa_pretrain_ext_batch_t* bx, void* workspace, int64_t workspace_bytes,
                                           int want_dz, void* stream, const vqa_pretrain_keep_t* keep) {
    return forward(Model::of(dims, ARCH_STANDARD), view(P), view(bx), workspace, workspace_bytes, want_dz, stream, keep);
}

extern "C" int vqa_pretrain_ext_forward(const vqa_pretrain_ext_dims_t* dims, const vqa_pretrain_ext_params_t* P,
                                        const vqa_pretrain_ext_batch_t* bx, void* workspace, int64_t workspace_bytes,
                                        int want_dz, void* stream) {
    return vqa_pretrain_ext_forward_ex(dims, P, bx, workspace, workspace_bytes, want_dz, stream, nullptr);
}

extern "C" int vqa_pretrain_ext_backward_phases_ex(const vqa_pretrain_ext_dims_t* dims, const vqa_pretrain_ext_params_t* P,
                                                   const vqa_pretrain_ext_params_t* G, const vqa_pretrain_ext_batch_t* bx,
                                                   void* workspace, int64_t workspace_bytes, float* slice_sq, int phases,
                                                   void* stream, const vqa_pretrain_keep_t* keep) {
    return backward(Model::of(dims, ARCH_STANDARD), view(P), view(G), view(bx), workspace, workspace_bytes, slice_sq, phases,
                    stream, keep);
}

extern "C" int vqa_pretrain_ext_backward_phases(const vqa_pretrain_ext_dims_t* dims, const vqa_pretrain_ext_params_t* P,
                                                const vqa_pretrain_ext_params_t* G, const vqa_pretrain_ext_batch_t* bx,
                                                void* workspace, int64_t workspace_bytes, float* slice_sq, int phases,
                                                void* stream) {
    return vqa_pretrain_ext_backward_phases_ex(dims, P, G, bx, workspace, workspace_bytes, slice_sq, phases, stream, nullptr);
}

extern "C" int vqa_pretrain_ext_backward(const vqa_pretrain_ext_dims_t* dims, const vqa_pretrain_ext_params_t* P,
                                         const vqa_pretrain_ext_params_t* G, const vqa_pretrain_ext_batch_t* bx,
                                         void* workspace, int64_t workspace_bytes, float* slice_sq, void* stream) {
    return vqa_pretrain_ext_backward_phases(dims, P, G, bx, workspace, workspace_bytes, slice_sq, 15, stream);
}

// ---- vqa_pretrain_noc_*: the "no composition" architecture, heads bf | ws or bf | ew
extern "C" const char* vqa_pretrain_noc_report_key(int heads, int i) { return report_key(ARCH_NOC, heads, i); }

extern "C" int64_t vqa_pretrain_noc_workspace_bytes(const vqa_pretrain_ext_dims_t* dims) {
    return layout_bytes(Model::of(dims, ARCH_NOC));
}

extern "C" int vqa_pretrain_noc_tensor(const vqa_pretrain_ext_dims_t* dims, const char* name, int64_t* offset_bytes,
                                       int64_t* n_elems) {
    return layout_tensor(Model::of(dims, ARCH_NOC), name, offset_bytes, n_elems);
}

extern "C" int vqa_pretrain_noc_forward_ex(const vqa_pretrain_ext_dims_t* dims, const vqa_pretrain_noc_params_t* P,
                                           const vqa_pretrain_noc_batch_t* bn, void* workspace, int64_t workspace_bytes,
                                           int want_dz, void* stream, const vqa_pretrain_keep_t* keep) {
    return forward(Model::of(dims, ARCH_NOC), view(P), view(bn), workspace, workspace_bytes, want_dz, stream, keep);
}

extern "C" int vqa_pretrain_noc_forward(const vqa_pretrain_ext_dims_t* dims, const vqa_pretrain_noc_params_t* P,
                                        const vqa_pretrain_noc_batch_t* bn, void* workspace, int64_t workspace_bytes,
                                        int want_dz, void* stream) {
    return vqa_pretrain_noc_forward_ex(dims, P, bn, workspace, workspace_bytes, want_dz, stream, nullptr);
}

extern "C" int vqa_pretrain_noc_backward_phases_ex(const vqa_pretrain_ext_dims_t* dims, const vqa_pretrain_noc_params_t* P,
                                                   const vqa_pretrain_noc_params_t* G, const vqa_pretrain_noc_batch_t* bn,
                                                   void* workspace, int64_t workspace_bytes, float* slice_sq, int phases,
                                                   void* stream, const vqa_pretrain_keep_t* keep) {
    return backward(Model::of(dims, ARCH_NOC), view(P), view(G), view(bn), workspace, workspace_bytes, slice_sq, phases,
                    stream, keep);
}

extern "C" int vqa_pretrain_noc_backward_phases(const vqa_pretrain_ext_dims_t* dims, const vqa_pretrain_noc_params_t* P,
                                                const vqa_pretrain_noc_params_t* G, const vqa_pretrain_noc_batch_t* bn,
                                                void* workspace, int64_t workspace_bytes, float* slice_sq, int phases,
                                                void* stream) {
    return vqa_pretrain_noc_backward_phases_ex(dims, P, G, bn, workspace, workspace_bytes, slice_sq, phases, stream, nullptr);
}

extern "C" int vqa_pretrain_noc_backward(const vqa_pretrain_ext_dims_t* dims, const vqa_pretrain_noc_params_t* P,
                                         const vqa_pretrain_noc_params_t* G, const vqa_pretrain_noc_batch_t* bn,
                                         void* workspace, int64_t workspace_bytes, float* slice_sq, void* stream) {
    return vqa_pretrain_noc_backward_phases(dims, P, G, bn, workspace, workspace_bytes, slice_sq, 15, stream);
}

// ---- vqa_pretrain_adapt_*: vlmap_memft/model_vlmap_bf_or_wordset_withatt_sp_adapt.py (bf | ws), the v_adapt layer (:346-350,
// :442-446) between the features and the attention pooling (:365-367, :461-463)
extern "C" const char* vqa_pretrain_adapt_report_key(int heads, int i) { return report_key(ARCH_ADAPT, heads, i); }

extern "C" int64_t vqa_pretrain_adapt_workspace_bytes(const vqa_pretrain_ext_dims_t* dims) {
    return layout_bytes(Model::of(dims, ARCH_ADAPT));
}

extern "C" int vqa_pretrain_adapt_tensor(const vqa_pretrain_ext_dims_t* dims, const char* name, int64_t* offset_bytes,
                                         int64_t* n_elems) {
    return layout_tensor(Model::of(dims, ARCH_ADAPT), name, offset_bytes, n_elems);
}

extern "C" int vqa_pretrain_adapt_forward_ex(const vqa_pretrain_ext_dims_t* dims, const vqa_pretrain_adapt_params_t* P,
                                             const vqa_pretrain_ext_batch_t* bx, void* workspace, int64_t workspace_bytes,
                                             int want_dz, void* stream, const vqa_pretrain_keep_t* keep) {
    return forward(Model::of(dims, ARCH_ADAPT), view(P), view(bx), workspace, workspace_bytes, want_dz, stream, keep);
}

extern "C" int vqa_pretrain_adapt_forward(const vqa_pretrain_ext_dims_t* dims, const vqa_pretrain_adapt_params_t* P,
                                          const vqa_pretrain_ext_batch_t* bx, void* workspace, int64_t workspace_bytes,
                                          int want_dz, void* stream) {
    return vqa_pretrain_adapt_forward_ex(dims, P, bx, workspace, workspace_bytes, want_dz, stream, nullptr);
}

extern "C" int vqa_pretrain_adapt_backward_phases_ex(const vqa_pretrain_ext_dims_t* dims, const vqa_pretrain_adapt_params_t* P,
                                                     const vqa_pretrain_adapt_params_t* G, const vqa_pretrain_ext_batch_t* bx,
                                                     void* workspace, int64_t workspace_bytes, float* slice_sq, int phases,
                                                     void* stream, const vqa_pretrain_keep_t* keep) {
    return backward(Model::of(dims, ARCH_ADAPT), view(P), view(G), view(bx), workspace, workspace_bytes, slice_sq, phases,
                    stream, keep);
}

extern "C" int vqa_pretrain_adapt_backward_phases(const vqa_pretrain_ext_dims_t* dims, const vqa_pretrain_adapt_params_t* P,
                                                  const vqa_pretrain_adapt_params_t* G, const vqa_pretrain_ext_batch_t* bx,
                                                  void* workspace, int64_t workspace_bytes, float* slice_sq, int phases,
                                                  void* stream) {
    return vqa_pretrain_adapt_backward_phases_ex(dims, P, G, bx, workspace, workspace_bytes, slice_sq, phases, stream, nullptr);
}

extern "C" int vqa_pretrain_adapt_backward(const vqa_pretrain_ext_dims_t* dims, const vqa_pretrain_adapt_params_t* P,
                                           const vqa_pretrain_adapt_params_t* G, const vqa_pretrain_ext_batch_t* bx,
                                           void* workspace, int64_t workspace_bytes, float* slice_sq, void* stream) {
    return vqa_pretrain_adapt_backward_phases(dims, P, G, bx, workspace, workspace_bytes, slice_sq, 15, stream);
}
