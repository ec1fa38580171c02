// Convolutions of the extractor's opt-in bf16 mode: bf16 NHWC activations and bf16 filters in HBM,
// f32 accumulation, one rounding on store.
//
//   y = [relu]( conv(x, w) * scale[co] + shift[co] + residual )
//
// x [B,Hi,Wi,Ci] bf16, w [Co][kh*kw*Ci] bf16 (k contiguous: packed once on the host from the HWIO filter), residual
// [B,Ho,Wo,Co] bf16, y bf16 (rounded to nearest even, once) or f32 (unrounded: the trunk's last layer).  An implicit GEMM:
// row m = output pixel, k = (ky, kx, ci).  Ci % 32 == 0, so a 32-deep k tile lies inside one filter tap and is 64
// contiguous bytes of one input pixel (zeros when the tap falls outside the image) and 64 contiguous bytes of one filter
// row: both operands travel global -> registers -> LDS as 16-byte pieces, with no conversion and no transposition.  1x1
// layers are the same kernel with one tap.
//
// Tile BM x BN (128 x 128, 128 x 64, 64 x 64), BK 32, 256 threads = 2 x 2 waves of (BM/2) x (BN/2), products on
// v_mfma_f32_32x32x16_bf16 with the fragment and C layouts of gemm_bf16.hip.  LDS rows are 80 bytes (32 k + 8 pad:
// conflict-free ds_read_b128 fragment reads), two buffers: while the matrix pipe works through k tile t the waves store
// tile t + 1 (already in registers) into the other buffer and fetch tile t + 2; one barrier per k tile.  Epilogue: scale and
// shift on the f32 accumulator, then each 32 x 32 tile goes through a wave-private LDS patch so that a lane owns 8
// consecutive channels of one pixel: 16-byte residual load, add and ReLU in f32, 16-byte store(s).
//
// Any M: rows beyond M are loaded as zeros and not stored; columns beyond Co likewise (Co % 8 == 0, so a lane's 8 channels
// are inside or outside together).
//
// vqa_maxpool3x3s2_same_nhwc_bf16 (f32 in, bf16 out: rounding is monotone, so this is the rounded f32 max-pool bit for bit)
// and vqa_subsample_nhwc_bf16 are the row kernels of conv_ops.hip on 8-channel pieces.
#include <algorithm>

#include "vqa_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 32, NT = 256;
constexpr int RS = 40;                       // bf16 per LDS row: 32 k + 8 pad = 80 bytes
constexpr int EP_LD = 36;                    // floats per row of the epilogue patch (32 + 4 pad, rows stay 16-byte aligned)
constexpr int EP_WAVE = 32 * EP_LD;          // floats per wave

int g_conv_bf16_cfg = -1;                    // vqa_conv_bf16_set_config; -1 = by shape

struct ConvArgs {
    const __bf16* x;
    const __bf16* w;
    const float* scale;
    const float* shift;
    const __bf16* residual;
    void* y;
    int M, Co, K;
    int Hi, Wi, Ci, Ho, Wo, kw, stride, pad_t, pad_l;
    int cpt;                                 // k tiles per filter tap = Ci / 32
    int nk;                                  // k tiles = kh * kw * cpt
    int tiles_n;
    int relu, y_is_f32;
};

template <int BM, int BN>
__global__ __launch_bounds__(NT, 2) void conv_bf16_kernel(const ConvArgs a) {
    constexpr int TM = BM / 64, TN = BN / 64;            // 32 x 32 MFMA tiles per wave
    constexpr int PA = BM * 4 / NT, PB = BN * 4 / NT;    // 16-byte pieces per thread and k tile
    constexpr int OPER_A = BM * RS, BUF = (BM + BN) * RS;
    constexpr int LDS_ELEMS = 2 * BUF > 4 * EP_WAVE * 2 ? 2 * BUF : 4 * EP_WAVE * 2;
    __shared__ __attribute__((aligned(16))) __bf16 lds[LDS_ELEMS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * (BM / 2), wn = (wave & 1) * (BN / 2);
    const int fr = lane & 31, fk = (lane >> 5) * 8;
    const int tile = blockIdx.x;
    const int m0 = (tile / a.tiles_n) * BM, n0 = (tile % a.tiles_n) * BN;

    // the rows this thread stages: output pixel -> (image, top-left input pixel of its window)
    int64_t a_img[PA];
    int a_iy0[PA], a_ix0[PA];
    bool a_ok[PA];
    const int pc = tid & 3;                              // which 16 bytes of the 64-byte row
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int m = m0 + (tid >> 2) + i * (NT / 4);
        a_ok[i] = m < a.M;
        const int mm = a_ok[i] ? m : 0;
        const int ox = mm % a.Wo, t = mm / a.Wo;
        const int oy = t % a.Ho, b = t / a.Ho;
        a_img[i] = (int64_t)b * a.Hi * a.Wi;
        a_iy0[i] = oy * a.stride - a.pad_t;
        a_ix0[i] = ox * a.stride - a.pad_l;
    }
    int64_t b_off[PB];
    bool b_ok[PB];
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        const int n = n0 + (tid >> 2) + i * (NT / 4);
        b_ok[i] = n < a.Co;
        b_off[i] = (int64_t)(b_ok[i] ? n : 0) * a.K + pc * 8;
    }

    i32x4 ra[PA], rb[PB];
    int f_ky = 0, f_kx = 0, f_c = 0, f_t = 0;            // the k tile the next fetch reads: tap (ky, kx), channel tile c
    auto fetch = [&]() {
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const int iy = a_iy0[i] + f_ky, ix = a_ix0[i] + f_kx;
            const bool ok = a_ok[i] && (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi;
            i32x4 v = {0, 0, 0, 0};
            if (ok) v = *reinterpret_cast<const i32x4*>(a.x + (a_img[i] + (int64_t)iy * a.Wi + ix) * a.Ci + f_c * BK + pc * 8);
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            i32x4 v = {0, 0, 0, 0};
            if (b_ok[i]) v = *reinterpret_cast<const i32x4*>(a.w + b_off[i] + (int64_t)f_t * BK);
            rb[i] = v;
        }
        ++f_t;
        if (++f_c == a.cpt) {
            f_c = 0;
            if (++f_kx == a.kw) { f_kx = 0; ++f_ky; }
        }
    };
    auto stage = [&](int buf) {
        __bf16* sA = lds + buf * BUF;
        __bf16* sB = sA + OPER_A;
#pragma unroll
        for (int i = 0; i < PA; ++i)
            *reinterpret_cast<i32x4*>(sA + ((tid >> 2) + i * (NT / 4)) * RS + pc * 8) = ra[i];
#pragma unroll
        for (int i = 0; i < PB; ++i)
            *reinterpret_cast<i32x4*>(sB + ((tid >> 2) + i * (NT / 4)) * RS + pc * 8) = rb[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    bf16x8 fa[2][TM], fb[2][TN];                          // [k step][tile]
    auto read_frags = [&](int t) {
        const __bf16* cA = lds + (t & 1) * BUF;
        const __bf16* cB = cA + OPER_A;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
                fa[ks][i] = *reinterpret_cast<const bf16x8*>(cA + (wm + i * 32 + fr) * RS + ks * 16 + fk);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                fb[ks][j] = *reinterpret_cast<const bf16x8*>(cB + (wn + j * 32 + fr) * RS + ks * 16 + fk);
        }
    };
    auto mfmas = [&]() {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][i], fb[ks][j], acc[i][j], 0, 0, 0);
    };

    const int nk = a.nk;
    fetch();
    stage(0);
    if (nk > 1) fetch();                                  // tile 1 waits in the registers
    __syncthreads();
    int t = 0;
    for (; t + 1 < nk; ++t) {
        read_frags(t);
        stage((t + 1) & 1);                               // tile t + 1 into the other buffer
        mfmas();
        if (t + 2 < nk) fetch();                          // its latency hides behind the next tile's MFMAs
        __syncthreads();                                  // tile t + 1 is in LDS; tile t's buffer is free
    }
    read_frags(t);
    mfmas();
    __syncthreads();                                      // every wave is done with the operand buffers

    // C / D map of a 32 x 32 tile: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float* ep = reinterpret_cast<float*>(lds) + wave * EP_WAVE;
    const int64_t Co = a.Co;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = n0 + wn + j * 32 + (lane & 31);
            const bool cok = col < a.Co;
            const float sc = (cok && a.scale != nullptr) ? a.scale[col] : 1.f;
            const float sh = (cok && a.shift != nullptr) ? a.shift[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rl = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                ep[rl * EP_LD + (lane & 31)] = acc[i][j][r] * sc + sh;
            }
            __syncthreads();
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                const int rl = pass * 16 + (lane >> 2), cg = (lane & 3) * 8;
                const int row = m0 + wm + i * 32 + rl, c0 = n0 + wn + j * 32 + cg;
                if (row < a.M && c0 < a.Co) {
                    const f32x4v lo = *reinterpret_cast<const f32x4v*>(ep + rl * EP_LD + cg);
                    const f32x4v hi = *reinterpret_cast<const f32x4v*>(ep + rl * EP_LD + cg + 4);
                    float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    const int64_t o = (int64_t)row * Co + c0;
                    if (a.residual != nullptr) {
                        const bf16x8 rr = *reinterpret_cast<const bf16x8*>(a.residual + o);
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] += (float)rr[e];
                    }
                    if (a.relu) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
                    }
                    if (a.y_is_f32) {
                        float* yo = static_cast<float*>(a.y) + o;
                        *reinterpret_cast<f32x4v*>(yo) = f32x4v{v[0], v[1], v[2], v[3]};
                        *reinterpret_cast<f32x4v*>(yo + 4) = f32x4v{v[4], v[5], v[6], v[7]};
                    } else {
                        bf16x8 h;
#pragma unroll
                        for (int e = 0; e < 8; ++e) h[e] = (__bf16)v[e];      // round to nearest even
                        *reinterpret_cast<bf16x8*>(static_cast<__bf16*>(a.y) + o) = h;
                    }
                }
            }
            __syncthreads();
        }
}

template <int BM, int BN>
int launch(ConvArgs a, hipStream_t st) {
    const int64_t tiles_m = ((int64_t)a.M + BM - 1) / BM;
    a.tiles_n = (a.Co + BN - 1) / BN;
    const int64_t tiles = tiles_m * a.tiles_n;
    if (tiles > 0x7fffffff) return VQA_ERR_ARG;
    hipLaunchKernelGGL((conv_bf16_kernel<BM, BN>), dim3((unsigned)tiles), dim3(NT), 0, st, a);
    VQA_CHECK_LAUNCH();
    return VQA_OK;
}

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int grid_for(int64_t items, int cap) { return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(items, 256), cap)); }

// slim pool1 (3x3 / stride 2 / 'SAME', padding never wins) on f32, stored as bf16: 8 channels per thread
__global__ __launch_bounds__(256) void maxpool3x3s2_bf16_kernel(const float* __restrict__ x, __bf16* __restrict__ y, int B, int Hi,
                                                                int Wi, int C, int Ho, int Wo, int pad_t, int pad_l) {
    const int C8 = C / 8;
    const int64_t total = (int64_t)B * Ho * Wo * C8;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c8 = (int)(i % C8);
        int64_t t = i / C8;
        const int ox = (int)(t % Wo); t /= Wo;
        const int oy = (int)(t % Ho);
        const int b = (int)(t / Ho);
        float m[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = oy * 2 - pad_t + ky, ix = ox * 2 - pad_l + kx;
                if ((unsigned)iy < (unsigned)Hi && (unsigned)ix < (unsigned)Wi) {
                    const f32x4v* p = reinterpret_cast<const f32x4v*>(x + (((int64_t)b * Hi + iy) * Wi + ix) * C) + c8 * 2;
                    const f32x4v lo = p[0], hi = p[1];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        m[e] = fmaxf(m[e], lo[e]);
                        m[4 + e] = fmaxf(m[4 + e], hi[e]);
                    }
                }
            }
        bf16x8 h;
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = (__bf16)m[e];
        reinterpret_cast<bf16x8*>(y)[i] = h;
    }
}

// resnet_utils.subsample on bf16: y[b, oy, ox, :] = x[b, oy*f, ox*f, :], 16-byte pieces
__global__ __launch_bounds__(256) void subsample_bf16_kernel(const __bf16* __restrict__ x, __bf16* __restrict__ y, int B, int Hi,
                                                             int Wi, int C, int Ho, int Wo, int f) {
    const int C8 = C / 8;
    const int64_t total = (int64_t)B * Ho * Wo * C8;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c8 = (int)(i % C8);
        int64_t t = i / C8;
        const int ox = (int)(t % Wo); t /= Wo;
        const int oy = (int)(t % Ho);
        const int b = (int)(t / Ho);
        reinterpret_cast<i32x4*>(y)[i] =
            reinterpret_cast<const i32x4*>(x + (((int64_t)b * Hi + (int64_t)oy * f) * Wi + (int64_t)ox * f) * C)[c8];
    }
}

}  // namespace

extern "C" int vqa_conv2d_nhwc_bf16(const void* x, int B, int Hi, int Wi, int Ci, const void* w, int kh, int kw, int Co,
                                    int stride, int pad_t, int pad_l, int Ho, int Wo, const float* scale, const float* shift,
                                    const void* residual, int relu, void* y, int y_is_f32, void* stream) {
    VQA_REQUIRE(x && w && y && B > 0 && Hi > 0 && Wi > 0 && Ci > 0 && Co > 0 && kh > 0 && kw > 0 && stride > 0 && Ho > 0 &&
                    Wo > 0 && pad_t >= 0 && pad_l >= 0,
                VQA_ERR_ARG);
    VQA_REQUIRE((int64_t)B * Ho * Wo < (1ll << 31) && (int64_t)B * Hi * Wi < (1ll << 31) && (int64_t)kh * kw * Ci < (1ll << 31),
                VQA_ERR_ARG);
    VQA_REQUIRE(Ci % 32 == 0 && vqa_aligned16(x) && vqa_aligned16(w) && vqa_aligned16(y) && vqa_aligned16(residual),
                VQA_ERR_ALIGN);
    const int64_t M = (int64_t)B * Ho * Wo, K = (int64_t)kh * kw * Ci, lim = 1ll << 32;
    VQA_REQUIRE(Co % 8 == 0 && (int64_t)B * Hi * Wi * Ci * 2 < lim && K * Co * 2 < lim && M * Co * (y_is_f32 ? 4 : 2) < lim,
                VQA_ERR_UNSUPPORTED);
    ConvArgs a;
    a.x = static_cast<const __bf16*>(x);
    a.w = static_cast<const __bf16*>(w);
    a.scale = scale;
    a.shift = shift;
    a.residual = static_cast<const __bf16*>(residual);
    a.y = y;
    a.M = (int)M; a.Co = Co; a.K = (int)K;
    a.Hi = Hi; a.Wi = Wi; a.Ci = Ci; a.Ho = Ho; a.Wo = Wo; a.kw = kw; a.stride = stride; a.pad_t = pad_t; a.pad_l = pad_l;
    a.cpt = Ci / BK;
    a.nk = kh * kw * a.cpt;
    a.tiles_n = 0;
    a.relu = relu ? 1 : 0;
    a.y_is_f32 = y_is_f32 ? 1 : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // by shape: 64-wide column tiles for the Co <= 64 layers (a 128-wide tile would run half empty); 64 x 64 tiles when
    // 128 x 128 ones would not give each of the 256 CUs its two workgroups; 128 x 128 otherwise
    int cfg = g_conv_bf16_cfg;
    if (cfg < 0) {
        if (Co <= 64) cfg = M >= 128 * 512 ? 1 : 2;
        else cfg = cdiv(M, 128) * cdiv(Co, 128) >= 512 ? 0 : 2;
    }
    switch (cfg) {
        case 0: return launch<128, 128>(a, st);
        case 1: return launch<128, 64>(a, st);
        default: return launch<64, 64>(a, st);
    }
}

extern "C" int vqa_conv_bf16_set_config(int cfg) {
    VQA_REQUIRE(cfg >= -1 && cfg <= 2, VQA_ERR_ARG);
    g_conv_bf16_cfg = cfg;
    return VQA_OK;
}

extern "C" int vqa_maxpool3x3s2_same_nhwc_bf16(const float* x, int B, int Hi, int Wi, int C, void* y, void* stream) {
    VQA_REQUIRE(x && y && B > 0 && Hi > 0 && Wi > 0 && C > 0, VQA_ERR_ARG);
    VQA_REQUIRE(C % 8 == 0 && vqa_aligned16(x) && vqa_aligned16(y), VQA_ERR_ALIGN);
    const int Ho = (Hi + 1) / 2, Wo = (Wi + 1) / 2;
    const int ph = std::max((Ho - 1) * 2 + 3 - Hi, 0), pw = std::max((Wo - 1) * 2 + 3 - Wi, 0);
    const int64_t total = (int64_t)B * Ho * Wo * (C / 8);
    hipLaunchKernelGGL(maxpool3x3s2_bf16_kernel, dim3(grid_for(total, 65536)), dim3(256), 0, (hipStream_t)stream, x,
                       static_cast<__bf16*>(y), B, Hi, Wi, C, Ho, Wo, ph / 2, pw / 2);
    VQA_CHECK_LAUNCH();
    return VQA_OK;
}

extern "C" int vqa_subsample_nhwc_bf16(const void* x, int B, int Hi, int Wi, int C, int factor, void* y, void* stream) {
    VQA_REQUIRE(x && y && B > 0 && Hi > 0 && Wi > 0 && C > 0 && factor > 0, VQA_ERR_ARG);
    VQA_REQUIRE(C % 8 == 0 && vqa_aligned16(x) && vqa_aligned16(y), VQA_ERR_ALIGN);
    const int Ho = (Hi - 1) / factor + 1, Wo = (Wi - 1) / factor + 1;
    const int64_t total = (int64_t)B * Ho * Wo * (C / 8);
    hipLaunchKernelGGL(subsample_bf16_kernel, dim3(grid_for(total, 65536)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const __bf16*>(x), static_cast<__bf16*>(y), B, Hi, Wi, C, Ho, Wo, factor);
    VQA_CHECK_LAUNCH();
    return VQA_OK;
}
