// The fused GRU-step GEMMs on the bf16 matrix unit: the four problems gru_step.hip builds per time step (gemm_args.h,
// EPI_GATES .. EPI_BWD_DH) with bf16 operands, f32 accumulation and the f32 epilogues of gemm_f32.hip.  GRU-step id
// GRU_CFG_BF16 (gemm_tiles.h) and the pre-training steps under VQA_PT_FLAG_BF16_ENCODER reach it.
//
// Rounding points: every element of the left operand (h_prev, r * h_prev, dc_pre, dr_pre | du_pre) and of the recurrent
// weights is rounded to bf16 (round to nearest even) on its way from the registers into LDS, exactly as gemm_bf16.hip
// does it; nothing is rounded in HBM.  Products run on v_mfma_f32_32x32x16_bf16, the sums stay in the f32 accumulators,
// the addend (xp or dh_acc), the gate math, the state update, the t < len mask and the backward formulas are f32 and
// written operation for operation as the f32 step kernel has them.  The state is carried in f32: only the operand copy
// of h is rounded, and a finished row's hs[t+1] is hs[t] bit for bit.  The weights are converted per k tile (no bf16
// copy of them exists anywhere).
//
// Two tiles, both 256 threads = 2 x 2 waves, BK 32, LDS rows of 80 bytes ([row or column][k] bf16, 32 k + 8 pad), two
// LDS buffers and one barrier per k tile (the pipeline of gemm_bf16_kernel): 64 x 64 (waves of 32 x 32, 20 KB of LDS),
// the default at every row count, and 128 x 128 (waves of 64 x 64, 40 KB), which the row threshold below can select.
// One workgroup per tile, plain launches, no atomics: same inputs, same bits.
//
// Any rows >= 1, N >= 1, K >= 1: loads outside a matrix are predicated off and read as zeros (the tapes sit end to end
// in one workspace), stores are predicated.  Rows that are not 16-byte aligned are fetched element by element.
#include "vqa_common.h"
#include "gemm_args.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4n __attribute__((ext_vector_type(4)));

constexpr int BK = 32, NT = 256;
constexpr int RS = 40;                       // bf16 per LDS row: 32 k + 8 pad = 80 bytes

// four consecutive floats at p, the first `valid` of them inside the matrix (the rest read as 0); vec: p is 16-byte aligned
__device__ __forceinline__ f32x4n load4(const float* __restrict__ p, int valid, bool vec) {
    f32x4n v = {0.f, 0.f, 0.f, 0.f};
    if (valid >= 4 && vec) return *reinterpret_cast<const f32x4n*>(p);
    if (valid > 0) v[0] = p[0];
    if (valid > 1) v[1] = p[1];
    if (valid > 2) v[2] = p[2];
    if (valid > 3) v[3] = p[3];
    return v;
}
__device__ __forceinline__ int clamp4(int n) { return n < 0 ? 0 : (n > 4 ? 4 : n); }

// One operand tile of ROWS (m of A, n of B) x 32 (k), ROWS / 32 quads per thread, in two storage forms:
//   KM = false: stored [row][k] (k contiguous).  Thread -> (row = idx / 8, 4 consecutive k), idx = tid + i * 256.
//   KM = true : stored [k][row] (row contiguous).  Thread -> a (ROWS / 32) (k) x 4 (row) block, transposed in registers.
template <bool KM, int ROWS>
__device__ __forceinline__ void fetch_tile(f32x4n (&r)[ROWS / 32], const float* __restrict__ P, int64_t ld, int r0, int rows,
                                           int k0, int K, bool vec, int tid) {
    constexpr int NQ = ROWS / 32;
    if (KM) {
        const int bk = (tid % (32 / NQ)) * NQ, br4 = (tid / (32 / NQ)) * 4;
        const int valid = clamp4(rows - (r0 + br4));
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int k = k0 + bk + i;
            r[i] = load4(P + (int64_t)k * ld + r0 + br4, k < K ? valid : 0, vec);
        }
    } else {
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int idx = tid + i * NT;
            const int row = r0 + idx / 8, k = k0 + (idx % 8) * 4;
            r[i] = load4(P + (int64_t)row * ld + k, row < rows ? clamp4(K - k) : 0, vec);
        }
    }
}
// ... and its way into LDS as [row][k] bf16: the rounding point of both operands
template <bool KM, int ROWS>
__device__ __forceinline__ void stage_tile(__bf16* __restrict__ s, const f32x4n (&r)[ROWS / 32], int tid) {
    constexpr int NQ = ROWS / 32;
    typedef __bf16 bf16xq __attribute__((ext_vector_type(NQ)));
    if (KM) {
        const int bk = (tid % (32 / NQ)) * NQ, br4 = (tid / (32 / NQ)) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {                 // row br4 + j of the tile: its NQ consecutive k
            bf16xq h;
#pragma unroll
            for (int i = 0; i < NQ; ++i) h[i] = (__bf16)r[i][j];
            *reinterpret_cast<bf16xq*>(s + (br4 + j) * RS + bk) = h;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int idx = tid + i * NT;
            bf16x4 h;
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = (__bf16)r[i][j];
            *reinterpret_cast<bf16x4*>(s + (idx / 8) * RS + (idx % 8) * 4) = h;
        }
    }
}

// what the kernel needs of the product: acc = A[M,K] (row major) * B, B stored [K,N] (B_KM) or [N,K]
struct StepGemm {
    const float* A; int lda;
    const float* B; int ldb;
    const float* D; int ldd;      // f32 addend of the epilogue, or null
    int M, N, K, tiles_n, vecA, vecB;
};

template <int BM, int BN, int EPI>
__global__ __launch_bounds__(NT, (BM * BN >= 128 * 128) ? 2 : 4) void gru_step_bf16_kernel(StepGemm p, EpiArgs ep) {
    constexpr bool B_KM = (EPI == EPI_GATES || EPI == EPI_CAND);      // forward: W[K,N]; backward: W^T, stored [N,K]
    constexpr int TM = BM / 64, TN = BN / 64;                         // 32 x 32 MFMA tiles per wave
    constexpr int OPER_A = BM * RS, BUF = (BM + BN) * RS;             // bf16 per operand tile / per LDS buffer
    __shared__ __attribute__((aligned(16))) __bf16 lds[2 * BUF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * (BM / 2), wn = (wave & 1) * (BN / 2);   // the wave's corner of the tile
    const int fr = lane & 31, fk = (lane >> 5) * 8;                      // the lane's row / column inside an MFMA tile, its 8 k
    const int m0 = ((int)blockIdx.x / p.tiles_n) * BM, n0 = ((int)blockIdx.x % p.tiles_n) * BN;

    f32x4n ra[BM / 32], rb[BN / 32];
    auto fetch = [&](int k0) {
        fetch_tile<false, BM>(ra, p.A, p.lda, m0, p.M, k0, p.K, p.vecA != 0, tid);
        fetch_tile<B_KM, BN>(rb, p.B, p.ldb, n0, p.N, k0, p.K, p.vecB != 0, tid);
    };
    auto stage = [&](int buf) {
        stage_tile<false, BM>(lds + buf * BUF, ra, tid);
        stage_tile<B_KM, BN>(lds + buf * BUF + OPER_A, rb, tid);
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int nk = (p.K + BK - 1) / BK;
    bf16x8 fa[2][TM], fb[2][TN];                              // [k step][tile]
    auto read_frags = [&](int t) {
        const __bf16* cA = lds + (t & 1) * BUF;
        const __bf16* cB = cA + OPER_A;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int x = 0; x < TM; ++x) fa[ks][x] = *reinterpret_cast<const bf16x8*>(cA + (wm + x * 32 + fr) * RS + ks * 16 + fk);
#pragma unroll
            for (int x = 0; x < TN; ++x) fb[ks][x] = *reinterpret_cast<const bf16x8*>(cB + (wn + x * 32 + fr) * RS + ks * 16 + fk);
        }
    };
    auto mfmas = [&]() {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][a], fb[ks][b], acc[a][b], 0, 0, 0);
    };
    fetch(0);
    stage(0);
    if (nk > 1) fetch(BK);                                    // tile 1 waits in the registers
    __syncthreads();
    int t = 0;
    for (; t + 1 < nk; ++t) {
        read_frags(t);
        stage((t + 1) & 1);                                   // tile t + 1: convert and store into the other buffer
        mfmas();
        if (t + 2 < nk) fetch((t + 2) * BK);                  // its latency hides behind the next tile's MFMAs
        __syncthreads();                                      // tile t + 1 is in LDS; tile t's buffer is free
    }
    read_frags(t);
    mfmas();

    // The fused epilogues, f32, element by element in the C / D map of a 32 x 32 tile (col = lane & 31, row = (reg & 3) +
    // 8 * (reg >> 2) + 4 * (lane >> 5)): the 32 lanes of a row move 128 contiguous bytes per access.
    const int H = ep.H;
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b) {
            const int col = n0 + wn + b * 32 + (lane & 31);
            if (col >= p.N) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row >= p.M) continue;
                const int64_t o = (int64_t)row * H + col;
                const float d = p.D != nullptr ? p.D[(int64_t)row * p.ldd + col] : 0.f;
                const float vv = acc[a][b][r] + d;
                if (EPI == EPI_GATES) {
                    const float s = sigmoidf_stable(vv);
                    if (col < H) {
                        ep.o0[o] = s;                       // r
                        ep.o2[o] = s * ep.h_prev[o];        // r * h_prev
                    } else {
                        ep.o1[o - H] = s;                   // u
                    }
                } else if (EPI == EPI_CAND) {
                    const float a0 = ep.h_prev[o], a1 = ep.i0[o];
                    const float c = tanhf(vv);
                    ep.o0[o] = c;
                    ep.o1[o] = (ep.t < ep.len[row]) ? (a1 * a0 + (1.f - a1) * c) : a0;      // h_new
                } else if (EPI == EPI_BWD_RH) {
                    const float a0 = ep.h_prev[o], a1 = ep.i0[o], a2 = ep.o1[o];
                    ep.o0[(int64_t)row * ep.ldo + col] = vv * a0 * a1 * (1.f - a1);         // dr_pre
                    ep.o1[o] = a2 + vv * a1;                                                // dh_acc
                } else {
                    const float a0 = ep.h_prev[o], a1 = ep.i0[o], a2 = ep.i1[o];
                    const bool live = ep.t < ep.len[row];
                    ep.o0[(int64_t)row * ep.ldo + col] = live ? vv * (1.f - a1) * (1.f - a2 * a2) : 0.f;       // dc_pre
                    ep.o1[(int64_t)row * ep.ldo + col] = live ? vv * (a0 - a2) * a1 * (1.f - a1) : 0.f;        // du_pre
                    ep.o2[o] = live ? vv * a1 : vv;                                                            // dh_acc
                }
            }
        }
}

template <int BM, int BN, int EPI>
int launch_tile(const GemmArgs& a, const EpiArgs& ep, hipStream_t st) {
    StepGemm p;
    p.A = a.A; p.lda = a.lda; p.B = a.B; p.ldb = a.ldb; p.D = a.D; p.ldd = a.ldd;
    p.M = a.M; p.N = a.N; p.K = a.K; p.vecA = a.vecA; p.vecB = a.vecB;
    p.tiles_n = (a.N + BN - 1) / BN;
    const int64_t tiles = (int64_t)((a.M + BM - 1) / BM) * p.tiles_n;
    if (tiles > 0x7fffffff) return VQA_ERR_ARG;
    hipLaunchKernelGGL((gru_step_bf16_kernel<BM, BN, EPI>), dim3((unsigned)tiles), dim3(NT), 0, st, p, ep);
    VQA_CHECK_LAUNCH();
    return VQA_OK;
}

// Tile by rows: the 128 x 128 tile from tall_rows rows, the 64 x 64 tile below.  Measured at H 1024, T 10
// (profiles/r28_gru_bf16_encoder.txt), 64 x 64 wins at every row count of the pre-training recurrence -- 5120 rows: forward
// 2050 against 2314 us, backward 1362 against 1982; 2560 rows: 1196 / 905 against 1866 / 1613; 1152 rows: 831 / 771 against
// 1699 / 1480 -- the large tile's element-wise epilogue moves 64 elements per lane at 3 waves per SIMD.  So no row
// count selects the large tile by default; VQA_HOT_GRU_BF16_TALL_ROWS sets the threshold (tuning; 0: always 128 x 128).
constexpr int TALL_ROWS_NEVER = 0x7fffffff;
template <int EPI>
int launch_epi(const GemmArgs& a, const EpiArgs& ep, hipStream_t st) {
    static const int tall_rows = vqa_env_int("VQA_HOT_GRU_BF16_TALL_ROWS", TALL_ROWS_NEVER);
    return a.M >= tall_rows ? launch_tile<128, 128, EPI>(a, ep, st) : launch_tile<64, 64, EPI>(a, ep, st);
}

}  // namespace

int vqa_gru_step_launch_bf16(int epi, const GemmArgs& a, const EpiArgs& ep, hipStream_t st) {
    VQA_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0 && a.A && a.B, VQA_ERR_ARG);
    switch (epi) {
        case EPI_GATES: return launch_epi<EPI_GATES>(a, ep, st);
        case EPI_CAND: return launch_epi<EPI_CAND>(a, ep, st);
        case EPI_BWD_RH: return launch_epi<EPI_BWD_RH>(a, ep, st);
        case EPI_BWD_DH: return launch_epi<EPI_BWD_DH>(a, ep, st);
        default: return VQA_ERR_ARG;
    }
}
