// Mixed-precision GEMM of the opt-in bf16 mode (VQA_FLAG_BF16_GEMM): f32 operands and results in
// HBM, bf16 operands in the matrix unit, f32 accumulation.
//
//   C[M,N] = op(A) op(B) (+ bias[N]) (+ D[M,N])        NN (forward), TN (dW = x^T d_pre), NT (dx = d_pre W^T)
//
// Every element of A and B is rounded to bf16 (round to nearest even: the f32 -> bf16 conversion of the hardware) on its
// way from the registers into LDS; no bf16 copy of an operand ever reaches HBM.  Products run on
// v_mfma_f32_32x32x16_bf16, sums stay in the f32 accumulators, bias and D are added in f32 and C is stored unrounded.
//
// Tile 128 x 128, BK 32, 256 threads = 4 waves of 64 x 64 (2 x 2 MFMA tiles of 32 x 32).  Both operands live in LDS as
// [row or column][k] bf16 with 80-byte rows (32 k + 8 pad: conflict-free ds_read_b128 of the 8 consecutive k one lane feeds
// to one MFMA), in TWO buffers of 20 KB: while the matrix pipe works through k tile t the same waves convert tile t + 1
// (already in registers) into the other buffer and fetch tile t + 2; one barrier per k tile.  40 KB of LDS and ~190
// VGPRs: two workgroups per CU.  (gemm_bf16x3.hip is this structure with three planes per operand.)
//
// Any M, N, K >= 1: loads outside the matrices are predicated off and replaced by zeros, stores are predicated.  Rows
// whose leading dimension or base address is not 16-byte aligned are fetched element by element (slower, same result).
// Split k cuts K into ranges (multiples of 32) whose partial products go to dense M x N slabs of the workspace and are
// summed in range order by a second kernel (bias rides in slab 0, D is added last): same inputs, same bits.
// max_blocks > 0: at most that many workgroups walk the (range, tile) units persistently.
//
// vqa_gemm_bf16_a16 (VQA_FLAG_BF16_FEATURES): the same kernel with a left operand that is bf16 in HBM already (the
// region-feature table at rest).  A thread fetches the same four elements as 8 bytes instead of 16 and stores them to LDS
// unconverted, so LDS -- and with it every bit of C -- is that of vqa_gemm_bf16 on the widened operand.
#include <algorithm>

#include "vqa_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4n __attribute__((ext_vector_type(4)));
typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));

// what a thread holds of an operand between its fetch and its LDS store: four consecutive elements as they are in HBM
template <typename T> struct Quad;
template <> struct Quad<float> { typedef f32x4n type; };
template <> struct Quad<uint16_t> { typedef u16x4 type; };      // raw bf16 patterns

constexpr int BM = 128, BN = 128, BK = 32, NT = 256;
constexpr int RS = 40;                       // bf16 per LDS row: 32 k + 8 pad = 80 bytes
constexpr int OPER = 128 * RS;               // bf16 per operand tile
constexpr int BUF = 2 * OPER;                // bf16 per LDS buffer (A tile | B tile)

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
// the same for bf16 elements; vec: p is 8-byte aligned
__device__ __forceinline__ u16x4 load4(const uint16_t* __restrict__ p, int valid, bool vec) {
    u16x4 v = {0, 0, 0, 0};
    if (valid >= 4 && vec) return *reinterpret_cast<const u16x4*>(p);
    if (valid > 0) v[0] = p[0];
    if (valid > 1) v[1] = p[1];
    if (valid > 2) v[2] = p[2];
    if (valid > 3) v[3] = p[3];
    return v;
}
__device__ __forceinline__ int clamp4(int n) { return n < 0 ? 0 : (n > 4 ? 4 : n); }
// an element on its way into LDS: f32 is rounded to bf16 (nearest even), a bf16 pattern goes through as it is
__device__ __forceinline__ __bf16 to_lds(float x) { return (__bf16)x; }
__device__ __forceinline__ __bf16 to_lds(uint16_t x) { return __builtin_bit_cast(__bf16, x); }

// One operand tile of 128 (rows: m of A, n of B) x 32 (k) in two storage forms:
//   KM = false: stored [row][k] (k contiguous).  Thread -> (row = idx / 8, 4 consecutive k), idx = tid + i * 256.
//   KM = true : stored [k][row] (row contiguous).  Thread -> a 4 (k) x 4 (row) block, transposed in registers.
// P points at the matrix, r0 / rows: the tile's first row and the matrix' row count, k0 / kend: this k tile and the end of
// the k range.
template <bool KM, typename T>
__device__ __forceinline__ void fetch_tile(typename Quad<T>::type (&r)[4], const T* __restrict__ P, int64_t ld, int r0, int rows,
                                           int k0, int kend, bool vec, int tid) {
    if (KM) {
        const int bk4 = (tid % 8) * 4, br4 = (tid / 8) * 4;
        const int valid = clamp4(rows - (r0 + br4));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + bk4 + i;
            r[i] = load4(P + (int64_t)k * ld + r0 + br4, k < kend ? valid : 0, vec);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + i * NT;
            const int row = r0 + idx / 8, k = k0 + (idx % 8) * 4;
            r[i] = load4(P + (int64_t)row * ld + k, row < rows ? clamp4(kend - k) : 0, vec);
        }
    }
}
template <bool KM, typename Q>
__device__ __forceinline__ void stage_tile(__bf16* __restrict__ s, const Q (&r)[4], int tid) {
    if (KM) {
        const int bk4 = (tid % 8) * 4, br4 = (tid / 8) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {                 // row br4 + j of the tile: its four consecutive k
            bf16x4 h;
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] = to_lds(r[i][j]);
            *reinterpret_cast<bf16x4*>(s + (br4 + j) * RS + bk4) = h;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + i * NT;
            bf16x4 h;
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = to_lds(r[i][j]);
            *reinterpret_cast<bf16x4*>(s + (idx / 8) * RS + (idx % 8) * 4) = h;
        }
    }
}

// A_KM: A stored [K][M] (transA); B_KM: B stored [K][N] (no transB).  Unit u = z * tiles + tile: k range z of the tile;
// with split k (slab > 0) C is the workspace, ldc = N, and slab z receives the partial product.  AT: element type of A in
// HBM (float, or uint16_t = bf16 patterns).
template <bool A_KM, bool B_KM, typename AT>
__global__ __launch_bounds__(NT, 2) void gemm_bf16_kernel(const AT* __restrict__ A, int lda, const float* __restrict__ B,
                                                          int ldb, float* Cbase, int ldc,
                                                          const float* __restrict__ bias0, const float* D0,
                                                          int ldd, int M, int N, int K, int tiles_n, int tiles, int units,
                                                          int k_per_split, int64_t slab, int vecA, int vecB) {
    __shared__ __attribute__((aligned(16))) __bf16 lds[2 * BUF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;           // the wave's 64 x 64 corner of the tile
    const int fr = lane & 31, fk = (lane >> 5) * 8;                    // the lane's row / column inside an MFMA tile, its 8 k

    for (int unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const int z = unit / tiles, tile = unit - z * tiles;
        const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
        const int kbeg = z * k_per_split, kend = min(K, kbeg + k_per_split);
        float* C = Cbase + z * slab;
        const float* bias = z > 0 ? nullptr : bias0;
        const float* D = z > 0 ? nullptr : D0;

        typename Quad<AT>::type ra[4];
        f32x4n rb[4];
        auto fetch = [&](int k0) {
            fetch_tile<A_KM>(ra, A, lda, m0, M, k0, kend, vecA != 0, tid);
            fetch_tile<B_KM>(rb, B, ldb, n0, N, k0, kend, vecB != 0, tid);
        };
        auto stage = [&](int buf) {
            stage_tile<A_KM>(lds + buf * BUF, ra, tid);
            stage_tile<B_KM>(lds + buf * BUF + OPER, rb, tid);
        };

        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

        const int nk = (kend - kbeg + BK - 1) / BK;
        bf16x8 fa[2][2], fb[2][2];                            // [k step][tile]
        auto read_frags = [&](int t) {
            const __bf16* cA = lds + (t & 1) * BUF;
            const __bf16* cB = cA + OPER;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    fa[ks][x] = *reinterpret_cast<const bf16x8*>(cA + (wm + x * 32 + fr) * RS + ks * 16 + fk);
                    fb[ks][x] = *reinterpret_cast<const bf16x8*>(cB + (wn + x * 32 + fr) * RS + ks * 16 + fk);
                }
        };
        auto mfmas = [&]() {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][a], fb[ks][b], acc[a][b], 0, 0, 0);
        };
        fetch(kbeg);
        stage(0);
        if (nk > 1) fetch(kbeg + BK);                         // tile 1 waits in the registers
        __syncthreads();
        int t = 0;
        for (; t + 1 < nk; ++t) {
            read_frags(t);
            stage((t + 1) & 1);                               // tile t + 1: convert and store into the other buffer
            mfmas();
            if (t + 2 < nk) fetch(kbeg + (t + 2) * BK);       // its latency hides behind the next tile's MFMAs
            __syncthreads();                                  // tile t + 1 is in LDS; tile t's buffer is free
        }
        read_frags(t);
        mfmas();
        // C / D map of a 32 x 32 tile: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int col = n0 + wn + b * 32 + (lane & 31);
                if (col >= N) continue;
                const float bv = bias != nullptr ? bias[col] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + wm + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (row >= M) continue;
                    float v = acc[a][b][r] + bv;
                    if (D != nullptr) v += D[(int64_t)row * ldd + col];
                    C[(int64_t)row * ldc + col] = v;
                }
            }
        __syncthreads();                                      // the next unit's first stage overwrites buffer 0
    }
}

// C[m, n] = (slab 0 + slab 1 + ... in range order) + D[m, n]     (slabs dense M x N)
__global__ __launch_bounds__(256) void gemm_bf16_reduce_kernel(const float* __restrict__ slabs, float* C, int ldc,
                                                               const float* D, int ldd, int M, int N, int S) {
    const int64_t n = (int64_t)M * N;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float v = slabs[i];
        for (int z = 1; z < S; ++z) v += slabs[(int64_t)z * n + i];
        const int64_t row = i / N;
        const int col = (int)(i - row * N);
        if (D != nullptr) v += D[row * ldd + col];
        C[row * ldc + col] = v;
    }
}

// the k ranges of a product: `split` ranges of kps (a multiple of 32) elements.  split_k <= 0 chooses by shape alone:
// enough (range, tile) units for two workgroups on each of the 256 CUs, at least 256 k per range, at most 8 slabs.
void plan_split(int M, int N, int K, int split_k, int* split, int* kps) {
    const int64_t tiles = (int64_t)((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    int s = split_k;
    if (s <= 0) {
        s = (int)std::min<int64_t>(512 / tiles, 8);
        s = std::min(s, K / 256);
    }
    if (s < 1) s = 1;
    int per = ((K + s - 1) / s + BK - 1) / BK * BK;
    if (per < BK) per = BK;
    *kps = per;
    *split = (K + per - 1) / per;
}

template <bool A_KM, bool B_KM, typename AT>
int launch(const AT* A, int lda, const float* B, int ldb, float* C, int ldc, const float* bias, const float* D, int ldd, int M,
           int N, int K, int split, int kps, int64_t slab, int max_blocks, hipStream_t st) {
    const int tiles_n = (N + BN - 1) / BN;
    const int64_t tiles = (int64_t)((M + BM - 1) / BM) * tiles_n, units = tiles * split;
    if (units > 0x7fffffff) return VQA_ERR_ARG;
    // four elements in one load: 16 bytes of f32, 8 bytes of bf16
    const int vecA = (lda % 4 == 0 && (reinterpret_cast<uintptr_t>(A) & (4 * sizeof(AT) - 1)) == 0) ? 1 : 0, vecB = (ldb % 4 == 0 && vqa_aligned16(B)) ? 1 : 0;
    const int grid = max_blocks > 0 ? (int)std::min<int64_t>(units, max_blocks) : (int)units;
    hipLaunchKernelGGL((gemm_bf16_kernel<A_KM, B_KM, AT>), dim3((unsigned)grid), dim3(NT), 0, st, A, lda, B, ldb, C, ldc, bias, D, ldd,
                       M, N, K, tiles_n, (int)tiles, (int)units, kps, slab, vecA, vecB);
    VQA_CHECK_LAUNCH();
    return VQA_OK;
}

}  // namespace

// floats of workspace vqa_gemm_bf16 needs for its split-k slabs (0: one range, no workspace); split_k <= 0: the split the
// kernel chooses for the shape
extern "C" int64_t vqa_gemm_bf16_workspace_floats(int M, int N, int K, int split_k) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    int split, kps;
    plan_split(M, N, K, split_k, &split, &kps);
    return split > 1 ? (int64_t)split * M * N : 0;
}

namespace {
template <typename AT>
int gemm_bf16_run(int transA, int transB, int M, int N, int K, const AT* A, int lda, const float* B, int ldb, float* C, int ldc,
                  const float* bias, const float* D, int ldd, int split_k, float* workspace, int64_t workspace_floats,
                  int max_blocks, void* stream) {
    VQA_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0, VQA_ERR_ARG);
    VQA_REQUIRE(!(transA && transB), VQA_ERR_UNSUPPORTED);
    VQA_REQUIRE(lda >= (transA ? M : K) && ldb >= (transB ? K : N) && ldc >= N && (D == nullptr || ldd >= N), VQA_ERR_ARG);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int split, kps;
    plan_split(M, N, K, split_k, &split, &kps);
    float* out = C;
    int ldo = ldc;
    int64_t slab = 0;
    if (split > 1) {
        VQA_REQUIRE(workspace != nullptr && workspace_floats >= (int64_t)split * M * N, VQA_ERR_WORKSPACE);
        out = workspace;
        ldo = N;
        slab = (int64_t)M * N;
    }
    const float* Dk = split > 1 ? nullptr : D;                // with slabs D joins in the reduction
    int rc;
    if (transA)
        rc = launch<true, true, AT>(A, lda, B, ldb, out, ldo, bias, Dk, ldd, M, N, K, split, kps, slab, max_blocks, st);
    else if (transB)
        rc = launch<false, false, AT>(A, lda, B, ldb, out, ldo, bias, Dk, ldd, M, N, K, split, kps, slab, max_blocks, st);
    else
        rc = launch<false, true, AT>(A, lda, B, ldb, out, ldo, bias, Dk, ldd, M, N, K, split, kps, slab, max_blocks, st);
    if (rc != VQA_OK || split <= 1) return rc;
    const int64_t n = (int64_t)M * N;
    int grid = (int)std::min<int64_t>((n + 255) / 256, 2048);
    if (max_blocks > 0) grid = std::min(grid, max_blocks);
    hipLaunchKernelGGL(gemm_bf16_reduce_kernel, dim3(grid), dim3(256), 0, st, workspace, C, ldc, D, ldd, M, N, split);
    VQA_CHECK_LAUNCH();
    return VQA_OK;
}
}  // namespace

extern "C" int vqa_gemm_bf16(int transA, int transB, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                             float* C, int ldc, const float* bias, const float* D, int ldd, int split_k, float* workspace,
                             int64_t workspace_floats, int max_blocks, void* stream) {
    return gemm_bf16_run<float>(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, D, ldd, split_k, workspace,
                                workspace_floats, max_blocks, stream);
}

// A: bf16 patterns in HBM, lda in elements; everything else as vqa_gemm_bf16 (workspace: vqa_gemm_bf16_workspace_floats)
extern "C" int vqa_gemm_bf16_a16(int transA, int transB, int M, int N, int K, const uint16_t* A, int lda, const float* B,
                                 int ldb, float* C, int ldc, const float* bias, const float* D, int ldd, int split_k,
                                 float* workspace, int64_t workspace_floats, int max_blocks, void* stream) {
    return gemm_bf16_run<uint16_t>(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, D, ldd, split_k, workspace,
                                   workspace_floats, max_blocks, stream);
}
