// Fused Hadamard attention + attention pooling for gfx950 (SURVEY rows a6+a7).
//
// Reference: modules.hadamard_attention (vlmap/modules.py:67-97) followed by
// modules.attention_pooling (vlmap/modules.py:23-39):
//   s[b,r]   = sum_h (v[b,r,h] * qv[b,h]) * keep[b,r,h]/keep_prob * w[h] + bias
//   s[r>=nb] = -inf ; att = softmax_R(s) ; pooled[b,:] = sum_r att[b,r] * V[b,r,:]
//
// `rep` queries may share one memory (the pre-training model attends 5 key boxes per image over the
// same 36 regions: vlmap_memft/model_vlmap_bf_or_wordset_withatt_sp.py:323-364 tiles V_ft x5 -- here
// the tile is never materialised): v, V, nb are indexed by the memory m, qv / keepmask / att / pooled
// by the query q = m*rep + j.
//
// HBM-bound.  One workgroup (4 waves) per sample keeps s/att for the <= 36
// regions in LDS, so v (147 KB), the keep mask (37 KB) and the raw features V
// (295 KB) are each read exactly once with 16-byte-per-lane coalesced loads and
// the scores never leave the CU.  Row dot products use wavefront (64-lane)
// shuffles; the softmax over R runs in one wave.
#include "keep_launch.h"

namespace {

constexpr int MAX_R = 1024;

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef unsigned u32x2v __attribute__((ext_vector_type(2)));

// The pooled memory V is f32, or bf16 at rest (VQA_FLAG_BF16_FEATURES; the _v16 entry points): VT = float or uint16_t (raw
// bf16 patterns).  A lane that loads four consecutive d as one 16-byte vector loads the same four d of a bf16 memory as 8
// bytes and widens them with a 16-bit shift, so every sum below keeps its elements and its order: the outputs are
// bit for bit those of the f32 kernels on the widened values.  Raw: what stays in registers between the load and the use.
template <typename VT> struct VMem;
template <> struct VMem<float> {
    typedef f32x4v Raw;
    static __device__ __forceinline__ Raw load(const float* __restrict__ p, int64_t i4) { return reinterpret_cast<const f32x4v*>(p)[i4]; }
    static __device__ __forceinline__ f32x4v widen(Raw r) { return r; }
    static __device__ __forceinline__ float4 load_f4(const float* __restrict__ p, int64_t i4) { return reinterpret_cast<const float4*>(p)[i4]; }
};
template <> struct VMem<uint16_t> {
    typedef u32x2v Raw;
    static __device__ __forceinline__ Raw load(const uint16_t* __restrict__ p, int64_t i4) { return reinterpret_cast<const u32x2v*>(p)[i4]; }
    static __device__ __forceinline__ f32x4v widen(Raw r) {
        f32x4v x;
        x.x = __uint_as_float(r.x << 16); x.y = __uint_as_float(r.x & 0xFFFF0000u);
        x.z = __uint_as_float(r.y << 16); x.w = __uint_as_float(r.y & 0xFFFF0000u);
        return x;
    }
    static __device__ __forceinline__ float4 load_f4(const uint16_t* __restrict__ p, int64_t i4) {
        const f32x4v x = widen(load(p, i4));
        return make_float4(x.x, x.y, x.z, x.w);
    }
};

// 512 threads: twice the waves (and loads in flight) per sample of the 256-thread form; the kernel is a
// pure stream over v, the keep mask and V (~480 KB per sample)
constexpr int FWD_THREADS = 512;
template <typename VT, int KP = KEEP_BYTES, typename... KS>
__global__ __launch_bounds__(FWD_THREADS) void attn_pool_fwd_kernel(
    const float* __restrict__ v, const float* __restrict__ qv, const VT* __restrict__ V,
    const int32_t* __restrict__ nb, const float* __restrict__ w, const float* __restrict__ bias,
    const uint8_t* __restrict__ keepmask, float inv_keep, float* __restrict__ att_out, float* __restrict__ pooled, int R,
    int H, int D, int rep, KS... ks) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // qw[H] | s[R]
    float* qw = lds;
    float* s = lds + H;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;   // b = query index
    const int mem = b / rep;
    const float* vb = v + (int64_t)mem * R * H;
    const uint8_t* mb = keepmask ? keepmask + (int64_t)b * R * H : nullptr;
    const VT* Vb = V + (int64_t)mem * R * D;

    for (int h = threadIdx.x; h < H; h += FWD_THREADS) qw[h] = qv[(int64_t)b * H + h] * w[h];
    __syncthreads();

    const int H4 = H / 4;
    for (int r = wave; r < R; r += FWD_THREADS / 64) {
        float acc = 0.f;
        const float* vr = vb + (int64_t)r * H;
#pragma unroll 4
        for (int hu = lane; hu < H4; hu += 64) {
            const float4 x = reinterpret_cast<const float4*>(vr)[hu];
            const float4 q = reinterpret_cast<const float4*>(qw)[hu];
            if constexpr (KP == KEEP_SEEDED) {
                const KeepSeed sd = keep_seed_of(ks...);
                const uchar4 m = keep_uchar4(keep_word4(sd.key, sd.word0 + ((uint64_t)b * R + r) * H4 + hu, sd.thr));
                // (the explicit form's two branches share ONE add, `acc += masked ? sum * inv_keep : sum`, so hipcc rounds the
                // product there; alone in its loop it would become fma(sum, inv_keep, acc) -- other bits)
                acc += mul_rounded(x.x * q.x * m.x + x.y * q.y * m.y + x.z * q.z * m.z + x.w * q.w * m.w, inv_keep);
            } else if (mb != nullptr) {
                const uchar4 m = reinterpret_cast<const uchar4*>(mb + (int64_t)r * H)[hu];
                acc += (x.x * q.x * m.x + x.y * q.y * m.y + x.z * q.z * m.z + x.w * q.w * m.w) * inv_keep;
            } else {
                acc += x.x * q.x + x.y * q.y + x.z * q.z + x.w * q.w;
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) s[r] = acc + bias[0];
    }
    __syncthreads();

    if (wave == 0) {
        const int n_valid = nb[mem];
        float mx = -INFINITY;
        for (int r = lane; r < R; r += 64) {
            const float x = (r < n_valid) ? s[r] : -INFINITY;
            s[r] = x;
            mx = fmaxf(mx, x);
        }
        mx = wave_max(mx);
        float sum = 0.f;
        for (int r = lane; r < R; r += 64) {
            const float e = expf(s[r] - mx);  // all -inf (nb == 0) -> NaN, like TF
            s[r] = e;
            sum += e;
        }
        sum = wave_sum(sum);
        for (int r = lane; r < R; r += 64) {
            const float a = s[r] / sum;
            s[r] = a;
            att_out[(int64_t)b * R + r] = a;
        }
    }
    __syncthreads();

    const int D4 = D / 4;
    for (int du = threadIdx.x; du < D4; du += FWD_THREADS) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 6
        for (int r = 0; r < R; ++r) {
            const float a = s[r];
            const float4 x = VMem<VT>::load_f4(Vb + (int64_t)r * D, du);
            acc.x += a * x.x; acc.y += a * x.y; acc.z += a * x.z; acc.w += a * x.w;
        }
        reinterpret_cast<float4*>(pooled + (int64_t)b * D)[du] = acc;
    }
}

// The same for the shapes of the models (H a multiple of 256 up to 1024, D a multiple of 2048 up to 4096 or 1024, R <= 40),
// restructured around loads in flight.  The generic kernel above streams 480 KB per sample in three dependent phases
// whose workgroups run in lockstep (all 512 are resident at once), so the memory system idles at every phase
// boundary: 251.9 MB in 64.5 us = 3.9 TB/s at bs 512.  Here (a) each thread fetches its first PF rows of V before
// anything else -- they do not depend on the scores and land during the score phase, (b) a wave issues the loads of
// all rows of a score batch (3 + 2 of its <= 5 rows, one query per workgroup) before the first use, so the batch costs
// one memory latency instead of one per row, (c) the pooling loop keeps 7 rows per thread in flight.
// (hipcc note: the loads are written on a native 4-float vector type and are UNCONDITIONAL -- row indices are clamped
// and rows past R get weight zero.  With HIP's float4 struct a guarded `in ? load : zero` becomes four scalar loads
// in four branches, each waited for before the next is issued.)
#ifndef VQA_ATTN_PF
#define VQA_ATTN_PF 8
#endif
#ifndef VQA_ATTN_POOL_BATCH
#define VQA_ATTN_POOL_BATCH 7
#endif

// The forms of the fast forward: one kernel (attn_pool_fwd_form_kernel), one row of constants per dispatch route.
//   REP     queries per workgroup.  1: one workgroup per QUERY (any rep: m = q / rep).  5: one workgroup per MEMORY (the
//           pre-training model: 5 key boxes per image), so v and V are read once per image instead of once per query (the
//           per-query form re-reads them REP times through L2: 1.2 GB of requests for 0.32 GB of distinct bytes at 512
//           images) and only the keep masks are per query
//   PF      rows of V a thread fetches before anything else; BATCH: rows per thread in flight in the pooling loop
//   S0..S2  rows per score batch of a wave (its <= 5 rows wave + 8 i, R <= 40)
//   BLOCKS  workgroups per CU the registers are allotted for (__launch_bounds__)
struct FwdFast     { static constexpr int REP = 1, PF = VQA_ATTN_PF, BATCH = VQA_ATTN_POOL_BATCH, S0 = 3, S1 = 2, S2 = 0, BLOCKS = 4; };
struct FwdRep      { static constexpr int REP = 5, PF = 4, BATCH = 6, S0 = 2, S1 = 2, S2 = 1, BLOCKS = 2; };
struct FwdRepD1024 { static constexpr int REP = 5, PF = 6, BATCH = 6, S0 = 2, S1 = 2, S2 = 1, BLOCKS = 2; };

// What a thread holds of one row of V and of pooled: N pieces, raw between the load and the use (half the registers for a
// bf16 memory), widened where they are used; lane -> element mapping and summation orders do not depend on VT.
// D a multiple of 2048: D / 2048 pieces of four elements at threadIdx.x + c * 512 ...
typedef float f32x2v __attribute__((ext_vector_type(2)));
template <typename VT, int D> struct VCols {
    static_assert(D % 2048 == 0, "a 1024-wide memory is f32");
    static constexpr int N = D / 2048;
    typedef typename VMem<VT>::Raw Raw;
    typedef f32x4v Acc;
    static __device__ __forceinline__ Raw load(const VT* __restrict__ Vb, int r, int c) {
        return VMem<VT>::load(Vb, (int64_t)r * (D / 4) + threadIdx.x + c * FWD_THREADS);
    }
    static __device__ __forceinline__ Acc widen(Raw x) { return VMem<VT>::widen(x); }
    static __device__ __forceinline__ void store(float* __restrict__ row, int c, Acc a) {
        reinterpret_cast<f32x4v*>(row)[threadIdx.x + c * FWD_THREADS] = a;
    }
};
// ... D == 1024 (v_adapt of the pre-training model, an f32 activation): a row is 512 float2 columns, one per thread, so
// every thread streams V with 8-byte loads (a wave still covers 512 contiguous bytes per row) and sums its rows in order
// -- the generic kernel's summation order, no thread idle and no partial sums to combine
template <> struct VCols<float, 1024> {
    static constexpr int N = 1;
    typedef f32x2v Raw;
    typedef f32x2v Acc;
    static __device__ __forceinline__ Raw load(const float* __restrict__ Vb, int r, int) {
        return reinterpret_cast<const f32x2v*>(Vb)[(int64_t)r * FWD_THREADS + threadIdx.x];
    }
    static __device__ __forceinline__ Acc widen(Raw x) { return x; }
    static __device__ __forceinline__ void store(float* __restrict__ row, int, Acc a) {
        reinterpret_cast<f32x2v*>(row)[threadIdx.x] = a;
    }
};

// scores of CNT rows (row0, row0 + 8, ...) of one wave against the REP queries of its workgroup, from one load of each
// row: every load of the batch is issued before the first use.  The mask word of query q0 + j is loaded from mb4 (the base
// of query q0; KEEP_BYTES) or computed (KEEP_SEEDED: sq.word0 = the word index of query q0's mask) -- at REP == 1
// together with the rows, before qw is awaited, so the batch costs one memory latency; at REP > 1 query by query.
template <int H4L, int CNT, int KP, int REP>
__device__ __forceinline__ void attn_score_rows(const f32x4v* __restrict__ vb4, const unsigned* __restrict__ mb4,
                                                const f32x4v* qw4, float* s, int R, int row0, float inv_keep, float bias0,
                                                int lane, bool sync_first, KeepSeed sq) {
    constexpr int H4 = H4L * 64;
    f32x4v x[CNT][H4L];
    unsigned m[CNT][H4L];
    int rr[CNT];
    auto mask_word = [&](int64_t at) -> unsigned {      // word `at` of the mask of query q0
        if constexpr (KP == KEEP_SEEDED) {
            return keep_word4(sq.key, sq.word0 + (uint64_t)at, sq.thr);
        } else {
            return mb4[at];
        }
    };
#pragma unroll
    for (int i = 0; i < CNT; ++i) {
        const int r = min(row0 + 8 * i, R - 1);
        rr[i] = r;
#pragma unroll
        for (int k = 0; k < H4L; ++k) {
            const int64_t at = (int64_t)r * H4 + lane + 64 * k;
            x[i][k] = vb4[at];
            if constexpr (REP == 1 && KP != KEEP_NONE) m[i][k] = mask_word(at);
        }
    }
    if (sync_first) __syncthreads();                 // qw is complete
#pragma unroll
    for (int j = 0; j < REP; ++j) {
        if constexpr (REP > 1 && KP != KEEP_NONE) {
#pragma unroll
            for (int i = 0; i < CNT; ++i)
#pragma unroll
                for (int k = 0; k < H4L; ++k) m[i][k] = mask_word(((int64_t)j * R + rr[i]) * H4 + lane + 64 * k);
        }
#pragma unroll
        for (int i = 0; i < CNT; ++i) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < H4L; ++k) {
                const f32x4v q = qw4[j * H4 + lane + 64 * k];
                if (KP != KEEP_NONE) {
                    const unsigned mm = m[i][k];
                    acc += (x[i][k].x * q.x * (float)(mm & 0xFFu) + x[i][k].y * q.y * (float)((mm >> 8) & 0xFFu) +
                            x[i][k].z * q.z * (float)((mm >> 16) & 0xFFu) + x[i][k].w * q.w * (float)(mm >> 24)) * inv_keep;
                } else {
                    acc += x[i][k].x * q.x + x[i][k].y * q.y + x[i][k].z * q.z + x[i][k].w * q.w;
                }
            }
            acc = wave_sum(acc);
            if (lane == 0 && row0 + 8 * i < R) s[j * 40 + row0 + 8 * i] = acc + bias0;
        }
    }
}

// Workgroup blockIdx.x takes the queries q0 .. q0 + REP - 1, q0 = blockIdx.x * REP, of the memory q0 / rep (REP == 1 with
// any rep, or REP == rep).  A wave scores its rows for all REP queries, waves 0..REP-1 run the REP softmaxes, and the
// pooling loop keeps REP accumulators per thread over one stream of V.
template <typename F, int H4L, int D, int KP, typename VT, typename... KS>
__global__ __launch_bounds__(FWD_THREADS, F::BLOCKS) void attn_pool_fwd_form_kernel(
    const float* __restrict__ v, const float* __restrict__ qv, const VT* __restrict__ V,
    const int32_t* __restrict__ nb, const float* __restrict__ w, const float* __restrict__ bias,
    const uint8_t* __restrict__ keepmask, float inv_keep, float* __restrict__ att_out, float* __restrict__ pooled, int R,
    int rep, KS... ks) {
    typedef VCols<VT, D> COL;
    constexpr int REP = F::REP, PF = F::PF, BATCH = F::BATCH, H = H4L * 256, N = COL::N;
    static_assert(REP <= FWD_THREADS / 64, "one softmax wave per query");
    static_assert(F::S0 + F::S1 + F::S2 == 5, "a wave owns rows wave + 8 i, i < 5 (R <= 40)");
    extern __shared__ __attribute__((aligned(16))) float lds[];  // qw[REP][H] | s[REP][40]
    float* qw = lds;
    float* s = lds + REP * H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * REP, mem = b / rep;
    const int64_t q0 = b;                                          // first query of this workgroup
    const f32x4v* vb4 = reinterpret_cast<const f32x4v*>(v + (int64_t)mem * R * H);
    const unsigned* mb4 = KP == KEEP_BYTES ? reinterpret_cast<const unsigned*>(keepmask + q0 * R * H) : nullptr;
    const VT* Vb = V + (int64_t)mem * R * D;

    // (a) first rows of this thread's V columns
    typename COL::Raw xv[PF][N];
#pragma unroll
    for (int r = 0; r < PF; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) xv[r][c] = COL::load(Vb, min(r, R - 1), c);

    for (int i = threadIdx.x; i < REP * H; i += FWD_THREADS) qw[i] = qv[q0 * H + i] * w[i % H];
    const float bias0 = bias[0];

    // (b) scores
    const f32x4v* qw4 = reinterpret_cast<const f32x4v*>(qw);
    KeepSeed sq = keep_seed_of(ks...);                              // zeros unless KEEP_SEEDED
    sq.word0 += (uint64_t)q0 * R * (H / 4);
    attn_score_rows<H4L, F::S0, KP, REP>(vb4, mb4, qw4, s, R, wave, inv_keep, bias0, lane, true, sq);
    attn_score_rows<H4L, F::S1, KP, REP>(vb4, mb4, qw4, s, R, wave + 8 * F::S0, inv_keep, bias0, lane, false, sq);
    if constexpr (F::S2 > 0)
        attn_score_rows<H4L, F::S2, KP, REP>(vb4, mb4, qw4, s, R, wave + 8 * (F::S0 + F::S1), inv_keep, bias0, lane, false, sq);
    __syncthreads();

    if (wave < REP) {
        float* sj = s + wave * 40;
        const int n_valid = nb[mem];
        const float x = (lane < R && lane < n_valid) ? sj[min(lane, R - 1)] : -INFINITY;      // R <= 40 < 64: one lane per row
        const float mx = wave_max(x);
        const float e = (lane < R) ? expf(x - mx) : 0.f;  // all -inf (nb == 0) -> NaN, like TF
        const float sum = wave_sum(e);
        if (lane < R) {
            const float a = e / sum;
            sj[lane] = a;
            att_out[(q0 + wave) * R + lane] = a;
        }
    }
    __syncthreads();

    // (c) pooling, rows in order
    typename COL::Acc acc[REP][N];
#pragma unroll
    for (int j = 0; j < REP; ++j)
#pragma unroll
        for (int c = 0; c < N; ++c) acc[j][c] = (typename COL::Acc)(0.f);
#pragma unroll
    for (int r = 0; r < PF; ++r) {
#pragma unroll
        for (int j = 0; j < REP; ++j) {
            const float a = (r < R) ? s[j * 40 + min(r, R - 1)] : 0.f;
#pragma unroll
            for (int c = 0; c < N; ++c) acc[j][c] += a * COL::widen(xv[r][c]);
        }
    }
    for (int r0 = PF; r0 < R; r0 += BATCH) {
        typename COL::Raw y[BATCH][N];
#pragma unroll
        for (int i = 0; i < BATCH; ++i)
#pragma unroll
            for (int c = 0; c < N; ++c) y[i][c] = COL::load(Vb, min(r0 + i, R - 1), c);
#pragma unroll
        for (int i = 0; i < BATCH; ++i) {
#pragma unroll
            for (int j = 0; j < REP; ++j) {
                const float a = (r0 + i < R) ? s[j * 40 + min(r0 + i, R - 1)] : 0.f;
#pragma unroll
                for (int c = 0; c < N; ++c) acc[j][c] += a * COL::widen(y[i][c]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < REP; ++j)
#pragma unroll
        for (int c = 0; c < N; ++c) COL::store(pooled + (q0 + j) * D, c, acc[j][c]);
}

// Backward.  One workgroup per MEMORY walks its `rep` queries, so dv (the gradient of the shared
// v block) is accumulated over the queries in registers and written once.  512 threads: the last
// phase gives every float4 column of v to TWO threads that take alternate rows (dv rows are
// independent; the per-query column sums are combined through LDS).
constexpr int BWD_THREADS = 512;
template <int REP, typename VT = float, int KP = KEEP_BYTES, typename... KS>
__global__ __launch_bounds__(BWD_THREADS) void attn_pool_bwd_kernel(
    const float* __restrict__ dpooled, const float* __restrict__ v, const float* __restrict__ qv,
    const VT* __restrict__ V, const float* __restrict__ att, const float* __restrict__ w,
    const uint8_t* __restrict__ keepmask, float inv_keep, float* __restrict__ dv, float* __restrict__ dqv,
    float* __restrict__ part_dw, float* __restrict__ part_db, int R, int H, int D, int rep, KS... ks) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // dp[D] | ds[REP][R] | comb[REP][H]
    float* dp = lds;
    float* ds = lds + D;
    float* comb = ds + ((REP * R + 3) / 4) * 4;
    const int mem = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int NW = BWD_THREADS / 64;
    const float* vb = v + (int64_t)mem * R * H;
    const VT* Vb = V + (int64_t)mem * R * D;
    const int D4 = D / 4;

    for (int j = 0; j < rep; ++j) {
        const int q = mem * rep + j;
        __syncthreads();
        for (int d = threadIdx.x; d < D; d += BWD_THREADS) dp[d] = dpooled[(int64_t)q * D + d];
        __syncthreads();
        // datt[r] = <dpooled[q], V[mem,r]>
        float* dsj = ds + j * R;
        for (int r = wave; r < R; r += NW) {
            float acc = 0.f;
#pragma unroll 8
            for (int du = lane; du < D4; du += 64) {
                const float4 x = VMem<VT>::load_f4(Vb + (int64_t)r * D, du);
                const float4 g = reinterpret_cast<const float4*>(dp)[du];
                acc += x.x * g.x + x.y * g.y + x.z * g.z + x.w * g.w;
            }
            acc = wave_sum(acc);
            if (lane == 0) dsj[r] = acc;
        }
        __syncthreads();
        // softmax backward: ds = att * (datt - sum(att*datt))
        if (wave == 0) {
            float dot = 0.f;
            for (int r = lane; r < R; r += 64) dot += att[(int64_t)q * R + r] * dsj[r];
            dot = wave_sum(dot);
            float tot = 0.f;
            for (int r = lane; r < R; r += 64) {
                const float g = att[(int64_t)q * R + r] * (dsj[r] - dot);
                dsj[r] = g;
                tot += g;
            }
            tot = wave_sum(tot);
            if (lane == 0) part_db[q] = tot;
        }
    }
    __syncthreads();

    const int H4 = H / 4;
    const int half = threadIdx.x / (BWD_THREADS / 2), tcol = threadIdx.x % (BWD_THREADS / 2);
    for (int hu0 = 0; hu0 < H4; hu0 += BWD_THREADS / 2) {
        const int hu = hu0 + tcol;
        const bool live = hu < H4;
        float4 ww = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 qj[REP], S[REP];
        if (live) ww = reinterpret_cast<const float4*>(w)[hu];
#pragma unroll
        for (int j = 0; j < REP; ++j) {
            S[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            qj[j] = (live && j < rep) ? reinterpret_cast<const float4*>(qv + (int64_t)(mem * rep + j) * H)[hu]
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (live) {
#pragma unroll 2
            for (int r = half; r < R; r += 2) {
                const float4 x = reinterpret_cast<const float4*>(vb + (int64_t)r * H)[hu];
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int j = 0; j < REP; ++j) {
                    if (j < rep) {
                        const float d = ds[j * R + r];
                        float4 g = make_float4(d, d, d, d);
                        if constexpr (KP == KEEP_SEEDED) {
                            const KeepSeed sd = keep_seed_of(ks...);
                            const uchar4 m =
                                keep_uchar4(keep_word4(sd.key, sd.word0 + ((uint64_t)(mem * rep + j) * R + r) * H4 + hu, sd.thr));
                            g.x *= m.x * inv_keep; g.y *= m.y * inv_keep; g.z *= m.z * inv_keep; g.w *= m.w * inv_keep;
                        } else if (keepmask != nullptr) {
                            const uchar4 m =
                                reinterpret_cast<const uchar4*>(keepmask + ((int64_t)(mem * rep + j) * R + r) * H)[hu];
                            g.x *= m.x * inv_keep; g.y *= m.y * inv_keep; g.z *= m.z * inv_keep; g.w *= m.w * inv_keep;
                        }
                        S[j].x += g.x * x.x; S[j].y += g.y * x.y; S[j].z += g.z * x.z; S[j].w += g.w * x.w;
                        acc.x += g.x * qj[j].x * ww.x; acc.y += g.y * qj[j].y * ww.y;
                        acc.z += g.z * qj[j].z * ww.z; acc.w += g.w * qj[j].w * ww.w;
                    }
                }
                reinterpret_cast<float4*>(dv + ((int64_t)mem * R + r) * H)[hu] = acc;
            }
        }
        // odd-row partial sums -> LDS, the even-row thread of the same column finishes (fixed order)
        __syncthreads();
        if (live && half == 1) {
#pragma unroll
            for (int j = 0; j < REP; ++j)
                if (j < rep) reinterpret_cast<float4*>(comb + (size_t)j * H)[hu] = S[j];
        }
        __syncthreads();
        if (live && half == 0) {
#pragma unroll
            for (int j = 0; j < REP; ++j) {
                if (j < rep) {
                    const float4 o = reinterpret_cast<const float4*>(comb + (size_t)j * H)[hu];
                    const float4 t = make_float4(S[j].x + o.x, S[j].y + o.y, S[j].z + o.z, S[j].w + o.w);
                    const int64_t q = (int64_t)mem * rep + j;
                    reinterpret_cast<float4*>(dqv + q * H)[hu] = make_float4(t.x * ww.x, t.y * ww.y, t.z * ww.z, t.w * ww.w);
                    reinterpret_cast<float4*>(part_dw + q * H)[hu] =
                        make_float4(t.x * qj[j].x, t.y * qj[j].y, t.z * qj[j].z, t.w * qj[j].w);
                }
            }
        }
    }
}

// The same backward for the models' shapes (D == 2048, H == 1024, R <= 40; 1 or 5 queries per memory), restructured around loads in
// flight like the forward: the generic kernel walks its queries one after the other (load dpooled[q], then one V row
// per wave at a time: REP x ~6 dependent memory latencies with two workgroups per CU), and its last phase keeps two
// rows per thread in flight.  Here dpooled of ALL queries of the memory sits in LDS, a wave reads each of its V rows
// ONCE (two rows in flight) and scores it against the REP queries, the REP softmax backwards run in REP waves, and
// the dv phase keeps four rows (+ their REP mask words) per thread in flight.  Same per-lane summation order.
// DD = 1024 (REP 5 only is dispatched): the adapted memory of the pre-training model; D4 is then half a workgroup, so
// half of the threads stage dpooled and a wave's V row is 4 float4 per lane instead of 8.
// Its phases 1-3, the score gradient of the REP queries of memory blockIdx.x: dpooled staged in LDS, datt[j][r] =
// <dpooled[q0 + j], V[mem, r]> with two V rows per wave in flight, the softmax backward ds = att * (datt - sum(att * datt))
// in one wave per query.  lds: dp[REP][DD] | ds[REP][40].  ds of query q0 + j goes to g_out + j * g_ld (the ds rows in
// LDS themselves, or global memory), its sum to part_db; the caller synchronises before it reads them.
template <int REP, int DD, typename VT>
__device__ __forceinline__ void attn_bwd_ds_phases(const float* __restrict__ dpooled, const VT* __restrict__ V,
                                                   const float* __restrict__ att, float* lds, float* g_out, int g_ld,
                                                   float* __restrict__ part_db, int R) {
    constexpr int D = DD, D4 = D / 4, DL = D4 / 64, NW = BWD_THREADS / 64;
    static_assert(REP <= NW, "one softmax wave per query");
    static_assert(D4 <= BWD_THREADS && D4 % 64 == 0, "dpooled is staged with one float4 per thread");
    float* ds = lds + REP * D;
    const int mem = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q0 = (int64_t)mem * REP;
    f32x4v* dp4 = reinterpret_cast<f32x4v*>(lds);
    if (D4 == BWD_THREADS || threadIdx.x < D4) {      // D == 2048: D4 == BWD_THREADS, every thread
        const f32x4v* g4 = reinterpret_cast<const f32x4v*>(dpooled + q0 * D);
        f32x4v t[REP];
#pragma unroll
        for (int j = 0; j < REP; ++j) t[j] = g4[j * D4 + threadIdx.x];
#pragma unroll
        for (int j = 0; j < REP; ++j) dp4[j * D4 + threadIdx.x] = t[j];
    }
    __syncthreads();
    const VT* Vb = V + (int64_t)mem * R * D;
    for (int r0 = wave; r0 < R; r0 += 2 * NW) {
        const int rb = min(r0 + NW, R - 1);
        const bool okb = r0 + NW < R;
        typename VMem<VT>::Raw ra[DL], rbw[DL];
#pragma unroll
        for (int k = 0; k < DL; ++k) {
            ra[k] = VMem<VT>::load(Vb, (int64_t)r0 * D4 + lane + 64 * k);
            rbw[k] = VMem<VT>::load(Vb, (int64_t)rb * D4 + lane + 64 * k);
        }
#pragma unroll
        for (int j = 0; j < REP; ++j) {
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int k = 0; k < DL; ++k) {
                const f32x4v g = dp4[j * D4 + lane + 64 * k];
                const f32x4v xa = VMem<VT>::widen(ra[k]), xb = VMem<VT>::widen(rbw[k]);
                a += xa.x * g.x + xa.y * g.y + xa.z * g.z + xa.w * g.w;
                b += xb.x * g.x + xb.y * g.y + xb.z * g.z + xb.w * g.w;
            }
            a = wave_sum(a);
            b = wave_sum(b);
            if (lane == 0) {
                ds[j * 40 + r0] = a;
                if (okb) ds[j * 40 + rb] = b;
            }
        }
    }
    __syncthreads();
    // R <= 40 < 64: one lane per region
    if (wave < REP) {
        const int64_t q = q0 + wave;
        const float a = lane < R ? att[q * R + lane] : 0.f;
        const float d = lane < R ? ds[wave * 40 + lane] : 0.f;
        const float dot = wave_sum(a * d);
        const float g = a * (d - dot);
        if (lane < R) g_out[wave * g_ld + lane] = g;
        const float tot = wave_sum(g);
        if (lane == 0) part_db[q] = tot;
    }
}

template <int REP, int KP, int DD = 2048, typename VT = float, typename... KS>
__global__ __launch_bounds__(BWD_THREADS) void attn_pool_bwd_fast_kernel(
    const float* __restrict__ dpooled, const float* __restrict__ v, const float* __restrict__ qv,
    const VT* __restrict__ V, const float* __restrict__ att, const float* __restrict__ w,
    const uint8_t* __restrict__ keepmask, float inv_keep, float* __restrict__ dv, float* __restrict__ dqv,
    float* __restrict__ part_dw, float* __restrict__ part_db, int R, int H, KS... ks) {
    constexpr int D = DD, RB = 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];  // dp[REP][D] | ds[REP][40] | comb[REP][H]
    float* ds = lds + REP * D;
    float* comb = ds + REP * 40;
    const int mem = blockIdx.x;
    const int64_t q0 = (int64_t)mem * REP;
    attn_bwd_ds_phases<REP, DD, VT>(dpooled, V, att, lds, ds, 40, part_db, R);
    __syncthreads();

    const int H4 = H / 4;
    const int half = threadIdx.x / (BWD_THREADS / 2), tcol = threadIdx.x % (BWD_THREADS / 2);
    const f32x4v* vb4 = reinterpret_cast<const f32x4v*>(v + (int64_t)mem * R * H);
    const unsigned* mk4 = KP == KEEP_BYTES ? reinterpret_cast<const unsigned*>(keepmask + q0 * R * H) : nullptr;
    f32x4v* dv4 = reinterpret_cast<f32x4v*>(dv + (int64_t)mem * R * H);
    for (int hu0 = 0; hu0 < H4; hu0 += BWD_THREADS / 2) {       // H == 1024: one pass, every thread has a column
        const int hu = hu0 + tcol;
        const f32x4v ww = reinterpret_cast<const f32x4v*>(w)[hu];
        f32x4v qj[REP], S[REP];
#pragma unroll
        for (int j = 0; j < REP; ++j) {
            S[j] = (f32x4v)(0.f);
            qj[j] = reinterpret_cast<const f32x4v*>(qv + (q0 + j) * H)[hu];
        }
        for (int rb = half; rb < R; rb += 2 * RB) {
            f32x4v x[RB];
            unsigned m[RB][REP];
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                const int r = min(rb + 2 * i, R - 1);
                x[i] = vb4[(int64_t)r * H4 + hu];
                if (KP == KEEP_BYTES) {
#pragma unroll
                    for (int j = 0; j < REP; ++j) m[i][j] = mk4[((int64_t)j * R + r) * H4 + hu];
                }
                if constexpr (KP == KEEP_SEEDED) {
                    const KeepSeed sd = keep_seed_of(ks...);
#pragma unroll
                    for (int j = 0; j < REP; ++j)
                        m[i][j] = keep_word4(sd.key, sd.word0 + ((uint64_t)(q0 + j) * R + r) * H4 + hu, sd.thr);
                }
            }
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                const int r = rb + 2 * i;
                if (r >= R) break;                                      // workgroup-uniform per half; no barrier inside
                f32x4v acc = (f32x4v)(0.f);
#pragma unroll
                for (int j = 0; j < REP; ++j) {
                    const float d = ds[j * 40 + r];
                    f32x4v g = (f32x4v)(d);
                    if (KP != KEEP_NONE) {
                        const unsigned mm = m[i][j];
                        g.x *= (float)(mm & 0xFFu) * inv_keep; g.y *= (float)((mm >> 8) & 0xFFu) * inv_keep;
                        g.z *= (float)((mm >> 16) & 0xFFu) * inv_keep; g.w *= (float)(mm >> 24) * inv_keep;
                    }
                    S[j].x += g.x * x[i].x; S[j].y += g.y * x[i].y; S[j].z += g.z * x[i].z; S[j].w += g.w * x[i].w;
                    acc.x += g.x * qj[j].x * ww.x; acc.y += g.y * qj[j].y * ww.y;
                    acc.z += g.z * qj[j].z * ww.z; acc.w += g.w * qj[j].w * ww.w;
                }
                dv4[(int64_t)r * H4 + hu] = acc;
            }
        }
        // odd-row partial sums -> LDS, the even-row thread of the same column finishes (fixed order)
        __syncthreads();
        if (half == 1) {
#pragma unroll
            for (int j = 0; j < REP; ++j) reinterpret_cast<f32x4v*>(comb + (size_t)j * H)[hu] = S[j];
        }
        __syncthreads();
        if (half == 0) {
#pragma unroll
            for (int j = 0; j < REP; ++j) {
                const f32x4v o = reinterpret_cast<const f32x4v*>(comb + (size_t)j * H)[hu];
                const f32x4v t = S[j] + o;
                reinterpret_cast<f32x4v*>(dqv + (q0 + j) * H)[hu] = t * ww;
                reinterpret_cast<f32x4v*>(part_dw + (q0 + j) * H)[hu] = t * qj[j];
            }
        }
    }
}

// Phases 1-3 of attn_pool_bwd_fast_kernel<1, ., 2048> on their own (vqa_attn_pool_bwd_ds): the same attn_bwd_ds_phases, so
// ds and part_db hold the bits of that kernel.  The score gradient ds [B,R] leaves the CU instead of dv [B,R,H]: dv is
// ds[b,r] x (keep/keep_prob * qv * w), which the LayerNorm backward of v_linear_v forms in registers
// (layernorm.hip: ln_att_bwd_reg_kernel), so neither v nor the keep mask is read here.
template <typename VT>
__global__ __launch_bounds__(BWD_THREADS) void attn_pool_bwd_ds_kernel(const float* __restrict__ dpooled,
                                                                       const VT* __restrict__ V,
                                                                       const float* __restrict__ att,
                                                                       float* __restrict__ ds_out,
                                                                       float* __restrict__ part_db, int R) {
    __shared__ __attribute__((aligned(16))) float lds[2048 + 40];  // dp[D] | ds[40]
    attn_bwd_ds_phases<1, 2048, VT>(dpooled, V, att, lds, ds_out + (int64_t)blockIdx.x * R, R, part_db, R);
}

int g_attn_fast = 1;   // tuning / A-B switch (vqa_attn_set_fast)

// base address of a pooled memory whose lanes load four consecutive elements at once: 16 bytes of f32, 8 of bf16
template <typename VT>
inline bool v_aligned(const VT* V) { return (reinterpret_cast<uintptr_t>(V) & (4 * sizeof(VT) - 1)) == 0; }
template <typename VT>
constexpr bool v_is_f32() { return sizeof(VT) == sizeof(float); }

// Forward for one memory type.  The route is chosen from rep, the shape and alignments; the keep source picks the
// instantiation on it.  (Pointers, then the keep source, then the integers: the order in which the *_seeded entry points
// always checked.)
template <typename VT>
int attn_fwd_typed(const float* v, const float* qv, const VT* V, const int32_t* nb, const float* w, const float* bias,
                   const KeepSrc& keep, float* att, float* pooled, int B, int rep, int R, int H, int D, void* stream,
                   bool seeded_one_query) {
    VQA_REQUIRE(v && qv && V && nb && w && bias && att && pooled, VQA_ERR_ARG);
    VQA_REQUIRE(keep.err == VQA_OK, keep.err);
    VQA_REQUIRE(!(seeded_one_query && keep.is_seeded()) || rep == 1, VQA_ERR_UNSUPPORTED);      // vqa_attn_pool_fwd_seeded
    VQA_REQUIRE(rep >= 1 && rep <= 8, VQA_ERR_ARG);
    VQA_REQUIRE(B >= 0 && R > 0 && R <= MAX_R && H > 0 && D > 0, VQA_ERR_ARG);
    VQA_REQUIRE(H % 4 == 0 && D % 4 == 0, VQA_ERR_ALIGN);
    VQA_REQUIRE(vqa_aligned16(v) && v_aligned(V) && vqa_aligned16(pooled) && keep.words_ok(), VQA_ERR_ALIGN);
    if (B == 0) return VQA_OK;
    const uint8_t* keepmask = keep.mask;
    const float ik = keep.inv_keep();
    hipStream_t st = (hipStream_t)stream;
    const bool fast = g_attn_fast && (rep == 1 || rep == 5 || g_attn_fast > 1) && R <= 40 && H % 256 == 0 && H <= 1024 && D % 2048 == 0 && D <= 4096 &&
                      vqa_aligned16(qv) && vqa_aligned16(w);
    // the 1024-wide memory (v_adapt of the pre-training model, an f32 activation -- never the table): per-memory kernel
    // for rep 5 only; one query per memory at D 1024 (vlmap_answer_adapt's step) stays on the generic kernel
    const bool fast1024 = v_is_f32<VT>() && g_attn_fast && g_attn_fast != 3 && rep == 5 && R <= 40 && H == 1024 && D == 1024 &&
                          vqa_aligned16(qv) && vqa_aligned16(w);
    // the one fast kernel with the row `form` of the form table at <H / 256, D>, one workgroup per form.REP queries
    auto launch_form = [&](auto form, auto h4l, auto d) {
        typedef decltype(form) F;
        keep_dispatch(keep, [&](auto kp, auto... ks) {
            hipLaunchKernelGGL(
                (attn_pool_fwd_form_kernel<F, decltype(h4l)::value, decltype(d)::value, decltype(kp)::value, VT, decltype(ks)...>),
                dim3(B * rep / F::REP), dim3(FWD_THREADS), (size_t)F::REP * (H + 40) * sizeof(float), st, v, qv, V, nb, w, bias,
                keepmask, ik, att, pooled, R, rep, ks...);
        });
    };
    auto launch_form_shapes = [&](auto form) {
        int_dispatch<2048, 4096>(D, [&](auto d) { int_dispatch<1, 2, 3, 4>(H / 256, [&](auto h4l) { launch_form(form, h4l, d); }); });
    };
    if constexpr (v_is_f32<VT>()) {
        if (fast1024) {
            launch_form(FwdRepD1024{}, std::integral_constant<int, 4>{}, std::integral_constant<int, 1024>{});
            VQA_CHECK_LAUNCH();
            return VQA_OK;
        }
    }
    if (fast && rep == 5 && g_attn_fast != 3) {
        launch_form_shapes(FwdRep{});               // one workgroup per memory for the pre-training model's 5 queries per image
    } else if (fast) {
        launch_form_shapes(FwdFast{});
    } else {
        keep_dispatch_generic(keep, [&](auto kp, auto... ks) {
            hipLaunchKernelGGL((attn_pool_fwd_kernel<VT, decltype(kp)::value, decltype(ks)...>), dim3(B * rep), dim3(FWD_THREADS),
                               (size_t)(H + R) * sizeof(float), st, v, qv, V, nb, w, bias, keepmask, ik, att, pooled, R, H, D, rep,
                               ks...);
        });
    }
    VQA_CHECK_LAUNCH();
    return VQA_OK;
}

template <typename VT>
int attn_bwd_typed(const float* dpooled, const float* v, const float* qv, const VT* V, const float* att, const float* w,
                   const KeepSrc& keep, float* dv, float* dqv, float* part_dw, float* part_db, int B, int rep, int R, int H,
                   int D, void* stream, bool seeded_one_query) {
    VQA_REQUIRE(dpooled && v && qv && V && att && w && dv && dqv && part_dw && part_db, VQA_ERR_ARG);
    VQA_REQUIRE(keep.err == VQA_OK, keep.err);
    VQA_REQUIRE(!(seeded_one_query && keep.is_seeded()) || rep == 1, VQA_ERR_UNSUPPORTED);      // vqa_attn_pool_bwd_seeded
    VQA_REQUIRE(rep >= 1 && rep <= 8, VQA_ERR_ARG);
    VQA_REQUIRE(B >= 0 && R > 0 && R <= MAX_R && H > 0 && D > 0, VQA_ERR_ARG);
    VQA_REQUIRE(H % 4 == 0 && D % 4 == 0, VQA_ERR_ALIGN);
    VQA_REQUIRE(vqa_aligned16(v) && v_aligned(V) && vqa_aligned16(dv) && vqa_aligned16(dqv) &&
                    vqa_aligned16(part_dw) && vqa_aligned16(qv) && vqa_aligned16(w) && keep.words_ok(),
                VQA_ERR_ALIGN);
    if (B == 0) return VQA_OK;
    const uint8_t* keepmask = keep.mask;
    const float ik = keep.inv_keep();
    hipStream_t st = (hipStream_t)stream;
    auto lds_for = [&](int REPt) { return (size_t)(D + ((REPt * R + 3) / 4) * 4 + REPt * H) * sizeof(float); };
    VQA_REQUIRE(lds_for(rep == 1 ? 1 : rep <= 5 ? 5 : 8) <= 64 * 1024, VQA_ERR_UNSUPPORTED);
    // one workgroup per memory: one query at D 2048; the pre-training model's 5 queries at D 2048 and at D 1024 (the
    // 1024-wide memory; one query per memory at D 1024 stays on the generic kernel)
    const bool fast_shape = g_attn_fast && H == 1024 && R <= 40 && vqa_aligned16(dpooled);
    auto launch_fast = [&](auto rept, auto dd) -> int {
        keep_dispatch(keep, [&](auto kp, auto... ks) {
            hipLaunchKernelGGL(
                (attn_pool_bwd_fast_kernel<decltype(rept)::value, decltype(kp)::value, decltype(dd)::value, VT, decltype(ks)...>),
                dim3(B), dim3(BWD_THREADS), (size_t)(rep * D + rep * 40 + rep * H) * sizeof(float), st, dpooled, v, qv, V, att, w,
                keepmask, ik, dv, dqv, part_dw, part_db, R, H, ks...);
        });
        VQA_CHECK_LAUNCH();
        return VQA_OK;
    };
    std::integral_constant<int, 1> one;
    std::integral_constant<int, 5> five;
    std::integral_constant<int, 1024> d1024;
    std::integral_constant<int, 2048> d2048;
    if (fast_shape && rep == 1 && D == 2048) return launch_fast(one, d2048);
    // several queries per memory.  (D 1024 is the adapted memory, an f32 activation: a bf16 memory of that width takes the
    // generic kernel, as its forward does)
    if (fast_shape && rep == 5 && D == 2048) return launch_fast(five, d2048);
    if constexpr (v_is_f32<VT>()) {
        if (fast_shape && rep == 5 && D == 1024) return launch_fast(five, d1024);
    }
    if (rep > 1) {
        int_dispatch<5, 8>(rep <= 5 ? 5 : 8, [&](auto rt) {
            keep_dispatch_generic(keep, [&](auto kp, auto... ks) {
                hipLaunchKernelGGL((attn_pool_bwd_kernel<decltype(rt)::value, VT, decltype(kp)::value, decltype(ks)...>),
                                   dim3(B), dim3(BWD_THREADS), lds_for(decltype(rt)::value), st, dpooled, v, qv, V, att, w,
                                   keepmask, ik, dv, dqv, part_dw, part_db, R, H, D, rep, ks...);
            });
        });
        VQA_CHECK_LAUNCH();
        return VQA_OK;
    }
    keep_dispatch_generic(keep, [&](auto kp, auto... ks) {
        hipLaunchKernelGGL((attn_pool_bwd_kernel<1, VT, decltype(kp)::value, decltype(ks)...>), dim3(B), dim3(BWD_THREADS),
                           lds_for(1), st, dpooled, v, qv, V, att, w, keepmask, ik, dv, dqv, part_dw, part_db, R, H, D, rep, ks...);
    });
    VQA_CHECK_LAUNCH();
    return VQA_OK;
}

}  // namespace

extern "C" int vqa_attn_set_fast(int on) {
    // 0 generic; 1 (default) fast kernel for one query per memory and the per-memory kernel for rep 5; 2 per-query fast
    // kernel for the other reps as well; 3 per-query fast kernel for every rep (A/B of the per-memory kernel)
    g_attn_fast = on;
    return VQA_OK;
}

int vqa_attn_fwd_run(const float* v, const float* qv, const void* V, bool v_bf16, const int32_t* nb, const float* w,
                     const float* bias, const KeepSrc& keep, float* att, float* pooled, int B, int rep, int R, int H, int D,
                     void* stream, bool seeded_one_query) {
    if (v_bf16)
        return attn_fwd_typed(v, qv, static_cast<const uint16_t*>(V), nb, w, bias, keep, att, pooled, B, rep, R, H, D, stream,
                              seeded_one_query);
    return attn_fwd_typed(v, qv, static_cast<const float*>(V), nb, w, bias, keep, att, pooled, B, rep, R, H, D, stream,
                          seeded_one_query);
}

int vqa_attn_bwd_run(const float* dpooled, const float* v, const float* qv, const void* V, bool v_bf16, const float* att,
                     const float* w, const KeepSrc& keep, float* dv, float* dqv, float* part_dw, float* part_db, int B, int rep,
                     int R, int H, int D, void* stream, bool seeded_one_query) {
    if (v_bf16)
        return attn_bwd_typed(dpooled, v, qv, static_cast<const uint16_t*>(V), att, w, keep, dv, dqv, part_dw, part_db, B, rep, R,
                              H, D, stream, seeded_one_query);
    return attn_bwd_typed(dpooled, v, qv, static_cast<const float*>(V), att, w, keep, dv, dqv, part_dw, part_db, B, rep, R, H, D,
                          stream, seeded_one_query);
}

extern "C" int vqa_attn_pool_fwd(const float* v, const float* qv, const float* V, const int32_t* nb, const float* w,
                                 const float* bias, const uint8_t* keepmask, float keep_prob, float* att,
                                 float* pooled, int B, int R, int H, int D, void* stream) {
    return vqa_attn_pool_fwd_rep(v, qv, V, nb, w, bias, keepmask, keep_prob, att, pooled, B, 1, R, H, D, stream);
}

extern "C" int vqa_attn_pool_fwd_rep(const float* v, const float* qv, const float* V, const int32_t* nb,
                                     const float* w, const float* bias, const uint8_t* keepmask, float keep_prob,
                                     float* att, float* pooled, int B, int rep, int R, int H, int D, void* stream) {
    return vqa_attn_fwd_run(v, qv, V, false, nb, w, bias, KeepSrc::bytes(keepmask, keep_prob), att, pooled, B, rep, R, H, D, stream);
}

// bf16 memory (raw patterns), one query per memory: the kernels vqa_attn_pool_fwd selects for the shape, V loads 8 bytes wide
extern "C" int vqa_attn_pool_fwd_v16(const float* v, const float* qv, const uint16_t* V, const int32_t* nb, const float* w,
                                     const float* bias, const uint8_t* keepmask, float keep_prob, float* att,
                                     float* pooled, int B, int R, int H, int D, void* stream) {
    return vqa_attn_fwd_run(v, qv, V, true, nb, w, bias, KeepSrc::bytes(keepmask, keep_prob), att, pooled, B, 1, R, H, D, stream);
}

// The keep bits of the score's dropout computed in the kernel instead of loaded: the kernels the explicit entry points
// select for the shape (same route selection), instantiated with KEEP_SEEDED.  These two entry points keep the contract
// they were published with: one query per memory, rep != 1 -> VQA_ERR_UNSUPPORTED.  Several queries per memory:
// vqa_attn_pool_fwd_rep_seeded / vqa_attn_pool_bwd_rep_seeded below.
extern "C" int vqa_attn_pool_fwd_seeded(const float* v, const float* qv, const void* V, int v_bf16, const int32_t* nb,
                                        const float* w, const float* bias, uint64_t seed, uint64_t offset, float keep_prob,
                                        float* att, float* pooled, int B, int rep, int R, int H, int D, void* stream) {
    return vqa_attn_fwd_run(v, qv, V, v_bf16 != 0, nb, w, bias, KeepSrc::seeded(seed, offset, H, keep_prob), att, pooled, B, rep,
                            R, H, D, stream, true);
}

// vqa_attn_pool_fwd_rep with the keep bits computed: rep queries per memory, the mask of query q = m * rep + j at stream
// position offset + q * R * H, as in the explicit [B * rep, R, H] mask
extern "C" int vqa_attn_pool_fwd_rep_seeded(const float* v, const float* qv, const float* V, const int32_t* nb, const float* w,
                                            const float* bias, uint64_t seed, uint64_t offset, float keep_prob, float* att,
                                            float* pooled, int B, int rep, int R, int H, int D, void* stream) {
    return vqa_attn_fwd_run(v, qv, V, false, nb, w, bias, KeepSrc::seeded(seed, offset, H, keep_prob), att, pooled, B, rep, R, H,
                            D, stream);
}

extern "C" int vqa_attn_pool_bwd(const float* dpooled, const float* v, const float* qv, const float* V,
                                 const float* att, const float* w, const uint8_t* keepmask, float keep_prob, float* dv,
                                 float* dqv, float* part_dw, float* part_db, int B, int R, int H, int D, void* stream) {
    return vqa_attn_pool_bwd_rep(dpooled, v, qv, V, att, w, keepmask, keep_prob, dv, dqv, part_dw, part_db, B, 1, R, H,
                                 D, stream);
}

extern "C" int vqa_attn_pool_bwd_rep(const float* dpooled, const float* v, const float* qv, const float* V,
                                     const float* att, const float* w, const uint8_t* keepmask, float keep_prob,
                                     float* dv, float* dqv, float* part_dw, float* part_db, int B, int rep, int R,
                                     int H, int D, void* stream) {
    return vqa_attn_bwd_run(dpooled, v, qv, V, false, att, w, KeepSrc::bytes(keepmask, keep_prob), dv, dqv, part_dw, part_db, B,
                            rep, R, H, D, stream);
}

extern "C" int vqa_attn_pool_bwd_v16(const float* dpooled, const float* v, const float* qv, const uint16_t* V,
                                     const float* att, const float* w, const uint8_t* keepmask, float keep_prob, float* dv,
                                     float* dqv, float* part_dw, float* part_db, int B, int R, int H, int D, void* stream) {
    return vqa_attn_bwd_run(dpooled, v, qv, V, true, att, w, KeepSrc::bytes(keepmask, keep_prob), dv, dqv, part_dw, part_db, B, 1,
                            R, H, D, stream);
}

extern "C" int vqa_attn_pool_bwd_seeded(const float* dpooled, const float* v, const float* qv, const void* V, int v_bf16,
                                        const float* att, const float* w, uint64_t seed, uint64_t offset, float keep_prob,
                                        float* dv, float* dqv, float* part_dw, float* part_db, int B, int rep, int R, int H,
                                        int D, void* stream) {
    return vqa_attn_bwd_run(dpooled, v, qv, V, v_bf16 != 0, att, w, KeepSrc::seeded(seed, offset, H, keep_prob), dv, dqv, part_dw,
                            part_db, B, rep, R, H, D, stream, true);
}

extern "C" int vqa_attn_pool_bwd_rep_seeded(const float* dpooled, const float* v, const float* qv, const float* V,
                                            const float* att, const float* w, uint64_t seed, uint64_t offset, float keep_prob,
                                            float* dv, float* dqv, float* part_dw, float* part_db, int B, int rep, int R, int H,
                                            int D, void* stream) {
    return vqa_attn_bwd_run(dpooled, v, qv, V, false, att, w, KeepSrc::seeded(seed, offset, H, keep_prob), dv, dqv, part_dw,
                            part_db, B, rep, R, H, D, stream);
}

// The chain v_linear_v's LayerNorm -> attention score and its gradient at the one shape of the register-resident
// LayerNorm kernels and the fast attention kernels: one query per memory, 36 regions, 1024 hidden units, 2048 features.
extern "C" int vqa_vtail_supported(int rep, int R, int H, int D) {
    return (rep == 1 && R == 36 && H == 1024 && D == 2048) ? 1 : 0;
}

extern "C" int vqa_attn_pool_bwd_ds(const float* dpooled, const float* V, const float* att, float* ds, float* part_db,
                                    int B, int rep, int R, int H, int D, void* stream) {
    VQA_REQUIRE(dpooled && V && att && ds && part_db && B >= 0, VQA_ERR_ARG);
    VQA_REQUIRE(vqa_vtail_supported(rep, R, H, D), VQA_ERR_UNSUPPORTED);
    VQA_REQUIRE(vqa_aligned16(dpooled) && vqa_aligned16(V), VQA_ERR_ALIGN);
    if (B == 0) return VQA_OK;
    hipLaunchKernelGGL(attn_pool_bwd_ds_kernel<float>, dim3(B), dim3(BWD_THREADS), 0, (hipStream_t)stream, dpooled, V, att, ds,
                       part_db, R);
    VQA_CHECK_LAUNCH();
    return VQA_OK;
}

extern "C" int vqa_attn_pool_bwd_ds_v16(const float* dpooled, const uint16_t* V, const float* att, float* ds, float* part_db,
                                        int B, int rep, int R, int H, int D, void* stream) {
    VQA_REQUIRE(dpooled && V && att && ds && part_db && B >= 0, VQA_ERR_ARG);
    VQA_REQUIRE(vqa_vtail_supported(rep, R, H, D), VQA_ERR_UNSUPPORTED);
    VQA_REQUIRE(vqa_aligned16(dpooled) && v_aligned(V), VQA_ERR_ALIGN);
    if (B == 0) return VQA_OK;
    hipLaunchKernelGGL(attn_pool_bwd_ds_kernel<uint16_t>, dim3(B), dim3(BWD_THREADS), 0, (hipStream_t)stream, dpooled, V, att,
                       ds, part_db, R);
    VQA_CHECK_LAUNCH();
    return VQA_OK;
}
