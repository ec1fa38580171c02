// Shared helpers for the gfx950 kernels of libvqahot.so.  Device code is written
// for CDNA4 only: wave = 64 lanes, 256-thread workgroups unless stated.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/vqa_hot.h"

#define VQA_WAVE 64

#define VQA_CHECK_LAUNCH()                                   \
    do {                                                     \
        hipError_t e__ = hipGetLastError();                  \
        if (e__ != hipSuccess) return VQA_ERR_LAUNCH;        \
    } while (0)

#define VQA_REQUIRE(cond, code) \
    do {                        \
        if (!(cond)) return (code); \
    } while (0)

// Measurement / trace scope around a launch group (csrc/probe.hip): HIP events on `st` when the label is probed, a roctx
// range when ranges are on.  Costs one branch when neither is.
int vqa_probe_begin(const char* label, hipStream_t st, void** handle);
void vqa_probe_end(int flags, hipStream_t st, void* handle);
struct ProbeScope {
    hipStream_t st;
    void* handle = nullptr;
    int flags;
    ProbeScope(const char* label, hipStream_t s) : st(s) { flags = vqa_probe_begin(label, s, &handle); }
    ~ProbeScope() {
        if (flags) vqa_probe_end(flags, st, handle);
    }
    ProbeScope(const ProbeScope&) = delete;
    ProbeScope& operator=(const ProbeScope&) = delete;
};

// early return of a host composition on the first failing call
#define TRY(x)                           \
    do {                                 \
        int rc__ = (x);                  \
        if (rc__ != VQA_OK) return rc__; \
    } while (0)

static inline int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

// row stride of the time-major GRU inputs (x_tm): W word-vector columns, the constant 1 (its row of the x-part weight
// gradient is the bias gradient), zero padding to 16 bytes
static inline int64_t x_stride(int64_t W) { return ((W + 1 + 3) / 4) * 4; }

static inline bool vqa_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// integer tuning override from the environment; callers keep the value in a function-local static (read once)
static inline int vqa_env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Block-wide sum for 256..1024-thread blocks; red must hold >= 16 floats.  All
// threads get the result.
__device__ __forceinline__ float block_sum(float v, float* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}

// ------------------------------------------------------------------ dropout keep bits
// Counter-based generator (splitmix64 finaliser on seed ^ counter): the keep bit of stream position p depends only on
// (seed, p), so vqa_dropout_mask, the forward and the backward produce identical bits, and a kernel that consumes a
// mask can compute the bits it would otherwise load (the *_seeded entry points).
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// one 64-bit hash serves the four positions of an aligned group (16-bit uniforms: keep probabilities resolve to
// 1.5e-5): the generator, not the 1 byte per element it writes, bounded the kernel at 1.3 TB/s with a hash per position
__host__ __device__ __forceinline__ unsigned keep_thr(float keep) {
    const float t = keep * 65536.0f;
    return t <= 0.f ? 0u : (t >= 65536.0f ? 65536u : (unsigned)t);
}
__device__ __forceinline__ unsigned keep_bit(uint64_t key, uint64_t pos, unsigned thr) {
    const uint64_t r = mix64(key ^ (pos >> 2));
    return ((unsigned)(r >> (16 * (pos & 3))) & 0xFFFFu) < thr ? 1u : 0u;
}
// the four mask bytes (0/1, position 4 * word_index in the low byte) of stream positions 4 * word_index .. + 3: the
// 4-byte word vqa_dropout_mask writes there, and the word a consuming kernel loads from a mask whose element 0 sits at a
// stream position that is a multiple of 4
__device__ __forceinline__ unsigned keep_word4(uint64_t key, uint64_t word_index, unsigned thr) {
    const uint64_t r = mix64(key ^ word_index);
    unsigned v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) v |= ((((unsigned)(r >> (16 * b))) & 0xFFFFu) < thr ? 1u : 0u) << (8 * b);
    return v;
}

__device__ __forceinline__ uchar4 keep_uchar4(unsigned w) {      // the word as a kernel that loads uchar4 sees it
    return make_uchar4((unsigned char)(w & 0xFFu), (unsigned char)((w >> 8) & 0xFFu), (unsigned char)((w >> 16) & 0xFFu),
                       (unsigned char)(w >> 24));
}

// Where a kernel's keep factors come from: nowhere (no dropout), a uint8 mask in memory, or the stream itself.
// (The generic kernels decide between the first two at run time, by the mask pointer: their KEEP_BYTES covers both.)
enum KeepPolicy { KEEP_NONE = 0, KEEP_BYTES = 1, KEEP_SEEDED = 2 };
// The by-value argument of a KEEP_SEEDED instantiation: key = mix64(seed), word0 = the word index (stream position / 4)
// of the site's element 0, thr = keep_thr(keep_prob).  Kernels take it as a trailing parameter pack, `KS... ks`, that is
// empty for the other two policies, so those instantiations keep the argument list they had.
struct KeepSeed { uint64_t key, word0; unsigned thr; };
static inline KeepSeed keep_seed_make(uint64_t seed, uint64_t offset, float keep_prob) {
    return KeepSeed{mix64(seed), offset >> 2, keep_thr(keep_prob)};
}
__device__ __forceinline__ KeepSeed keep_seed_of() { return KeepSeed{0, 0, 0}; }
__device__ __forceinline__ KeepSeed keep_seed_of(KeepSeed s) { return s; }

// The keep source of one dropout site, as the host passes it to a launch function: no dropout, a uint8 mask, or the
// (seed, offset) stream.  The two makers are the one place the source's own arguments are checked; `err` is what the
// entry point returns for a source that failed them (a launch function checks it after its pointer checks).
struct KeepSrc {
    KeepPolicy policy = KEEP_NONE;
    const uint8_t* mask = nullptr;      // KEEP_BYTES
    KeepSeed sd = {0, 0, 0};            // KEEP_SEEDED
    float keep_prob = 1.f;
    int err = VQA_OK;

    // mask NULL: no dropout (keep_prob is not looked at)
    static KeepSrc bytes(const uint8_t* mask, float keep_prob) {
        KeepSrc k;
        if (mask == nullptr) return k;
        k.policy = KEEP_BYTES, k.mask = mask, k.keep_prob = keep_prob;
        if (!(keep_prob > 0.f)) k.err = VQA_ERR_ARG;
        return k;
    }
    // offset: stream position of the site's element 0; row_len: the site's row length.  Both multiples of 4, so a
    // kernel's 4-byte mask word is one word of the stream
    static KeepSrc seeded(uint64_t seed, uint64_t offset, int64_t row_len, float keep_prob) {
        KeepSrc k;
        k.policy = KEEP_SEEDED, k.sd = keep_seed_make(seed, offset, keep_prob), k.keep_prob = keep_prob;
        if (!(keep_prob > 0.f)) k.err = VQA_ERR_ARG;
        else if ((offset & 3u) != 0 || row_len % 4 != 0) k.err = VQA_ERR_ALIGN;
        return k;
    }
    bool is_seeded() const { return policy == KEEP_SEEDED; }
    float inv_keep() const { return policy == KEEP_NONE ? 1.f : 1.f / keep_prob; }
    // the kernels that read a mask four bytes at a time can take it (no mask: yes)
    bool words_ok() const { return (reinterpret_cast<uintptr_t>(mask) & 3u) == 0; }
};

// fn(std::integral_constant<int, V>) for the V of the list that equals v; false (and no call) when none does
template <int... Vs, typename F>
inline bool int_dispatch(int v, F&& fn) {
    return ((v == Vs ? (fn(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
// fn(policy tag, trailing by-value kernel arguments...): the KeepPolicy template argument of a kernel and its `KS... ks`
// pack from a KeepSrc.  Three policies for the kernels that are instantiated once per policy ...
template <typename F>
inline void keep_dispatch(const KeepSrc& k, F&& fn) {
    if (k.policy == KEEP_SEEDED) fn(std::integral_constant<int, KEEP_SEEDED>{}, k.sd);
    else if (k.policy == KEEP_BYTES) fn(std::integral_constant<int, KEEP_BYTES>{});
    else fn(std::integral_constant<int, KEEP_NONE>{});
}
// ... two for the generic kernels, whose KEEP_BYTES instantiation decides "no mask" at run time by the mask pointer
template <typename F>
inline void keep_dispatch_generic(const KeepSrc& k, F&& fn) {
    if (k.policy == KEEP_SEEDED) fn(std::integral_constant<int, KEEP_SEEDED>{}, k.sd);
    else fn(std::integral_constant<int, KEEP_BYTES>{});
}

__device__ __forceinline__ float mul_rounded(float a, float b) {      // a product that no later add absorbs into an fma
#pragma clang fp contract(off)
    return a * b;
}

__device__ __forceinline__ float sigmoidf_stable(float x) {
    // same value as the oracle's piecewise logistic to rounding
    if (x >= 0.f) return 1.f / (1.f + expf(-x));
    const float e = expf(x);
    return e / (1.f + e);
}
