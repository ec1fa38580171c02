// Shared helpers for the gfx950 kernels of libvqahot.so.  Device code is written
// for CDNA4 only: wave = 64 lanes, 256-thread workgroups unless stated.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

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

__device__ __forceinline__ float sigmoidf_stable(float x) {
    // same value as the oracle's piecewise logistic to rounding
    if (x >= 0.f) return 1.f / (1.f + expf(-x));
    const float e = expf(x);
    return e / (1.f + e);
}
