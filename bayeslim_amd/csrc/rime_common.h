// rime_common.h -- shared host-side helpers of librime_hip.so (not part of the public ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include "../../include/rime_hip.h"

namespace rime {

extern char g_last_error[256];

// Call after launching: maps a failed launch to RIME_ELAUNCH and records the HIP message.
inline int check_launch()
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) return RIME_OK;
    std::snprintf(g_last_error, sizeof(g_last_error), "%s", hipGetErrorString(e));
    return RIME_ELAUNCH;
}

// The real working types of the C ABI: whether dtype names one, and its size in bytes (8 for anything but RIME_F32).
inline bool real_dtype_ok(int dtype) { return dtype == RIME_F32 || dtype == RIME_F64; }
inline int real_bytes(int dtype) { return dtype == RIME_F32 ? 4 : 8; }

// ---- host: from the run-time arguments of an entry point to the template arguments of its kernels ----
inline hipStream_t as_stream(void* stream) { return reinterpret_cast<hipStream_t>(stream); }

// f(float{}) for RIME_F32, f(double{}) for RIME_F64, and what f returns; RIME_EINVAL for any other dtype, f not called.
// Inside f: `using T = decltype(t);`
template <class F>
inline int with_real(int dtype, F&& f)
{
    if (dtype == RIME_F32) return f(float{});
    if (dtype == RIME_F64) return f(double{});
    return RIME_EINVAL;
}

// f(std::true_type) or f(std::false_type): a run-time flag as a template argument of the kernel f launches
template <class F>
inline void with_bool(bool flag, F&& f)
{
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}

// an int as an argument of a generic lambda: the cases of a switch over a run-time count call go(int_c<4>{})
template <int N> using int_c = std::integral_constant<int, N>;

// Reads of matrix-core results by the vector ALU.  hipcc (ROCm 7.2) places the wait states of the ISA hazard table
// between an MFMA and the first VALU read of its destination.  Observed on gfx950 (round 2, complex-psky backward of
// the diagonal fringe blocks at 393 216 pixels): when that first reader was a PACKED f32 op (v_pk_fma_f32 with op_sel,
// the compiler's fusion of two accumulation chains) sitting at exactly that distance, its low half sporadically saw a
// stale accumulator (wrong imaginary-plane gradients in a few hundred of 12 288 pixel tiles, different from run to run;
// the high half -- the real plane -- was always right).  Epilogues that read accumulators therefore start with 16 more
// wait states, fenced so that the scheduler keeps them between the last MFMA and the reads.
#if defined(RIME_NO_SETTLE)          /* lab: measure what the margin costs */
#define RIME_MFMA_SETTLE() do { } while (0)
#else
#define RIME_MFMA_SETTLE()                                   \
    do {                                                     \
        __builtin_amdgcn_sched_barrier(0);                   \
        asm volatile("s_nop 15" ::: "memory");               \
        __builtin_amdgcn_sched_barrier(0);                   \
    } while (0)
#endif

template <typename T> __device__ __forceinline__ T tfma(T a, T b, T c);
template <> __device__ __forceinline__ float tfma<float>(float a, float b, float c) { return fmaf(a, b, c); }
template <> __device__ __forceinline__ double tfma<double>(double a, double b, double c) { return fma(a, b, c); }

} // namespace rime
