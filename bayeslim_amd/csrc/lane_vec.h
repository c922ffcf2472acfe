// lane_vec.h -- what the vector-ALU kernels share of a lane's 16-byte accesses and of the wave sum: the 16-byte vector of a real
// type, its packing, the alignment test, the two lane layouts (lbfgs.hip and hmc.hip the strided one, lstbin.hip the contiguous
// rows; hmat.hip takes the vector and its unpacking for a load of its own) and the butterfly.  Everything here is force-inlined
// or constexpr: a kernel that uses it assembles to the code object it would with the text written out in place.
//
// Both layouts rest on one rule.  A vector whose accesses all fall on 16-byte boundaries is read and written with 16-byte
// accesses; any other takes element accesses of the SAME elements from and into the SAME registers.  The caller decides which
// (`vec`), by a test that is uniform across the wave at the least, so the arithmetic, its order and hence every bit of the
// result do not depend on alignment, and there is no misaligned vector access.
//
// Strided layout (lane_load / lane_store; lbfgs.hip, hmc.hip): a lane holds GROUPS 16-byte groups of every vector it touches,
// THREADS groups apart, so a wave's accesses of one group index are contiguous: E = GROUPS * W elements per lane,
// SPAN = THREADS * E elements per work-group and chunk.  The vectors are contiguous and aligned to sizeof(T) only; `vec` is
// aligned16(base): the chunk start and the group offsets are multiples of W, so every group of an aligned base is aligned.
// Contiguous-row layout (row_load / row_store; lstbin.hip): a lane holds N consecutive elements from element e on; `vec` says
// that e is a multiple of W off a 16-byte aligned base and that all N are valid.
#pragma once
#include "rime_common.h"

namespace rime {

template <typename T> struct Vec16;                      // the 16-byte vector of T and its width in elements
template <> struct Vec16<float>  { using type = float4;  static constexpr int W = 4; };
template <> struct Vec16<double> { using type = double2; static constexpr int W = 2; };

__device__ __forceinline__ void unpack16(const float4& q, float (&x)[4]) { x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w; }
__device__ __forceinline__ void unpack16(const double2& q, double (&x)[2]) { x[0] = q.x; x[1] = q.y; }
__device__ __forceinline__ float4 pack16(const float (&x)[4]) { return float4{x[0], x[1], x[2], x[3]}; }
__device__ __forceinline__ double2 pack16(const double (&x)[2]) { return double2{x[0], x[1]}; }

__host__ __device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<unsigned long long>(p) & 15ull) == 0; }

// the sum over the 64 lanes of a wave, in every lane: partners 32, 16, ..., 1 apart, in that order.  hmat.hip and chisq.hip
// write the same loop out: through this call the compiler allocates hmat's registers and orders chisq's prologue differently
template <typename T>
__device__ __forceinline__ T wave_sum(T x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// the GROUPS * W elements of this lane of the chunk starting at c0: group g covers c0 + (g * THREADS + tid) * W ... + W - 1;
// elements at or beyond N read as 0 and are not written
template <typename T, int THREADS, int GROUPS>
__device__ __forceinline__ void lane_load(const T* p, long long c0, long long N, bool vec, T (&x)[GROUPS * Vec16<T>::W])
{
    constexpr int W = Vec16<T>::W;
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) {
        const long long e = c0 + (long long)(g * THREADS + (int)threadIdx.x) * W;
        T t[W];
        if (vec && e + W <= N) {
            unpack16(*reinterpret_cast<const typename Vec16<T>::type*>(p + e), t);
        } else {
#pragma unroll
            for (int i = 0; i < W; ++i) t[i] = (e + i < N) ? p[e + i] : (T)0;
        }
#pragma unroll
        for (int i = 0; i < W; ++i) x[g * W + i] = t[i];
    }
}

template <typename T, int THREADS, int GROUPS>
__device__ __forceinline__ void lane_store(T* p, long long c0, long long N, bool vec, const T (&x)[GROUPS * Vec16<T>::W])
{
    constexpr int W = Vec16<T>::W;
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) {
        const long long e = c0 + (long long)(g * THREADS + (int)threadIdx.x) * W;
        T t[W];
#pragma unroll
        for (int i = 0; i < W; ++i) t[i] = x[g * W + i];
        if (vec && e + W <= N) {
            *reinterpret_cast<typename Vec16<T>::type*>(p + e) = pack16(t);
        } else {
#pragma unroll
            for (int i = 0; i < W; ++i)
                if (e + i < N) p[e + i] = t[i];
        }
    }
}

// N reals (N a multiple of W) starting at element e; those at or beyond nvalid read as 0 and are not written
template <typename T, int N>
__device__ __forceinline__ void row_load(const T* p, size_t e, int nvalid, bool vec, T (&x)[N])
{
    constexpr int W = Vec16<T>::W;
#pragma unroll
    for (int g = 0; g < N / W; ++g) {
        T t[W];
        if (vec) {
            unpack16(*reinterpret_cast<const typename Vec16<T>::type*>(p + e + g * W), t);
        } else {
#pragma unroll
            for (int i = 0; i < W; ++i) t[i] = (g * W + i < nvalid) ? p[e + g * W + i] : (T)0;
        }
#pragma unroll
        for (int i = 0; i < W; ++i) x[g * W + i] = t[i];
    }
}

template <typename T, int N>
__device__ __forceinline__ void row_store(T* p, size_t e, int nvalid, bool vec, const T (&x)[N])
{
    constexpr int W = Vec16<T>::W;
#pragma unroll
    for (int g = 0; g < N / W; ++g) {
        T t[W];
#pragma unroll
        for (int i = 0; i < W; ++i) t[i] = x[g * W + i];
        if (vec) {
            *reinterpret_cast<typename Vec16<T>::type*>(p + e + g * W) = pack16(t);
        } else {
#pragma unroll
            for (int i = 0; i < W; ++i)
                if (g * W + i < nvalid) p[e + g * W + i] = t[i];
        }
    }
}

// chunks of N elements of the strided layout: work-group spans of `threads` lanes with `bytes` bytes each
inline long long lane_chunks(long long N, int dtype, int threads, int bytes)
{
    const long long span = (long long)threads * (bytes / real_bytes(dtype));
    return (N + span - 1) / span;
}

} // namespace rime
