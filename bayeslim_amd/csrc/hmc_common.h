// hmc_common.h -- what the three leapfrog files share: hmc.hip (one stage with a diagonal mass), nuts.hip (the two halves of a tree
// leaf) and massmat.hip (a stage with a block-dense mass).  Device side: the geometry of a launch, the strided lane layout of
// lane_vec.h at that geometry, the per-lane chain of the kinetic energy and the whole second stage (hmc_final: the sum of the
// work-groups' partials).  Host side: the checks the entry points share (the bound of N, overlapping ranges, a flag that
// underflows in float32) and the workspace.  Everything on the device side is force-inlined or constexpr (lane_vec.h).  The sums
// of all three files are summed in ONE order: the chain of hmc_sumsq in T, the butterfly, the chunks of a work-group in the order
// b, b + gridDim.x, ..., the waves as ((w0 + w1) + w2) + w3, and partial_sum over the work-groups.
// The kick, the projection c o p, the drift, the two no-U-turn chains and the tail that writes the partials are NOT here: written
// as force-inlined fragments they change the instruction stream of the kernels that stream over chunks (the sampler
// kernels: the comparison per kernel), so each of those kernels keeps that text in place, and tests/test_*_gpu.py hold the
// three files to the same bits.
#pragma once
#include "lane_vec.h"

namespace rime {

constexpr int HMC_THREADS = 256, HMC_BYTES = 64, HMC_GROUPS = 4, HMC_MAXBLOCKS = 1024;

// the strided layout of lane_vec.h at this file's geometry
template <typename T>
__device__ __forceinline__ void hmc_load(const T* p, long long c0, long long N, bool vec, T (&x)[HMC_BYTES / sizeof(T)])
{
    lane_load<T, HMC_THREADS, HMC_GROUPS>(p, c0, N, vec, x);
}

template <typename T>
__device__ __forceinline__ void hmc_store(T* p, long long c0, long long N, bool vec, const T (&x)[HMC_BYTES / sizeof(T)])
{
    lane_store<T, HMC_THREADS, HMC_GROUPS>(p, c0, N, vec, x);
}

// sum of squares: the lane's chain in T, then float64 across the wave (every lane ends with the wave's sum)
template <typename T>
__device__ __forceinline__ double hmc_sumsq(const T (&z)[HMC_BYTES / sizeof(T)])
{
    constexpr int E = HMC_BYTES / sizeof(T);
    T c = (T)0;
#pragma unroll
    for (int i = 0; i < E; ++i) c = tfma<T>(z[i], z[i], c);
    return wave_sum((double)c);
}

// the sum of nb partials by one wave, in every lane: lane l takes partials l, l + 64, ..., then the butterfly
__device__ __forceinline__ double partial_sum(const double* __restrict__ partial, int nb)
{
    double s = 0.0;
    for (int b = (int)(threadIdx.x & 63); b < nb; b += 64) s += partial[b];
    return wave_sum(s);
}

// the second stage, one work-group of `nsums` waves or more: wave k of `nsums` writes out[k] = sum_b partial[k nb + b], the first
// halved
__device__ __forceinline__ void hmc_final(const double* __restrict__ partial, int nb, int nsums, double* __restrict__ out)
{
    const int k = threadIdx.x >> 6;
    if (k >= nsums) return;
    const double s = partial_sum(partial + (size_t)k * nb, nb);
    if ((threadIdx.x & 63) == 0) out[k] = k == 0 ? 0.5 * s : s;
}

// ---------------------------------------------------------------------------------------------------------------- host side
inline long long hmc_chunks(long long N, int dtype) { return lane_chunks(N, dtype, HMC_THREADS, HMC_BYTES); }

// work-groups of a launch over N elements
inline int hmc_blocks(long long N, int dtype) { return (int)std::min<long long>(hmc_chunks(N, dtype), HMC_MAXBLOCKS); }

// the lengths the entry points take
inline bool hmc_size_ok(long long N) { return N >= 0 && N <= 0x3fffffffffffffffLL; }

// `nsums` partials per work-group of the smaller span (float64), so that the workspace serves either dtype; 0 for a bad N
inline size_t hmc_workspace_bytes(long long N, int nsums)
{
    return hmc_size_ok(N) ? (size_t)nsums * (size_t)std::max(1, hmc_blocks(N, RIME_F64)) * sizeof(double) : 0;
}

// [a, a + bytes) and [b, b + bytes) share a byte (null: no)
inline bool hmc_overlap(const void* a, const void* b, size_t bytes)
{
    if (!a || !b) return false;
    const unsigned long long x = (unsigned long long)a, y = (unsigned long long)b;
    return x < y + bytes && y < x + bytes;
}

// a flag that is not zero but rounds to zero in float32 would skip its pass
inline bool hmc_flag_underflows(int dtype, double f) { return dtype == RIME_F32 && f != 0.0 && (float)f == 0.0f; }

} // namespace rime
