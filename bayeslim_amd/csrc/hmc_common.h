// hmc_common.h -- what hmc.hip (one leapfrog stage) and nuts.hip (the two halves of a tree leaf) share: the geometry of a launch,
// the strided lane layout of lane_vec.h at that geometry, the per-lane chain of the kinetic energy and the second stage's sum of
// the work-groups' partials.  Everything here is force-inlined or constexpr (lane_vec.h): a kernel that uses it assembles to the
// code object it would with the text written out in place.  The energy of either file is summed in ONE order, which is why the
// pieces of that order live here: the chain of hmc_sumsq in T, the butterfly, the chunks of a work-group in the order b,
// b + gridDim.x, ..., the waves as ((w0 + w1) + w2) + w3, and partial_sum over the work-groups.
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

inline long long hmc_chunks(long long N, int dtype) { return lane_chunks(N, dtype, HMC_THREADS, HMC_BYTES); }

// work-groups of a launch over N elements
inline int hmc_blocks(long long N, int dtype) { return (int)std::min<long long>(hmc_chunks(N, dtype), HMC_MAXBLOCKS); }

} // namespace rime
