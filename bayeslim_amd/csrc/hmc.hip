// hmc.hip -- one leapfrog stage of Hamiltonian Monte Carlo with a diagonal mass over the flat parameter vector (sampler.leapfrog,
// sampler.HMC.K): the momentum kick, the position drift and the kinetic energy in ONE pass,
//     p <- fma(-(T(kick) * eps), g, p)          if kick  != 0
//     q <- fma(T(drift) * eps, c * (c * p), q)  if drift != 0     (the updated p)
//     energy[0] = 1/2 sum (c * p)^2             if energy         (the updated p)
// with eps (step size per element) and c (diagonal Cholesky factor of the covariance) each optional (null: ones).  A trajectory
// of N leapfrog steps is N + 1 launches: (kick, drift) = (1/2, 1), (1, 1) x (N - 1), (1/2, 0) with the energy.
//
// The vectors are held in the strided lane layout of lane_vec.h (HMC_BYTES = 64 bytes per lane as HMC_GROUPS = 4 groups); the
// 16-byte / element branch is uniform across the launch.
//
// Energy: the per-lane chain of E fused multiply-adds in T (ascending element index), then float64: butterfly across the wave,
// accumulation over the chunks of a work-group (chunk b, b + gridDim.x, ... in that order) by lane 0 of each wave, waves added
// as ((w0 + w1) + w2) + w3, one partial per work-group in the caller's workspace, and a second kernel that adds the partials
// (lane l takes partials l, l + 64, ..., then the same butterfly) and halves the sum.  No atomics; the order is a function of
// (N, dtype) alone: bit-reproducible, and the same for the energy-only pass and the pass fused with the last kick.
// Vector ALU only; the register arrays are indexed by unrolled loops only (no scratch).
#include "hmc_common.h"

namespace rime {

// q, p in place; g, eps, c read only; null pointers as in the header.  partial [gridDim.x] when want_energy
template <typename T>
__global__ __launch_bounds__(HMC_THREADS) void hmc_step_kernel(T* q, T* p, const T* __restrict__ g, const T* __restrict__ eps,
                                                              const T* __restrict__ c, T kick, T drift, int want_energy,
                                                              long long N, long long nchunks, double* __restrict__ partial)
{
    constexpr int E = HMC_BYTES / sizeof(T);
    constexpr long long SPAN = (long long)HMC_THREADS * E;
    __shared__ double acc[HMC_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool do_kick = kick != (T)0, do_drift = drift != (T)0;
    const bool q_vec = aligned16(q), p_vec = aligned16(p), g_vec = aligned16(g), e_vec = aligned16(eps), c_vec = aligned16(c);
    double mine = 0.0;                                       // lane 0 of a wave: the wave's sum over this work-group's chunks
    for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const long long c0 = chunk * SPAN;
        T xp[E], xe[E], xc[E];
        hmc_load<T>(p, c0, N, p_vec, xp);
        if (eps != nullptr) hmc_load<T>(eps, c0, N, e_vec, xe);
        if (c != nullptr) hmc_load<T>(c, c0, N, c_vec, xc);
        if (do_kick) {
            T xg[E];
            hmc_load<T>(g, c0, N, g_vec, xg);
            if (eps != nullptr) {
#pragma unroll
                for (int i = 0; i < E; ++i) xp[i] = tfma<T>(-(kick * xe[i]), xg[i], xp[i]);
            } else {
#pragma unroll
                for (int i = 0; i < E; ++i) xp[i] = tfma<T>(-kick, xg[i], xp[i]);
            }
            hmc_store<T>(p, c0, N, p_vec, xp);
        }
        T z[E];                                              // c o p
        if (c != nullptr) {
#pragma unroll
            for (int i = 0; i < E; ++i) z[i] = xc[i] * xp[i];
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) z[i] = xp[i];
        }
        if (do_drift) {
            T xq[E];
            hmc_load<T>(q, c0, N, q_vec, xq);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const T de = eps != nullptr ? drift * xe[i] : drift;
                const T v = c != nullptr ? xc[i] * z[i] : z[i];
                xq[i] = tfma<T>(de, v, xq[i]);
            }
            hmc_store<T>(q, c0, N, q_vec, xq);
        }
        if (want_energy) mine += hmc_sumsq<T>(z);
    }
    if (want_energy) {
        if (lane == 0) acc[wave] = mine;
        __syncthreads();
        if (tid == 0) partial[blockIdx.x] = ((acc[0] + acc[1]) + acc[2]) + acc[3];
    }
}

// energy[0] = 1/2 sum_b partial[b]; one wave
__global__ __launch_bounds__(64) void hmc_energy_final_kernel(const double* __restrict__ partial, int nb, double* __restrict__ energy)
{
    hmc_final(partial, nb, 1, energy);
}

template <typename T>
static int hmc_step(long long N, void* q, void* p, const void* g, const void* eps, const void* c, double kick, double drift,
                   double* energy, double* part, hipStream_t st, int dtype)
{
    const long long nchunks = hmc_chunks(N, dtype);
    const int nb = hmc_blocks(N, dtype);
    if (nb > 0)
        hipLaunchKernelGGL((hmc_step_kernel<T>), dim3((unsigned)nb), dim3(HMC_THREADS), 0, st, (T*)q, (T*)p, (const T*)g, (const T*)eps,
                           (const T*)c, (T)kick, (T)drift, energy != nullptr ? 1 : 0, N, nchunks, part);
    if (energy != nullptr)
        hipLaunchKernelGGL(hmc_energy_final_kernel, dim3(1), dim3(64), 0, st, (const double*)part, nb, energy);
    return check_launch();
}

} // namespace rime

using namespace rime;

// one partial per work-group
extern "C" size_t rime_hmc_workspace(long long N) { return hmc_workspace_bytes(N, 1); }

extern "C" int rime_hmc_step(int dtype, long long N, void* q, void* p, const void* g, const void* eps, const void* c, double kick,
                             double drift, double* energy, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!real_dtype_ok(dtype) || !hmc_size_ok(N) || !p) return RIME_EINVAL;
    if (!(kick == kick) || !(drift == drift)) return RIME_EINVAL;                      // NaN flags
    if ((kick != 0.0 && !g) || (drift != 0.0 && !q)) return RIME_EINVAL;
    if (energy != nullptr && (!workspace || workspace_bytes < rime_hmc_workspace(N))) return RIME_EWORKSPACE;
    // a flag that rounds to zero in the working type would skip its pass: refuse it
    if (hmc_flag_underflows(dtype, kick) || hmc_flag_underflows(dtype, drift)) return RIME_EINVAL;
    if (kick == 0.0 && drift == 0.0 && energy == nullptr) return RIME_OK;               // nothing to do
    return with_real(dtype, [&](auto t) {
        return hmc_step<decltype(t)>(N, q, p, g, eps, c, kick, drift, energy, (double*)workspace, as_stream(stream), dtype);
    });
}
