// recycle.hip -- one step of a recycled Hamiltonian Monte Carlo trajectory (recycled.RecycledHMC; Nishimura & Dunson 2020) with a
// diagonal mass over the flat parameter vector: the closing half kick of step i with its kinetic energy, the snapshot of the
// state into row i of the trajectory buffers, and the opening half kick and drift of step i + 1, in ONE pass:
//     p1    = fma(-(T(half) * eps), g, p)
//     energy[0] = 1/2 sum (c * p1)^2
//     q_out = q ;  p_out = p1
//     drift != 0:   p2 = fma(-(T(half) * eps), g, p1) ;  p = p2 ;  q = fma(T(drift) * eps, c * (c * p2), q)
//     drift == 0:   p = p1
// eps and c optional (null: ones) as in hmc.hip.  Five vector reads (p, g, q, eps, c) and four writes (p, q, q_out, p_out), where
// rime_hmc_step(half, 0, energy), two device copies and rime_hmc_step(half, drift) take eleven and five.
//
// Bit contract: q, p, q_out, p_out and energy carry the bits of that sequence of four operations -- two half kicks, each a fused
// multiply-add of its own, never one full kick -- for every N, dtype, alignment and null combination.  The layout is that of
// hmc.hip (lane_vec.h at the geometry of hmc_common.h), the energy is summed in its order (the chain of hmc_sumsq in T, the
// butterfly, chunks, waves, partial_sum) and the kick, the projection, the drift and the tail that writes the partials are written
// out in place, as hmc_common.h asks of a kernel that streams over chunks.  Vector ALU only, no atomics; the register arrays are
// indexed by unrolled loops only (no scratch).
#include "hmc_common.h"

namespace rime {

// q, p in place; g, eps, c read only (eps, c null: ones); q_out, p_out written; partial [gridDim.x]
template <typename T>
__global__ __launch_bounds__(HMC_THREADS) void hmc_recycle_kernel(T* q, T* p, const T* __restrict__ g, const T* __restrict__ eps,
                                                                 const T* __restrict__ c, T half, T drift, T* __restrict__ q_out,
                                                                 T* __restrict__ p_out, long long N, long long nchunks,
                                                                 double* __restrict__ partial)
{
    constexpr int E = HMC_BYTES / sizeof(T);
    constexpr long long SPAN = (long long)HMC_THREADS * E;
    __shared__ double acc[HMC_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool do_drift = drift != (T)0;
    const bool q_vec = aligned16(q), p_vec = aligned16(p), g_vec = aligned16(g), e_vec = aligned16(eps), c_vec = aligned16(c);
    const bool qo_vec = aligned16(q_out), po_vec = aligned16(p_out);
    double mine = 0.0;                                       // lane 0 of a wave: the wave's sum over this work-group's chunks
    for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const long long c0 = chunk * SPAN;
        T xp[E], xg[E], xq[E], xe[E], xc[E];
        hmc_load<T>(p, c0, N, p_vec, xp);
        hmc_load<T>(g, c0, N, g_vec, xg);
        hmc_load<T>(q, c0, N, q_vec, xq);
        if (eps != nullptr) hmc_load<T>(eps, c0, N, e_vec, xe);
        if (c != nullptr) hmc_load<T>(c, c0, N, c_vec, xc);
        hmc_store<T>(q_out, c0, N, qo_vec, xq);
        // the closing half kick
        if (eps != nullptr) {
#pragma unroll
            for (int i = 0; i < E; ++i) xp[i] = tfma<T>(-(half * xe[i]), xg[i], xp[i]);
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) xp[i] = tfma<T>(-half, xg[i], xp[i]);
        }
        hmc_store<T>(p_out, c0, N, po_vec, xp);
        T z[E];                                              // c o p1
        if (c != nullptr) {
#pragma unroll
            for (int i = 0; i < E; ++i) z[i] = xc[i] * xp[i];
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) z[i] = xp[i];
        }
        mine += hmc_sumsq<T>(z);
        if (do_drift) {
            // the opening half kick of the next step, then its drift
            if (eps != nullptr) {
#pragma unroll
                for (int i = 0; i < E; ++i) xp[i] = tfma<T>(-(half * xe[i]), xg[i], xp[i]);
            } else {
#pragma unroll
                for (int i = 0; i < E; ++i) xp[i] = tfma<T>(-half, xg[i], xp[i]);
            }
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const T de = eps != nullptr ? drift * xe[i] : drift;
                const T zi = c != nullptr ? xc[i] * xp[i] : xp[i];
                const T v = c != nullptr ? xc[i] * zi : zi;
                xq[i] = tfma<T>(de, v, xq[i]);
            }
            hmc_store<T>(q, c0, N, q_vec, xq);
        }
        hmc_store<T>(p, c0, N, p_vec, xp);
    }
    if (lane == 0) acc[wave] = mine;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = ((acc[0] + acc[1]) + acc[2]) + acc[3];
}

// energy[0] = 1/2 sum_b partial[b]; one wave
__global__ __launch_bounds__(64) void hmc_recycle_final_kernel(const double* __restrict__ partial, int nb, double* __restrict__ energy)
{
    hmc_final(partial, nb, 1, energy);
}

template <typename T>
static int hmc_recycle(long long N, void* q, void* p, const void* g, const void* eps, const void* c, double half, double drift,
                      void* q_out, void* p_out, double* energy, double* part, hipStream_t st, int dtype)
{
    const long long nchunks = hmc_chunks(N, dtype);
    const int nb = hmc_blocks(N, dtype);
    if (nb > 0)
        hipLaunchKernelGGL((hmc_recycle_kernel<T>), dim3((unsigned)nb), dim3(HMC_THREADS), 0, st, (T*)q, (T*)p, (const T*)g,
                           (const T*)eps, (const T*)c, (T)half, (T)drift, (T*)q_out, (T*)p_out, N, nchunks, part);
    hipLaunchKernelGGL(hmc_recycle_final_kernel, dim3(1), dim3(64), 0, st, (const double*)part, nb, energy);
    return check_launch();
}

} // namespace rime

using namespace rime;

extern "C" int rime_hmc_recycle(int dtype, long long N, void* q, void* p, const void* g, const void* eps, const void* c, double half,
                                double drift, void* q_out, void* p_out, double* energy, void* workspace, size_t workspace_bytes,
                                void* stream)
{
    if (!real_dtype_ok(dtype) || !hmc_size_ok(N) || !p || !q || !g || !q_out || !p_out || !energy) return RIME_EINVAL;
    if (!(half == half) || !(drift == drift) || half == 0.0) return RIME_EINVAL;        // NaN flags; no kick: nothing to recycle
    const size_t bytes = (size_t)N * (size_t)real_bytes(dtype);
    for (const void* out : {(const void*)q_out, (const void*)p_out})
        for (const void* in : {(const void*)q, (const void*)p, g, eps, c})
            if (hmc_overlap(out, in, bytes)) return RIME_EINVAL;
    if (hmc_overlap(q_out, p_out, bytes)) return RIME_EINVAL;
    if (!workspace || workspace_bytes < hmc_workspace_bytes(N, 1)) return RIME_EWORKSPACE;
    // a flag that rounds to zero in the working type would skip its pass: refuse it
    if (hmc_flag_underflows(dtype, half) || hmc_flag_underflows(dtype, drift)) return RIME_EINVAL;
    return with_real(dtype, [&](auto t) {
        return hmc_recycle<decltype(t)>(N, q, p, g, eps, c, half, drift, q_out, p_out, energy, (double*)workspace,
                                        as_stream(stream), dtype);
    });
}
