// nuts.hip -- one leaf of the No-U-Turn sampler's tree (bayeslim_amd/nuts.py): a leapfrog step of signed size h from an edge state
// that stays as it is, in two launches around the potential's gradient,
//     open:    p1 = fma(-(T(h/2) * eps), g0, p0);   q1 = fma(T(h) * eps, c * (c * p1), q0)          (q0, p0, g0 read only)
//     close:   p1 <- fma(-(T(h/2) * eps), g1, p1);  out[0] = 1/2 sum (c * p1)^2
//              out[1] = sum (q1 - q_far) * p_far;   out[2] = sum (q1 - q_far) * p1                 (the updated p1)
// with eps (step size per element) and c (diagonal Cholesky factor of the covariance) each optional (null: ones).  open is the
// first stage of hmc.hip, (kick, drift) = (h/2, h), written out of place: the same operations on the same operands, hence the
// same bits as a copy and that stage.  close is its last stage, (h/2, 0) with the energy, plus the two projections of the span
// from the far edge of the tree on the momenta at its ends: the no-U-turn criterion of Hoffman & Gelman (2014) costs no pass.
//
// Layout and sums are hmc.hip's (hmc_common.h): the strided lane layout, 64 bytes per lane, the 16-byte / element branch uniform
// across the launch.  Each of the three sums is a per-lane chain of E fused multiply-adds in T (ascending element index; the
// difference q1 - q_far is rounded once in T), then float64: the butterfly across the wave, the chunks of a work-group in the
// order b, b + gridDim.x, ..., the waves as ((w0 + w1) + w2) + w3, one partial per work-group and sum in the caller's workspace
// (sum k of work-group b at k * gridDim.x + b), and a second kernel whose wave k adds the partials of sum k.  No atomics; out[0]
// carries the bits of rime_hmc_step's energy.  Vector ALU only; the register arrays are indexed by unrolled loops only.
#include "hmc_common.h"

namespace rime {

// T(scale) * eps per element, or T(scale) alone
template <typename T, int E>
__device__ __forceinline__ void nuts_kick(T (&xp)[E], const T (&xg)[E], const T (&xe)[E], bool has_eps, T kick)
{
    if (has_eps) {
#pragma unroll
        for (int i = 0; i < E; ++i) xp[i] = tfma<T>(-(kick * xe[i]), xg[i], xp[i]);
    } else {
#pragma unroll
        for (int i = 0; i < E; ++i) xp[i] = tfma<T>(-kick, xg[i], xp[i]);
    }
}

template <typename T>
__global__ __launch_bounds__(HMC_THREADS) void nuts_leaf_open_kernel(const T* __restrict__ q0, const T* __restrict__ p0,
                                                                    const T* __restrict__ g0, T* __restrict__ q1, T* __restrict__ p1,
                                                                    const T* __restrict__ eps, const T* __restrict__ c, T kick, T drift,
                                                                    long long N, long long nchunks)
{
    constexpr int E = HMC_BYTES / sizeof(T);
    constexpr long long SPAN = (long long)HMC_THREADS * E;
    const bool q0_vec = aligned16(q0), p0_vec = aligned16(p0), g_vec = aligned16(g0), q1_vec = aligned16(q1), p1_vec = aligned16(p1),
               e_vec = aligned16(eps), c_vec = aligned16(c);
    for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const long long c0 = chunk * SPAN;
        T xp[E], xg[E], xe[E], xc[E], xq[E];
        hmc_load<T>(p0, c0, N, p0_vec, xp);
        hmc_load<T>(g0, c0, N, g_vec, xg);
        if (eps != nullptr) hmc_load<T>(eps, c0, N, e_vec, xe);
        if (c != nullptr) hmc_load<T>(c, c0, N, c_vec, xc);
        nuts_kick<T, E>(xp, xg, xe, eps != nullptr, kick);
        hmc_store<T>(p1, c0, N, p1_vec, xp);
        hmc_load<T>(q0, c0, N, q0_vec, xq);
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const T de = eps != nullptr ? drift * xe[i] : drift;
            const T z = c != nullptr ? xc[i] * xp[i] : xp[i];
            const T v = c != nullptr ? xc[i] * z : z;
            xq[i] = tfma<T>(de, v, xq[i]);
        }
        hmc_store<T>(q1, c0, N, q1_vec, xq);
    }
}

// partial [3 gridDim.x]: the sums of squares, then (with DOTS) the two projections
template <typename T, bool DOTS>
__global__ __launch_bounds__(HMC_THREADS) void nuts_leaf_close_kernel(const T* __restrict__ q1, T* p1, const T* __restrict__ g1,
                                                                     const T* __restrict__ eps, const T* __restrict__ c,
                                                                     const T* __restrict__ q_far, const T* __restrict__ p_far, T kick,
                                                                     long long N, long long nchunks, double* __restrict__ partial)
{
    constexpr int E = HMC_BYTES / sizeof(T);
    constexpr long long SPAN = (long long)HMC_THREADS * E;
    __shared__ double acc[3][HMC_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool q_vec = aligned16(q1), p_vec = aligned16(p1), g_vec = aligned16(g1), e_vec = aligned16(eps), c_vec = aligned16(c),
               qf_vec = aligned16(q_far), pf_vec = aligned16(p_far);
    double mine = 0.0, far = 0.0, near = 0.0;              // lane 0 of a wave: the wave's sums over this work-group's chunks
    for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const long long c0 = chunk * SPAN;
        T xp[E], xg[E], xe[E];
        hmc_load<T>(p1, c0, N, p_vec, xp);
        hmc_load<T>(g1, c0, N, g_vec, xg);
        if (eps != nullptr) hmc_load<T>(eps, c0, N, e_vec, xe);
        nuts_kick<T, E>(xp, xg, xe, eps != nullptr, kick);
        hmc_store<T>(p1, c0, N, p_vec, xp);
        T z[E];                                              // c o p
        if (c != nullptr) {
            hmc_load<T>(c, c0, N, c_vec, z);
#pragma unroll
            for (int i = 0; i < E; ++i) z[i] = z[i] * xp[i];
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) z[i] = xp[i];
        }
        mine += hmc_sumsq<T>(z);
        if (DOTS) {
            T d[E], xf[E];
            hmc_load<T>(q1, c0, N, q_vec, d);
            hmc_load<T>(q_far, c0, N, qf_vec, xf);
#pragma unroll
            for (int i = 0; i < E; ++i) d[i] = d[i] - xf[i];
            hmc_load<T>(p_far, c0, N, pf_vec, xf);
            T a = (T)0, b = (T)0;
#pragma unroll
            for (int i = 0; i < E; ++i) {
                a = tfma<T>(d[i], xf[i], a);
                b = tfma<T>(d[i], xp[i], b);
            }
            far += wave_sum((double)a);
            near += wave_sum((double)b);
        }
    }
    if (lane == 0) {
        acc[0][wave] = mine;
        if (DOTS) acc[1][wave] = far, acc[2][wave] = near;
    }
    __syncthreads();
    if (tid < (DOTS ? 3 : 1)) partial[(size_t)tid * gridDim.x + blockIdx.x] = ((acc[tid][0] + acc[tid][1]) + acc[tid][2]) + acc[tid][3];
}

// wave k of `nsums`: out[k] = sum_b partial[k nb + b], the first halved
__global__ __launch_bounds__(192) void nuts_leaf_final_kernel(const double* __restrict__ partial, int nb, int nsums, double* __restrict__ out)
{
    hmc_final(partial, nb, nsums, out);
}

template <typename T>
static int nuts_open(long long N, const void* q0, const void* p0, const void* g0, void* q1, void* p1, const void* eps, const void* c,
                     double h, hipStream_t st, int dtype)
{
    const int nb = hmc_blocks(N, dtype);
    if (nb > 0)
        hipLaunchKernelGGL((nuts_leaf_open_kernel<T>), dim3((unsigned)nb), dim3(HMC_THREADS), 0, st, (const T*)q0, (const T*)p0,
                           (const T*)g0, (T*)q1, (T*)p1, (const T*)eps, (const T*)c, (T)(h / 2), (T)h, N, hmc_chunks(N, dtype));
    return check_launch();
}

template <typename T>
static int nuts_close(long long N, const void* q1, void* p1, const void* g1, const void* eps, const void* c, double h,
                      const void* q_far, const void* p_far, double* out, double* part, hipStream_t st, int dtype)
{
    const int nb = hmc_blocks(N, dtype);
    const long long nchunks = hmc_chunks(N, dtype);
    const bool dots = q_far != nullptr;
    if (nb > 0) {
        if (dots)
            hipLaunchKernelGGL((nuts_leaf_close_kernel<T, true>), dim3((unsigned)nb), dim3(HMC_THREADS), 0, st, (const T*)q1, (T*)p1,
                               (const T*)g1, (const T*)eps, (const T*)c, (const T*)q_far, (const T*)p_far, (T)(h / 2), N, nchunks, part);
        else
            hipLaunchKernelGGL((nuts_leaf_close_kernel<T, false>), dim3((unsigned)nb), dim3(HMC_THREADS), 0, st, (const T*)q1, (T*)p1,
                               (const T*)g1, (const T*)eps, (const T*)c, (const T*)nullptr, (const T*)nullptr, (T)(h / 2), N, nchunks,
                               part);
    }
    hipLaunchKernelGGL(nuts_leaf_final_kernel, dim3(1), dim3(192), 0, st, (const double*)part, nb, dots ? 3 : 1, out);
    return check_launch();
}

// the signed step: a number, not zero, and with a half that is not zero in T (nor in float64)
static int nuts_step_ok(double h) { return h == h && h != 0.0; }
static bool nuts_step_underflows(int dtype, double h) { return h / 2 == 0.0 || hmc_flag_underflows(dtype, h / 2); }

} // namespace rime

using namespace rime;

// three partials per work-group
extern "C" size_t rime_nuts_workspace(long long N) { return hmc_workspace_bytes(N, 3); }

extern "C" int rime_nuts_leaf_open(int dtype, long long N, const void* q0, const void* p0, const void* g0, void* q1, void* p1,
                                   const void* eps, const void* c, double h, void* stream)
{
    if (!real_dtype_ok(dtype) || !hmc_size_ok(N) || !q0 || !p0 || !g0 || !q1 || !p1) return RIME_EINVAL;
    const size_t bytes = (size_t)N * real_bytes(dtype);
    for (const void* in : {q0, p0, g0, eps, c})
        if (hmc_overlap(q1, in, bytes) || hmc_overlap(p1, in, bytes)) return RIME_EINVAL;
    if (hmc_overlap(q1, p1, bytes)) return RIME_EINVAL;
    if (!nuts_step_ok(h) || nuts_step_underflows(dtype, h)) return RIME_EINVAL;
    return with_real(dtype, [&](auto t) {
        return nuts_open<decltype(t)>(N, q0, p0, g0, q1, p1, eps, c, h, as_stream(stream), dtype);
    });
}

extern "C" int rime_nuts_leaf_close(int dtype, long long N, const void* q1, void* p1, const void* g1, const void* eps, const void* c,
                                    double h, const void* q_far, const void* p_far, double* out, void* workspace,
                                    size_t workspace_bytes, void* stream)
{
    if (!real_dtype_ok(dtype) || !hmc_size_ok(N) || !q1 || !p1 || !g1 || !out) return RIME_EINVAL;
    if ((q_far == nullptr) != (p_far == nullptr)) return RIME_EINVAL;
    if (!nuts_step_ok(h)) return RIME_EINVAL;
    if (!workspace || workspace_bytes < rime_nuts_workspace(N)) return RIME_EWORKSPACE;
    if (nuts_step_underflows(dtype, h)) return RIME_EINVAL;                              // as rime_hmc_step: after the workspace
    return with_real(dtype, [&](auto t) {
        return nuts_close<decltype(t)>(N, q1, p1, g1, eps, c, h, q_far, p_far, out, (double*)workspace, as_stream(stream), dtype);
    });
}
