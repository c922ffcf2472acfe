// lbfgs.hip -- the L-BFGS search direction in its compact form (Byrd, Nocedal & Schnabel 1994): the two-loop recursion over a
// history of m pairs (s_j, y_j) is a function of a few inner products and ONE linear combination,
//     r = gamma * d o (v - sum_j a_j y_j) + sum_j b_j s_j ,
// so a direction costs one pass for the inner products (rime_lbfgs_dots), an m x m recurrence on the host (bfgs.compact_coeffs)
// and one pass for the combination (rime_lbfgs_combine), instead of 4 m dependent vector operations.
//
// The history is two device tables of m row addresses (oldest first); every address is a contiguous N-vector of T, aligned to
// sizeof(T) only.  The vectors are held in the strided lane layout of lane_vec.h (LB_BYTES = 64 bytes per lane as LB_GROUPS = 4
// groups); the 16-byte / element branch is uniform across the launch for v, d and r, across the wave for a row.
//
// rime_lbfgs_dots, per row j and chunk: the per-lane chains of E fused multiply-adds in T (ascending element index), then
// float64: butterfly across the wave, accumulation over the chunks of a work-group (chunk c, c + gridDim.x, ... in that
// order) in LDS by lane 0 of each wave, waves added as ((w0 + w1) + w2) + w3, one partial per work-group in the caller's
// workspace, and a second kernel that adds the partials of an output (lane l takes partials l, l + 64, ..., then the same
// butterfly).  No atomics; the order is a function of (N, dtype) alone: bit-reproducible, and the same for a launch with and
// without the new-pair index k.  Rows are processed in groups of LB_ROWS over gridDim.y.
// Vector ALU only; the register arrays are indexed by unrolled loops only (no scratch).
#include "lane_vec.h"

namespace rime {

constexpr int LB_THREADS = 256, LB_BYTES = 64, LB_GROUPS = 4, LB_ROWS = 128, LB_MAXBLOCKS = 1024;

// the strided layout of lane_vec.h at this file's geometry
template <typename T>
__device__ __forceinline__ void lb_load(const T* p, long long c0, long long N, bool vec, T (&x)[LB_BYTES / sizeof(T)])
{
    lane_load<T, LB_THREADS, LB_GROUPS>(p, c0, N, vec, x);
}

// the lane's chain in T, then float64 across the wave (every lane ends with the wave's sum)
template <typename T>
__device__ __forceinline__ double lb_dot(const T (&a)[LB_BYTES / sizeof(T)], const T (&b)[LB_BYTES / sizeof(T)])
{
    constexpr int E = LB_BYTES / sizeof(T);
    T c = (T)0;
#pragma unroll
    for (int i = 0; i < E; ++i) c = tfma<T>(a[i], b[i], c);
    return wave_sum((double)c);
}

// partial [gridDim.x][m][NQ]: NQ = 2 (s_j.v, y_j.(d o v)) or, with a new pair k, 5 (+ s_j.y_k, y_j.s_k, y_j.(d o y_k))
template <typename T, bool HASK>
__global__ __launch_bounds__(LB_THREADS) void lbfgs_dots_kernel(const T* const* __restrict__ S, const T* const* __restrict__ Y,
                                                                const T* __restrict__ v, const T* __restrict__ d, int k, int m,
                                                                long long N, long long nchunks, double* __restrict__ partial)
{
    constexpr int E = LB_BYTES / sizeof(T), NQ = HASK ? 5 : 2;
    constexpr long long SPAN = (long long)LB_THREADS * E;
    __shared__ double acc[LB_THREADS / 64][LB_ROWS * NQ];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r0 = blockIdx.y * LB_ROWS, nr = min(LB_ROWS, m - r0);
    for (int o = lane; o < nr * NQ; o += 64) acc[wave][o] = 0.0;
    __syncthreads();
    const bool v_vec = aligned16(v), d_vec = aligned16(d);
    const T* sk = HASK ? S[k] : nullptr;
    const T* yk = HASK ? Y[k] : nullptr;
    const bool sk_vec = aligned16(sk), yk_vec = aligned16(yk);
    for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const long long c0 = chunk * SPAN;
        T xv[E], xdv[E], xsk[E], xyk[E], xdyk[E];
        lb_load<T>(v, c0, N, v_vec, xv);
        if (d != nullptr) {
            lb_load<T>(d, c0, N, d_vec, xdv);
#pragma unroll
            for (int i = 0; i < E; ++i) xdyk[i] = xdv[i];
#pragma unroll
            for (int i = 0; i < E; ++i) xdv[i] *= xv[i];
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) { xdv[i] = xv[i]; xdyk[i] = (T)1; }
        }
        if (HASK) {
            lb_load<T>(sk, c0, N, sk_vec, xsk);
            lb_load<T>(yk, c0, N, yk_vec, xyk);
#pragma unroll
            for (int i = 0; i < E; ++i) xdyk[i] *= xyk[i];
        }
        for (int j = 0; j < nr; ++j) {
            const T* sj = S[r0 + j];
            const T* yj = Y[r0 + j];
            T xs[E], xy[E];
            lb_load<T>(sj, c0, N, aligned16(sj), xs);
            lb_load<T>(yj, c0, N, aligned16(yj), xy);
            double p[NQ];
            p[0] = lb_dot<T>(xs, xv);
            p[1] = lb_dot<T>(xy, xdv);
            if (HASK) {
                p[2] = lb_dot<T>(xs, xyk);
                p[3] = lb_dot<T>(xy, xsk);
                p[4] = lb_dot<T>(xy, xdyk);
            }
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[wave][j * NQ + q] += p[q];
            }
        }
    }
    __syncthreads();
    double* out = partial + ((long long)blockIdx.x * m + r0) * NQ;
    for (int o = tid; o < nr * NQ; o += LB_THREADS) out[o] = ((acc[0][o] + acc[1][o]) + acc[2][o]) + acc[3][o];
}

// out[q * m + j] = sum_b partial[b][j][q]; one wave per output
__global__ __launch_bounds__(LB_THREADS) void lbfgs_dots_final_kernel(const double* __restrict__ partial, int nb, int m, int NQ,
                                                                      double* __restrict__ out)
{
    const int o = blockIdx.x * (LB_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= m * NQ) return;                                  // whole waves leave together
    double s = 0.0;
    for (int b = lane; b < nb; b += 64) s += partial[(long long)b * m * NQ + o];
    s = wave_sum(s);
    if (lane == 0) out[(long long)(o % NQ) * m + o / NQ] = s;
}

// r = gamma * d o (v - sum_j a_j y_j) + sum_j b_j s_j, every element one chain in T: q = v, q = fma(-a_j, y_j, q) for
// j = 0 .. m - 1, t = (gamma * d) * q, t = fma(b_j, s_j, t) for j = 0 .. m - 1
template <typename T>
__global__ __launch_bounds__(LB_THREADS) void lbfgs_combine_kernel(const T* const* __restrict__ S, const T* const* __restrict__ Y,
                                                                   const T* __restrict__ v, const T* __restrict__ d,
                                                                   const double* __restrict__ a, const double* __restrict__ b,
                                                                   double gamma, int m, long long N, T* __restrict__ r)
{
    constexpr int E = LB_BYTES / sizeof(T);
    const long long c0 = (long long)blockIdx.x * LB_THREADS * E;
    T q[E];
    lb_load<T>(v, c0, N, aligned16(v), q);
    for (int j = 0; j < m; ++j) {
        const T* yj = Y[j];
        const T na = (T)(-a[j]);
        T x[E];
        lb_load<T>(yj, c0, N, aligned16(yj), x);
#pragma unroll
        for (int i = 0; i < E; ++i) q[i] = tfma<T>(na, x[i], q[i]);
    }
    const T g = (T)gamma;
    if (d != nullptr) {
        T x[E];
        lb_load<T>(d, c0, N, aligned16(d), x);
#pragma unroll
        for (int i = 0; i < E; ++i) q[i] = (g * x[i]) * q[i];
    } else {
#pragma unroll
        for (int i = 0; i < E; ++i) q[i] = g * q[i];
    }
    for (int j = 0; j < m; ++j) {
        const T* sj = S[j];
        const T bj = (T)b[j];
        T x[E];
        lb_load<T>(sj, c0, N, aligned16(sj), x);
#pragma unroll
        for (int i = 0; i < E; ++i) q[i] = tfma<T>(bj, x[i], q[i]);
    }
    lane_store<T, LB_THREADS, LB_GROUPS>(r, c0, N, aligned16(r), q);
}

// chunks of a pass; the workspace is sized for the smaller span (float64) so that it serves either dtype
static long long lb_chunks(long long N, int dtype) { return lane_chunks(N, dtype, LB_THREADS, LB_BYTES); }

static bool lb_bad(int dtype, const void* s_rows, const void* y_rows, int m, long long N)
{
    return !real_dtype_ok(dtype) || m < 1 || N < 1 || N > 0x3fffffffffffffffLL || !s_rows || !y_rows;
}

template <typename T>
static int lb_dots(const void* const* S, const void* const* Y, int m, long long N, const void* v, const void* d, int k, double* out,
                   double* part, int nb, long long nchunks, hipStream_t st)
{
    const dim3 grid((unsigned)nb, (unsigned)((m + LB_ROWS - 1) / LB_ROWS));
    const int NQ = k >= 0 ? 5 : 2;
    if (k >= 0)
        hipLaunchKernelGGL((lbfgs_dots_kernel<T, true>), grid, dim3(LB_THREADS), 0, st, (const T* const*)S, (const T* const*)Y,
                           (const T*)v, (const T*)d, k, m, N, nchunks, part);
    else
        hipLaunchKernelGGL((lbfgs_dots_kernel<T, false>), grid, dim3(LB_THREADS), 0, st, (const T* const*)S, (const T* const*)Y,
                           (const T*)v, (const T*)d, 0, m, N, nchunks, part);
    hipLaunchKernelGGL(lbfgs_dots_final_kernel, dim3((unsigned)((m * NQ + 3) / 4)), dim3(LB_THREADS), 0, st, (const double*)part, nb, m,
                       NQ, out);
    return check_launch();
}

} // namespace rime

using namespace rime;

extern "C" size_t rime_lbfgs_workspace(int m, long long N)
{
    if (m < 1 || N < 1 || N > 0x3fffffffffffffffLL) return 0;
    const long long nb = std::min<long long>(lb_chunks(N, RIME_F64), LB_MAXBLOCKS);
    return (size_t)nb * (size_t)m * 5 * sizeof(double);
}

extern "C" int rime_lbfgs_dots(int dtype, const void* const* s_rows, const void* const* y_rows, int m, long long N, const void* v,
                               const void* d, int k, double* out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (lb_bad(dtype, s_rows, y_rows, m, N) || !v || !out) return RIME_EINVAL;
    if (k < -1 || k >= m || m > 65535 * LB_ROWS) return RIME_EINVAL;
    if (!workspace || workspace_bytes < rime_lbfgs_workspace(m, N)) return RIME_EWORKSPACE;
    const long long nchunks = lb_chunks(N, dtype);
    const int nb = (int)std::min<long long>(nchunks, LB_MAXBLOCKS);
    return with_real(dtype, [&](auto t) {
        return lb_dots<decltype(t)>(s_rows, y_rows, m, N, v, d, k, out, (double*)workspace, nb, nchunks, as_stream(stream));
    });
}

extern "C" int rime_lbfgs_combine(int dtype, const void* const* s_rows, const void* const* y_rows, int m, long long N, const void* v,
                                  const void* d, const double* a, const double* b, double gamma, void* r, void* stream)
{
    if (lb_bad(dtype, s_rows, y_rows, m, N) || !v || !a || !b || !r) return RIME_EINVAL;
    const long long nchunks = lb_chunks(N, dtype);
    if (nchunks > 0x7fffffffLL) return RIME_EINVAL;
    return with_real(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((lbfgs_combine_kernel<T>), dim3((unsigned)nchunks), dim3(LB_THREADS), 0, as_stream(stream),
                           (const T* const*)s_rows, (const T* const*)y_rows, (const T*)v, (const T*)d, a, b, gamma, m, N, (T*)r);
        return check_launch();
    });
}
