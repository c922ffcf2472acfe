// prior.hip -- log-priors of the optimiser loop (gfx950): the summed value and the per-element derivative of
//     laplace        t = -|r| / s,  r = x - m (side 'upper': r < 0 -> 0; 'lower': r > 0 -> 0)     d = -sign(r) / s
//     taper_sigmoid  t = logsig(c (x - l)) + logsig(-c (x - u))                                    d = c sig(-c (x - l)) - c sig(c (x - u))
//     taper_tanh     t = log tanh(c (x - l)) + log tanh(-c (x - u))                                d = 2c / sinh(2c (x - l)) - 2c / sinh(-2c (x - u))
// (optim.LogLaplacePrior, optim.LogTaperedUniformPrior; DESIGN.md, "Log-priors") in ONE pass over x: out = sum t, dx = d,
// so that the backward is the scaling g dx.  HBM-bound: x is read once and dx written once with the 16-byte lane
// accesses of lane_vec.h; an operand (m, s, l, u, c) is one scalar (period 1), a full tensor (period N, the same
// accesses) or a trailing broadcast (1 < period < N, period | N: element i % period by element loads).
// Deterministic: terms in T, per-thread and per-block sums in double, per-block partials in the workspace, summed in block
// order by a second kernel.  No atomics.
//
// Forms (each equal to its law wherever the law is finite, accurate relative to |t| + |z t'(z)|):
//   logsig(z) = min(z, 0) - log1p(e),  sig(-z) = (z >= 0 ? e : 1) / (1 + e),  e = exp(-|z|): finite for every finite z,
//     where log(sigmoid(z)) is -inf below z = -88 (float);
//   z > 0, q = exp(-2z), em = -expm1(-2z) = 1 - q, p = 1 + q:  tanh z = em / p,  1 / sinh 2z = 2q / (em p),
//     log tanh z = log(em / p) for z < 0.55, else log1p(a) with a = -2q / p = tanh z - 1, taken as log(w) a / (w - 1),
//     w = 1 + a (a itself where w rounds to 1): log(tanh z) read literally rounds to 0 from z = 9 on (float), where the
//     law is -2 exp(-2z);  z < 0: NaN (the law's log of a negative number), the derivative by 1 / sinh's oddness.
#include <hip/hip_runtime.h>
#include "lane_vec.h"

namespace rime {

constexpr int PRIOR_THREADS = 256, PRIOR_BYTES = 32, PRIOR_GROUPS = 2;   // 32 bytes of x per lane and chunk
constexpr int PRIOR_MAX_BLOCKS = 2048;                                   // 8 work-groups per CU; the rest by grid stride
enum { PRIOR_LAPLACE = 0, PRIOR_SIGMOID = 1, PRIOR_TANH = 2 };
enum { PRIOR_BOTH = 0, PRIOR_UPPER = 1, PRIOR_LOWER = 2 };

struct PriorOperand { const void* p; unsigned long long period; };
struct PriorOperands { PriorOperand m, s, l, u, c; };

// exp of x <= 0 in float.  Not expf: this library is built with -ffp-contract=fast, under which the compiler's own expansion
// of expf fuses the rounded product x log2(e) into the subtraction of its integer part and then adds the product's rounding
// error a second time: measured 0.7 |x| ulp (45 ulp at x = -64).  Here the reduced argument x log2(e) - E is formed by two
// explicit fused multiply-adds (log2(e) = hi + lo), so that no contraction can change it: measured 0.97 ulp.
__device__ __forceinline__ float t_exp(float x)
{
    const float xc = fmaxf(x, -126.0f);                                    // 2^-181 is 0; keeps E finite for x = -inf
    const float E = rintf(xc * 0x1.715476p+0f);
    const float A = fmaf(xc, 0x1.4ae0bep-26f, fmaf(xc, 0x1.715476p+0f, -E));
    const float r = ldexpf(__builtin_amdgcn_exp2f(A), (int)E);
    return x != x ? x : r;
}
__device__ __forceinline__ double t_exp(double x) { return exp(x); }
__device__ __forceinline__ float t_expm1(float x) { return expm1f(x); }
__device__ __forceinline__ double t_expm1(double x) { return expm1(x); }
__device__ __forceinline__ float t_log(float x) { return logf(x); }
__device__ __forceinline__ double t_log(double x) { return log(x); }
__device__ __forceinline__ float t_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double t_log1p(double x) { return log1p(x); }

// this lane's elements of an operand for the chunk at c0: one value for a scalar, the lane layout of x for a full operand,
// element i % period for a trailing broadcast (always inside the operand, also past the end of x); absent: left as it is
template <typename T, int E>
__device__ __forceinline__ void prior_operand(const PriorOperand& o, long long c0, long long N, T (&v)[E])
{
    constexpr int W = Vec16<T>::W;
    const T* p = static_cast<const T*>(o.p);
    if (!p) return;
    if (o.period == 1ull) {
        const T a = p[0];
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] = a;
    } else if (o.period == (unsigned long long)N) {
        lane_load<T, PRIOR_THREADS, PRIOR_GROUPS>(p, c0, N, aligned16(p), v);
    } else {
#pragma unroll
        for (int g = 0; g < PRIOR_GROUPS; ++g) {
            const unsigned long long e = (unsigned long long)(c0 + (long long)(g * PRIOR_THREADS + (int)threadIdx.x) * W);
            unsigned long long k = e % o.period;
#pragma unroll
            for (int i = 0; i < W; ++i) {
                v[g * W + i] = p[k];
                k = (k + 1 == o.period) ? 0ull : k + 1;
            }
        }
    }
}

// logsig(z) and sig(-z)
template <typename T>
__device__ __forceinline__ void prior_logsig(T z, T& t, T& sneg)
{
    const T e = t_exp(-fabs(z));
    t = fmin(z, T(0)) - t_log1p(e);
    sneg = (z >= T(0) ? e : T(1)) / (T(1) + e);
}

// log tanh z and 1 / sinh 2z
template <typename T>
__device__ __forceinline__ void prior_logtanh(T z, T& t, T& rsinh)
{
    const T za = fabs(z);
    const T q = t_exp(T(-2) * za), em = -t_expm1(T(-2) * za), p = T(1) + q;
    const bool small = za < T(0.55);
    const T a = T(-2) * q / p, w = T(1) + a;
    const T lw = t_log(small ? em / p : w);
    t = small ? lw : (w == T(1) ? a : lw * a / (w - T(1)));
    rsinh = T(2) * q / (em * p);
    if (z < T(0)) { t = __builtin_nan(""); rsinh = -rsinh; }
}

template <typename T, int KIND>
__global__ void __launch_bounds__(PRIOR_THREADS)
prior_fwd_kernel(const T* __restrict__ x, long long N, long long nchunks, PriorOperands ops, int side, T* __restrict__ dx,
                 double* __restrict__ partial)
{
    constexpr int W = Vec16<T>::W, E = PRIOR_GROUPS * W;
    constexpr long long SPAN = (long long)PRIOR_THREADS * E;
    __shared__ double red[PRIOR_THREADS / 64];
    const bool xvec = aligned16(x), dvec = aligned16(dx);
    double acc = 0.0;
    for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const long long c0 = chunk * SPAN;
        T xv[E], d[E], t[E];
        lane_load<T, PRIOR_THREADS, PRIOR_GROUPS>(x, c0, N, xvec, xv);
        if constexpr (KIND == PRIOR_LAPLACE) {
            T m[E], s[E];
            prior_operand<T, E>(ops.m, c0, N, m);
            prior_operand<T, E>(ops.s, c0, N, s);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                T r = xv[i] - m[i];
                if ((side == PRIOR_UPPER && r < T(0)) || (side == PRIOR_LOWER && r > T(0))) r = T(0);
                const T sg = r > T(0) ? T(1) : (r < T(0) ? T(-1) : r);       // 0 at r == 0, NaN stays NaN
                t[i] = -fabs(r) / s[i];
                d[i] = -sg / s[i];
            }
        } else {
            T l[E], u[E], c[E];
            prior_operand<T, E>(ops.l, c0, N, l);
            prior_operand<T, E>(ops.u, c0, N, u);
            prior_operand<T, E>(ops.c, c0, N, c);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                T ti = T(0), di = T(0), tj, dj;
                if (ops.l.p) {
                    const T z = c[i] * (xv[i] - l[i]);
                    if constexpr (KIND == PRIOR_SIGMOID) { prior_logsig(z, tj, dj); di = c[i] * dj; }
                    else { prior_logtanh(z, tj, dj); di = T(2) * c[i] * dj; }
                    ti = tj;
                }
                if (ops.u.p) {
                    const T z = -c[i] * (xv[i] - u[i]);
                    if constexpr (KIND == PRIOR_SIGMOID) { prior_logsig(z, tj, dj); di -= c[i] * dj; }
                    else { prior_logtanh(z, tj, dj); di -= T(2) * c[i] * dj; }
                    ti += tj;
                }
                t[i] = ti;
                d[i] = di;
            }
        }
#pragma unroll
        for (int g = 0; g < PRIOR_GROUPS; ++g) {
            const long long e = c0 + (long long)(g * PRIOR_THREADS + (int)threadIdx.x) * W;
#pragma unroll
            for (int i = 0; i < W; ++i)
                if (e + i < N) acc += (double)t[g * W + i];
        }
        if (dx) lane_store<T, PRIOR_THREADS, PRIOR_GROUPS>(dx, c0, N, dvec, d);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

template <typename T>
__global__ void __launch_bounds__(256)
prior_final_kernel(const double* __restrict__ partial, int nb, T* __restrict__ out)
{
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) acc += partial[i];      // fixed assignment: deterministic
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (T)red[0];
}

// gx = g[0] dx
template <typename T>
__global__ void __launch_bounds__(PRIOR_THREADS)
prior_bwd_kernel(const T* __restrict__ dx, const T* __restrict__ g, long long N, long long nchunks, T* __restrict__ gx)
{
    constexpr int E = PRIOR_GROUPS * Vec16<T>::W;
    constexpr long long SPAN = (long long)PRIOR_THREADS * E;
    const bool dvec = aligned16(dx), gvec = aligned16(gx);
    const T g0 = g[0];
    for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        T v[E];
        lane_load<T, PRIOR_THREADS, PRIOR_GROUPS>(dx, chunk * SPAN, N, dvec, v);
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] *= g0;
        lane_store<T, PRIOR_THREADS, PRIOR_GROUPS>(gx, chunk * SPAN, N, gvec, v);
    }
}

// a period names one of the three operand modes of an N-element x
static bool prior_period_ok(const PriorOperand& o, size_t N)
{
    if (!o.p) return true;
    if (o.period == 0 || o.period > N) return false;
    return o.period == 1 || o.period == N || N % o.period == 0;
}

} // namespace rime

using namespace rime;

extern "C" size_t rime_prior_workspace(void) { return PRIOR_MAX_BLOCKS * sizeof(double); }

extern "C" int rime_prior_fwd(int dtype, int kind, int side, const void* x, size_t N, const void* m, size_t m_period,
                              const void* s, size_t s_period, const void* l, size_t l_period, const void* u, size_t u_period,
                              const void* c, size_t c_period, void* out, void* dx, void* workspace, size_t workspace_bytes,
                              void* stream)
{
    if (!x || !out || N == 0 || N > (size_t)1 << 62 || !real_dtype_ok(dtype)) return RIME_EINVAL;
    if (kind < PRIOR_LAPLACE || kind > PRIOR_TANH || side < PRIOR_BOTH || side > PRIOR_LOWER) return RIME_EINVAL;
    const PriorOperands ops = {{m, m_period}, {s, s_period}, {l, l_period}, {u, u_period}, {c, c_period}};
    for (const PriorOperand* o : {&ops.m, &ops.s, &ops.l, &ops.u, &ops.c})
        if (!prior_period_ok(*o, N)) return RIME_EINVAL;
    if (kind == PRIOR_LAPLACE ? (!m || !s) : ((!l && !u) || !c)) return RIME_EINVAL;
    if (!workspace || workspace_bytes < rime_prior_workspace()) return RIME_EWORKSPACE;
    const long long nchunks = lane_chunks((long long)N, dtype, PRIOR_THREADS, PRIOR_BYTES);
    const int nb = (int)std::min<long long>(nchunks, PRIOR_MAX_BLOCKS);
    double* part = (double*)workspace;
    hipStream_t st = as_stream(stream);
    return with_real(dtype, [&](auto t) {
        using T = decltype(t);
        auto launch = [&](auto k) {
            hipLaunchKernelGGL((prior_fwd_kernel<T, decltype(k)::value>), dim3(nb), dim3(PRIOR_THREADS), 0, st, (const T*)x,
                               (long long)N, nchunks, ops, side, (T*)dx, part);
        };
        if (kind == PRIOR_LAPLACE) launch(int_c<PRIOR_LAPLACE>{});
        else if (kind == PRIOR_SIGMOID) launch(int_c<PRIOR_SIGMOID>{});
        else launch(int_c<PRIOR_TANH>{});
        hipLaunchKernelGGL((prior_final_kernel<T>), dim3(1), dim3(256), 0, st, part, nb, (T*)out);
        return check_launch();
    });
}

extern "C" int rime_prior_bwd(int dtype, const void* dx, const void* g, size_t N, void* gx, void* stream)
{
    if (!dx || !g || !gx || N == 0 || N > (size_t)1 << 62 || !real_dtype_ok(dtype)) return RIME_EINVAL;
    const long long nchunks = lane_chunks((long long)N, dtype, PRIOR_THREADS, PRIOR_BYTES);
    const int nb = (int)std::min<long long>(nchunks, PRIOR_MAX_BLOCKS);
    return with_real(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((prior_bwd_kernel<T>), dim3(nb), dim3(PRIOR_THREADS), 0, as_stream(stream), (const T*)dx,
                           (const T*)g, (long long)N, nchunks, (T*)gx);
        return check_launch();
    });
}
