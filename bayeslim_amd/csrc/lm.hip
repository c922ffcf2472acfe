// lm.hip -- y = M x along the middle axis of a contiguous x [O][K_in][I] with the gather, the two real scalings and the
// real-part projection of the reference's LinearModel.forward fused into ONE launch (linear_model.py:121-169: params * coeff,
// index_select, matmul / einsum, .real), and the same launch with M = A^H for the backward pass and least squares:
//     y[o, r, i] = post[r] * sum_{k < K} M[r, k] * (pre[k] * x[o, idx[k], i])            y [O][R][I]
// x and M are real or complex (interleaved), y is complex when either is, unless out_real asks for Re(M x) only
// (Mr xr - Mi xi: half the arithmetic, half the bytes).  M is read through element strides (m_rs, m_ks), uniform across a wave
// (scalar loads); the caller stores it so that the index the kernel walks fastest is contiguous.
//
// Strided mapping (I > 1): one lane per column (o, i), lanes along the flattened column index, so that every load and store
// of a row of x or y is contiguous across the wave (in runs of I elements).
// The form follows K alone (the host picks it; R plays no part in the choice):
//   few-in  (K <= 32): the K inputs of the column are loaded once into registers; loop over r, one store per r.  The rows
//                      are split over gridDim.y in chunks of at least 32 when there are too few columns to fill the chip.
//   few-out (K > 32):  up to 32 rows r are accumulated in registers (4, 8, 16 or 32 accumulators for R <= 32, else gridDim.y
//                      tiles R by 32); loop over k, one load per k.
// A lane holds 4, 2 or 1 columns (256 columns apart, so each access of a wave stays contiguous), as many as the register arrays
// and the size of the grid allow: one scalar load of M then serves that many outputs.
// Last-axis mapping (I == 1): lanes along r (16 ... 64 of them), 256 / lanes line groups of 4 lines each per work-group;
// M and the lines are staged in LDS in tiles of 16 along k (zero-padded, so the inner loop has no tail).
// Every output element is written by exactly one thread, the sum runs in ascending k, no atomics: bit-reproducible.
// The register arrays are indexed by unrolled loops only (no scratch).
#include "rime_common.h"

namespace rime {

constexpr int LM_THREADS = 256, LM_REG = 32, LM_KT = 16, LM_LPT = 4, LM_MAXLINES = 64, LM_TARGET_BLOCKS = 1024;

struct LmArgs {
    const void *x, *M, *pre, *post;
    const int* idx;
    void* y;
    long long O, I, m_rs, m_ks;
    int K, K_in, R;
    hipStream_t st;
};

template <typename T> struct V2;
template <> struct V2<float>  { using type = float2; };
template <> struct V2<double> { using type = double2; };

// one element (W = 1 real, W = 2 complex) at element offset e of p
template <typename T, bool C> __device__ __forceinline__ void lm_load(const T* __restrict__ p, long long e, T& re, T& im)
{
    if (C) {
        const typename V2<T>::type v = reinterpret_cast<const typename V2<T>::type*>(p)[e];
        re = v.x; im = v.y;
    } else {
        re = p[e]; im = (T)0;
    }
}
template <typename T, bool C> __device__ __forceinline__ void lm_store(T* __restrict__ p, long long e, T re, T im)
{
    if (C) reinterpret_cast<typename V2<T>::type*>(p)[e] = typename V2<T>::type{re, im};
    else p[e] = re;
}

// acc += m * x for the type combination; ai is touched only when the output is complex
template <typename T, bool XC, bool MC, bool YC>
__device__ __forceinline__ void lm_mac(T mr, T mi, T xr, T xi, T& ar, T& ai)
{
    ar = tfma<T>(mr, xr, ar);
    if (XC && MC) ar = tfma<T>(-mi, xi, ar);
    if (YC) {
        if (XC) ai = tfma<T>(mr, xi, ai);
        if (MC) ai = tfma<T>(mi, xr, ai);
    }
}

// columns of one lane: c0 + j * LM_THREADS, j < CPL (a wave's accesses stay contiguous for every j); a column past the end
// reads column 0 instead (always there) and stores nothing
template <int CPL>
__device__ __forceinline__ void lm_columns(long long C, long long I, int K_in, int R, long long (&xb)[CPL], long long (&yb)[CPL],
                                           bool (&live)[CPL])
{
    const long long c0 = (long long)blockIdx.x * (LM_THREADS * CPL) + threadIdx.x;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const long long c = c0 + (long long)j * LM_THREADS;
        live[j] = c < C;
        const long long cc = live[j] ? c : 0;
        const long long o = cc / I, i = cc - o * I;
        xb[j] = o * K_in * I + i;
        yb[j] = o * R * I + i;
    }
}

template <typename T, bool XC, bool MC, bool OR, int KT, int CPL>
__global__ __launch_bounds__(LM_THREADS) void lm_few_in_kernel(const T* __restrict__ x, const T* __restrict__ M,
                                                               const int* __restrict__ idx, const T* __restrict__ pre,
                                                               const T* __restrict__ post, long long C, long long I, int K, int K_in,
                                                               int R, int rchunk, long long m_rs, long long m_ks, T* __restrict__ y)
{
    constexpr bool YC = (XC || MC) && !OR;
    long long xb[CPL], yb[CPL];
    bool live[CPL];
    lm_columns<CPL>(C, I, K_in, R, xb, yb, live);
    if (!live[0]) return;
    T xr[CPL][KT], xi[CPL][KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        const long long kk = (k < K && idx != nullptr) ? (long long)idx[k] : (long long)k;
        const T p = (k < K && pre != nullptr) ? pre[k] : (T)1;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            xr[j][k] = (T)0; xi[j][k] = (T)0;
            if (k < K) {
                lm_load<T, XC>(x, xb[j] + kk * I, xr[j][k], xi[j][k]);
                xr[j][k] *= p; xi[j][k] *= p;
            }
        }
    }
    const int r0 = blockIdx.y * rchunk, r1 = min(R, r0 + rchunk);
    for (int r = r0; r < r1; ++r) {
        const long long mb = (long long)r * m_rs;
        T ar[CPL], ai[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) { ar[j] = (T)0; ai[j] = (T)0; }
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            if (k < K) {
                T mr, mi;
                lm_load<T, MC>(M, mb + k * m_ks, mr, mi);
#pragma unroll
                for (int j = 0; j < CPL; ++j) lm_mac<T, XC, MC, YC>(mr, mi, xr[j][k], xi[j][k], ar[j], ai[j]);
            }
        }
        const T p = post != nullptr ? post[r] : (T)1;
#pragma unroll
        for (int j = 0; j < CPL; ++j)
            if (live[j]) lm_store<T, YC>(y, yb[j] + (long long)r * I, ar[j] * p, ai[j] * p);
    }
}

template <typename T, bool XC, bool MC, bool OR, int RT, int CPL>
__global__ __launch_bounds__(LM_THREADS) void lm_few_out_kernel(const T* __restrict__ x, const T* __restrict__ M,
                                                                const int* __restrict__ idx, const T* __restrict__ pre,
                                                                const T* __restrict__ post, long long C, long long I, int K, int K_in,
                                                                int R, long long m_rs, long long m_ks, T* __restrict__ y)
{
    constexpr bool YC = (XC || MC) && !OR;
    long long xb[CPL], yb[CPL];
    bool live[CPL];
    lm_columns<CPL>(C, I, K_in, R, xb, yb, live);
    if (!live[0]) return;
    const int r0 = blockIdx.y * LM_REG, nr = min(RT, R - r0);
    T ar[CPL][RT], ai[CPL][RT];
#pragma unroll
    for (int j = 0; j < CPL; ++j)
#pragma unroll
        for (int q = 0; q < RT; ++q) { ar[j][q] = (T)0; ai[j][q] = (T)0; }
#pragma unroll 2
    for (int k = 0; k < K; ++k) {
        const long long kk = idx != nullptr ? (long long)idx[k] : (long long)k;
        const T p = pre != nullptr ? pre[k] : (T)1;
        T xr[CPL], xi[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            lm_load<T, XC>(x, xb[j] + kk * I, xr[j], xi[j]);
            xr[j] *= p; xi[j] *= p;
        }
        const long long mb = (long long)r0 * m_rs + (long long)k * m_ks;
#pragma unroll
        for (int q = 0; q < RT; ++q) {
            if (q < nr) {
                T mr, mi;
                lm_load<T, MC>(M, mb + q * m_rs, mr, mi);
#pragma unroll
                for (int j = 0; j < CPL; ++j) lm_mac<T, XC, MC, YC>(mr, mi, xr[j], xi[j], ar[j][q], ai[j][q]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < RT; ++q) {
        if (q < nr) {
            const T p = post != nullptr ? post[r0 + q] : (T)1;
#pragma unroll
            for (int j = 0; j < CPL; ++j)
                if (live[j]) lm_store<T, YC>(y, yb[j] + (long long)(r0 + q) * I, ar[j][q] * p, ai[j][q] * p);
        }
    }
}

template <typename T, bool XC, bool MC, bool OR>
__global__ __launch_bounds__(LM_THREADS) void lm_last_kernel(const T* __restrict__ x, const T* __restrict__ M,
                                                             const int* __restrict__ idx, const T* __restrict__ pre,
                                                             const T* __restrict__ post, long long O, int K, int K_in, int R,
                                                             int lgRL, long long m_rs, long long m_ks, T* __restrict__ y)
{
    constexpr bool YC = (XC || MC) && !OR;
    constexpr int XW = XC ? 2 : 1, MW = MC ? 2 : 1;
    __shared__ T Ms[LM_KT][64 * MW];                       // [k][r][re, im]
    __shared__ T xs[LM_MAXLINES][LM_KT * XW + 1];          // [line][k][re, im], odd row length
    const int tid = threadIdx.x, RL = 1 << lgRL, LG = LM_THREADS >> lgRL, NL = LG * LM_LPT;
    const int rl = tid & (RL - 1), lg = tid >> lgRL;
    const int rbase = blockIdx.y * RL, r = rbase + rl;
    const long long line0 = (long long)blockIdx.x * NL;
    T ar[LM_LPT], ai[LM_LPT];
#pragma unroll
    for (int j = 0; j < LM_LPT; ++j) { ar[j] = (T)0; ai[j] = (T)0; }
    for (int k0 = 0; k0 < K; k0 += LM_KT) {
        for (int e = tid; e < RL * LM_KT; e += LM_THREADS) {
            const int kk = e >> lgRL, rr = e & (RL - 1), k = k0 + kk;
            T mr = (T)0, mi = (T)0;
            if (k < K && rbase + rr < R) lm_load<T, MC>(M, (long long)(rbase + rr) * m_rs + (long long)k * m_ks, mr, mi);
            Ms[kk][rr * MW] = mr;
            if (MC) Ms[kk][rr * MW + MW - 1] = mi;
        }
        for (int e = tid; e < NL * LM_KT; e += LM_THREADS) {
            const int l = e / LM_KT, kk = e - l * LM_KT, k = k0 + kk;
            const long long line = line0 + l;
            T xr = (T)0, xi = (T)0;
            if (k < K && line < O) {
                const long long ks = idx != nullptr ? (long long)idx[k] : (long long)k;
                lm_load<T, XC>(x, line * K_in + ks, xr, xi);
                if (pre != nullptr) { const T p = pre[k]; xr *= p; xi *= p; }
            }
            xs[l][kk * XW] = xr;
            if (XC) xs[l][kk * XW + XW - 1] = xi;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < LM_KT; ++kk) {
            const T mr = Ms[kk][rl * MW], mi = MC ? Ms[kk][rl * MW + MW - 1] : (T)0;
#pragma unroll
            for (int j = 0; j < LM_LPT; ++j) {
                const int l = lg * LM_LPT + j;
                const T xr = xs[l][kk * XW], xi = XC ? xs[l][kk * XW + XW - 1] : (T)0;
                lm_mac<T, XC, MC, YC>(mr, mi, xr, xi, ar[j], ai[j]);
            }
        }
        __syncthreads();
    }
    if (r >= R) return;
    const T p = post != nullptr ? post[r] : (T)1;
#pragma unroll
    for (int j = 0; j < LM_LPT; ++j) {
        const long long line = line0 + lg * LM_LPT + j;
        if (line < O) lm_store<T, YC>(y, line * R + r, ar[j] * p, ai[j] * p);
    }
}

template <typename T, bool XC, bool MC, bool OR, int KT, int CPL> static void lm_launch_few_in(const LmArgs& a, dim3 grid, int rchunk)
{
    hipLaunchKernelGGL((lm_few_in_kernel<T, XC, MC, OR, KT, CPL>), grid, dim3(LM_THREADS), 0, a.st, (const T*)a.x, (const T*)a.M, a.idx,
                       (const T*)a.pre, (const T*)a.post, a.O * a.I, a.I, a.K, a.K_in, a.R, rchunk, a.m_rs, a.m_ks, (T*)a.y);
}

template <typename T, bool XC, bool MC, bool OR, int RT, int CPL> static void lm_launch_few_out(const LmArgs& a, dim3 grid)
{
    hipLaunchKernelGGL((lm_few_out_kernel<T, XC, MC, OR, RT, CPL>), grid, dim3(LM_THREADS), 0, a.st, (const T*)a.x, (const T*)a.M, a.idx,
                       (const T*)a.pre, (const T*)a.post, a.O * a.I, a.I, a.K, a.K_in, a.R, a.m_rs, a.m_ks, (T*)a.y);
}

// columns per lane: as many (4, 2, 1) as the register arrays allow (N of them per column: N * CPL <= 32) while the grid
// still holds LM_TARGET_BLOCKS work-groups with `ysplit` of them per column block
static int lm_cpl(long long C, int N, long long ysplit)
{
    for (int cpl = 4; cpl > 1; cpl >>= 1)
        if (N * cpl <= LM_REG && ((C + LM_THREADS * cpl - 1) / (LM_THREADS * cpl)) * ysplit >= LM_TARGET_BLOCKS) return cpl;
    return 1;
}

template <typename T, bool XC, bool MC, bool OR> static int lm_go(const LmArgs& a)
{
    if (a.I == 1) {
        int lgRL = 4;
        while (lgRL < 6 && (1 << lgRL) < a.R) ++lgRL;
        const int RL = 1 << lgRL, NL = (LM_THREADS >> lgRL) * LM_LPT;
        const long long nb = (a.O + NL - 1) / NL, nr = ((long long)a.R + RL - 1) / RL;
        if (nb > 0x7fffffffLL || nr > 65535) return RIME_EINVAL;
        hipLaunchKernelGGL((lm_last_kernel<T, XC, MC, OR>), dim3((unsigned)nb, (unsigned)nr), dim3(LM_THREADS), 0, a.st, (const T*)a.x,
                           (const T*)a.M, a.idx, (const T*)a.pre, (const T*)a.post, a.O, a.K, a.K_in, a.R, lgRL, a.m_rs, a.m_ks,
                           (T*)a.y);
        return check_launch();
    }
    const long long C = a.O * a.I;
    if ((C + LM_THREADS - 1) / LM_THREADS > 0x7fffffffLL) return RIME_EINVAL;
    if (a.K <= LM_REG) {
        const int KT = a.K <= 4 ? 4 : a.K <= 8 ? 8 : a.K <= 16 ? 16 : 32;
        const long long maxsplit = ((long long)a.R + LM_REG - 1) / LM_REG;
        const int cpl = lm_cpl(C, KT, maxsplit);
        const long long nb = (C + LM_THREADS * cpl - 1) / (LM_THREADS * cpl);
        // split the rows over the grid while the columns alone leave compute units idle; a chunk re-reads the K inputs, so it
        // holds at least 32 rows
        const long long split = std::max(1LL, std::min((LM_TARGET_BLOCKS + nb - 1) / nb, maxsplit));
        const int rchunk = (int)((a.R + split - 1) / split);
        const dim3 grid((unsigned)nb, (unsigned)((a.R + rchunk - 1) / rchunk));
        if (grid.y > 65535) return RIME_EINVAL;
        if (KT == 4) { if (cpl == 4) lm_launch_few_in<T, XC, MC, OR, 4, 4>(a, grid, rchunk); else if (cpl == 2) lm_launch_few_in<T, XC, MC, OR, 4, 2>(a, grid, rchunk); else lm_launch_few_in<T, XC, MC, OR, 4, 1>(a, grid, rchunk); }
        else if (KT == 8) { if (cpl == 4) lm_launch_few_in<T, XC, MC, OR, 8, 4>(a, grid, rchunk); else if (cpl == 2) lm_launch_few_in<T, XC, MC, OR, 8, 2>(a, grid, rchunk); else lm_launch_few_in<T, XC, MC, OR, 8, 1>(a, grid, rchunk); }
        else if (KT == 16) { if (cpl == 2) lm_launch_few_in<T, XC, MC, OR, 16, 2>(a, grid, rchunk); else lm_launch_few_in<T, XC, MC, OR, 16, 1>(a, grid, rchunk); }
        else lm_launch_few_in<T, XC, MC, OR, 32, 1>(a, grid, rchunk);
        return check_launch();
    }
    const long long nt = ((long long)a.R + LM_REG - 1) / LM_REG;
    if (nt > 65535) return RIME_EINVAL;
    const int RT = a.R <= 4 ? 4 : a.R <= 8 ? 8 : a.R <= 16 ? 16 : 32;
    const int cpl = lm_cpl(C, RT, nt);
    const dim3 grid((unsigned)((C + LM_THREADS * cpl - 1) / (LM_THREADS * cpl)), (unsigned)nt);
    if (RT == 4) { if (cpl == 4) lm_launch_few_out<T, XC, MC, OR, 4, 4>(a, grid); else if (cpl == 2) lm_launch_few_out<T, XC, MC, OR, 4, 2>(a, grid); else lm_launch_few_out<T, XC, MC, OR, 4, 1>(a, grid); }
    else if (RT == 8) { if (cpl == 4) lm_launch_few_out<T, XC, MC, OR, 8, 4>(a, grid); else if (cpl == 2) lm_launch_few_out<T, XC, MC, OR, 8, 2>(a, grid); else lm_launch_few_out<T, XC, MC, OR, 8, 1>(a, grid); }
    else if (RT == 16) { if (cpl == 2) lm_launch_few_out<T, XC, MC, OR, 16, 2>(a, grid); else lm_launch_few_out<T, XC, MC, OR, 16, 1>(a, grid); }
    else lm_launch_few_out<T, XC, MC, OR, 32, 1>(a, grid);
    return check_launch();
}

template <typename T> static int lm_dispatch(const LmArgs& a, int xc, int mc, int out_real)
{
    if (out_real) return mc ? lm_go<T, true, true, true>(a) : lm_go<T, true, false, true>(a);
    if (xc) return mc ? lm_go<T, true, true, false>(a) : lm_go<T, true, false, false>(a);
    return mc ? lm_go<T, false, true, false>(a) : lm_go<T, false, false, false>(a);
}

} // namespace rime

using namespace rime;

extern "C" int rime_lm_apply(int dtype, int xcplx, int mcplx, int out_real, const void* x, const void* M, long long m_rs,
                             long long m_ks, const int* idx, const void* pre, const void* post, long long O, int K, int K_in,
                             int R, long long I, void* y, void* stream)
{
    if (!real_dtype_ok(dtype)) return RIME_EINVAL;
    if ((xcplx != 0 && xcplx != 1) || (mcplx != 0 && mcplx != 1) || (out_real != 0 && out_real != 1)) return RIME_EINVAL;
    if (out_real && !xcplx) return RIME_EINVAL;               // Re(M x) of a real x is Re(M) x: the caller passes Re(M)
    if (K <= 0 || R <= 0 || O <= 0 || I <= 0) return RIME_EINVAL;
    if (idx != nullptr ? K_in <= 0 : K_in != K) return RIME_EINVAL;
    if (!x || !M || !y) return RIME_EINVAL;
    if (m_rs <= 0 || m_ks <= 0) return RIME_EINVAL;
    // every element offset of x and y fits 63 bits: O * max(K_in, R) * I, with room for the complex factor 2
    const long long big = std::max(K_in, R);
    if (O > 0x3fffffffffffffffLL / I || O * I > 0x3fffffffffffffffLL / big) return RIME_EINVAL;
    LmArgs a;
    a.x = x; a.M = M; a.pre = pre; a.post = post; a.idx = idx; a.y = y;
    a.O = O; a.I = I; a.m_rs = m_rs; a.m_ks = m_ks; a.K = K; a.K_in = K_in; a.R = R;
    a.st = as_stream(stream);
    return with_real(dtype, [&](auto t) { return lm_dispatch<decltype(t)>(a, xcplx, mcplx, out_real); });
}
