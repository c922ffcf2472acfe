// bfgs.hip -- the two passes over the dense inverse Hessian of bfgs.BFGS: the product r = H x (rime_bfgs_matvec) and the
// symmetric rank-two correction H += a (x z^T + z x^T) + b x x^T in place (rime_bfgs_rank2).  One BFGS iteration is one of
// each: H is read once for H g, and read and written once for the correction (3 N^2 sizeof(T) bytes; both passes stream H
// and are bound by memory bandwidth).  H is real T [N][ld], ld >= N; only columns 0 .. N - 1 of a row are touched.
//
// The row segments of H are moved by the rule of lane_vec.h: a lane holds W = 16 / sizeof(T) adjacent columns starting at a
// multiple of W; when the base of H and ld are multiples of 16 bytes these are 16-byte accesses, otherwise element accesses of
// the same elements (the branch is uniform across the launch), so the bits do not depend on the placement of H.
//
// rime_bfgs_matvec: a work-group owns BF_MROWS = 8 whole rows, wave w the rows w and w + 4 of them.  The columns go in
// chunks of CK = 256 W; the segment of x of a chunk is staged in LDS once for the work-group.  Lane l holds the columns
// cb + (g * 64 + l) W ... + W - 1 of the chunk at cb (g = 0 .. 3) and runs ONE chain of fused multiply-adds in T per (row,
// right-hand side) over chunks, g and the W columns in ascending order, starting from 0; columns at or beyond N enter as
// fma(0, 0, acc) and change nothing.  The 64 chains of a row are added by a butterfly (partners 32, 16, ..., 1 apart) in T and
// lane 0 writes the row.  No atomics, no workspace, no work-group waits for another: the bits of a row are a function of the
// row, x and N alone.
//
// rime_bfgs_rank2: a work-group owns a tile of BF_RROWS = 16 rows by CT = 128 W columns, wave w the rows w, w + 4, w + 8,
// w + 12; a lane keeps x_j and z_j of its 2 W columns in registers, loaded once for the work-group's tile, and takes x_i, z_i
// of a row as wave-uniform values.  Per element, in T, every operation rounded on its own (no contraction of the sum):
//     p = x_i * z_j;  q = z_i * x_j;  t = p + q;  h = fma(T(a), t, H_ij);  H_ij = fma(T(b), x_i * x_j, h)
// which is symmetric under i <-> j bit for bit.
// Vector ALU only; the register arrays are indexed by unrolled loops only (no scratch memory).
#include "lane_vec.h"

namespace rime {

constexpr int BF_THREADS = 256, BF_WAVES = 4, BF_MROWS = 8, BF_MG = 4, BF_RROWS = 16, BF_RG = 2;

// W columns of a row of H from column c (a multiple of W) on; columns at or beyond N read as 0 and are not written
template <typename T>
__device__ __forceinline__ void bf_load(const T* row, long long c, long long N, bool vec, T (&a)[Vec16<T>::W])
{
    constexpr int W = Vec16<T>::W;
    const bool full = c + W <= N;
    row_load<T, W>(row, (size_t)c, full ? W : (int)(N - c), vec && full, a);
}

template <typename T>
__device__ __forceinline__ void bf_store(T* row, long long c, long long N, bool vec, const T (&a)[Vec16<T>::W])
{
    constexpr int W = Vec16<T>::W;
    if (vec && c + W <= N) {
        // the column passes through an empty asm: hipcc otherwise sinks this store and the element stores below into one
        // run of element stores (seen in the assembly: no 16-byte store left in the kernel)
        asm volatile("" : "+v"(c));
        *reinterpret_cast<typename Vec16<T>::type*>(row + c) = pack16(a);
    } else {
#pragma unroll
        for (int e = 0; e < W; ++e)
            if (c + e < N) row[c + e] = a[e];
    }
}

// x is T [N][NR] (the interleaved view of a complex vector for NR = 2), r likewise
template <typename T, int NR>
__global__ __launch_bounds__(BF_THREADS) void bfgs_matvec_kernel(const T* __restrict__ H, long long ld, long long N,
                                                                 const T* __restrict__ x, T* __restrict__ r)
{
    constexpr int W = Vec16<T>::W, CK = 64 * W * BF_MG, RW = BF_MROWS / BF_WAVES;
    __shared__ __attribute__((aligned(16))) T xs[NR * CK];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long row0 = (long long)blockIdx.x * BF_MROWS;
    const bool vec = aligned16(H) && (ld % W == 0);

    T acc[RW][NR];
#pragma unroll
    for (int k = 0; k < RW; ++k)
#pragma unroll
        for (int c = 0; c < NR; ++c) acc[k][c] = (T)0;

    for (long long cb = 0; cb < N; cb += CK) {
        __syncthreads();                                              // the last readers of xs are done
        for (int o = tid; o < CK * NR; o += BF_THREADS) {
            const int j = o / NR, c = o % NR;                         // right-hand-side major: a lane's W columns are 16 bytes
            xs[c * CK + j] = (cb + j < N) ? x[(cb + j) * NR + c] : (T)0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < RW; ++k) {
            const long long i = row0 + k * BF_WAVES + wave;
            if (i < N) {                                              // uniform across the wave
                const T* row = H + i * ld;
#pragma unroll
                for (int g = 0; g < BF_MG; ++g) {
                    const int j = (g * 64 + lane) * W;
                    T a[W];
                    bf_load<T>(row, cb + j, N, vec, a);
#pragma unroll
                    for (int e = 0; e < W; ++e)
#pragma unroll
                        for (int c = 0; c < NR; ++c) acc[k][c] = tfma<T>(a[e], xs[c * CK + j + e], acc[k][c]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < RW; ++k) {
        const long long i = row0 + k * BF_WAVES + wave;
        if (i < N) {
#pragma unroll
            for (int c = 0; c < NR; ++c) {
                const T s = wave_sum(acc[k][c]);
                if (lane == 0) r[i * NR + c] = s;
            }
        }
    }
}

// the element update of the header; contraction is off so that the two products of the sum are rounded before they are added
template <typename T>
__device__ __forceinline__ T bf_rank2_elem(T h, T xi, T zi, T xj, T zj, T a, T b)
{
#pragma clang fp contract(off)
    const T p = xi * zj;
    const T q = zi * xj;
    const T t = p + q;
    const T xx = xi * xj;
    return tfma<T>(b, xx, tfma<T>(a, t, h));
}

template <typename T>
__global__ __launch_bounds__(BF_THREADS) void bfgs_rank2_kernel(T* __restrict__ H, long long ld, long long N, const T* __restrict__ x,
                                                                const T* __restrict__ z, T a, T b, unsigned ctiles)
{
    constexpr int W = Vec16<T>::W, CT = 64 * W * BF_RG, RW = BF_RROWS / BF_WAVES;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long row0 = (long long)(blockIdx.x / ctiles) * BF_RROWS, col0 = (long long)(blockIdx.x % ctiles) * CT;
    const bool vec = aligned16(H) && (ld % W == 0), x_vec = aligned16(x), z_vec = aligned16(z);

    T xj[BF_RG][W], zj[BF_RG][W];
#pragma unroll
    for (int g = 0; g < BF_RG; ++g) {
        const long long j = col0 + (g * 64 + lane) * W;
        bf_load<T>(x, j, N, x_vec, xj[g]);
        bf_load<T>(z, j, N, z_vec, zj[g]);
    }
    T h[RW][BF_RG][W], xi[RW], zi[RW];
#pragma unroll
    for (int k = 0; k < RW; ++k) {
        const long long i = row0 + k * BF_WAVES + wave;
        if (i < N) {                                                  // uniform across the wave
            xi[k] = x[i];
            zi[k] = z[i];
#pragma unroll
            for (int g = 0; g < BF_RG; ++g) bf_load<T>(H + i * ld, col0 + (g * 64 + lane) * W, N, vec, h[k][g]);
        }
    }
#pragma unroll
    for (int k = 0; k < RW; ++k) {
        const long long i = row0 + k * BF_WAVES + wave;
        if (i < N) {
#pragma unroll
            for (int g = 0; g < BF_RG; ++g) {
#pragma unroll
                for (int e = 0; e < W; ++e) h[k][g][e] = bf_rank2_elem<T>(h[k][g][e], xi[k], zi[k], xj[g][e], zj[g][e], a, b);
                bf_store<T>(H + i * ld, col0 + (g * 64 + lane) * W, N, vec, h[k][g]);
            }
        }
    }
}

static bool bf_bad(int dtype, const void* H, long long ld, long long N)
{
    return !real_dtype_ok(dtype) || N < 1 || N > 0x7fffffffLL || ld < N || ld > 0x0fffffffffffffffLL / N || !H;
}

// whether the N-vector at p (NR values per element) shares a byte with the N rows of H
static bool bf_alias(int dtype, const void* H, long long ld, long long N, const void* p, int nr)
{
    const unsigned long long sz = (unsigned long long)real_bytes(dtype);
    const unsigned long long h0 = (unsigned long long)H, h1 = h0 + ((unsigned long long)(N - 1) * ld + N) * sz;
    const unsigned long long p0 = (unsigned long long)p, p1 = p0 + (unsigned long long)N * nr * sz;
    return p0 < h1 && h0 < p1;
}

} // namespace rime

using namespace rime;

extern "C" int rime_bfgs_matvec(int dtype, const void* H, long long ld, long long N, const void* x, int nrhs, void* r, void* stream)
{
    if (bf_bad(dtype, H, ld, N) || !x || !r || nrhs < 1 || nrhs > 2) return RIME_EINVAL;
    if (bf_alias(dtype, H, ld, N, x, nrhs) || bf_alias(dtype, H, ld, N, r, nrhs)) return RIME_EINVAL;
    const dim3 grid((unsigned)((N + BF_MROWS - 1) / BF_MROWS));
    return with_real(dtype, [&](auto t) {
        using T = decltype(t);
        if (nrhs == 1)
            hipLaunchKernelGGL((bfgs_matvec_kernel<T, 1>), grid, dim3(BF_THREADS), 0, as_stream(stream), (const T*)H, ld, N, (const T*)x,
                               (T*)r);
        else
            hipLaunchKernelGGL((bfgs_matvec_kernel<T, 2>), grid, dim3(BF_THREADS), 0, as_stream(stream), (const T*)H, ld, N, (const T*)x,
                               (T*)r);
        return check_launch();
    });
}

extern "C" int rime_bfgs_rank2(int dtype, void* H, long long ld, long long N, const void* x, const void* z, double a, double b,
                               void* stream)
{
    if (bf_bad(dtype, H, ld, N) || !x || !z || !std::isfinite(a) || !std::isfinite(b)) return RIME_EINVAL;
    if (bf_alias(dtype, H, ld, N, x, 1) || bf_alias(dtype, H, ld, N, z, 1)) return RIME_EINVAL;
    const long long ct = 64LL * (16 / real_bytes(dtype)) * BF_RG;
    const long long ctiles = (N + ct - 1) / ct, rtiles = (N + BF_RROWS - 1) / BF_RROWS;
    if (ctiles * rtiles > 0x7fffffffLL) return RIME_EINVAL;
    return with_real(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((bfgs_rank2_kernel<T>), dim3((unsigned)(ctiles * rtiles)), dim3(BF_THREADS), 0, as_stream(stream), (T*)H, ld,
                           N, (const T*)x, (const T*)z, (T)a, (T)b, (unsigned)ctiles);
        return check_launch();
    });
}
