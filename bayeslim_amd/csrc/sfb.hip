// sfb.hip -- radial step of the spherical Fourier-Bessel sky (gfx950):
//     a_lm(r) = sum_n g_l(k_ln r) t_lmn                     (SFBModel.forward_gln, sph_harm.py:1979-1982)
// One small matrix product PER DEGREE l in the reference (slice, reshape, matmul, indexed assignment, and the same chain
// again in autograd); here ONE launch per direction over a host-built tile list that covers every degree.
//
//   forward   out[b, r, cols[col_off + c]] = sum_n g[g_off + n Nr + r] p[b, p_off + n Nl + c]
//   backward  gp[b, p_off + n Nl + c]      = sum_r g[g_off + n Nr + r] gout[b, r, cols[col_off + c]]
//
// Both are  res[i, c] = sum_k A[k, i] X[k, c]  on a 64 (i) x 32 (c) tile: i = r, k = n forwards, i = n, k = r backwards.  The
// work-group (256 lanes) stages 32 values of k at a time through LDS -- the A tile as [k][i], the X tile as [k][c] -- and every
// lane keeps 8 (i) x 1 (c) accumulators: lane % 32 is the column, so the loads of the parameters and the stores of a degree whose
// columns are contiguous coalesce, and the 8 values of A a lane needs are one 32-byte broadcast read.  g is real, so a complex
// column is two real ones (V = 2) held side by side: no complex multiply, and re / im leave in one 8- or 16-byte store.
// The sum over k runs in ascending order in one lane: no atomics, bit-reproducible.  The tiles of one direction write disjoint
// elements (the params_idx slices partition the Nlmn axis; the column sets of the degrees are disjoint), so nothing is zero-filled
// here: a degree with Nk = 0 has forward tiles that store its zeros, and columns without any degree are the caller's.
// Vector ALU on purpose: ~0.5 GFLOP at lmax 128 -- the launch count is what this file removes, not arithmetic.
#include <hip/hip_runtime.h>
#include "rime_common.h"

namespace rime {

constexpr int SFB_TI = 64;       // tile rows (r forwards, n backwards)
constexpr int SFB_TC = 32;       // tile columns (a_lm columns of one degree)
constexpr int SFB_KC = 32;       // contraction chunk staged in LDS
constexpr int SFB_LDA = SFB_TI + 4;     // row stride of the A tile: keeps 16-byte alignment, spreads the transposed store

template <typename T, int V> struct SfbVec;
template <> struct SfbVec<float, 1> { using type = float; };
template <> struct SfbVec<float, 2> { using type = float2; };
template <> struct SfbVec<double, 1> { using type = double; };
template <> struct SfbVec<double, 2> { using type = double2; };

// V = 1: real parameters, V = 2: complex (interleaved re, im).  BWD exchanges the roles of n and r.
template <typename T, int V, bool BWD>
__global__ void __launch_bounds__(256)
sfb_kernel(const T* __restrict__ X, const T* __restrict__ g, const int* __restrict__ blocks, const int* __restrict__ cols,
           const int* __restrict__ tiles, int Nblk, int Ntile, int Nlmn, int Nr, int Nlm, T* __restrict__ res)
{
    using VT = typename SfbVec<T, V>::type;
    __shared__ __attribute__((aligned(16))) T a_s[SFB_KC][SFB_LDA];
    __shared__ __attribute__((aligned(16))) T x_s[SFB_KC][SFB_TC * V];

    const int tile = blockIdx.x % Ntile;
    const size_t b = blockIdx.x / Ntile;
    const int blk = tiles[3 * tile];
    if (blk < 0 || blk >= Nblk) return;                       // malformed table: write nothing
    const int i0 = tiles[3 * tile + 1], c0 = tiles[3 * tile + 2];
    const int g_off = blocks[5 * blk], Nk = blocks[5 * blk + 1], p_off = blocks[5 * blk + 2];
    const int col_off = blocks[5 * blk + 3], Nl = blocks[5 * blk + 4];
    const int NI = BWD ? Nk : Nr;         // extent of the tile's row axis
    const int NK = BWD ? Nr : Nk;         // extent of the contraction
    const T* gb = g + g_off;
    const T* pin = X + b * (size_t)(BWD ? (size_t)Nr * Nlm : (size_t)Nlmn) * V;      // batch row of the input
    T* pout = res + b * (size_t)(BWD ? (size_t)Nlmn : (size_t)Nr * Nlm) * V;         // batch row of the output

    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c = c0 + tx;
    int col = -1;                                              // a_lm column of this lane (-1: past the degree's columns)
    if (c < Nl) {
        col = cols[col_off + c];
        if (col < 0 || col >= Nlm) col = -1;
    }

    T acc[8][V];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int v = 0; v < V; v++) acc[i][v] = T(0);

    for (int k0 = 0; k0 < NK; k0 += SFB_KC) {
        // A tile -> a_s[kk][ii]
        if (!BWD) {
            // g[(k0 + kk) Nr + i0 + ii]: lanes along ii (r), coalesced
            for (int e = threadIdx.x; e < SFB_KC * SFB_TI; e += 256) {
                const int kk = e / SFB_TI, ii = e % SFB_TI;
                const int k = k0 + kk, i = i0 + ii;
                a_s[kk][ii] = (k < NK && i < NI) ? gb[(size_t)k * Nr + i] : T(0);
            }
        } else {
            // g[(i0 + ii) Nr + k0 + kk]: lanes along kk (r), coalesced; stored transposed
            for (int e = threadIdx.x; e < SFB_KC * SFB_TI; e += 256) {
                const int ii = e / SFB_KC, kk = e % SFB_KC;
                const int k = k0 + kk, i = i0 + ii;
                a_s[kk][ii] = (k < NK && i < NI) ? gb[(size_t)i * Nr + k] : T(0);
            }
        }
        // X tile -> x_s[kk][cc V + v]: one lane per (kk, cc), V-wide
        for (int e = threadIdx.x; e < SFB_KC * SFB_TC; e += 256) {
            const int kk = e / SFB_TC, cc = e % SFB_TC;
            const int k = k0 + kk;
            VT val = VT();
            if (k < NK && c0 + cc < Nl) {
                if (!BWD) {
                    const int idx = p_off + k * Nl + c0 + cc;
                    if (idx < Nlmn) val = *reinterpret_cast<const VT*>(pin + (size_t)idx * V);
                } else {
                    const int cl = cols[col_off + c0 + cc];
                    if (cl >= 0 && cl < Nlm) val = *reinterpret_cast<const VT*>(pin + ((size_t)k * Nlm + cl) * V);
                }
            }
            *reinterpret_cast<VT*>(&x_s[kk][cc * V]) = val;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < SFB_KC; kk++) {
            T a[8], x[V];
#pragma unroll
            for (int i = 0; i < 8; i++) a[i] = a_s[kk][ty * 8 + i];
#pragma unroll
            for (int v = 0; v < V; v++) x[v] = x_s[kk][tx * V + v];
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int v = 0; v < V; v++) acc[i][v] = tfma<T>(a[i], x[v], acc[i][v]);
        }
        __syncthreads();
    }

    if (col < 0) return;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int ir = i0 + ty * 8 + i;
        if (ir >= NI) break;
        VT val;
        if constexpr (V == 2) { val.x = acc[i][0]; val.y = acc[i][1]; } else { val = acc[i][0]; }
        if (!BWD) {
            *reinterpret_cast<VT*>(pout + ((size_t)ir * Nlm + col) * V) = val;
        } else {
            const int idx = p_off + ir * Nl + c;
            if (idx < Nlmn) *reinterpret_cast<VT*>(pout + (size_t)idx * V) = val;
        }
    }
}

template <bool BWD>
static int sfb_launch(int dtype, int cplx, const void* X, const void* g, const int* blocks, const int* cols, const int* tiles,
                      int Nblk, int Ntile, int B, int Nlmn, int Nr, int Nlm, void* res, void* stream)
{
    if (!real_dtype_ok(dtype)) return RIME_EINVAL;
    if (cplx != 0 && cplx != 1) return RIME_EINVAL;
    if (Nr <= 0 || Nlm <= 0 || Nlmn < 0 || B < 0 || Nblk < 0 || Ntile < 0) return RIME_EINVAL;
    if (Nblk > 0 && (!blocks || !cols)) return RIME_EINVAL;
    if (Ntile > 0 && (!tiles || Nblk == 0)) return RIME_EINVAL;
    if ((long long)Ntile * (long long)B > 0x7fffffffLL) return RIME_EINVAL;
    if (Ntile == 0 || B == 0) return RIME_OK;                 // nothing to write
    if (!X || !g || !res) return RIME_EINVAL;
    return with_real(dtype, [&](auto t) {
        using T = decltype(t);
        with_bool(cplx != 0, [&](auto c) {
            hipLaunchKernelGGL((sfb_kernel<T, c.value ? 2 : 1, BWD>), dim3((unsigned)(Ntile * B)), dim3(256), 0,
                               as_stream(stream), (const T*)X, (const T*)g, blocks, cols, tiles, Nblk, Ntile, Nlmn, Nr, Nlm,
                               (T*)res);
        });
        return check_launch();
    });
}

} // namespace rime

using namespace rime;

extern "C" int rime_sfb_fwd(int dtype, int cplx, const void* params, const void* g, const int* blocks, const int* cols,
                            const int* tiles, int Nblk, int Ntile, int B, int Nlmn, int Nr, int Nlm, void* out, void* stream)
{
    return sfb_launch<false>(dtype, cplx, params, g, blocks, cols, tiles, Nblk, Ntile, B, Nlmn, Nr, Nlm, out, stream);
}

extern "C" int rime_sfb_bwd(int dtype, int cplx, const void* gout, const void* g, const int* blocks, const int* cols,
                            const int* tiles, int Nblk, int Ntile, int B, int Nlmn, int Nr, int Nlm, void* gparams, void* stream)
{
    return sfb_launch<true>(dtype, cplx, gout, g, blocks, cols, tiles, Nblk, Ntile, B, Nlmn, Nr, Nlm, gparams, stream);
}
