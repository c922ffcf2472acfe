// massmat.hip -- one leapfrog stage with a block-dense mass matrix over the flat parameter vector (bayeslim_amd/massmat.py): with
// the lower-triangular Cholesky factor L of a key's covariance (C = L L^T),
//     rime_mass_project:   p_out = fma(-(T(kick) * eps), g, p_in);   z = L^T p_out  (blocks),   z = c * p_out     (elsewhere)
//     rime_mass_drift:     q_out = fma(T(drift) * eps, L z, q_in)    (blocks),      fma(T(drift) * eps, c * z, q_in) (elsewhere)
//                          out[0] = 1/2 sum z^2;  out[1] = sum (q_out - q_far) * p_far;  out[2] = sum (q_out - q_far) * p
// The blocks are a DEVICE table of rime_mass_block (include/rime_hip.h); elements of the flat vector that no block covers are
// diagonal, exactly as in hmc.hip.  Each entry point is a short fixed sequence of kernels on the caller's stream:
//     project:  mass_kick_kernel (every element: the kick and z = c * p_out, in the layout of hmc.hip), then mass_upper_kernel
//               (z = L^T p_out on the blocks, overwriting what the first kernel left there)
//     drift:    mass_lower_kernel (q_out on the rows of the blocks; skipped for drift = 0), then mass_drift_kernel (q_out on the
//               diagonal elements, and the three sums over ALL elements in the order of hmc.hip / nuts.hip), then mass_final_kernel
// so no work-group waits for another, there are no atomics, and with nblocks = 0 the triangular kernels are not launched and the
// other two perform the operations of hmc_step_kernel / nuts_leaf_close_kernel on the same operands in the same order.
//
// Summation order of the triangular products (fixed; a function of the block's n alone, not of the launch or of other blocks).
// W = 16 / sizeof(T).  A 16-byte group of a row of L is loaded with one 16-byte access when the base of L and ld are multiples of
// 16 bytes AND the whole group lies at or below the diagonal; any other group takes element loads of its elements j <= i only.
// Either way the same elements reach the same registers: the bits do not depend on the placement, and L[i][j], j > i, is never read.
//   L z (mass_lower_kernel)     row i, per right-hand side: lane l of the 64 lanes of a wave runs ONE chain acc = fma(L[i][j], z[j], acc)
//       from 0 over its columns j <= i in ascending order -- the columns 256 W q + (64 g + l) W + e for q = 0, 1, ..., g = 0 .. 3,
//       e < W -- and the 64 chains are added by the butterfly of lane_vec.h (partners 32, 16, ..., 1 apart), in T.
//   L^T p (mass_upper_kernel)   column j, per right-hand side: slot s of 32 runs ONE chain acc = fma(L[i][j], p[i], acc) from 0 over the
//       rows i >= j with i = s (mod 32) in ascending order; the 32 chains are added in T: the eight slots s = 8 w + u of wave w by a
//       butterfly over u (partners 4, 2, 1 apart), then the four waves as ((w0 + w1) + w2) + w3.
// Balance: the rows (columns) of a block go in strips of MASS_ROWS (8 W); a work-group takes strip k and strip last - k, so every
// work-group of a block streams about the same part of the triangle.  The host does not read the table: the grid is sized from N
// and nblocks (the blocks do not overlap, so their strips are bounded), a work-group finds its block by walking the table, and
// work-groups beyond the last strip pair return.  A table entry that does not fit the vector (n < 1, nrhs outside {1, 2}, ld < n,
// off < 0 or off + n nrhs > N) is skipped by every kernel.
// Vector ALU only; the register arrays are indexed by unrolled loops only (no scratch).
#include "hmc_common.h"

namespace rime {

constexpr int MASS_ROWS = 4, MASS_SLOTS = 32;

struct mass_block {                                          // rime_mass_block of the header, 64 bytes
    const void* L;
    long long ld, off;
    int n, nrhs;
    long long reserved[4];
};
static_assert(sizeof(mass_block) == 64, "rime_mass_block is 64 bytes");

__device__ __forceinline__ bool mass_block_ok(const mass_block& b, long long N)
{
    return b.L != nullptr && b.n >= 1 && (b.nrhs == 1 || b.nrhs == 2) && b.ld >= b.n && b.off >= 0 && b.off <= N
        && (long long)b.n * b.nrhs <= N - b.off;
}

// the block and strip pair of work-group wg: strips of `width` rows or columns, pair k = strips k and S - 1 - k
__device__ __forceinline__ bool mass_find(const mass_block* __restrict__ blocks, int nblocks, long long N, int width, long long wg,
                                          int& b, long long& k, long long& S)
{
    for (b = 0; b < nblocks; ++b) {
        if (!mass_block_ok(blocks[b], N)) continue;
        S = ((long long)blocks[b].n + width - 1) / width;
        const long long pairs = (S + 1) / 2;
        if (wg < pairs) {
            k = wg;
            return true;
        }
        wg -= pairs;
    }
    return false;
}

// work-groups that cover every strip pair of any valid table: sum_b (n_b / (2 width) + 1) <= N / (2 width) + nblocks
inline long long mass_grid(long long N, int nblocks, int width) { return N / (2 * width) + nblocks; }

// q_out = fma(T(drift) * eps, L z, q_in) on the rows of the blocks
template <typename T>
__global__ __launch_bounds__(HMC_THREADS) void mass_lower_kernel(const mass_block* __restrict__ blocks, int nblocks, long long N,
                                                                const T* __restrict__ z, const T* q_in, T* q_out,
                                                                const T* __restrict__ eps, T drift)
{
    constexpr int W = Vec16<T>::W, G = 4, CK = 64 * W * G;
    int b;
    long long k, S;
    if (!mass_find(blocks, nblocks, N, MASS_ROWS, blockIdx.x, b, k, S)) return;
    const mass_block blk = blocks[b];
    const T* L = (const T*)blk.L;
    const bool vec = aligned16(L) && (blk.ld % W == 0), two = blk.nrhs == 2;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nrhs = blk.nrhs;
    const T* zb = z + blk.off;
    for (int h = 0; h < 2; ++h) {
        const long long strip = h == 0 ? k : S - 1 - k;
        if (h == 1 && strip == k) break;
        const long long i = strip * MASS_ROWS + wave;
        if (i >= blk.n) continue;                              // uniform across the wave
        const T* row = L + i * blk.ld;
        T a0 = (T)0, a1 = (T)0;
        for (long long cb = 0; cb <= i; cb += CK) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const long long c = cb + (long long)(g * 64 + lane) * W;
                const int nv = (int)std::min<long long>(W, i + 1 - c);          // elements of the group at or below the diagonal
                if (nv > 0) {
                    T a[W];
                    row_load<T, W>(row, (size_t)c, nv, vec && nv == W, a);
#pragma unroll
                    for (int e = 0; e < W; ++e)
                        if (e < nv) {
                            a0 = tfma<T>(a[e], zb[(c + e) * nrhs], a0);
                            if (two) a1 = tfma<T>(a[e], zb[(c + e) * nrhs + 1], a1);
                        }
                }
            }
        }
        a0 = wave_sum(a0);
        a1 = wave_sum(a1);
        if (lane < nrhs) {
            const long long e = blk.off + i * nrhs + lane;
            const T de = eps != nullptr ? drift * eps[e] : drift;
            q_out[e] = tfma<T>(de, lane == 0 ? a0 : a1, q_in[e]);
        }
    }
}

// z = L^T p on the columns of the blocks
template <typename T>
__global__ __launch_bounds__(HMC_THREADS) void mass_upper_kernel(const mass_block* __restrict__ blocks, int nblocks, long long N,
                                                                const T* __restrict__ p, T* __restrict__ z)
{
    constexpr int W = Vec16<T>::W, CS = 8 * W;
    __shared__ T red[HMC_THREADS / 64][2][CS];
    int b;
    long long k, S;
    if (!mass_find(blocks, nblocks, N, CS, blockIdx.x, b, k, S)) return;      // uniform across the work-group
    const mass_block blk = blocks[b];
    const T* L = (const T*)blk.L;
    const bool vec = aligned16(L) && (blk.ld % W == 0), two = blk.nrhs == 2;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nrhs = blk.nrhs, n = blk.n;
    const int slot = wave * 8 + (lane >> 3);
    const T* pb = p + blk.off;
    for (int h = 0; h < 2; ++h) {
        const long long strip = h == 0 ? k : S - 1 - k;
        if (h == 1 && strip == k) break;
        const long long j0 = strip * CS, jc = j0 + (lane & 7) * W;            // this lane's first column
        T acc[2][W];
#pragma unroll
        for (int e = 0; e < W; ++e) acc[0][e] = acc[1][e] = (T)0;
        if (jc < n) {
#pragma unroll 4
            for (long long i = (j0 / MASS_SLOTS) * MASS_SLOTS + slot; i < n; i += MASS_SLOTS) {
                const int nv = (int)std::min<long long>(W, i + 1 - jc);
                if (nv > 0) {
                    T a[W];
                    row_load<T, W>(L + i * blk.ld, (size_t)jc, nv, vec && nv == W, a);
                    const T p0 = pb[i * nrhs], p1 = two ? pb[i * nrhs + 1] : (T)0;
#pragma unroll
                    for (int e = 0; e < W; ++e)
                        if (e < nv) {
                            acc[0][e] = tfma<T>(a[e], p0, acc[0][e]);
                            if (two) acc[1][e] = tfma<T>(a[e], p1, acc[1][e]);
                        }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int e = 0; e < W; ++e) {
                T v = acc[r][e];
                v += __shfl_xor(v, 32, 64);
                v += __shfl_xor(v, 16, 64);
                v += __shfl_xor(v, 8, 64);
                acc[r][e] = v;
            }
        __syncthreads();                                       // the readers of the first strip are done
        if (lane < 8) {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int e = 0; e < W; ++e) red[wave][r][lane * W + e] = acc[r][e];
        }
        __syncthreads();
        if (tid < CS * nrhs) {
            const int r = tid / CS, ci = tid % CS;
            const long long j = j0 + ci;
            if (j < n) z[blk.off + j * nrhs + r] = ((red[0][r][ci] + red[1][r][ci]) + red[2][r][ci]) + red[3][r][ci];
        }
    }
}

// every element: p_out = fma(-(T(kick) * eps), g, p_in) if kick != 0, and z = c * p_out (the first stage of hmc_step_kernel)
template <typename T>
__global__ __launch_bounds__(HMC_THREADS) void mass_kick_kernel(const T* p_in, const T* __restrict__ g, const T* __restrict__ eps,
                                                               const T* __restrict__ c, T kick, T* p_out, T* __restrict__ z,
                                                               long long N, long long nchunks)
{
    constexpr int E = HMC_BYTES / sizeof(T);
    constexpr long long SPAN = (long long)HMC_THREADS * E;
    const bool do_kick = kick != (T)0;
    const bool pi_vec = aligned16(p_in), po_vec = aligned16(p_out), g_vec = aligned16(g), e_vec = aligned16(eps), c_vec = aligned16(c),
               z_vec = aligned16(z);
    for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const long long c0 = chunk * SPAN;
        T xp[E];
        hmc_load<T>(p_in, c0, N, pi_vec, xp);
        if (do_kick) {
            T xg[E];
            hmc_load<T>(g, c0, N, g_vec, xg);
            if (eps != nullptr) {
                T xe[E];
                hmc_load<T>(eps, c0, N, e_vec, xe);
#pragma unroll
                for (int i = 0; i < E; ++i) xp[i] = tfma<T>(-(kick * xe[i]), xg[i], xp[i]);
            } else {
#pragma unroll
                for (int i = 0; i < E; ++i) xp[i] = tfma<T>(-kick, xg[i], xp[i]);
            }
            hmc_store<T>(p_out, c0, N, po_vec, xp);
        }
        if (c != nullptr) {
            T xc[E];
            hmc_load<T>(c, c0, N, c_vec, xc);
#pragma unroll
            for (int i = 0; i < E; ++i) xp[i] = xc[i] * xp[i];
        }
        hmc_store<T>(z, c0, N, z_vec, xp);
    }
}

// bit g * W + i of the result: element c0 + (g * THREADS + tid) * W + i of this lane lies in a block
template <typename T>
__device__ __forceinline__ unsigned mass_cover(const mass_block* __restrict__ blocks, int nblocks, long long N, long long c0)
{
    constexpr int W = Vec16<T>::W, E = HMC_BYTES / sizeof(T);
    constexpr long long SPAN = (long long)HMC_THREADS * E;
    unsigned m = 0;
    for (int b = 0; b < nblocks; ++b) {
        if (!mass_block_ok(blocks[b], N)) continue;
        const long long lo = blocks[b].off, hi = lo + (long long)blocks[b].n * blocks[b].nrhs;
        if (hi <= c0 || lo >= c0 + SPAN) continue;             // uniform across the work-group
#pragma unroll
        for (int g = 0; g < HMC_GROUPS; ++g)
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const long long e = c0 + (long long)(g * HMC_THREADS + (int)threadIdx.x) * W + i;
                if (e >= lo && e < hi) m |= 1u << (g * W + i);
            }
    }
    return m;
}

// the diagonal elements' drift and the three sums over every element; partial [3 gridDim.x] as in nuts_leaf_close_kernel
template <typename T, bool DOTS>
__global__ __launch_bounds__(HMC_THREADS) void mass_drift_kernel(const mass_block* __restrict__ blocks, int nblocks,
                                                                const T* __restrict__ z, const T* q_in, T* q_out,
                                                                const T* __restrict__ eps, const T* __restrict__ c, T drift,
                                                                const T* __restrict__ p, const T* __restrict__ q_far,
                                                                const T* __restrict__ p_far, int want_sums, long long N,
                                                                long long nchunks, double* __restrict__ partial)
{
    constexpr int E = HMC_BYTES / sizeof(T);
    constexpr long long SPAN = (long long)HMC_THREADS * E;
    __shared__ double acc[3][HMC_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool do_drift = drift != (T)0;
    const T* q_now = q_out != nullptr ? q_out : q_in;        // where the position stands after this call
    const bool z_vec = aligned16(z), qi_vec = aligned16(q_in), qo_vec = aligned16(q_out), qn_vec = aligned16(q_now), e_vec = aligned16(eps),
               c_vec = aligned16(c), p_vec = aligned16(p), qf_vec = aligned16(q_far), pf_vec = aligned16(p_far);
    double mine = 0.0, far = 0.0, near = 0.0;
    for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const long long c0 = chunk * SPAN;
        T xz[E], xq[E];
        hmc_load<T>(z, c0, N, z_vec, xz);
        if (do_drift) {
            T xe[E], xc[E];
            hmc_load<T>(q_in, c0, N, qi_vec, xq);
            if (eps != nullptr) hmc_load<T>(eps, c0, N, e_vec, xe);
            if (c != nullptr) hmc_load<T>(c, c0, N, c_vec, xc);
            const unsigned cover = mass_cover<T>(blocks, nblocks, N, c0);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const T de = eps != nullptr ? drift * xe[i] : drift;
                const T v = c != nullptr ? xc[i] * xz[i] : xz[i];
                xq[i] = tfma<T>(de, v, xq[i]);
            }
            if (cover == 0u) {
                hmc_store<T>(q_out, c0, N, qo_vec, xq);
            } else {                                         // a lane with elements in a block: theirs are already in q_out
                constexpr int W = Vec16<T>::W;
#pragma unroll
                for (int g = 0; g < HMC_GROUPS; ++g)
#pragma unroll
                    for (int i = 0; i < W; ++i) {
                        const long long e = c0 + (long long)(g * HMC_THREADS + tid) * W + i;
                        if (e < N) {
                            if ((cover >> (g * W + i)) & 1u) xq[g * W + i] = q_out[e];
                            else q_out[e] = xq[g * W + i];
                        }
                    }
            }
        } else if (DOTS) {
            hmc_load<T>(q_now, c0, N, qn_vec, xq);
        }
        if (want_sums) mine += hmc_sumsq<T>(xz);
        if (DOTS) {
            T xf[E], xp[E];
            hmc_load<T>(q_far, c0, N, qf_vec, xf);
#pragma unroll
            for (int i = 0; i < E; ++i) xq[i] = xq[i] - xf[i];
            hmc_load<T>(p_far, c0, N, pf_vec, xf);
            hmc_load<T>(p, c0, N, p_vec, xp);
            T a = (T)0, b = (T)0;
#pragma unroll
            for (int i = 0; i < E; ++i) {
                a = tfma<T>(xq[i], xf[i], a);
                b = tfma<T>(xq[i], xp[i], b);
            }
            far += wave_sum((double)a);
            near += wave_sum((double)b);
        }
    }
    if (want_sums) {
        if (lane == 0) {
            acc[0][wave] = mine;
            if (DOTS) acc[1][wave] = far, acc[2][wave] = near;
        }
        __syncthreads();
        if (tid < (DOTS ? 3 : 1)) partial[(size_t)tid * gridDim.x + blockIdx.x] = ((acc[tid][0] + acc[tid][1]) + acc[tid][2]) + acc[tid][3];
    }
}

// wave k of `nsums`: out[k] = sum_b partial[k nb + b], the first halved
__global__ __launch_bounds__(192) void mass_final_kernel(const double* __restrict__ partial, int nb, int nsums, double* __restrict__ out)
{
    hmc_final(partial, nb, nsums, out);
}

template <typename T>
static int mass_project(long long N, const mass_block* blocks, int nblocks, const void* p_in, const void* g, const void* eps,
                        const void* c, double kick, void* p_out, void* z, hipStream_t st, int dtype)
{
    const int nb = hmc_blocks(N, dtype);
    if (nb > 0)
        hipLaunchKernelGGL((mass_kick_kernel<T>), dim3((unsigned)nb), dim3(HMC_THREADS), 0, st, (const T*)p_in, (const T*)g,
                           (const T*)eps, (const T*)c, (T)kick, (T*)p_out, (T*)z, N, hmc_chunks(N, dtype));
    if (nb > 0 && nblocks > 0)
        hipLaunchKernelGGL((mass_upper_kernel<T>), dim3((unsigned)mass_grid(N, nblocks, 8 * Vec16<T>::W)), dim3(HMC_THREADS), 0, st,
                           blocks, nblocks, N, (const T*)(kick != 0.0 ? p_out : p_in), (T*)z);
    return check_launch();
}

template <typename T>
static int mass_drift(long long N, const mass_block* blocks, int nblocks, const void* z, const void* q_in, const void* eps, const void* c,
                      double drift, void* q_out, const void* p, const void* q_far, const void* p_far, double* out, double* part,
                      hipStream_t st, int dtype)
{
    const int nb = hmc_blocks(N, dtype);
    const long long nchunks = hmc_chunks(N, dtype);
    const bool dots = p != nullptr, sums = out != nullptr;
    if (nb > 0 && nblocks > 0 && drift != 0.0)
        hipLaunchKernelGGL((mass_lower_kernel<T>), dim3((unsigned)mass_grid(N, nblocks, MASS_ROWS)), dim3(HMC_THREADS), 0, st, blocks,
                           nblocks, N, (const T*)z, (const T*)q_in, (T*)q_out, (const T*)eps, (T)drift);
    if (nb > 0)
        with_bool(dots && sums, [&](auto d) {
            hipLaunchKernelGGL((mass_drift_kernel<T, decltype(d)::value>), dim3((unsigned)nb), dim3(HMC_THREADS), 0, st, blocks, nblocks,
                               (const T*)z, (const T*)q_in, (T*)q_out, (const T*)eps, (const T*)c, (T)drift, (const T*)p,
                               (const T*)q_far, (const T*)p_far, sums ? 1 : 0, N, nchunks, part);
        });
    if (sums) hipLaunchKernelGGL(mass_final_kernel, dim3(1), dim3(192), 0, st, (const double*)part, nb, dots ? 3 : 1, out);
    return check_launch();
}

static bool mass_size_ok(long long N, int nblocks)
{
    return hmc_size_ok(N) && nblocks >= 0 && mass_grid(N, nblocks, MASS_ROWS) <= 0x7fffffffLL;
}

} // namespace rime

using namespace rime;

// three partials per work-group
extern "C" size_t rime_mass_workspace(long long N) { return hmc_workspace_bytes(N, 3); }

extern "C" int rime_mass_project(int dtype, long long N, const void* blocks, int nblocks, const void* p_in, const void* g,
                                 const void* eps, const void* c, double kick, void* p_out, void* z, void* stream)
{
    if (!real_dtype_ok(dtype) || !mass_size_ok(N, nblocks) || (nblocks > 0 && !blocks) || !p_in || !z) return RIME_EINVAL;
    if (!(kick == kick)) return RIME_EINVAL;
    if (kick != 0.0 && (!g || !p_out)) return RIME_EINVAL;
    const size_t bytes = (size_t)N * real_bytes(dtype);
    if (kick != 0.0 && hmc_overlap(p_out, p_in, bytes)) return RIME_EINVAL;
    if (hmc_overlap(z, p_in, bytes) || (kick != 0.0 && hmc_overlap(z, p_out, bytes))) return RIME_EINVAL;
    if (hmc_flag_underflows(dtype, kick)) return RIME_EINVAL;
    return with_real(dtype, [&](auto t) {
        return mass_project<decltype(t)>(N, (const mass_block*)blocks, nblocks, p_in, g, eps, c, kick, p_out, z, as_stream(stream), dtype);
    });
}

extern "C" int rime_mass_drift(int dtype, long long N, const void* blocks, int nblocks, const void* z, const void* q_in,
                               const void* eps, const void* c, double drift, void* q_out, const void* p, const void* q_far,
                               const void* p_far, double* out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!real_dtype_ok(dtype) || !mass_size_ok(N, nblocks) || (nblocks > 0 && !blocks) || !z) return RIME_EINVAL;
    if (!(drift == drift)) return RIME_EINVAL;
    if (drift != 0.0 && (!q_in || !q_out)) return RIME_EINVAL;
    const int given = (p != nullptr) + (q_far != nullptr) + (p_far != nullptr);
    if (given != 0 && given != 3) return RIME_EINVAL;
    if (given == 3 && out != nullptr && !q_in && !q_out) return RIME_EINVAL;           // projections of no position
    const size_t bytes = (size_t)N * real_bytes(dtype);
    if (drift != 0.0 && (hmc_overlap(q_out, z, bytes) || (q_out != q_in && hmc_overlap(q_out, q_in, bytes)))) return RIME_EINVAL;
    if (out != nullptr && (!workspace || workspace_bytes < rime_mass_workspace(N))) return RIME_EWORKSPACE;
    if (hmc_flag_underflows(dtype, drift)) return RIME_EINVAL;
    if (drift == 0.0 && out == nullptr) return RIME_OK;                                  // nothing to do
    return with_real(dtype, [&](auto t) {
        return mass_drift<decltype(t)>(N, (const mass_block*)blocks, nblocks, z, q_in, eps, c, drift, q_out, p, q_far, p_far, out,
                                       (double*)workspace, as_stream(stream), dtype);
    });
}
