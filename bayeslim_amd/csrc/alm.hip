// alm.hip -- a_lm -> pixel transform and its adjoint (gfx950).
//
//   fwd : out[r, j]  = sum_c ( are[r,c] Yre[c,j] - aim[r,c] Yim[c,j] ) = Re( alm @ Ylm )
//   bwd : galm[r, c] = sum_j gout[r, j] * conj(Ylm[c, j])
// Replaces AlmModel.forward_alm (sph_harm.py:1342-1372, real_output=True) and the einsum
// backward autograd derives for it.
//
// Both are real GEMMs against the interleaved complex Ylm [Ncoeff, Npix, 2] viewed as a
// (2 Ncoeff) x Npix matrix (fwd: K = 2 Ncoeff) or its transpose (bwd: K = Npix).  Ylm is the
// only large operand (C3: 3.3 GB) and is streamed exactly once per <= BM rows of alm; the
// alm / gout operand is small and stays in L2.
//
// float32: exact-f32 matrix cores (v_mfma_f32_32x32x2_f32; one complex coefficient / one pixel
// pair per K-step), operands staged through LDS in fragment order, Ylm streamed once.
// float64 (parity oracle precision) and tiny shapes: VALU register-tiled kernels.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "rime_common.h"

namespace rime {

// ---------------------------------------------------------------------------------------
// forward: lane = pixel, RTA rows per block (grid.y walks row blocks)
// ---------------------------------------------------------------------------------------
template <typename T, int RTA>
__global__ void __launch_bounds__(256)
alm2pix_fwd_kernel(const T* __restrict__ alm, const T* __restrict__ Ylm, int R, int Ncoeff,
                   int Npix, T* __restrict__ out)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int r0 = blockIdx.y * RTA;
    const int jc = min(j, Npix - 1);
    T acc[RTA];
#pragma unroll
    for (int i = 0; i < RTA; ++i) acc[i] = T(0);
    for (int c = 0; c < Ncoeff; ++c) {
        const T yre = Ylm[((size_t)c * Npix + jc) * 2];
        const T yim = Ylm[((size_t)c * Npix + jc) * 2 + 1];
#pragma unroll
        for (int i = 0; i < RTA; ++i) {
            const int r = min(r0 + i, R - 1);                  // wave-uniform -> scalar loads
            const T are = alm[((size_t)r * Ncoeff + c) * 2];
            const T aim = alm[((size_t)r * Ncoeff + c) * 2 + 1];
            acc[i] = tfma<T>(are, yre, acc[i]);
            acc[i] = tfma<T>(-aim, yim, acc[i]);
        }
    }
    if (j < Npix) {
#pragma unroll
        for (int i = 0; i < RTA; ++i)
            if (r0 + i < R) out[(size_t)(r0 + i) * Npix + j] = acc[i];
    }
}

// ---------------------------------------------------------------------------------------
// backward: block = CT coefficients x RTB rows; lanes stride over pixels; deterministic
// wave-shuffle + LDS reduction at the end
// ---------------------------------------------------------------------------------------
template <typename T, int CT, int RTB>
__global__ void __launch_bounds__(256)
alm2pix_bwd_kernel(const T* __restrict__ gout, const T* __restrict__ Ylm, int R, int Ncoeff,
                   int Npix, T* __restrict__ galm)
{
    __shared__ T red[4][CT * RTB * 2];
    const int c0 = blockIdx.x * CT;
    const int r0 = blockIdx.y * RTB;
    T acc[CT][RTB][2];
#pragma unroll
    for (int a = 0; a < CT; ++a)
#pragma unroll
        for (int i = 0; i < RTB; ++i) { acc[a][i][0] = T(0); acc[a][i][1] = T(0); }
    for (int j = threadIdx.x; j < Npix; j += blockDim.x) {
        T g[RTB];
#pragma unroll
        for (int i = 0; i < RTB; ++i) g[i] = gout[(size_t)min(r0 + i, R - 1) * Npix + j];
#pragma unroll
        for (int a = 0; a < CT; ++a) {
            const int c = min(c0 + a, Ncoeff - 1);
            const T yre = Ylm[((size_t)c * Npix + j) * 2];
            const T yim = Ylm[((size_t)c * Npix + j) * 2 + 1];
#pragma unroll
            for (int i = 0; i < RTB; ++i) {
                acc[a][i][0] = tfma<T>(g[i], yre, acc[a][i][0]);
                acc[a][i][1] = tfma<T>(-g[i], yim, acc[a][i][1]);
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < CT; ++a)
#pragma unroll
        for (int i = 0; i < RTB; ++i)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                T v = acc[a][i][q];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
                if (lane == 0) red[wave][(a * RTB + i) * 2 + q] = v;
            }
    __syncthreads();
    const int nw = blockDim.x >> 6;
    for (int e = threadIdx.x; e < CT * RTB * 2; e += blockDim.x) {
        T v = T(0);
        for (int w = 0; w < nw; ++w) v += red[w][e];
        const int q = e & 1, i = (e >> 1) % RTB, a = (e >> 1) / RTB;
        if (c0 + a < Ncoeff && r0 + i < R)
            galm[((size_t)(r0 + i) * Ncoeff + c0 + a) * 2 + q] = v;
    }
}


// ---------------------------------------------------------------------------------------
// f32 MFMA kernels.  v_mfma_f32_32x32x2_f32: D[32x32] += A[32x2] * B[2x32]; lane l holds
// A[i = l&31][k = l>>5], B[k = l>>5][j = l&31]; D[row = (reg&3) + 8*(reg>>2) + 4*(l>>5)][col = l&31].
// ---------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int MT> __device__ __forceinline__ void zero(f32x16 (&acc)[MT])
{
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[m][e] = 0.f;
}

// the row of accumulator element e of a lane's row tile m (the D layout above), tiles from row r0 on
__device__ __forceinline__ int tile_row(int r0, int m, int e, int lane)
{
    return r0 + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
}

// forward epilogue: the lane's column `col` of MT row tiles into one output plane [R][Npix]; the f16-split kernels
// undo the row scales and y_scale on the way
template <int MT>
__device__ __forceinline__ void store_fwd_tile(const f32x16 (&acc)[MT], float* plane, int r0, int R, int Npix,
                                               int col, int lane)
{
    if (col < Npix) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = tile_row(r0, m, e, lane);
                if (row < R) plane[(size_t)row * Npix + col] = acc[m][e];
            }
    }
}

template <int MT>
__device__ __forceinline__ void store_fwd_tile(const f32x16 (&acc)[MT], float* plane, int r0, int R, int Npix,
                                               int col, int lane, const float* __restrict__ inv_scale, float y_scale)
{
    if (col < Npix) {
        const float iy = 1.0f / y_scale;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = tile_row(r0, m, e, lane);
                if (row < R) plane[(size_t)row * Npix + col] = acc[m][e] * inv_scale[row] * iy;
            }
    }
}

// forward: out[r, j] = sum_c are[r,c] Yre[c,j] - aim[r,c] Yim[c,j].
//   K-step = one coefficient c (k = re / im).  Block = 4 waves x 32 pixels; every wave keeps
//   MT row tiles (MT*32 rows) of accumulators.  alm chunks [CT coeffs][re,-im][rows] are staged in
//   LDS (row-fastest, +1 pad: conflict-free both ways); Ylm fragments come straight from global
//   memory: the 64 lanes of a wave read 64 consecutive floats (32 pixels x re/im) per coefficient.
template <int MT>
__global__ void __launch_bounds__(256)
alm2pix_fwd_mfma_kernel(const float* __restrict__ alm, const float* __restrict__ Ylm, int R,
                        int Ncoeff, int Npix, float* __restrict__ out)
{
    constexpr int CT = 32;                 // coefficients per LDS chunk
    constexpr int ROWS = MT * 32;
    constexpr int RP = ROWS + 1;           // padded row count
    __shared__ float a_lds[CT * 2 * RP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.y * ROWS;
    const int j0 = (blockIdx.x * 4 + wave) * 32;
    const int jl = min(j0 + (lane & 31), Npix - 1);
    const int ri = lane >> 5;
    f32x16 acc[MT];
    zero(acc);

    // Ylm fragments of one chunk live in registers and are fetched one chunk ahead, so the
    // 32 independent 256-B reads of chunk k+1 are in flight under the MFMAs of chunk k
    float bcur[CT], bnxt[CT];
    auto load_b = [&](int c0, float (&b)[CT]) {
#pragma unroll
        for (int cc = 0; cc < CT; ++cc) {
            const int c = min(c0 + cc, Ncoeff - 1);
            b[cc] = Ylm[((size_t)c * Npix + jl) * 2 + ri];
        }
    };
    load_b(0, bcur);
    for (int c0 = 0; c0 < Ncoeff; c0 += CT) {
        __syncthreads();
        // stage alm[r0 .. r0+ROWS, c0 .. c0+CT] -> a_lds[(cc*2+q)*RP + row], imaginary part negated
        // (coefficients past Ncoeff are zero-filled, so the clamped Ylm prefetch contributes 0)
        for (int i = tid; i < ROWS * CT * 2; i += 256) {
            const int e = i % (CT * 2), row = i / (CT * 2);
            const int c = c0 + (e >> 1), r = r0 + row;
            float v = 0.f;
            if (c < Ncoeff && r < R) v = alm[((size_t)r * Ncoeff + c) * 2 + (e & 1)];
            a_lds[e * RP + row] = (e & 1) ? -v : v;
        }
        if (c0 + CT < Ncoeff) load_b(c0 + CT, bnxt);
        __syncthreads();
#pragma unroll
        for (int cc = 0; cc < CT; ++cc) {
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float a = a_lds[(cc * 2 + ri) * RP + m * 32 + (lane & 31)];
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bcur[cc], acc[m], 0, 0, 0);
            }
        }
#pragma unroll
        for (int cc = 0; cc < CT; ++cc) bcur[cc] = bnxt[cc];
    }
    RIME_MFMA_SETTLE();
    store_fwd_tile(acc, out, r0, R, Npix, j0 + (lane & 31), lane);
}

// backward: galm[r, (c,q)] = sum_j gout[r, j] * Y[c, j, q] * (q ? -1 : +1).
//   K-step = two pixels.  Block = one tile of 16 coefficients (32 (c,q) columns) x MT*32 rows,
//   wave m owns row tile m; grid.y splits the pixel axis (partials in `part`, reduced afterwards).
//   gout and Ylm tiles of KT pixels are staged in LDS: gout [row][KT+1] (A fragments: lanes =
//   rows, odd stride), Ylm [coef][KT*2+2] (B fragments: lanes = (c,q), stride = 2 mod 32).
template <int MT>
__global__ void __launch_bounds__(64 * MT)
alm2pix_bwd_mfma_kernel(const float* __restrict__ gout, const float* __restrict__ Ylm, int R,
                        int Ncoeff, int Npix, int pix_per_split, float* __restrict__ part)
{
    constexpr int KT = 64;
    constexpr int ROWS = MT * 32;
    constexpr int GP = KT + 1;
    constexpr int YP = KT * 2 + 2;
    __shared__ float g_lds[ROWS * GP];
    __shared__ float y_lds[16 * YP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthr = 64 * MT;
    const int c0 = blockIdx.x * 16;
    const int r0 = blockIdx.z * ROWS;
    const int jbeg = blockIdx.y * pix_per_split;
    const int jend = min(Npix, jbeg + pix_per_split);
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const int n = lane & 31, kk = lane >> 5;
    // global -> registers -> LDS, one tile ahead: the loads of tile t+1 are issued before the
    // MFMAs of tile t and written to LDS after them (single LDS buffer, two barriers per tile)
    constexpr int NG = (ROWS * KT) / (64 * MT);        // gout values per thread per tile (= 32)
    constexpr int NY = (16 * KT * 2) / (64 * MT);      // Ylm values per thread per tile
    float gq[NG], yq[NY];
    auto fetch = [&](int jt) {
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const int i = tid + u * nthr;
            const int jj = i % KT, row = i / KT;
            const int r = r0 + row, j = jt + jj;
            gq[u] = (r < R && j < jend) ? gout[(size_t)r * Npix + j] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < NY; ++u) {
            const int i = tid + u * nthr;
            const int e = i % (KT * 2), cc = i / (KT * 2);
            const int c = c0 + cc, j = jt + (e >> 1);
            const float v = (c < Ncoeff && j < jend) ? Ylm[((size_t)c * Npix + jt) * 2 + e] : 0.f;
            yq[u] = (e & 1) ? -v : v;
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const int i = tid + u * nthr;
            g_lds[(i / KT) * GP + (i % KT)] = gq[u];
        }
#pragma unroll
        for (int u = 0; u < NY; ++u) {
            const int i = tid + u * nthr;
            y_lds[(i / (KT * 2)) * YP + (i % (KT * 2))] = yq[u];
        }
    };
    if (jbeg < jend) fetch(jbeg);
    for (int jt = jbeg; jt < jend; jt += KT) {
        __syncthreads();                     // previous tile fully consumed
        commit();
        __syncthreads();
        if (jt + KT < jend) fetch(jt + KT);
#pragma unroll 8
        for (int jj = 0; jj < KT; jj += 2) {
            const float a = g_lds[(wave * 32 + n) * GP + jj + kk];
            const float b = y_lds[(n >> 1) * YP + (jj + kk) * 2 + (n & 1)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
    // D[row][col = (c,q)] -> part[split][r][c][q]
    const int c = c0 + (n >> 1);
    RIME_MFMA_SETTLE();
    if (c < Ncoeff) {
        float* dst = part + (size_t)blockIdx.y * R * Ncoeff * 2;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = r0 + wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
            if (row < R) dst[((size_t)row * Ncoeff + c) * 2 + (n & 1)] = acc[e];
        }
    }
}

// ---------------------------------------------------------------------------------------
// float32 fast path: f16 hi/lo split operands on v_mfma_f32_32x32x16_f16 (three cross products,
// f32 accumulation -- the scheme of fringe_mfma.hip; 22 significant bits, 16x the f32-MFMA rate), so
// that both directions run at the speed Ylm streams from HBM instead of the f32 matrix-core rate.
// The small operand (alm rows / gout rows) is scaled per row by a power of two, split once by
// split_rows_kernel into A-fragment order in a workspace and copied to LDS by the GEMM blocks; the
// streamed operand (Ylm, scaled by the caller's power of two y_scale) is split in registers by the
// lane that loaded it.
// ---------------------------------------------------------------------------------------
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split2h(float a, float b, uint32_t& hi, uint32_t& lo)
{
    auto h = __builtin_amdgcn_cvt_pkrtz(a, b);
    hi = __builtin_bit_cast(uint32_t, h);
    auto l = __builtin_amdgcn_cvt_pkrtz(a - (float)h[0], b - (float)h[1]);
    lo = __builtin_bit_cast(uint32_t, l);
}
#define ALM_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0)

// eight consecutive K values -> the hi / lo granules of a fragment
__device__ __forceinline__ void split8(const float (&v)[8], uint4& hi, uint4& lo)
{
    split2h(v[0], v[1], hi.x, lo.x); split2h(v[2], v[3], hi.y, lo.y);
    split2h(v[4], v[5], hi.z, lo.z); split2h(v[6], v[7], hi.w, lo.w);
}

// eight pixels of one Ylm row (four float4 = 2 x (re, im) each) x y_scale -> the re and im B fragments of the backward
__device__ __forceinline__ void split_y4(const float4 (&y)[4], float y_scale, uint4& rh, uint4& rl, uint4& ih, uint4& il)
{
    split2h(y[0].x * y_scale, y[0].z * y_scale, rh.x, rl.x);
    split2h(y[1].x * y_scale, y[1].z * y_scale, rh.y, rl.y);
    split2h(y[2].x * y_scale, y[2].z * y_scale, rh.z, rl.z);
    split2h(y[3].x * y_scale, y[3].z * y_scale, rh.w, rl.w);
    split2h(y[0].y * y_scale, y[0].w * y_scale, ih.x, il.x);
    split2h(y[1].y * y_scale, y[1].w * y_scale, ih.y, il.y);
    split2h(y[2].y * y_scale, y[2].w * y_scale, ih.z, il.z);
    split2h(y[3].y * y_scale, y[3].w * y_scale, ih.w, il.w);
}

// the three cross products of one K step (lo x lo is below the f32 accumulation error), forward and backward
__device__ __forceinline__ void mfma3(uint4 ah, uint4 al, uint4 bh, uint4 bl, f32x16& acc)
{
    acc = ALM_MFMA(ah, bh, acc);
    acc = ALM_MFMA(ah, bl, acc);
    acc = ALM_MFMA(al, bh, acc);
}

__device__ __forceinline__ void mfma6(uint4 ah, uint4 al, uint4 rh, uint4 rl, uint4 ih, uint4 il, f32x16& accr, f32x16& acci)
{
    accr = ALM_MFMA(ah, rh, accr);
    acci = ALM_MFMA(ah, ih, acci);
    accr = ALM_MFMA(ah, rl, accr);
    acci = ALM_MFMA(ah, il, acci);
    accr = ALM_MFMA(al, rh, accr);
    acci = ALM_MFMA(al, ih, acci);
}

// backward epilogue: the lane's coefficient c of MT row tiles into one partial plane [R][Ncoeff][re, im], row scales and
// y_scale undone, the imaginary part conjugated
template <int MT>
__device__ __forceinline__ void store_bwd_tile(const f32x16 (&accr)[MT], const f32x16 (&acci)[MT], float* __restrict__ plane,
                                               int r0, int R, int Ncoeff, int c, int lane,
                                               const float* __restrict__ inv_scale, float y_scale)
{
    if (c < Ncoeff) {
        const float iy = 1.0f / y_scale;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = tile_row(r0, m, e, lane);
                if (row < R) {
                    const float sc = inv_scale[row] * iy;
                    *reinterpret_cast<float2*>(plane + ((size_t)row * Ncoeff + c) * 2) =
                        make_float2(accr[m][e] * sc, -acci[m][e] * sc);
                }
            }
    }
}

// register-staged kernels: this thread's share of the pre-split row granules of KS K steps from s0 on, (ks * 2 + h) * ROWS
// + row in block order, zero beyond the `nsteps` K steps the images hold
template <int ROWS, int KS>
__device__ __forceinline__ void fetch_granules(const uint4* __restrict__ img_hi, const uint4* __restrict__ img_lo, int Rpad,
                                               int r0, int s0, int nsteps, int tid, uint4 (&ahq)[(2 * KS * ROWS + 255) / 256],
                                               uint4 (&alq)[(2 * KS * ROWS + 255) / 256])
{
    constexpr int NG = 2 * KS * ROWS, PT = (NG + 255) / 256;
#pragma unroll
    for (int u = 0; u < PT; ++u) {
        const int i = tid + u * 256;
        const int row = i % ROWS, g = i / ROWS;        // g = ks * 2 + h
        const int sg = s0 * 2 + g;
        const bool ok = (NG % 256 == 0 || i < NG) && sg < nsteps * 2;
        ahq[u] = ok ? img_hi[(size_t)sg * Rpad + r0 + row] : make_uint4(0, 0, 0, 0);
        alq[u] = ok ? img_lo[(size_t)sg * Rpad + r0 + row] : make_uint4(0, 0, 0, 0);
    }
}

// Row operand X [R][L] (f32) -> per-row power-of-two scale, f16 hi / lo images in A-fragment order:
// granule ((s * 2 + h) * Rpad + r) holds k = 16 s + 8 h + 0..7 of row r (zero beyond L / R).
// `neg_odd`: negate odd k (the imaginary parts of alm: out = are Yre - aim Yim).
// Two kernels so that long rows (gout: Npix values) spread over the chip: row_absmax_kernel
// (grid = rows x segments, integer atomicMax on the bit patterns of |x|: order-independent) and
// split_rows_kernel (same grid).
constexpr int SPLIT_SEG = 4096;                        // values per block

__global__ void __launch_bounds__(256)
row_absmax_kernel(const float* __restrict__ X, int R, int L, unsigned int* __restrict__ rowmax)
{
    const int r = blockIdx.x, tid = threadIdx.x;
    const int k0 = blockIdx.y * SPLIT_SEG, k1 = min(L, k0 + SPLIT_SEG);
    float m = 0.f;
    for (int i = k0 + tid; i < k1; i += 256) m = fmaxf(m, fabsf(X[(size_t)r * L + i]));
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((tid & 63) == 0 && m > 0.f) atomicMax(rowmax + r, __float_as_uint(m));
}

__global__ void __launch_bounds__(256)
split_rows_kernel(const float* __restrict__ X, int R, int L, int Rpad, int neg_odd,
                  const unsigned int* __restrict__ rowmax, uint4* __restrict__ img_hi,
                  uint4* __restrict__ img_lo, float* __restrict__ inv_scale)
{
    const int r = blockIdx.x, tid = threadIdx.x;
    const int nsteps = (L + 15) / 16;
    float scale = 1.0f;
    if (r < R) {
        const float m = __uint_as_float(rowmax[r]);
        if (m > 0.f) scale = exp2f(fminf(fmaxf(floorf(log2f(8192.0f / m)), -100.f), 100.f));   // max|x| * scale in [2^12, 2^13]
    }
    if (blockIdx.y == 0 && tid == 0) inv_scale[r] = (r < R) ? 1.0f / scale : 0.f;
    const int g0 = blockIdx.y * (SPLIT_SEG / 8), g1 = min(nsteps * 2, g0 + SPLIT_SEG / 8);
    for (int g = g0 + tid; g < g1; g += 256) {
        float v[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int k = g * 8 + jj;
            float x = (r < R && k < L) ? X[(size_t)r * L + k] * scale : 0.f;
            v[jj] = (neg_odd && (jj & 1)) ? -x : x;
        }
        uint4 hi, lo;
        split8(v, hi, lo);
        img_hi[(size_t)g * Rpad + r] = hi;
        img_lo[(size_t)g * Rpad + r] = lo;
    }
}

// Long rows (round 3; gout: 128 rows of 49 152 values in front of every C3-shape backward): the two kernels above cost 64 us
// there, mostly because every 16-byte granule store of split_rows_kernel lands 2 KB from the next (granule-major images,
// one block per row).  Two launches without atomics or memset instead: the scale of every row by one block per row
// (coalesced float4 reads), then a TILED split -- a block reads 64 rows x 32 granules along the rows (a wave reads 2 KB
// contiguous pieces), turns the tile through LDS and writes it granule-major, 64 rows x 16 B = 1 KB contiguous per store.
__global__ void __launch_bounds__(256)
row_scale_alm_kernel(const float* __restrict__ X, int R, int L, float* __restrict__ scale, float* __restrict__ inv_scale)
{
    __shared__ float wmax[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    float m = 0.f;
    if (r < R) {
        const float* row = X + (size_t)r * L;
        if ((L & 3) == 0 && (reinterpret_cast<uintptr_t>(row) & 15) == 0) {
            for (int i = tid; i < L / 4; i += 256) {
                const float4 v = reinterpret_cast<const float4*>(row)[i];
                m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
            }
        } else {
            for (int i = tid; i < L; i += 256) m = fmaxf(m, fabsf(row[i]));
        }
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((tid & 63) == 0) wmax[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
        float sc = 1.0f;
        if (r < R && m > 0.f) sc = exp2f(fminf(fmaxf(floorf(log2f(8192.0f / m)), -100.f), 100.f));   // max|x| * scale in [2^12, 2^13]
        scale[r] = sc;
        inv_scale[r] = (r < R) ? 1.0f / sc : 0.f;
    }
}

__global__ void __launch_bounds__(256)
split_rows_tiled_kernel(const float* __restrict__ X, int R, int L, int Rpad, int neg_odd, const float* __restrict__ scale,
                        uint4* __restrict__ img_hi, uint4* __restrict__ img_lo)
{
    __shared__ uint4 t_hi[32 * 65], t_lo[32 * 65];     // [granule][row], rows padded to 65: the turn is (nearly) conflict-free
    const int tid = threadIdx.x;
    const int g0 = blockIdx.x * 32, r0 = blockIdx.y * 64;
    const int ngran = ((L + 15) / 16) * 2;
    const int gl = tid & 31;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int rr = (tid >> 5) + 8 * it, r = r0 + rr, g = g0 + gl;
        float v[8];
        const float sc = r < R ? scale[r] : 0.f;
        const size_t base = (size_t)r * L + (size_t)g * 8;
        if (r < R && g * 8 + 7 < L && ((base & 3) == 0)) {
            const float4 a = *reinterpret_cast<const float4*>(X + base), b = *reinterpret_cast<const float4*>(X + base + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) v[jj] = (r < R && g * 8 + jj < L) ? X[base + jj] : 0.f;
        }
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) { v[jj] *= sc; if (neg_odd && (jj & 1)) v[jj] = -v[jj]; }
        uint4 hi, lo;
        split8(v, hi, lo);
        t_hi[gl * 65 + rr] = hi;
        t_lo[gl * 65 + rr] = lo;
    }
    __syncthreads();
    const int rr = tid & 63;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int gq = (tid >> 6) + 4 * it, g = g0 + gq;
        if (g < ngran) {
            img_hi[(size_t)g * Rpad + r0 + rr] = t_hi[gq * 65 + rr];
            img_lo[(size_t)g * Rpad + r0 + rr] = t_lo[gq * 65 + rr];
        }
    }
}

// forward: out[r, j] = sum_k A[r, k] Y[k, j], k = (c, re|im).  Block = 4 waves x 32 pixels, MT row
// tiles per wave; per chunk of 32 coefficients (4 K steps) the block copies the pre-split A
// granules to LDS (fetched one chunk ahead into registers) and every lane splits the 16 Ylm values
// it loaded (also one chunk ahead): 12 MT MFMAs against ~130 VALU instructions per chunk and wave.
template <int MT>
__global__ void __launch_bounds__(256)
alm2pix_fwd_f16_kernel(const uint4* __restrict__ a_hi, const uint4* __restrict__ a_lo,
                       const float* __restrict__ inv_scale, const float* __restrict__ Ylm, float y_scale,
                       int R, int Rpad, int Ncoeff, int Npix, float* __restrict__ out)
{
    constexpr int ROWS = MT * 32;
    constexpr int NG = 8 * ROWS;                       // granules per image and chunk: (ks, h, row)
    constexpr int PT = NG / 256;                       // per thread
    __shared__ uint4 lds_hi[NG], lds_lo[NG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.y * ROWS;
    const int j0 = (blockIdx.x * 4 + wave) * 32;
    const int jl = min(j0 + (lane & 31), Npix - 1);
    const int h = lane >> 5;
    const int nsteps = (2 * Ncoeff + 15) / 16;
    f32x16 acc[MT];
    zero(acc);

    float2 bcur[16], bnxt[16];                        // [ks * 4 + i]: coefficient c0 + 8 ks + 4 h + i
    uint4 ahq[PT], alq[PT];
    auto load_b = [&](int c0, float2 (&b)[16]) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int c = c0 + 8 * (u >> 2) + 4 * h + (u & 3);
            b[u] = (c < Ncoeff) ? *reinterpret_cast<const float2*>(Ylm + ((size_t)c * Npix + jl) * 2)
                                : make_float2(0.f, 0.f);
        }
    };
    auto fetch_a = [&](int s0) {                       // K steps s0 .. s0 + 3
        fetch_granules<ROWS, 4>(a_hi, a_lo, Rpad, r0, s0, nsteps, tid, ahq, alq);
    };
    load_b(0, bcur);
    fetch_a(0);
    for (int c0 = 0; c0 < Ncoeff; c0 += 32) {
        __syncthreads();                               // previous chunk consumed
#pragma unroll
        for (int u = 0; u < PT; ++u) { lds_hi[tid + u * 256] = ahq[u]; lds_lo[tid + u * 256] = alq[u]; }
        __syncthreads();
        if (c0 + 32 < Ncoeff) { load_b(c0 + 32, bnxt); fetch_a(c0 / 8 + 4); }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            uint4 bh, bl;
            split2h(bcur[ks * 4 + 0].x * y_scale, bcur[ks * 4 + 0].y * y_scale, bh.x, bl.x);
            split2h(bcur[ks * 4 + 1].x * y_scale, bcur[ks * 4 + 1].y * y_scale, bh.y, bl.y);
            split2h(bcur[ks * 4 + 2].x * y_scale, bcur[ks * 4 + 2].y * y_scale, bh.z, bl.z);
            split2h(bcur[ks * 4 + 3].x * y_scale, bcur[ks * 4 + 3].y * y_scale, bh.w, bl.w);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int gi = (ks * 2 + h) * ROWS + m * 32 + (lane & 31);
                mfma3(lds_hi[gi], lds_lo[gi], bh, bl, acc[m]);
            }
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) bcur[u] = bnxt[u];
    }
    RIME_MFMA_SETTLE();
    store_fwd_tile(acc, out, r0, R, Npix, j0 + (lane & 31), lane, inv_scale, y_scale);
}

// backward: galm[r, c, q] = sum_j gout[r, j] Y[c, j, q] (q ? -1 : +1).  K = pixels (16 per MFMA).
// Wave = 32 coefficients x MT row tiles with separate accumulators for the re and im columns (a
// B fragment needs 8 consecutive pixels of ONE coefficient row, and both components are used).
// Block = 4 waves = 128 coefficients.  Per chunk of 32 pixels the block stages the Ylm tile
// [128 coefficients][32 px][re,im] through LDS -- global loads are 256-B row segments, 16 B per lane,
// fetched one chunk ahead -- together with the pre-split gout granules; the 32-pixel chunks are
// dealt cyclically to S blocks (partials reduced by alm_reduce_kernel).  Measured 2.0 TB/s of Ylm
// at R = 128 and 3.5 TB/s at R = 4: latency-bound (one chunk = 32 KB per block in flight, ~7 us
// loaded latency); per-lane row streaming without LDS staging and contiguous split ranges are
// within 5 % of this.
template <int MT>
__global__ void __launch_bounds__(256, 2)       // two blocks per CU: the kernel is bound by the Ylm bytes in flight
alm2pix_bwd_f16_kernel(const uint4* __restrict__ g_hi, const uint4* __restrict__ g_lo,
                       const float* __restrict__ inv_scale, const float* __restrict__ Ylm, float y_scale,
                       int R, int Rpad, int Ncoeff, int Npix, int S, float* __restrict__ part)
{
    constexpr int ROWS = MT * 32;
    constexpr int NG = 4 * ROWS;                       // gout granules per image and chunk of 2 K steps
    constexpr int PT = (NG + 255) / 256;
    constexpr int YROW = 272;                          // 32 px x 8 B + 16 B pad: conflict-free 16-B reads
    __shared__ uint4 lds_hi[NG], lds_lo[NG];
    __shared__ __align__(16) unsigned char y_lds[128 * YROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // 32-pixel chunks are dealt cyclically to the S blocks of a coefficient tile, and the split index is
    // the fastest grid dimension: blocks that run together read ADJACENT 256-B segments of the same
    // Ylm rows (contiguous split ranges stream 128 x S scattered segments: 2.2 instead of 3+ TB/s)
    const int split = blockIdx.x;
    const int r0 = blockIdx.z * ROWS;
    const int cblk = blockIdx.y * 128;
    const int c = cblk + wave * 32 + (lane & 31);
    const int h = lane >> 5;
    const int nsteps = (Npix + 15) / 16;
    const int send = nsteps;
    f32x16 accr[MT], acci[MT];
    zero(accr);
    zero(acci);

    float4 yq[8];                                      // this thread's 8 x 16 B of the next Ylm tile
    uint4 ahq[PT], alq[PT];
    const bool aligned = (Npix & 1) == 0;              // rows start 16-B aligned
    auto fetch_y = [&](int s0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = tid + u * 256;               // (row, 16-B segment): 2 pixels
            const int row = i >> 4, seg = i & 15;
            const int cc = cblk + row, j = 16 * s0 + 2 * seg;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (cc < Ncoeff && j < Npix) {
                const float* src = Ylm + ((size_t)cc * Npix + j) * 2;
                if (j + 1 < Npix) {
                    if (aligned) v = *reinterpret_cast<const float4*>(src);
                    else v = make_float4(src[0], src[1], src[2], src[3]);
                } else { v.x = src[0]; v.y = src[1]; }
            }
            yq[u] = v;
        }
    };
    auto fetch_a = [&](int s0) {
        fetch_granules<ROWS, 2>(g_hi, g_lo, Rpad, r0, s0, send, tid, ahq, alq);
    };
    if (2 * split < send) { fetch_y(2 * split); fetch_a(2 * split); }
    const unsigned char* ymine = y_lds + (wave * 32 + (lane & 31)) * YROW + 64 * h;
    for (int s0 = 2 * split; s0 < send; s0 += 2 * S) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PT; ++u)
            if (tid + u * 256 < NG) { lds_hi[tid + u * 256] = ahq[u]; lds_lo[tid + u * 256] = alq[u]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = tid + u * 256;
            *reinterpret_cast<float4*>(y_lds + (i >> 4) * YROW + (i & 15) * 16) = yq[u];
        }
        __syncthreads();
        if (s0 + 2 * S < send) { fetch_y(s0 + 2 * S); fetch_a(s0 + 2 * S); }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            float4 y[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) y[q] = *reinterpret_cast<const float4*>(ymine + 128 * ks + 16 * q);
            uint4 rh, rl, ih, il;
            split_y4(y, y_scale, rh, rl, ih, il);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int gi = (ks * 2 + h) * ROWS + m * 32 + (lane & 31);
                mfma6(lds_hi[gi], lds_lo[gi], rh, rl, ih, il, accr[m], acci[m]);
            }
        }
    }
    RIME_MFMA_SETTLE();
    store_bwd_tile(accr, acci, part + (size_t)split * R * Ncoeff * 2, r0, R, Ncoeff, c, lane, inv_scale, y_scale);
}

// backward, LDS-DMA form (even Npix): the kernel above is bound by the Ylm bytes it keeps in flight (one 32-KB tile
// per block in registers, two blocks per CU: 64 KB -> 2.8 TB/s).  Here the Ylm tile and the pre-split gout granules of a
// chunk (KS K steps of 16 pixels) go from global memory straight into LDS (global_load_lds_dwordx4: no registers hold
// bytes in flight) through a ring of NSLOT slots, ONE raw barrier per chunk and a counted s_waitcnt vmcnt that leaves
// the NSLOT - 2 younger chunks in flight across it (MI355X guide, "Pipelining across barriers"), one 4-wave block per CU.
// An LDS-DMA wave instruction deposits 64 x 16 B contiguously in lane order, so rows cannot be padded; the fragment
// reads stay conflict-free through an XOR swizzle applied to the SOURCE address: the chunk's tile is 128 rows of
// GR = 8 KS granules (two pixels each), granule s of row c lands at position s ^ (c & 15) (KS 2) or s ^ ((c >> 1) & 7)
// (KS 1: two rows per 256 B of banks).  Rows / pixels beyond the
// matrix read a 16-byte block of zeros.  Every wave issues the same number of DMA instructions per chunk (the counted
// wait depends on it): a remainder is padded with loads of the zero block into a scratch KB.
// The load is issued from inline asm: hipcc counts a builtin LDS-DMA as a pending LDS write and drains it (vmcnt(0))
// before the next ds_read, which would serialise the ring; the kernel counts its own DMA queue.
__device__ __forceinline__ void glds16(const void* src, unsigned lds_wave_base)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(lds_wave_base) : "memory");
}

template <int N> __device__ __forceinline__ void wait_vmcnt()
{
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// wait until all but the `younger` most recent chunks (NPW instructions each) of this wave have landed
template <int NPW, int MAXY> __device__ __forceinline__ void wait_chunks(int younger)
{
    if constexpr (MAXY == 0) wait_vmcnt<0>();
    else {
        if (younger >= MAXY) wait_vmcnt<NPW * MAXY>();
        else wait_chunks<NPW, MAXY - 1>(younger);
    }
}

template <int MT, int KS, int NSLOT> struct BwdDma {
    static constexpr int ROWS = MT * 32;
    static constexpr int GR = 8 * KS;                  // 16-byte granules (two pixels) per row of the chunk's Ylm tile
    static constexpr int RP = 64 / GR;                 // tile rows per wave instruction (1 KB)
    static constexpr int YB = 128 * GR * 16;           // the chunk's Ylm tile: 128 coefficients x KS x 16 px x (re, im) f32
    static constexpr int GB = 2 * ROWS * 16;           // one K step of one gout image (hi or lo)
    static constexpr int SLOT = YB + KS * 2 * GB;
    static constexpr int NGW = GB / 1024;              // wave instructions per gout image and K step
    static constexpr int TI = KS * (16 + 2 * NGW);     // wave instructions per chunk
    static constexpr int NPW = (TI + 3) / 4;           // per wave
    static constexpr int LDS = NSLOT * SLOT + 1024;    // + the scratch KB of the padding loads
    static constexpr int AHEAD = NSLOT - 1;            // chunks in flight ahead of the one being read
    static_assert(LDS <= 160 * 1024, "LDS ring too large");
    static_assert(NPW * (NSLOT - 2) < 64, "vmcnt range");
};

// Workgroups go to the 8 XCDs round-robin by linear id.  The blocks of one pixel split read the SAME gout chunks
// (and, over row tiles, the same Ylm tile): each XCD takes a contiguous range of the (split, coefficient tile,
// row tile) order, so the ~32 blocks an XCD holds at a time share a split and the gout stream is served by that
// XCD's L2 instead of crossing the fabric once per coefficient tile (it was half as many bytes as Ylm itself).
// The grid is ring_grid() blocks; `valid` is false for the whole of a surplus block, which returns before any barrier.
struct XcdBlock { bool valid; int split, row_tile, col_tile; };

__device__ __forceinline__ XcdBlock xcd_block(int S, int CT, int RT)
{
    const int NB = S * CT * RT, per_xcd = (NB + 7) / 8;
    const int q = (int)(blockIdx.x % 8) * per_xcd + (int)(blockIdx.x / 8);
    return {(int)(blockIdx.x / 8) < per_xcd && q < NB, q / (CT * RT), q % RT, (q / RT) % CT};
}

// ring kernels: wave instruction tg of the chunk's pre-split gout granules, (K step, hi | lo image, KB) = tg, into the
// slot's granule area at LDS address `gbase`; K steps from `send` on read the zero block.  C: the ring's constants
template <typename C, int KS>
__device__ __forceinline__ void issue_gout(int tg, int lane, int s0, int send, const uint4* __restrict__ g_hi,
                                           const uint4* __restrict__ g_lo, const float* __restrict__ zero16, int Rpad, int r0,
                                           unsigned gbase)
{
    const int ks = KS == 1 ? 0 : tg / (2 * C::NGW), r = KS == 1 ? tg : tg % (2 * C::NGW);    // (one K step: tg < 2 NGW)
    const int img = r / C::NGW, k = r % C::NGW;
    const int i = k * 64 + lane;
    const int row = i % C::ROWS, hh = i / C::ROWS;
    const int qq = (s0 + ks) * 2 + hh;
    const uint4* g = img ? g_lo : g_hi;
    const void* src = s0 + ks < send ? (const void*)&g[(size_t)qq * Rpad + r0 + row] : (const void*)zero16;
    glds16(src, gbase + (ks * 2 + img) * C::GB + k * 1024);
}

// A ring step.  C::AHEAD chunks (C::NPW wave instructions per wave each) are in flight; per chunk ONE raw barrier behind a
// counted wait that leaves the `younger` chunks in flight across it.  After ring_wait the oldest chunk of every wave has
// landed and everyone is done with the chunk before it, whose slot (`nslot`) the next issue fills; `slot` is the one to read.
template <typename C> __device__ __forceinline__ void ring_wait(int younger)
{
    wait_chunks<C::NPW, C::AHEAD - 1>(younger);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}

template <typename C> __device__ __forceinline__ void ring_advance(int& slot, int& nslot)
{
    slot = slot == C::AHEAD ? 0 : slot + 1;
    nslot = nslot == C::AHEAD ? 0 : nslot + 1;
}

template <int MT, int KS, int NSLOT>
__global__ void __launch_bounds__(256, 1)
alm2pix_bwd_f16_dma_kernel(const uint4* __restrict__ g_hi, const uint4* __restrict__ g_lo,
                           const float* __restrict__ inv_scale, const float* __restrict__ Ylm,
                           const float* __restrict__ zero16, float y_scale,
                           int R, int Rpad, int Ncoeff, int Npix, int S, int CT, int RT, float* __restrict__ part)
{
    using C = BwdDma<MT, KS, NSLOT>;
    constexpr int ROWS = C::ROWS;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned smem_addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const XcdBlock blk = xcd_block(S, CT, RT);
    if (!blk.valid) return;                            // whole block, before any barrier
    const int split = blk.split;
    const int r0 = blk.row_tile * ROWS;
    const int cblk = blk.col_tile * 128;
    const int cl = wave * 32 + (lane & 31);            // this lane's coefficient row of the tile
    const int c = cblk + cl;
    const int h = lane >> 5;
    const int send = (Npix + 15) / 16;                 // K steps of 16 pixels
    const int nchunk = (send + KS - 1) / KS;
    const int niter = split < nchunk ? (nchunk - split + S - 1) / S : 0;      // chunks split, split + S, ...
    f32x16 accr[MT], acci[MT];
    zero(accr);
    zero(acci);

    auto issue = [&](int it, int slot) {
        const int s0 = KS * (split + it * S);
        const unsigned base = smem_addr + (unsigned)(slot * C::SLOT);
#pragma unroll
        for (int u = 0; u < C::NPW; ++u) {
            const int t = wave + 4 * u;                // wave-uniform
            if (t < 16 * KS) {                         // RP whole rows of the chunk's tile
                const int cr = C::RP * t + lane / C::GR;
                const int sg = (lane % C::GR) ^ ((cr >> (KS == 1 ? 1 : 0)) & (C::GR - 1));
                const int cc = cblk + cr, j = 16 * s0 + 2 * sg;
                const float* src = (cc < Ncoeff && j < Npix) ? Ylm + ((size_t)cc * Npix + j) * 2 : zero16;
                glds16(src, base + t * 1024);
            } else if (t < C::TI) {
                issue_gout<C, KS>(t - 16 * KS, lane, s0, send, g_hi, g_lo, zero16, Rpad, r0, base + C::YB);
            } else {
                glds16(zero16, smem_addr + NSLOT * C::SLOT);
            }
        }
    };
#pragma unroll
    for (int a = 0; a < C::AHEAD; ++a)
        if (a < niter) issue(a, a);
    const uint32_t ybase = (uint32_t)cl * (C::GR * 16u);
    const uint32_t sw = (uint32_t)((cl >> (KS == 1 ? 1 : 0)) & (C::GR - 1));
    int slot = 0, nslot = C::AHEAD;
    for (int it = 0; it < niter; ++it) {
        ring_wait<C>(niter - 1 - it);
        if (it + C::AHEAD < niter) issue(it + C::AHEAD, nslot);
        const unsigned char* sl = smem + slot * C::SLOT;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const uint4* lds_hi = reinterpret_cast<const uint4*>(sl + C::YB + ks * 2 * C::GB);
            const uint4* lds_lo = reinterpret_cast<const uint4*>(sl + C::YB + (ks * 2 + 1) * C::GB);
            float4 y[4];
#pragma unroll
            for (int qd = 0; qd < 4; ++qd)
                y[qd] = *reinterpret_cast<const float4*>(sl + ybase + ((((uint32_t)(8 * ks + 4 * h + qd)) ^ sw) * 16u));
            uint4 rh, rl, ih, il;
            split_y4(y, y_scale, rh, rl, ih, il);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int gi = h * ROWS + m * 32 + (lane & 31);
                mfma6(lds_hi[gi], lds_lo[gi], rh, rl, ih, il, accr[m], acci[m]);
            }
        }
        ring_advance<C>(slot, nslot);
    }
    RIME_MFMA_SETTLE();
    store_bwd_tile(accr, acci, part + (size_t)split * R * Ncoeff * 2, r0, R, Ncoeff, c, lane, inv_scale, y_scale);
}

// ---------------------------------------------------------------------------------------
// PACKED Ylm (round 3): Ylm x y_scale split ONCE into f16 hi / lo halves and stored in MFMA fragment order -- the
// same 8 bytes per (coefficient, pixel) as the complex64 matrix, one copy per direction (the forward contracts over
// coefficients, the backward over pixels: the 16-byte granule a lane feeds to the matrix core holds 8 consecutive K
// values, so the two directions need transposed granules).  The GEMM kernels then do no arithmetic on the streamed
// operand at all: a wave's fragment is ONE fully coalesced 1-KB load (forward: into registers; backward: LDS-DMA into
// the wave's own ring region, read back with linear, conflict-free ds_read_b128).  Callers cache the packed copies per
// Ylm object (bayeslim_amd/ops.py); a new or modified Ylm is packed again.
//   forward  Yf: [pixel tile jt of 32][K step s of 8 coefficients][hi | lo][lane][8 x f16]
//                lane (n = lane & 31 -> pixel 32 jt + n, h = lane >> 5): k = (c, q) = (8 s + 4 h + i, re | im), i = 0..3
//   backward Yb: [coefficient tile ct of 128][K step s of 16 pixels][wave w][re_hi, re_lo, im_hi, im_lo][lane][8 x f16]
//                lane (c = 128 ct + 32 w + (lane & 31), h = lane >> 5): pixels 16 s + 8 h + 0..7
//   rows / pixels / K steps beyond the matrix hold zeros; the K-step count is padded to a whole number of chunks
// ---------------------------------------------------------------------------------------
constexpr int PK_FWD_CHUNK = 4;                        // forward: K steps per chunk (32 coefficients)
constexpr int PK_BWD_KS = 2;                           // backward: K steps per ring chunk (32 pixels)

__host__ __device__ inline int pk_fwd_steps(int Ncoeff) { const int n = (2 * Ncoeff + 15) / 16; return (n + PK_FWD_CHUNK - 1) / PK_FWD_CHUNK * PK_FWD_CHUNK; }
__host__ __device__ inline int pk_bwd_steps(int Npix) { const int n = (Npix + 15) / 16; return (n + PK_BWD_KS - 1) / PK_BWD_KS * PK_BWD_KS; }

__global__ void __launch_bounds__(256)
alm_pack_fwd_kernel(const float* __restrict__ Ylm, float y_scale, int Ncoeff, int Npix, int nsteps, size_t ntile,
                    uint4* __restrict__ Yf)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // (jt, s, lane)
    const int lane = (int)(i & 63);
    const size_t js = i >> 6;
    const int s = (int)(js % nsteps);
    const size_t jt = js / nsteps;
    if (jt >= ntile) return;                           // (tiles beyond the map are written too: zeros)
    const size_t j = jt * 32 + (lane & 31);
    const int h = lane >> 5;
    float v[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = 8 * s + 4 * h + q;
        float2 y = make_float2(0.f, 0.f);
        if (c < Ncoeff && j < (size_t)Npix) y = *reinterpret_cast<const float2*>(Ylm + ((size_t)c * Npix + j) * 2);
        v[2 * q] = y.x * y_scale; v[2 * q + 1] = y.y * y_scale;
    }
    uint4 hi, lo;
    split8(v, hi, lo);
    uint4* dst = Yf + ((jt * nsteps + s) * 2) * 64 + lane;
    dst[0] = hi;
    dst[64] = lo;
}

__global__ void __launch_bounds__(256)
alm_pack_bwd_kernel(const float* __restrict__ Ylm, float y_scale, int Ncoeff, int Npix, int nsteps, uint4* __restrict__ Yb)
{
    // block = (ct, s): thread = (wave w, lane); reads 8 pixels x (re, im) = 64 contiguous bytes of one coefficient row
    const int s = (int)(blockIdx.x % nsteps), ct = (int)(blockIdx.x / nsteps);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = ct * 128 + w * 32 + (lane & 31);
    const int j0 = 16 * s + 8 * (lane >> 5);
    float re[8], im[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        float2 y = make_float2(0.f, 0.f);
        if (c < Ncoeff && j0 + q < Npix) y = *reinterpret_cast<const float2*>(Ylm + ((size_t)c * Npix + j0 + q) * 2);
        re[q] = y.x * y_scale; im[q] = y.y * y_scale;
    }
    uint4 rh, rl, ih, il;
    split8(re, rh, rl);
    split8(im, ih, il);
    uint4* dst = Yb + ((((size_t)ct * nsteps + s) * 4 + w) * 4) * 64 + lane;
    dst[0] = rh; dst[64] = rl; dst[128] = ih; dst[192] = il;
}

// forward on the packed copy: block = 4 waves x 32 pixels, MT row tiles per wave.  A (the pre-split alm granules) goes
// through LDS, double buffered (one barrier per chunk of 4 K steps); the B fragments are coalesced 16-byte loads per
// lane from the wave's own contiguous stream: the two registers of a K step are reloaded, right after their MFMAs, with
// the same K step of the chunk TWO ahead, so a wave keeps 4 to 8 K steps (8 - 16 KB) of its stream in flight.
template <int MT>
__global__ void __launch_bounds__(256)
alm2pix_fwd_packed_kernel(const uint4* __restrict__ a_hi, const uint4* __restrict__ a_lo,
                          const float* __restrict__ inv_scale, const uint4* __restrict__ Yf, float y_scale,
                          int R, int Rpad, int Ncoeff, int Npix, int nsteps, int chunks_per_split, float* __restrict__ out)
{
    // blockIdx.z = K split: chunks [z * chunks_per_split, ...) of the coefficient axis; the split's partial result goes
    // to plane z of `out` (S > 1: a workspace, summed in a fixed order by alm_reduce_kernel).  A wave owns a pixel tile, so
    // a map of Npix pixels offers only Npix / 32 waves: small maps are split over K as well (49 152 px: 384 blocks for
    // 512 resident ones -> 2 splits, - 6 %)
    constexpr int ROWS = MT * 32;
    constexpr int NG = 8 * ROWS;                       // A granules per image and chunk: (ks, h, row)
    constexpr int PT = NG / 256;
    __shared__ uint4 lds_hi[2][NG], lds_lo[2][NG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.y * ROWS;
    const size_t jt = (size_t)blockIdx.x * 4 + wave;
    const int j0 = (int)(jt * 32);
    const int asteps = (2 * Ncoeff + 15) / 16;         // K steps the A images hold
    f32x16 acc[MT];
    zero(acc);
    const uint4* ysrc = Yf + (jt * nsteps * 2) * 64 + lane;            // this wave's stream: 2 KB per K step
    uint4 b0[8], b1[8];                                // even / odd chunk: [ks * 2 + (hi | lo)]
    uint4 ahq[PT], alq[PT];
    auto load_b = [&](int s0, uint4 (&b)[8]) {
#pragma unroll
        for (int u = 0; u < 8; ++u) b[u] = ysrc[(size_t)(s0 * 2 + u) * 64];
    };
    auto fetch_a = [&](int s0) {
        fetch_granules<ROWS, 4>(a_hi, a_lo, Rpad, r0, s0, asteps, tid, ahq, alq);
    };
    auto compute = [&](uint4 (&b)[8], int buf, int s_next) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int gi = (ks * 2 + (lane >> 5)) * ROWS + m * 32 + (lane & 31);
                mfma3(lds_hi[buf][gi], lds_lo[buf][gi], b[2 * ks], b[2 * ks + 1], acc[m]);
            }
            if (s_next >= 0) {                         // uniform
                b[2 * ks] = ysrc[(size_t)((s_next + ks) * 2) * 64];
                b[2 * ks + 1] = ysrc[(size_t)((s_next + ks) * 2 + 1) * 64];
            }
        }
    };
    const int ch0 = blockIdx.z * chunks_per_split;
    const int nchunk = min(nsteps / PK_FWD_CHUNK, ch0 + chunks_per_split);
    if (ch0 < nchunk) load_b(4 * ch0, b0);
    if (ch0 + 1 < nchunk) load_b(4 * (ch0 + 1), b1);
    fetch_a(4 * ch0);
    for (int ch = ch0; ch < nchunk; ch += 2) {
#pragma unroll
        for (int u = 0; u < PT; ++u) { lds_hi[0][tid + u * 256] = ahq[u]; lds_lo[0][tid + u * 256] = alq[u]; }
        __syncthreads();
        if (ch + 1 < nchunk) fetch_a(4 * (ch + 1));
        compute(b0, 0, ch + 2 < nchunk ? 4 * (ch + 2) : -1);
        if (ch + 1 < nchunk) {
#pragma unroll
            for (int u = 0; u < PT; ++u) { lds_hi[1][tid + u * 256] = ahq[u]; lds_lo[1][tid + u * 256] = alq[u]; }
            __syncthreads();
            if (ch + 2 < nchunk) fetch_a(4 * (ch + 2));
            compute(b1, 1, ch + 3 < nchunk ? 4 * (ch + 3) : -1);
        }
    }
    RIME_MFMA_SETTLE();
    store_fwd_tile(acc, out + (size_t)blockIdx.z * R * Npix, r0, R, Npix, j0 + (lane & 31), lane, inv_scale, y_scale);
}

// backward on the packed copy: the LDS-DMA ring of alm2pix_bwd_f16_dma_kernel with the chunk's Ylm tile replaced by
// the wave-private packed fragments (16 wave instructions of 1 KB per K step, contiguous in memory AND in the slot: the
// chunk is one 32-KB run) -- no swizzle, no split, no multiply; the gout granules are staged as before (shared by the
// four waves, hence the one barrier per chunk).
template <int MT, int NSLOT>
__global__ void __launch_bounds__(256, 1)
alm2pix_bwd_packed_kernel(const uint4* __restrict__ g_hi, const uint4* __restrict__ g_lo,
                          const float* __restrict__ inv_scale, const uint4* __restrict__ Yb,
                          const float* __restrict__ zero16, float y_scale,
                          int R, int Rpad, int Ncoeff, int Npix, int nsteps, int S, int CT, int RT, float* __restrict__ part)
{
    constexpr int KS = PK_BWD_KS;
    using C = BwdDma<MT, KS, NSLOT>;
    constexpr int ROWS = C::ROWS;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned smem_addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const XcdBlock blk = xcd_block(S, CT, RT);
    if (!blk.valid) return;                            // whole block, before any barrier
    const int split = blk.split;
    const int r0 = blk.row_tile * ROWS;
    const int ct = blk.col_tile;
    const int c = ct * 128 + wave * 32 + (lane & 31);
    const int h = lane >> 5;
    const int send = (Npix + 15) / 16;                 // K steps the gout images hold
    const int nchunk = nsteps / KS;
    const int niter = split < nchunk ? (nchunk - split + S - 1) / S : 0;
    f32x16 accr[MT], acci[MT];
    zero(accr);
    zero(acci);

    const uint4* ytile = Yb + (size_t)ct * nsteps * 16 * 64 + lane;
    auto issue = [&](int it, int slot) {
        const int s0 = KS * (split + it * S);
        const unsigned base = smem_addr + (unsigned)(slot * C::SLOT);
#pragma unroll
        for (int u = 0; u < C::NPW; ++u) {
            const int t = wave + 4 * u;                // wave-uniform
            if (t < 16 * KS) {                         // KB number t of the chunk's 32-KB run: (ks, w, plane) = t
                glds16(ytile + ((size_t)s0 * 16 + t) * 64, base + t * 1024);
            } else if (t < C::TI) {
                issue_gout<C, KS>(t - 16 * KS, lane, s0, send, g_hi, g_lo, zero16, Rpad, r0, base + C::YB);
            } else {
                glds16(zero16, smem_addr + NSLOT * C::SLOT);
            }
        }
    };
#pragma unroll
    for (int a = 0; a < C::AHEAD; ++a)
        if (a < niter) issue(a, a);
    int slot = 0, nslot = C::AHEAD;
    for (int it = 0; it < niter; ++it) {
        ring_wait<C>(niter - 1 - it);
        if (it + C::AHEAD < niter) issue(it + C::AHEAD, nslot);
        const unsigned char* sl = smem + slot * C::SLOT;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const uint4* lds_hi = reinterpret_cast<const uint4*>(sl + C::YB + ks * 2 * C::GB);
            const uint4* lds_lo = reinterpret_cast<const uint4*>(sl + C::YB + (ks * 2 + 1) * C::GB);
            const uint4* yf = reinterpret_cast<const uint4*>(sl + (ks * 16 + wave * 4) * 1024) + lane;
            const uint4 rh = yf[0], rl = yf[64], ih = yf[128], il = yf[192];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int gi = h * ROWS + m * 32 + (lane & 31);
                mfma6(lds_hi[gi], lds_lo[gi], rh, rl, ih, il, accr[m], acci[m]);
            }
        }
        ring_advance<C>(slot, nslot);
    }
    RIME_MFMA_SETTLE();
    store_bwd_tile(accr, acci, part + (size_t)split * R * Ncoeff * 2, r0, R, Ncoeff, c, lane, inv_scale, y_scale);
}

// Backward on the packed copy, 8-wave form (MT = 4): one block = 256 coefficients (two packed coefficient tiles) x 128 rows.
// The gout granules a chunk needs are the same for every coefficient tile, so doubling the coefficients per block halves
// their share of the LDS-DMA intake (16 px: Ylm 32 KB + gout 8 KB instead of 16 + 8) -- and that intake, ~21-23 GB/s per
// CU whatever it carries, is what bounds the ring kernels.  Chunks of ONE K step in a ring of four 40-KB
// slots (exactly the 160 KB of a CU: 40 wave instructions per chunk = 5 per wave, no padding loads, no scratch).
struct BwdDma8 {
    static constexpr int ROWS = 128, NW = 8, NSLOT = 4;
    static constexpr int YB = NW * 4 * 1024;           // 8 waves x (re_hi, re_lo, im_hi, im_lo) x 1 KB
    static constexpr int GB = 2 * ROWS * 16;           // one gout image (hi or lo) of the K step: 4 KB
    static constexpr int SLOT = YB + 2 * GB;           // 40 KB
    static constexpr int NGW = GB / 1024;              // 4
    static constexpr int TI = 4 * NW + 2 * NGW;        // 40
    static constexpr int NPW = TI / NW;                // 5
    static constexpr int LDS = NSLOT * SLOT;
    static constexpr int AHEAD = NSLOT - 1;
    static_assert(TI % NW == 0 && LDS <= 160 * 1024 && NPW * (NSLOT - 2) < 64, "ring shape");
};

__global__ void __launch_bounds__(512, 1)
alm2pix_bwd_packed8_kernel(const uint4* __restrict__ g_hi, const uint4* __restrict__ g_lo,
                           const float* __restrict__ inv_scale, const uint4* __restrict__ Yb,
                           const float* __restrict__ zero16, float y_scale,
                           int R, int Rpad, int Ncoeff, int Npix, int nsteps, int S, int CT2, int RT, float* __restrict__ part)
{
    using C = BwdDma8;
    constexpr int MT = 4, ROWS = C::ROWS;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned smem_addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const XcdBlock blk = xcd_block(S, CT2, RT);
    if (!blk.valid) return;                            // whole block, before any barrier
    const int split = blk.split;
    const int r0 = blk.row_tile * ROWS;
    const int ct0 = 2 * blk.col_tile;                  // first of this block's two packed coefficient tiles
    const int c = ct0 * 128 + wave * 32 + (lane & 31);
    const int h = lane >> 5;
    const int send = (Npix + 15) / 16;
    const int nchunk = nsteps;                         // one K step per chunk
    const int niter = split < nchunk ? (nchunk - split + S - 1) / S : 0;
    f32x16 accr[MT], acci[MT];
    zero(accr);
    zero(acci);

    const uint4* ytile = Yb + (size_t)ct0 * nsteps * 16 * 64 + lane;
    const size_t ct_stride = (size_t)nsteps * 16 * 64;                 // uint4 elements between packed coefficient tiles
    auto issue = [&](int it, int slot) {
        const int s0 = split + it * S;
        const unsigned base = smem_addr + (unsigned)(slot * C::SLOT);
#pragma unroll
        for (int u = 0; u < C::NPW; ++u) {
            const int t = wave + C::NW * u;            // wave-uniform, 0 .. 39
            if (t < 4 * C::NW) {                       // KB number t of the chunk's Ylm: (tile half, wave, plane)
                glds16(ytile + (size_t)(t >> 4) * ct_stride + ((size_t)s0 * 16 + (t & 15)) * 64, base + t * 1024);
            } else {
                issue_gout<C, 1>(t - 4 * C::NW, lane, s0, send, g_hi, g_lo, zero16, Rpad, r0, base + C::YB);
            }
        }
    };
#pragma unroll
    for (int a = 0; a < C::AHEAD; ++a)
        if (a < niter) issue(a, a);
    int slot = 0, nslot = C::AHEAD;
    for (int it = 0; it < niter; ++it) {
        ring_wait<C>(niter - 1 - it);
        if (it + C::AHEAD < niter) issue(it + C::AHEAD, nslot);
        const unsigned char* sl = smem + slot * C::SLOT;
        const uint4* lds_hi = reinterpret_cast<const uint4*>(sl + C::YB);
        const uint4* lds_lo = reinterpret_cast<const uint4*>(sl + C::YB + C::GB);
        const uint4* yf = reinterpret_cast<const uint4*>(sl + (wave * 4) * 1024) + lane;
        const uint4 rh = yf[0], rl = yf[64], ih = yf[128], il = yf[192];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int gi = h * ROWS + m * 32 + (lane & 31);
            mfma6(lds_hi[gi], lds_lo[gi], rh, rl, ih, il, accr[m], acci[m]);
        }
        ring_advance<C>(slot, nslot);
    }
    RIME_MFMA_SETTLE();
    store_bwd_tile(accr, acci, part + (size_t)split * R * Ncoeff * 2, r0, R, Ncoeff, c, lane, inv_scale, y_scale);
}

__global__ void alm_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, size_t len, int S)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int s = 0; s < S; ++s) v += part[(size_t)s * len + i];
        out[i] = v;
    }
}

// row tiles of 32 per block of every matrix-core kernel here
static int row_mt(int R) { return R > 64 ? 4 : (R > 32 ? 2 : 1); }

// f(std::integral_constant<int, MT>): the one place a run-time MT picks a kernel instantiation
template <typename F> static auto with_mt(int MT, F f)
{
    if (MT == 4) return f(std::integral_constant<int, 4>{});
    if (MT == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 1>{});
}

// compute units of the calling thread's device (read once); 0 without a device: every planner has its own fallback
static long cu_count()
{
    static long cache = -1;
    if (cache < 0) {
        int dev = 0; hipDeviceProp_t prop;
        cache = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 0;
        (void)hipGetLastError();
    }
    return cache;
}

// Launch of a kernel with more dynamic LDS than the default limit.  The attribute belongs to the (function, device)
// pair: remembered per kernel instantiation and device of the calling thread.
template <auto Kernel, typename... Args>
static hipError_t launch_dynamic_lds(dim3 grid, dim3 block, int lds, hipStream_t st, Args... args)
{
    static unsigned long long configured = 0ull;
    int devid = 0;
    if (hipGetDevice(&devid) != hipSuccess) devid = 0;
    const unsigned long long bit = 1ull << (devid & 63);
    if (!(configured & bit)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        configured |= bit;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
    return hipSuccess;
}

static void reduce_planes(const float* part, float* out, size_t len, int S, hipStream_t st)
{
    if (S <= 1) return;
    int nb = (int)std::min<size_t>((len + 255) / 256, 2048);
    hipLaunchKernelGGL(alm_reduce_kernel, dim3(nb), dim3(256), 0, st, part, out, len, S);
}

// K splits of the packed forward (two 4-wave blocks per CU are resident), each split >= 16 chunks
static int fwd_packed_splits(int R, int Ncoeff, int Npix, int MT)
{
    const long resident = cu_count() ? 2 * cu_count() : 512;
    const long blocks = (long)((Npix + 127) / 128) * ((R + MT * 32 - 1) / (MT * 32));
    const int nchunk = pk_fwd_steps(Ncoeff) / PK_FWD_CHUNK;
    // measured at the C3 shape (384 blocks of 263 chunks, 512 resident): S 1 / 2 / 3 / 4 / 6 -> 0.911 / 0.853 / 0.890 /
    // 0.871 / 0.898 ms including the reduction of the partial planes: enough blocks for 1.5 resident grids, no more
    int best = (int)std::min<long>(4, std::max<long>(1, (3 * resident / 2 + blocks - 1) / blocks));
    while (best > 1 && nchunk / best < 16) --best;
    if (const char* e = getenv("RIME_ALM_FWD_SPLITS")) { const int v = atoi(e); if (v >= 1 && v <= 8 && nchunk / v >= 1) best = v; }   // lab
    return best;
}

static int bwd_splits(int R, int Ncoeff, int Npix)
{
    // enough blocks to keep Ylm streaming: >= ~2048 waves; each split covers a multiple of 64 pixels
    const int MT = row_mt(R);
    const long blocks = (long)((Ncoeff + 15) / 16) * ((R + MT * 32 - 1) / (MT * 32));
    long S = (2048 + blocks * MT - 1) / (blocks * MT);
    const long maxS = std::max(1, Npix / 1024);
    if (S > maxS) S = maxS;
    return (int)std::max<long>(1, S);
}

// ---- f16-split fast path: shapes and workspace layout ---------------------------------------
struct SplitPlan {
    int MT, Rpad, nsteps;            // row tiles per block, padded rows, K steps of 16
    size_t img_bytes;                // one f16 image (hi or lo) of the row operand
    int S, steps_per_split;          // backward only: pixel splits
};

// blocks of the f16-split backward kernel the chip holds at once (occupancy query, cached per shape)
static long bwd_resident_blocks(int MT)
{
    static long cache[5] = {0, 0, 0, 0, 0};
    if (cache[MT] == 0) {
        int per_cu = 0;
        const bool ok = cu_count() && with_mt(MT, [&](auto mt) {
            return hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, alm2pix_bwd_f16_kernel<decltype(mt)::value>, 256, 0);
        }) == hipSuccess;
        cache[MT] = (ok && per_cu > 0) ? (long)per_cu * cu_count() : 512;
        (void)hipGetLastError();
    }
    return cache[MT];
}

// LDS-DMA backward kernel: even pixel counts (16-byte aligned Ylm granules); RIME_ALM_BWD_DMA=0 selects the
// register-staged kernel
static bool bwd_use_dma(int Npix)
{
    static int env = -1;
    if (env < 0) { const char* e = getenv("RIME_ALM_BWD_DMA"); env = (e && e[0] == '0') ? 0 : 1; }
    return env == 1 && Npix % 2 == 0;
}

// the LDS-DMA kernel's ring (3 slots of 32 KB Ylm + the gout granules) leaves room for one block per CU
static long bwd_dma_resident_blocks() { return cu_count() ? cu_count() : 256; }

static SplitPlan split_plan(int R, int K, int Ncoeff, bool backward, int dma = -1)      // dma: -1 auto, 1 the ring kernels
{
    const bool use_dma = dma < 0 ? bwd_use_dma(K) : dma != 0;
    const bool wide = dma == 2 && R > 64;                          // 8-wave blocks of 256 coefficients, one K step per chunk
    SplitPlan p{};
    p.MT = row_mt(R);
    p.Rpad = ((R + p.MT * 32 - 1) / (p.MT * 32)) * p.MT * 32;
    p.nsteps = (K + 15) / 16;
    p.img_bytes = (size_t)p.nsteps * 2 * p.Rpad * 16;
    p.S = 1; p.steps_per_split = p.nsteps;
    if (backward) {
        // ~2048 blocks of 128 coefficients x MT row tiles, as WHOLE rounds of the resident grid: every block
        // streams the same number of chunks, so 4.1 rounds cost 5 (C3: 66 tiles x 32 splits = 2112 blocks over
        // 512 resident ones; 31 splits = 2046 blocks = 4.0 rounds)
        const long blocks = (long)(wide ? (Ncoeff + 255) / 256 : (Ncoeff + 127) / 128) * (p.Rpad / (p.MT * 32));
        const long resident = use_dma ? bwd_dma_resident_blocks() : bwd_resident_blocks(p.MT);
        long S = (2048 + blocks - 1) / blocks;                   // measured flat between 1024 and 4096 blocks
        const long maxS = std::max(1, p.nsteps / 32);          // >= 16 chunks of 2 K steps per block
        S = std::max<long>(1, std::min(S, maxS));
        if (use_dma) {
            // LDS-DMA kernel, one block per CU.  Cost of S splits in units of one chunk (2 K steps) of one block:
            // rounds of the chip x (chunks per block + ~3 for the ring's ramp and the epilogue) + the partial plane
            // each split writes and the reduce kernel reads back (R Ncoeff 16 B at ~4 TB/s against ~2.2 us per
            // chunk).  Measured (C3 shape, 66 tiles): S 11 / 15 / 19 / 23 / 31 -> 1.09 / 1.08 / 1.10 / 1.17 / 1.21 ms,
            // S 8 (2.06 rounds) 1.31 ms; 17 tiles x 196608 px: S 15 / 30 / 45 / 60 -> 1.12 / 1.16 / 1.17 / 1.25 ms.
            const long nchunk = wide ? p.nsteps : (p.nsteps + 1) / 2;
            const double c1 = (double)R * Ncoeff * 1.8e-6;
            double best = 1e300;
            const long top = std::min<long>(maxS, 8 * resident / blocks + 1);
            for (long s = 1; s <= std::max<long>(1, top); ++s) {
                const long rounds = (blocks * s + resident - 1) / resident;
                const double cost = (double)rounds * ((nchunk + s - 1) / s + 3) + c1 * s;
                if (cost < best) { best = cost; S = s; }
            }
        } else if (blocks * S > resident) {
            const long rounds = std::max<long>(1, (blocks * S + resident / 2) / resident);    // nearest whole number of rounds
            const long S2 = (rounds * resident) / blocks;                                      // largest split count that fits them
            if (S2 >= 1 && S2 <= maxS) S = S2;
        }
        if (const char* e = getenv("RIME_ALM_BWD_SPLITS")) { const long v = atol(e); if (v >= 1 && v <= maxS) S = v; }   // lab
        p.S = (int)S;
        p.steps_per_split = 0;                                   // chunks are dealt cyclically
    }
    return p;
}

// long rows: scale per row (one block each), then the tiled transposing split (row_scale_alm_kernel, split_rows_tiled_kernel)
static bool split_long_rows(const SplitPlan& p, int R, int L)
{
    return p.Rpad % 64 == 0 && (long)R * L >= (1L << 20);
}

static size_t split_ws_bytes(const SplitPlan& p)
{
    return 2 * p.img_bytes + (size_t)p.Rpad * (sizeof(float) + sizeof(unsigned int)) + 64;    // 64: a zero granule
}

// RIME_ALM_BWD_WIDE=0 keeps the 4-wave ring kernel of the packed backward above 64 rows (read once)
static bool bwd_packed_wide()
{
    static int env = -1;
    if (env < 0) { const char* e = getenv("RIME_ALM_BWD_WIDE"); env = (e && e[0] == '0') ? 0 : 1; }
    return env == 1;
}

// The plan of one transform: what the four entry points below launch and check their workspace against, and what
// rime_alm2pix_plan and the two workspace queries report.
struct AlmPlan {
    int family, MT, row_tiles, col_tiles, S, long_rows;
    size_t ws_bytes;                 // workspace: the split images (f16-split families) + the partial planes
    SplitPlan p;                     // the f16-split families only
};

// the families without a row split: `rows` x `cols` of the output per block
static AlmPlan plan_plain(int family, int MT, int R, int rows, int N, int cols)
{
    AlmPlan a{};
    a.family = family; a.MT = MT; a.S = 1;
    a.row_tiles = (R + rows - 1) / rows; a.col_tiles = (N + cols - 1) / cols;
    return a;
}

// the f16-split families: K = 2 Ncoeff (forward) or Npix (backward), `cols` output columns per block; `dma` as in split_plan
static AlmPlan plan_f16(int family, int R, int Ncoeff, int Npix, bool backward, int dma, int cols)
{
    AlmPlan a{};
    const int K = backward ? Npix : 2 * Ncoeff;
    a.p = split_plan(R, K, Ncoeff, backward, dma);
    a.family = family; a.MT = a.p.MT; a.S = a.p.S;
    a.row_tiles = a.p.Rpad / (a.p.MT * 32); a.col_tiles = ((backward ? Ncoeff : Npix) + cols - 1) / cols;
    a.long_rows = split_long_rows(a.p, R, K);
    a.ws_bytes = split_ws_bytes(a.p) + (backward ? (size_t)a.S * R * Ncoeff * 2 * sizeof(float) : 0);
    return a;
}

// packed: 0 Ylm as it is, 1 the packed copy
static AlmPlan plan_fwd(int dtype, double y_scale, int packed, int R, int Ncoeff, int Npix)
{
    if (dtype != RIME_F32) return plan_plain(RIME_ALM_F64_VALU, 0, R, 16, Npix, 256);
    if (!(y_scale > 0)) return plan_plain(RIME_ALM_F32_MFMA, row_mt(R), R, row_mt(R) * 32, Npix, 128);
    AlmPlan a = plan_f16(packed ? RIME_ALM_PACKED4 : RIME_ALM_F16_REG, R, Ncoeff, Npix, false, -1, 128);
    if (packed) {
        a.S = fwd_packed_splits(R, Ncoeff, Npix, a.MT);
        if (a.S > 1) a.ws_bytes += (size_t)a.S * R * Npix * sizeof(float);
    }
    return a;
}

// wide8: the packed copy goes to the 8-wave ring where it applies (above 64 rows)
static AlmPlan plan_bwd(int dtype, double y_scale, int packed, int R, int Ncoeff, int Npix, bool wide8 = bwd_packed_wide())
{
    if (dtype != RIME_F32) return plan_plain(RIME_ALM_F64_VALU, 0, R, 8, Ncoeff, 4);
    if (!(y_scale > 0)) {
        AlmPlan a = plan_plain(RIME_ALM_F32_MFMA, row_mt(R), R, row_mt(R) * 32, Ncoeff, 16);
        a.S = bwd_splits(R, Ncoeff, Npix);
        if (a.S > 1) a.ws_bytes = (size_t)a.S * R * Ncoeff * 2 * sizeof(float);
        return a;
    }
    if (!packed) return plan_f16(bwd_use_dma(Npix) ? RIME_ALM_F16_DMA : RIME_ALM_F16_REG, R, Ncoeff, Npix, true, -1, 128);
    const bool wide = wide8 && R > 64;
    return plan_f16(wide ? RIME_ALM_PACKED8 : RIME_ALM_PACKED4, R, Ncoeff, Npix, true, wide ? 2 : 1, wide ? 256 : 128);
}

// the linear grid of the ring kernels (xcd_block): whole rounds of the 8 XCDs
static dim3 ring_grid(const AlmPlan& a) { return dim3(8 * ((a.S * a.col_tiles * a.row_tiles + 7) / 8)); }

// The row operand of an f16-split transform in the caller's workspace: the hi / lo images, the row scales, the zero granule
// the ring kernels read beyond the matrix, and where the kernel writes -- `out`, or S partial planes behind the images.
struct Staged { uint4 *hi, *lo; float* inv; const float* zero16; float* part; };

// part == nullptr: the workspace is smaller than the plan's figure (nothing launched)
static Staged stage_rows(const float* X, int R, int L, const AlmPlan& a, int neg_odd, void* workspace, size_t bytes, void* out,
                         hipStream_t st)
{
    const SplitPlan& p = a.p;
    if (!workspace || bytes < a.ws_bytes) return Staged{};
    Staged s;
    s.hi = (uint4*)workspace;
    s.lo = (uint4*)((char*)workspace + p.img_bytes);
    s.inv = (float*)((char*)workspace + 2 * p.img_bytes);
    s.zero16 = (const float*)((char*)workspace + split_ws_bytes(p) - 64);
    s.part = a.S > 1 ? (float*)((char*)workspace + split_ws_bytes(p)) : (float*)out;
    unsigned int* rowmax = (unsigned int*)(s.inv + p.Rpad);
    const int nseg = (2 * p.nsteps * 8 + SPLIT_SEG - 1) / SPLIT_SEG;
    if (a.long_rows) {
        // `rowmax` doubles as the scale array
        float* scale = reinterpret_cast<float*>(rowmax);
        (void)hipMemsetAsync((char*)rowmax + (size_t)p.Rpad * sizeof(unsigned int), 0, 64, st);     // the zero granule
        hipLaunchKernelGGL(row_scale_alm_kernel, dim3(p.Rpad), dim3(256), 0, st, X, R, L, scale, s.inv);
        hipLaunchKernelGGL(split_rows_tiled_kernel, dim3((2 * p.nsteps + 31) / 32, p.Rpad / 64), dim3(256), 0, st, X, R, L,
                           p.Rpad, neg_odd, scale, s.hi, s.lo);
        return s;
    }
    (void)hipMemsetAsync(rowmax, 0, (size_t)p.Rpad * sizeof(unsigned int) + 64, st);     // + the zero granule behind it
    hipLaunchKernelGGL(row_absmax_kernel, dim3(R, (L + SPLIT_SEG - 1) / SPLIT_SEG), dim3(256), 0, st, X, R, L, rowmax);
    hipLaunchKernelGGL(split_rows_kernel, dim3(p.Rpad, std::max(1, nseg)), dim3(256), 0, st, X, R, L, p.Rpad,
                       neg_odd, rowmax, s.hi, s.lo, s.inv);
    return s;
}

} // namespace rime

using namespace rime;

extern "C" int rime_alm2pix_plan(int dtype, double y_scale, int R, int Ncoeff, int Npix, int direction, int packed, int* plan)
{
    if (!plan || (dtype != RIME_F32 && dtype != RIME_F64) || !(y_scale >= 0) || R <= 0 || Ncoeff <= 0 || Npix <= 0 ||
        (direction != 0 && direction != 1) || (packed != 0 && packed != 1)) return RIME_EINVAL;
    if (packed && (dtype != RIME_F32 || !(y_scale > 0))) return RIME_EINVAL;
    const AlmPlan a = direction ? plan_bwd(dtype, y_scale, packed, R, Ncoeff, Npix) : plan_fwd(dtype, y_scale, packed, R, Ncoeff, Npix);
    plan[0] = a.family; plan[1] = a.MT; plan[2] = a.row_tiles; plan[3] = a.col_tiles; plan[4] = a.S; plan[5] = a.long_rows;
    return RIME_OK;
}

extern "C" size_t rime_alm2pix_fwd_workspace(int dtype, int R, int Ncoeff, int Npix)
{
    if (dtype != RIME_F32 || R <= 0 || Ncoeff <= 0) return 0;
    // one buffer for rime_alm2pix_fwd and rime_alm2pix_fwd_packed (the K-split partial planes; none without a pixel count)
    return std::max(plan_fwd(RIME_F32, 1.0, 0, R, Ncoeff, Npix).ws_bytes,
                    Npix > 0 ? plan_fwd(RIME_F32, 1.0, 1, R, Ncoeff, Npix).ws_bytes : 0);
}

extern "C" int rime_alm2pix_fwd(int dtype, const void* alm, const void* Ylm, double y_scale, int R, int Ncoeff,
                                int Npix, void* out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!alm || !Ylm || !out || R <= 0 || Ncoeff <= 0 || Npix <= 0 || y_scale < 0) return RIME_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype != RIME_F32 && dtype != RIME_F64) return RIME_EINVAL;
    const AlmPlan pl = plan_fwd(dtype, y_scale, 0, R, Ncoeff, Npix);
    const dim3 grid(pl.col_tiles, pl.row_tiles);
    if (pl.family == RIME_ALM_F16_REG) {
        const Staged s = stage_rows((const float*)alm, R, 2 * Ncoeff, pl, 1, workspace, workspace_bytes, out, st);
        if (!s.part) return RIME_EWORKSPACE;
        with_mt(pl.MT, [&](auto mt) {
            hipLaunchKernelGGL((alm2pix_fwd_f16_kernel<decltype(mt)::value>), grid, dim3(256), 0, st, s.hi, s.lo, s.inv,
                               (const float*)Ylm, (float)y_scale, R, pl.p.Rpad, Ncoeff, Npix, s.part);
        });
    } else if (pl.family == RIME_ALM_F32_MFMA) {
        with_mt(pl.MT, [&](auto mt) {
            hipLaunchKernelGGL((alm2pix_fwd_mfma_kernel<decltype(mt)::value>), grid, dim3(256), 0, st, (const float*)alm,
                               (const float*)Ylm, R, Ncoeff, Npix, (float*)out);
        });
    } else {
        constexpr int RTA = 16;                        // plan_fwd: row_tiles
        hipLaunchKernelGGL((alm2pix_fwd_kernel<double, RTA>), grid, dim3(256), 0, st,
                           (const double*)alm, (const double*)Ylm, R, Ncoeff, Npix, (double*)out);
    }
    return check_launch();
}

extern "C" size_t rime_alm2pix_bwd_workspace(int dtype, int R, int Ncoeff, int Npix)
{
    if (dtype != RIME_F32 || R <= 0 || Ncoeff <= 0 || Npix <= 0) return 0;
    // one buffer for the exact-f32 path (split partials), the f16-split path (images + row scales + split partials) and
    // rime_alm2pix_bwd_packed on either ring
    size_t need = 0;
    for (const double ys : {0.0, 1.0}) need = std::max(need, plan_bwd(RIME_F32, ys, 0, R, Ncoeff, Npix).ws_bytes);
    for (const bool wide8 : {false, true}) need = std::max(need, plan_bwd(RIME_F32, 1.0, 1, R, Ncoeff, Npix, wide8).ws_bytes);
    return need;
}

extern "C" int rime_alm2pix_bwd(int dtype, const void* gout, const void* Ylm, double y_scale, int R, int Ncoeff,
                                int Npix, void* galm, void* workspace, size_t workspace_bytes,
                                void* stream)
{
    if (!gout || !Ylm || !galm || R <= 0 || Ncoeff <= 0 || Npix <= 0 || y_scale < 0) return RIME_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype != RIME_F32 && dtype != RIME_F64) return RIME_EINVAL;
    const AlmPlan pl = plan_bwd(dtype, y_scale, 0, R, Ncoeff, Npix);
    const size_t len = (size_t)R * Ncoeff * 2;
    if (pl.family == RIME_ALM_F16_DMA || pl.family == RIME_ALM_F16_REG) {
        const Staged s = stage_rows((const float*)gout, R, Npix, pl, 0, workspace, workspace_bytes, galm, st);
        if (!s.part) return RIME_EWORKSPACE;
        const float ys = (float)y_scale;
        const float* Y = (const float*)Ylm;
        const hipError_t e = with_mt(pl.MT, [&](auto mt) {
            constexpr int MT = decltype(mt)::value;
            if (pl.family == RIME_ALM_F16_DMA)
                // chunks of 2 K steps in a ring of 3 slots; 1 K step in 6 slots (more, smaller loads in flight) measured the same
                return launch_dynamic_lds<alm2pix_bwd_f16_dma_kernel<MT, 2, 3>>(
                    ring_grid(pl), dim3(256), BwdDma<MT, 2, 3>::LDS, st, s.hi, s.lo, s.inv, Y, s.zero16, ys, R, pl.p.Rpad, Ncoeff,
                    Npix, pl.S, pl.col_tiles, pl.row_tiles, s.part);
            hipLaunchKernelGGL((alm2pix_bwd_f16_kernel<MT>), dim3(pl.S, pl.col_tiles, pl.row_tiles), dim3(256), 0, st, s.hi, s.lo,
                               s.inv, Y, ys, R, pl.p.Rpad, Ncoeff, Npix, pl.S, s.part);
            return hipSuccess;
        });
        if (e != hipSuccess) return RIME_ELAUNCH;
        reduce_planes(s.part, (float*)galm, len, pl.S, st);
        return check_launch();
    }
    if (pl.family == RIME_ALM_F32_MFMA) {
        const int S = pl.S;
        if (pl.ws_bytes && (!workspace || workspace_bytes < pl.ws_bytes)) return RIME_EWORKSPACE;
        float* part = S > 1 ? (float*)workspace : (float*)galm;
        int pps = (Npix + S - 1) / S;
        pps = ((pps + 63) / 64) * 64;
        with_mt(pl.MT, [&](auto mt) {
            constexpr int MT = decltype(mt)::value;
            hipLaunchKernelGGL((alm2pix_bwd_mfma_kernel<MT>), dim3(pl.col_tiles, S, pl.row_tiles), dim3(64 * MT), 0, st,
                               (const float*)gout, (const float*)Ylm, R, Ncoeff, Npix, pps, part);
        });
        reduce_planes(part, (float*)galm, len, S, st);
        return check_launch();
    }
    constexpr int CT = 4, RTB = 8;                     // plan_bwd: col_tiles, row_tiles
    dim3 grid(pl.col_tiles, pl.row_tiles);
    hipLaunchKernelGGL((alm2pix_bwd_kernel<double, CT, RTB>), grid, dim3(256), 0, st,
                       (const double*)gout, (const double*)Ylm, R, Ncoeff, Npix, (double*)galm);
    return check_launch();
}


// ---- packed Ylm (see the kernels): size, packing, and the two transforms on a packed copy ------------------------
extern "C" size_t rime_alm2pix_packed_bytes(int Ncoeff, int Npix, int direction)
{
    if (Ncoeff <= 0 || Npix <= 0 || (direction != 0 && direction != 1)) return 0;
    if (direction == 0) return (size_t)((Npix + 127) / 128 * 4) * pk_fwd_steps(Ncoeff) * 2048;     // whole 4-wave blocks of pixel tiles
    return (size_t)((Ncoeff + 255) / 256 * 2) * pk_bwd_steps(Npix) * 16384;      // whole 256-coefficient (8-wave) blocks
}

extern "C" int rime_alm2pix_pack(const void* Ylm, double y_scale, int Ncoeff, int Npix, int direction, void* packed,
                                 void* stream)
{
    if (!Ylm || !packed || Ncoeff <= 0 || Npix <= 0 || !(y_scale > 0) || (direction != 0 && direction != 1)) return RIME_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (direction == 0) {
        const int nsteps = pk_fwd_steps(Ncoeff);
        const size_t ntile = (size_t)(Npix + 127) / 128 * 4;
        const size_t nthr = ntile * nsteps * 64;
        if ((nthr + 255) / 256 > 0x7fffffffull) return RIME_EUNSUPPORTED;
        hipLaunchKernelGGL(alm_pack_fwd_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, (const float*)Ylm, (float)y_scale,
                           Ncoeff, Npix, nsteps, ntile, (uint4*)packed);
    } else {
        const int nsteps = pk_bwd_steps(Npix);
        const size_t nblk = (size_t)((Ncoeff + 255) / 256 * 2) * nsteps;
        if (nblk > 0x7fffffffull) return RIME_EUNSUPPORTED;
        hipLaunchKernelGGL(alm_pack_bwd_kernel, dim3((unsigned)nblk), dim3(256), 0, st, (const float*)Ylm, (float)y_scale,
                           Ncoeff, Npix, nsteps, (uint4*)packed);
    }
    return check_launch();
}

extern "C" int rime_alm2pix_fwd_packed(const void* alm, const void* packed, double y_scale, int R, int Ncoeff, int Npix,
                                       void* out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!alm || !packed || !out || R <= 0 || Ncoeff <= 0 || Npix <= 0 || !(y_scale > 0)) return RIME_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const AlmPlan pl = plan_fwd(RIME_F32, y_scale, 1, R, Ncoeff, Npix);
    const int S = pl.S;
    const Staged s = stage_rows((const float*)alm, R, 2 * Ncoeff, pl, 1, workspace, workspace_bytes, out, st);
    if (!s.part) return RIME_EWORKSPACE;
    const int nsteps = pk_fwd_steps(Ncoeff);
    const int cps = (nsteps / PK_FWD_CHUNK + S - 1) / S;
    with_mt(pl.MT, [&](auto mt) {
        hipLaunchKernelGGL((alm2pix_fwd_packed_kernel<decltype(mt)::value>), dim3(pl.col_tiles, pl.row_tiles, S), dim3(256), 0, st,
                           s.hi, s.lo, s.inv, (const uint4*)packed, (float)y_scale, R, pl.p.Rpad, Ncoeff, Npix, nsteps, cps, s.part);
    });
    reduce_planes(s.part, (float*)out, (size_t)R * Npix, S, st);
    return check_launch();
}

extern "C" int rime_alm2pix_bwd_packed(const void* gout, const void* packed, double y_scale, int R, int Ncoeff, int Npix,
                                       void* galm, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!gout || !packed || !galm || R <= 0 || Ncoeff <= 0 || Npix <= 0 || !(y_scale > 0)) return RIME_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const AlmPlan pl = plan_bwd(RIME_F32, y_scale, 1, R, Ncoeff, Npix);
    const Staged s = stage_rows((const float*)gout, R, Npix, pl, 0, workspace, workspace_bytes, galm, st);
    if (!s.part) return RIME_EWORKSPACE;
    const uint4* Y = (const uint4*)packed;
    const float ys = (float)y_scale;
    const int nsteps = pk_bwd_steps(Npix);
    const hipError_t e = pl.family == RIME_ALM_PACKED8
        ? launch_dynamic_lds<alm2pix_bwd_packed8_kernel>(ring_grid(pl), dim3(512), BwdDma8::LDS, st, s.hi, s.lo, s.inv, Y, s.zero16,
                                                         ys, R, pl.p.Rpad, Ncoeff, Npix, nsteps, pl.S, pl.col_tiles, pl.row_tiles, s.part)
        : with_mt(pl.MT, [&](auto mt) {
              constexpr int MT = decltype(mt)::value;
              return launch_dynamic_lds<alm2pix_bwd_packed_kernel<MT, 3>>(
                  ring_grid(pl), dim3(256), BwdDma<MT, PK_BWD_KS, 3>::LDS, st, s.hi, s.lo, s.inv, Y, s.zero16, ys, R, pl.p.Rpad,
                  Ncoeff, Npix, nsteps, pl.S, pl.col_tiles, pl.row_tiles, s.part);
          });
    if (e != hipSuccess) return RIME_ELAUNCH;
    reduce_planes(s.part, (float*)galm, (size_t)R * Ncoeff * 2, pl.S, st);
    return check_launch();
}
