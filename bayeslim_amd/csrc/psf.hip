// psf.hip -- full PSF matrix of the imaging path (gfx950): a fused phasor-Gram kernel ("Full PSF matrix").
//
//   S[f,i,j]                 = sum_b w[b,f] cos(2 pi nu_f/c (b_b.s_i - b_b.t_j))  =  sum_b (w c_bi) c_bj + (w s_bi) s_bj
//   out[f, rows[i], cols[j]]  (= or +=)  rs[f,i] cs[f,j] S[f,i,j]
//
// The real part of D A^T w conj(A) with A = conj(fringe) beam (imaging.py:818-861): a real Gram product of rank 2 Nbl
// per channel over phasors that are generated here, so A never exists.  Vector ALU only:
//   * one work-group = one PSF_TILE x PSF_TILE tile of one channel; 16 x 16 lanes, each a PSF_TILE/16 square of
//     accumulators laid out as 4 x 4 sub-squares 64 apart, so that every LDS read is a conflict-free 16-byte read;
//   * per chunk of PSF_BCHUNK baselines every lane generates the phasors of ONE pixel (a row or a column of the tile, its
//     direction kept in registers): b.s and the product with nu/c in f64, reduced to [-1/2, 1/2] turns, one sincos of the
//     working precision per channel (turns.h; MODE_DIRECT of fringe.hip, any channel grid); rows are weighted by w.
//     The chunk is written to LDS once and read back by the register-tiled product;
//   * symmetric form (no column directions): only tile pairs ti <= tj run; a block stores its tile and the mirrored one
//     (scales rs[f,j] cs[f,i]); on a diagonal tile the elements i <= j own both stores.  Every output element has one
//     owner: += is load, add, store, no atomics, the same bits on every run;
//   * sums are flushed to the output every PSF_FLUSH baselines (2048 terms), the rule of fringe.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rime_common.h"
#include "turns.h"

namespace rime {

#ifndef RIME_PSF_TILE
#define RIME_PSF_TILE 64                      /* lab: 128 = an 8 x 8 square per lane (DESIGN.md has the measurement) */
#endif
constexpr int PSF_TILE = RIME_PSF_TILE;       // ops.PSF_TILE
constexpr int PSF_BCHUNK = 16;                // ops.PSF_BCHUNK: baselines per LDS chunk
constexpr int PSF_THREADS = 256;
constexpr int PSF_MT = PSF_TILE / 16;         // side of a lane's square
constexpr int PSF_FLUSH = 1024;               // baselines between two flushes: 2048 terms
static_assert(PSF_TILE == 64 || PSF_TILE == 128, "16 x 16 lanes of 4 x 4 sub-squares");
static_assert(PSF_FLUSH % PSF_BCHUNK == 0, "a flush falls between two chunks");

struct PsfArgs {
    const double* blvecs;
    const double* freqs;
    const void* w;
    long long w_sb, w_sf;
    const double* sr;          // row directions [3][ld_sr]
    const double* sq;          // column directions [3][ld_sq]; null: the rows (symmetric form)
    long long ld_sr, ld_sq;
    const void* rs;            // [Nf][Pr] or null
    const void* cs;            // [Nf][Pq] or null
    const int* rows;
    const int* cols;
    void* out;                 // [Nf][ldr][ldc]
    long long ldr, ldc;
    int Nbl, Pr, Pq, ntr, ntc, accumulate;
};

template <typename T> __device__ __forceinline__ void psf_read4(const T* p, T* dst);
template <> __device__ __forceinline__ void psf_read4<float>(const float* p, float* dst)
{
    const float4 v = *reinterpret_cast<const float4*>(p);
    dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
}
template <> __device__ __forceinline__ void psf_read4<double>(const double* p, double* dst)
{
    const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
    dst[0] = a.x; dst[1] = a.y; dst[2] = b.x; dst[3] = b.y;
}

template <typename T>
__global__ void __launch_bounds__(PSF_THREADS)
psf_gram_kernel(PsfArgs A)
{
    constexpr int TL = PSF_TILE, C = PSF_BCHUNK, MT = PSF_MT;
    constexpr int NG = PSF_THREADS / (2 * TL);                 // lane groups that share a chunk's baselines (1 or 2)
    __shared__ __align__(16) T lds[C][4][TL];                  // per baseline: w cos, w sin of the rows; cos, sin of the columns

    const int tid = threadIdx.x, f = blockIdx.y;
    const bool sym = A.sq == nullptr;
    int ti, tj;
    if (sym) {                                                 // pair index -> (ti <= tj), row by row of the upper triangle
        int p = blockIdx.x;
        ti = 0;
        while (p >= A.ntr - ti) { p -= A.ntr - ti; ++ti; }
        tj = ti + p;
    } else {
        ti = blockIdx.x / A.ntc;
        tj = blockIdx.x % A.ntc;
    }
    const int i0 = ti * TL, j0 = tj * TL;

    // this lane as a generator: one pixel of the tile's rows (gp < TL) or columns
    const int gp = tid % (2 * TL), kg = tid / (2 * TL);
    const bool is_col = gp >= TL;
    const int pl = is_col ? gp - TL : gp;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    {
        const double* sd = (is_col && !sym) ? A.sq : A.sr;
        const long long ld = (is_col && !sym) ? A.ld_sq : A.ld_sr;
        const int pg = (is_col ? j0 : i0) + pl;
        if (pg < (is_col ? A.Pq : A.Pr)) { sx = sd[pg]; sy = sd[ld + pg]; sz = sd[2 * ld + pg]; }
    }
    const double nu_c = A.freqs[f] * (1.0 / 2.99792458e8);
    const T* w = reinterpret_cast<const T*>(A.w) + (long long)f * A.w_sf;

    // ... and as an owner of MT x MT outputs: local row (ii / 4) 64 + ty 4 + ii % 4, column likewise with tx
    const int ty = tid / 16, tx = tid % 16;
    T acc[MT][MT];
#pragma unroll
    for (int ii = 0; ii < MT; ++ii)
#pragma unroll
        for (int jj = 0; jj < MT; ++jj) acc[ii][jj] = T(0);

    const T* rs = reinterpret_cast<const T*>(A.rs);
    const T* cs = reinterpret_cast<const T*>(A.cs);
    T* out = reinterpret_cast<T*>(A.out) + (size_t)f * (size_t)A.ldr * (size_t)A.ldc;
    bool first = true;

    for (int seg = 0; seg < A.Nbl; seg += PSF_FLUSH) {
        const int seg_end = min(A.Nbl, seg + PSF_FLUSH);
        for (int b0 = seg; b0 < seg_end; b0 += C) {
            __syncthreads();
            for (int k = kg; k < C; k += NG) {
                const int b = b0 + k;
                const bool live = b < seg_end;
                const int bc = live ? b : seg_end - 1;
                const double tau = A.blvecs[3 * bc] * sx + A.blvecs[3 * bc + 1] * sy + A.blvecs[3 * bc + 2] * sz;
                T s, c;
                sincos_turns(reduce_turns<T>(tau * nu_c), s, c);
                if (!is_col) {
                    const T wk = live ? w[(long long)bc * A.w_sb] : T(0);      // past the end: a zero row term
                    c *= wk;
                    s *= wk;
                }
                lds[k][is_col ? 2 : 0][pl] = c;
                lds[k][is_col ? 3 : 1][pl] = s;
            }
            __syncthreads();
#pragma unroll 2
            for (int k = 0; k < C; ++k) {
                T ac[MT], as[MT], bc[MT], bs[MT];
#pragma unroll
                for (int q = 0; q < MT / 4; ++q) {
                    psf_read4<T>(&lds[k][0][q * 64 + ty * 4], ac + 4 * q);
                    psf_read4<T>(&lds[k][1][q * 64 + ty * 4], as + 4 * q);
                    psf_read4<T>(&lds[k][2][q * 64 + tx * 4], bc + 4 * q);
                    psf_read4<T>(&lds[k][3][q * 64 + tx * 4], bs + 4 * q);
                }
#pragma unroll
                for (int ii = 0; ii < MT; ++ii)
#pragma unroll
                    for (int jj = 0; jj < MT; ++jj) {
                        acc[ii][jj] = tfma<T>(ac[ii], bc[jj], acc[ii][jj]);
                        acc[ii][jj] = tfma<T>(as[ii], bs[jj], acc[ii][jj]);
                    }
            }
        }

        // flush: this segment's sums to the owned elements (and their mirror images)
        const bool add = A.accumulate || !first;
#pragma unroll
        for (int ii = 0; ii < MT; ++ii) {
            const int gi = i0 + (ii / 4) * 64 + ty * 4 + ii % 4;
#pragma unroll
            for (int jj = 0; jj < MT; ++jj) {
                const int gj = j0 + (jj / 4) * 64 + tx * 4 + jj % 4;
                const T v = acc[ii][jj];
                acc[ii][jj] = T(0);
                if (gi >= A.Pr || gj >= A.Pq) continue;
                if (sym && ti == tj && gj < gi) continue;              // diagonal tile: (i <= j) owns (i, j) and (j, i)
                {
                    const T scale = (rs ? rs[(size_t)f * A.Pr + gi] : T(1)) * (cs ? cs[(size_t)f * A.Pq + gj] : T(1));
                    T* o = out + (size_t)(A.rows ? A.rows[gi] : gi) * (size_t)A.ldc + (size_t)(A.cols ? A.cols[gj] : gj);
                    T x = scale * v;
                    if (add) x += *o;
                    *o = x;
                }
                if (sym && gi != gj) {
                    const T scale = (rs ? rs[(size_t)f * A.Pr + gj] : T(1)) * (cs ? cs[(size_t)f * A.Pq + gi] : T(1));
                    T* o = out + (size_t)(A.rows ? A.rows[gj] : gj) * (size_t)A.ldc + (size_t)(A.cols ? A.cols[gi] : gi);
                    T x = scale * v;
                    if (add) x += *o;
                    *o = x;
                }
            }
        }
        first = false;
    }
}

} // namespace rime

using namespace rime;

extern "C" int rime_psf_gram(int dtype, const double* blvecs, const double* freqs, const void* w, long long w_sb,
                             long long w_sf, int Nbl, int Nf, const double* sr, long long ld_sr, int Pr, const double* sq,
                             long long ld_sq, int Pq, const void* rs, const void* cs, const int* rows, const int* cols,
                             void* out, long long ldr, long long ldc, int accumulate, void* stream)
{
    if (!real_dtype_ok(dtype) || !blvecs || !freqs || !w || !sr || !out) return RIME_EINVAL;
    if (Nbl <= 0 || Nf <= 0 || Nf > 65535 || Pr <= 0 || (sq && Pq <= 0)) return RIME_EINVAL;
    if (w_sb < 0 || w_sf < 0 || ld_sr < Pr || (sq && ld_sq < Pq)) return RIME_EINVAL;
    if (accumulate != 0 && accumulate != 1) return RIME_EINVAL;
    if (!sq) Pq = Pr;
    if (ldr <= 0 || ldc <= 0 || (!rows && ldr < Pr) || (!cols && ldc < Pq)) return RIME_EINVAL;
    const long long ntr = (Pr + PSF_TILE - 1) / PSF_TILE, ntc = (Pq + PSF_TILE - 1) / PSF_TILE;
    const long long nblocks = sq ? ntr * ntc : ntr * (ntr + 1) / 2;
    if (nblocks > 0x7fffffffLL) return RIME_EINVAL;
    const PsfArgs A = {blvecs, freqs, w, w_sb, w_sf, sr, sq, ld_sr, ld_sq, rs, cs, rows, cols, out, ldr, ldc,
                       Nbl, Pr, Pq, (int)ntr, (int)ntc, accumulate};
    return with_real(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((psf_gram_kernel<T>), dim3((unsigned)nblocks, (unsigned)Nf), dim3(PSF_THREADS), 0, as_stream(stream), A);
        return check_launch();
    });
}
