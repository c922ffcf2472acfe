// hmat.hip -- grouped block mat-vec y (+)= scalar * A x for an operator tree flattened into a table of tiles (hmat.py):
// dense and diagonal blocks at offsets of an extended vector (x, y and a scratch vector).  A low-rank leaf U V is two dense
// tiles: V from x into the scratch vector in stage 0, U from the scratch vector into y in stage 1.  One launch per stage and
// group of at most HM_NR right-hand sides; the stages are separate launches on the caller's stream.
//
// Work is dealt by destination rows: a work-group owns one row range of the per-stage index, keeps one accumulator per (row,
// right-hand side) in LDS (zero at the start), visits the tiles listed for the range in that order and writes every row of the
// range once at the end.  No atomics, no flags, no work-group waits for another.  What a row receives is a function of its own
// tiles and their order alone; it does not depend on the row ranges, on the other tiles of the table or on alignment.
//
// N form (y_i = sum_j A[i, j] x_j, the row of A contiguous): a wave takes a row; the columns go in chunks of CK = 128 W
// (W = 16 / sizeof(T)), the x segment of a chunk staged in LDS once for 32 rows; lane l holds columns (g * 64 + l) W ... + W - 1
// of the chunk (g = 0, 1) and runs ONE chain of fused multiply-adds per right-hand side in ascending column order over all
// chunks; the 64 chains are added by a butterfly (xor 32, 16, ..., 1).
// T form (y_i = sum_j A[j, i] x_j, the outputs contiguous): a lane takes W adjacent outputs, wave w the rows j = w, w + 4, ...
// in ascending order as one chain each; the four waves are added through LDS as ((w0 + w1) + w2) + w3.
// A narrow matrix (at most 32 W columns) is dealt differently in both forms: G = 2^k >= cols / W lanes cover a stored row, so
// that one wave load covers 64 / G adjacent rows.  Plain: the lane's chain over its W columns, then a butterfly over the G
// lanes of the row (xor G / 2, ..., 1).  Transposed: wave w and row slot u run the chain over the stored rows
// j = (64 / G) w + u, + 256 / G, ...; the 256 / G chains of an output are added in the order (w, u) ascending, w major.
// Diagonal: d_i * x_i.  Every tile's sum s enters the accumulator as acc = fma(T(scale), s, acc).
// A matrix whose base and leading dimension are multiples of 16 bytes is read with 16-byte loads, any other with element
// loads (the rule of lane_vec.h; the branch is uniform across the tile), so the bits do not change.
// Vector ALU only; the register arrays are indexed by unrolled loops only (no scratch memory).
#include "lane_vec.h"

namespace rime {

constexpr int HM_THREADS = 256, HM_WAVES = 4, HM_ROWS = 256, HM_RW = 8, HM_G = 2, HM_NR = 4, HM_MAXSTAGES = 8;
constexpr int HM_TRANS = 1, HM_DIAG = 2, HM_SRC_SCRATCH = 4;       // tile flags
constexpr int HM_DST_SCRATCH = 1, HM_ACCUMULATE = 2;              // range flags

struct HmTile {                      // rime_hmat_tile of the header, 64 bytes
    const void* a;
    long long ld, src_off, dst_off;
    double scale;
    int rows, cols, flags, stage;
    long long reserved;
};
static_assert(sizeof(HmTile) == 64, "tile layout");

// W elements of a matrix row from column c on; columns at or beyond `end` read as 0
template <typename T>
__device__ __forceinline__ void hm_load(const T* __restrict__ row, long long c, long long end, bool vec, T (&a)[Vec16<T>::W])
{
    constexpr int W = Vec16<T>::W;
    if (vec && c + W <= end) {
        unpack16(*reinterpret_cast<const typename Vec16<T>::type*>(row + c), a);
    } else {
#pragma unroll
        for (int e = 0; e < W; ++e) a[e] = (c + e < end) ? row[c + e] : (T)0;
    }
}

// ranges: long long [5] per work-group: flags, first destination row, rows (<= HM_ROWS), first entry of ids, entries
template <typename T, int NR>
__global__ __launch_bounds__(HM_THREADS) void hmat_apply_kernel(const HmTile* __restrict__ tiles, const long long* __restrict__ ranges,
                                                               const int* __restrict__ ids, const T* __restrict__ x, T* __restrict__ y,
                                                               T* __restrict__ scratch, int nrhs, int c0, T scalar, int accumulate)
{
    constexpr int W = Vec16<T>::W, CK = 64 * W * HM_G, BW = 64 * W;
    __shared__ T yacc[HM_ROWS * NR];
    __shared__ T xs[CK * NR];
    __shared__ T red[HM_WAVES][BW * NR];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long* rg = ranges + 5 * (long long)blockIdx.x;
    const int rflags = (int)rg[0];
    const long long row0 = rg[1];
    const int nr = (int)min(rg[2], (long long)HM_ROWS);
    const int first = (int)rg[3], count = (int)rg[4];

    for (int o = tid; o < nr * NR; o += HM_THREADS) yacc[o] = (T)0;
    __syncthreads();

    for (int t = 0; t < count; ++t) {
        const HmTile tile = tiles[ids[first + t]];
        const bool diag = tile.flags & HM_DIAG, trans = tile.flags & HM_TRANS;
        const long long orows = diag ? tile.rows : (trans ? tile.cols : tile.rows);
        const long long lo = max(row0, tile.dst_off), hi = min(row0 + nr, tile.dst_off + orows);
        if (lo >= hi) continue;                                       // uniform across the work-group
        const long long i0 = lo - tile.dst_off;                       // first row of the tile served here
        const int n = (int)(hi - lo), yb = (int)(lo - row0);
        const T* src = ((tile.flags & HM_SRC_SCRATCH) ? scratch : x) + c0;
        const T* A = static_cast<const T*>(tile.a);
        const T scale = (T)tile.scale;
        const long long ld = tile.ld;
        const bool vec = aligned16(A) && (ld % W == 0);

        if (diag) {
            for (int o = tid; o < n * NR; o += HM_THREADS) {
                const int i = o / NR, r = o % NR;
                const T d = tile.cols ? A[i0 + i] : A[0];
                const T s = d * src[(tile.src_off + i0 + i) * nrhs + r];
                yacc[(yb + i) * NR + r] = tfma<T>(scale, s, yacc[(yb + i) * NR + r]);
            }
        } else if (!trans && tile.cols <= BW / 2) {
            // narrow plain form: G = 2^k >= cols / W lanes share a row, a wave load covers 64 / G adjacent rows
            const int ncols = tile.cols;
            int G = 1;
            while (G * W < ncols) G <<= 1;
            const int S = 64 / G, cg = lane % G, sub = lane / G;
            __syncthreads();                                          // the last readers of xs are done
            for (int o = tid; o < G * W * NR; o += HM_THREADS) {
                const int c = o % (G * W), r = o / (G * W);
                xs[r * CK + c] = (c < ncols) ? src[(tile.src_off + c) * nrhs + r] : (T)0;
            }
            __syncthreads();
            T xv[W][NR];
#pragma unroll
            for (int e = 0; e < W; ++e)
#pragma unroll
                for (int r = 0; r < NR; ++r) xv[e][r] = xs[r * CK + cg * W + e];
            for (int ib = wave * S; ib < n; ib += HM_WAVES * S) {     // uniform across the wave
                const int i = ib + sub;
                const bool valid = i < n;
                T a[W];
#pragma unroll
                for (int e = 0; e < W; ++e) a[e] = (T)0;
                if (valid) hm_load<T>(A + (i0 + i) * ld, cg * W, ncols, vec, a);
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    T s = (T)0;
#pragma unroll
                    for (int e = 0; e < W; ++e) s = tfma<T>(a[e], xv[e][r], s);
                    for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
                    if (valid && cg == 0) yacc[(yb + i) * NR + r] = tfma<T>(scale, s, yacc[(yb + i) * NR + r]);
                }
            }
        } else if (!trans) {
            const long long ncols = tile.cols;
            for (int sb = 0; sb < n; sb += HM_WAVES * HM_RW) {
                T acc[HM_RW][NR];
#pragma unroll
                for (int k = 0; k < HM_RW; ++k)
#pragma unroll
                    for (int r = 0; r < NR; ++r) acc[k][r] = (T)0;
                for (long long cb = 0; cb < ncols; cb += CK) {
                    __syncthreads();                                  // the last readers of xs are done
                    for (int o = tid; o < CK * NR; o += HM_THREADS) {
                        const int c = o % CK, r = o / CK;             // right-hand-side major: a lane's W columns are 16 bytes
                        xs[o] = (cb + c < ncols) ? src[(tile.src_off + cb + c) * nrhs + r] : (T)0;
                    }
                    __syncthreads();
#pragma unroll
                    for (int k = 0; k < HM_RW; ++k) {
                        const int i = sb + k * HM_WAVES + wave;
                        if (i < n) {                                  // uniform across the wave
                            const T* row = A + (i0 + i) * ld;
#pragma unroll
                            for (int g = 0; g < HM_G; ++g) {
                                const int c = (g * 64 + lane) * W;
                                T a[W];
                                hm_load<T>(row, cb + c, ncols, vec, a);
#pragma unroll
                                for (int e = 0; e < W; ++e)
#pragma unroll
                                    for (int r = 0; r < NR; ++r) acc[k][r] = tfma<T>(a[e], xs[r * CK + c + e], acc[k][r]);
                            }
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < HM_RW; ++k) {
                    const int i = sb + k * HM_WAVES + wave;
                    if (i < n) {
#pragma unroll
                        for (int r = 0; r < NR; ++r) {
                            T s = acc[k][r];                      // wave_sum (lane_vec.h) written out: the call changes this
#pragma unroll                                                    // kernel's register allocation
                            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
                            if (lane == 0) yacc[(yb + i) * NR + r] = tfma<T>(scale, s, yacc[(yb + i) * NR + r]);
                        }
                    }
                }
            }
        } else {
            // transposed form; narrow (cols <= BW / 2): G = 2^k >= cols / W lanes cover the outputs, a wave load 64 / G stored rows
            const long long nin = tile.rows, nout = tile.cols;
            int G = 64;
            if (nout <= BW / 2) {
                G = 1;
                while (G * W < nout) G <<= 1;
            }
            const int S = 64 / G, cg = lane % G, sub = lane / G, GW = G * W;
            for (long long ib = (i0 / BW) * BW; ib < i0 + n; ib += BW) {
                const long long i = ib + cg * W;                      // a multiple of W: 16-byte aligned when vec
                const bool active = i + W > i0 && i < i0 + n;
                T acc[W][NR];
#pragma unroll
                for (int e = 0; e < W; ++e)
#pragma unroll
                    for (int r = 0; r < NR; ++r) acc[e][r] = (T)0;
                if (active) {
#pragma unroll 2
                    for (long long j = wave * S + sub; j < nin; j += HM_WAVES * S) {
                        T a[W];
                        hm_load<T>(A + j * ld, i, nout, vec, a);
                        const T* xj = src + (tile.src_off + j) * nrhs;
#pragma unroll
                        for (int r = 0; r < NR; ++r) {
                            const T xv = xj[r];
#pragma unroll
                            for (int e = 0; e < W; ++e) acc[e][r] = tfma<T>(a[e], xv, acc[e][r]);
                        }
                    }
                }
                __syncthreads();                                      // the last readers of red are done
#pragma unroll
                for (int e = 0; e < W; ++e)
#pragma unroll
                    for (int r = 0; r < NR; ++r) red[wave][(lane * W + e) * NR + r] = acc[e][r];
                __syncthreads();
                for (int o = tid; o < GW * NR; o += HM_THREADS) {
                    const int il = o / NR, r = o % NR;
                    const long long ig = ib + il;
                    if (ig >= i0 && ig < i0 + n) {
                        T s = red[0][il * NR + r];                    // chains in the order (wave, row slot): wave 0 slot 0, 1, ...
                        for (int q = 1; q < HM_WAVES * S; ++q) s += red[q / S][((q % S) * GW + il) * NR + r];
                        const int yo = (yb + (int)(ig - i0)) * NR + r;
                        yacc[yo] = tfma<T>(scale, s, yacc[yo]);
                    }
                }
            }
        }
        __syncthreads();
    }

    const bool to_scratch = rflags & HM_DST_SCRATCH;
    const bool add = !to_scratch && (accumulate || (rflags & HM_ACCUMULATE));
    T* dst = (to_scratch ? scratch : y) + c0;
    for (int o = tid; o < nr * NR; o += HM_THREADS) {
        T* p = dst + (row0 + o / NR) * nrhs + o % NR;
        *p = to_scratch ? yacc[o] : (add ? tfma<T>(scalar, yacc[o], *p) : scalar * yacc[o]);
    }
}

template <typename T, int NR>
static void hm_launch(const void* tiles, const long long* ranges, const int* ids, int nranges, const void* x, void* y, void* scratch,
                      int nrhs, int c0, double scalar, int accumulate, hipStream_t st)
{
    hipLaunchKernelGGL((hmat_apply_kernel<T, NR>), dim3((unsigned)nranges), dim3(HM_THREADS), 0, st, (const HmTile*)tiles, ranges, ids,
                       (const T*)x, (T*)y, (T*)scratch, nrhs, c0, (T)scalar, accumulate);
}

template <typename T>
static int hm_apply(const void* tiles, const long long* ranges, const int* ids, const int* stage_first, int nstages, const void* x,
                    void* y, void* scratch, int nrhs, double scalar, int accumulate, hipStream_t st)
{
    for (int c0 = 0; c0 < nrhs; c0 += HM_NR) {
        const int nr = std::min(HM_NR, nrhs - c0);
        for (int s = 0; s < nstages; ++s) {
            const int n = stage_first[s + 1] - stage_first[s];
            if (n == 0) continue;
            const long long* rg = ranges + 5 * (long long)stage_first[s];
            switch (nr) {
            case 1: hm_launch<T, 1>(tiles, rg, ids, n, x, y, scratch, nrhs, c0, scalar, accumulate, st); break;
            case 2: hm_launch<T, 2>(tiles, rg, ids, n, x, y, scratch, nrhs, c0, scalar, accumulate, st); break;
            case 3: hm_launch<T, 3>(tiles, rg, ids, n, x, y, scratch, nrhs, c0, scalar, accumulate, st); break;
            default: hm_launch<T, 4>(tiles, rg, ids, n, x, y, scratch, nrhs, c0, scalar, accumulate, st); break;
            }
            const int rc = check_launch();
            if (rc != RIME_OK) return rc;
        }
    }
    return RIME_OK;
}

} // namespace rime

using namespace rime;

extern "C" size_t rime_hmat_workspace(int dtype, long long scratch_rows, int nrhs)
{
    if (!real_dtype_ok(dtype) || scratch_rows < 0 || nrhs < 1 || scratch_rows > 0x0fffffffffffffffLL / nrhs) return 0;
    return (size_t)scratch_rows * (size_t)nrhs * real_bytes(dtype);
}

extern "C" int rime_hmat_apply(int dtype, const void* tiles, int ntiles, const long long* ranges, const int* tile_ids,
                               const int* stage_first, int nstages, long long scratch_rows, const void* x, void* y, int nrhs,
                               double scalar, int accumulate, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!real_dtype_ok(dtype)) return RIME_EINVAL;
    if (ntiles < 0 || nstages < 1 || nstages > HM_MAXSTAGES || nrhs < 1 || scratch_rows < 0) return RIME_EINVAL;
    if (scratch_rows > 0x0fffffffffffffffLL / nrhs) return RIME_EINVAL;
    if (!ranges || !stage_first || !x || !y || (ntiles > 0 && (!tiles || !tile_ids))) return RIME_EINVAL;
    if (stage_first[0] < 0) return RIME_EINVAL;
    for (int s = 0; s < nstages; ++s)
        if (stage_first[s + 1] < stage_first[s]) return RIME_EINVAL;
    if (scratch_rows > 0 && (!workspace || workspace_bytes < rime_hmat_workspace(dtype, scratch_rows, nrhs))) return RIME_EWORKSPACE;
    return with_real(dtype, [&](auto t) {
        return hm_apply<decltype(t)>(tiles, ranges, tile_ids, stage_first, nstages, x, y, workspace, nrhs, scalar, accumulate,
                                     as_stream(stream));
    });
}
