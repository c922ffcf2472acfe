// icov.hip -- correlated-noise likelihood of the RIME path (gfx950): the quadratic form of a residual with an inverse
// covariance that couples ONE data axis (optim.apply_icov, cov_axis 'bl' / 'time' / 'freq' / 'pix'; DESIGN.md, "Axis covariances").
//     data viewed as (O, n, I), covariance axis in the middle; icov (O*I, n, n), batch b = o*I + i, rows contiguous
//     r = pred - data;   y[o,a,i] = sum_c W[b][a][c] r[o,c,i];   q[b] = Re sum_a conj(r[o,a,i]) y[o,a,i];   chi^2 = sum_b q[b]
//     backward: gpred[o,a,i] = 2 g y[o,a,i]   (W Hermitian -- an inverse covariance; not checked)
// HBM-bound on W (n^2 complex per batch, about one flop per byte): W is read exactly once, 16 bytes per lane and load, a
// row by a group of L = 8..64 lanes (chosen from n), four rows per group and pass so that a lane has several loads in
// flight and reads r from LDS once for four rows.  r is staged in LDS once per work-group for a tile of T consecutive
// batches (T consecutive inner indices: whole 64-byte segments of pred / data / y; for I = 1 T consecutive outer
// indices: one contiguous stretch).  Few, large batches: the rows of a batch are split over work-groups.
// Deterministic: per-row terms in double in LDS, summed in a fixed tree; per-work-group totals in double in the
// workspace, summed in block order by a second kernel.
#include <hip/hip_runtime.h>
#include "rime_common.h"

namespace rime {

constexpr int ICOV_THREADS = 256;
constexpr int ICOV_MAX_BLOCKS = 4096;         // 16 per CU; a work-group walks the items beyond that
constexpr int ICOV_ROWS = 4;                  // rows of W per lane group and pass
constexpr int ICOV_STAGE = 32 * 1024;         // LDS bytes of the staged residual: 4 work-groups per CU with the row terms
constexpr int ICOV_STAGE_MAX = 64 * 1024;     // ... allowed where the tile would otherwise fall below a 64-byte segment
constexpr int ICOV_MIN_ITEMS = 512;           // two work-groups per CU (256 CUs): fewer items split their rows
constexpr int ICOV_ITEM_BYTES = 32 * 1024;    // bytes of W a work-group should at least get per item

struct IcovPlan {
    int lanes, vec, T, lgT, splits, rows_per, grid, ldr, outer_tile;
    size_t stage_bytes, lds_bytes;
    long long NO, NI, ntiles, items;
};

// The one place where (dtype, O, n, I) becomes lanes per row, tile, row splits and grid ("Axis covariances").
static int icov_plan(int dtype, long long O, int n, long long I, IcovPlan& p)
{
    if (!real_dtype_ok(dtype) || O <= 0 || n <= 0 || I <= 0) return RIME_EINVAL;
    if ((double)O * (double)I * (double)n * (double)n >= 4.0e18) return RIME_EINVAL;
    const int cb = 2 * real_bytes(dtype);
    p.vec = (dtype == RIME_F32 && n % 2 == 0) ? 2 : 1;          // complex numbers per 16-byte load (odd n, float: 8-byte loads)
    const int nv = n / p.vec;
    p.lanes = nv <= 8 ? 8 : nv <= 16 ? 16 : nv <= 32 ? 32 : 64;
    p.ldr = p.vec == 2 ? n + 2 : (dtype == RIME_F32 ? (n + 2) & ~1 : n + 1);   // padded LDS row, a multiple of 16 bytes
    p.outer_tile = I == 1;
    p.NO = p.outer_tile ? 1 : O;
    p.NI = p.outer_tile ? O : I;
    const size_t row = (size_t)p.ldr * cb;
    const int Tgood = 64 / cb;                                   // a 64-byte segment of the data
    int T = p.outer_tile ? 1 : 128 / cb;                         // I = 1: the tile is contiguous whatever its length
    while (T < ICOV_THREADS && (double)T * n * n * cb < ICOV_ITEM_BYTES) T *= 2;
    while (T > 1 && T / 2 >= p.NI) T /= 2;
    while (T > 1 && T * row > (size_t)ICOV_STAGE && !(T <= Tgood && T * row <= (size_t)ICOV_STAGE_MAX)) T /= 2;
    if (T * row > (size_t)ICOV_STAGE_MAX) return RIME_EUNSUPPORTED;
    p.T = T;
    p.lgT = 0;
    while ((1 << p.lgT) < T) ++p.lgT;
    p.ntiles = (p.NI + T - 1) / T;
    const long long tiles = p.NO * p.ntiles;
    int S = 1;
    if (tiles < ICOV_MIN_ITEMS) S = (int)std::min<long long>((ICOV_MIN_ITEMS + tiles - 1) / tiles, (n + ICOV_ROWS - 1) / ICOV_ROWS);
    p.rows_per = ((n + S - 1) / S + ICOV_ROWS - 1) / ICOV_ROWS * ICOV_ROWS;
    p.splits = (n + p.rows_per - 1) / p.rows_per;
    p.items = tiles * p.splits;
    p.grid = (int)std::min<long long>(p.items, ICOV_MAX_BLOCKS);
    p.stage_bytes = T * row;
    p.lds_bytes = p.stage_bytes + ((size_t)p.rows_per * T + ICOV_THREADS) * sizeof(double);
    return RIME_OK;
}

static size_t icov_workspace(const IcovPlan& p)
{
    return (size_t)ICOV_MAX_BLOCKS * sizeof(double)
         + (p.splits > 1 ? (size_t)p.NO * p.NI * p.splits * sizeof(double) : 0);
}

struct IcovArgs {
    long long NI, ntiles, items;
    int n, T, lgT, splits, rows_per, ldr, outer_tile;
};

template <typename T, int VEC> struct icov_vec;
template <> struct icov_vec<float, 2> { using type = float4; };
template <> struct icov_vec<float, 1> { using type = float2; };
template <> struct icov_vec<double, 1> { using type = double2; };

// acc += w * r for VEC complex numbers
template <typename T, int VEC, typename V>
__device__ __forceinline__ void icov_mac(const V& w, const V& r, T& re, T& im)
{
    re = tfma<T>(w.x, r.x, re); re = tfma<T>(-w.y, r.y, re); im = tfma<T>(w.x, r.y, im); im = tfma<T>(w.y, r.x, im);
    if constexpr (VEC == 2) {
        re = tfma<T>(w.z, r.z, re); re = tfma<T>(-w.w, r.w, re); im = tfma<T>(w.z, r.w, im); im = tfma<T>(w.w, r.z, im);
    }
}

template <typename T, int L, int VEC>
__global__ void __launch_bounds__(ICOV_THREADS)
icov_fwd_kernel(const T* __restrict__ pred, const T* __restrict__ data, const T* __restrict__ icov, IcovArgs A,
                T* __restrict__ y, T* __restrict__ q, double* __restrict__ qpart, double* __restrict__ wpart)
{
    using V = typename icov_vec<T, VEC>::type;
    using C = typename icov_vec<T, 1>::type;
    extern __shared__ __align__(16) unsigned char smem[];
    C* rs = reinterpret_cast<C*>(smem);                                            // [T][ldr] residual
    double* term = reinterpret_cast<double*>(smem + (size_t)A.T * A.ldr * sizeof(C));   // [rows_per][T] Re(conj(r_a) y_a)
    double* red = term + (size_t)A.rows_per * A.T;                                 // [256]
    const C* predc = reinterpret_cast<const C*>(pred);
    const C* datac = reinterpret_cast<const C*>(data);
    C* yc = reinterpret_cast<C*>(y);
    constexpr int G = ICOV_THREADS / L;
    const int tid = threadIdx.x, grp = tid / L, lane = tid % L;
    const int n = A.n, TT = A.T, ldr = A.ldr, nv = n / VEC;
    const long long NI = A.NI;
    double total = 0.0;

    for (long long item = blockIdx.x; item < A.items; item += gridDim.x) {
        const int s = (int)(item % A.splits);
        const long long rest = item / A.splits, tile = rest % A.ntiles, o = rest / A.ntiles;
        const long long i0 = tile * TT;
        const int tv = (int)((NI - i0) < (long long)TT ? (NI - i0) : (long long)TT);
        const int a0 = s * A.rows_per, a1 = (a0 + A.rows_per) < n ? (a0 + A.rows_per) : n, nrows = a1 - a0;
        // element (t, c) of the tile: outer tile (I = 1): (i0 + t) n + c; else (o n + c) NI + i0 + t
        if (A.outer_tile) {
            const long long base = i0 * n;
            for (int j = tid; j < tv * n; j += ICOV_THREADS) {
                const int t = j / n, c = j - t * n;
                C v = predc[base + j];
                if (datac) { const C d = datac[base + j]; v.x -= d.x; v.y -= d.y; }
                rs[t * ldr + c] = v;
            }
        } else {
            const long long base = o * n * NI + i0;
            for (int j = tid; j < (n << A.lgT); j += ICOV_THREADS) {
                const int c = j >> A.lgT, t = j & (TT - 1);
                if (t < tv) {
                    C v = predc[base + c * NI + t];
                    if (datac) { const C d = datac[base + c * NI + t]; v.x -= d.x; v.y -= d.y; }
                    rs[t * ldr + c] = v;
                }
            }
        }
        __syncthreads();

        const int ntask = (nrows + ICOV_ROWS - 1) / ICOV_ROWS * tv;                // t fastest
        for (int task = grp; task < ntask; task += G) {
            const int rb = task / tv, t = task - rb * tv;
            const int ar = a0 + rb * ICOV_ROWS;
            const long long b = o * NI + i0 + t;
            const V* W = reinterpret_cast<const V*>(icov) + (size_t)b * n * nv;
            const V* w[ICOV_ROWS];
#pragma unroll
            for (int j = 0; j < ICOV_ROWS; ++j) w[j] = W + (size_t)((ar + j) < a1 ? (ar + j) : (a1 - 1)) * nv;
            const V* rv = reinterpret_cast<const V*>(rs + t * ldr);
            T re[ICOV_ROWS], im[ICOV_ROWS];
#pragma unroll
            for (int j = 0; j < ICOV_ROWS; ++j) re[j] = im[j] = T(0);
#pragma unroll 2
            for (int k = lane; k < nv; k += L) {
                V wv[ICOV_ROWS];
#pragma unroll
                for (int j = 0; j < ICOV_ROWS; ++j) wv[j] = w[j][k];
                const V r = rv[k];
#pragma unroll
                for (int j = 0; j < ICOV_ROWS; ++j) icov_mac<T, VEC>(wv[j], r, re[j], im[j]);
            }
#pragma unroll
            for (int off = L / 2; off > 0; off >>= 1) {
#pragma unroll
                for (int j = 0; j < ICOV_ROWS; ++j) {
                    re[j] += __shfl_xor(re[j], off, 64);
                    im[j] += __shfl_xor(im[j], off, 64);
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < ICOV_ROWS; ++j) {
                    const int a = ar + j;
                    if (a < a1) {
                        const C r = rs[t * ldr + a];
                        term[(a - a0) * TT + t] = (double)r.x * (double)re[j] + (double)r.y * (double)im[j];
                        if (yc) {
                            C out; out.x = re[j]; out.y = im[j];
                            yc[A.outer_tile ? (i0 + t) * n + a : (o * n + a) * NI + i0 + t] = out;
                        }
                    }
                }
            }
        }
        __syncthreads();

        // q of the tile's batches: thread (row slot, t) sums its rows in order, then a fixed tree over the row slots
        {
            const int t = tid & (TT - 1), J = ICOV_THREADS >> A.lgT;
            double acc = 0.0;
            if (t < tv)
                for (int al = tid >> A.lgT; al < nrows; al += J) acc += term[al * TT + t];
            red[tid] = acc;
        }
        __syncthreads();
        for (int st = ICOV_THREADS / 2; st >= TT; st >>= 1) {
            if (tid < st) red[tid] += red[tid + st];
            __syncthreads();
        }
        if (tid < tv) {
            const long long b = o * NI + i0 + tid;
            if (A.splits > 1) qpart[b * A.splits + s] = red[tid];
            else if (q) q[b] = (T)red[tid];
        }
        __syncthreads();
        for (int st = TT / 2; st > 0; st >>= 1) {
            if (tid < st) red[tid] += red[tid + st];
            __syncthreads();
        }
        if (tid == 0) total += red[0];
    }
    if (tid == 0) wpart[blockIdx.x] = total;
}

// q[b] = sum of its row splits' partials, in split order
template <typename T>
__global__ void __launch_bounds__(256)
icov_q_kernel(const double* __restrict__ qpart, long long nb, int splits, T* __restrict__ q)
{
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += (long long)gridDim.x * blockDim.x) {
        double acc = 0.0;
        for (int s = 0; s < splits; ++s) acc += qpart[b * splits + s];
        q[b] = (T)acc;
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
icov_final_kernel(const double* __restrict__ partial, int nb, T* __restrict__ out)
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

// gpred[o,a,i] = 2 g y[o,a,i]; g one scalar (per_batch 0) or g[o I + i]
template <typename T>
__global__ void __launch_bounds__(256)
icov_bwd_kernel(const T* __restrict__ y, const T* __restrict__ g, int per_batch, size_t N, long long nI, long long I,
                T* __restrict__ gpred)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < N; e += (size_t)gridDim.x * blockDim.x) {
        const T w = T(2) * (per_batch ? g[(long long)(e / nI) * I + (long long)(e % I)] : g[0]);
        gpred[2 * e] = w * y[2 * e];
        gpred[2 * e + 1] = w * y[2 * e + 1];
    }
}

template <typename T, int L, int VEC>
static int icov_launch(const IcovPlan& p, const IcovArgs& A, const void* pred, const void* data, const void* icov, void* y,
                       void* q, double* qpart, double* wpart, hipStream_t st)
{
    if (p.lds_bytes > 48 * 1024) {
        // the attribute belongs to the (function, device) pair: remembered per device of the calling thread
        static unsigned long long configured = 0ull;
        int devid = 0;
        if (hipGetDevice(&devid) != hipSuccess) devid = 0;
        const unsigned long long bit = 1ull << (devid & 63);
        if (!(configured & bit)) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&icov_fwd_kernel<T, L, VEC>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
                return check_launch();
            configured |= bit;
        }
    }
    hipLaunchKernelGGL((icov_fwd_kernel<T, L, VEC>), dim3(p.grid), dim3(ICOV_THREADS), p.lds_bytes, st, (const T*)pred,
                       (const T*)data, (const T*)icov, A, (T*)y, (T*)q, qpart, wpart);
    return check_launch();
}

template <typename T, int VEC>
static int icov_launch_lanes(const IcovPlan& p, const IcovArgs& A, const void* pred, const void* data, const void* icov,
                             void* y, void* q, double* qpart, double* wpart, hipStream_t st)
{
    switch (p.lanes) {
    case 8: return icov_launch<T, 8, VEC>(p, A, pred, data, icov, y, q, qpart, wpart, st);
    case 16: return icov_launch<T, 16, VEC>(p, A, pred, data, icov, y, q, qpart, wpart, st);
    case 32: return icov_launch<T, 32, VEC>(p, A, pred, data, icov, y, q, qpart, wpart, st);
    default: return icov_launch<T, 64, VEC>(p, A, pred, data, icov, y, q, qpart, wpart, st);
    }
}

} // namespace rime

using namespace rime;

extern "C" int rime_icov_plan(int dtype, long long O, int n, long long I, int* plan_host)
{
    if (!plan_host) return RIME_EINVAL;
    IcovPlan p;
    const int rc = icov_plan(dtype, O, n, I, p);
    if (rc != RIME_OK) return rc;
    const int out[10] = {p.lanes, p.vec, p.T, p.splits, p.rows_per, p.grid, (int)p.stage_bytes, (int)p.lds_bytes,
                         ICOV_STAGE_MAX, p.outer_tile};
    std::memcpy(plan_host, out, sizeof(out));
    return RIME_OK;
}

extern "C" size_t rime_icov_workspace(int dtype, long long O, int n, long long I)
{
    IcovPlan p;
    return icov_plan(dtype, O, n, I, p) == RIME_OK ? icov_workspace(p) : 0;
}

extern "C" int rime_icov_fwd(int dtype, const void* pred, const void* data, const void* icov, long long O, int n,
                             long long I, void* y, void* q, void* out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!pred || !icov || O <= 0 || n <= 0 || I <= 0) return RIME_EINVAL;
    if (!y && !q && !out) return RIME_EINVAL;
    // one complex number per access of pred / data / y: 8 bytes (RIME_F32) or 16 (RIME_F64, also any unknown dtype)
    const uintptr_t cmask = dtype == RIME_F32 ? 7 : 15;
    if (((uintptr_t)icov & 15) || ((uintptr_t)pred & cmask) || ((uintptr_t)data & cmask) || ((uintptr_t)y & cmask)) return RIME_EINVAL;
    IcovPlan p;
    const int rc = icov_plan(dtype, O, n, I, p);
    if (rc != RIME_OK) return rc;
    if (!workspace || workspace_bytes < icov_workspace(p)) return RIME_EWORKSPACE;
    double* wpart = (double*)workspace;
    double* qpart = p.splits > 1 ? wpart + ICOV_MAX_BLOCKS : nullptr;
    const IcovArgs A = {p.NI, p.ntiles, p.items, n, p.T, p.lgT, p.splits, p.rows_per, p.ldr, p.outer_tile};
    hipStream_t st = as_stream(stream);
    return with_real(dtype, [&](auto t) {
        using T = decltype(t);
        int r;
        if constexpr (std::is_same<T, float>::value) {
            r = p.vec == 2 ? icov_launch_lanes<float, 2>(p, A, pred, data, icov, y, q, qpart, wpart, st)
                           : icov_launch_lanes<float, 1>(p, A, pred, data, icov, y, q, qpart, wpart, st);
        } else {
            r = icov_launch_lanes<double, 1>(p, A, pred, data, icov, y, q, qpart, wpart, st);
        }
        if (r != RIME_OK) return r;
        const long long nb = O * I;
        if (q && p.splits > 1)
            hipLaunchKernelGGL((icov_q_kernel<T>), dim3((unsigned)std::min<long long>((nb + 255) / 256, 4096)), dim3(256), 0, st,
                               qpart, nb, p.splits, (T*)q);
        if (out)
            hipLaunchKernelGGL((icov_final_kernel<T>), dim3(1), dim3(256), 0, st, wpart, p.grid, (T*)out);
        return check_launch();
    });
}

extern "C" int rime_icov_bwd(int dtype, const void* y, const void* g, int g_per_batch, long long O, int n, long long I,
                             void* gpred, void* stream)
{
    if (!y || !g || !gpred || O <= 0 || n <= 0 || I <= 0 || (g_per_batch != 0 && g_per_batch != 1)) return RIME_EINVAL;
    if ((double)O * (double)I * (double)n >= 4.0e18) return RIME_EINVAL;
    const size_t N = (size_t)O * n * I;
    const int nb = (int)std::min<size_t>((N + 255) / 256, 8192);
    return with_real(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((icov_bwd_kernel<T>), dim3(nb), dim3(256), 0, as_stream(stream), (const T*)y, (const T*)g,
                           g_per_batch, N, (long long)n * I, I, (T*)gpred);
        return check_launch();
    });
}
