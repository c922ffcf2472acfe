// redvis.hip -- the redundant-visibility (and per-baseline visibility) model term of calibration.RedVisModel / VisModel
// (calibration.py:877-1209):
//     out[p, b, t, f] = vis[p, b, t, f] + sign * model[p, red[b], tmap[t], f]
// Forward: the baseline gather, the time selection and the add in ONE pass over the visibility tensor (the reference makes two
// gathered copies of the model, each the size of vis, and adds).  The model is read through element strides, so a broadcast or
// sliced view needs no copy.
// Backward: gmodel[p, r, t', f] = sign * sum_{t: tmap[t] = t'} sum_{b: red[b] = r} gout[p, b, t, f] as a SEGMENTED reduction
// over two CSR tables built on the host (members of every group, members of every model time), in place of the atomic
// scatter-add that autograd gives index_select.  One block owns 64 consecutive (model time, channel) columns of one
// (pol entry, group): lanes run along the columns, so member rows are read coalesced and a short channel axis is filled up with
// model times; the RV_WAVES waves of the block take the members w, w + RV_WAVES, ... of the group (a long group costs a quarter
// of its length in row reads per wave), each wave adds its members in ascending list position, and wave 0 adds the partial sums
// from LDS in wave order.  The order is a function of the tables alone: two runs give the same bits.  Every element of gmodel is
// written exactly once (groups and model times without members get 0); no atomics, no workspace, no prior memset.
#include <hip/hip_runtime.h>
#include "rime_common.h"
#include "cplx.h"

namespace rime {

constexpr int RV_WAVES = 4;          // waves of a backward block = slices of a group's member list
constexpr int RV_COLS = 64;          // columns (model time x channel) of a backward block = lanes of a wave

struct RedVisArgs {
    const void* vis; const void* model; void* out;             // vis / out [NP*NP, Nbl, Nt, Nf] complex; model strided
    const int* red; const int* tmap;                           // [Nbl] group of a baseline; [Nt] model time of a time or null
    const void* gout; void* gmodel;                            // [NP*NP, Nbl, Nt, Nf]; [NP*NP, Nred, Ntm, Nf]
    const int* goff; const int* gmem; const int* toff; const int* tmem;   // CSR: [Nred + 1], [Nbl], [Ntm + 1], [Nt]
    int Nbl, Nt, Nf, Nred, Ntm;
    long long mst_p, mst_r, mst_t, mst_f;                      // model strides in complex elements
    int sign;
};

template <typename T, int NP>
__global__ void __launch_bounds__(256)
redvis_fwd_kernel(RedVisArgs A)
{
    const size_t plane = (size_t)A.Nbl * A.Nt * A.Nf;          // complex elements per pol entry of vis
    const cx<T>* vis = reinterpret_cast<const cx<T>*>(A.vis);
    const cx<T>* model = reinterpret_cast<const cx<T>*>(A.model);
    cx<T>* out = reinterpret_cast<cx<T>*>(A.out);
    const T s = (T)A.sign;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(i % A.Nf);
        const int t = (int)((i / A.Nf) % A.Nt);
        const int b = (int)(i / ((size_t)A.Nf * A.Nt));
        const int r = A.red[b];
        const int tm = A.tmap ? A.tmap[t] : t;
        const bool in = (unsigned)r < (unsigned)A.Nred && (unsigned)tm < (unsigned)A.Ntm;    // the host checks the tables; never read outside
        const size_t mo = in ? (size_t)r * A.mst_r + (size_t)tm * A.mst_t + (size_t)f * A.mst_f : 0;
#pragma unroll
        for (int p = 0; p < NP * NP; ++p) {
            cx<T> m = model[mo + (size_t)p * A.mst_p];
            if (!in) m = {T(0), T(0)};
            cx<T> v = {T(0), T(0)};
            if (vis) v = vis[(size_t)p * plane + i];
            out[(size_t)p * plane + i] = {v.re + s * m.re, v.im + s * m.im};
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(RV_WAVES * RV_COLS)
redvis_bwd_kernel(RedVisArgs A)
{
    __shared__ cx<T> part[RV_WAVES - 1][RV_COLS];
    const cx<T>* gout = reinterpret_cast<const cx<T>*>(A.gout);
    cx<T>* gmodel = reinterpret_cast<cx<T>*>(A.gmodel);
    const int lane = threadIdx.x % RV_COLS, w = threadIdx.x / RV_COLS;
    const size_t ncol = (size_t)A.Ntm * A.Nf;                  // columns of one (pol entry, group)
    const size_t ntile = (ncol + RV_COLS - 1) / RV_COLS;
    const size_t row = (size_t)A.Nt * A.Nf;                    // complex elements of one (pol entry, baseline) of gout
    const size_t nwork = (size_t)A.Nred * ntile;               // per pol entry; blockIdx.y is the pol entry
    const size_t p = blockIdx.y;
    const T s = (T)A.sign;
    for (size_t wk = blockIdx.x; wk < nwork; wk += gridDim.x) {                 // block-uniform trip count
        const int r = (int)(wk / ntile);
        const size_t col = (wk % ntile) * RV_COLS + lane;
        const int m0 = max(A.goff[r], 0), m1 = min(A.goff[r + 1], A.Nbl);        // the host checks the tables; never read outside
        cx<T> acc = {T(0), T(0)};
        if (col < ncol) {
            const int tp = (int)(col / A.Nf), f = (int)(col % A.Nf);
            const int q0 = max(A.toff[tp], 0), q1 = min(A.toff[tp + 1], A.Nt);
            for (int q = q0; q < q1; ++q) {                                     // almost always one time per model time
                const int t = A.tmem[q];
                if ((unsigned)t >= (unsigned)A.Nt) continue;
                const size_t base = p * (size_t)A.Nbl * row + (size_t)t * A.Nf + f;
#pragma unroll 4
                for (int m = m0 + w; m < m1; m += RV_WAVES) {
                    const int b = A.gmem[m];
                    if ((unsigned)b >= (unsigned)A.Nbl) continue;
                    const cx<T> g = gout[base + (size_t)b * row];
                    acc += g;
                }
            }
        }
        if (w > 0) part[w - 1][lane] = acc;
        __syncthreads();
        if (w == 0 && col < ncol) {
#pragma unroll
            for (int k = 0; k < RV_WAVES - 1; ++k) { acc.re += part[k][lane].re; acc.im += part[k][lane].im; }
            gmodel[(p * A.Nred + r) * ncol + col] = {s * acc.re, s * acc.im};
        }
        __syncthreads();                                                        // part is rewritten by the next item
    }
}

template <typename T>
static int redvis_fwd_launch(const RedVisArgs& A, int NP, hipStream_t st)
{
    const size_t n = (size_t)A.Nbl * A.Nt * A.Nf;
    const int nb = (int)std::min<size_t>((n + 255) / 256, 16384);
    if (NP == 1) hipLaunchKernelGGL((redvis_fwd_kernel<T, 1>), dim3(nb), dim3(256), 0, st, A);
    else hipLaunchKernelGGL((redvis_fwd_kernel<T, 2>), dim3(nb), dim3(256), 0, st, A);
    return check_launch();
}

template <typename T>
static int redvis_bwd_launch(const RedVisArgs& A, int NP, hipStream_t st)
{
    const size_t ncol = (size_t)A.Ntm * A.Nf;
    const size_t nwork = (size_t)A.Nred * ((ncol + RV_COLS - 1) / RV_COLS);
    const int nb = (int)std::min<size_t>(nwork, 1u << 20);
    hipLaunchKernelGGL((redvis_bwd_kernel<T>), dim3(nb, NP * NP), dim3(RV_WAVES * RV_COLS), 0, st, A);
    return check_launch();
}

static bool redvis_args_ok(int NP, int Nbl, int Nt, int Nf, int Nred, int Ntm, int sign)
{
    return (NP == 1 || NP == 2) && Nbl > 0 && Nt > 0 && Nf > 0 && Nred > 0 && Ntm > 0 && (sign == 1 || sign == -1);
}

} // namespace rime

using namespace rime;

extern "C" int rime_redvis_fwd(int dtype, int NP, const void* vis, const void* model, const int* red, const int* tmap,
                               int Nbl, int Nt, int Nf, int Nred, int Ntm, long long mst_p, long long mst_r,
                               long long mst_t, long long mst_f, int sign, void* out, void* stream)
{
    if (!model || !red || !out || !redvis_args_ok(NP, Nbl, Nt, Nf, Nred, Ntm, sign)) return RIME_EINVAL;
    if (mst_p < 0 || mst_r < 0 || mst_t < 0 || mst_f < 0) return RIME_EINVAL;
    if (!tmap && Ntm != Nt) return RIME_EINVAL;                // the identity needs as many model times as times
    RedVisArgs A{};
    A.vis = vis; A.model = model; A.red = red; A.tmap = tmap; A.out = out;
    A.Nbl = Nbl; A.Nt = Nt; A.Nf = Nf; A.Nred = Nred; A.Ntm = Ntm;
    A.mst_p = mst_p; A.mst_r = mst_r; A.mst_t = mst_t; A.mst_f = mst_f; A.sign = sign;
    return with_real(dtype, [&](auto t) { return redvis_fwd_launch<decltype(t)>(A, NP, as_stream(stream)); });
}

extern "C" int rime_redvis_bwd(int dtype, int NP, const void* gout, const int* goff, const int* gmem, const int* toff,
                               const int* tmem, int Nbl, int Nt, int Nf, int Nred, int Ntm, int sign, void* gmodel,
                               void* stream)
{
    if (!gout || !goff || !gmem || !toff || !tmem || !gmodel || !redvis_args_ok(NP, Nbl, Nt, Nf, Nred, Ntm, sign))
        return RIME_EINVAL;
    RedVisArgs A{};
    A.gout = gout; A.goff = goff; A.gmem = gmem; A.toff = toff; A.tmem = tmem; A.gmodel = gmodel;
    A.Nbl = Nbl; A.Nt = Nt; A.Nf = Nf; A.Nred = Nred; A.Ntm = Ntm; A.sign = sign;
    return with_real(dtype, [&](auto t) { return redvis_bwd_launch<decltype(t)>(A, NP, as_stream(stream)); });
}
