// partred.hip -- the sparse learnable mixing of calibration.PartialRedVisInflate (calibration.py:2178-2344):
//     out[p, i, t, f] = sum over the entries e of row i, in list order, of  c[e] * V[p, col[e], t, f]      c real, one per entry
// The reference builds a CSR matrix on every forward, moves the baseline axis to the front (a copy), calls torch.sparse.mm on
// the real and the imaginary plane and recombines: about six passes over the visibility tensor, an atomic scatter for the
// gradient of V and a dense gradient of the sparse matrix for that of c.  Here:
// Forward (partred_fwd_kernel): ONE pass.  Lanes run along (baseline, time, channel) of the output, so the rows of V are read
//   coalesced; V is read through element strides (a sliced or expanded view needs no copy); a row's entries are added in list
//   order with one FMA per real component and term; a row without entries gets 0.
// Gradient of V (partred_bwd_data_kernel): gV[p, j, t, f] = sum over the entries e of column j, ascending entry number, of
//   c[e] * G[p, row[e], t, f], a SEGMENTED reduction over the column CSR (coff, cmem) built on the host, as redvis_bwd_kernel:
//   one block owns PR_COLS consecutive (time, channel) columns of one (pol entry, column j); its PR_WAVES waves take the members
//   w, w + PR_WAVES, ... of the list, each wave adds its members in ascending order, wave 0 adds the partial sums from LDS in
//   wave order.  A column without entries gets 0.
// Gradient of c (partred_bwd_coeff_kernel): gc[e] = sum over (p, t, f) of Re V Re G + Im V Im G, V = V[p, col[e], t, f],
//   G = G[p, row[e], t, f]: one block per output row; it takes the row's entries in chunks of PR_ECH, and for a chunk sweeps the
//   L = NP^2 Nt Nf elements of the row of G once (thread k holds elements k, k + PR_THREADS, ...), so a row of G is read once
//   per chunk and not once per entry.  Order of every sum: the lane's chain in T (ascending element, the real product first,
//   the imaginary one fused onto it), then float64: the butterfly across the wave (partners 32, 16, ..., 1), the waves in order
//   by thread 0, rounded to T once.
// No atomics, no workspace, no prior memset: every element of out, gV and gc is written exactly once, and every order of
// summation is a function of the tables alone, so two runs give the same bits.  Every table read is clamped to the buffers.
#include <hip/hip_runtime.h>
#include "rime_common.h"
#include "cplx.h"
#include "lane_vec.h"

namespace rime {

constexpr int PR_WAVES = 4;          // waves of a block = slices of a column's member list (gradient of V)
constexpr int PR_COLS = 64;          // (time, channel) columns of a block of the gradient of V = lanes of a wave
constexpr int PR_THREADS = 256;      // threads of a block of the forward and of the gradient of c
constexpr int PR_ECH = 4;            // entries of a row that one sweep of the gradient of c serves

struct PartRedArgs {
    const void* V; const void* c; void* out;                   // V strided [NP*NP, Nin, Nt, Nf] complex; c [Nnz] real; out [NP*NP, Nout, Nt, Nf]
    const void* G; void* gV; void* gc;                         // G [NP*NP, Nout, Nt, Nf]; gV [NP*NP, Nin, Nt, Nf]; gc [Nnz] real
    const int* roff; const int* col; const int* row;           // [Nout + 1] entries of every row; [Nnz] column, [Nnz] row of an entry
    const int* coff; const int* cmem;                          // [Nin + 1], [Nnz]: the entries of every column, ascending
    int Nout, Nin, Nnz, Nt, Nf;
    long long vst_p, vst_b, vst_t, vst_f;                      // strides of V in complex elements
};

template <typename T, int NP>
__global__ void __launch_bounds__(PR_THREADS)
partred_fwd_kernel(PartRedArgs A)
{
    const size_t plane = (size_t)A.Nout * A.Nt * A.Nf;         // complex elements per pol entry of out
    const cx<T>* V = reinterpret_cast<const cx<T>*>(A.V);
    const T* c = reinterpret_cast<const T*>(A.c);
    cx<T>* out = reinterpret_cast<cx<T>*>(A.out);
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < plane; k += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(k % A.Nf);
        const int t = (int)((k / A.Nf) % A.Nt);
        const int i = (int)(k / ((size_t)A.Nf * A.Nt));
        const int e0 = max(A.roff[i], 0), e1 = min(A.roff[i + 1], A.Nnz);      // the host checks the tables; never read outside
        const size_t vo = (size_t)t * A.vst_t + (size_t)f * A.vst_f;
        cx<T> acc[NP * NP];
#pragma unroll
        for (int p = 0; p < NP * NP; ++p) acc[p] = {T(0), T(0)};
        for (int e = e0; e < e1; ++e) {
            const int j = A.col[e];
            if ((unsigned)j >= (unsigned)A.Nin) continue;
            const T ce = c[e];
#pragma unroll
            for (int p = 0; p < NP * NP; ++p) {
                const cx<T> v = V[vo + (size_t)j * A.vst_b + (size_t)p * A.vst_p];
                acc[p].re = tfma<T>(ce, v.re, acc[p].re);
                acc[p].im = tfma<T>(ce, v.im, acc[p].im);
            }
        }
#pragma unroll
        for (int p = 0; p < NP * NP; ++p) out[(size_t)p * plane + k] = acc[p];
    }
}

template <typename T>
__global__ void __launch_bounds__(PR_WAVES * PR_COLS)
partred_bwd_data_kernel(PartRedArgs A)
{
    __shared__ cx<T> part[PR_WAVES - 1][PR_COLS];
    const cx<T>* G = reinterpret_cast<const cx<T>*>(A.G);
    const T* c = reinterpret_cast<const T*>(A.c);
    cx<T>* gV = reinterpret_cast<cx<T>*>(A.gV);
    const int lane = threadIdx.x % PR_COLS, w = threadIdx.x / PR_COLS;
    const size_t ncol = (size_t)A.Nt * A.Nf;                   // (time, channel) columns of one (pol entry, baseline)
    const size_t ntile = (ncol + PR_COLS - 1) / PR_COLS;
    const size_t nwork = (size_t)A.Nin * ntile;                // per pol entry; blockIdx.y is the pol entry
    const size_t p = blockIdx.y;
    for (size_t wk = blockIdx.x; wk < nwork; wk += gridDim.x) {                 // block-uniform trip count
        const int j = (int)(wk / ntile);
        const size_t cl = (wk % ntile) * PR_COLS + lane;
        const int m0 = max(A.coff[j], 0), m1 = min(A.coff[j + 1], A.Nnz);        // the host checks the tables; never read outside
        cx<T> acc = {T(0), T(0)};
        if (cl < ncol) {
            const size_t base = p * (size_t)A.Nout * ncol + cl;
#pragma unroll 4
            for (int m = m0 + w; m < m1; m += PR_WAVES) {
                const int e = A.cmem[m];
                if ((unsigned)e >= (unsigned)A.Nnz) continue;
                const int i = A.row[e];
                if ((unsigned)i >= (unsigned)A.Nout) continue;
                const T ce = c[e];
                const cx<T> g = G[base + (size_t)i * ncol];
                acc.re = tfma<T>(ce, g.re, acc.re);
                acc.im = tfma<T>(ce, g.im, acc.im);
            }
        }
        if (w > 0) part[w - 1][lane] = acc;
        __syncthreads();
        if (w == 0 && cl < ncol) {
#pragma unroll
            for (int k = 0; k < PR_WAVES - 1; ++k) { acc.re += part[k][lane].re; acc.im += part[k][lane].im; }
            gV[(p * A.Nin + j) * ncol + cl] = acc;
        }
        __syncthreads();                                                        // part is rewritten by the next item
    }
}

template <typename T>
__global__ void __launch_bounds__(PR_THREADS)
partred_bwd_coeff_kernel(PartRedArgs A, int NPP)
{
    __shared__ double part[PR_THREADS / 64][PR_ECH];
    const cx<T>* V = reinterpret_cast<const cx<T>*>(A.V);
    const cx<T>* G = reinterpret_cast<const cx<T>*>(A.G);
    T* gc = reinterpret_cast<T*>(A.gc);
    const int lane = threadIdx.x % 64, w = threadIdx.x / 64;
    const size_t ncol = (size_t)A.Nt * A.Nf;
    const size_t L = (size_t)NPP * ncol;                       // elements of the reduction of one entry
    for (int i = blockIdx.x; i < A.Nout; i += gridDim.x) {                      // block-uniform trip counts throughout
        const int e0 = max(A.roff[i], 0), e1 = min(A.roff[i + 1], A.Nnz);        // the host checks the tables; never read outside
        for (int eb = e0; eb < e1; eb += PR_ECH) {
            const int ne = min(PR_ECH, e1 - eb);
            size_t vb[PR_ECH];
            bool ok[PR_ECH];
            T acc[PR_ECH];
#pragma unroll
            for (int q = 0; q < PR_ECH; ++q) {
                const int j = q < ne ? A.col[eb + q] : -1;
                ok[q] = (unsigned)j < (unsigned)A.Nin;
                vb[q] = ok[q] ? (size_t)j * A.vst_b : 0;
                acc[q] = T(0);
            }
            for (size_t l = threadIdx.x; l < L; l += PR_THREADS) {
                const size_t p = l / ncol, tf = l % ncol;
                const size_t vo = p * A.vst_p + (tf / A.Nf) * A.vst_t + (tf % A.Nf) * A.vst_f;
                const cx<T> g = G[(p * A.Nout + i) * ncol + tf];
#pragma unroll
                for (int q = 0; q < PR_ECH; ++q) {
                    if (!ok[q]) continue;
                    const cx<T> v = V[vo + vb[q]];
                    acc[q] = tfma<T>(v.im, g.im, tfma<T>(v.re, g.re, acc[q]));
                }
            }
#pragma unroll
            for (int q = 0; q < PR_ECH; ++q) {
                const double s = wave_sum((double)acc[q]);
                if (lane == 0) part[w][q] = s;
            }
            __syncthreads();
            if (threadIdx.x < ne) {
                double s = part[0][threadIdx.x];
#pragma unroll
                for (int k = 1; k < PR_THREADS / 64; ++k) s += part[k][threadIdx.x];
                gc[eb + threadIdx.x] = (T)s;
            }
            __syncthreads();                                                    // part is rewritten by the next chunk
        }
    }
}

template <typename T>
static int partred_fwd_launch(const PartRedArgs& A, int NP, hipStream_t st)
{
    const size_t n = (size_t)A.Nout * A.Nt * A.Nf;
    const int nb = (int)std::min<size_t>((n + PR_THREADS - 1) / PR_THREADS, 16384);
    if (NP == 1) hipLaunchKernelGGL((partred_fwd_kernel<T, 1>), dim3(nb), dim3(PR_THREADS), 0, st, A);
    else hipLaunchKernelGGL((partred_fwd_kernel<T, 2>), dim3(nb), dim3(PR_THREADS), 0, st, A);
    return check_launch();
}

template <typename T>
static int partred_bwd_data_launch(const PartRedArgs& A, int NP, hipStream_t st)
{
    const size_t ncol = (size_t)A.Nt * A.Nf;
    const size_t nwork = (size_t)A.Nin * ((ncol + PR_COLS - 1) / PR_COLS);
    const int nb = (int)std::min<size_t>(nwork, 1u << 20);
    hipLaunchKernelGGL((partred_bwd_data_kernel<T>), dim3(nb, NP * NP), dim3(PR_WAVES * PR_COLS), 0, st, A);
    return check_launch();
}

template <typename T>
static int partred_bwd_coeff_launch(const PartRedArgs& A, int NP, hipStream_t st)
{
    const int nb = std::min(A.Nout, 1 << 20);
    hipLaunchKernelGGL((partred_bwd_coeff_kernel<T>), dim3(nb), dim3(PR_THREADS), 0, st, A, NP * NP);
    return check_launch();
}

static bool partred_args_ok(int NP, int Nout, int Nin, int Nnz, int Nt, int Nf)
{
    return (NP == 1 || NP == 2) && Nout > 0 && Nin > 0 && Nnz > 0 && Nt > 0 && Nf > 0;
}

} // namespace rime

using namespace rime;

extern "C" int rime_partred_fwd(int dtype, int NP, const void* V, const void* c, const int* roff, const int* col,
                                int Nout, int Nin, int Nnz, int Nt, int Nf, long long vst_p, long long vst_b,
                                long long vst_t, long long vst_f, void* out, void* stream)
{
    if (!real_dtype_ok(dtype) || !V || !c || !roff || !col || !out || !partred_args_ok(NP, Nout, Nin, Nnz, Nt, Nf)) return RIME_EINVAL;
    if (vst_p < 0 || vst_b < 0 || vst_t < 0 || vst_f < 0) return RIME_EINVAL;
    PartRedArgs A{};
    A.V = V; A.c = c; A.roff = roff; A.col = col; A.out = out;
    A.Nout = Nout; A.Nin = Nin; A.Nnz = Nnz; A.Nt = Nt; A.Nf = Nf;
    A.vst_p = vst_p; A.vst_b = vst_b; A.vst_t = vst_t; A.vst_f = vst_f;
    return with_real(dtype, [&](auto t) { return partred_fwd_launch<decltype(t)>(A, NP, as_stream(stream)); });
}

extern "C" int rime_partred_bwd_data(int dtype, int NP, const void* G, const void* c, const int* row, const int* coff,
                                     const int* cmem, int Nout, int Nin, int Nnz, int Nt, int Nf, void* gV, void* stream)
{
    if (!real_dtype_ok(dtype) || !G || !c || !row || !coff || !cmem || !gV || !partred_args_ok(NP, Nout, Nin, Nnz, Nt, Nf))
        return RIME_EINVAL;
    PartRedArgs A{};
    A.G = G; A.c = c; A.row = row; A.coff = coff; A.cmem = cmem; A.gV = gV;
    A.Nout = Nout; A.Nin = Nin; A.Nnz = Nnz; A.Nt = Nt; A.Nf = Nf;
    return with_real(dtype, [&](auto t) { return partred_bwd_data_launch<decltype(t)>(A, NP, as_stream(stream)); });
}

extern "C" int rime_partred_bwd_coeff(int dtype, int NP, const void* V, const void* G, const int* roff, const int* col,
                                      int Nout, int Nin, int Nnz, int Nt, int Nf, long long vst_p, long long vst_b,
                                      long long vst_t, long long vst_f, void* gc, void* stream)
{
    if (!real_dtype_ok(dtype) || !V || !G || !roff || !col || !gc || !partred_args_ok(NP, Nout, Nin, Nnz, Nt, Nf)) return RIME_EINVAL;
    if (vst_p < 0 || vst_b < 0 || vst_t < 0 || vst_f < 0) return RIME_EINVAL;
    PartRedArgs A{};
    A.V = V; A.G = G; A.roff = roff; A.col = col; A.gc = gc;
    A.Nout = Nout; A.Nin = Nin; A.Nnz = Nnz; A.Nt = Nt; A.Nf = Nf;
    A.vst_p = vst_p; A.vst_b = vst_b; A.vst_t = vst_t; A.vst_f = vst_f;
    return with_real(dtype, [&](auto t) { return partred_bwd_coeff_launch<decltype(t)>(A, NP, as_stream(stream)); });
}
