// redcoupling.hip -- mutual coupling of REDUNDANT visibilities, calibration.RedVisCoupling (calibration.py:1588-2115):
//     Vc = A(eps) Vr + B(eps) conj(Vr)
// with A, B the (Nout, Nin) matrices of first-order (eps, conj eps) and second-order single-path (eps conj eps') coupling terms.
// The reference fills two dense (Nout, Nin, Nt, Nf) matrices and contracts them; here the matrices never exist.  Everything the
// forward adds up is ONE list of entries, entry e = (output row i, input column j, conjugate-the-visibility flag, a, b) with
//     coef(e) = (a >= 0 ? C[a] : 1) (b >= 0 ? conj(C[b]) : 1),     C = x o dly built on the fly,
//     out[i] = sum over the entries of row i of coef(e) (flag ? conj(data[j]) : data[j])
// (the zeroth-order term, the inflation by redundancy included, is an entry with a = b = -1), and three CSR orderings of it:
//   by row     forward:  one wave per (row, 64 columns), the row's entries in ascending order
//   by column  gdata[j] = sum over the readers of j of  conj(coef) gout[i]  (plain reader),  coef conj(gout[i])  (conjugated)
//   by term    gx[c] = conj(dly[c]) sum over the (entry, role) pairs of c of
//                          conj(w) gout[i],  w  = (b >= 0 ? conj(C[b]) : 1) v    (role a: c == a)
//                          w' conj(gout[i]), w' = (a >= 0 ? C[a] : 1) v          (role b: c == b),   v the visibility as read,
//              summed over t when Tm = 1 and over f when Fm = 1.  A term of a compressed set has ~1e5 pairs, so its list is cut
//              into segments of `seg` pairs: one wave per (segment, 64 columns) adds its pairs in ascending order into the
//              workspace, then one block per (term, tm, 64 channels) adds the segment sums: wave w the segments w, w + 4, ... in
//              ascending order (t outer of f where those are summed too), the lanes by the butterfly when Fm = 1, and wave 0 the
//              four wave sums in wave order.
// A "column" of a work item is a flattened (t, f): lanes run along it, so every access of data, gout, x and dly is a contiguous
// run and a short channel axis is filled up with times; the entry words are uniform across the wave.
// Every output element is written by exactly one thread, in an order fixed by the tables: no atomics, no prior memset, the same
// bits from run to run; rows, columns and terms without entries get zeros.  Every index followed comes from a table the caller
// has range-checked (ops.RedCouplingPlan); the kernels also skip any word that points outside.
#include <hip/hip_runtime.h>
#include "rime_common.h"
#include "cplx.h"
#include "lane_vec.h"

namespace rime {

constexpr int RC_WAVES = 4;          // waves of a block
constexpr int RC_COLS = 64;          // columns of a work item = lanes of a wave
constexpr int RC_IDX = 0x3fffffff, RC_FLAG = 0x40000000;       // column word: conjugated visibility; term word: role b

struct RcArgs {
    const void* x; const void* dly; const void* data; const void* gout;     // [Nterms][Tm][Fm], [Nterms][Nf], [Nin][Nt][Nf], [Nout][Nt][Nf]
    const int* ent;                                                         // [Nent][4]: i, j | flag, a, b
    const int* off; const int* mem;                                         // the CSR ordering of the launch
    const int* segterm; const int* segstart; const int* tsoff;              // [Nseg], [Nseg], [Nterms + 1]
    void* out; void* ws;
    int Nout, Nin, Nterms, Nent, Nmem, Nseg, seg, Nt, Nf, Tm, Fm;
};

// C[c] = x[c] o dly[c] at (t, f); c in [0, Nterms)
template <typename T>
__device__ __forceinline__ cx<T> rc_C(const RcArgs& A, int c, int t, int f)
{
    const int tt = A.Tm == 1 ? 0 : t, ff = A.Fm == 1 ? 0 : f;
    cx<T> v = reinterpret_cast<const cx<T>*>(A.x)[((size_t)c * A.Tm + tt) * A.Fm + ff];
    if (A.dly) v = cmul_fma<T>(v, reinterpret_cast<const cx<T>*>(A.dly)[(size_t)c * A.Nf + f]);
    return v;
}

template <typename T>
__device__ __forceinline__ cx<T> rc_coef(const RcArgs& A, int a, int b, int t, int f)
{
    cx<T> k = {T(1), T(0)};
    if (a >= 0) k = rc_C<T>(A, a, t, f);
    if (b >= 0) {
        const cx<T> cb = rc_C<T>(A, b, t, f);
        k = a >= 0 ? cmulc_fma<T>(k, cb) : cx<T>{cb.re, -cb.im};
    }
    return k;
}

// the entry word e, decoded; false for a word that points outside (never produced by the plan)
struct RcEntry { int i, j, cj, a, b; };
__device__ __forceinline__ bool rc_entry(const RcArgs& A, int e, RcEntry& E)
{
    if ((unsigned)e >= (unsigned)A.Nent) return false;
    const int4 q = reinterpret_cast<const int4*>(A.ent)[e];
    E.i = q.x; E.j = q.y & RC_IDX; E.cj = q.y & RC_FLAG; E.a = q.z; E.b = q.w;
    return q.y >= 0 && (unsigned)E.i < (unsigned)A.Nout && E.j < A.Nin && E.a >= -1 && E.a < A.Nterms && E.b >= -1 && E.b < A.Nterms;
}

// BWD 0: out[i] over the entries of row i (off: [Nout + 1], rows of ent are in row order);  BWD 1: gdata[j] over the readers
// of column j (off: [Nin + 1], mem: [Nent] entry numbers)
template <typename T, int BWD>
__global__ void __launch_bounds__(RC_WAVES * RC_COLS)
redcoupling_row_kernel(RcArgs A)
{
    const int lane = threadIdx.x % RC_COLS, w = threadIdx.x / RC_COLS;
    const size_t ncol = (size_t)A.Nt * A.Nf, ntile = (ncol + RC_COLS - 1) / RC_COLS;
    const int nrow = BWD ? A.Nin : A.Nout;
    const size_t nwork = (size_t)nrow * ntile;
    const cx<T>* src = reinterpret_cast<const cx<T>*>(BWD ? A.gout : A.data);
    cx<T>* out = reinterpret_cast<cx<T>*>(A.out);
    for (size_t wk = (size_t)blockIdx.x * RC_WAVES + w; wk < nwork; wk += (size_t)gridDim.x * RC_WAVES) {
        const int r = (int)(wk / ntile);
        const size_t col = (wk % ntile) * RC_COLS + lane;
        if (col >= ncol) continue;
        const int t = (int)(col / A.Nf), f = (int)(col % A.Nf);
        const int m0 = max(A.off[r], 0), m1 = min(A.off[r + 1], A.Nent);
        cx<T> acc = {T(0), T(0)};
        for (int m = m0; m < m1; ++m) {
            RcEntry E;
            if (!rc_entry(A, BWD ? A.mem[m] : m, E)) continue;
            const cx<T> k = rc_coef<T>(A, E.a, E.b, t, f);
            cx<T> v = src[(size_t)(BWD ? E.i : E.j) * ncol + col];
            if (E.cj) v.im = -v.im;                             // forward: conj(data);  backward: coef conj(g)
            if (BWD && !E.cj) cfmac<T>(acc, k, v);             // conj(coef) g
            else cfma<T>(acc, k, v);
        }
        out[(size_t)r * ncol + col] = acc;
    }
}

// ws[s][t][f] = conj(dly[c][f]) * sum over the (entry, role) pairs of segment s of term c = segterm[s], in ascending order
template <typename T>
__global__ void __launch_bounds__(RC_WAVES * RC_COLS)
redcoupling_seg_kernel(RcArgs A)
{
    const int lane = threadIdx.x % RC_COLS, w = threadIdx.x / RC_COLS;
    const size_t ncol = (size_t)A.Nt * A.Nf, ntile = (ncol + RC_COLS - 1) / RC_COLS;
    const size_t nwork = (size_t)A.Nseg * ntile;
    const cx<T>* data = reinterpret_cast<const cx<T>*>(A.data);
    const cx<T>* gout = reinterpret_cast<const cx<T>*>(A.gout);
    cx<T>* ws = reinterpret_cast<cx<T>*>(A.ws);
    for (size_t wk = (size_t)blockIdx.x * RC_WAVES + w; wk < nwork; wk += (size_t)gridDim.x * RC_WAVES) {
        const int s = (int)(wk / ntile);
        const size_t col = (wk % ntile) * RC_COLS + lane;
        if (col >= ncol) continue;
        const int t = (int)(col / A.Nf), f = (int)(col % A.Nf);
        const int c = A.segterm[s];
        cx<T> acc = {T(0), T(0)};
        if ((unsigned)c < (unsigned)A.Nterms) {
            const int m0 = max(A.segstart[s], 0);
            const int m1 = min(min(m0 + A.seg, A.off[c + 1]), A.Nmem);
            for (int m = m0; m < m1; ++m) {
                const int word = A.mem[m];
                RcEntry E;
                if (word < 0 || !rc_entry(A, word & RC_IDX, E)) continue;
                cx<T> v = data[(size_t)E.j * ncol + col];
                if (E.cj) v.im = -v.im;
                const cx<T> g = gout[(size_t)E.i * ncol + col];
                if (word & RC_FLAG) {                           // role b: w' conj(g)
                    if (E.a >= 0) v = cmul_fma<T>(rc_C<T>(A, E.a, t, f), v);
                    cfma<T>(acc, v, cx<T>{g.re, -g.im});
                } else {                                        // role a: conj(w) g
                    if (E.b >= 0) v = cmulc_fma<T>(v, rc_C<T>(A, E.b, t, f));
                    cfmac<T>(acc, v, g);
                }
            }
            if (A.dly) acc = cmulc_fma<T>(acc, reinterpret_cast<const cx<T>*>(A.dly)[(size_t)c * A.Nf + f]);
        }
        ws[(size_t)s * ncol + col] = acc;
    }
}

// gx[c][tm][fm] = sum of ws over the segments of term c (and over t, f where x broadcasts), in the order given at the top
template <typename T>
__global__ void __launch_bounds__(RC_WAVES * RC_COLS)
redcoupling_combine_kernel(RcArgs A)
{
    __shared__ cx<T> part[RC_WAVES - 1][RC_COLS];
    const int lane = threadIdx.x % RC_COLS, w = threadIdx.x / RC_COLS;
    const cx<T>* ws = reinterpret_cast<const cx<T>*>(A.ws);
    cx<T>* gx = reinterpret_cast<cx<T>*>(A.out);
    const int nft = A.Fm == 1 ? 1 : (A.Nf + RC_COLS - 1) / RC_COLS;
    const size_t nwork = (size_t)A.Nterms * A.Tm * nft;
    for (size_t wk = blockIdx.x; wk < nwork; wk += gridDim.x) {                  // block-uniform trip count
        const int ft = (int)(wk % nft), tm = (int)((wk / nft) % A.Tm), c = (int)(wk / ((size_t)nft * A.Tm));
        const int s0 = max(A.tsoff[c], 0), s1 = min(A.tsoff[c + 1], A.Nseg);
        const int ta = A.Tm == 1 ? 0 : tm, tb = A.Tm == 1 ? A.Nt : tm + 1;
        const int fa = ft * RC_COLS + lane, fb = A.Fm == 1 ? A.Nf : min(fa + 1, A.Nf);
        cx<T> acc = {T(0), T(0)};
        for (int s = s0 + w; s < s1; s += RC_WAVES)
            for (int t = ta; t < tb; ++t)
                for (int f = fa; f < fb; f += RC_COLS) {
                    const cx<T> v = ws[((size_t)s * A.Nt + t) * A.Nf + f];
                    acc.re += v.re; acc.im += v.im;
                }
        if (A.Fm == 1) { acc.re = wave_sum<T>(acc.re); acc.im = wave_sum<T>(acc.im); }
        if (w > 0) part[w - 1][lane] = acc;
        __syncthreads();
        if (w == 0) {
#pragma unroll
            for (int k = 0; k < RC_WAVES - 1; ++k) { acc.re += part[k][lane].re; acc.im += part[k][lane].im; }
            if (A.Fm == 1) { if (lane == 0) gx[(size_t)c * A.Tm + tm] = acc; }
            else if (fa < A.Nf) gx[((size_t)c * A.Tm + tm) * A.Nf + fa] = acc;
        }
        __syncthreads();                                                        // part is rewritten by the next item
    }
}

static int rc_blocks(size_t nwork, int per_block)
{
    return (int)std::min<size_t>((nwork + per_block - 1) / per_block, 1u << 20);
}

static bool rc_shape_ok(int dtype, int Nout, int Nin, int Nterms, int Nent, int Nt, int Nf, int Tm, int Fm)
{
    if (!real_dtype_ok(dtype) || Nout < 1 || Nin < 1 || Nterms < 1 || Nent < 1 || Nt < 1 || Nf < 1) return false;
    if (Nout > RC_IDX || Nin > RC_IDX || Nent > RC_IDX) return false;
    return (Tm == 1 || Tm == Nt) && (Fm == 1 || Fm == Nf);
}

template <int BWD>
static int rc_row_launch(int dtype, const RcArgs& A, hipStream_t st)
{
    const size_t ntile = ((size_t)A.Nt * A.Nf + RC_COLS - 1) / RC_COLS;
    const int nb = rc_blocks((size_t)(BWD ? A.Nin : A.Nout) * ntile, RC_WAVES);
    return with_real(dtype, [&](auto t) {
        hipLaunchKernelGGL((redcoupling_row_kernel<decltype(t), BWD>), dim3(nb), dim3(RC_WAVES * RC_COLS), 0, st, A);
        return check_launch();
    });
}

} // namespace rime

using namespace rime;

extern "C" size_t rime_redcoupling_workspace(int dtype, int Nseg, int Nt, int Nf)
{
    if (!real_dtype_ok(dtype) || Nseg < 0 || Nt < 1 || Nf < 1) return 0;
    return (size_t)Nseg * Nt * Nf * 2 * real_bytes(dtype);
}

extern "C" int rime_redcoupling_fwd(int dtype, const void* x, const void* dly, const void* data, const int* ent, const int* roff,
                                    int Nout, int Nin, int Nterms, int Nent, int Nt, int Nf, int Tm, int Fm, void* out,
                                    void* stream)
{
    if (!x || !data || !ent || !roff || !out || !rc_shape_ok(dtype, Nout, Nin, Nterms, Nent, Nt, Nf, Tm, Fm)) return RIME_EINVAL;
    RcArgs A{};
    A.x = x; A.dly = dly; A.data = data; A.ent = ent; A.off = roff; A.out = out;
    A.Nout = Nout; A.Nin = Nin; A.Nterms = Nterms; A.Nent = Nent; A.Nt = Nt; A.Nf = Nf; A.Tm = Tm; A.Fm = Fm;
    return rc_row_launch<0>(dtype, A, as_stream(stream));
}

extern "C" int rime_redcoupling_bwd_data(int dtype, const void* x, const void* dly, const void* gout, const int* ent,
                                         const int* coff, const int* cmem, int Nout, int Nin, int Nterms, int Nent, int Nt,
                                         int Nf, int Tm, int Fm, void* gdata, void* stream)
{
    if (!x || !gout || !ent || !coff || !cmem || !gdata || !rc_shape_ok(dtype, Nout, Nin, Nterms, Nent, Nt, Nf, Tm, Fm))
        return RIME_EINVAL;
    RcArgs A{};
    A.x = x; A.dly = dly; A.gout = gout; A.ent = ent; A.off = coff; A.mem = cmem; A.out = gdata;
    A.Nout = Nout; A.Nin = Nin; A.Nterms = Nterms; A.Nent = Nent; A.Nt = Nt; A.Nf = Nf; A.Tm = Tm; A.Fm = Fm;
    return rc_row_launch<1>(dtype, A, as_stream(stream));
}

extern "C" int rime_redcoupling_bwd_coupling(int dtype, const void* x, const void* dly, const void* data, const void* gout,
                                             const int* ent, const int* toff, const int* tmem, const int* segterm,
                                             const int* segstart, const int* tsoff, int Nout, int Nin, int Nterms, int Nent,
                                             int Nmem, int Nseg, int seg, int Nt, int Nf, int Tm, int Fm, void* gx,
                                             void* workspace, size_t workspace_bytes, void* stream)
{
    if (!x || !data || !gout || !ent || !toff || !tsoff || !gx) return RIME_EINVAL;
    if (!rc_shape_ok(dtype, Nout, Nin, Nterms, Nent, Nt, Nf, Tm, Fm)) return RIME_EINVAL;
    if (Nmem < 0 || Nmem > RC_IDX || Nseg < 0 || Nseg > Nmem || seg < 1 || seg > (1 << 20)) return RIME_EINVAL;
    if ((Nmem > 0) != (Nseg > 0) || (Nseg > 0 && (!tmem || !segterm || !segstart))) return RIME_EINVAL;
    const size_t need = rime_redcoupling_workspace(dtype, Nseg, Nt, Nf);
    if (need && (!workspace || workspace_bytes < need)) return RIME_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    RcArgs A{};
    A.x = x; A.dly = dly; A.data = data; A.gout = gout; A.ent = ent; A.off = toff; A.mem = tmem;
    A.segterm = segterm; A.segstart = segstart; A.tsoff = tsoff; A.out = gx; A.ws = workspace;
    A.Nout = Nout; A.Nin = Nin; A.Nterms = Nterms; A.Nent = Nent; A.Nmem = Nmem; A.Nseg = Nseg; A.seg = seg;
    A.Nt = Nt; A.Nf = Nf; A.Tm = Tm; A.Fm = Fm;
    if (Nseg > 0) {
        const size_t ntile = ((size_t)Nt * Nf + RC_COLS - 1) / RC_COLS;
        const int nb = rc_blocks((size_t)Nseg * ntile, RC_WAVES);
        const int rc = with_real(dtype, [&](auto t) {
            hipLaunchKernelGGL((redcoupling_seg_kernel<decltype(t)>), dim3(nb), dim3(RC_WAVES * RC_COLS), 0, st, A);
            return check_launch();
        });
        if (rc != RIME_OK) return rc;
    }
    const int nft = Fm == 1 ? 1 : (Nf + RC_COLS - 1) / RC_COLS;
    const int nb = rc_blocks((size_t)Nterms * Tm * nft, 1);
    return with_real(dtype, [&](auto t) {
        hipLaunchKernelGGL((redcoupling_combine_kernel<decltype(t)>), dim3(nb), dim3(RC_WAVES * RC_COLS), 0, st, A);
        return check_launch();
    });
}
