// coupling.hip -- antenna mutual coupling W = E V E^H of calibration.VisCoupling (calibration.py:1258-1586), forward and
// backward, on ONE batched complex product body
//     C[s] = [addend[s]] + sum_{phase} op(A_phase[s]) . op(B_phase[s])      s = (t, f),  N x N complex,  op in {plain, ^H}
// The batch axes (t, f) are the contiguous ones of every tensor involved, so nothing is transposed through HBM: a block owns a
// run of CP_FR consecutive channels of one time and a CP_TILE x CP_TILE tile of the matrix, lanes run along f first (every
// global access is a run of CP_FR complex numbers), and the k axis is re-tiled through LDS in slabs of CP_TK.
// The fusion sits in how operands are READ and how the result is WRITTEN:
//   dense operand   (N, N, Tm, Fm), Tm in {1, Nt}, Fm in {1, Nf}; optionally times a second dense (N, N, 1, Nf) (the delay
//                   phasor) and plus the identity: E = I + X o D is built on the fly from the response output
//   table operand   element (a, b) read from rows (Nrows, Nt, Nf) through an (N, N) int32 table: row | conjugate bit, or -1
//                   for zero -- the visibility matrix V from the data, and the gradient matrix G from gout
//   dense result    (N, N, Nt, Nf), optionally plus a dense addend and times conj of a dense (N, N, 1, Nf)
//   picked result   only the entries whose table entry is a row are written, to (Nrows, Nt, Nf); with two phases an entry whose
//                   table word carries CP_BIT keeps the second phase only -- the fold gdata[bl(a,b)] = gV[a,b] + conj(gV[b,a])
//                   evaluated as (P^H E)[a,b] + (E^H P)[a,b], the single term for an auto-correlation
// Every output element is summed by exactly one thread of one block: phase 0 then phase 1, k ascending within each; no
// atomics, the same bits from run to run.  Vector-ALU FMAs in the precision of the data; no matrix cores.
// Every index followed comes from a table the caller has range-checked; the kernel also treats a row outside [0, Nrows) as
// null and clamps on the N, Nt, Nf edges (N and Nf need not be multiples of anything).
#include <hip/hip_runtime.h>
#include "rime_common.h"
#include "cplx.h"

namespace rime {

constexpr int CP_TILE = 32;          // matrix tile of a block (rows of op(A), columns of op(B))
constexpr int CP_TT = 4;             // a thread owns CP_TT x CP_TT entries of the tile, strided by CP_TILE / CP_TT, at one f
constexpr int CP_TS = CP_TILE / CP_TT;
constexpr int CP_FR = 8;             // consecutive channels of a block
constexpr int CP_TK = 8;             // k slab held in LDS
constexpr int CP_THREADS = CP_TS * CP_TS * CP_FR;                  // 512
constexpr int CP_ROW = 0x3fffffff, CP_BIT = 0x40000000;            // table word: row, conjugate (operand) / single term (result)
enum { CP_DENSE = 0, CP_TABLE = 1 };

struct CpOperand {
    const void* p;                   // dense: (N, N, Tm, Fm) complex;  table: (Nrows, Nt, Nf) complex
    const void* mul;                 // dense: optional (N, N, Nf) complex factor
    const int* tab;                  // table: (N, N)
    int mode, op, addI, Tm, Fm, Nrows;
};

struct CpResult {
    void* p;                         // dense: (N, N, Nt, Nf);  picked: (Nrows, Nt, Nf)
    const void* cmul;                // dense: optional (N, N, Nf), the result is multiplied by its conjugate
    const int* tab;                  // picked: (N, N)
    int mode, Nrows;
};

struct CpArgs {
    CpOperand A0, B0, A1, B1, add;   // add: dense addend of a dense result (p null: none)
    CpResult C;
    int nphase, N, Nt, Nf;
};

// element (r, c) of op(O) at batch (t, f); zero outside the matrix and beyond the last channel
template <typename T>
__device__ __forceinline__ cx<T> cp_fetch(const CpOperand& O, int r, int c, int t, int f, int N, int Nt, int Nf)
{
    cx<T> v = {T(0), T(0)};
    if (r >= N || c >= N || f >= Nf) return v;
    if (O.op) { const int s = r; r = c; c = s; }
    const size_t rc = (size_t)r * N + c;
    if (O.mode == CP_TABLE) {
        const int e = O.tab[rc];
        const int row = e & CP_ROW;
        if (e < 0 || row >= O.Nrows) return v;
        v = reinterpret_cast<const cx<T>*>(O.p)[((size_t)row * Nt + t) * Nf + f];
        if (e & CP_BIT) v.im = -v.im;
    } else {
        const int tt = O.Tm == 1 ? 0 : t, ff = O.Fm == 1 ? 0 : f;
        v = reinterpret_cast<const cx<T>*>(O.p)[(rc * O.Tm + tt) * O.Fm + ff];
        if (O.mul) {
            const cx<T> m = reinterpret_cast<const cx<T>*>(O.mul)[rc * Nf + f];
            v = cmul(v, m);
        }
        if (O.addI && r == c) v.re += T(1);
    }
    if (O.op) v.im = -v.im;
    return v;
}

// acc += op(A) . op(B) over all k in ascending order, for the block's tile (i0, j0) and channels f0 .. f0 + CP_FR - 1 of time t
template <typename T>
__device__ __forceinline__ void cp_accumulate(const CpOperand& A, const CpOperand& B, cx<T> (&acc)[CP_TT][CP_TT],
                                              cx<T> (&As)[CP_TK][CP_TILE][CP_FR], cx<T> (&Bs)[CP_TK][CP_TILE][CP_FR],
                                              int i0, int j0, int t, int f0, int N, int Nt, int Nf)
{
    const int tid = threadIdx.x;
    const int lf = tid % CP_FR, tj = (tid / CP_FR) % CP_TS, ti = tid / (CP_FR * CP_TS);
    for (int k0 = 0; k0 < N; k0 += CP_TK) {                    // block-uniform trip count
        for (int e = tid; e < CP_TK * CP_TILE * CP_FR; e += CP_THREADS) {
            const int ef = e % CP_FR, m = (e / CP_FR) % CP_TILE, kk = e / (CP_FR * CP_TILE);
            As[kk][m][ef] = cp_fetch<T>(A, i0 + m, k0 + kk, t, f0 + ef, N, Nt, Nf);
            Bs[kk][m][ef] = cp_fetch<T>(B, k0 + kk, j0 + m, t, f0 + ef, N, Nt, Nf);
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < CP_TK; ++kk) {
            cx<T> a[CP_TT], b[CP_TT];
#pragma unroll
            for (int x = 0; x < CP_TT; ++x) { a[x] = As[kk][ti + CP_TS * x][lf]; b[x] = Bs[kk][tj + CP_TS * x][lf]; }
#pragma unroll
            for (int x = 0; x < CP_TT; ++x)
#pragma unroll
                for (int y = 0; y < CP_TT; ++y) cfma(acc[x][y], a[x], b[y]);
        }
        __syncthreads();                                       // the slabs are rewritten by the next step
    }
}

template <typename T>
__global__ void __launch_bounds__(CP_THREADS)
coupling_product_kernel(CpArgs P)
{
    __shared__ cx<T> As[CP_TK][CP_TILE][CP_FR], Bs[CP_TK][CP_TILE][CP_FR];
    const int N = P.N, Nt = P.Nt, Nf = P.Nf;
    const int nfr = (Nf + CP_FR - 1) / CP_FR;
    const int t = (int)(blockIdx.x / nfr), f0 = (int)(blockIdx.x % nfr) * CP_FR;
    const int i0 = blockIdx.y * CP_TILE, j0 = blockIdx.z * CP_TILE;
    const int tid = threadIdx.x;
    const int lf = tid % CP_FR, tj = (tid / CP_FR) % CP_TS, ti = tid / (CP_FR * CP_TS);
    const int f = f0 + lf;
    if (t >= Nt) return;                                       // block-uniform; the grid is exact, this is the clamp

    cx<T> acc[CP_TT][CP_TT];
#pragma unroll
    for (int x = 0; x < CP_TT; ++x)
#pragma unroll
        for (int y = 0; y < CP_TT; ++y) acc[x][y] = {T(0), T(0)};

    cp_accumulate<T>(P.A0, P.B0, acc, As, Bs, i0, j0, t, f0, N, Nt, Nf);
    if (P.nphase == 2) {
        if (P.C.mode == CP_TABLE) {                            // the fold: an entry with CP_BIT keeps the second phase only
#pragma unroll
            for (int x = 0; x < CP_TT; ++x)
#pragma unroll
                for (int y = 0; y < CP_TT; ++y) {
                    const int i = i0 + ti + CP_TS * x, j = j0 + tj + CP_TS * y;
                    if (i < N && j < N && P.C.tab[(size_t)i * N + j] >= 0 && (P.C.tab[(size_t)i * N + j] & CP_BIT))
                        acc[x][y] = {T(0), T(0)};
                }
        }
        cp_accumulate<T>(P.A1, P.B1, acc, As, Bs, i0, j0, t, f0, N, Nt, Nf);
    }

    if (f >= Nf) return;
#pragma unroll
    for (int x = 0; x < CP_TT; ++x)
#pragma unroll
        for (int y = 0; y < CP_TT; ++y) {
            const int i = i0 + ti + CP_TS * x, j = j0 + tj + CP_TS * y;
            if (i >= N || j >= N) continue;
            const size_t ij = (size_t)i * N + j;
            cx<T> v = acc[x][y];
            if (P.C.mode == CP_TABLE) {
                const int e = P.C.tab[ij];
                const int row = e & CP_ROW;
                if (e < 0 || row >= P.C.Nrows) continue;
                reinterpret_cast<cx<T>*>(P.C.p)[((size_t)row * Nt + t) * Nf + f] = v;
            } else {
                if (P.add.p) {
                    const cx<T> s = cp_fetch<T>(P.add, i, j, t, f, N, Nt, Nf);
                    v.re += s.re; v.im += s.im;                // `v += s` swaps the operands of the packed add
                }
                if (P.C.cmul) {
                    const cx<T> m = reinterpret_cast<const cx<T>*>(P.C.cmul)[ij * Nf + f];
                    v = cmulc(v, m);
                }
                reinterpret_cast<cx<T>*>(P.C.p)[(ij * Nt + t) * Nf + f] = v;
            }
        }
}

// out[ab, tm, fm] = sum_t sum_f in[ab, t, f] over the axes that Tm = 1 / Fm = 1 broadcast, t outer, f inner, ascending, by one
// thread per output element
template <typename T>
__global__ void __launch_bounds__(256)
coupling_reduce_kernel(const void* in_, void* out_, size_t NN, int Nt, int Nf, int Tm, int Fm)
{
    const cx<T>* in = reinterpret_cast<const cx<T>*>(in_);
    cx<T>* out = reinterpret_cast<cx<T>*>(out_);
    const size_t total = NN * Tm * Fm;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const int fm = (int)(o % Fm), tm = (int)((o / Fm) % Tm);
        const size_t ab = o / ((size_t)Fm * Tm);
        const int ta = Tm == 1 ? 0 : tm, tb = Tm == 1 ? Nt : tm + 1;
        const int fa = Fm == 1 ? 0 : fm, fb = Fm == 1 ? Nf : fm + 1;
        cx<T> s = {T(0), T(0)};
        for (int t = ta; t < tb; ++t)
            for (int f = fa; f < fb; ++f) {
                const cx<T> v = in[(ab * Nt + t) * Nf + f];
                s.re += v.re; s.im += v.im;                    // `s += v` moves the zeroing of s in the double kernel
            }
        out[o] = s;
    }
}

static CpOperand cp_dense(const void* p, const void* mul, int Tm, int Fm, int addI, int op)
{
    CpOperand O{};
    O.p = p; O.mul = mul; O.mode = CP_DENSE; O.op = op; O.addI = addI; O.Tm = Tm; O.Fm = Fm;
    return O;
}

static CpOperand cp_table(const void* rows, const int* tab, int Nrows, int op)
{
    CpOperand O{};
    O.p = rows; O.tab = tab; O.mode = CP_TABLE; O.op = op; O.Nrows = Nrows;
    return O;
}

static CpOperand cp_h(CpOperand O) { O.op = !O.op; return O; }

static CpResult cp_dense_result(void* p, const void* cmul)
{
    CpResult C{};
    C.p = p; C.cmul = cmul; C.mode = CP_DENSE;
    return C;
}

static CpResult cp_picked_result(void* rows, const int* tab, int Nrows)
{
    CpResult C{};
    C.p = rows; C.tab = tab; C.mode = CP_TABLE; C.Nrows = Nrows;
    return C;
}

struct CpShape { int dtype, N, Nt, Nf; hipStream_t st; };

static int cp_launch(const CpShape& S, const CpResult& C, const CpOperand& A0, const CpOperand& B0,
                     const CpOperand* A1 = nullptr, const CpOperand* B1 = nullptr, const CpOperand* add = nullptr)
{
    CpArgs P{};
    P.A0 = A0; P.B0 = B0; P.C = C; P.nphase = 1; P.N = S.N; P.Nt = S.Nt; P.Nf = S.Nf;
    if (A1 && B1) { P.A1 = *A1; P.B1 = *B1; P.nphase = 2; }
    if (add) P.add = *add;
    const unsigned nfr = (S.Nf + CP_FR - 1) / CP_FR, nt = (S.N + CP_TILE - 1) / CP_TILE;
    const dim3 grid(nfr * (unsigned)S.Nt, nt, nt);
    return with_real(S.dtype, [&](auto t) {
        hipLaunchKernelGGL((coupling_product_kernel<decltype(t)>), grid, dim3(CP_THREADS), 0, S.st, P);
        return check_launch();
    });
}

static int cp_reduce(const CpShape& S, const void* in, void* out, int Tm, int Fm)
{
    const size_t NN = (size_t)S.N * S.N, total = NN * Tm * Fm;
    const int nb = (int)std::min<size_t>((total + 255) / 256, 1u << 20);
    return with_real(S.dtype, [&](auto t) {
        hipLaunchKernelGGL((coupling_reduce_kernel<decltype(t)>), dim3(nb), dim3(256), 0, S.st, in, out, NN, S.Nt, S.Nf, Tm, Fm);
        return check_launch();
    });
}

static bool cp_shape_ok(int dtype, int N, int Nt, int Nf, int Tm, int Fm)
{
    if (!real_dtype_ok(dtype) || N < 1 || Nt < 1 || Nf < 1) return false;
    if ((Tm != 1 && Tm != Nt) || (Fm != 1 && Fm != Nf)) return false;
    return (size_t)Nt * ((Nf + CP_FR - 1) / CP_FR) < (1ull << 31) && (N + CP_TILE - 1) / CP_TILE <= 65535;
}

static bool cp_prod_ok(int prod) { return prod == RIME_COUPLING_BOTH || prod == RIME_COUPLING_LEFT || prod == RIME_COUPLING_RIGHT; }

// complex elements of the (N, N, Nt, Nf) intermediates a stage keeps in the workspace
static size_t cp_workspace_mats(int Nt, int Nf, int Tm, int Fm, int prod, int stage)
{
    const bool bcast = Tm != Nt || Fm != Nf;
    if (stage == RIME_COUPLING_FWD) return prod == RIME_COUPLING_BOTH ? 1 : 0;
    if (stage == RIME_COUPLING_BWD) return (prod == RIME_COUPLING_BOTH ? 2 : 0) + (bcast ? 1 : 0);
    return bcast ? 1 : 0;                                      // RIME_COUPLING_EXPAND_BWD
}

} // namespace rime

using namespace rime;

extern "C" size_t rime_coupling_workspace(int dtype, int N, int Nt, int Nf, int Tm, int Fm, int prod, int stage)
{
    if (!cp_shape_ok(dtype, N, Nt, Nf, Tm, Fm) || !cp_prod_ok(prod)) return 0;
    if (stage != RIME_COUPLING_FWD && stage != RIME_COUPLING_BWD && stage != RIME_COUPLING_EXPAND_BWD) return 0;
    return cp_workspace_mats(Nt, Nf, Tm, Fm, prod, stage) * (size_t)N * N * Nt * Nf * 2 * real_bytes(dtype);
}

extern "C" int rime_coupling_fwd(int dtype, const void* x, const void* dly, const void* data, const int* tab, const int* otab,
                                 int N, int Nbl, int Nout, int Nt, int Nf, int Tm, int Fm, int addI, int prod, void* out,
                                 void* workspace, size_t workspace_bytes, void* stream)
{
    if (!x || !data || !tab || !otab || !out) return RIME_EINVAL;
    if (!cp_shape_ok(dtype, N, Nt, Nf, Tm, Fm) || !cp_prod_ok(prod) || Nbl < 1 || Nout < 1 || Nbl > CP_ROW || Nout > CP_ROW)
        return RIME_EINVAL;
    if (addI != 0 && addI != 1) return RIME_EINVAL;
    const size_t need = rime_coupling_workspace(dtype, N, Nt, Nf, Tm, Fm, prod, RIME_COUPLING_FWD);
    if (need && (!workspace || workspace_bytes < need)) return RIME_EWORKSPACE;
    const CpShape S{dtype, N, Nt, Nf, as_stream(stream)};
    const CpOperand E = cp_dense(x, dly, Tm, Fm, addI, 0), EH = cp_h(E), V = cp_table(data, tab, Nbl, 0);
    const CpResult W = cp_picked_result(out, otab, Nout);
    if (prod == RIME_COUPLING_LEFT) return cp_launch(S, W, E, V);
    if (prod == RIME_COUPLING_RIGHT) return cp_launch(S, W, V, EH);
    const int rc = cp_launch(S, cp_dense_result(workspace, nullptr), E, V);             // T = E V
    if (rc != RIME_OK) return rc;
    return cp_launch(S, W, cp_dense(workspace, nullptr, Nt, Nf, 0, 0), EH);             // W = T E^H, picked
}

extern "C" int rime_coupling_bwd(int dtype, const void* x, const void* dly, const void* data, const void* gout, const int* tab,
                                 const int* otab, const int* ftab, int N, int Nbl, int Nout, int Nt, int Nf, int Tm, int Fm,
                                 int addI, int prod, void* gdata, void* gx, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!x || !data || !gout || !tab || !otab || (!gdata && !gx) || (gdata && !ftab)) return RIME_EINVAL;
    if (!cp_shape_ok(dtype, N, Nt, Nf, Tm, Fm) || !cp_prod_ok(prod) || Nbl < 1 || Nout < 1 || Nbl > CP_ROW || Nout > CP_ROW)
        return RIME_EINVAL;
    if (addI != 0 && addI != 1) return RIME_EINVAL;
    const size_t need = rime_coupling_workspace(dtype, N, Nt, Nf, Tm, Fm, prod, RIME_COUPLING_BWD);
    if (need && (!workspace || workspace_bytes < need)) return RIME_EWORKSPACE;
    const CpShape S{dtype, N, Nt, Nf, as_stream(stream)};
    const size_t mat = (size_t)N * N * Nt * Nf * 2 * real_bytes(dtype);
    const bool both = prod == RIME_COUPLING_BOTH, bcast = Tm != Nt || Fm != Nf;
    char* ws = static_cast<char*>(workspace);
    void* Tbuf = both ? ws : nullptr;
    void* Pbuf = both ? ws + mat : nullptr;
    void* gEbuf = bcast ? ws + (both ? 2 * mat : 0) : gx;      // gE o conj(dly), (N, N, Nt, Nf), before the broadcast sums
    const CpOperand E = cp_dense(x, dly, Tm, Fm, addI, 0), EH = cp_h(E);
    const CpOperand V = cp_table(data, tab, Nbl, 0), VH = cp_h(V);
    const CpOperand G = cp_table(gout, otab, Nout, 0), GH = cp_h(G);
    int rc = RIME_OK;
    if (both) {
        rc = cp_launch(S, cp_dense_result(Pbuf, nullptr), G, E);                        // P = G E
        if (rc != RIME_OK) return rc;
    }
    const CpOperand Pd = cp_dense(Pbuf, nullptr, Nt, Nf, 0, 0), PH = cp_h(Pd);
    if (gx) {
        const CpResult R = cp_dense_result(gEbuf, dly);
        if (both) {
            rc = cp_launch(S, cp_dense_result(Tbuf, nullptr), E, V);                    // T = E V, recomputed
            if (rc != RIME_OK) return rc;
            const CpOperand Td = cp_dense(Tbuf, nullptr, Nt, Nf, 0, 0);
            rc = cp_launch(S, R, Pd, VH, &GH, &Td);                                     // gE = P V^H + G^H T
        } else if (prod == RIME_COUPLING_LEFT) {
            rc = cp_launch(S, R, G, VH);                                                // gE = G V^H
        } else {
            rc = cp_launch(S, R, GH, V);                                                // gE = G^H V
        }
        if (rc != RIME_OK) return rc;
        if (bcast) {
            rc = cp_reduce(S, gEbuf, gx, Tm, Fm);
            if (rc != RIME_OK) return rc;
        }
    }
    if (gdata) {                                                                        // gV = E^H G E, folded
        const CpResult R = cp_picked_result(gdata, ftab, Nbl);
        if (both) rc = cp_launch(S, R, PH, E, &EH, &Pd);                                // (P^H E) + (E^H P)
        else if (prod == RIME_COUPLING_LEFT) rc = cp_launch(S, R, GH, E, &EH, &G);      // gV = E^H G
        else rc = cp_launch(S, R, EH, GH, &G, &E);                                      // gV = G E
    }
    return rc;
}

extern "C" int rime_coupling_expand(int dtype, const void* x, const void* dly, int N, int Nt, int Nf, int Tm, int Fm, int addI,
                                    void* e, void* stream)
{
    if (!x || !e || !cp_shape_ok(dtype, N, Nt, Nf, Tm, Fm) || (addI != 0 && addI != 1)) return RIME_EINVAL;
    const CpShape S{dtype, N, Nt, Nf, as_stream(stream)};
    const CpOperand Xd = cp_dense(x, dly, Tm, Fm, 0, 0), add = cp_dense(x, dly, Tm, Fm, addI, 0);
    return cp_launch(S, cp_dense_result(e, nullptr), Xd, Xd, nullptr, nullptr, &add);   // E = [I] + Xd + Xd Xd
}

extern "C" int rime_coupling_expand_bwd(int dtype, const void* x, const void* dly, const void* ge, int N, int Nt, int Nf, int Tm,
                                        int Fm, void* gx, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!x || !ge || !gx || !cp_shape_ok(dtype, N, Nt, Nf, Tm, Fm)) return RIME_EINVAL;
    const size_t need = rime_coupling_workspace(dtype, N, Nt, Nf, Tm, Fm, RIME_COUPLING_BOTH, RIME_COUPLING_EXPAND_BWD);
    if (need && (!workspace || workspace_bytes < need)) return RIME_EWORKSPACE;
    const CpShape S{dtype, N, Nt, Nf, as_stream(stream)};
    const bool bcast = Tm != Nt || Fm != Nf;
    void* buf = bcast ? workspace : gx;
    const CpOperand XH = cp_dense(x, dly, Tm, Fm, 0, 1), gE = cp_dense(ge, nullptr, Nt, Nf, 0, 0);
    int rc = cp_launch(S, cp_dense_result(buf, dly), gE, XH, &XH, &gE, &gE);            // gXd = gE + gE Xd^H + Xd^H gE
    if (rc != RIME_OK || !bcast) return rc;
    return cp_reduce(S, buf, gx, Tm, Fm);
}
