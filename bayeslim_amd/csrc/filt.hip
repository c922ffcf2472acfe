// filt.hip -- grouped matrix filter along the last axis of a complex tensor (gfx950):
//     acc_i       = sum_k W[f(l)][i, k] x[l, ic[k]]                 i < M, k < K
//     y[l, oc[i]] = s acc_i + base[i] x[l, oc[i]]
// for every line l (Nx contiguous complex samples) with filter index f(l): the reference's MatFilter / GPFilter forward (W = G)
// and its adjoint (W = G^H), and WedgeFilter -- a Python loop of gather / complex einsum / scatter per baseline group in the
// reference (filt.py:382-397) -- as ONE launch over a host-built tile list.
//
// One real GEMM body.  D[(line, re|im)][i] = sum_kr X[(line, re|im)][kr] Wt[kr][i] on a tile of 64 lines (128 real rows) x 128
// output rows i.  A real W reads re and im of x as two rows of X (kr = k).  A complex W rides the same product with
//     Wt[2k][i] = Re W[i,k],  Wt[2k+1][i] = -Im W[i,k]      (the host packs view_as_real(conj W), transposed: kr-major)
//     X[(l,re)][2k] = xr,  X[(l,re)][2k+1] = xi,  X[(l,im)][2k] = xi,  X[(l,im)][2k+1] = -xr
// so only the staging of x differs.  The lines are the MFMA rows on purpose: the C/D map of the 32 x 32 instruction keeps rows
// 2p, 2p+1 in adjacent registers of ONE lane and the column on the lane, so a lane stores (re, im) of a line as one 8-byte
// element and 32 lanes cover 32 consecutive output samples: coalesced, no LDS transpose.
//   float : v_mfma_f32_32x32x2_f32, exact f32 (a k-ordered fmaf chain); 4 waves, each 2 x 2 fragments of 32 x 32.
//   double: plain vector-ALU FMAs in the same tile (the parity precision), each lane 4 lines x 8 output rows.
// The host groups the lines by filter and lists tiles of up to 64 line indices (padded with -1 at the end); tiles of filter -1
// copy their lines (legal only if Nx == Ny).  Exactly one block writes each output element, sums run in ascending k: no
// atomics, bit-reproducible.  Columns of y outside oc are never written.
#include <hip/hip_runtime.h>
#include "rime_common.h"

namespace rime {

constexpr int FILT_TL = 64;               // lines of a tile
constexpr int FILT_TR = 2 * FILT_TL;      // real rows of a tile: (line, re | im)
constexpr int FILT_TC = 128;              // output rows i of a tile
constexpr int FILT_TILE_INTS = 1 + FILT_TL;   // (filter, 64 line indices)
constexpr int FILT_LDX = FILT_TR + 2;     // row stride of the x tile: the transposed 8-byte stores of a chunk spread over the banks
constexpr int FILT_LDW = FILT_TC + 32;    // row stride of the W tile: the two k rows an MFMA reads sit in different bank halves

template <typename T> struct FiltT;
template <> struct FiltT<float>  { using v2 = float2;  static constexpr int KC = 32; };
template <> struct FiltT<double> { using v2 = double2; static constexpr int KC = 16; };

typedef float filt_f32x16 __attribute__((ext_vector_type(16)));

// CW: complex W.  KR = K (CW ? 2 : 1) real contraction length; Wt [Nfilt][KR][M]; x [Nlines][Nx] complex; y [Nlines][Ny] complex.
template <typename T, bool CW>
__global__ void __launch_bounds__(256)
filt_kernel(const T* __restrict__ x, const T* __restrict__ Wt, const int* __restrict__ ic, const int* __restrict__ oc,
            const T* __restrict__ base, const int* __restrict__ tiles, int NRT, int Nfilt, int M, int K, int Nx, int Ny,
            long long Nlines, T s, T* __restrict__ y)
{
    using V2 = typename FiltT<T>::v2;
    constexpr int KC = FiltT<T>::KC;              // real k rows per chunk (even)
    constexpr int KCC = CW ? KC / 2 : KC;         // complex samples of x per chunk
    __shared__ __attribute__((aligned(16))) T x_s[KC][FILT_LDX];
    __shared__ __attribute__((aligned(16))) T w_s[KC][FILT_LDW];
    __shared__ int line_s[FILT_TL];

    const int tile = blockIdx.x / NRT, rt = blockIdx.x % NRT;
    const int* tl = tiles + (size_t)tile * FILT_TILE_INTS;
    const int f = tl[0];
    const int tid = threadIdx.x;
    if (tid < FILT_TL) {
        const int l = tl[1 + tid];
        line_s[tid] = (l >= 0 && (long long)l < Nlines) ? l : -1;
    }
    __syncthreads();

    if (f < 0) {                                   // pass-through lines: copied by the first row tile only
        if (rt != 0 || Nx != Ny) return;
        for (int ln = 0; ln < FILT_TL; ln++) {
            const int l = line_s[ln];
            if (l < 0) continue;
            const V2* src = reinterpret_cast<const V2*>(x) + (size_t)l * Nx;
            V2* dst = reinterpret_cast<V2*>(y) + (size_t)l * Ny;
            for (int c = tid; c < Nx; c += 256) dst[c] = src[c];
        }
        return;
    }
    if (f >= Nfilt) return;                        // malformed table: write nothing

    const int i0 = rt * FILT_TC;
    const int KR = CW ? 2 * K : K;
    const T* Wf = Wt + (size_t)f * KR * M;

    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;       // float: the wave's 64 x 64 quadrant
    const int l31 = lane & 31, h = lane >> 5;
    const int tx = tid & 15, ty = tid >> 4;        // double: output rows tx + 16 u, lines 4 ty + v

    filt_f32x16 acc[2][2];
    T accd[4][8][2];
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int u = 0; u < 2; u++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[t][u][e] = 0.f;
    } else {
#pragma unroll
        for (int v = 0; v < 4; v++)
#pragma unroll
            for (int u = 0; u < 8; u++) accd[v][u][0] = accd[v][u][1] = T(0);
    }

    for (int k0 = 0; k0 < KR; k0 += KC) {
        // x tile: lanes along the samples of a line (contiguous when ic is the identity)
        const int c0 = CW ? k0 / 2 : k0;
        for (int e = tid; e < KCC * FILT_TL; e += 256) {
            const int cc = e % KCC, ln = e / KCC;
            const int c = c0 + cc, l = line_s[ln];
            V2 v; v.x = T(0); v.y = T(0);
            if (l >= 0 && c < K) {
                const int col = ic[c];
                if (col >= 0 && col < Nx) v = *(reinterpret_cast<const V2*>(x) + (size_t)l * Nx + col);
            }
            if constexpr (CW) {
                V2 r; r.x = v.y; r.y = -v.x;
                *reinterpret_cast<V2*>(&x_s[2 * cc][2 * ln]) = v;
                *reinterpret_cast<V2*>(&x_s[2 * cc + 1][2 * ln]) = r;
            } else {
                *reinterpret_cast<V2*>(&x_s[cc][2 * ln]) = v;
            }
        }
        // W tile: Wt[kr][i], lanes along i
        for (int e = tid; e < KC * FILT_TC; e += 256) {
            const int ii = e % FILT_TC, kk = e / FILT_TC;
            const int kr = k0 + kk, i = i0 + ii;
            w_s[kk][ii] = (kr < KR && i < M) ? Wf[(size_t)kr * M + i] : T(0);
        }
        __syncthreads();
        if constexpr (sizeof(T) == 4) {
#pragma unroll 4
            for (int kk = 0; kk < KC; kk += 2) {
                float a[2], b[2];
#pragma unroll
                for (int t = 0; t < 2; t++) a[t] = x_s[kk + h][wr * 64 + t * 32 + l31];
#pragma unroll
                for (int u = 0; u < 2; u++) b[u] = w_s[kk + h][wc * 64 + u * 32 + l31];
#pragma unroll
                for (int t = 0; t < 2; t++)
#pragma unroll
                    for (int u = 0; u < 2; u++)
                        acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[u], acc[t][u], 0, 0, 0);
            }
        } else {
#pragma unroll 2
            for (int kk = 0; kk < KC; kk++) {
                T w[8];
#pragma unroll
                for (int u = 0; u < 8; u++) w[u] = w_s[kk][tx + 16 * u];
#pragma unroll
                for (int v = 0; v < 4; v++) {
                    const V2 xv = *reinterpret_cast<const V2*>(&x_s[kk][2 * (4 * ty + v)]);
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        accd[v][u][0] = tfma<T>(xv.x, w[u], accd[v][u][0]);
                        accd[v][u][1] = tfma<T>(xv.y, w[u], accd[v][u][1]);
                    }
                }
            }
        }
        __syncthreads();
    }

    // y[l, oc[i]] = s acc + base[i] x[l, oc[i]]
    auto store = [&](int ln, int i, T re, T im) {
        const int l = line_s[ln];
        if (l < 0 || i >= M) return;
        const int col = oc[i];
        if (col < 0 || col >= Ny) return;
        V2 out; out.x = s * re; out.y = s * im;
        const T bs = base[i];
        if (bs != T(0) && col < Nx) {
            const V2 xv = *(reinterpret_cast<const V2*>(x) + (size_t)l * Nx + col);
            out.x = tfma<T>(bs, xv.x, out.x);
            out.y = tfma<T>(bs, xv.y, out.y);
        }
        *(reinterpret_cast<V2*>(y) + (size_t)l * Ny + col) = out;
    };
    if constexpr (sizeof(T) == 4) {
        RIME_MFMA_SETTLE();
        // C/D map: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5): registers 2p, 2p + 1 are re, im of line
        // (p & 1) + 4 (p >> 1) + 2 (lane >> 5) of the fragment's 16 lines
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int i = i0 + wc * 64 + u * 32 + l31;
#pragma unroll
                for (int p = 0; p < 8; p++) {
                    const int ln = wr * 32 + t * 16 + (p & 1) + 4 * (p >> 1) + 2 * h;
                    store(ln, i, acc[t][u][2 * p], acc[t][u][2 * p + 1]);
                }
            }
    } else {
#pragma unroll
        for (int v = 0; v < 4; v++)
#pragma unroll
            for (int u = 0; u < 8; u++) store(4 * ty + v, i0 + tx + 16 * u, accd[v][u][0], accd[v][u][1]);
    }
}

} // namespace rime

using namespace rime;

extern "C" int rime_filt_apply(int dtype, int wcplx, const void* x, const void* Wt, const int* ic, const int* oc, const void* base,
                               const int* tiles, int Ntile, int Npass, int Nfilt, int M, int K, int Nx, int Ny, long long Nlines,
                               double s, void* y, void* stream)
{
    if (!real_dtype_ok(dtype)) return RIME_EINVAL;
    if (wcplx != 0 && wcplx != 1) return RIME_EINVAL;
    if (M <= 0 || K <= 0 || Nx <= 0 || Ny <= 0 || Nfilt <= 0 || Nlines < 0 || Nlines > 0x7fffffffLL) return RIME_EINVAL;
    if (K > 0x3fffffff || Ntile < 0 || Npass < 0 || Npass > Ntile) return RIME_EINVAL;
    if (s != 1.0 && s != -1.0) return RIME_EINVAL;
    if (!ic || !oc || !base) return RIME_EINVAL;
    if (Npass > 0 && Nx != Ny) return RIME_EINVAL;            // a copied line keeps its length
    if (Ntile > 0 && !tiles) return RIME_EINVAL;
    const int NRT = (M + FILT_TC - 1) / FILT_TC;
    if ((long long)Ntile * (long long)NRT > 0x7fffffffLL) return RIME_EINVAL;
    if (Ntile == 0 || Nlines == 0) return RIME_OK;            // nothing to write
    if (!x || !Wt || !y) return RIME_EINVAL;
    return with_real(dtype, [&](auto t) {
        using T = decltype(t);
        with_bool(wcplx != 0, [&](auto cw) {
            hipLaunchKernelGGL((filt_kernel<T, cw.value>), dim3((unsigned)(Ntile * NRT)), dim3(256), 0, as_stream(stream),
                               (const T*)x, (const T*)Wt, ic, oc, (const T*)base, tiles, NRT, Nfilt, M, K, Nx, Ny, Nlines, (T)s,
                               (T*)y);
        });
        return check_launch();
    });
}
