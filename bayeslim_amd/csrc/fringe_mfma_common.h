// fringe_mfma_common.h -- what the matrix-core fringe sources (fringe_mfma.hip, fringe_xpair.hip) share: the small device
// helpers of their kernels and the host layer between the C ABI and hipLaunchKernelGGL.  No kernels, not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdlib>
#include <type_traits>
#include "rime_common.h"

namespace rime {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int MF_SPLIT_PIX = 16384;           // pixels per block (bounds the f32 MFMA accumulation chain)
constexpr int MF_KP = 32;                       // pixels per panel (one barrier per panel); 16 per MFMA

// ---- device helpers ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pack_rtz(float a, float b)
{
    auto h = __builtin_amdgcn_cvt_pkrtz(a, b);
    return __builtin_bit_cast(uint32_t, h);
}

// split (a, b) into f16 hi and lo pairs: x = hi + lo + O(2^-21 |x|)
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo)
{
    auto h = __builtin_amdgcn_cvt_pkrtz(a, b);
    hi = __builtin_bit_cast(uint32_t, h);
    const float ra = a - (float)h[0];
    const float rb = b - (float)h[1];
    lo = pack_rtz(ra, rb);
}

// the same split for values that are not products: the residual a - hi is one mixed-precision FMA
// (a * 1.0 - hi, the f16 half read in place) instead of v_cvt_f32_f16 + v_sub_f32 -- the compiler
// only forms v_fma_mix when there is a multiply to fuse
__device__ __forceinline__ void split2_plain(float a, float b, uint32_t& hi, uint32_t& lo)
{
    auto h = __builtin_amdgcn_cvt_pkrtz(a, b);
    hi = __builtin_bit_cast(uint32_t, h);
    float ra, rb;
    asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(ra) : "v"(a), "v"(hi));
    asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(rb) : "v"(b), "v"(hi));
    lo = pack_rtz(ra, rb);
}

// Keeps a float a scalar computation of its own: the compiler's SLP pass pairs independent f32 adds / multiplies / FMAs into
// v_pk_*_f32.  Round 5: in the conjugate-pair backward -- the first kernel here whose blocks SHARE a CU, so that one block stages its
// G planes while another block's waves stream MFMAs on the same SIMDs -- the build whose staging arithmetic the compiler had
// vectorised (65 v_pk_add_f32: sums of two freshly loaded gradients) produced wrong planes in a fraction of the blocks that
// were dispatched late, different from run to run; alone on the CU, or with scalar adds, the same code is exact
// (tools/debug_pair_bwd.py, profiles/r05/pair_form.txt 3 and 8).  A hand-written v_pk_add_f32 in the same place, and the
// compiler's add / subtract / select sequence verbatim in inline asm, are exact too: the mechanism is open.  With round 2's
// stale packed reads of matrix-core results (rime_common.h) it is the second sighting of compiler-packed f32 arithmetic going
// wrong beside a busy matrix pipe, so the pair kernels contain NO packed f32 instruction (the build scans for them): a fence
// around an observed failure, not an explanation of it.
__device__ __forceinline__ void keep_scalar(float& x) { asm("" : "+v"(x)); }

// Phase of a phasor in turns: a.s = ax sx + ay sy + az sz in float64 (antenna coordinates pre-multiplied by sign nu / c), reduced to
// its fraction as a float32 for v_sin_f32 / v_cos_f32 (a fixed-point reduction in the low mantissa bits saves two instructions
// per phasor for 2.2 x the phase noise: measured, not adopted -- profiles/r04/phase_magic_ab.txt, tools/lab/).
__device__ __forceinline__ double phase3(double ax, double sx, double ay, double sy, double az, double sz)
{
    return ax * sx + ay * sy + az * sz;
}
__device__ __forceinline__ float turn_frac(double ph) { return (float)__builtin_amdgcn_fract(ph); }

// FLAT (round 5, the conjugate-pair kernels): every row's z coordinate is zero (a coplanar array measured from a centre in its
// plane -- the layouts simulations run on), so the third term of the phase is exactly zero and is not evaluated: one f64 FMA
// less per phasor (3 % of a headline step; a licence stated by the caller, like `mirror`)
template <bool FLAT>
__device__ __forceinline__ double phase_of(double ax, double sx, double ay, double sy, double az, double sz)
{
    if constexpr (FLAT) return ax * sx + ay * sy;
    else return phase3(ax, sx, ay, sy, az, sz);
}

__device__ __forceinline__ f16x8 as_frag(const uint4& v) { return __builtin_bit_cast(f16x8, v); }

#define RIME_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16(as_frag(a), as_frag(b), c, 0, 0, 0)

// ---- host: from the arguments of a block entry point to its launches -----------------------------------------------------
// An A/B switch of the environment: atoi of the variable, `dflt` where it is not set.  A caller keeps the answer in a
// function-local static, so that the variable is read once, on first use.
inline bool env_flag(const char* name, int dflt)
{
    const char* e = getenv(name);
    return (e ? atoi(e) : dflt) != 0;
}

struct PixelSplit { int S, per; };            // blocks along the pixel axis of one (t, f) row, panels or tiles in each

// Forward: every block writes a slab of its own, summed by reduce_vis_kernel.  At most MF_SPLIT_PIX pixels per block; more
// splits while the grid is below ~4 blocks per CU; splits start on 64-pixel boundaries (four panels)
inline PixelSplit fwd_split_plan(int Nt, int Nf, int Pstride)
{
    long S = (Pstride + MF_SPLIT_PIX - 1) / MF_SPLIT_PIX;
    const long blocks = (long)Nt * Nf;
    const long maxS = std::max(1, Pstride / 1024);
    while (blocks * S < 1024 && S < maxS) ++S;
    S = std::max<long>(1, S);
    const int npanel = Pstride / MF_KP;
    const int per = (((npanel + (int)S - 1) / (int)S + 3) / 4) * 4;
    return {(npanel + per - 1) / per, per};
}

inline size_t fwd_workspace_bytes(int Nbl, int Nt, int Nf, int Pstride)
{
    return (size_t)fwd_split_plan(Nt, Nf, Pstride).S * Nbl * Nt * Nf * 2 * sizeof(float);
}

// Backward: pixel ranges are independent outputs, split freely for parallelism (>= 256 pixel tiles of 32 per block amortise
// the G staging; fewer when the grid would otherwise be small)
inline PixelSplit bwd_split_plan(int Nt, int Nf, int Pstride)
{
    const int ntile = Pstride / 32;
    int per = 256;
    while (per > 8 && (long)Nt * Nf * ((ntile + per - 1) / per) < 1024) per /= 2;
    return {(ntile + per - 1) / per, per};
}

// Conjugate-pair backward: every block of a (t, f) row builds the same eight G planes from ~250 scattered loads per thread
// before its pixel loop, and its waves issue nothing else meanwhile (three blocks share a CU).  Where the grid is large the
// splits widen -- up to 1024 tiles, while 8 rounds of 3 blocks x 256 CUs remain to level the tail: the C4 diffuse launch
// (2048 rows x 3072 tiles) stages 3 times per row instead of 12 (12.72 -> 12.28 ms per step, profiles/r14/pair_bwd_stage.txt).
// Below 12 288 blocks of 256 tiles this is bwd_split_plan.  Pixel tiles are independent outputs: same bits for every split.
// The threshold is calibrated on ONE shape, the C4 diffuse launch of the two-tile kernel (3 blocks per CU on the 256 CUs of
// an MI355X; 6 and 3 stagings measured there): other shapes that widen (say 1024 rows x 98 304 pixels) follow the rule, not
// a measurement of their own.  RIME_PAIR_BWD_WIDE=0 keeps bwd_split_plan (A/B measurements, tests/test_pair_bwd_wide_gpu.py).
constexpr long PAIR_BWD_MIN_GRID = 8 * 3 * 256;
inline PixelSplit pair_bwd_split_plan(int Nt, int Nf, int Pstride)
{
    const int ntile = Pstride / 32;
    int per = bwd_split_plan(Nt, Nf, Pstride).per;
    while (per >= 256 && per < 1024 && (long)Nt * Nf * ((ntile + 2 * per - 1) / (2 * per)) >= PAIR_BWD_MIN_GRID) per *= 2;
    return {(ntile + per - 1) / per, per};
}
// the plan the pair backward launches with (the switch is read once)
inline PixelSplit pair_bwd_launch_plan(int Nt, int Nf, int Pstride)
{
    static const bool wide = env_flag("RIME_PAIR_BWD_WIDE", 1);
    return wide ? pair_bwd_split_plan(Nt, Nf, Pstride) : bwd_split_plan(Nt, Nf, Pstride);
}

// The fields every argument struct of these kernels has, under the same names
template <class Args>
inline void fill_geometry(Args& A, const double* antpos, const double* sdir, const double* freqs, const int* pair_direct,
                          const int* pair_conj, int Nbl, int Nt, int Nf, int Pstride, long long st_t, long long st_f,
                          long long st_p, int sign)
{
    A.antpos = antpos; A.sdir = sdir; A.freqs = freqs; A.pair_direct = pair_direct; A.pair_conj = pair_conj;
    A.Nbl = Nbl; A.Nt = Nt; A.Nf = Nf; A.Pstride = Pstride;
    A.st_t = st_t; A.st_f = st_f; A.st_p = st_p; A.sign = (double)sign;
}

// ... those of a forward block (after fill_geometry): input plane, slab workspace, pixel split; returns the grid
template <class Args>
inline dim3 fill_forward(Args& A, const float* psky, const float* scale, const float* rowmin, void* workspace)
{
    A.psky = psky; A.scale = scale; A.rowmin = rowmin; A.ws = (float*)workspace;
    const PixelSplit p = fwd_split_plan(A.Nt, A.Nf, A.Pstride);
    A.S = p.S; A.panels_per_split = p.per;
    return dim3((unsigned)A.Nt * A.S * A.Nf, 1, 1);
}

// ... and of a backward block: transposed gradient (the workspace rime_fringe_ant_bwd_prepare wrote), output plane, pixel split
template <class Args>
inline dim3 fill_backward(Args& A, const float* gscale, float* gpsky, const void* workspace, int accumulate,
                          PixelSplit (*plan)(int, int, int) = bwd_split_plan)
{
    A.gscale = gscale; A.gpsky = gpsky; A.gvt = (const float*)workspace; A.accumulate = accumulate ? 1 : 0;
    const PixelSplit p = plan(A.Nt, A.Nf, A.Pstride);
    A.S = p.S; A.tiles_per_split = p.per;
    return dim3((unsigned)A.Nt * A.S * A.Nf, 1, 1);
}

// One real plane of psky: the SIGNED = true instantiation serves the rows that hold a negative value, the SIGNED = false one
// (no sign masks) the others; each returns at once from the blocks of the other's rows.  Without row minima every row is signed.
template <class Args>
inline void launch_real_plane(void (*signed_kernel)(Args), void (*unsigned_kernel)(Args), dim3 grid, int threads, size_t lds,
                              hipStream_t st, const Args& A)
{
    hipLaunchKernelGGL(signed_kernel, grid, dim3(threads), lds, st, A);
    if (A.rowmin) hipLaunchKernelGGL(unsigned_kernel, grid, dim3(threads), lds, st, A);
}

} // namespace rime
