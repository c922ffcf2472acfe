// fringe_mfma_common.h -- what the matrix-core fringe sources (fringe_mfma.hip, fringe_xpair.hip) share: the small device
// helpers of their kernels and the host layer between the C ABI and hipLaunchKernelGGL.  No kernels, not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <utility>
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

// ---- device fragments of the forward kernels ------------------------------------------------------------
// What ant_fwd_body, ant_fwd_packed_body, pair_fwd_body, pair_fwd1_body (fringe_mfma.hip) and xpair_fwd_body (fringe_xpair.hip)
// share, once each, all forced inline.  KNOWN WEAKNESS: the f64 phase ax sx + ay sy + az sz is contracted by the compiler
// (-ffp-contract=fast), and which product stays a rounded multiply is its choice for every inlined copy of `generate`, so the
// last bit of a few visibilities per 10^6 depends on code structure.  A body uses a fragment only where tools/fringe_digest.py
// prints the same lines with and without it; DESIGN.md 5.1f lists what is written out where.  Follow-up: explicit fma() in
// phase3 / phase_of (an arithmetic change, to be made on its own), after which every body can take every fragment.
constexpr int MF_NA = 128;                      // antennas per block (4 x 4 tiles): rows / columns of the slot tables
constexpr int MF_NH = MF_KP / 16;               // 16-pixel K steps per panel
constexpr int MF_ROWB = 4 * MF_KP + 16;         // image row: [re KP x f16][im KP x f16][pad], an odd number of 16-B granules

// 1. Block coordinates.  1-D grid, channel fastest: blocks that run together share (t, split), i.e. the same pointing vectors
// (L2 hits), and no grid dimension hits the 65535 cap.  Panels [pbeg, pend) are this block's pixel split.
struct FwdBlock { int f, t, split, pbeg, pend; };
// `bid`: the block's index within its launch, or within its segment of a merged launch (blockIdx.x - A.block0)
template <class Args>
__device__ __forceinline__ FwdBlock fwd_block_at(const Args& A, unsigned bid)
{
    FwdBlock b;
    b.f = __builtin_amdgcn_readfirstlane(bid % A.Nf);
    const int ts = bid / A.Nf;
    b.t = __builtin_amdgcn_readfirstlane(ts / A.S);
    b.split = __builtin_amdgcn_readfirstlane(ts % A.S);
    b.pbeg = __builtin_amdgcn_readfirstlane(b.split * A.panels_per_split);
    b.pend = __builtin_amdgcn_readfirstlane(min(A.Pstride / MF_KP, b.pbeg + A.panels_per_split));
    return b;
}
template <class Args>
__device__ __forceinline__ FwdBlock fwd_block(const Args& A) { return fwd_block_at(A, blockIdx.x); }

// 1b. Segments (the conjugate-pair kernels): one launch serves up to MF_MAXSEG psky planes that share times, channels, rows and
// slot tables but have their own pixels -- the sky components of one RIME call.  The grid is the concatenation of the
// segments' grids (SegPlan below); a block finds its segment from blockIdx.x with scalar compares against the segments' first
// blocks and from then on reads that segment's bases: everything here is wave-uniform (SGPRs), no lane branches on it.
constexpr int MF_MAXSEG = 4;
template <class Seg>
__device__ __forceinline__ int segment_of(const Seg* seg, int nseg)
{
    int k = 0;
#pragma unroll
    for (int i = 1; i < MF_MAXSEG; ++i) k += (i < nseg && blockIdx.x >= seg[i].block0) ? 1 : 0;
    return __builtin_amdgcn_readfirstlane(k);
}
// A block works on one psky row (t, f): rows without a negative value (beam-weighted emission is non-negative) take the kernel
// instantiation without sign masks.  Both instantiations are launched over the full grid and a block returns at once when its
// row belongs to the other one: a branch inside one kernel costs registers (the allocator serves the union of both paths and spills).
template <class Args>
__device__ __forceinline__ bool row_is_signed(const Args& A, const FwdBlock& b)
{
    if (!A.rowmin) return true;
    return A.rowmin[b.t * A.Nf + b.f] < 0.f;
}

// 2. Panel source.  Wave-uniform bases (scalar address arithmetic) + constant 32-bit lane offsets; psky is read as two dwords
// with the runtime pixel stride (a branch on the stride makes the compiler issue both variants with 64-bit vector multiplies:
// 17 % of the loop's VALU work).  Buffer loads: descriptor (SGPRs, wave-uniform: built from kernel arguments and the block
// index) + constant per-lane offset + scalar panel offset -- no vector address arithmetic in the generation phase, whose cost
// is its instruction count (profiles/r03/lab_forward_experiments.txt); the descriptors bound the fetch to the row ([3][Pstride]
// doubles of sdir, Pstride strided floats of psky) and out-of-range reads return 0 instead of faulting.  The descriptor inputs
// go through readfirstlane: a base pointer the compiler cannot PROVE wave-uniform makes it wrap every buffer load in a
// waterfall loop of ~14 instructions -- seen on the psky descriptor, guide T20.
__device__ __forceinline__ void* uniform_ptr(const void* q)
{
    const unsigned long long a = reinterpret_cast<unsigned long long>(q);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo);
}
struct PanelSource {
    __amdgpu_buffer_rsrc_t rs, ra;               // the three sdir rows of time t; the psky row (t, f)
    uint32_t lo_s, lo_a0, lo_a1;                 // lane offsets of pixel pair pp: its two directions, its two psky values
    int Pstride, st_p;
};
template <class Args>
__device__ __forceinline__ PanelSource panel_source(const Args& A, const FwdBlock& b, int pp)
{
    const float* arow = A.psky + (size_t)b.t * A.st_t + (size_t)b.f * A.st_f;
    const double* sd = A.sdir + (size_t)b.t * 3 * A.Pstride;
    const int st_p = __builtin_amdgcn_readfirstlane((int)A.st_p);
    PanelSource s;
    s.Pstride = A.Pstride; s.st_p = st_p;
    s.lo_s = 16u * pp; s.lo_a0 = 8u * pp * (uint32_t)st_p; s.lo_a1 = s.lo_a0 + 4u * (uint32_t)st_p;
    s.rs = __builtin_amdgcn_make_buffer_rsrc(
        uniform_ptr(sd), 0, __builtin_amdgcn_readfirstlane((int)min((long long)3 * A.Pstride * 8, 0x7fffffffLL)), 0x00020000);
    s.ra = __builtin_amdgcn_make_buffer_rsrc(
        uniform_ptr(arow), 0, __builtin_amdgcn_readfirstlane((int)min((long long)A.Pstride * st_p * 4, 0x7fffffffLL)), 0x00020000);
    return s;
}
// the directions of this lane's pixel pair in the 16-pixel half `hf` of `panel`
__device__ __forceinline__ void fetch_dirs(const PanelSource& s, int panel, int hf, double2& sx, double2& sy, double2& sz)
{
    const int p0 = panel * MF_KP + 16 * hf;          // uniform
    sx = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(s.rs, (int)s.lo_s, p0 * 8, 0));
    sy = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(s.rs, (int)s.lo_s, (s.Pstride + p0) * 8, 0));
    sz = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(s.rs, (int)s.lo_s, (2 * s.Pstride + p0) * 8, 0));
}
// ... and its two psky values: the real plane (av), with CPLX the imaginary plane too (aw)
template <bool CPLX>
__device__ __forceinline__ void fetch_psky(const PanelSource& s, int panel, int hf, float2& av, float2& aw)
{
    const int so = (panel * MF_KP + 16 * hf) * s.st_p * 4;
    av = make_float2(__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(s.ra, (int)s.lo_a0, so, 0)),
                     __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(s.ra, (int)s.lo_a1, so, 0)));
    if constexpr (CPLX)
        aw = make_float2(__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(s.ra, (int)s.lo_a0 + 4, so, 0)),
                         __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(s.ra, (int)s.lo_a1 + 4, so, 0)));
}
__device__ __forceinline__ void fetch_psky(const PanelSource& s, int panel, int hf, float2& av)
{
    fetch_psky<false>(s, panel, hf, av, av);
}

// 3. Row mapping of the half-panel generation: lane = (pixel pair pp = lane & 7, row ag = lane >> 3 of an octet); the rows of a
// sweep are one OCTET per wave pair p = W >> 1 -- 2 apart inside a wave: conflict-free ds_write_b32 -- and the sweeps of a wave
// pair walk the octets of ONE 16-row group after the other: sweep u = rows 32 (u >> 1) + 16 p + 8 (u & 1) + i, so that the
// mirror antennas of a sweep's rows (AntArgs.mirror) are the next sweep's rows of the same lanes.
__device__ __forceinline__ int octet_lane_row(int W, int ag) { return 16 * (W >> 1) + 2 * (ag & 3) + (ag >> 2); }
__device__ __forceinline__ int octet_row(int u, int orow) { return 32 * (u >> 1) + 8 * (u & 1) + orow; }
// sweeps whose octet starts below Nant (monotone in u; uniform): the others are whole octets of padding and are skipped
__device__ __forceinline__ int octet_sweeps(int Nant, int W, int ngen)
{
    const int mrow = Nant - 16 * (W >> 1);
    return min(ngen, (max(mrow, 0) + 31) / 32 + (max(mrow - 8, 0) + 31) / 32);
}
// coordinates of antenna `an` scaled by sign nu / c; zero for a padding row
__device__ __forceinline__ void load_ant(const double* antpos, int an, bool ok, double nu_c, double& ax, double& ay, double& az)
{
    ax = ok ? nu_c * antpos[3 * an] : 0.0;
    ay = ok ? nu_c * antpos[3 * an + 1] : 0.0;
    az = ok ? nu_c * antpos[3 * an + 2] : 0.0;
}

// 4. Phasor pair: E = c + i s of the antenna at (bx, by, bz) for the lane's two pixels (.x and .y of the directions)
template <bool FLAT>
__device__ __forceinline__ void phasor_pair(double bx, double by, double bz, const double2& sx, const double2& sy,
                                            const double2& sz, float& c0, float& s0, float& c1, float& s1)
{
    const double ph0 = phase_of<FLAT>(bx, sx.x, by, sy.x, bz, sz.x);
    const double ph1 = phase_of<FLAT>(bx, sx.y, by, sy.y, bz, sz.y);
    const float r0 = turn_frac(ph0), r1 = turn_frac(ph1);
    s0 = __builtin_amdgcn_sinf(r0); c0 = __builtin_amdgcn_cosf(r0);
    s1 = __builtin_amdgcn_sinf(r1); c1 = __builtin_amdgcn_cosf(r1);
}

// 5. Weights of the symmetric form, w = sqrt(|psky| scale) for the lane's two pixels; g: the same with the sign of psky (SIGNED
// ROWS in fringe_mfma.hip); sign_dword: the signs as the XOR mask of a packed f16 pair, stored behind the images of a panel
__device__ __forceinline__ void pixel_weights(const float2& av, float scl, float& w0, float& w1)
{
    w0 = __builtin_amdgcn_sqrtf(fabsf(av.x) * scl); w1 = __builtin_amdgcn_sqrtf(fabsf(av.y) * scl);
}
__device__ __forceinline__ void signed_weights(const float2& av, float w0, float w1, float& g0, float& g1)
{
    g0 = __uint_as_float(__float_as_uint(w0) | (__float_as_uint(av.x) & 0x80000000u));
    g1 = __uint_as_float(__float_as_uint(w1) | (__float_as_uint(av.y) & 0x80000000u));
}
__device__ __forceinline__ uint32_t sign_dword(const float2& av)
{
    return ((__float_as_uint(av.x) >> 16) & 0x8000u) | (__float_as_uint(av.y) & 0x80000000u);
}

// 6. Image store: the packed f16 (p, p + 1) pairs of one row at o = row and half-panel offset; IMG = bytes of the hi image
template <int IMG>
__device__ __forceinline__ void store_image(unsigned char* o, uint32_t rh, uint32_t rl, uint32_t ih, uint32_t il)
{
    *reinterpret_cast<uint32_t*>(o) = rh;
    *reinterpret_cast<uint32_t*>(o + 2 * MF_KP) = ih;
    *reinterpret_cast<uint32_t*>(o + IMG) = rl;
    *reinterpret_cast<uint32_t*>(o + IMG + 2 * MF_KP) = il;
}

// 7. Accumulators.  Element e of a 32 x 32 accumulator is row acc_row(e, lane >> 5), column lane & 31.
__device__ __forceinline__ void zero(f32x16& a)
{
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] = 0.f;
}
__device__ __forceinline__ int acc_row(int e, int half) { return (e & 3) + 8 * (e >> 2) + 4 * half; }
// the transpose of a tile through a private 32 x 33 float tile of LDS (written and read by this wave only)
__device__ __forceinline__ f32x16 transposed(float* tr, const f32x16& v, int col, int half)
{
    f32x16 tv;
#pragma unroll
    for (int e = 0; e < 16; ++e) tr[acc_row(e, half) * 33 + col] = v[e];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int e = 0; e < 16; ++e) tv[e] = tr[col * 33 + acc_row(e, half)];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    return tv;
}
// This block's slab ws[split][t][f][re|im][Nbl]: consecutive lanes (columns j) hit consecutive baseline slots, so the stores
// coalesce (a scattered store into the [Nbl][Nt][Nf][2] result costs a 32-B sector per 4-B value: 8 GB instead of 1.6 GB per
// launch at C4); reduce_vis_kernel sums the splits in a fixed order and transposes into the result layout.
template <class Args>
__device__ __forceinline__ float* fwd_slab(const Args& A, const FwdBlock& b)
{
    return A.ws + (((size_t)b.split * A.Nt + b.t) * A.Nf + b.f) * 2 * A.Nbl;
}
// V[r, c] = vr + i vi -> the baseline slot(s) of pair (r, c) in the slab; put1: one plane of it
template <class Args>
__device__ __forceinline__ void put(const Args& A, float* dst, int r, int c, float vr, float vi)
{
    const int bd = A.pair_direct[r * MF_NA + c];
    if (bd >= 0) { dst[bd] = vr; dst[(size_t)A.Nbl + bd] = vi; }
    const int bc = A.pair_conj[r * MF_NA + c];
    if (bc >= 0) { dst[bc] = vr; dst[(size_t)A.Nbl + bc] = -vi; }
}
template <class Args>
__device__ __forceinline__ void put1(const Args& A, float* dst, int r, int c, int im, float v)
{
    const int bd = A.pair_direct[r * MF_NA + c];
    if (bd >= 0) dst[(size_t)im * A.Nbl + bd] = v;
    const int bc = A.pair_conj[r * MF_NA + c];
    if (bc >= 0) dst[(size_t)im * A.Nbl + bc] = im ? -v : v;
}

// 8. Wave dispatch: go(int_c<W>{}) for this thread's wave W of NW.  Wave-uniform: every wave runs the same barriers.
template <int NW, class F>
__device__ __forceinline__ void for_wave(F&& go)
{
    static_assert(NW == 4 || NW == 8, "blocks of four or eight waves");
    const int w = threadIdx.x >> 6;
    if constexpr (NW == 4) {
        switch (w) {
            case 0: go(int_c<0>{}); break;
            case 1: go(int_c<1>{}); break;
            case 2: go(int_c<2>{}); break;
            default: go(int_c<3>{}); break;
        }
    } else {
        switch (w) {
            case 0: go(int_c<0>{}); break;
            case 1: go(int_c<1>{}); break;
            case 2: go(int_c<2>{}); break;
            case 3: go(int_c<3>{}); break;
            case 4: go(int_c<4>{}); break;
            case 5: go(int_c<5>{}); break;
            case 6: go(int_c<6>{}); break;
            default: go(int_c<7>{}); break;
        }
    }
}

// ---- device fragments of the backward kernels -----------------------------------------------------------
// What the four backward kernels (fringe_mfma.hip, fringe_xpair.hip) share, once each, all forced inline.  A kernel takes a fragment
// only where every one of its instantiations compiles to the instruction stream it had without it (tools/compare_kernel_asm.py);
// DESIGN.md 5.1g lists what was tried and stays written out where, with the figures.
// 1. Antenna staging: coordinates x sign nu / c into LDS, zero for the padding rows (NT = threads of the block)
template <class Args> __device__ __forceinline__ double scaled_freq(const Args& A, int f) { return A.sign * A.freqs[f] * (1.0 / 2.99792458e8); }
template <int NT>
__device__ __forceinline__ void stage_ant(double* ant_lds, const double* antpos, int nlds, int nlive, double nu_c)
{
    for (int i = threadIdx.x; i < nlds; i += NT) ant_lds[i] = (i < nlive) ? nu_c * antpos[i] : 0.0;
}

// 2. G gather: the gradient with respect to V[r, c] of the block, slot = r * MF_NA + c -- the direct slot plus the conjugate
// of the conj slot, ADDED to (gr, gi).  SCALAR: every sum fenced (the conjugate-pair kernels, see keep_scalar).
template <bool SCALAR = false>
__device__ __forceinline__ void gather_g(const float* gre, const float* gim, const int* direct, const int* conj, int slot,
                                         float& gr, float& gi)
{
    const int bd = direct[slot];
    if (bd >= 0) {
        gr += gre[bd]; if constexpr (SCALAR) keep_scalar(gr);
        gi += gim[bd]; if constexpr (SCALAR) keep_scalar(gi);
    }
    const int bc = conj[slot];
    if (bc >= 0) {
        gr += gre[bc]; if constexpr (SCALAR) keep_scalar(gr);
        gi -= gim[bc]; if constexpr (SCALAR) keep_scalar(gi);
    }
}

// 3. Plane stores.  A staging thread packs the (jj, jj + 1) pair of fragment element (tile, ks, h, row), g_off bytes into a plane;
// store_planes: the complex entry (rh + rl) + i (ih + il) into planes [re, im, (-im)] hi, then lo (NEG: with the negated copy)
__device__ __forceinline__ int g_off(int tile, int ks, int h, int row, int jp) { return ((((tile * 2 + ks) * 2 + h) * 32 + row) * 4 + jp) * 4; }
template <int PLANE, bool NEG>
__device__ __forceinline__ void store_planes(unsigned char* g_img, int off, uint32_t rh, uint32_t rl, uint32_t ih, uint32_t il)
{
    constexpr int NP = NEG ? 3 : 2;
    *reinterpret_cast<uint32_t*>(g_img + 0 * PLANE + off) = rh;
    *reinterpret_cast<uint32_t*>(g_img + 1 * PLANE + off) = ih;
    if constexpr (NEG) *reinterpret_cast<uint32_t*>(g_img + 2 * PLANE + off) = ih ^ 0x80008000u;
    *reinterpret_cast<uint32_t*>(g_img + NP * PLANE + off) = rl;
    *reinterpret_cast<uint32_t*>(g_img + (NP + 1) * PLANE + off) = il;
    if constexpr (NEG) *reinterpret_cast<uint32_t*>(g_img + 5 * PLANE + off) = il ^ 0x80008000u;
}

// 4. K index -> row: element jj of K step ks of column tile tj, in half-wave h = 32 tj + acc_row(8 ks + jj, h), the accumulator rows a lane holds
__device__ __forceinline__ int bwd_row_of(int tj, int ks, int jj, int h) { return 32 * tj + (jj & 3) + 8 * (2 * ks + (jj >> 2)) + 4 * h; }
// ... of the pair (jj, jj + 1) = (2 jp, 2 jp + 1) a staging thread packs: the row of its first element
__device__ __forceinline__ int bwd_row_of_pair(int tj, int ks, int jp, int h) { return 32 * tj + ((2 * jp) & 3) + 8 * (2 * ks + (jp >> 1)) + 4 * h; }

// 5. Directions of the lane's pixel, and the phasor c + i s of row `an` of ant_lds ([row][3], scaled) towards it
template <bool FLAT>
__device__ __forceinline__ void load_dir(const double* sd, int Pstride, int p, double& sx, double& sy, double& sz)
{
    sx = sd[p]; sy = sd[Pstride + p]; sz = FLAT ? 0.0 : sd[2 * (size_t)Pstride + p];
}
template <bool FLAT>
__device__ __forceinline__ void phasor(const double* ant_lds, int an, double sx, double sy, double sz, float& c, float& s)
{
    const double ph = phase_of<FLAT>(ant_lds[3 * an], sx, ant_lds[3 * an + 1], sy, ant_lds[3 * an + 2], sz);
    const float rr = turn_frac(ph);
    c = __builtin_amdgcn_cosf(rr);
    s = __builtin_amdgcn_sinf(rr);
}

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

// ---- host: the segment plan of a merged pair launch -----------------------------------------------------
// Segment k (caller's order) has Pstride[k] pixels per (t, f) row.  Forward: every segment keeps fwd_split_plan; its slabs
// follow those of the segments before it in the CALLER's order (slab0), which is the order reduce_vis_kernel sums in.
// Backward: every segment starts from bwd_split_plan and widens by the rule of pair_bwd_split_plan with the grid condition
// taken on the COMBINED grid (the other segments' blocks level the tail as well as its own).  In the grid the segments stand
// by falling work per block row (pixels), ties in caller order: the short blocks of the small segments fill the tail
// (order[], block0[] in grid order).  One segment: exactly the plan of the single launch.
struct SegPlan {
    int nseg;
    int S[MF_MAXSEG], per[MF_MAXSEG];           // by segment: splits, panels (forward) / tiles (backward) per split
    long slab0[MF_MAXSEG];                      // by segment: first slab (forward)
    int order[MF_MAXSEG];                       // grid position -> segment
    long block0[MF_MAXSEG];                     // grid position -> first block
    long grid, slabs;
};
struct SegBlock { int seg, f, t, split, begin, end; };      // [begin, end): panels (forward) or pixel tiles (backward)

inline bool seg_plan(bool backward, bool wide, int Nt, int Nf, const int* Pstride, int nseg, SegPlan& p)
{
    if (nseg < 1 || nseg > MF_MAXSEG || Nt <= 0 || Nf <= 0) return false;
    p = SegPlan{};
    p.nseg = nseg;
    const long rows = (long)Nt * Nf;
    for (int k = 0; k < nseg; ++k) {
        if (Pstride[k] <= 0 || Pstride[k] % 64 != 0) return false;
        const PixelSplit s = backward ? bwd_split_plan(Nt, Nf, Pstride[k]) : fwd_split_plan(Nt, Nf, Pstride[k]);
        p.S[k] = s.S; p.per[k] = s.per;
        p.order[k] = k;
    }
    for (int a = 1; a < nseg; ++a)              // stable insertion sort, most pixels first
        for (int b = a; b > 0 && Pstride[p.order[b]] > Pstride[p.order[b - 1]]; --b) std::swap(p.order[b], p.order[b - 1]);
    if (backward && wide) {
        long total = 0;
        for (int k = 0; k < nseg; ++k) total += rows * p.S[k];
        for (int g = 0; g < nseg; ++g) {
            const int k = p.order[g], ntile = Pstride[k] / 32;
            int per = p.per[k];
            long others = total - rows * p.S[k];
            while (per >= 256 && per < 1024 && others + rows * ((ntile + 2 * per - 1) / (2 * per)) >= PAIR_BWD_MIN_GRID) per *= 2;
            p.per[k] = per; p.S[k] = (ntile + per - 1) / per;
            total = others + rows * p.S[k];
        }
    }
    for (int k = 0; k < nseg; ++k) { p.slab0[k] = p.slabs; p.slabs += p.S[k]; }
    for (int g = 0; g < nseg; ++g) { p.block0[g] = p.grid; p.grid += rows * p.S[p.order[g]]; }
    return p.grid <= 0x7fffffffL;
}

// the block -> (segment, f, t, split, range) map of the kernels (segment_of, fwd_block_at), on the host
inline SegBlock seg_block(const SegPlan& p, int Nf, const int* Pstride, bool backward, long b)
{
    int g = 0;
    for (int i = 1; i < p.nseg; ++i) g += b >= p.block0[i] ? 1 : 0;
    const int k = p.order[g];
    const long bid = b - p.block0[g], ts = bid / Nf;
    SegBlock r;
    r.seg = k; r.f = (int)(bid % Nf); r.t = (int)(ts / p.S[k]); r.split = (int)(ts % p.S[k]);
    r.begin = r.split * p.per[k];
    r.end = std::min(Pstride[k] / 32, r.begin + p.per[k]);
    return r;
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
