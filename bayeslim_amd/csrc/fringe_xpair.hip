// fringe_xpair.hip -- conjugate-pair CROSS blocks of the antenna-factored fringe sum on the matrix cores (gfx950).
//
// fringe_mfma.hip contracts a point-symmetric group of up to 128 antennas from the phasors of one antenna of every mirror pair
// (CONJUGATE-PAIR FORM there).  An array with more antennas is cut into several such groups, all symmetric about the SAME
// centre c, and the block between two groups I and J has the same structure.  Row k of I holds a first x_k (its mirror x'_k has
// the phasor conj(E_x)), row l of J a first y_l.  With E = C + i S, w one real plane of psky and the real products over pixels
//     Pcc = Cx^T w Cy,   Pss = Sx^T w Sy,   Pcs = Cx^T w Sy,   Psc = Sx^T w Cy              (each rows_i x rows_j)
// a baseline a -> b has V = sum_p w conj(E_a) E_b, so
//     V[x , y ] = (Pcc + Pss) + i (Pcs - Psc)        V[x', y'] = its conjugate
//     V[x', y ] = (Pcc - Pss) + i (Pcs + Psc)        V[x , y'] = its conjugate
// Four real products of at most 64 x 64 give the four quadrants of what is a 128 x 128 generic cross block otherwise: 4 products
// x 4 tiles x 3 (f16 hi / lo split) = 48 MFMAs per 16-pixel K step instead of 192, from 128 generated rows instead of 256.
// An antenna without a partner is a row whose mirror quadrants have no slot; an antenna AT the centre is a row with position 0.
//
// Backward, real psky:  gpsky[p] = Cx^T Ncc Cy + Sx^T Nss Sy + Cx^T Ncs Sy + Sx^T Nsc Cy  with (gA = g V[x,y], gA' = g V[x',y'],
// gB = g V[x',y], gB' = g V[x,y'])
//     Ncc = Re(gA + gA' + gB + gB')    Nss = Re(gA + gA' - gB - gB')    Ncs = Im(gA - gA' + gB - gB')    Nsc = Im(-gA + gA' + gB - gB')
// i.e. T1 = Ncc Cy + Ncs Sy, T2 = Nsc Cy + Nss Sy on the matrix cores (48 MFMAs per 16 pixels as well) and a lane-local
// contraction with (Cx, Sx).
//
// The operand formats, the f16 hi / lo split, the f64 phase with hardware sine / cosine in turns, the LDS image layout, the
// pixel-split slabs of the forward (summed by rime_fringe_ant_fwd_finish) and the transposed gradient of the backward (written by
// rime_fringe_ant_bwd_prepare) are those of fringe_mfma.hip; the small device helpers and the host layer between the C ABI and the
// launches are shared with it (fringe_mfma_common.h).  This file stays a translation unit of its own: built and scanned on its
// own.  Blocks of these kernels share a CU, so -- like the pair kernels -- they hold no packed f32 instruction (keep_scalar in
// fringe_mfma_common.h; the build scans for them).  The kernels' names carry `xpair`.
#include "fringe_mfma_common.h"

namespace rime {
namespace xp {

constexpr int NA = MF_NA;                    // rows / columns of the slot tables (virtual block: 64 firsts + 64 mirrors a side)
constexpr int XR = 64;                       // rows of one group
constexpr int KP = MF_KP;                    // pixels per panel; 16 per MFMA
constexpr int NH = MF_NH;
constexpr int ROWB = MF_ROWB;                // [re KP x f16][im KP x f16][pad]: odd number of 16-B granules
constexpr int IMG = 2 * XR * ROWB;           // one image (hi or lo): rows 0..63 group I, 64..127 group J
constexpr int BUF = 2 * IMG + 64;            // hi + lo (+ 64 bytes that held the panel's sign dwords: unused, the offsets stay)
constexpr size_t FWD_LDS = 2 * (size_t)BUF;

struct FwdArgs {
    const double* antpos;      // [rows_i + rows_j, 3] from the centre of symmetry: group I, then group J
    const double* sdir;        // [Nt, 3, Pstride]
    const double* freqs;       // [Nf]
    const float* psky;         // strided [t][f][p]
    const float* scale;        // [Nt, Nf] power-of-two pre-scale of psky rows
    const float* rowmin;       // [Nt, Nf] min of each psky row, or NULL
    const int* pair_direct;    // [128*128]: slot receiving V[r, c], r = x_k (k) | x'_k (64 + k), c = y_l (l) | y'_l (64 + l)
    const int* pair_conj;      // [128*128]: slot receiving conj(V[r, c])
    float* ws;                 // partial slabs [S][Nt][Nf][re | im][Nbl]
    int rows_i, rows_j, Nbl, Nt, Nf, Pstride;
    int S, panels_per_split;
    long long st_t, st_f, st_p;
    double sign;
};

// Forward.  Block = one (t, f, pixel split), four waves.  Generation as in the pair kernels: lane = (pixel pair, row of an octet),
// a wave writes one 16-pixel half of the panel for every second 16-row group of the 128 image rows (8 sweeps; octets that hold
// padding rows only are skipped).  Symmetric weighting: both groups' rows hold sqrt(|psky| scale) E, and the rows of group I are
// GENERATED with the sign of psky in their weight (SIGNED ROWS in fringe_mfma.hip: L always comes from group I, B from group J, so
// no fragment is signed after it is read; the stored f16 pairs are bit for bit those an XOR mask on the group-I fragments gave:
// cvt_pkrtz is odd, the residual of the split an exact negation).  Wave W contracts output tile (W >> 1, W & 1): Pcc, Pss, Pcs, Psc in four accumulators, 12
// MFMAs per K step.  The pieces shared with the other forward kernels are the fragments of fringe_mfma_common.h.
template <int W, bool SIGNED, bool FLAT>
__device__ __forceinline__ void xpair_fwd_body(const FwdArgs& A, unsigned char* smem)
{
    const FwdBlock blk = fwd_block(A);
    const int tid = threadIdx.x, lane = tid & 63;
    const int f = blk.f, t = blk.t;

    const double nu_c = A.sign * A.freqs[f] * (1.0 / 2.99792458e8);
    const float scl = A.scale[t * A.Nf + f];

    const int pp = lane & 7, ag = lane >> 3;
    constexpr int hf = W & 1;
    constexpr int NGEN = 8;
    const int orow = octet_lane_row(W, ag);
    // sweeps whose octet holds a row of its group (uniform over the wave)
    uint32_t live = 0;
    double ax[NGEN], ay[NGEN], az[NGEN];
#pragma unroll
    for (int u = 0; u < NGEN; ++u) {
        const int base = octet_row(u, 16 * (W >> 1));
        const bool on = base < XR ? base < A.rows_i : base - XR < A.rows_j;
        live |= (on ? 1u : 0u) << u;
        const int r = octet_row(u, orow);            // image row of this lane in sweep u
        const bool ok = r < XR ? r < A.rows_i : r - XR < A.rows_j;
        load_ant(A.antpos, r < XR ? r : A.rows_i + (r - XR), ok, nu_c, ax[u], ay[u], az[u]);
    }
    live = __builtin_amdgcn_readfirstlane(live);

    f32x16 acc[4];                                   // 0 Pcc, 1 Pss, 2 Pcs, 3 Psc
#pragma unroll
    for (int s = 0; s < 4; ++s) zero(acc[s]);

    if (blk.pbeg >= blk.pend) return;                // uniform over the block

    double2 sx, sy, sz = make_double2(0.0, 0.0); float2 av;
    // panel source in place, offsets through readfirstlane (bit-stable results, no waterfall loop)
    const float* arow = A.psky + (size_t)t * A.st_t + (size_t)f * A.st_f;
    const double* sd = A.sdir + (size_t)t * 3 * A.Pstride;
    const int st_p = __builtin_amdgcn_readfirstlane((int)A.st_p);
    const uint32_t lo_s = 16u * pp, lo_a0 = 8u * pp * (uint32_t)st_p, lo_a1 = lo_a0 + 4u * (uint32_t)st_p;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        uniform_ptr(sd), 0, __builtin_amdgcn_readfirstlane((int)min((long long)3 * A.Pstride * 8, 0x7fffffffLL)), 0x00020000);
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
        uniform_ptr(arow), 0, __builtin_amdgcn_readfirstlane((int)min((long long)A.Pstride * st_p * 4, 0x7fffffffLL)), 0x00020000);
    auto fetch = [&](int panel) {
        const int p0 = panel * KP + 16 * hf;         // uniform
        const int oy = __builtin_amdgcn_readfirstlane((A.Pstride + p0) * 8), oz = __builtin_amdgcn_readfirstlane((2 * A.Pstride + p0) * 8);
        sx = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)lo_s, p0 * 8, 0));
        sy = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)lo_s, oy, 0));
        if constexpr (!FLAT) sz = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)lo_s, oz, 0));
        const int so = __builtin_amdgcn_readfirstlane(p0 * st_p * 4);
        av = make_float2(__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ra, (int)lo_a0, so, 0)),
                         __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ra, (int)lo_a1, so, 0)));
    };
    auto generate = [&](unsigned char* buf, int next_panel) {
        float w0, w1;
        pixel_weights(av, scl, w0, w1);
        // the weight of group I's rows (sweeps 0..3) carries the sign of psky
        float g0 = w0, g1 = w1;
        if constexpr (SIGNED) signed_weights(av, w0, w1, g0, g1);
#pragma unroll
        for (int u = 0; u < NGEN; ++u) {
            if ((live >> u) & 1u) {
                const float m0 = u < 4 ? g0 : w0, m1 = u < 4 ? g1 : w1;
                float c0, s0, c1, s1;
                phasor_pair<FLAT>(ax[u], ay[u], az[u], sx, sy, sz, c0, s0, c1, s1);
                float xr0 = m0 * c0, xr1 = m1 * c1, xi0 = m0 * s0, xi1 = m1 * s1;
                keep_scalar(xr0); keep_scalar(xr1); keep_scalar(xi0); keep_scalar(xi1);
                uint32_t rh, rl, ih, il;
                split2(xr0, xr1, rh, rl);
                split2(xi0, xi1, ih, il);
                store_image<IMG>(buf + octet_row(u, orow) * ROWB + pp * 4 + 32 * hf, rh, rl, ih, il);
            }
        }
        fetch(next_panel);
    };

    constexpr int ti = W >> 1, tj = W & 1;
    const int foff = (lane & 31) * ROWB + (lane >> 5) * 16;      // fragment: row, k-half
    auto contract = [&](const unsigned char* buf) {
        auto frag = [&](int tile, int img, int im, int ks) {
            return *reinterpret_cast<const uint4*>(buf + img * IMG + tile * 32 * ROWB + foff + im * 2 * KP + 32 * ks);
        };
#pragma unroll
        for (int ks = 0; ks < NH; ++ks) {
            const uint4 Lrh = frag(ti, 0, 0, ks), Lih = frag(ti, 0, 1, ks);
            const uint4 Lrl = frag(ti, 1, 0, ks), Lil = frag(ti, 1, 1, ks);
            const uint4 Brh = frag(2 + tj, 0, 0, ks), Bih = frag(2 + tj, 0, 1, ks);
            const uint4 Brl = frag(2 + tj, 1, 0, ks), Bil = frag(2 + tj, 1, 1, ks);
            acc[0] = RIME_MFMA(Lrh, Brh, acc[0]);
            acc[1] = RIME_MFMA(Lih, Bih, acc[1]);
            acc[2] = RIME_MFMA(Lrh, Bih, acc[2]);
            acc[3] = RIME_MFMA(Lih, Brh, acc[3]);
            acc[0] = RIME_MFMA(Lrh, Brl, acc[0]);
            acc[1] = RIME_MFMA(Lih, Bil, acc[1]);
            acc[2] = RIME_MFMA(Lrh, Bil, acc[2]);
            acc[3] = RIME_MFMA(Lih, Brl, acc[3]);
            acc[0] = RIME_MFMA(Lrl, Brh, acc[0]);
            acc[1] = RIME_MFMA(Lil, Bih, acc[1]);
            acc[2] = RIME_MFMA(Lrl, Bih, acc[2]);
            acc[3] = RIME_MFMA(Lil, Brh, acc[3]);
        }
    };

    fetch(blk.pbeg);
    // two panels per trip: buffer addresses are compile-time offsets
    unsigned char* const buf0 = smem;
    unsigned char* const buf1 = smem + BUF;
    const int pbeg = blk.pbeg, pend = blk.pend;
    generate(buf0, min(pbeg + 1, pend - 1));
    __syncthreads();
    for (int panel = pbeg; panel < pend; panel += 2) {
        if (panel + 1 < pend) generate(buf1, min(panel + 2, pend - 1));
        contract(buf0);
        __syncthreads();
        if (panel + 1 < pend) {
            if (panel + 2 < pend) generate(buf0, min(panel + 3, pend - 1));
            contract(buf1);
        }
        __syncthreads();
    }

    // epilogue: the block's slab through the tables of the virtual 128 x 128 block
    float* dst = fwd_slab(A, blk);
    const float inv = 1.0f / scl;
    const int col = lane & 31;
    RIME_MFMA_SETTLE();
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int i = 32 * ti + acc_row(e, lane >> 5), j = 32 * tj + col;
        float ar = acc[0][e] + acc[1][e]; keep_scalar(ar);
        float br = acc[0][e] - acc[1][e]; keep_scalar(br);
        float ai = acc[2][e] - acc[3][e]; keep_scalar(ai);
        float bi = acc[2][e] + acc[3][e]; keep_scalar(bi);
        ar *= inv; keep_scalar(ar); br *= inv; keep_scalar(br); ai *= inv; keep_scalar(ai); bi *= inv; keep_scalar(bi);
        put(A, dst, i, j, ar, ai);                   // x  -> y
        put(A, dst, XR + i, XR + j, ar, -ai);        // x' -> y'
        put(A, dst, XR + i, j, br, bi);              // x' -> y
        put(A, dst, i, XR + j, br, -bi);             // x  -> y'
    }
}

template <bool SIGNED, bool FLAT>
__global__ void __launch_bounds__(256, 2)
fringe_xpair_fwd_kernel(FwdArgs A)
{
    extern __shared__ __align__(16) unsigned char smem[];
    if (row_is_signed(A, fwd_block(A)) != SIGNED) return;        // uniform over the block
    for_wave<4>([&](auto w) { xpair_fwd_body<w(), SIGNED, FLAT>(A, smem); });
}

struct BwdArgs {
    const double* antpos; const double* sdir; const double* freqs;
    const float* gvt;          // workspace: gvis transposed to [Nt, Nf, re | im, Nbl]
    const float* gscale;       // [Nt, Nf] power-of-two pre-scale of gvis
    const int* pair_direct; const int* pair_conj;
    float* gpsky;              // strided [t][f][p]
    int rows_i, rows_j, Nbl, Nt, Nf, Pstride;
    int S, tiles_per_split;    // pixel tiles (32 px) per block
    int accumulate;
    long long st_t, st_f, st_p;
    double sign;
};

// Backward.  Block = one (t, f, pixel range), four waves, a wave per 32-pixel tile.  Staging: the four N planes (hi and lo) of
// the block in A-fragment order -- (tile, K step, half-wave, row) x 8 f16, tile = 2 ti + tj -- and the coordinates of all rows.
// A lane generates the phasors of ITS pixel: the 16 group-J rows of a K step as the B fragment, in the order of the accumulator
// rows ((e & 3) + 8 (e >> 2) + 4 h), and at the end the group-I rows of each row tile in the same order for the lane-local
// contraction with T1, T2.  G is scaled by gscale / 8: an entry sums up to eight gradients (four quadrants, two orientations).
constexpr int XB_TILE = 2 * 2 * 32 * 16;             // bytes of one tile of a plane: (ks, h, row) x 8 f16
constexpr int XB_PLANE = 4 * XB_TILE;                // 8192
constexpr int XB_THREADS = 256;
constexpr size_t XB_LDS = 8 * (size_t)XB_PLANE + 2 * XR * 3 * sizeof(double);

template <bool FLAT>
__global__ void __launch_bounds__(XB_THREADS, 2)
fringe_xpair_bwd_kernel(BwdArgs A)
{
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* g_img = smem;              // planes: 0 Ncc, 1 Ncs, 2 Nsc, 3 Nss (hi), 4..7 the same (lo)
    double* ant_lds = reinterpret_cast<double*>(smem + 8 * XB_PLANE);      // [128][3]: rows 0..63 group I, 64..127 group J

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int f = blockIdx.x % A.Nf, ts = blockIdx.x / A.Nf;
    const int t = ts / A.S, split = ts % A.S;
    const int rows_i = __builtin_amdgcn_readfirstlane(A.rows_i), rows_j = __builtin_amdgcn_readfirstlane(A.rows_j);

    const double nu_c = A.sign * A.freqs[f] * (1.0 / 2.99792458e8);
    for (int i = tid; i < 2 * XR * 3; i += XB_THREADS) {
        const int r = i / 3, k = i - 3 * r;
        const bool ok = r < XR ? r < rows_i : r - XR < rows_j;
        const int an = r < XR ? r : rows_i + (r - XR);
        ant_lds[i] = ok ? nu_c * A.antpos[3 * an + k] : 0.0;
    }
    const float gs = A.gscale[t * A.Nf + f] * 0.125f;
    const float* gre = A.gvt + ((size_t)t * A.Nf + f) * 2 * A.Nbl;
    const float* gim = gre + A.Nbl;
    // gradient with respect to V[r, c] of the virtual block (scalar adds: see keep_scalar)
    auto grad_of = [&](int r, int c, float& vr, float& vi) {
        vr = 0.f; vi = 0.f;
        gather_g<true>(gre, gim, A.pair_direct, A.pair_conj, r * NA + c, vr, vi);
    };
    for (int e = tid; e < 4 * 2 * 2 * 32 * 4; e += XB_THREADS) {
        const int jp = e & 3, row = (e >> 2) & 31, h = (e >> 7) & 1, ks = (e >> 8) & 1, tile = e >> 9;
        const int ti = tile >> 1, tj = tile & 1;
        const int i = 32 * ti + row;
        const int j0 = bwd_row_of_pair(tj, ks, jp, h);
        float ncc[2] = {0.f, 0.f}, ncs[2] = {0.f, 0.f}, nsc[2] = {0.f, 0.f}, nss[2] = {0.f, 0.f};
        if (i < rows_i) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int j = j0 + q;
                if (j < rows_j) {
                    float ar, ai, pr, pi, br, bi, qr, qi;
                    grad_of(i, j, ar, ai);                   // gA
                    grad_of(XR + i, XR + j, pr, pi);         // gA'
                    grad_of(XR + i, j, br, bi);              // gB
                    grad_of(i, XR + j, qr, qi);              // gB'
                    float sa = ar + pr; keep_scalar(sa);
                    float sb = br + qr; keep_scalar(sb);
                    float da = ai - pi; keep_scalar(da);
                    float db = bi - qi; keep_scalar(db);
                    ncc[q] = sa + sb; keep_scalar(ncc[q]);
                    nss[q] = sa - sb; keep_scalar(nss[q]);
                    ncs[q] = da + db; keep_scalar(ncs[q]);
                    nsc[q] = db - da; keep_scalar(nsc[q]);
                }
            }
        }
        uint32_t hi_, lo_;
        const int off = ((((tile * 2 + ks) * 2 + h) * 32 + row) * 4 + jp) * 4;
        float v0, v1;
        v0 = ncc[0] * gs; keep_scalar(v0); v1 = ncc[1] * gs; keep_scalar(v1);
        split2(v0, v1, hi_, lo_);
        *reinterpret_cast<uint32_t*>(g_img + 0 * XB_PLANE + off) = hi_; *reinterpret_cast<uint32_t*>(g_img + 4 * XB_PLANE + off) = lo_;
        v0 = ncs[0] * gs; keep_scalar(v0); v1 = ncs[1] * gs; keep_scalar(v1);
        split2(v0, v1, hi_, lo_);
        *reinterpret_cast<uint32_t*>(g_img + 1 * XB_PLANE + off) = hi_; *reinterpret_cast<uint32_t*>(g_img + 5 * XB_PLANE + off) = lo_;
        v0 = nsc[0] * gs; keep_scalar(v0); v1 = nsc[1] * gs; keep_scalar(v1);
        split2(v0, v1, hi_, lo_);
        *reinterpret_cast<uint32_t*>(g_img + 2 * XB_PLANE + off) = hi_; *reinterpret_cast<uint32_t*>(g_img + 6 * XB_PLANE + off) = lo_;
        v0 = nss[0] * gs; keep_scalar(v0); v1 = nss[1] * gs; keep_scalar(v1);
        split2(v0, v1, hi_, lo_);
        *reinterpret_cast<uint32_t*>(g_img + 3 * XB_PLANE + off) = hi_; *reinterpret_cast<uint32_t*>(g_img + 7 * XB_PLANE + off) = lo_;
    }
    __syncthreads();

    const double* sd = A.sdir + (size_t)t * 3 * A.Pstride;
    float* orow = A.gpsky + (size_t)t * A.st_t + (size_t)f * A.st_f;
    const float inv = 1.0f / gs;
    const int h = lane >> 5;
    const int ntile = A.Pstride / 32;
    const int tbeg = split * A.tiles_per_split;
    const int tend = min(ntile, tbeg + A.tiles_per_split);

    const uint32_t gl0 = (h * 32 + (lane & 31)) * 16;
    for (int pt = tbeg + wave; pt < tend; pt += XB_THREADS / 64) {
        const int p = pt * 32 + (lane & 31);                     // < Pstride: pt < ntile
        double sx, sy, sz;
        load_dir<FLAT>(sd, A.Pstride, p, sx, sy, sz);
        f32x16 accC[2], accS[2];                                 // T1 = Ncc Cy + Ncs Sy,  T2 = Nsc Cy + Nss Sy, per row tile of I
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int e = 0; e < 16; ++e) { accC[q][e] = 0.f; accS[q][e] = 0.f; }
        // phasors of the eight rows base + (jj & 3) + 8 (jj >> 2) + 4 h of ant_lds, jj = 0..7
        auto phasors8 = [&](int base, int live_rows, float* ec, float* es) {
#pragma unroll
            for (int jq = 0; jq < 2; ++jq) {
                if (8 * jq >= live_rows) {                       // uniform: 8 padding rows
#pragma unroll
                    for (int u = 0; u < 4; ++u) { ec[4 * jq + u] = 0.f; es[4 * jq + u] = 0.f; }
                    continue;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int an = base + u + 8 * jq + 4 * h;
                    const double ph = phase_of<FLAT>(ant_lds[3 * an], sx, ant_lds[3 * an + 1], sy, ant_lds[3 * an + 2], sz);
                    const float rr = turn_frac(ph);
                    ec[4 * jq + u] = __builtin_amdgcn_cosf(rr);
                    es[4 * jq + u] = __builtin_amdgcn_sinf(rr);
                }
            }
        };
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int j0 = 32 * tj + 16 * ks;
                if (j0 >= rows_j) continue;                      // uniform: 16 padding rows (their N columns are zero)
                float ec[8], es[8];
                phasors8(XR + j0, rows_j - j0, ec, es);
                uint4 Erh, Erl, Eih, Eil;
                uint32_t* erh = reinterpret_cast<uint32_t*>(&Erh); uint32_t* erl = reinterpret_cast<uint32_t*>(&Erl);
                uint32_t* eih = reinterpret_cast<uint32_t*>(&Eih); uint32_t* eil = reinterpret_cast<uint32_t*>(&Eil);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    split2_plain(ec[2 * q], ec[2 * q + 1], erh[q], erl[q]);
                    split2_plain(es[2 * q], es[2 * q + 1], eih[q], eil[q]);
                }
#pragma unroll
                for (int ti = 0; ti < 2; ++ti) {
                    if (32 * ti >= rows_i) continue;             // uniform
                    const int tk = (2 * ti + tj) * XB_TILE + ks * 1024;
                    const uint4 Icc_h = *reinterpret_cast<const uint4*>(g_img + gl0 + 0 * XB_PLANE + tk);
                    const uint4 Ics_h = *reinterpret_cast<const uint4*>(g_img + gl0 + 1 * XB_PLANE + tk);
                    const uint4 Isc_h = *reinterpret_cast<const uint4*>(g_img + gl0 + 2 * XB_PLANE + tk);
                    const uint4 Iss_h = *reinterpret_cast<const uint4*>(g_img + gl0 + 3 * XB_PLANE + tk);
                    const uint4 Icc_l = *reinterpret_cast<const uint4*>(g_img + gl0 + 4 * XB_PLANE + tk);
                    const uint4 Ics_l = *reinterpret_cast<const uint4*>(g_img + gl0 + 5 * XB_PLANE + tk);
                    const uint4 Isc_l = *reinterpret_cast<const uint4*>(g_img + gl0 + 6 * XB_PLANE + tk);
                    const uint4 Iss_l = *reinterpret_cast<const uint4*>(g_img + gl0 + 7 * XB_PLANE + tk);
                    accC[ti] = RIME_MFMA(Icc_h, Erh, accC[ti]);
                    accS[ti] = RIME_MFMA(Isc_h, Erh, accS[ti]);
                    accC[ti] = RIME_MFMA(Ics_h, Eih, accC[ti]);
                    accS[ti] = RIME_MFMA(Iss_h, Eih, accS[ti]);
                    accC[ti] = RIME_MFMA(Icc_h, Erl, accC[ti]);
                    accS[ti] = RIME_MFMA(Isc_h, Erl, accS[ti]);
                    accC[ti] = RIME_MFMA(Ics_h, Eil, accC[ti]);
                    accS[ti] = RIME_MFMA(Iss_h, Eil, accS[ti]);
                    accC[ti] = RIME_MFMA(Icc_l, Erh, accC[ti]);
                    accS[ti] = RIME_MFMA(Isc_l, Erh, accS[ti]);
                    accC[ti] = RIME_MFMA(Ics_l, Eih, accC[ti]);
                    accS[ti] = RIME_MFMA(Iss_l, Eih, accS[ti]);
                }
            }
        }
        // contraction with the phasors of group I: accumulator element e of row tile ti is row 32 ti + (e & 3) + 8 (e >> 2) + 4 h
        RIME_MFMA_SETTLE();
        float part = 0.f;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
            if (32 * ti >= rows_i) continue;                     // uniform
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int i0 = 32 * ti + 16 * ks;
                if (i0 >= rows_i) continue;                      // uniform: rows of N that are zero
                float ec[8], es[8];
                phasors8(i0, rows_i - i0, ec, es);
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    part = fmaf(ec[jj], accC[ti][8 * ks + jj], part); keep_scalar(part);
                    part = fmaf(es[jj], accS[ti][8 * ks + jj], part); keep_scalar(part);
                }
            }
        }
        part += __shfl_xor(part, 32, 64);
        if (h == 0) {
            float* o = orow + (size_t)p * A.st_p;
            *o = A.accumulate ? *o + part * inv : part * inv;
        }
    }
}

static bool common_ok(int rows_i, int rows_j, int Nbl, int Nt, int Nf, int Pstride, long long st_p, int sign)
{
    if (rows_i <= 0 || rows_i > XR || rows_j <= 0 || rows_j > XR) return false;
    if (st_p != 1 && st_p != 2) return false;                      // 2: one plane of a complex buffer
    if (Nbl <= 0 || Nt <= 0 || Nt > 65535 || Nf <= 0 || Pstride <= 0 || Pstride % 64 != 0) return false;
    return sign == 1 || sign == -1;
}

} // namespace xp
} // namespace rime

using namespace rime;

extern "C" int rime_fringe_pair_cross_fwd_block(const double* antpos, int rows_i, int rows_j, int flat, const double* sdir,
                                                const double* freqs, const float* psky, const float* scale, const float* rowmin,
                                                const int* pair_direct, const int* pair_conj, int Nbl, int Nt, int Nf, int Pstride,
                                                long long st_t, long long st_f, long long st_p, int sign,
                                                void* workspace, size_t workspace_bytes, void* stream)
{
    if (!antpos || !sdir || !freqs || !psky || !scale || !pair_direct || !pair_conj) return RIME_EINVAL;
    if (!xp::common_ok(rows_i, rows_j, Nbl, Nt, Nf, Pstride, st_p, sign)) return RIME_EINVAL;
    if (!workspace || workspace_bytes < fwd_workspace_bytes(Nbl, Nt, Nf, Pstride)) return RIME_EWORKSPACE;
    xp::FwdArgs A{};
    fill_geometry(A, antpos, sdir, freqs, pair_direct, pair_conj, Nbl, Nt, Nf, Pstride, st_t, st_f, st_p, sign);
    const dim3 grid = fill_forward(A, psky, scale, rowmin, workspace);
    A.rows_i = rows_i; A.rows_j = rows_j;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    with_bool(flat != 0, [&](auto FLAT) {
        launch_real_plane(xp::fringe_xpair_fwd_kernel<true, FLAT()>, xp::fringe_xpair_fwd_kernel<false, FLAT()>, grid, 256,
                          xp::FWD_LDS, st, A);
    });
    return check_launch();
}

extern "C" int rime_fringe_pair_cross_bwd_block(const double* antpos, int rows_i, int rows_j, int flat, const double* sdir,
                                                const double* freqs, const float* gscale, const int* pair_direct,
                                                const int* pair_conj, int Nbl, int Nt, int Nf, int Pstride,
                                                long long st_t, long long st_f, long long st_p, int sign, int accumulate,
                                                float* gpsky, const void* workspace, size_t workspace_bytes, void* stream)
{
    if (!antpos || !sdir || !freqs || !gscale || !pair_direct || !pair_conj || !gpsky) return RIME_EINVAL;
    if (!xp::common_ok(rows_i, rows_j, Nbl, Nt, Nf, Pstride, st_p, sign)) return RIME_EINVAL;
    if (!workspace || workspace_bytes < rime_fringe_ant_bwd_workspace(Nbl, Nt, Nf)) return RIME_EWORKSPACE;
    xp::BwdArgs A{};
    fill_geometry(A, antpos, sdir, freqs, pair_direct, pair_conj, Nbl, Nt, Nf, Pstride, st_t, st_f, st_p, sign);
    const dim3 grid = fill_backward(A, gscale, gpsky, workspace, accumulate);
    A.rows_i = rows_i; A.rows_j = rows_j;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    with_bool(flat != 0, [&](auto FLAT) {
        hipLaunchKernelGGL(xp::fringe_xpair_bwd_kernel<FLAT()>, grid, dim3(xp::XB_THREADS), xp::XB_LDS, st, A);
    });
    return check_launch();
}
