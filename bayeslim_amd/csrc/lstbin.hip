// lstbin.hip -- LST alignment of drift-scan visibilities (telescope_model.vis_rephase, VisData.lst_rephase / time_nn_interp /
// time_average; reference dataset.py:1363-1566, telescope_model.py:594-645): the rephasing phasor, the weighting and the
// average of the integrations of every bin in ONE pass.  For every (pol entry p, baseline b, bin k, channel f), over the
// members m of the bin (table positions bin_ptr[k] ... bin_ptr[k + 1] - 1, t = members[m]) IN TABLE ORDER:
//     sum_w    = sum_m w[p, b, t, f]                                                        (w = 1 without weights)
//     avg      = sum_m w V[p, b, t, f] exp(2 pi i nu_f tau[b, j]) / max(sum_w, 1e-40)        (V = 1 without data: the phasor)
//     avg_cov  = sum_m w^2 cov[p, b, t, f] / max(sum_w, 1e-40)^2
//     avg_flag = every member flagged
// with j = t, or j = m when tau has one column per table position (a time that serves several bins with different delays:
// nearest-neighbour interpolation).  The reference makes a phasor tensor of the data's size, a product, three index_add_
// passes (atomic scatters on the GPU), a fourth for the flags and two divisions.
// Phase: nu tau in float64, reduced to [-1/2, 1/2] turns in float64, THEN sine and cosine in the working precision T (as
// the fringe kernels, fringe.hip; rephasing phases reach tens of turns).  Sums in T, one chain per output element, ascending
// table position: no atomics, no communication between lanes, the bits are a function of the inputs and the table alone.
//
// Layout: a lane owns TA_BYTES = 16 bytes of a real row = CH = 16 / sizeof(T) consecutive channels (4 in float32, 2 in float64)
// of one (p, b, k): 32 bytes of data, 16 of weights and of variances, CH flag bytes per member.  Consecutive lanes take
// consecutive channel groups, then the next bin / baseline / pol entry (the flat index runs over [p][b][k][channel group]),
// so a work-group of 256 lanes spans 256 CH channels and short channel axes are filled up with further rows.  A launch
// whose tensors all have 16-byte aligned bases, with Nf a multiple of CH (every row then starts aligned), reads and writes
// with 16-byte accesses (the VEC instantiation, chosen on the host); any other takes element accesses (the contiguous-row
// layout of lane_vec.h): the bits do not depend on alignment.  Flags are bytes, read and written one by one.
//
// Backward (data only): gV[p, b, t, f] = sum over the table positions m that hold t (transposed table, built on the host,
// ascending m) of  w[p, b, t, f] conj(phasor) g_avg[p, b, k(m), f] / max(sum_w[p, b, k(m), f], 1e-40),  one lane per
// (p, b, t, channel group), every element of gV written once (0 for a time in no bin).  Weights, tau and cov get no gradient.
// Table entries are clamped / skipped in the kernels, never followed outside the tensors; the host checks them beforehand.
// Vector ALU only.
#include "lane_vec.h"
#include <initializer_list>

namespace rime {

constexpr int TA_THREADS = 256, TA_BYTES = 16, TA_MAXBLOCKS = 1 << 20;

// the 16-byte form serves a launch whose rows all start on 16 bytes: every tensor given has an aligned base (null counts as
// aligned) and Nf is a multiple of CH
static bool ta_vec(int dtype, long long Nf, std::initializer_list<const void*> ptrs)
{
    if (Nf % (TA_BYTES / real_bytes(dtype)) != 0) return false;
    for (const void* p : ptrs)
        if (!aligned16(p)) return false;
    return true;
}

// sine and cosine of nu * tau turns: the product and its reduction to [-1/2, 1/2] in float64, the functions in T.  The
// fraction is fma(nu, tau, -rint(nu * tau)), written out so that -ffp-contract has nothing left to decide: every
// instantiation computes the same bits (a contracted and an uncontracted ph - rint(ph) differ by an ulp of the phase)
__device__ __forceinline__ double ta_fraction(double nu, double tau)
{
    return fma(nu, tau, -rint(nu * tau));
}

__device__ __forceinline__ void ta_phasor(double nu, double tau, float& s, float& c)
{
    const float r = (float)ta_fraction(nu, tau);
    s = __builtin_amdgcn_sinf(r);                       // the hardware functions take revolutions (fringe.hip, sincos_turns)
    c = __builtin_amdgcn_cosf(r);
}

__device__ __forceinline__ void ta_phasor(double nu, double tau, double& s, double& c)
{
    sincospi(2.0 * ta_fraction(nu, tau), &s, &c);
}

// (xr + i xi) (c + i sgn s), one product and one fused multiply-add per part, the same in every instantiation
template <typename T>
__device__ __forceinline__ void ta_rotate(T& xr, T& xi, T s, T c, bool conj)
{
    const T sr = conj ? -s : s;
    const T zr = tfma<T>(xr, c, -(xi * sr)), zi = tfma<T>(xr, sr, xi * c);
    xr = zr; xi = zi;
}

struct LstBinArgs {
    const void* data; const void* wgts; const void* cov; const unsigned char* flags;     // [Npp, Nbl, Nt, Nf]; each may be null
    const double* tau; const double* freqs;                    // [Nbl, Ntau] (Ntau = Nmem when by_member, else Nt) or null; [Nf]
    const int* bin_ptr; const int* members;                    // forward CSR: [Nbin + 1], [Nmem]
    const int* t_ptr; const int* t_pos;                        // backward CSR: [Nt + 1], [Nmem] table positions of every time
    const int* pos_bin;                                        // [Nmem] bin of every table position (backward)
    void* avg; void* sum_w; void* avg_cov; unsigned char* avg_flag;                       // [Npp, Nbl, Nbin, Nf]
    const void* gavg; void* gdata;                             // backward: [Npp, Nbl, Nbin, Nf] in, [Npp, Nbl, Nt, Nf] out
    int by_member;
    long long Npp, Nbl, Nt, Nf, Nbin, Nmem;
};

template <typename T, bool VEC>
__global__ __launch_bounds__(TA_THREADS) void vis_timeavg_fwd_kernel(LstBinArgs A)
{
    constexpr int CH = TA_BYTES / sizeof(T);
    const T* data = reinterpret_cast<const T*>(A.data);
    const T* wgts = reinterpret_cast<const T*>(A.wgts);
    const T* cov = reinterpret_cast<const T*>(A.cov);
    T* avg = reinterpret_cast<T*>(A.avg);
    T* sum_w = reinterpret_cast<T*>(A.sum_w);
    T* avg_cov = reinterpret_cast<T*>(A.avg_cov);
    constexpr bool d_vec = VEC, w_vec = VEC, c_vec = VEC, a_vec = VEC, s_vec = VEC, ac_vec = VEC;
    const size_t nfg = (size_t)((A.Nf + CH - 1) / CH);
    const size_t total = (size_t)A.Npp * A.Nbl * A.Nbin * nfg;
    const size_t Ntau = (size_t)(A.by_member ? A.Nmem : A.Nt);
    for (size_t i = (size_t)blockIdx.x * TA_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * TA_THREADS) {
        const size_t fg = i % nfg, row = i / nfg;              // row = (p * Nbl + b) * Nbin + k
        const size_t k = row % (size_t)A.Nbin, pb = row / (size_t)A.Nbin, b = pb % (size_t)A.Nbl;
        const long long f0 = (long long)fg * CH;
        const int nvalid = (int)std::min<long long>(CH, A.Nf - f0);
        const long long m0 = std::max<long long>(A.bin_ptr[k], 0), m1 = std::min<long long>(A.bin_ptr[k + 1], A.Nmem);
        double nu[CH];
        if (A.tau != nullptr) {
#pragma unroll
            for (int c = 0; c < CH; ++c) nu[c] = c < nvalid ? A.freqs[f0 + c] : 0.0;
        }
        T are[CH], aim[CH], sw[CH], ac[CH];
        bool fl[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) { are[c] = (T)0; aim[c] = (T)0; sw[c] = (T)0; ac[c] = (T)0; fl[c] = true; }
        for (long long m = m0; m < m1; ++m) {
            const int t = A.members[m];
            if ((unsigned)t >= (unsigned)A.Nt) continue;
            const size_t e = (pb * (size_t)A.Nt + (size_t)t) * (size_t)A.Nf + (size_t)f0;
            T v[2 * CH], w[CH];
            if (data != nullptr) {
                row_load<T, 2 * CH>(data, 2 * e, 2 * nvalid, d_vec, v);
            } else {
#pragma unroll
                for (int c = 0; c < CH; ++c) { v[2 * c] = (T)1; v[2 * c + 1] = (T)0; }
            }
            if (wgts != nullptr) {
                row_load<T, CH>(wgts, e, nvalid, w_vec, w);
            } else {
#pragma unroll
                for (int c = 0; c < CH; ++c) w[c] = (T)1;
            }
            if (A.tau != nullptr) {
                const double tau = A.tau[b * Ntau + (size_t)(A.by_member ? m : (long long)t)];
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    T s, co;
                    ta_phasor(nu[c], tau, s, co);
                    ta_rotate<T>(v[2 * c], v[2 * c + 1], s, co, false);
                }
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                are[c] = tfma<T>(w[c], v[2 * c], are[c]);
                aim[c] = tfma<T>(w[c], v[2 * c + 1], aim[c]);
                sw[c] += w[c];
            }
            if (cov != nullptr) {
                T cv[CH];
                row_load<T, CH>(cov, e, nvalid, c_vec, cv);
#pragma unroll
                for (int c = 0; c < CH; ++c) ac[c] = tfma<T>(w[c] * w[c], cv[c], ac[c]);
            }
            if (A.flags != nullptr) {
#pragma unroll
                for (int c = 0; c < CH; ++c)
                    if (c < nvalid) fl[c] = fl[c] && A.flags[e + c] != 0;
            }
        }
        const size_t o = row * (size_t)A.Nf + (size_t)f0;
        T out[2 * CH], oc[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const T d = sw[c] > (T)1e-40 ? sw[c] : (T)1e-40;
            out[2 * c] = are[c] / d; out[2 * c + 1] = aim[c] / d;
            oc[c] = ac[c] / (d * d);
        }
        row_store<T, 2 * CH>(avg, 2 * o, 2 * nvalid, a_vec, out);
        if (sum_w != nullptr) row_store<T, CH>(sum_w, o, nvalid, s_vec, sw);
        if (avg_cov != nullptr) row_store<T, CH>(avg_cov, o, nvalid, ac_vec, oc);
        if (A.avg_flag != nullptr) {
#pragma unroll
            for (int c = 0; c < CH; ++c)
                if (c < nvalid) A.avg_flag[o + c] = fl[c] ? 1 : 0;
        }
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(TA_THREADS) void vis_timeavg_bwd_kernel(LstBinArgs A)
{
    constexpr int CH = TA_BYTES / sizeof(T);
    const T* gavg = reinterpret_cast<const T*>(A.gavg);
    const T* wgts = reinterpret_cast<const T*>(A.wgts);
    const T* sum_w = reinterpret_cast<const T*>(A.sum_w);
    T* gdata = reinterpret_cast<T*>(A.gdata);
    constexpr bool g_vec = VEC, w_vec = VEC, s_vec = VEC, o_vec = VEC;
    const size_t nfg = (size_t)((A.Nf + CH - 1) / CH);
    const size_t total = (size_t)A.Npp * A.Nbl * A.Nt * nfg;
    const size_t Ntau = (size_t)(A.by_member ? A.Nmem : A.Nt);
    for (size_t i = (size_t)blockIdx.x * TA_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * TA_THREADS) {
        const size_t fg = i % nfg, row = i / nfg;              // row = (p * Nbl + b) * Nt + t
        const size_t t = row % (size_t)A.Nt, pb = row / (size_t)A.Nt, b = pb % (size_t)A.Nbl;
        const long long f0 = (long long)fg * CH;
        const int nvalid = (int)std::min<long long>(CH, A.Nf - f0);
        const long long q0 = std::max<long long>(A.t_ptr[t], 0), q1 = std::min<long long>(A.t_ptr[t + 1], A.Nmem);
        const size_t e = row * (size_t)A.Nf + (size_t)f0;
        double nu[CH];
        if (A.tau != nullptr) {
#pragma unroll
            for (int c = 0; c < CH; ++c) nu[c] = c < nvalid ? A.freqs[f0 + c] : 0.0;
        }
        T w[CH], acc[2 * CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) { w[c] = (T)1; acc[2 * c] = (T)0; acc[2 * c + 1] = (T)0; }
        if (wgts != nullptr && q1 > q0) row_load<T, CH>(wgts, e, nvalid, w_vec, w);
        for (long long q = q0; q < q1; ++q) {
            const int m = A.t_pos[q];
            if ((unsigned)m >= (unsigned)A.Nmem) continue;
            const int k = A.pos_bin[m];
            if ((unsigned)k >= (unsigned)A.Nbin) continue;
            const size_t o = (pb * (size_t)A.Nbin + (size_t)k) * (size_t)A.Nf + (size_t)f0;
            T g[2 * CH], sw[CH];
            row_load<T, 2 * CH>(gavg, 2 * o, 2 * nvalid, g_vec, g);
            row_load<T, CH>(sum_w, o, nvalid, s_vec, sw);
            double tau = 0.0;
            if (A.tau != nullptr) tau = A.tau[b * Ntau + (A.by_member ? (size_t)m : t)];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const T d = sw[c] > (T)1e-40 ? sw[c] : (T)1e-40;
                const T coef = w[c] / d;
                T gr = g[2 * c], gi = g[2 * c + 1];
                if (A.tau != nullptr) {                        // conj(phasor) * g
                    T s, co;
                    ta_phasor(nu[c], tau, s, co);
                    ta_rotate<T>(gr, gi, s, co, true);
                }
                acc[2 * c] = tfma<T>(coef, gr, acc[2 * c]);
                acc[2 * c + 1] = tfma<T>(coef, gi, acc[2 * c + 1]);
            }
        }
        row_store<T, 2 * CH>(gdata, 2 * e, 2 * nvalid, o_vec, acc);
    }
}

static int ta_blocks(long long rows, long long Nf, int dtype)
{
    const long long ch = TA_BYTES / real_bytes(dtype);
    const long long items = rows * ((Nf + ch - 1) / ch);
    return (int)std::min<long long>((items + TA_THREADS - 1) / TA_THREADS, TA_MAXBLOCKS);
}

// sizes: non-negative, and the element counts of the tensors fit in 62 bits
static bool ta_sizes_ok(long long Npp, long long Nbl, long long Nt, long long Nf, long long Nbin, long long Nmem)
{
    if (Npp < 0 || Nbl < 0 || Nt < 0 || Nf < 0 || Nbin < 0 || Nmem < 0) return false;
    const long double lim = 4.0e18L;
    return (long double)Npp * Nbl * std::max(Nt, Nbin) * Nf < lim && (long double)Nbl * std::max(Nt, Nmem) < lim;
}

// a host CSR table: ptr [n + 1] from 0, non-decreasing, ending at nmem; idx [nmem] in [0, bound)
static bool ta_table_ok(const int* ptr, long long n, const int* idx, long long nmem, long long bound)
{
    if (ptr[0] != 0) return false;
    for (long long i = 0; i < n; ++i)
        if (ptr[i + 1] < ptr[i]) return false;
    if (ptr[n] != nmem) return false;
    for (long long m = 0; m < nmem; ++m)
        if (idx[m] < 0 || idx[m] >= bound) return false;
    return true;
}

} // namespace rime

using namespace rime;

extern "C" int rime_vis_timeavg_fwd(int dtype, const void* data, const void* wgts, const void* cov, const void* flags,
                                    const double* tau, int tau_by_member, const double* freqs, const int* bin_ptr,
                                    const int* members, const int* bin_ptr_host, const int* members_host, int Npp, int Nbl,
                                    int Nt, int Nf, int Nbin, int Nmem, void* avg, void* sum_w, void* avg_cov, void* avg_flag,
                                    void* stream)
{
    if (!real_dtype_ok(dtype)) return RIME_EINVAL;
    if (!ta_sizes_ok(Npp, Nbl, Nt, Nf, Nbin, Nmem)) return RIME_EINVAL;
    if (tau_by_member != 0 && tau_by_member != 1) return RIME_EINVAL;
    if (!avg || !bin_ptr || !bin_ptr_host || (Nmem > 0 && (!members || !members_host))) return RIME_EINVAL;
    if (tau != nullptr && !freqs) return RIME_EINVAL;
    if ((cov != nullptr) != (avg_cov != nullptr) || (flags != nullptr) != (avg_flag != nullptr)) return RIME_EINVAL;
    if (!ta_table_ok(bin_ptr_host, Nbin, members_host, Nmem, Nt)) return RIME_EINVAL;
    const int nb = ta_blocks((long long)Npp * Nbl * Nbin, Nf, dtype);
    if (nb == 0) return RIME_OK;                               // an empty output
    LstBinArgs A{};
    A.data = data; A.wgts = wgts; A.cov = cov; A.flags = (const unsigned char*)flags; A.tau = tau; A.freqs = freqs;
    A.bin_ptr = bin_ptr; A.members = members; A.avg = avg; A.sum_w = sum_w; A.avg_cov = avg_cov;
    A.avg_flag = (unsigned char*)avg_flag; A.by_member = tau_by_member;
    A.Npp = Npp; A.Nbl = Nbl; A.Nt = Nt; A.Nf = Nf; A.Nbin = Nbin; A.Nmem = Nmem;
    const bool vec = ta_vec(dtype, Nf, {data, wgts, cov, avg, sum_w, avg_cov});
    return with_real(dtype, [&](auto t) {
        with_bool(vec, [&](auto v) {
            hipLaunchKernelGGL((vis_timeavg_fwd_kernel<decltype(t), v.value>), dim3(nb), dim3(TA_THREADS), 0, as_stream(stream), A);
        });
        return check_launch();
    });
}

extern "C" int rime_vis_timeavg_bwd(int dtype, const void* gavg, const void* wgts, const void* sum_w, const double* tau,
                                    int tau_by_member, const double* freqs, const int* t_ptr, const int* t_pos,
                                    const int* pos_bin, const int* t_ptr_host, const int* t_pos_host, const int* pos_bin_host,
                                    int Npp, int Nbl, int Nt, int Nf, int Nbin, int Nmem, void* gdata, void* stream)
{
    if (!real_dtype_ok(dtype)) return RIME_EINVAL;
    if (!ta_sizes_ok(Npp, Nbl, Nt, Nf, Nbin, Nmem)) return RIME_EINVAL;
    if (tau_by_member != 0 && tau_by_member != 1) return RIME_EINVAL;
    if (!gavg || !sum_w || !gdata || !t_ptr || !t_ptr_host) return RIME_EINVAL;
    if (Nmem > 0 && (!t_pos || !pos_bin || !t_pos_host || !pos_bin_host)) return RIME_EINVAL;
    if (tau != nullptr && !freqs) return RIME_EINVAL;
    if (!ta_table_ok(t_ptr_host, Nt, t_pos_host, Nmem, Nmem)) return RIME_EINVAL;
    for (long long m = 0; m < Nmem; ++m)
        if (pos_bin_host[m] < 0 || pos_bin_host[m] >= Nbin) return RIME_EINVAL;
    const int nb = ta_blocks((long long)Npp * Nbl * Nt, Nf, dtype);
    if (nb == 0) return RIME_OK;
    LstBinArgs A{};
    A.gavg = gavg; A.wgts = wgts; A.sum_w = const_cast<void*>(sum_w); A.tau = tau; A.freqs = freqs;
    A.t_ptr = t_ptr; A.t_pos = t_pos; A.pos_bin = pos_bin; A.gdata = gdata; A.by_member = tau_by_member;
    A.Npp = Npp; A.Nbl = Nbl; A.Nt = Nt; A.Nf = Nf; A.Nbin = Nbin; A.Nmem = Nmem;
    const bool vec = ta_vec(dtype, Nf, {gavg, wgts, sum_w, gdata});
    return with_real(dtype, [&](auto t) {
        with_bool(vec, [&](auto v) {
            hipLaunchKernelGGL((vis_timeavg_bwd_kernel<decltype(t), v.value>), dim3(nb), dim3(TA_THREADS), 0, as_stream(stream), A);
        });
        return check_launch();
    });
}
