// fft.hip -- batched 1-D complex DFT along the last axis with the window, the shifts, the norm and the reference's
// abs / peak-normalise / square / peak-delay epilogues fused into ONE launch (reference fft.py:99-202).
//
// One work-group of 256 threads transforms L lines of N samples (L a power of two, L N <= 1024 where N allows; G = 256 / L
// threads per line).  A line lives in LDS from its load to its store: load (ifftshift folded into the index, window),
// Stockham autosort passes between two ping-pong images, store (norm, fftshift folded into the index, epilogue).
//
// Pass with radix r after sub-transforms of length Ns (Ns = product of the earlier radices), M = N / r butterflies:
//     j < M, k = j mod Ns:   v_q = in[j + q M] * tw[q k N / (Ns r)]          q < r
//                            out[(j - k) r + k + m Ns] = sum_q v_q * exp(-+2 pi i q m / r)     m < r
// Reads are contiguous in j.  Writes have stride r elements in the first pass (Ns = 1): the images are padded by one element
// per 128 B (the modulus of the store banking), which spreads a 16-lane store group over all banks; a line's padded length
// is odd so that the lines a wave holds at small N start on different banks.
// Radices 2, 3, 4, 5 are written out; any other radix runs as N independent r-term sums (one per OUTPUT, accumulated as it
// goes, twiddle and root of unity merged into one table index that advances by a fixed step), slow only in proportion to r.
// Twiddles come from the caller's table exp(-+2 pi i j / N); the kernel evaluates no sine or cosine.
// Every output element is written by exactly one thread, all sums run in a fixed order, no atomics: bit-reproducible.
#include "rime_common.h"

namespace rime {

constexpr int FFT_MAXN = 4096, FFT_MAXPASS = 12, FFT_THREADS = 256, FFT_LINE_ELEMS = 1024;
enum { FFT_ABS = 1, FFT_PEAKNORM = 2, FFT_SQUARE = 4, FFT_PEAK = 8 };

struct FftPasses { int n; int radix[FFT_MAXPASS]; };

template <typename T> struct Cx;
template <> struct Cx<float>  { using type = float2;  static constexpr int PSH = 4; };   // 16 x 8 B  = 128 B
template <> struct Cx<double> { using type = double2; static constexpr int PSH = 3; };   //  8 x 16 B = 128 B

template <typename T> __host__ __device__ __forceinline__ int fft_pidx(int i) { return i + (i >> Cx<T>::PSH); }
// padded, odd length of one line image
template <typename T> static int fft_line_stride(int N) { return (fft_pidx<T>(N - 1) + 1) | 1; }
static int fft_lines_per_group(int N)
{
    int L = 1;
    while (L < FFT_THREADS && 2 * L * N <= FFT_LINE_ELEMS) L *= 2;
    return L;
}

template <typename C> __device__ __forceinline__ C cmul(C a, C b) { return C{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
template <typename C> __device__ __forceinline__ C cadd(C a, C b) { return C{a.x + b.x, a.y + b.y}; }
template <typename C> __device__ __forceinline__ C csub(C a, C b) { return C{a.x - b.x, a.y - b.y}; }
// (sgn i) a
template <typename C, typename T> __device__ __forceinline__ C crot(C a, T sgn) { return C{-sgn * a.y, sgn * a.x}; }

// t / d for 0 <= t < 2^22, 1 <= d <= 4096 with inv = 1 / d rounded: (t + 1/2) / d is at least 1/(2 t) (relative) away from
// an integer, far above the two roundings; the correction keeps it exact whatever the rounding does
__device__ __forceinline__ int fft_div(int t, int d, float inv)
{
    int q = (int)(((float)t + 0.5f) * inv);
    const int r = t - q * d;
    if (r < 0) --q; else if (r >= d) ++q;
    return q;
}

template <typename T> __device__ __forceinline__ T tsqrt(T a);
template <> __device__ __forceinline__ float tsqrt<float>(float a) { return sqrtf(a); }
template <> __device__ __forceinline__ double tsqrt<double>(double a) { return sqrt(a); }
template <typename T> __device__ __forceinline__ T tlog(T a);
template <> __device__ __forceinline__ float tlog<float>(float a) { return logf(a); }
template <> __device__ __forceinline__ double tlog<double>(double a) { return log(a); }

// Quinn's second estimator: the correction term k() of the reference (fft.py:154-157)
template <typename T> __device__ __forceinline__ T quinn_k(T x)
{
    const T s23 = (T)0.81649658092772603273;          // sqrt(2/3)
    const T c = (T)0.10206207261596575409;            // sqrt(6) / 24
    return (T)0.25 * tlog<T>((T)3 * x * x + (T)6 * x + (T)1) - c * tlog<T>((x + (T)1 - s23) / (x + (T)1 + s23));
}

// the reference's chain abs -> peaknorm -> square on one sample (fft.py:128-135); re is the value when the result is real
template <typename T, typename C> __device__ __forceinline__ void fft_chain(C& v, T& re, int epi, T m)
{
    bool real = false;
    if (epi & FFT_ABS) { re = tsqrt<T>(v.x * v.x + v.y * v.y); real = true; }
    if (epi & FFT_PEAKNORM) { if (real) re = re / m; else { v.x = v.x / m; v.y = v.y / m; } }
    if (epi & FFT_SQUARE) re = real ? re * re : v.x * v.x + v.y * v.y;
}

template <typename T>
__global__ __launch_bounds__(FFT_THREADS) void fft_kernel(const T* __restrict__ x, const T* __restrict__ tw_, const T* __restrict__ win,
                                                          int win_store, FftPasses P, int N, long long nlines, int lgL, int LS, T sgn,
                                                          int sh_in, int sh_out, T scale, int epi, double start, double df,
                                                          T* __restrict__ y)
{
    using C = typename Cx<T>::type;
    extern __shared__ __align__(16) unsigned char smem[];
    const int L = 1 << lgL, lgG = 8 - lgL, G = 1 << lgG;
    const int tid = threadIdx.x, g = tid & (G - 1), ll = tid >> lgG;
    C* a = reinterpret_cast<C*>(smem) + (size_t)ll * LS;
    C* b = a + (size_t)L * LS;
    T* rv = reinterpret_cast<T*>(reinterpret_cast<C*>(smem) + (size_t)2 * L * LS);
    int* ri = reinterpret_cast<int*>(rv + FFT_THREADS);
    const C* tw = reinterpret_cast<const C*>(tw_);
    const long long line = (long long)blockIdx.x * L + ll;
    const bool live = line < nlines;

    // ---- load: X[k] = w[src] x[src], src = (k + sh_in) mod N
    if (live) {
        const C* xl = reinterpret_cast<const C*>(x) + (size_t)line * N;
        const bool wl = win != nullptr && !win_store;
        for (int k = g; k < N; k += G) {
            int src = k + sh_in;
            if (src >= N) src -= N;
            C v = xl[src];
            if (wl) { const T w = win[src]; v.x *= w; v.y *= w; }
            a[fft_pidx<T>(k)] = v;
        }
    }
    __syncthreads();

    // ---- Stockham passes
    int Ns = 1;
    for (int p = 0; p < P.n; ++p) {
        const int r = P.radix[p];
        const int M = N / r, ts = M / Ns;               // butterflies per line; twiddle index step N / (Ns r)
        const float invNs = 1.0f / (float)Ns;
        const bool twd = Ns > 1;
        if (live) {
            if (r == 4) {
                for (int j = g; j < M; j += G) {
                    const int k = j - fft_div(j, Ns, invNs) * Ns, jo = (j - k) * 4 + k;
                    C v0 = a[fft_pidx<T>(j)], v1 = a[fft_pidx<T>(j + M)], v2 = a[fft_pidx<T>(j + 2 * M)], v3 = a[fft_pidx<T>(j + 3 * M)];
                    if (twd) { v1 = cmul(v1, tw[k * ts]); v2 = cmul(v2, tw[2 * k * ts]); v3 = cmul(v3, tw[3 * k * ts]); }
                    const C t0 = cadd(v0, v2), t1 = csub(v0, v2), t2 = cadd(v1, v3), t3 = crot(csub(v1, v3), sgn);
                    b[fft_pidx<T>(jo)] = cadd(t0, t2);
                    b[fft_pidx<T>(jo + Ns)] = cadd(t1, t3);
                    b[fft_pidx<T>(jo + 2 * Ns)] = csub(t0, t2);
                    b[fft_pidx<T>(jo + 3 * Ns)] = csub(t1, t3);
                }
            } else if (r == 2) {
                for (int j = g; j < M; j += G) {
                    const int k = j - fft_div(j, Ns, invNs) * Ns, jo = (j - k) * 2 + k;
                    C v0 = a[fft_pidx<T>(j)], v1 = a[fft_pidx<T>(j + M)];
                    if (twd) v1 = cmul(v1, tw[k * ts]);
                    b[fft_pidx<T>(jo)] = cadd(v0, v1);
                    b[fft_pidx<T>(jo + Ns)] = csub(v0, v1);
                }
            } else if (r == 3) {
                const T h3 = (T)0.86602540378443864676;                  // sqrt(3) / 2
                for (int j = g; j < M; j += G) {
                    const int k = j - fft_div(j, Ns, invNs) * Ns, jo = (j - k) * 3 + k;
                    C v0 = a[fft_pidx<T>(j)], v1 = a[fft_pidx<T>(j + M)], v2 = a[fft_pidx<T>(j + 2 * M)];
                    if (twd) { v1 = cmul(v1, tw[k * ts]); v2 = cmul(v2, tw[2 * k * ts]); }
                    const C s = cadd(v1, v2), d = csub(v1, v2);
                    const C m = C{v0.x - (T)0.5 * s.x, v0.y - (T)0.5 * s.y};
                    const C e = crot(C{h3 * d.x, h3 * d.y}, sgn);
                    b[fft_pidx<T>(jo)] = cadd(v0, s);
                    b[fft_pidx<T>(jo + Ns)] = cadd(m, e);
                    b[fft_pidx<T>(jo + 2 * Ns)] = csub(m, e);
                }
            } else if (r == 5) {
                const T c1 = (T)0.30901699437494742410, c2 = (T)-0.80901699437494742410;     // cos(2 pi / 5), cos(4 pi / 5)
                const T s1 = (T)0.95105651629515357212, s2 = (T)0.58778525229247312917;      // sin(2 pi / 5), sin(4 pi / 5)
                for (int j = g; j < M; j += G) {
                    const int k = j - fft_div(j, Ns, invNs) * Ns, jo = (j - k) * 5 + k;
                    C v0 = a[fft_pidx<T>(j)], v1 = a[fft_pidx<T>(j + M)], v2 = a[fft_pidx<T>(j + 2 * M)], v3 = a[fft_pidx<T>(j + 3 * M)],
                      v4 = a[fft_pidx<T>(j + 4 * M)];
                    if (twd) {
                        v1 = cmul(v1, tw[k * ts]); v2 = cmul(v2, tw[2 * k * ts]); v3 = cmul(v3, tw[3 * k * ts]);
                        v4 = cmul(v4, tw[4 * k * ts]);
                    }
                    const C a1 = cadd(v1, v4), a2 = cadd(v2, v3), b1 = csub(v1, v4), b2 = csub(v2, v3);
                    const C m1 = C{v0.x + c1 * a1.x + c2 * a2.x, v0.y + c1 * a1.y + c2 * a2.y};
                    const C m2 = C{v0.x + c2 * a1.x + c1 * a2.x, v0.y + c2 * a1.y + c1 * a2.y};
                    const C n1 = crot(C{s1 * b1.x + s2 * b2.x, s1 * b1.y + s2 * b2.y}, sgn);
                    const C n2 = crot(C{s2 * b1.x - s1 * b2.x, s2 * b1.y - s1 * b2.y}, sgn);
                    b[fft_pidx<T>(jo)] = C{v0.x + a1.x + a2.x, v0.y + a1.y + a2.y};
                    b[fft_pidx<T>(jo + Ns)] = cadd(m1, n1);
                    b[fft_pidx<T>(jo + 2 * Ns)] = cadd(m2, n2);
                    b[fft_pidx<T>(jo + 3 * Ns)] = csub(m2, n2);
                    b[fft_pidx<T>(jo + 4 * Ns)] = csub(m1, n1);
                }
            } else {
                // generic radix: output (j, m) = sum_q in[j + q M] tw[q (k ts + m M) mod N], one output per thread and turn
                const float invM = 1.0f / (float)M;
                for (int o = g; o < N; o += G) {
                    const int m = fft_div(o, M, invM), j = o - m * M;
                    const int k = j - fft_div(j, Ns, invNs) * Ns, jo = (j - k) * r + k;
                    int step = k * ts + m * M;              // < M + N
                    if (step >= N) step -= N;
                    int idx = 0;
                    C acc = C{(T)0, (T)0};
                    for (int q = 0; q < r; ++q) {
                        acc = cadd(acc, cmul(a[fft_pidx<T>(j + q * M)], tw[idx]));
                        idx += step;
                        if (idx >= N) idx -= N;
                    }
                    b[fft_pidx<T>(jo + m * Ns)] = acc;
                }
            }
        }
        __syncthreads();
        C* t = a; a = b; b = t;
        Ns *= r;
    }

    // ---- line maximum of |s Y| and its first index in output order (peaknorm, peak)
    T mx = (T)1;
    int nmax = 0;
    if (epi & (FFT_PEAKNORM | FFT_PEAK)) {
        T best = (T)-1;
        int bi = 0;
        if (live) {
            for (int k = g; k < N; k += G) {
                int src = k + sh_out;
                if (src >= N) src -= N;
                C v = a[fft_pidx<T>(src)];
                v.x *= scale; v.y *= scale;
                if (win != nullptr && win_store) { const T w = win[k]; v.x *= w; v.y *= w; }
                const T mag = tsqrt<T>(v.x * v.x + v.y * v.y);
                if (mag > best) { best = mag; bi = k; }
            }
        }
        rv[tid] = best; ri[tid] = bi;
        __syncthreads();
        for (int s = G >> 1; s > 0; s >>= 1) {
            if (g < s) {
                const T ov = rv[tid + s];
                const int oi = ri[tid + s];
                if (ov > rv[tid] || (ov == rv[tid] && oi < ri[tid])) { rv[tid] = ov; ri[tid] = oi; }
            }
            __syncthreads();
        }
        mx = rv[tid - g];
        nmax = ri[tid - g];
    }
    if (!live) return;

    // ---- store: out[k] = epilogue(s Y[(k + sh_out) mod N])
    const bool ws = win != nullptr && win_store;
    auto sample = [&](int k, C& v, T& re) {
        int src = k + sh_out;
        if (src >= N) src -= N;
        v = a[fft_pidx<T>(src)];
        v.x *= scale; v.y *= scale;
        if (ws) { const T w = win[k]; v.x *= w; v.y *= w; }
        re = (T)0;
        fft_chain<T, C>(v, re, epi, mx);
    };
    const bool real_out = (epi & (FFT_ABS | FFT_SQUARE)) != 0;
    if (epi & FFT_PEAK) {
        if (g != 0) return;
        const int np = nmax + 1 == N ? 0 : nmax + 1, nn = nmax == 0 ? N - 1 : nmax - 1;
        C z0, zp, zn;
        T r0, rp, rn;
        sample(nmax, z0, r0); sample(np, zp, rp); sample(nn, zn, rn);
        T rpos, rneg;
        if (real_out) { rpos = rp / r0; rneg = rn / r0; }
        else {
            const T den = z0.x * z0.x + z0.y * z0.y;
            rpos = (zp.x * z0.x + zp.y * z0.y) / den;
            rneg = (zn.x * z0.x + zn.y * z0.y) / den;
        }
        const T dpos = -rpos / ((T)1 - rpos), dneg = rneg / ((T)1 - rneg);
        const T delta = (dneg + dpos) / (T)2 + quinn_k<T>(dneg * dneg) - quinn_k<T>(dpos * dpos);
        y[line] = (T)(start + ((double)nmax + (double)delta) * df);
        return;
    }
    if (real_out) {
        T* yl = y + (size_t)line * N;
        for (int k = g; k < N; k += G) {
            C v; T re;
            sample(k, v, re);
            yl[k] = re;
        }
    } else {
        C* yl = reinterpret_cast<C*>(y) + (size_t)line * N;
        for (int k = g; k < N; k += G) {
            C v; T re;
            sample(k, v, re);
            yl[k] = v;
        }
    }
}

template <typename T>
static int fft_launch(const void* x, const void* tw, const void* win, int win_store, const FftPasses& P, int N, long long nlines,
                      int inverse, int sh_in, int sh_out, double scale, int epi, double start, double df, void* y, hipStream_t st)
{
    using C = typename Cx<T>::type;
    const int L = fft_lines_per_group(N), LS = fft_line_stride<T>(N);
    int lgL = 0;
    while ((1 << lgL) < L) ++lgL;
    const long long nblk = (nlines + L - 1) / L;
    if (nblk > 0x7fffffffLL) return RIME_EINVAL;
    const size_t lds = (size_t)2 * L * LS * sizeof(C) + FFT_THREADS * (sizeof(T) + sizeof(int));
    if (lds > 160 * 1024) return RIME_EUNSUPPORTED;
    if (lds > 48 * 1024) {
        // the attribute belongs to the (function, device) pair: remembered per device of the calling thread
        static unsigned long long configured = 0ull;
        int devid = 0;
        if (hipGetDevice(&devid) != hipSuccess) devid = 0;
        const unsigned long long bit = 1ull << (devid & 63);
        if (!(configured & bit)) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&fft_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    160 * 1024) != hipSuccess)
                return check_launch();
            configured |= bit;
        }
    }
    hipLaunchKernelGGL((fft_kernel<T>), dim3((unsigned)nblk), dim3(FFT_THREADS), lds, st, (const T*)x, (const T*)tw, (const T*)win,
                       win_store, P, N, nlines, lgL, LS, (T)(inverse ? 1 : -1), sh_in, sh_out, (T)scale, epi, start, df, (T*)y);
    return check_launch();
}

} // namespace rime

using namespace rime;

extern "C" int rime_fft_apply(int dtype, const void* x, const void* tw, const void* win, int win_on_store, const int* radix,
                              int nradix, int N, long long nlines, int inverse, int shift_in, int shift_out, double scale,
                              int epilogue, double start, double df, void* y, void* stream)
{
    if (!real_dtype_ok(dtype)) return RIME_EINVAL;
    if (N < 1 || N > FFT_MAXN || nlines < 0) return RIME_EINVAL;
    if (epilogue < 0 || epilogue > (FFT_ABS | FFT_PEAKNORM | FFT_SQUARE | FFT_PEAK)) return RIME_EINVAL;
    if ((inverse != 0 && inverse != 1) || (win_on_store != 0 && win_on_store != 1)) return RIME_EINVAL;
    if (shift_in < 0 || shift_in >= N || shift_out < 0 || shift_out >= N) return RIME_EINVAL;
    if (nradix < 0 || nradix > FFT_MAXPASS || (nradix > 0 && !radix)) return RIME_EINVAL;
    FftPasses P;
    P.n = nradix;
    long long prod = 1;
    for (int p = 0; p < FFT_MAXPASS; ++p) {
        P.radix[p] = p < nradix ? radix[p] : 1;
        if (p < nradix) {
            if (radix[p] < 2 || radix[p] > N) return RIME_EINVAL;
            prod *= radix[p];
            if (prod > N) return RIME_EINVAL;
        }
    }
    if (prod != N) return RIME_EINVAL;
    if (!x || !y || !tw) return RIME_EINVAL;
    if (!(scale == scale)) return RIME_EINVAL;
    if (nlines == 0) return RIME_OK;                          // nothing to write
    return with_real(dtype, [&](auto t) {
        return fft_launch<decltype(t)>(x, tw, win, win_on_store, P, N, nlines, inverse, shift_in, shift_out, scale, epilogue, start,
                                       df, y, as_stream(stream));
    });
}
