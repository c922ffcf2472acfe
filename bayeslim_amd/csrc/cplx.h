// cplx.h -- the complex value of the vector-ALU kernels on interleaved (re, im) pairs: cal.hip, jones.hip, redvis.hip, coupling.hip,
// redcoupling.hip (fft.hip keeps float2 / double2: its type carries the LDS padding rule).  Everything is force-inlined: a kernel
// that uses it assembles to the code object it would with the text written out in place.  A product has two forms that may round
// differently, so neither replaces the other:
//   expression form  cmul, cmulc: a * b - c * d as written; under -ffp-contract=fast the COMPILER picks the product it fuses.
//                    cal.hip, jones.hip; coupling.hip where it builds E (cp_fetch) and applies conj(dly) to a dense result
//   fixed form       cmul_fma, cmulc_fma, cfma, cfmac: explicit tfma, the re * re (re * im) product first, the im product fused
//                    onto it.  redcoupling.hip throughout; coupling.hip in the tile product (cp_accumulate)
// cadd, cconj and `s += a` are exact; redvis.hip uses only the last.  partred.hip takes the type alone: its coefficients are real,
// so it writes one tfma per component.  Some sites keep `{a.re, -a.im}` or `s.re += a.re; s.im +=
// a.im;` written out: through the call the compiler orders their kernel differently (same bits, other instructions) -- the
// conjugates and the combine kernel of redcoupling.hip, the block sum of redvis.hip, the two sums of coupling.hip.
#pragma once
#include "rime_common.h"

namespace rime {

template <typename T> struct cx { T re, im; };
template <typename T> __device__ __forceinline__ void operator+=(cx<T>& s, const cx<T>& a) { s.re += a.re; s.im += a.im; }
template <typename T> __device__ __forceinline__ cx<T> cadd(cx<T> a, cx<T> b) { return {a.re + b.re, a.im + b.im}; }
template <typename T> __device__ __forceinline__ cx<T> cconj(cx<T> a) { return {a.re, -a.im}; }
// expression form: a b, a conj(b)
template <typename T> __device__ __forceinline__ cx<T> cmul(cx<T> a, cx<T> b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
template <typename T> __device__ __forceinline__ cx<T> cmulc(cx<T> a, cx<T> b) { return {a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im}; }
// fixed form: a b, a conj(b), s += a b, s += conj(a) b
template <typename T> __device__ __forceinline__ cx<T> cmul_fma(cx<T> a, cx<T> b) { return {tfma<T>(-a.im, b.im, a.re * b.re), tfma<T>(a.im, b.re, a.re * b.im)}; }
template <typename T> __device__ __forceinline__ cx<T> cmulc_fma(cx<T> a, cx<T> b) { return {tfma<T>(a.im, b.im, a.re * b.re), tfma<T>(a.im, b.re, -(a.re * b.im))}; }
template <typename T> __device__ __forceinline__ void cfma(cx<T>& s, cx<T> a, cx<T> b)
{ s.re = tfma<T>(-a.im, b.im, tfma<T>(a.re, b.re, s.re)); s.im = tfma<T>(a.im, b.re, tfma<T>(a.re, b.im, s.im)); }
template <typename T> __device__ __forceinline__ void cfmac(cx<T>& s, cx<T> a, cx<T> b)
{ s.re = tfma<T>(a.im, b.im, tfma<T>(a.re, b.re, s.re)); s.im = tfma<T>(-a.im, b.re, tfma<T>(a.re, b.im, s.im)); }

} // namespace rime
