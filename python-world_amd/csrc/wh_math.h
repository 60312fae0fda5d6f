// Double-precision log (and exp / sincospi) for the spectral kernels (round 6).  The device library's are built for the last
// ulp over the whole range — log() is 113 instructions (double-double sums), exp() 56 and sincospi() 82, a third of them
// v_mov / s_mov pairs that materialise polynomial coefficients on every call — and one frame of a minimum-phase chain takes
// 513 logs and 514 complex exponentials, a frame of CheapTrick 513 logs and as many exponentials.
//   wh::flog — 74 instructions, <= 2 ulp (tests/test_hip_math.py: 5e-16 relative against NumPy over 1e-300 .. 1e300, near 1,
//   denormals, the ends of the domain) — is what the kernels use: CheapTrick 1.12 -> 1.04 ms and response_kernel 3.43 -> 3.33 ms
//   at config 2, req_filter 25.1 -> 24.3 and CheapTrick 17.7 -> 16.5 ms in the north-star batch.
//   wh::fexp / wh::fsincospi are accurate to the same few ulp but no shorter than the library's once the compiler has
//   materialised their coefficients (66 / 75 instructions), and with the coefficients read as a scalar __constant__
//   table every evaluation waits for the table: response 3.43 -> 3.90 ms, req_filter 25.0 -> 34.5.
//   Measured, tested (wh_math_probe), not used by any kernel.
// The table-driven forms (round 22; below, with the table's layout): a per-lane table value takes over the coarse part of
// the range reduction and leaves a polynomial of three to five terms.  Per PAIR of evaluations inside one call, as the
// minimum-phase chains make them (tools/ubench/math_tables.hip, profiles/r22_math_tables_ubench.txt):
//   wh::tsincospi — 256 entries (the context's own twiddle table), 3 + 3 terms; sincospi + exp of a pair of bins 214 -> 132
//   instructions together with wh::texp.  Used by the complex exponentials of the pulse responses from N = 1024 on
//   (cis_pair_tab_call, wh_minphase.h): response_kernel 2.73 -> 2.66 ms at config 2, 35.6 -> 34.9 ms at config 5; alone
//   (with the library's exp) 2.73 -> 2.67.  A 2048-entry table with 2 + 2 terms measured the same (2.66): not kept.
//   wh::texp — 128 entries, degree 5.  On its own no gain over the library's exp (response_kernel 2.73 -> 2.73 with the
//   library's sincospi, cheaptrick_kernel 0.994 -> 0.996 ms); next to tsincospi, whose coefficients and loads it shares
//   the call with, it is the last 0.02 ms.  Used there only.
//   wh::tlog — 93 nodes; 70 instructions against flog's 74 as a call, and its table value is the FIRST thing it needs, so
//   every call starts by waiting for the load: response_kernel 2.65 -> 2.69 ms, cheaptrick_kernel 0.996 -> 1.005 ms,
//   the micro-benchmark 2.66 -> 3.92 ms.  Measured, tested, not used by any kernel.
//   Where the table forms lost although they are shorter: req_filter_kernel (the Requiem filter, 70 VGPRs and seven waves
//   per SIMD by registers) — the table call holds 50 VGPRs where the library call holds 22, the kernel went to 84 VGPRs
//   and from 1.43 to 1.53 ms at config 4; serialised to fit (74 VGPRs) it was 1.43, no gain.  It keeps the library call,
//   and so does response_kernel<512> (92 -> 107 VGPRs, a wave per SIMD).
// No loops and no branches: the ends of the domains are selects (log 0 = -inf, log of a negative = NaN, exp of +-inf = inf / 0),
// NaN goes through.
#pragma once
#include <hip/hip_runtime.h>

#include "wh_device.h"

namespace wh {

// The coefficients are literals the compiler materialises.  (As a __constant__ table read through the scalar unit the
// s_load latency in front of every evaluation made all three kernels SLOWER than the device library: response 3.43 ->
// 3.90 ms, req_filter 25.0 -> 34.5.)
struct MathTab {
  static constexpr double v[44] = {
    // [0..8] atanh series 2/(2k+1), k = 1..9
    2.0 / 3, 2.0 / 5, 2.0 / 7, 2.0 / 9, 2.0 / 11, 2.0 / 13, 2.0 / 15, 2.0 / 17, 2.0 / 19,
    // [9] ln2 high part (33 bits), [10] low part, [11] log2(e)
    0x1.62e42fee00000p-1, 0x1.a39ef35793c76p-33, 0x1.71547652b82fep+0,
    // [12..25] 1/n!, n = 13 .. 0
    1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0,
    1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0,
    // [26..33] sin(pi t) = t (c7 u^7 + ... + c0), u = t^2: (-1)^k pi^(2k+1) / (2k+1)!, k = 7 .. 0
    -0x1.6fadb9f155744p-16, 0x1.e8f434d018d63p-12, -0x1.e3074fde8871fp-8, 0x1.50783487ee782p-4, -0x1.32d2cce62bd86p-1,
    0x1.466bc6775aae2p+1, -0x1.4abbce625be53p+2, 0x1.921fb54442d18p+1,
    // [34..42] cos(pi t) = d8 u^8 + ... + d0: (-1)^k pi^(2k) / (2k)!, k = 8 .. 0
    0x1.20c62c2f2d7f5p-18, -0x1.b6e24f44b128fp-14, 0x1.f9d38a3763cc3p-10, -0x1.a6d1f2a204a8cp-6, 0x1.e1f506891babbp-3,
    -0x1.55d3c7e3cbffap+0, 0x1.03c1f081b5ac4p+2, -0x1.3bd3cc9be45dep+2, 1.0,
    0.0};
  __device__ __forceinline__ constexpr double operator[](int i) const { return v[i]; }
};
__device__ __forceinline__ constexpr MathTab math_tab() { return MathTab(); }

// a / b through the reciprocal: v_rcp_f64, two Newton steps, the quotient and one residual correction — 8 instructions and
// <= 1 ulp where the IEEE division the compiler emits is ~15 (two v_div_scale, the reciprocal, five fused steps, v_div_fmas,
// v_div_fixup).  For divides whose operands are ordinary normal numbers and whose result feeds values compared at
// tolerances (the interval frequencies and interpolation slopes of Harvest's raw candidates, eight per frame and channel:
// hv_rawdet_kernel 5.65 -> 5.50 ms at 256 x 10 s; both forms of the raw-candidate stage use it, so they still agree bit for bit;
// the quotients of the refinement's epilogue and the crossing positions of the band walkers).  b = 0, Inf or NaN give Inf / NaN like the hardware reciprocal does.
__device__ __forceinline__ double fdiv(double a, double b) {
  double y = __builtin_amdgcn_rcp(b);
  y = fma(fma(-b, y, 1.0), y, y);
  y = fma(fma(-b, y, 1.0), y, y);
  const double q = a * y;
  return fma(fma(-b, q, a), y, q);
}

// log(x), x > 0: x = m 2^e with m in [sqrt(1/2), sqrt(2)), log m = 2 atanh((m-1)/(m+1)) as nine terms of the series in
// r^2 <= 0.0295 (truncation 2e-17), e ln2 added in two parts.  The quotient is a reciprocal with two Newton steps and a
// residual correction.
__device__ __forceinline__ double flog(double x) {
  const auto T = math_tab();
  double m = __builtin_amdgcn_frexp_mant(x);  // [0.5, 1) (denormals included)
  int e = __builtin_amdgcn_frexp_exp(x);
  const bool low = m < 0.70710678118654752440;
  m = low ? m + m : m;
  e = low ? e - 1 : e;
  const double f = m - 1.0, d = m + 1.0;
  double y = __builtin_amdgcn_rcp(d);
  y = fma(fma(-d, y, 1.0), y, y);
  y = fma(fma(-d, y, 1.0), y, y);
  double r = f * y;
  r = fma(fma(-d, r, f), y, r);
  const double s = r * r;
  double p = T[8];
#pragma unroll
  for (int k = 7; k >= 0; --k) p = fma(p, s, T[k]);
  const double ed = (double)e;
  // e ln2_hi is exact (33-bit constant, |e| < 2^11); the small terms are summed first
  const double small = fma(ed, T[10], (r * s) * p);
  double res = fma(ed, T[9], (r + r) + small);
  // the ends of the domain as the library has them: log(0) = -inf, log(inf) = inf, log(x < 0) = NaN (a NaN goes through by itself)
  res = x == 0.0 ? -__builtin_inf() : res;
  res = x == __builtin_inf() ? x : res;
  res = x < 0.0 ? __builtin_nan("") : res;
  return res;
}

// exp(x): x = k ln2 + r, |r| <= ln2 / 2, Taylor to r^13 (truncation 4e-18), scaled by v_ldexp
__device__ __forceinline__ double fexp(double x) {
  const auto T = math_tab();
  const double k = rint(x * T[11]);
  double r = fma(-k, T[9], x);
  r = fma(-k, T[10], r);
  double p = T[12];
#pragma unroll
  for (int i = 13; i <= 25; ++i) p = fma(p, r, T[i]);
  // (k beyond the int range only for |x| > 1e9: the clamp keeps the conversion defined, ldexp saturates to 0 / inf)
  const double kc = fmin(fmax(k, -4000.0), 4000.0);
  double res = ldexp(p, (int)kc);
  res = x > 709.79 ? __builtin_inf() : res;   // (also +inf, where r = inf - inf)
  res = x < -745.2 ? 0.0 : res;               // (also -inf)
  return res;
}

// (sin, cos)(pi x): x reduced to t in [-1/4, 1/4] around the nearest multiple of 1/2, two polynomials in t^2
// (truncation 5e-17 / 2e-18), quadrant by selects
__device__ __forceinline__ double2 fsincospi(double x) {
  const auto T = math_tab();
  const double r = fma(-2.0, rint(0.5 * x), x);  // [-1, 1]  (exact)
  const double qd = rint(r + r);                  // -2 .. 2
  const double t = fma(-0.5, qd, r);              // [-1/4, 1/4]  (exact)
  const double u = t * t;
  double ps = T[26], pc = T[34];
#pragma unroll
  for (int i = 27; i <= 33; ++i) ps = fma(ps, u, T[i]);
#pragma unroll
  for (int i = 35; i <= 42; ++i) pc = fma(pc, u, T[i]);
  const double s = t * ps, c = pc;
  const int q = (int)qd & 3;  // 0: (s, c)   1: (c, -s)   2: (-s, -c)   3: (-c, s)
  const double a = (q & 1) ? c : s, b = (q & 1) ? s : c;
  const double sn = (q & 2) ? -a : a;
  const double cs = ((q + 1) & 2) ? -b : b;
  return make_double2(sn, cs);
}

// ------------------------------------------------------------------------------------------
// Table-driven forms: a per-lane table value does the coarse part of the range reduction, a short polynomial the rest.
// ------------------------------------------------------------------------------------------
// The context's math table (wh::math_table, wh_api.hip: built on the host in long double, uploaded once), in doubles:
//   [kMtExp, +128)         2^(j/128), j < 128
//   [kMtLog, +4 * 93)      the logarithm's nodes c = (90 + i)/128, i < 93 (they cover [sqrt(1/2), sqrt(2)) with one node of
//                          margin at either end): (inv, Lhi, Llo, 0) with inv = 1/c rounded to 24 bits, -log(inv) = Lhi + Llo
//                          and Lhi a multiple of 2^-42, so that e ln2_hi + Lhi is exact; the node c = 1 is (1, 0, 0, 0)
// The sine / cosine table is the context's twiddle table of size 256 (d_twiddle + 256: (cos, -sin)(pi j/128), exact on
// the axes, the upper half the bitwise mirror of the lower one).
// Every index is masked or clamped in a way that holds for NaN, +-Inf, 0, denormals and 1e300 as well: no input reads
// outside the tables.
constexpr int kMtExp = 0, kMtLog = 128, kMtLogNodes = 93, kMtLogFirst = 90, kMtEntries = kMtLog + 4 * kMtLogNodes;
constexpr double kMtMagic = 0x1.8p+52;  // t + 1.5 * 2^52 leaves rint(t) in the low mantissa bits (|t| < 2^51)

// (sin, cos)(pi b): n = rint(128 b), r = b - n/128 (exact for every double), x = pi r with |x| <= pi/256, sin x to x^7
// and cos x to x^6 (truncation 3e-20 / 6e-18), rotated by the table's (cos, sin)(pi n/128).  <= 2 ulp of 1 absolute for
// |b| < 2^44; beyond that the reduction no longer sees the fraction (the kernels' angles stay below 600).
__device__ __forceinline__ double2 tsincospi(double b, ckp<const double2> tw256) {
  const double t = fma(b, 128.0, kMtMagic);
  const int j = (int)(unsigned)__double_as_longlong(t) & 255;
  const double n = t - kMtMagic;
  const double r = fma(-n, 1.0 / 128, b);
  const double2 w = ldg2(tw256 + j);  // (C, -S)
  const double x = 0x1.921fb54442d18p+1 * r;
  const double u = x * x;
  const double ps = fma(u, fma(u, -0x1.a01a01a01a01ap-13, 0x1.1111111111111p-7), -0x1.5555555555555p-3);
  const double pc = fma(u, fma(u, -0x1.6c16c16c16c17p-10, 0x1.5555555555555p-5), -0.5);
  const double sx = fma(x * u, ps, x), cq = u * pc;  // sin x, cos x - 1
  const double C = w.x, S = -w.y;
  return make_double2(S + fma(S, cq, C * sx), C + fma(C, cq, -(S * sx)));
}

// exp(a): n = rint(a 128/ln2), r = a - n ln2/128 in two parts (n hi is exact: 33-bit hi, |n| < 2^18), |r| <= ln2/256,
// 2^(n/128) = 2^(n >> 7) T[n & 127], exp r - 1 to r^5 (truncation 6e-19).  <= 1.5 ulp.
__device__ __forceinline__ double texp(double a, ckp<const double> mt) {
  const double t = fma(a, 0x1.71547652b82fep+7, kMtMagic);
  const int ni = (int)(unsigned)__double_as_longlong(t);
  const double n = t - kMtMagic;
  const double T = ldg(mt + (kMtExp + (ni & 127)));
  double r = fma(-n, 0x1.62e42fee00000p-8, a);
  r = fma(-n, 0x1.a39ef35793c76p-40, r);
  double q = fma(r, 0x1.1111111111111p-7, 0x1.5555555555555p-5);
  q = fma(r, q, 0x1.5555555555555p-3);
  q = fma(r, q, 0.5);
  q = fma(r * r, q, r);  // exp r - 1
  double res = ldexp(fma(T, q, T), ni >> 7);
  res = a > 709.79 ? __builtin_inf() : res;  // (also +inf, and every a whose n has left the low mantissa bits)
  res = a < -745.2 ? 0.0 : res;              // (also -inf)
  return res;
}

// log(x): flog's m in [sqrt(1/2), sqrt(2)) and e; the node c nearest to m, r = m inv - 1 (|r| < 0.0056),
// log m = -log(inv) + log1p(r), log1p to r^7 (truncation 2e-19).  <= 1.5 ulp; x next to 1 keeps its relative accuracy (the node
// c = 1 is exact: r = m - 1, no constant is added).
__device__ __forceinline__ double tlog(double x, ckp<const double> mt) {
  double m = __builtin_amdgcn_frexp_mant(x);
  int e = __builtin_amdgcn_frexp_exp(x);
  const bool low = m < 0.70710678118654752440;
  m = low ? m + m : m;
  e = low ? e - 1 : e;
  // (fmax / fmin return the other operand for a NaN: the index stays inside the table for every input)
  const int i = (int)fmin(fmax(rint(m * 128.0) - (double)kMtLogFirst, 0.0), (double)(kMtLogNodes - 1));
  const ckp<const double2> node = ck_as<const double2>(mt + (kMtLog + 4 * i));
  const double2 n0 = ldg2(node), n1 = ldg2(node + 1);  // (inv, Lhi), (Llo, 0)
  const double r = fma(m, n0.x, -1.0);
  double p = fma(r, 0x1.2492492492492p-3, -0x1.5555555555555p-3);
  p = fma(r, p, 0x1.999999999999ap-3);
  p = fma(r, p, -0.25);
  p = fma(r, p, 0x1.5555555555555p-2);
  p = fma(r, p, -0.5);
  const double ed = (double)e;
  const double small = fma(r * r, p, fma(ed, 0x1.a39ef35793c76p-33, n1.x));
  double res = fma(ed, 0x1.62e42fee00000p-1, n0.y) + (r + small);
  res = x == 0.0 ? -__builtin_inf() : res;
  res = x == __builtin_inf() ? x : res;
  res = x < 0.0 ? __builtin_nan("") : res;
  return res;
}

}  // namespace wh
