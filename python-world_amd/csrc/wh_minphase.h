// The minimum-phase chain shared by the pulse responses (wh_synthesis.hip) and the Requiem filter (wh_requiem.hip): the
// transcendentals of its loops as real calls, and min_phase_response.  Its arithmetic may fuse a*b+c into one FP64
// instruction (the library is built with -ffp-contract=off): the outputs are compared with the reference at tolerances.
// Include after wh_math.h and the unit's opaque WH_TID (wh_tid.h).
#pragma once
#include <type_traits>
#include "wh_fft.h"

namespace {

// Threads cooperating on one pulse / frame: 256 up to N = 1024, 512 from N = 2048 (44.1 / 48 kHz), where the 54 KB
// of LDS per pulse leave two workgroups per CU and the thread count is the occupancy (measured 58.6 -> 50.5 ms on
// config 5).
constexpr int ft_syn(int n) { return n >= 2048 ? 512 : 256; }

// Transcendentals of the per-pulse loop as real calls: inlined, their polynomial coefficients (64-bit literals live in
// VGPR pairs) are loop invariants of response_kernel's pulse loop and get parked in registers across the whole body.
// (exp(a0) cos(pi b0), exp(a0) sin(pi b0), exp(a1) cos(pi b1), exp(a1) sin(pi b1)): two bins of a minimum-phase spectrum
__device__ __attribute__((noinline)) double4 cis_pair_call(double a0, double b0, double a1, double b1) {
  const double e0 = exp(a0), e1 = exp(a1);
  double s0, c0, s1, c1;
  sincospi(b0, &s0, &c0);
  sincospi(b1, &s1, &c1);
  return make_double4(e0 * c0, e0 * s0, e1 * c1, e1 * s1);
}
// The same through wh_math.h's table-driven forms: `tw256` is the context's twiddle table of size 256, `mt` its math table.
// 214 -> 132 instructions per pair of bins (145 -> 95 VALU, 60 -> 25 coefficient moves); the four table values are needed
// by the last multiplies only, the polynomials run while they are on their way.  It holds more values at once — 50 VGPRs
// against the library form's 22 — so it is taken where the kernel has them to spare (TAB of min_phase_response).
__device__ __attribute__((noinline)) double4 cis_pair_tab_call(double a0, double b0, double a1, double b1, wh::ckp<const double2> tw256,
                                                               wh::ckp<const double> mt) {
  const double2 sc0 = wh::tsincospi(b0, tw256), sc1 = wh::tsincospi(b1, tw256);
  const double e0 = wh::texp(a0, mt), e1 = wh::texp(a1, mt);
  return make_double4(e0 * sc0.y, e0 * sc0.x, e1 * sc1.y, e1 * sc1.x);
}
__device__ __attribute__((noinline)) double2 log_pair_call(double x, double y) { return make_double2(wh::flog(x), wh::flog(y)); }
__device__ __attribute__((noinline)) double log_call(double x) { return wh::flog(x); }
// (wh::tlog needs its table value — the node's reciprocal — for its FIRST instruction, so every call begins by waiting for
// the load: measured slower than wh::flog here, not used.  wh_math.h has the numbers.)

// Minimum-phase response (synthesis.py:100-116; synthesisRequiem.py:112-118) from the mirrored log-amplitude to the time
// domain, with the O(N) passes between the three transforms fused:
//   in : zr[n] = log|S[min(n, N-n)]| / 2, n < N (real, even), visible;  out: time-domain response N * h[n] in zr.
//   (1) forward transform of a real EVEN sequence: its spectrum is real, so the post-pass of the half-size transform
//       computes real parts only, and writes them where the next transform wants them — folded onto the upper half,
//       doubled (cepstrum fold) — instead of: post-pass -> copy real parts -> fold (three LDS round trips, three barriers);
//   (2) after the second transform a thread holds the pair of bins (k, N/2-k) in registers through the post-pass, the
//       complex exponential AND the pre-pass of the inverse real transform: exp(r.x/N) * cis(-r.y/N - delay*k), where
//       `delay_pi` (units of pi per bin) is the pulse's fractional delay — the reference multiplies the spectrum by
//       exp(-i*coef*shift*k) afterwards (synthesis.py:61-64); folding it into the angle saves one sincospi and one
//       complex product per bin, and the four passes over the half spectrum become one.
// TAB: the exponentials through cis_pair_tab_call and `mt`, the context's math table (wh_math.h); otherwise `mt` is not read.
// `mul(k, E)`: what the minimum-phase bin k (0 <= k <= N/2) is multiplied with before the inverse transform — identity
// for the pulse responses, the excitation frame's spectrum in the Requiem filter (synthesisRequiem.py:112-118).
// The chain's three 512-point transforms (N = 1024, the 16 kHz shape): WAVE puts each on one wave of its GT-thread group
// (wh::fft_lds_wave: one barrier per transform where the workgroup-wide plan takes six; the voiced chains' plan and bits
// are unchanged, an unvoiced pulse's single chain goes from 4-4-4-4-2 on two waves to 8-8-8 on one).  Other lengths and
// the Requiem filter keep the workgroup-wide plans.
template <int M, bool INV, int GT, int FT, bool WAVE>
__device__ __forceinline__ void mp_fft(wh::ckp<double2> zb, wh::ckp<const double2> tw) {
  if constexpr (WAVE) wh::fft_lds_wave<M, INV, GT, FT>(zb, tw);
  else wh::fft_lds<M, INV, GT, FT>(zb, tw);
}
struct SpectrumIdentity {
  __device__ __forceinline__ double2 operator()(int, double2 e) const { return e; }
};
// `side(i, n)`: a job for the waves that a WAVE chain's FIRST transform leaves without butterflies (wh::fft_lds_wave) —
// the pulse's noise run in response_pulse.  NoSide: they go straight to the transform's barrier.
struct NoSide {};
template <int N, int GT, bool WAVE = false, bool TAB = false, class Mul = SpectrumIdentity, class Side = NoSide>
__device__ __forceinline__ void min_phase_response(wh::ckp<double2> zb, wh::ckp<const double2> tw_base, wh::ckp<const double> mt, double delay_pi, Mul mul = Mul(),
                                                   Side side = Side()) {
#pragma clang fp contract(fast)
  constexpr int FT = ft_syn(N);
  constexpr int M = N / 2;
  constexpr int PP = (M / 2 + 1 + GT - 1) / GT;  // bin pairs (k, M-k), k <= M/2, per thread
  const wh::ckp<double> zr = wh::ck_as<double>(zb);
  const int gt = WH_TID & (GT - 1);
  const wh::ckp<const double2> WH_RESTRICT w = tw_base + N;
  if constexpr (WAVE && !std::is_same<Side, NoSide>::value) wh::fft_lds_wave<M, false, GT, FT>(zb, tw_base + M, side);
  else mp_fft<M, false, GT, FT, WAVE>(zb, tw_base + M);
  {
    double ck[PP], cm[PP];
#pragma unroll
    for (int p = 0; p < PP; ++p) {
      const int k = gt + p * GT;
      ck[p] = cm[p] = 0.0;
      if (k <= M / 2) {
        const double2 a = zb[k], b = zb[M - k];
        if (k == 0) {
          ck[p] = a.x + a.y;
          cm[p] = a.x - a.y;
        } else {
          const double er = 0.5 * (a.x + b.x), dr = 0.5 * (a.x - b.x), di = 0.5 * (a.y + b.y);
          const double2 wk = wh::ldg2(w + k);
          const double tr = fma(wk.x, di, wk.y * dr);
          ck[p] = er + tr;  // Re X[k]
          cm[p] = er - tr;  // Re X[M-k]
        }
      }
    }
    wh::sync<FT>();  // every pair has been read
#pragma unroll
    for (int p = 0; p < PP; ++p) {
      const int k = gt + p * GT;
      if (k <= M / 2) {
        if (k == 0) {
          zr[0] = ck[p];
          zr[M] = 2 * cm[p];
        } else {
          zr[N - k] = 2 * ck[p];
          zr[M + k] = 2 * cm[p];  // (k = M/2: the same slot, the same value)
        }
      }
    }
    for (int n = 1 + gt; n < M; n += GT) zr[n] = 0.0;
    wh::sync<FT>();
  }
  mp_fft<M, false, GT, FT, WAVE>(zb, tw_base + M);
#pragma unroll 1
  for (int k = gt; k <= M / 2; k += GT) {
    const double2 a = zb[k], b = zb[M - k];
    double2 x0, x1;  // R[k], R[M-k]: spectrum of the folded cepstrum
    const double2 wk = wh::ldg2(w + k);
    if (k == 0) {
      x0 = make_double2(a.x + a.y, 0.0);
      x1 = make_double2(a.x - a.y, 0.0);
    } else {
      const double er = 0.5 * (a.x + b.x), ei = 0.5 * (a.y - b.y);
      const double dr = 0.5 * (a.x - b.x), di = 0.5 * (a.y + b.y);
      const double tr = fma(wk.x, di, wk.y * dr);
      const double ti = fma(wk.y, di, -(wk.x * dr));
      x0 = make_double2(er + tr, ei + ti);
      x1 = make_double2(er - tr, ti - ei);
    }
    // minimum-phase spectrum exp(conj(R) / N) with the fractional delay in the angle (both in units of pi)
    // the pair of bins through ONE call: the library's exp / sincospi spend a third of their instructions putting polynomial
    // coefficients into registers, and two evaluations inside one function share them
    const double a0 = x0.x / N, b0 = -x0.y / N * M_1_PI - delay_pi * (double)k;
    const double a1 = x1.x / N, b1 = -x1.y / N * M_1_PI - delay_pi * (double)(M - k);
    double4 cis;
    if constexpr (TAB) cis = cis_pair_tab_call(a0, b0, a1, b1, tw_base + 256, mt);
    else cis = cis_pair_call(a0, b0, a1, b1);
    double2 A = mul(k, make_double2(cis.x, cis.y)), B = mul(M - k, make_double2(cis.z, cis.w));
    if (k == 0) {  // DC and Nyquist bins: only their real parts reach a real output
      A.y = 0.0;
      B.y = 0.0;
    }
    // pre-pass of the inverse real transform (wh::irfft_lds) on the pair
    const double er = A.x + B.x, ei = A.y - B.y;
    const double dr = A.x - B.x, di = A.y + B.y;
    const double orr = fma(dr, wk.x, di * wk.y);
    const double oi = fma(di, wk.x, -(dr * wk.y));
    zb[k] = make_double2(er - oi, ei + orr);
    if (k != 0) zb[M - k] = make_double2(er + oi, orr - ei);
  }
  wh::sync<FT>();
  mp_fft<M, true, GT, FT, WAVE>(zb, tw_base + M);
}

// The same response from the EXPONENT of a transfer function that is minimum phase as it stands — a mel-cepstrum on a
// warped axis, H = exp(sum_j d[j] z~^-j) (wh_specfilter.hip, kind 2): no logarithm, no cepstral fold and none of the two
// forward transforms; only the tail of min_phase_response from its comment "minimum-phase spectrum" on.
//   `expo(k0, k1)`: (re_0, im_0, re_1, im_1), the exponents re - i im of the bins k0 and k1 = M - k0 (0 <= k <= N/2),
//   computed by the thread that owns the pair; bin k of the spectrum is exp(re) cis(-im), times mul(k, .).
//   in: zb is FREE (nobody reads it) and whatever mul reads is visible;  out: time-domain response N * h[n] in zr.
// (The lines from cis_pair_call to the inverse transform are min_phase_response's own, repeated here so that the chains
// of response_kernel and req_filter_kernel compile as they did: DESIGN section 23 names the merge as a follow-up.)
template <int N, int GT, class Expo, class Mul = SpectrumIdentity>
__device__ __forceinline__ void exponent_response(wh::ckp<double2> zb, wh::ckp<const double2> tw_base, Expo expo, Mul mul = Mul()) {
#pragma clang fp contract(fast)
  constexpr int FT = ft_syn(N);
  constexpr int M = N / 2;
  const int gt = WH_TID & (GT - 1);
  const wh::ckp<const double2> WH_RESTRICT w = tw_base + N;
#pragma unroll 1
  for (int k = gt; k <= M / 2; k += GT) {
    const double2 wk = wh::ldg2(w + k);
    const double4 e = expo(k, M - k);
    const double4 cis = cis_pair_call(e.x, -e.y * M_1_PI, e.z, -e.w * M_1_PI);
    double2 A = mul(k, make_double2(cis.x, cis.y)), B = mul(M - k, make_double2(cis.z, cis.w));
    if (k == 0) {  // DC and Nyquist bins: only their real parts reach a real output
      A.y = 0.0;
      B.y = 0.0;
    }
    // pre-pass of the inverse real transform (wh::irfft_lds) on the pair
    const double er = A.x + B.x, ei = A.y - B.y;
    const double dr = A.x - B.x, di = A.y + B.y;
    const double orr = fma(dr, wk.x, di * wk.y);
    const double oi = fma(di, wk.x, -(dr * wk.y));
    zb[k] = make_double2(er - oi, ei + orr);
    if (k != 0) zb[M - k] = make_double2(er + oi, orr - ei);
  }
  wh::sync<FT>();
  mp_fft<M, true, GT, FT, false>(zb, tw_base + M);
}

}  // namespace
