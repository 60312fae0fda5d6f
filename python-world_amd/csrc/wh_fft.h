// The FFT engine (gfx950, wave64, FP64).
//  * fft_lds<N>            : in-place complex FP64 Stockham FFT on an LDS-resident buffer.  Every pass pulls
//    its radix-8 / 4 / 2 operands into registers, barriers, and writes the auto-sorted outputs back into the
//    same buffer, so no ping-pong copy is needed and a 4096-point transform fits 64 KiB of the CU's 160 KiB
//    LDS; intermediate layouts are XOR-swizzled against store bank conflicts; fft_lds_from_regs feeds the
//    first pass from registers; rfft_lds / irfft_lds do real transforms through half-size complex ones.
// The twiddle tables' geometry (fft_ptw_offset, WH_TWIDDLE_ENTRIES) is in wh_device.h, with WH_MAX_FFT: host code sizes
// d_twiddle from it without reading the passes.  The thread index is WH_TID (wh_device.h): a unit that defines it
// opaquely (wh_tid.h, wh_d4c_types.h) does so before this header is read.
#pragma once
#include "wh_device.h"

namespace wh {

// ------------------------------------------------------------------------------------------
// FFT
// ------------------------------------------------------------------------------------------
// complex multiply with fused multiply-adds (2 mul + 2 fma instead of 4 mul + 2 add)
__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x));
}
// a * conj(b): the same roundings as cmul(a, (b.x, -b.y)), the negations riding on the operands
__device__ __forceinline__ double2 cmul_conj(double2 a, double2 b) {
  return make_double2(fma(a.x, b.x, a.y * b.y), fma(-a.x, b.y, a.y * b.x));
}

// In-place Stockham passes of radix 8 (then 4 or 2 for what is left of N), NT threads on one N-point buffer.
//
// LDS cost model (MI355X_MICROARCH.md, LDS): a ds_write_b128 costs ~13 cycles per wave against 4 for a
// ds_read_b128, and stores are serviced in groups of 8 consecutive lanes over a 128-byte bank row — so the
// transforms are priced in *stores*: radix 8 needs 4 passes for 2048 points where radix 4 needs 6, and the
// scattered stores of the early passes (lane stride R complex values: every lane of a group on the same 16-byte
// slot) are made conflict-free by an XOR swizzle of the intermediate layout, element i living at
// i ^ ((i >> 3) & 7).  The swizzle is internal: the first pass reads and the last pass writes natural order.
//
// tw[i] = exp(-2*pi*i*sqrt(-1)/N), i in [0,N).  INV conjugates twiddles and butterflies.
// SNT >= NT: the barrier spans SNT threads while NT of them (thread index modulo NT) cooperate on this buffer,
// so that SNT/NT independent transforms on different buffers advance in lockstep through the same barriers.

// index of element i in the swizzled intermediate layout
__device__ __forceinline__ int fft_swz(int i) { return i ^ ((i >> 3) & 7); }

__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
// multiply by -i (forward) / +i (inverse)
template <bool INV>
__device__ __forceinline__ double2 crot(double2 a) {
  return INV ? make_double2(-a.y, a.x) : make_double2(a.y, -a.x);
}

// R-point DFT of v[0..R) in place, natural order out.
template <int R, bool INV>
__device__ __forceinline__ void dft_small(double2 (&v)[R]) {
  if constexpr (R == 2) {
    const double2 a = v[0], b = v[1];
    v[0] = cadd(a, b);
    v[1] = csub(a, b);
  } else if constexpr (R == 4) {
    const double2 e0 = cadd(v[0], v[2]), e1 = csub(v[0], v[2]);
    const double2 e2 = cadd(v[1], v[3]), e3 = crot<INV>(csub(v[1], v[3]));
    v[0] = cadd(e0, e2);
    v[1] = cadd(e1, e3);
    v[2] = csub(e0, e2);
    v[3] = csub(e1, e3);
  } else {
    static_assert(R == 8, "radix");
    constexpr double h = 0.70710678118654752440;
    double2 a[4], b[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      a[r] = cadd(v[r], v[r + 4]);
      b[r] = csub(v[r], v[r + 4]);
    }
    // b1 *= W8, b2 *= W8^2 = -i, b3 *= W8^3   (W8 = exp(-i*pi/4); conjugated for the inverse)
    b[1] = INV ? make_double2(h * (b[1].x - b[1].y), h * (b[1].x + b[1].y))
               : make_double2(h * (b[1].x + b[1].y), h * (b[1].y - b[1].x));
    b[2] = crot<INV>(b[2]);
    b[3] = INV ? make_double2(-h * (b[3].x + b[3].y), h * (b[3].x - b[3].y))
               : make_double2(h * (b[3].y - b[3].x), -h * (b[3].x + b[3].y));
    dft_small<4, INV>(a);
    dft_small<4, INV>(b);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[2 * r] = a[r];
      v[2 * r + 1] = b[r];
    }
  }
}

// Radix of the pass that follows NS: 8 while that leaves at least half of the NT threads a butterfly (a 512-point
// transform on 256 threads is faster as 4-4-4-4-2 on 128 lanes than as 8-8-8 on 64: its passes are latency-,
// not throughput-bound), else 4, else 2.
// MAXR caps the radix for a kernel whose register budget is set elsewhere (radix-4 butterflies hold half as many
// operands).  No kernel caps it today — d4c_kernel, the last to, settled on radix 8 at every length —; the radix-4 plans
// stay built and tested as engine functions (wh_fft_probe.hip).
template <int N, int NT, int NS, int MAXR = 8>
struct FftRadix {
  static constexpr int value = (MAXR >= 8 && NS * 8 <= N && N / 8 >= NT / 2) ? 8 : (NS * 4 <= N ? 4 : 2);
};

// Twiddle, butterfly and store of one pass for the butterflies this thread owns: v[p][r] = element
// j + r*(N/R), j = tid + p*NT.
template <int N, int NT, int R, int NS, bool INV, bool SWZ_OUT>
__device__ __forceinline__ void fft_pass_finish(ckp<double2> WH_RESTRICT s, double2 (&v)[(N / R + NT - 1) / NT][R],
                                                const double2 (&w)[(N / R + NT - 1) / NT][R]) {
  constexpr int J = N / R;
  constexpr int PER = (J + NT - 1) / NT;
  const int tid = WH_TID & (NT - 1);
#pragma unroll
  for (int p = 0; p < PER; ++p) {
    const int j = tid + p * NT;
    if (J % NT == 0 || j < J) {
      const int k = j & (NS - 1);
      if (NS > 1) {
#pragma unroll
        for (int r = 1; r < R; ++r) v[p][r] = INV ? cmul_conj(v[p][r], w[p][r]) : cmul(v[p][r], w[p][r]);
      }
      dft_small<R, INV>(v[p]);
      const int base = (j - k) * R + k;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int o = base + r * NS;
        s[SWZ_OUT ? (NS % 64 == 0 ? fft_swz(base) + r * NS : fft_swz(o)) : o] = v[p][r];
      }
    }
  }
}

// The twiddles of one pass (global table, L1/L2 resident): fetched before the pass's barrier so that their
// latency is spent waiting for the other waves.
template <int N, int NT, int R, int NS, bool INV>
__device__ __forceinline__ void fft_pass_twiddles(ckp<const double2> WH_RESTRICT tw, double2 (&w)[(N / R + NT - 1) / NT][R]) {
  constexpr int J = N / R;
  constexpr int PER = (J + NT - 1) / NT;
  const int tid = WH_TID & (NT - 1);
  if (NS > 1) {
    static_assert(NS * R <= WH_MAX_FFT, "pass twiddle tables stop at WH_MAX_FFT");
    const ckp<const double2> pt = tw + (fft_ptw_offset(NS * R, R) - N);  // tw: the size-N table, at offset N
#pragma unroll
    for (int p = 0; p < PER; ++p) {
      const int j = tid + p * NT;
      if (J % NT == 0 || j < J) {
        const int k = j & (NS - 1);
#pragma unroll
        for (int r = 1; r < R; ++r) {
          // as stored: the inverse transform's conjugation is folded into the multiply (fft_pass_finish) — negating
          // here made every load's wait come right behind it, in front of the pass's LDS reads instead of under them
          w[p][r] = ldg2(pt + (k * (R - 1) + r - 1));
        }
      }
    }
  }
}

template <int N, int NT, int R, int NS, bool INV, int SNT, bool SWZ_IN, bool SWZ_OUT>
__device__ __forceinline__ void fft_pass(ckp<double2> WH_RESTRICT s, ckp<const double2> WH_RESTRICT tw) {
  constexpr int J = N / R;
  constexpr int PER = (J + NT - 1) / NT;
  double2 v[PER][R], w[PER][R];
  const int tid = WH_TID & (NT - 1);
  fft_pass_twiddles<N, NT, R, NS, INV>(tw, w);  // (behind the barrier instead, the loads' latency is the pass's own)
#pragma unroll
  for (int p = 0; p < PER; ++p) {
    const int j = tid + p * NT;
    if (J % NT == 0 || j < J) {
#pragma unroll
      for (int r = 0; r < R; ++r)
        v[p][r] = s[SWZ_IN ? (J % 64 == 0 ? fft_swz(j) + r * J : fft_swz(j + r * J)) : j + r * J];
    }
  }
  sync_lds<SNT>();
  fft_pass_finish<N, NT, R, NS, INV, SWZ_OUT>(s, v, w);
  sync_lds<SNT>();
}

template <int N, int NT, int NS, bool INV, int SNT = NT, int MAXR = 8>
__device__ __forceinline__ void fft_passes(ckp<double2> s, ckp<const double2> tw) {
  if constexpr (NS < N) {
    constexpr int R = FftRadix<N, NT, NS, MAXR>::value;
    constexpr bool SWZ = N >= 64 && MAXR >= 8;  // radix-4 plans keep the natural layout (one address VGPR per pass)
    fft_pass<N, NT, R, NS, INV, SNT, SWZ && (NS > 1), SWZ && (NS * R < N)>(s, tw);
    fft_passes<N, NT, NS * R, INV, SNT, MAXR>(s, tw);
  }
}

// In-place unnormalised DFT of N complex doubles resident in LDS.  Caller guarantees that the
// buffer is fully written and visible (barrier) on entry; visible on exit.  The inverse does
// NOT divide by N.
template <int N, bool INV, int NT = WH_BLOCK, int SNT = NT, int MAXR = 8>
__device__ __forceinline__ void fft_lds(ckp<double2> s, ckp<const double2> tw) {
  fft_passes<N, NT, 1, INV, SNT, MAXR>(s, tw);
}

// The same transform by ONE wave of a GT-thread group: a 512-point transform is exactly 64 radix-8 butterflies per
// pass, so the wave that the workgroup-wide plan (fft_lds<512, .., 128, ..>) left alone with the butterflies anyway
// owns all of them, and its passes are ordered by wavefront fences instead of two s_barrier each (6 per transform).
// The group's other waves go straight to the one barrier at the end, which spans SNT threads like fft_lds's and makes
// the result visible to all of them.  Where fft_lds<N, INV, GT> runs 8-8-8 (GT <= 128 at N = 512) this is the same plan,
// layout and twiddles: the same bits; a 256-thread group's 4-4-4-4-2 plan rounds differently (ulps).
// Feature macro for tools/ubench/fft_plans.hip only: its -DFFT_HEADER A/B builds against older revisions of this header,
// which lack fft_lds_wave; nothing in the library tests it.
#define WH_HAVE_FFT_WAVE 1
template <int N, bool INV, int GT, int SNT = GT>
__device__ __forceinline__ void fft_lds_wave(ckp<double2> s, ckp<const double2> tw) {
  static_assert(N / 8 <= WH_WAVE && GT % WH_WAVE == 0 && SNT % GT == 0, "one wave must own a pass's butterflies");
  if ((WH_TID & (GT - 1)) < WH_WAVE) fft_lds<N, INV, WH_WAVE, WH_WAVE>(s, tw);
  sync_lds<SNT>();
}
// The same with a job for the waves that own no butterflies: side(i, n) runs on them while the first wave transforms,
// i = 0 .. n - 1 numbering the n = (SNT / GT) (GT - 64) such threads of the SNT-thread workgroup (all of its groups are
// expected here at the same time).  side() may write LDS that the transform does not touch — the closing barrier makes
// it visible with the transform's result — and must not synchronise: the first waves do not go with it.
template <int N, bool INV, int GT, int SNT, class Side>
__device__ __forceinline__ void fft_lds_wave(ckp<double2> s, ckp<const double2> tw, Side side) {
  static_assert(N / 8 <= WH_WAVE && GT % WH_WAVE == 0 && GT > WH_WAVE && SNT % GT == 0, "one wave owns the butterflies, the others the side job");
  const int gt = WH_TID & (GT - 1);
  if (gt < WH_WAVE) fft_lds<N, INV, WH_WAVE, WH_WAVE>(s, tw);
  else side((int)(WH_TID / GT) * (GT - WH_WAVE) + gt - WH_WAVE, (SNT / GT) * (GT - WH_WAVE));
  sync_lds<SNT>();
}

// The same transform with the input still in registers: x[q] = element tid + q*NT, q < N/NT (the layout a
// thread-strided producer loop leaves behind).  When N >= R*NT (R the first radix) those are exactly the operands
// of this thread's first-pass butterflies, so the input never makes the trip through LDS.  The buffer must be
// free (no other thread still reading it): a barrier is taken on entry.
template <int N, bool INV, int NT = WH_BLOCK, int MAXR = 8>
__device__ __forceinline__ void fft_lds_from_regs(const double2 (&x)[N / NT], ckp<double2> s, ckp<const double2> tw) {
  constexpr int R = FftRadix<N, NT, 1, MAXR>::value;
  static_assert(N % (R * NT) == 0 && N >= 64, "register-fed first pass needs N >= R*NT");
  constexpr int PER = N / R / NT;
  double2 v[PER][R], w[PER][R];
#pragma unroll
  for (int p = 0; p < PER; ++p)
#pragma unroll
    for (int r = 0; r < R; ++r) v[p][r] = x[p + r * PER];
  sync_lds<NT>();
  fft_pass_finish<N, NT, R, 1, INV, (R < N && MAXR >= 8)>(s, v, w);
  sync_lds<NT>();
  fft_passes<N, NT, R, INV, NT, MAXR>(s, tw);
}

// ------------------------------------------------------------------------------------------
// Real-input / real-output transforms through a half-size complex FFT
// ------------------------------------------------------------------------------------------
// Every WORLD transform is of real data or produces real data, so an N-point transform is done as an
// N/2-point complex FFT on the sample pairs (x[2j], x[2j+1]) plus one O(N) butterfly pass: half the
// butterflies and half the LDS of a complex N-point FFT.  tw_base is the context's table base: the table of
// size M (exp(-2*pi*i*k/M), k < M) lives at tw_base + M.

// Forward.  in: z[j] = (x[2j], x[2j+1]), j < N/2 (i.e. the real array itself).  out: z[k] = X[k], k = 0..N/2
// (N/2 + 1 entries).  Buffer must be visible on entry; visible on exit.
template <int N, int NT = WH_BLOCK, int SNT = NT, int MAXR = 8>
__device__ __forceinline__ void rfft_lds(ckp<double2> z, ckp<const double2> WH_RESTRICT tw_base) {
  fft_lds<N / 2, false, NT, SNT, MAXR>(z, tw_base + N / 2);
  ckp<const double2> WH_RESTRICT w = tw_base + N;
  for (int k = WH_TID & (NT - 1); k <= N / 4; k += NT) {
    if (k == 0) {
      const double2 a = z[0];
      z[0] = make_double2(a.x + a.y, 0.0);
      z[N / 2] = make_double2(a.x - a.y, 0.0);
    } else {
      const double2 a = z[k], b = z[N / 2 - k];
      const double er = 0.5 * (a.x + b.x), ei = 0.5 * (a.y - b.y);  // E = (A + conj(B))/2   (even samples)
      const double dr = 0.5 * (a.x - b.x), di = 0.5 * (a.y + b.y);  // D = (A - conj(B))/2 ; O = -i*D (odd samples)
      const double2 wk = ldg2(w + k);
      const double tr = fma(wk.x, di, wk.y * dr);   // T = W^k * O,  O = (di, -dr)
      const double ti = fma(wk.y, di, -(wk.x * dr));
      z[k] = make_double2(er + tr, ei + ti);
      z[N / 2 - k] = make_double2(er - tr, ti - ei);  // conj(E - T)
    }
  }
  sync_lds<SNT>();
}

// The forward real transform of one analysis frame that stands beside a minimum-phase chain (wh_minphase.h): the frame
// filters of recordings take it from here.  Only the (N, NT) pairs of that chain — 256 threads up to N = 1024, 512 beyond,
// the shapes the Requiem filter instantiates rfft_lds with and csrc/wh_fft_probe.hip runs (kind 2) — can be instantiated,
// so a caller of this name cannot bring a transform shape into the library that the engine's tests do not run.
template <int N, int NT>
__device__ __forceinline__ void rfft_frame_lds(ckp<double2> z, ckp<const double2> WH_RESTRICT tw_base) {
  static_assert((N == 512 && NT == 256) || (N == 1024 && NT == 256) || (N == 2048 && NT == 512) || (N == 4096 && NT == 512),
                "a shape of the minimum-phase chains: add any other to WH_PROBE_SHAPES and tests/test_hip_fft_engine.py first");
  rfft_lds<N, NT>(z, tw_base);
}

// Inverse.  in: z[k] = X[k], k = 0..N/2: the half spectrum; the result is Re(IDFT) of its Hermitian extension
// (imaginary parts of the DC / Nyquist bins are ignored, as taking .real of a full complex IFFT would).
// out: z[j] = N * (x[2j], x[2j+1]), j < N/2 (unnormalised like fft_lds<.., true>: divide by N).
template <int N, int NT = WH_BLOCK, int SNT = NT, int MAXR = 8>
__device__ __forceinline__ void irfft_lds(ckp<double2> z, ckp<const double2> WH_RESTRICT tw_base) {
  ckp<const double2> WH_RESTRICT w = tw_base + N;
  for (int k = WH_TID & (NT - 1); k <= N / 4; k += NT) {
    double2 a = z[k], b = z[N / 2 - k];
    if (k == 0) {  // DC and Nyquist bins: only their real parts reach a real output (Re of the inverse DFT)
      a.y = 0.0;
      b.y = 0.0;
    }
    const double er = a.x + b.x, ei = a.y - b.y;  // 2E = A + conj(B)
    const double dr = a.x - b.x, di = a.y + b.y;  // 2D = A - conj(B)
    const double2 wk = ldg2(w + k);
    const double orr = fma(dr, wk.x, di * wk.y);     // 2O = 2D * conj(W^k),  conj(wk) = (wk.x, -wk.y)
    const double oi = fma(di, wk.x, -(dr * wk.y));
    z[k] = make_double2(er - oi, ei + orr);                      // Z[k]     = 2E + i*2O
    if (k != 0) z[N / 2 - k] = make_double2(er + oi, orr - ei);  // Z[N/2-k] = conj(2E) + i*conj(2O)
  }
  sync_lds<SNT>();
  fft_lds<N / 2, true, NT, SNT, MAXR>(z, tw_base + N / 2);
}


}  // namespace wh
