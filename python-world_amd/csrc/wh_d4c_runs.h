// The run-resident spectral helpers of d4c_frame (Runs<N>, wh_d4c_types.h: thread t owns the bins [t KR, (t + 1) KR) in
// registers): the low-band replica and the Hermitian-mirrored fill, the counterparts of wh_spectral.h's LDS forms.
// wh_d4c_runs_probe (wh_d4c_probe.hip) runs them on caller data.  Include after wh_d4c_types.h.
#pragma once

namespace wh {

// Mirror-add of the bins below f0 (wh::low_band_replica, d4c.py:213-220) for a run-resident array: the owners of
// the bins below `reach` publish them to tmp (LDS, >= 2*nlow doubles), the interpolated replica is evaluated by a
// thread-strided loop (a handful of bins; kept out of the unrolled per-run code, whose five copies of the divides and
// searches cost ~30 VGPRs of spills) and the owners add it to their registers.
template <int N>
__device__ __forceinline__ void low_band_replica_runs(double (&p)[Runs<N>::KR], wh::ckp<double> tmp, double fs, double f0,
                                                      double reach) {
  constexpr int FT = Runs<N>::FT, K = Runs<N>::K, KR = Runs<N>::KR;
  const int k0 = threadIdx.x * KR;
  int nlow = (int)(reach / fs * N) + 2;  // count of bins with k/N*fs < reach (monotone in k)
  if (nlow > K) nlow = K;                // (the reference indexes the half spectrum: bins beyond it do not exist)
  while (nlow > 0 && !(((double)(nlow - 1) / N * fs) < reach)) --nlow;
  const wh::ckp<double> add = tmp + ((nlow + 1) & ~1);
  // The bins below `reach` (1.2 f0 <= 960 Hz: a few dozen) all belong to the first lanes of wave 0.  When they fit one
  // wave — always, at the supported rates — that wave does the whole correction with wave-level ordering and the other
  // waves only meet it at the closing barrier: one barrier instead of three, and three waves skip the code.
  const bool one_wave = nlow <= 64 * KR;
  if (!one_wave || threadIdx.x < 64) {
#pragma unroll
    for (int r = 0; r < KR; ++r)
      if (k0 + r < nlow) tmp[k0 + r] = p[r];
    if (one_wave) wh::sync<64>(); else wh::sync<FT>();
#pragma unroll 1
    for (int kk = threadIdx.x; kk < nlow; kk += (one_wave ? 64 : FT)) {
      const double fk = (double)kk / N * fs;
      double inc = 0.0;
      if (nlow >= 2 && fk < f0) {
        // ascending nodes a_m = f0 - f_{nlow-1-m}; hi = clamp(#nodes < fk, 1, nlow-1).  The node predicate
        // a_m < fk is monotone in m, so the count is its boundary: estimated in closed form, then settled with
        // the exact floating-point predicate (the estimate is within one of the truth).
        auto below = [&](int mm) { return (f0 - ((double)(nlow - 1 - mm) / N * fs)) < fk; };
        int cnt = (int)ceil((double)(nlow - 1) - (f0 - fk) / fs * N);
        cnt = cnt < 0 ? 0 : (cnt > nlow ? nlow : cnt);
        while (cnt > 0 && !below(cnt - 1)) --cnt;
        while (cnt < nlow && below(cnt)) ++cnt;
        const int hi = cnt < 1 ? 1 : (cnt > nlow - 1 ? nlow - 1 : cnt);
        const int lo = hi - 1;
        const double a_lo = f0 - ((double)(nlow - 1 - lo) / N * fs);
        const double a_hi = f0 - ((double)(nlow - 1 - hi) / N * fs);
        const double y_lo = tmp[nlow - 1 - lo];
        const double y_hi = tmp[nlow - 1 - hi];
        const double slope = (y_hi - y_lo) / (a_hi - a_lo);
        inc = slope * (fk - a_lo) + y_lo;
      }
      add[kk] = inc;
    }
    if (one_wave) wh::sync<64>(); else wh::sync<FT>();
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      const int kk = k0 + r;
      if (kk < nlow && nlow >= 2 && ((double)kk / N * fs) < f0) p[r] = add[kk] + p[r];
    }
  }
  wh::sync<FT>();  // tmp is reused by the caller
}

// v[0..N) = Hermitian mirror of the run-resident half spectrum times fs/N (wh::fill_mirrored for runs).
template <int N>
__device__ __forceinline__ void fill_mirrored_runs(const double (&p)[Runs<N>::KR], wh::ckp<double> v, double fs) {
  constexpr int FT = Runs<N>::FT, K = Runs<N>::K, KR = Runs<N>::KR;
  const int k0 = threadIdx.x * KR;
  const double df = fs / N;
#pragma unroll
  for (int r = 0; r < KR; ++r) {
    const int k = k0 + r;
    if (k < K) {
      const double val = p[r] * df;
      v[k] = val;
      if (k > 0 && k < N / 2) v[N - k] = val;
    }
  }
  wh::sync<FT>();
}

}  // namespace wh
