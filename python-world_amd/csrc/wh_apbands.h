// Band aperiodicity -> dense aperiodicity (world/d4c.py:45-59): the ONE place where the interpolation
//
//     10 ** (interp1d(coarse_axis, [-60, coarse..., -1e-12])(k * fs / fft_size) / 20),   coarse_axis = [0, fi, ..., nap fi, fs / 2]
//
// is written.  d4c_kernel (wh_d4c.hip: the tail of a frame) and ap_from_bands_kernel (wh_apbands.hip,
// wh_aperiodicity_from_bands: the expansion of a stored band aperiodicity) both evaluate it through these functions, in two
// translation units under one set of flags (build.py), so the expansion reproduces D4C's dense rows bit for bit.  Every function keeps `#pragma clang fp contract(off)`
// whatever the unit's setting: with a 0 dB band a fused slope * dx + y_lo can land an ulp ABOVE 0 dB, i.e. an
// aperiodicity above 1 (the reference's interpolation, d4c.py:58-59, is unfused NumPy).
#pragma once

namespace wh {

struct ApAxis {
  double fs;
  int nap;       // bands; nodes: 0, interval, ..., interval * nap, fs / 2
  int interval;  // Hz
  // k * fs / (2 (K-1)): the divisor is a power of two for every FFT size, so k * (fs / divisor) is the same double
  // (both roundings are of the exact quotient) without a divide per bin
  int qden;
  bool qexact;
  double qstep;
};

__host__ __device__ inline ApAxis ap_axis(double fs, int nap, int interval, int k_bins) {
  ApAxis ax;
  ax.fs = fs;
  ax.nap = nap;
  ax.interval = interval;
  ax.qden = 2 * (k_bins - 1);
  ax.qexact = (ax.qden & (ax.qden - 1)) == 0;
  ax.qstep = fs / (double)ax.qden;
  return ax;
}

__device__ __forceinline__ double ap_node(const ApAxis& ax, int m) { return m <= ax.nap ? (double)(m * ax.interval) : ax.fs / 2; }

// frequency of bin k
__device__ __forceinline__ double ap_bin_hz(const ApAxis& ax, int k) {
#pragma clang fp contract(off)
  return ax.qexact ? (double)k * ax.qstep : (double)k * ax.fs / (double)ax.qden;
}

// upper node of the segment that holds q: searchsorted-left over the coarse axis, clamped to [1, nap + 1]
__device__ __forceinline__ int ap_segment(const ApAxis& ax, double q) {
  const int nn = ax.nap + 2;
  int cnt = 0;
  for (int m = 0; m < nn; ++m) cnt += (ap_node(ax, m) < q) ? 1 : 0;
  return cnt < 1 ? 1 : (cnt > nn - 1 ? nn - 1 : cnt);
}

// slope of the segment below node hi, from its end values in dB
__device__ __forceinline__ double ap_slope(const ApAxis& ax, int hi, double y_lo, double y_hi) {
#pragma clang fp contract(off)
  return (y_hi - y_lo) / (ap_node(ax, hi) - ap_node(ax, hi - 1));
}

// the amplitude at q inside the segment below node hi
__device__ __forceinline__ double ap_value(const ApAxis& ax, int hi, double q, double slope, double y_lo) {
#pragma clang fp contract(off)
  const double db = slope * (q - ap_node(ax, hi - 1)) + y_lo;
  return exp(db * (M_LN10 / 20));  // 10^(db/20)
}

// dB value of node m: -60 at 0 Hz, -1e-12 at fs / 2, band(m - 1) — the value as coarse_ap stores it — in between
template <class Band>
__device__ __forceinline__ double ap_node_db(const ApAxis& ax, int m, Band&& band) {
  return m == 0 ? -60.0 : (m == ax.nap + 1 ? -0.000000000001 : band(m - 1));
}

// bin k of a frame whose band values are band(0 .. nap-1)
template <class Band>
__device__ __forceinline__ double ap_from_bands(const ApAxis& ax, int k, Band&& band) {
  const double q = ap_bin_hz(ax, k);
  const int hi = ap_segment(ax, q);
  const double y_lo = ap_node_db(ax, hi - 1, band);
  const double y_hi = ap_node_db(ax, hi, band);
  return ap_value(ax, hi, q, ap_slope(ax, hi, y_lo, y_hi), y_lo);
}

}  // namespace wh
