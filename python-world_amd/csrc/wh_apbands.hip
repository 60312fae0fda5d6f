// Band aperiodicity <-> dense aperiodicity outside D4C: ap_from_bands_kernel expands stored band values to dense rows
// (wh_aperiodicity_from_bands; world/compact.py, world/regrid.py), ap_gate_kernel reads the voicing gate back off a dense
// row (wh_aperiodicity_gate).  The interpolation itself is wh_apbands.h, shared with d4c_kernel; this unit is compiled with
// wh_d4c.hip's flags (build.py), so the expansion reproduces D4C's dense rows bit for bit.
#include "wh_host.h"
#include "wh_device.h"
#include "wh_apbands.h"

namespace {

// ---- band aperiodicity -> dense aperiodicity (wh_aperiodicity_from_bands; d4c.py:45-59) ---------------------------
// A workgroup expands kApFrames consecutive frames.  Their nodes' dB values and the slopes of their segments go to LDS
// first (one division per frame and segment instead of one per bin; the quotient is the one d4c_kernel forms per bin,
// same operands, same unfused division: wh_apbands.h), then the threads walk the group's bins as PAIRS of the flat
// output: K is odd, so single rows are not 16-byte aligned, but an even number of rows is — every pair is one
// 16-byte store, whichever frames its two bins belong to.  The kernel is write-bound: 8 B out per bin against
// nap + 1 doubles in per frame.
constexpr int kApFrames = 8;
constexpr int kApThreads = 256;
constexpr int kApNodes = 10;  // nap + 2 <= 10

__device__ __forceinline__ double ap_bin_of_group(const wh::ApAxis& ax, int e, int k_bins, const wh::ckp<const double>& y,
                                                  const wh::ckp<const double>& sl, const wh::ckp<const int>& open_gate) {
  const int fr = e / k_bins;
  const int k = e - fr * k_bins;
  if (!open_gate[fr]) return 1 - 0.000000000001;  // d4c.py:50
  const double q = wh::ap_bin_hz(ax, k);
  const int hi = wh::ap_segment(ax, q);
  return wh::ap_value(ax, hi, q, sl[fr * kApNodes + hi], y[fr * kApNodes + hi - 1]);
}

template <bool VEC>
__global__ __launch_bounds__(kApThreads) void ap_from_bands_kernel(const double* __restrict__ coarse_,
                                                                   const double* __restrict__ gate_, double* __restrict__ out_,
                                                                   long long n_frames, int k_bins, wh::ApAxis ax) {
  __shared__ double s_y[kApFrames * kApNodes];
  __shared__ double s_sl[kApFrames * kApNodes];
  __shared__ int s_gate[kApFrames];
  const wh::ckp<double> y = wh::ck_make(s_y, kApFrames * kApNodes, wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> sl = wh::ck_make(s_sl, kApFrames * kApNodes, wh::WH_CK_LDS_OTHER);
  const wh::ckp<int> og = wh::ck_make(s_gate, kApFrames, wh::WH_CK_LDS_OTHER);
  const wh::ckp<const double> coarse = wh::ck_make(coarse_, n_frames * ax.nap, wh::WH_CK_IN);
  const wh::ckp<const double> gate = wh::ck_make(gate_, n_frames, wh::WH_CK_IN);
  const wh::ckp<double> out = wh::ck_make(out_, n_frames * k_bins, wh::WH_CK_OUT);
  const long long f0 = (long long)blockIdx.x * kApFrames;
  const int nf = (int)(n_frames - f0 < kApFrames ? n_frames - f0 : kApFrames);
  const int nn = ax.nap + 2;
  for (int i = threadIdx.x; i < nf * nn; i += kApThreads) {
    const int fr = i / nn, m = i - fr * nn;
    y[fr * kApNodes + m] = wh::ap_node_db(ax, m, [&](int b) { return coarse[(f0 + fr) * ax.nap + b]; });
    if (m == 0) og[fr] = gate[f0 + fr] != 0.0 ? 1 : 0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nf * (nn - 1); i += kApThreads) {
    const int fr = i / (nn - 1), hi = 1 + i - fr * (nn - 1);
    sl[fr * kApNodes + hi] = wh::ap_slope(ax, hi, y[fr * kApNodes + hi - 1], y[fr * kApNodes + hi]);
  }
  __syncthreads();
  const int n_el = nf * k_bins;
  const long long e0 = f0 * k_bins;  // (64-bit: 2 049 024 frames x 513 bins x 8 B is beyond 2^31 bytes)
  if constexpr (VEC) {
    const wh::ckp<double2> out2 = wh::ck_as<double2>(out);  // f0 * k_bins is even: kApFrames is
    for (int e = 2 * threadIdx.x; e < n_el; e += 2 * kApThreads) {
      const double v0 = ap_bin_of_group(ax, e, k_bins, y, sl, og);
      if (e + 1 < n_el) {
        const double v1 = ap_bin_of_group(ax, e + 1, k_bins, y, sl, og);
        out2[(e0 + e) >> 1] = make_double2(v0, v1);
      } else {
        out[e0 + e] = v0;  // the last bin of a batch with an odd number of frames
      }
    }
  } else {  // an output that does not start on a 16-byte boundary
    for (int e = threadIdx.x; e < n_el; e += kApThreads) out[e0 + e] = ap_bin_of_group(ax, e, k_bins, y, sl, og);
  }
}

// gate[f] = 1 where row f of a dense aperiodicity came from the bands, 0 where D4C's voicing gate wrote the constant
// row: bin 0 holds 1 - 1e-12 there and 10^(-60/20) = 1e-3 everywhere else, so the comparison with 0.5 is exact
__global__ __launch_bounds__(256) void ap_gate_kernel(const double* __restrict__ ap_, double* __restrict__ gate_,
                                                      long long n_frames, int k_bins) {
  const wh::ckp<const double> ap = wh::ck_make(ap_, n_frames * k_bins, wh::WH_CK_IN);
  const wh::ckp<double> gate = wh::ck_make(gate_, n_frames, wh::WH_CK_OUT);
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f < n_frames) gate[f] = ap[f * k_bins] > 0.5 ? 0.0 : 1.0;
}

}  // namespace

extern "C" int wh_aperiodicity_from_bands(wh_ctx* ctx, void* stream, int64_t n_frames, int nap, int k_bins, double fs,
                                          int frequency_interval, const double* coarse, const double* gate,
                                          double* out) {
  if (!ctx) return wh::fail_msg("wh_aperiodicity_from_bands", "null argument");
  WH_ENTER(ctx);
  if (n_frames < 0) return wh::fail_msg("wh_aperiodicity_from_bands", "negative frame count");
  if (nap < 1 || nap > 8) return wh::fail_msg("wh_aperiodicity_from_bands", "1 to 8 aperiodicity bands supported");
  if (k_bins < 2 || k_bins > 16385) return wh::fail_msg("wh_aperiodicity_from_bands", "k_bins out of range");
  if (!(fs > 0) || frequency_interval <= 0 || !((double)nap * frequency_interval < fs / 2))
    return wh::fail_msg("wh_aperiodicity_from_bands", "the coarse axis 0, fi, ..., nap fi, fs/2 must be increasing");
  if (n_frames == 0) return 0;
  if (!coarse || !gate || !out) return wh::fail_msg("wh_aperiodicity_from_bands", "null argument");
  hipStream_t st = (hipStream_t)stream;
  const long long groups = (n_frames + kApFrames - 1) / kApFrames;
  if (groups > 0x7fffffffLL) return wh::fail_msg("wh_aperiodicity_from_bands", "too many frames for one launch");
  const wh::ApAxis ax = wh::ap_axis(fs, nap, frequency_interval, k_bins);
  const bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  WH_LAUNCH(ctx, st, "ap_from_bands_kernel", vec ? ap_from_bands_kernel<true> : ap_from_bands_kernel<false>,
            dim3((unsigned)groups), dim3(kApThreads), 0, coarse, gate, out, n_frames, k_bins, ax);
  return 0;
}

extern "C" int wh_aperiodicity_gate(wh_ctx* ctx, void* stream, int64_t n_frames, int k_bins, const double* aperiodicity,
                                    double* gate) {
  if (!ctx) return wh::fail_msg("wh_aperiodicity_gate", "null argument");
  WH_ENTER(ctx);
  if (n_frames < 0 || k_bins < 1) return wh::fail_msg("wh_aperiodicity_gate", "bad shape");
  if (n_frames == 0) return 0;
  if (!aperiodicity || !gate) return wh::fail_msg("wh_aperiodicity_gate", "null argument");
  hipStream_t st = (hipStream_t)stream;
  const long long blocks = (n_frames + 255) / 256;
  WH_LAUNCH(ctx, st, "ap_gate_kernel", ap_gate_kernel, dim3((unsigned)blocks), dim3(256), 0, aperiodicity, gate,
            n_frames, k_bins);
  return 0;
}
