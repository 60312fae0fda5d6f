// Test hooks: sum_smallest (wh_d4c_select.h) and the run-resident helpers (wh_d4c_runs.h) on caller data
// (tests/test_hip_d4c_select.py, tests/test_hip_spectral_helpers.py).  Nothing in the library calls them.  One workgroup of
// ft_of(N) threads per row, the LDS block laid out as the front of d4c_frame's (d4c_lds_front: 2N doubles of transform
// buffer — work area / low-band scratch / mirrored spectrum —, 40 doubles of reduction scratch), the helpers instantiated
// with d4c_frame's own template arguments and compiled with wh_d4c.hip's flags (build.py).
#include "wh_d4c_types.h"
#include "wh_d4c_select.h"
#include "wh_d4c_runs.h"

namespace {
using namespace wh;

template <int N>
__global__ __launch_bounds__(ft_of(N)) void d4c_select_probe_kernel(const double* __restrict__ vals_, double* __restrict__ out_,
                                                                    int layout, int m, long long count) {
  constexpr int FT = Runs<N>::FT, K = Runs<N>::K;
  constexpr int MB = N / 2;
  constexpr int PJ = (MB / 2 + 1 + FT - 1) / FT;  // pair jobs per thread, as in the band stage
  static_assert((K + FT - 1) / FT <= 2 * PJ, "layout 1 needs ceil(K / FT) slots");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const wh::ckp<double> lds_all = wh::ck_make(reinterpret_cast<double*>(smem), d4c_lds_front(N), wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> zr = wh::ck_sub(lds_all, 0, 2 * N, wh::WH_CK_LDS_MAIN);
  const wh::ckp<double> scratch = wh::ck_sub(lds_all, 2 * N, 40, wh::WH_CK_LDS_SCRATCH);
  const long long c = blockIdx.x;
  if (c >= count) return;
  const wh::ckp<const double> v = wh::ck_make(vals_ + c * K, K, wh::WH_CK_IN);
  const wh::ckp<double> o = wh::ck_make(out_ + 2 * c, 2, wh::WH_CK_OUT);
  double px[2 * PJ];
  unsigned pvalid = 0;
#pragma unroll
  for (int q = 0; q < 2 * PJ; ++q) px[q] = 0.0;
  if (layout == 0) {
    // the band stage's own assignment: job i of thread t holds the bins t + i FT and N/2 - (t + i FT)
#pragma unroll
    for (int i = 0; i < PJ; ++i) {
      const int k = threadIdx.x + i * FT;
      if (k <= MB / 2) {
        px[2 * i] = v[k];
        pvalid |= 1u << (2 * i);
        if (k != MB - k) {  // (the middle bin pairs with itself; k = 0 pairs with N/2)
          px[2 * i + 1] = v[MB - k];
          pvalid |= 2u << (2 * i);
        }
      }
    }
  } else {
    // bin k on thread (K - 1 - k) % FT, slots filled in the order of k
    const int kfirst = (K - 1 - (int)threadIdx.x) % FT;
#pragma unroll
    for (int q = 0; q < 2 * PJ; ++q) {
      const int k = kfirst + q * FT;
      if (k < K) {
        px[q] = v[k];
        pvalid |= 1u << q;
      }
    }
  }
  double s_small, s_total;
  sum_smallest<K, FT, 2 * PJ>(px, pvalid, m, zr, scratch, &s_small, &s_total);
  if (threadIdx.x == 0) {
    o[0] = s_small;
    o[1] = s_total;
  }
}

// which 0: low_band_replica_runs(p, fs, f0[c], rh[c]) -> p;  1: fill_mirrored_runs(p), BandWindow(half = rh[c]) -> band
template <int N>
__global__ __launch_bounds__(ft_of(N)) void d4c_runs_probe_kernel(const double* __restrict__ in_, double* __restrict__ out_,
                                                                  const double* __restrict__ f0_, const double* __restrict__ rh_,
                                                                  int which, double fs, long long count) {
  constexpr int K = Runs<N>::K, KR = Runs<N>::KR;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const wh::ckp<double> lds_all = wh::ck_make(reinterpret_cast<double*>(smem), d4c_lds_front(N), wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> zr = wh::ck_sub(lds_all, 0, 2 * N, wh::WH_CK_LDS_MAIN);
  const long long c = blockIdx.x;
  if (c >= count) return;
  const wh::ckp<const double> in = wh::ck_make(in_ + c * K, K, wh::WH_CK_IN);
  const wh::ckp<double> o = wh::ck_make(out_ + c * K, K, wh::WH_CK_OUT);
  const int k0 = threadIdx.x * KR;
  double p[KR], res[KR];
#pragma unroll
  for (int r = 0; r < KR; ++r) p[r] = k0 + r < K ? in[k0 + r] : 0.0;
  const double rh = rh_[c];
  if (which == 0) {
    low_band_replica_runs<N>(p, zr, fs, f0_[c], rh);
#pragma unroll
    for (int r = 0; r < KR; ++r) res[r] = p[r];
  } else {
#pragma unroll
    for (int r = 0; r < KR; ++r) res[r] = 0.0;
    fill_mirrored_runs<N>(p, zr, fs);
    // (a half-width outside [0, fs] is not a smoothing anyone runs, and its window would be walked bin by bin)
    if (rh >= 0.0 && rh <= fs) {
      wh::BandWindow bw;
      bw.init(zr, N, fs, rh);
      bw.run<KR>(k0, K, res);
    }
  }
#pragma unroll
  for (int r = 0; r < KR; ++r)
    if (k0 + r < K) o[k0 + r] = res[r];
}
template <int N>
int launch_select_probe(hipStream_t st, int layout, int m, const double* vals, double* out, long long count) {
  const size_t lds = sizeof(double) * d4c_lds_front(N);
  if (int rc = wh::allow_lds(&d4c_select_probe_kernel<N>, lds)) return rc;
  return wh::launch_untimed(st, "d4c_select_probe_kernel", d4c_select_probe_kernel<N>, dim3((unsigned)count),
                            dim3(ft_of(N)), lds, vals, out, layout, m, count);
}

template <int N>
int launch_runs_probe(hipStream_t st, int which, double fs, const double* f0, const double* rh, const double* in, double* out,
                      long long count) {
  const size_t lds = sizeof(double) * d4c_lds_front(N);
  if (int rc = wh::allow_lds(&d4c_runs_probe_kernel<N>, lds)) return rc;
  return wh::launch_untimed(st, "d4c_runs_probe_kernel", d4c_runs_probe_kernel<N>, dim3((unsigned)count),
                            dim3(ft_of(N)), lds, in, out, f0, rh, which, fs, count);
}

}  // namespace

extern "C" int wh_d4c_select_probe(wh_ctx* ctx, void* stream, int n, int layout, int m, const double* vals, double* out,
                                   int64_t count) {
  if (!ctx || !vals || !out || count < 0 || count > 0x7fffffffLL || (layout != 0 && layout != 1))
    return wh::fail_msg("wh_d4c_select_probe", "bad argument");
  if (n != 512 && n != 1024 && n != 2048 && n != 4096 && n != 8192)
    return wh::fail_msg("wh_d4c_select_probe", "n must be one of D4C's transform lengths 512 ... 8192");
  if (m < 1 || m > n / 2) return wh::fail_msg("wh_d4c_select_probe", "m must lie in [1, K - 1] (at least one value is left out)");
  WH_ENTER(ctx);
  if (count == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  wh::dispatch_fft_size<8192>(n, [&](auto nn) { rc = launch_select_probe<decltype(nn)::value>(st, layout, m, vals, out, (long long)count); });
  return rc;
}

extern "C" int wh_d4c_runs_probe(wh_ctx* ctx, void* stream, int n, int which, double fs, const double* f0,
                                 const double* reach_or_half, const double* in, double* out, int64_t count) {
  if (!ctx || !reach_or_half || !in || !out || count < 0 || count > 0x7fffffffLL || (which != 0 && which != 1) ||
      (which == 0 && !f0) || !(fs > 0))
    return wh::fail_msg("wh_d4c_runs_probe", "bad argument");
  if (n != 512 && n != 1024 && n != 2048 && n != 4096 && n != 8192)
    return wh::fail_msg("wh_d4c_runs_probe", "n must be one of D4C's transform lengths 512 ... 8192");
  WH_ENTER(ctx);
  if (count == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  wh::dispatch_fft_size<8192>(n, [&](auto nn) { rc = launch_runs_probe<decltype(nn)::value>(st, which, fs, f0, reach_or_half, in, out, (long long)count); });
  return rc;
}
