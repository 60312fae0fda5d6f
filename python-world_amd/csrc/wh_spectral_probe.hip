// Test hook for the LDS forms of wh_spectral.h: wh_spectral_probe runs low_band_replica<FT>, or fill_mirrored<FT, N> followed
// by BandWindow::init / run<KR>, on caller data at CheapTrick's (N, FT) pairs, one frame per workgroup, with the LDS block
// laid out as cheaptrick_kernel lays it out.  Nothing in the library calls it (tests/test_hip_spectral_helpers.py does; the
// run-resident forms of wh_d4c_runs.h have wh_d4c_runs_probe).  Compiled with wh_cheaptrick.hip's flags (build.py), so the
// a * b + c of the interpolation and of the window's two fractional terms fuse here as they do there.
#include "wh_host.h"
#include "wh_spectral.h"

namespace {

// which 0: low_band_replica<FT>(aux, zr, N, fs, f0[c], rh[c]) -> aux;  1: fill_mirrored<FT, N>(aux -> zr), BandWindow(half = rh[c])
template <int N, int FT>
__global__ __launch_bounds__(FT) void spectral_probe_kernel(const double* __restrict__ in_, double* __restrict__ out_,
                                                            const double* __restrict__ f0_, const double* __restrict__ rh_,
                                                            int which, double fs, long long count) {
  constexpr int K = N / 2 + 1;
  constexpr int KR = (K + FT - 1) / FT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const wh::ckp<double> lds_all = wh::ck_make(reinterpret_cast<double*>(smem), (N + 2) + (K + 1) + 32, wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> zr = wh::ck_sub(lds_all, 0, N + 2, wh::WH_CK_LDS_MAIN);       // low-band scratch, then the mirrored spectrum
  const wh::ckp<double> aux = wh::ck_sub(lds_all, N + 2, K + 1, wh::WH_CK_LDS_AUX);  // the half spectrum
  const long long c = blockIdx.x;
  if (c >= count) return;
  const wh::ckp<const double> in = wh::ck_make(in_ + c * K, K, wh::WH_CK_IN);
  const wh::ckp<double> o = wh::ck_make(out_ + c * K, K, wh::WH_CK_OUT);
  for (int k = threadIdx.x; k < K; k += FT) aux[k] = in[k];
  wh::sync<FT>();
  const double rh = rh_[c];
  if (which == 0) {
    wh::low_band_replica<FT>(aux, zr, N, fs, f0_[c], rh);
    for (int k = threadIdx.x; k < K; k += FT) o[k] = aux[k];
  } else {
    wh::fill_mirrored<FT, N>(aux, zr, fs);
    const int k0 = threadIdx.x * KR;
    double bandv[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) bandv[r] = 0.0;
    // (a half-width outside [0, fs] is not a smoothing anyone runs, and its window would be walked bin by bin)
    if (rh >= 0.0 && rh <= fs) {
      wh::BandWindow bw;
      bw.init(zr, N, fs, rh);
      bw.run<KR>(k0, K, bandv);
    }
#pragma unroll
    for (int r = 0; r < KR; ++r)
      if (k0 + r < K) o[k0 + r] = bandv[r];
  }
}

}  // namespace

extern "C" int wh_spectral_probe(wh_ctx* ctx, void* stream, int n, int ft, int which, double fs, const double* f0,
                                 const double* reach_or_half, const double* in, double* out, int64_t count) {
  if (!ctx || !reach_or_half || !in || !out || count < 0 || count > 0x7fffffffLL || (which != 0 && which != 1) ||
      (which == 0 && !f0) || !(fs > 0))
    return wh::fail_msg("wh_spectral_probe", "bad argument");
  WH_ENTER(ctx);
  if (count == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  // cheaptrick_kernel's (N, FT): 128 threads up to N = 1024, 256 from N = 2048
  const auto kernel = n == 256 && ft == 128    ? spectral_probe_kernel<256, 128>
                      : n == 512 && ft == 128  ? spectral_probe_kernel<512, 128>
                      : n == 1024 && ft == 128 ? spectral_probe_kernel<1024, 128>
                      : n == 2048 && ft == 256 ? spectral_probe_kernel<2048, 256>
                      : n == 4096 && ft == 256 ? spectral_probe_kernel<4096, 256>
                                               : nullptr;
  if (!kernel)
    return wh::fail_msg("wh_spectral_probe", "shape (n, ft) not built: CheapTrick's (256 | 512 | 1024, 128) and (2048 | 4096, 256)");
  const size_t lds = sizeof(double) * ((n + 2) + (n / 2 + 2) + 32);
  if (int rc = wh::allow_lds(kernel, lds)) return rc;
  WH_LAUNCH_UNTIMED(st, "spectral_probe_kernel", kernel, dim3((unsigned)count), dim3(ft), lds, in, out, f0,
                    reach_or_half, which, fs, count);
  return 0;
}
