// Test hooks for the shared transform engine of wh_fft.h: wh_fft_engine_probe runs fft_lds / fft_lds_from_regs / rfft_lds /
// irfft_lds / fft_lds_wave on caller data at the (N, NT, SNT, MAXR, direction) shapes the kernels instantiate them with, one transform per
// NT-thread group of an SNT-thread workgroup; wh_twiddle_read copies the context's twiddle block to the host.  Nothing in
// the library calls either (tests/test_hip_fft_engine.py does).  Compiled with the spectral units' flags (build.py): the
// complex products of the passes fuse here as they do in CheapTrick, D4C and the response chains.
#include "wh_fft.h"
#include "wh_host.h"

namespace {

// kind: 0 fft_lds<N, INV, NT, SNT, MAXR>          N complex          -> N complex
//       1 fft_lds_from_regs<N, false, NT, MAXR>   N complex          -> N complex   (x[q] = element tid + q * NT)
//       2 rfft_lds<N, NT, SNT, MAXR>              N reals            -> N / 2 + 1 complex
//       3 irfft_lds<N, NT, SNT, MAXR>             N / 2 + 1 complex  -> N reals, unnormalised
//       4 fft_lds_wave<N, INV, NT, SNT>           N complex          -> N complex   (the first wave of each NT-thread group)
template <int KIND, int N>
struct ProbeShape {
  static constexpr bool REAL = KIND == 2 || KIND == 3;
  static constexpr int NB = REAL ? N / 2 + 1 : N;                             // double2 per LDS buffer
  static constexpr int IN_D = KIND == 2 ? N : KIND == 3 ? N + 2 : 2 * N;     // doubles per transform, in
  static constexpr int OUT_D = KIND == 2 ? N + 2 : KIND == 3 ? N : 2 * N;    // and out
};

template <int KIND, int N, int NT, int SNT, int MAXR, bool INV>
__global__ __launch_bounds__(SNT) void fft_engine_probe_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                              const double2* __restrict__ tw_base, long long count) {
  using S = ProbeShape<KIND, N>;
  static_assert(SNT % NT == 0 && (KIND != 1 || SNT == NT), "groups per workgroup");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int g = threadIdx.x / NT, t = threadIdx.x % NT;
  const long long b = (long long)blockIdx.x * (SNT / NT) + g;
  const bool live = b < count;  // (the buffers of a half-filled last workgroup are zero and go through the same barriers)
  const wh::ckp<double2> lds = wh::ck_make(reinterpret_cast<double2*>(smem), (long long)S::NB * (SNT / NT), wh::WH_CK_LDS_OTHER);
  const wh::ckp<double2> s = wh::ck_sub(lds, (long long)g * S::NB, S::NB, wh::WH_CK_LDS_MAIN);
  const wh::ckp<double> sr = wh::ck_as<double>(s);
  const wh::ckp<const double2> tw = wh::ck_make(tw_base, WH_TWIDDLE_ENTRIES, wh::WH_CK_TWIDDLE);
  if constexpr (KIND == 1) {
    double2 x[N / NT];
#pragma unroll
    for (int q = 0; q < N / NT; ++q) {
      const long long i = 2 * (b * N + t + q * NT);
      x[q] = live ? make_double2(in[i], in[i + 1]) : make_double2(0.0, 0.0);
    }
    wh::fft_lds_from_regs<N, false, NT, MAXR>(x, s, tw + N);
  } else {
    for (int i = t; i < 2 * S::NB; i += NT) sr[i] = (live && i < S::IN_D) ? in[b * S::IN_D + i] : 0.0;
    __syncthreads();
    if constexpr (KIND == 0) wh::fft_lds<N, INV, NT, SNT, MAXR>(s, tw + N);
    else if constexpr (KIND == 2) wh::rfft_lds<N, NT, SNT, MAXR>(s, tw);
    else if constexpr (KIND == 3) wh::irfft_lds<N, NT, SNT, MAXR>(s, tw);
    else wh::fft_lds_wave<N, INV, NT, SNT>(s, tw + N);
  }
  if (live)
    for (int i = t; i < S::OUT_D; i += NT) out[b * S::OUT_D + i] = sr[i];
}

template <int KIND, int N, int NT, int SNT, int MAXR, bool INV>
int launch_probe(wh_ctx* ctx, hipStream_t st, const double* in, double* out, long long count) {
  constexpr int per = SNT / NT;
  constexpr size_t lds = sizeof(double2) * (size_t)ProbeShape<KIND, N>::NB * per;
  static_assert(lds <= 160 * 1024, "one workgroup's buffers must fit the CU's LDS");
  auto kernel = fft_engine_probe_kernel<KIND, N, NT, SNT, MAXR, INV>;
  if (int rc = wh::allow_lds(kernel, lds)) return rc;
  return wh::launch_untimed(st, "fft_engine_probe_kernel", kernel, dim3((unsigned)((count + per - 1) / per)), dim3(SNT),
                            lds, in, out, ctx->d_twiddle, count);
}

}  // namespace

// The shapes that are built: X(kind, n, nt, snt, maxr, inverse), n the template argument N of the function (kinds 2 and 3:
// twice the complex size).  Read off the call sites (tests/test_fft_reference_host.py counts them: a new one adds its
// shapes here and to SHAPES of tests/test_hip_fft_engine.py).
#define WH_PROBE_FWD_INV(X, n, nt, snt, maxr) X(0, n, nt, snt, maxr, 0) X(0, n, nt, snt, maxr, 1)
#define WH_PROBE_SHAPES(X)                                                                                              \
  /* fft_lds.  CheapTrick (FT 128, 256 from 2048 real points on), forward and inverse */                                \
  WH_PROBE_FWD_INV(X, 128, 128, 128, 8) WH_PROBE_FWD_INV(X, 256, 128, 128, 8) WH_PROBE_FWD_INV(X, 512, 128, 128, 8)     \
  WH_PROBE_FWD_INV(X, 1024, 256, 256, 8) WH_PROBE_FWD_INV(X, 2048, 256, 256, 8)                                         \
  /* the synthesis chains: two in lockstep (FT = 2 GT), and one alone; D4C runs the forward ones of the second row too */ \
  WH_PROBE_FWD_INV(X, 256, 128, 256, 8) WH_PROBE_FWD_INV(X, 512, 128, 256, 8) WH_PROBE_FWD_INV(X, 1024, 256, 512, 8)    \
  WH_PROBE_FWD_INV(X, 2048, 256, 512, 8)                                                                                \
  WH_PROBE_FWD_INV(X, 256, 256, 256, 8) WH_PROBE_FWD_INV(X, 512, 256, 256, 8) WH_PROBE_FWD_INV(X, 1024, 512, 512, 8)    \
  WH_PROBE_FWD_INV(X, 2048, 512, 512, 8)                                                                                \
  /* D4C at 4096 and 8192 points; the band filters' 4096-point inverse on 256 threads (wh_bands.h) */                   \
  X(0, 4096, 512, 512, 8, 0) X(0, 8192, 512, 512, 8, 0) X(0, 4096, 256, 256, 8, 1)                                      \
  /* what fft_lds_wave runs on its one wave; the workgroup-wide twin of the register-fed (1024, 128) */                 \
  WH_PROBE_FWD_INV(X, 512, 64, 64, 8) X(0, 1024, 128, 128, 8, 0)                                                        \
  /* the radix-4 plans (MAXR = 4, natural layout; no caller today): D4C's fft_lds and rfft_lds shapes */                \
  X(0, 2048, 256, 256, 4, 0) X(0, 4096, 512, 512, 4, 0) X(0, 8192, 512, 512, 4, 0)                                      \
  X(2, 4096, 256, 256, 4, 0) X(2, 8192, 512, 512, 4, 0) X(2, 16384, 512, 512, 4, 0)                                     \
  /* fft_lds_wave: response_kernel<1024>'s chains (GT 128 and 256 in a 256-thread workgroup), and a one-wave workgroup */ \
  X(4, 512, 128, 256, 8, 0) X(4, 512, 128, 256, 8, 1) X(4, 512, 256, 256, 8, 0) X(4, 512, 256, 256, 8, 1)               \
  X(4, 512, 64, 64, 8, 0) X(4, 512, 64, 64, 8, 1)                                                                       \
  /* fft_lds_from_regs: D4C's windows, N == 8 FT */                                                                     \
  X(1, 1024, 128, 128, 8, 0) X(1, 2048, 256, 256, 8, 0) X(1, 4096, 512, 512, 8, 0)                                      \
  /* rfft_lds.  SWIPE' (WS = 64 ... 16384 on min(WS / 2, 256) threads), CheapTrick, D4C, the love-train gate (half of D4C's \
     threads, 64 at least), the Requiem filter */                                                                       \
  X(2, 64, 32, 32, 8, 0) X(2, 128, 64, 64, 8, 0) X(2, 256, 128, 128, 8, 0) X(2, 512, 128, 128, 8, 0)                    \
  X(2, 512, 256, 256, 8, 0) X(2, 1024, 64, 64, 8, 0) X(2, 1024, 128, 128, 8, 0) X(2, 1024, 256, 256, 8, 0)              \
  X(2, 2048, 128, 128, 8, 0) X(2, 2048, 256, 256, 8, 0) X(2, 2048, 512, 512, 8, 0) X(2, 4096, 256, 256, 8, 0)           \
  X(2, 4096, 512, 512, 8, 0) X(2, 8192, 256, 256, 8, 0) X(2, 8192, 512, 512, 8, 0) X(2, 16384, 256, 256, 8, 0)          \
  /* irfft_lds (no caller today): CheapTrick's and D4C's rfft_lds shapes */                                             \
  X(3, 256, 128, 128, 8, 1) X(3, 512, 128, 128, 8, 1) X(3, 1024, 128, 128, 8, 1) X(3, 2048, 256, 256, 8, 1)             \
  X(3, 4096, 256, 256, 8, 1) X(3, 512, 256, 256, 8, 1) X(3, 4096, 512, 512, 8, 1) X(3, 8192, 512, 512, 8, 1)

extern "C" {

int wh_fft_engine_probe(wh_ctx* ctx, void* stream, int kind, int n, int nt, int snt, int maxr, int inverse, const double* in,
                        double* out, int64_t count) {
  if (!ctx || !in || !out || count < 0 || kind < 0 || kind > 4 || n < 2 || (n & (n - 1)) != 0 || nt < 1 || snt < nt ||
      snt % nt != 0 || (inverse != 0 && inverse != 1) || ((kind == 1 || kind == 2) && inverse) || (kind == 3 && !inverse))
    return wh::fail_msg("wh_fft_engine_probe", "bad argument");
  WH_ENTER(ctx);
  if (count == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  static const struct {
    int kind, n, nt, snt, maxr, inverse;
    int (*launch)(wh_ctx*, hipStream_t, const double*, double*, long long);
  } built[] = {
#define WH_PROBE_ROW(K, N_, NT_, SNT_, MAXR_, INV_) \
  {K, N_, NT_, SNT_, MAXR_, INV_, launch_probe<K, N_, NT_, SNT_, MAXR_, (INV_) != 0>},
      WH_PROBE_SHAPES(WH_PROBE_ROW)
#undef WH_PROBE_ROW
  };
  for (const auto& s : built)
    if (kind == s.kind && n == s.n && nt == s.nt && snt == s.snt && maxr == s.maxr && inverse == s.inverse)
      return s.launch(ctx, st, in, out, count);
  return wh::fail_msg("wh_fft_engine_probe", "shape (kind, n, nt, snt, maxr, inverse) not built: see WH_PROBE_SHAPES in csrc/wh_fft_probe.hip");
}

int wh_twiddle_read(wh_ctx* ctx, double* h_out, int64_t n_entries) {
  if (!ctx) return wh::fail_msg("wh_twiddle_read", "null ctx");
  if (!h_out) return WH_TWIDDLE_ENTRIES;
  if (n_entries != WH_TWIDDLE_ENTRIES) return wh::fail_msg("wh_twiddle_read", "n_entries is not the block's entry count");
  WH_ENTER(ctx);
  WH_CHECK(hipMemcpy(h_out, ctx->d_twiddle, (size_t)WH_TWIDDLE_ENTRIES * sizeof(double2), hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
