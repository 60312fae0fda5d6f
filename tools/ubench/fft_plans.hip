// Micro-benchmark of the in-LDS FP64 transform engine (wh_fft.h: fft_lds / fft_lds_from_regs) at the shapes config 2's
// three heavy kernels run it: the same header, the same context twiddle table, config 2's count of transforms (128 k),
// device-event timing, and every bin of 16 of the transforms checked against a host FP64 DFT.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off fft_plans.hip -o fft_plans.bin && ./fft_plans.bin
//
// -DFFT_HEADER='"path/wh_fft.h"' times another revision of the engine (an A/B of two builds of this file; wh_device.h
// for a revision from before the engine had a header of its own).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

#ifndef FFT_HEADER
#define FFT_HEADER "../../python-world_amd/csrc/wh_fft.h"
#endif
#include FFT_HEADER

#ifndef WH_MAX_TWIDDLE
#define WH_MAX_TWIDDLE 32768
#endif
#ifdef WH_TWIDDLE_ENTRIES
constexpr int kTwEntries = WH_TWIDDLE_ENTRIES;
#else
constexpr int kTwEntries = 2 * WH_MAX_TWIDDLE;
#endif

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

constexpr int kInputs = 64;  // distinct inputs (L2-resident); transform t reads input t % kInputs
constexpr int kReps = 8;     // transforms per buffer per workgroup

// One workgroup: SNT threads, SNT / NT buffers of N points, kReps transforms each.  Transform 0 of the first kInputs
// buffers is written out for the check; the rest feed a checksum so that nothing is optimised away.
// WAVE: wh::fft_lds_wave — the first wave of each NT-thread group runs the transform, one SNT-wide barrier at the end.
template <int N, int NT, int SNT, int MINW, bool REGFED, bool WAVE = false>
__global__ __launch_bounds__(SNT, MINW) void fft_case(const double2* __restrict__ in, const double2* __restrict__ tw,
                                                      double2* __restrict__ out, double* __restrict__ sink, int n_buf) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int sub = threadIdx.x / NT, tid = threadIdx.x % NT;
  double2* s = reinterpret_cast<double2*>(smem) + sub * N;
  const int b = blockIdx.x * (SNT / NT) + sub;
  double acc = 0.0;
  for (int rep = 0; rep < kReps; ++rep) {
    const double2* x = in + (size_t)((b * kReps + rep) % kInputs) * N;
    const double2* t = tw;
    asm volatile("" : "+s"(t));  // as the kernels' fresh_table: every transform derives its twiddles afresh
    if constexpr (REGFED) {
      double2 v[N / NT];
#pragma unroll
      for (int q = 0; q < N / NT; ++q) v[q] = x[tid + q * NT];
      wh::fft_lds_from_regs<N, false, NT, 8>(v, s, t + N);
    } else if constexpr (WAVE) {
      for (int i = tid; i < N; i += NT) s[i] = x[i];
      __syncthreads();
      wh::fft_lds_wave<N, false, NT, SNT>(s, t + N);
    } else {
      for (int i = tid; i < N; i += NT) s[i] = x[i];
      __syncthreads();
      wh::fft_lds<N, false, NT, SNT, 8>(s, t + N);
    }
    if (rep == 0 && b < kInputs)
      for (int i = tid; i < N; i += NT) out[(size_t)b * N + i] = s[i];
    acc += s[tid].x;
    __syncthreads();
  }
  if (b < n_buf) sink[(size_t)b * NT + tid] = acc;
}

template <int N, int NT, int SNT, int MINW, bool REGFED, bool WAVE = false>
int run_case(const char* name, const double2* d_tw, const std::vector<double2>& h_in, const double2* d_in) {
  constexpr int PER_WG = SNT / NT;
  const int n_transforms = 131072;
  const int n_buf = n_transforms / kReps;
  const int grid = n_buf / PER_WG;
  double2* d_out;
  double* d_sink;
  CK(hipMalloc(&d_out, sizeof(double2) * N * kInputs));
  CK(hipMalloc(&d_sink, sizeof(double) * n_buf * NT));
  const size_t lds = sizeof(double2) * N * PER_WG;
  auto k = fft_case<N, NT, SNT, MINW, REGFED, WAVE>;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  hipLaunchKernelGGL(k, dim3(grid), dim3(SNT), lds, 0, d_in, d_tw, d_out, d_sink, n_buf);  // warm-up
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  float best = 1e30f;
  for (int it = 0; it < 5; ++it) {
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL(k, dim3(grid), dim3(SNT), lds, 0, d_in, d_tw, d_out, d_sink, n_buf);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    best = ms < best ? ms : best;
  }
  std::vector<double2> h_out((size_t)N * kInputs);
  CK(hipMemcpy(h_out.data(), d_out, sizeof(double2) * N * kInputs, hipMemcpyDeviceToHost));
  // host FP64 DFT of the inputs the first kInputs buffers transformed (buffer b, rep 0: input (b * kReps) % kInputs)
  double max_rel = 0.0, sum_sq = 0.0;
  long long cnt = 0;
  std::vector<double> c(N), sn(N);
  for (int i = 0; i < N; ++i) {
    c[i] = cos(-2.0 * M_PI * i / N);
    sn[i] = sin(-2.0 * M_PI * i / N);
  }
  for (int bb = 0; bb < kInputs; bb += 4) {  // a quarter of them: the host DFT is O(N^2)
    const double2* x = h_in.data() + (size_t)((bb * kReps) % kInputs) * N;
    std::vector<double2> ref(N);
    double norm = 0.0;
    for (int kk = 0; kk < N; ++kk) {
      double re = 0.0, im = 0.0;
      for (int j = 0; j < N; ++j) {
        const int t = (int)(((long long)kk * j) % N);
        re += x[j].x * c[t] - x[j].y * sn[t];
        im += x[j].x * sn[t] + x[j].y * c[t];
      }
      ref[kk] = make_double2(re, im);
      norm += re * re + im * im;
    }
    norm = sqrt(norm);
    for (int kk = 0; kk < N; ++kk) {
      const double2 g = h_out[(size_t)bb * N + kk];
      const double e = hypot(g.x - ref[kk].x, g.y - ref[kk].y) / norm;
      max_rel = e > max_rel ? e : max_rel;
      sum_sq += e * e;
      ++cnt;
    }
  }
  printf("%-34s %5d %4d %4d %5d %10.3f %10.2f %10.2e %10.2e\n", name, N, NT, SNT, MINW, best,
         1e6 * best / n_transforms, max_rel, sqrt(sum_sq / cnt));
  CK(hipFree(d_out));
  CK(hipFree(d_sink));
  return 0;
}

int main() {
  // the context's table (wh_api.hip: wh_ctx_create), pass tables included when the header has them
  std::vector<double2> tw(kTwEntries);
  tw[0] = tw[1] = make_double2(1.0, 0.0);
  for (int n = 2; n <= WH_MAX_TWIDDLE; n <<= 1) {
    for (int k = 0; k < n; ++k) {
      long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)n;
      tw[n + k] = make_double2((double)cosl(a), (double)sinl(a));
    }
    tw[n] = make_double2(1.0, 0.0);
    tw[n + n / 2] = make_double2(-1.0, 0.0);
    if (n >= 4) {
      tw[n + n / 4] = make_double2(0.0, -1.0);
      tw[n + 3 * n / 4] = make_double2(0.0, 1.0);
    }
  }
#ifdef WH_TWIDDLE_ENTRIES
  for (int R = 2; R <= 8; R <<= 1)
    for (int m = R; m <= WH_MAX_FFT; m <<= 1)
      for (int k = 0; k < m / R; ++k)
        for (int r = 1; r < R; ++r) tw[wh::fft_ptw_offset(m, R) + k * (R - 1) + r - 1] = tw[m + k * r];
#endif
  constexpr int NMAX = 2048;
  std::vector<double2> h_in((size_t)NMAX * kInputs);
  unsigned long long st = 12345;
  for (auto& v : h_in) {
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    const double a = (double)(st >> 11) / 9007199254740992.0 - 0.5;
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    const double b = (double)(st >> 11) / 9007199254740992.0 - 0.5;
    v = make_double2(a, b);
  }
  double2 *d_tw, *d_in;
  CK(hipMalloc(&d_tw, sizeof(double2) * tw.size()));
  CK(hipMemcpy(d_tw, tw.data(), sizeof(double2) * tw.size(), hipMemcpyHostToDevice));
  printf("%-34s %5s %4s %4s %5s %10s %10s %10s %10s\n", "case", "N", "NT", "SNT", "minw", "ms", "ns/xform", "max_rel",
         "rms_rel");
  int rc = 0;
  // inputs laid out per size: input i of size N at h_in[i * N]
  for (int N : {2048, 1024, 512}) {
    std::vector<double2> hin((size_t)N * kInputs);
    for (size_t i = 0; i < hin.size(); ++i) hin[i] = h_in[i];
    CK(hipMalloc(&d_in, sizeof(double2) * hin.size()));
    CK(hipMemcpy(d_in, hin.data(), sizeof(double2) * hin.size(), hipMemcpyHostToDevice));
    if (N == 2048) rc |= run_case<2048, 256, 256, 4, true>("d4c 2048 register-fed", d_tw, hin, d_in);
    if (N == 1024) rc |= run_case<1024, 256, 256, 4, false>("d4c 1024 band", d_tw, hin, d_in);
    if (N == 512) {
      rc |= run_case<512, 128, 128, 6, false>("cheaptrick 512 (ct_minw)", d_tw, hin, d_in);
      rc |= run_case<512, 128, 256, 4, false>("response 512 x 2 buffers", d_tw, hin, d_in);
#ifdef WH_HAVE_FFT_WAVE
      rc |= run_case<512, 64, 64, 4, false>("512 one wave per workgroup", d_tw, hin, d_in);
      rc |= run_case<512, 128, 128, 6, false, true>("cheaptrick 512 wave-local", d_tw, hin, d_in);
      rc |= run_case<512, 128, 256, 4, false, true>("response 512 wave-local x 2 buffers", d_tw, hin, d_in);
      rc |= run_case<512, 256, 256, 4, false>("response 512 unvoiced (4-4-4-4-2)", d_tw, hin, d_in);
      rc |= run_case<512, 256, 256, 4, false, true>("response 512 unvoiced wave-local", d_tw, hin, d_in);
#endif
    }
    CK(hipFree(d_in));
  }
  CK(hipFree(d_tw));
  return rc;
}
