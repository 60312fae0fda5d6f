// Micro-benchmark of the spectral kernels' transcendentals (wh_math.h): per function the device library's, the polynomial
// form (wh::flog / fexp / fsincospi) and the table-driven form (wh::tlog / texp / tsincospi), as the minimum-phase chains call
// them: two evaluations per real (noinline) call on register-resident arguments (|a| <= 12, |b| <= 600, log arguments over
// 1e-16 .. 1e6), 256 threads per workgroup at response_kernel's occupancy (40 KB of LDS per workgroup: four workgroups per
// CU, four waves per SIMD).  Every case runs twice: with nothing else touching memory (the tables stay in L1), and with a
// second access stream of 2 x 4 KB rows per workgroup and iteration, as the spectrogram rows of the pulses evict lines.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off math_tables.hip -o math_tables.bin && ./math_tables.bin
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

#include "../../python-world_amd/csrc/wh_math.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

constexpr int kIters = 512;
constexpr int kBlocks = 256 * 4 * 8;  // eight rounds of a full chip
constexpr int kRowDoubles = 512;      // 4 KB
constexpr size_t kStreamRows = 1 << 15;

enum { LOG_LIB, LOG_POLY, LOG_TAB, EXP_LIB, EXP_POLY, EXP_TAB, SC_LIB, SC_POLY, SC_TAB, N_CASES };
static const char* kNames[N_CASES] = {"log       library", "log       wh::flog", "log       wh::tlog", "exp       library", "exp       wh::fexp",
                                      "exp       wh::texp", "sincospi  library", "sincospi  wh::fsincospi", "sincospi  wh::tsincospi"};

template <int WHICH>
__device__ __attribute__((noinline)) double2 pair_call(double x, double y, const double2* tw256, const double* mt) {
  if constexpr (WHICH == LOG_LIB) return make_double2(log(x), log(y));
  else if constexpr (WHICH == LOG_POLY) return make_double2(wh::flog(x), wh::flog(y));
  else if constexpr (WHICH == LOG_TAB) return make_double2(wh::tlog(x, mt), wh::tlog(y, mt));
  else if constexpr (WHICH == EXP_LIB) return make_double2(exp(x), exp(y));
  else if constexpr (WHICH == EXP_POLY) return make_double2(wh::fexp(x), wh::fexp(y));
  else if constexpr (WHICH == EXP_TAB) return make_double2(wh::texp(x, mt), wh::texp(y, mt));
  else if constexpr (WHICH == SC_LIB) {
    double s0, c0, s1, c1;
    sincospi(x, &s0, &c0);
    sincospi(y, &s1, &c1);
    return make_double2(s0 + c0, s1 + c1);
  } else if constexpr (WHICH == SC_POLY) {
    const double2 p = wh::fsincospi(x), q = wh::fsincospi(y);
    return make_double2(p.x + p.y, q.x + q.y);
  } else {
    const double2 p = wh::tsincospi(x, tw256), q = wh::tsincospi(y, tw256);
    return make_double2(p.x + p.y, q.x + q.y);
  }
}

template <int WHICH, bool EVICT>
__global__ __launch_bounds__(256) void math_case(const double2* __restrict__ tw256, const double* __restrict__ mt,
                                                 const double* __restrict__ stream, double* __restrict__ sink) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // (occupancy only)
  const unsigned gid = blockIdx.x * 256 + threadIdx.x;
  // arguments in the chains' ranges, different per lane, moved along every iteration
  const double u = (double)((gid * 2654435761u) >> 8) * (1.0 / 16777216.0);  // [0, 1)
  double x, y, dx, dy;
  if (WHICH <= LOG_TAB) { x = exp2(-53.0 + 73.0 * u); y = exp2(20.0 - 73.0 * u); dx = 1.0009765625; dy = 0.9990234375; }
  else if (WHICH <= EXP_TAB) { x = -12.0 + 24.0 * u; y = 12.0 - 24.0 * u; dx = 0.001; dy = -0.001; }
  else { x = -600.0 + 1200.0 * u; y = 600.0 - 1200.0 * u; dx = 0.37; dy = -0.41; }
  double acc = 0.0;
  for (int it = 0; it < kIters; ++it) {
    const double2* t = tw256;
    const double* m = mt;
    asm volatile("" : "+s"(t), "+s"(m));  // per call, as the kernels take their tables afresh per pulse
    if (EVICT) {
      const double* row = stream + ((size_t)(blockIdx.x * 37u + it * 2u) % kStreamRows) * kRowDoubles;
      acc += row[threadIdx.x] + row[256 + threadIdx.x] + row[kRowDoubles + threadIdx.x] + row[kRowDoubles + 256 + threadIdx.x];
    }
    const double2 r = pair_call<WHICH>(x, y, t, m);
    acc += r.x + r.y;
    if (WHICH <= LOG_TAB) { x *= dx; y *= dy; } else { x += dx; y += dy; }
  }
  if (acc == 12345.678 || smem[threadIdx.x] == 77) sink[gid] = acc;  // (keeps the work and the LDS)
  if (gid == 0) sink[0] = acc;
}

template <int WHICH>
static int run_case(const double2* tw, const double* mt, const double* stream, double* sink) {
  float ms[2] = {0, 0};
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int evict = 0; evict < 2; ++evict) {
    float best = 1e30f;
    for (int rep = 0; rep < 4; ++rep) {  // the first is the warm-up
      CK(hipEventRecord(e0, 0));
      if (evict) hipLaunchKernelGGL((math_case<WHICH, true>), dim3(kBlocks), dim3(256), 40 * 1024, 0, tw, mt, stream, sink);
      else hipLaunchKernelGGL((math_case<WHICH, false>), dim3(kBlocks), dim3(256), 40 * 1024, 0, tw, mt, stream, sink);
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float t;
      CK(hipEventElapsedTime(&t, e0, e1));
      if (rep > 0 && t < best) best = t;
    }
    ms[evict] = best;
  }
  double chk = 0;
  CK(hipMemcpy(&chk, sink, sizeof chk, hipMemcpyDeviceToHost));
  printf("%-26s  quiet %8.3f ms   with the row stream %8.3f ms   (check %.6g)\n", kNames[WHICH], ms[0], ms[1], chk);
  return 0;
}

int main() {
  // the two tables as the library's context holds them (wh_api.hip)
  std::vector<double2> tw(256);
  for (int k = 0; k < 256; ++k) {
    const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / 256.0L;
    tw[k] = make_double2((double)cosl(a), (double)sinl(a));
  }
  tw[0] = make_double2(1, 0); tw[64] = make_double2(0, -1); tw[128] = make_double2(-1, 0); tw[192] = make_double2(0, 1);
  for (int k = 129; k < 256; ++k) tw[k] = make_double2(tw[256 - k].x, -tw[256 - k].y);
  std::vector<double> mt(wh::kMtEntries, 0.0);
  for (int j = 0; j < 128; ++j) mt[wh::kMtExp + j] = (double)exp2l((long double)j / 128.0L);
  for (int i = 0; i < wh::kMtLogNodes; ++i) {
    const double inv = (double)(float)(128.0 / (double)(wh::kMtLogFirst + i));
    const long double L = -logl((long double)inv);
    const double hi = (double)(rintl(L * 0x1p42L) * 0x1p-42L);
    mt[wh::kMtLog + 4 * i] = inv;
    mt[wh::kMtLog + 4 * i + 1] = hi;
    mt[wh::kMtLog + 4 * i + 2] = (double)(L - (long double)hi);
  }
  double2* d_tw;
  double *d_mt, *d_stream, *d_sink;
  CK(hipMalloc((void**)&d_tw, tw.size() * sizeof(double2)));
  CK(hipMalloc((void**)&d_mt, mt.size() * sizeof(double)));
  CK(hipMalloc((void**)&d_stream, (kStreamRows + 2) * kRowDoubles * sizeof(double)));
  CK(hipMalloc((void**)&d_sink, (size_t)kBlocks * 256 * sizeof(double)));
  CK(hipMemcpy(d_tw, tw.data(), tw.size() * sizeof(double2), hipMemcpyHostToDevice));
  CK(hipMemcpy(d_mt, mt.data(), mt.size() * sizeof(double), hipMemcpyHostToDevice));
  CK(hipMemset(d_stream, 0, (kStreamRows + 2) * kRowDoubles * sizeof(double)));
  printf("%d workgroups x 256 threads x %d calls of two evaluations\n", kBlocks, kIters);
  if (run_case<LOG_LIB>(d_tw, d_mt, d_stream, d_sink) || run_case<LOG_POLY>(d_tw, d_mt, d_stream, d_sink) ||
      run_case<LOG_TAB>(d_tw, d_mt, d_stream, d_sink) || run_case<EXP_LIB>(d_tw, d_mt, d_stream, d_sink) ||
      run_case<EXP_POLY>(d_tw, d_mt, d_stream, d_sink) || run_case<EXP_TAB>(d_tw, d_mt, d_stream, d_sink) ||
      run_case<SC_LIB>(d_tw, d_mt, d_stream, d_sink) || run_case<SC_POLY>(d_tw, d_mt, d_stream, d_sink) ||
      run_case<SC_TAB>(d_tw, d_mt, d_stream, d_sink))
    return 1;
  return 0;
}
