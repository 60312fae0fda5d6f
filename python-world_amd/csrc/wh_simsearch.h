// The similarity search of the two overlap-add methods (wsola_search_kernel: wh_wsola.hip, DESIGN section 20;
// psola_marks_kernel: wh_psola.hip): of the 2 D + 1 shifts d in [-D, D] of a template over a candidate
// region, the one with the best normalised cross-correlation.  One workgroup of kSimThreads searches; the arithmetic is a
// contract (include/world_hip.h, tests/_wsola_reference.py) and both callers' results are compared with it bit for bit.
#pragma once
#include "wh_device.h"

#include <limits>
#include <type_traits>

namespace wh {

constexpr int kSimThreads = 256;                  // the workgroup sim_search runs in,
constexpr int kSimWaves = kSimThreads / WH_WAVE;  // and the slots of s_score and s_delta: one per wave
// The largest D the dispatcher below has an instantiation for.  Both entry points' tolerance limits are this constant:
// raising either limit means another case in dispatch_sim_width, not another value here alone.
constexpr int kSimMaxTol = 512;
constexpr int kSimMaxPerThread = (2 * kSimMaxTol + 1 + kSimThreads - 1) / kSimThreads;  // 5

// a is the better candidate: the greater score, then the smaller |shift|, then the negative shift (scores are never NaN here)
__device__ __forceinline__ bool sim_better(double sa, int da, double sb, int db) {
  if (sa != sb) return sa > sb;
  const int aa = da < 0 ? -da : da, ab = db < 0 ? -db : db;
  return aa != ab ? aa < ab : da < db;
}

// The best shift of tpl[0 .. len) over reg[0 .. len + 2 D), in every thread: candidate k = d + D scores
// sum_j tpl[j] reg[k + j] / sqrt(sum_j reg[k + j]^2) (0 where the region is all zero), the key is (score, -|d|, d < 0), a
// total order.  Thread tid runs the two add chains of its U candidates side by side, j ascending, each product and sum
// rounded on its own (build.py's default -ffp-contract=off).  The caller has staged tpl and reg and passed its barrier; the
// one barrier in here is between the waves' writes of s_score / s_delta (kSimWaves entries) and their reads, so the
// caller needs a barrier of its own before the slots, tpl or reg are written again.  U >= ceil((2 D + 1) / kSimThreads).
template <int U>
__device__ __forceinline__ int sim_search(const ckp<double>& tpl, const ckp<double>& reg, int len, int D, const ckp<double>& s_score,
                                          const ckp<int>& s_delta, int tid) {
  const int ncand = 2 * D + 1;
  // this thread's candidates: k = tid + 256 u; one beyond the list runs the last one again and is discarded
  int k[U];
  double num[U], den[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    k[u] = min(tid + kSimThreads * u, ncand - 1);
    num[u] = den[u] = 0.0;
  }
#pragma unroll 4
  for (int j = 0; j < (tid < ncand ? len : 0); ++j) {  // (a wave without a candidate leaves its SIMD to the others)
    const double t = tpl[j];  // (one address for the wave: a broadcast)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const double g = reg[k[u] + j];  // (consecutive lanes, consecutive addresses)
      num[u] = num[u] + t * g;
      den[u] = den[u] + g * g;
    }
  }
  double best_s = -std::numeric_limits<double>::infinity();
  int best_d = std::numeric_limits<int>::max();  // (no candidate: loses to every candidate)
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (tid + kSimThreads * u < ncand) {
      double s = den[u] > 0 ? num[u] / sqrt(den[u]) : 0.0;
      if (s != s) s = -std::numeric_limits<double>::infinity();
      const int d = k[u] - D;
      if (sim_better(s, d, best_s, best_d)) best_s = s, best_d = d;
    }
  }
#pragma unroll
  for (int off = WH_WAVE / 2; off > 0; off >>= 1) {
    const double os = __shfl_xor(best_s, off, WH_WAVE);
    const int od = __shfl_xor(best_d, off, WH_WAVE);
    if (sim_better(os, od, best_s, best_d)) best_s = os, best_d = od;
  }
  if ((tid & (WH_WAVE - 1)) == 0) {
    s_score[tid / WH_WAVE] = best_s;
    s_delta[tid / WH_WAVE] = best_d;
  }
  __syncthreads();
  best_s = s_score[0], best_d = s_delta[0];
#pragma unroll
  for (int w = 1; w < kSimWaves; ++w) {
    const double os = s_score[w];
    const int od = s_delta[w];
    if (sim_better(os, od, best_s, best_d)) best_s = os, best_d = od;
  }
  return best_d;  // (candidate 0 always exists, so |best_d| <= D)
}

// f(std::integral_constant<int, U>()) for the candidates a thread runs side by side at the tolerance D in [0, kSimMaxTol]:
// U = ceil((2 D + 1) / kSimThreads), one search kernel instantiation per count; f's result is returned.
template <class F>
inline int dispatch_sim_width(int D, F&& f) {
  static_assert(kSimMaxPerThread == 5, "one instantiation per count");
  switch ((2 * D + 1 + kSimThreads - 1) / kSimThreads) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, 5>());
  }
}

}  // namespace wh
