// ================================================================================================
// Time-domain pitch-synchronous overlap-add (TD-PSOLA): a new f0 contour and a new timing for a recording without
// analysis and synthesis.  Grains two periods wide are cut around pitch marks of the recording and re-spaced at the
// target period: the spacing sets f0, the grain content — and with it the envelope — stays.  Contract:
// include/world_hip.h; tests/_psola_reference.py is the same in NumPy, and every output (the marks,
// their periods, the synthesis marks, the selection, the flips, the counts and y) is compared bit for bit.
//
//   psola_marks_kernel    stage A, one workgroup per utterance: the analysis marks are one sequential chain.  Per voiced
//                         mark the template (P doubles) and the candidate region (P + 2 D doubles) are staged in LDS,
//                         zero-filled outside the utterance; thread i runs the two add chains of the candidates i,
//                         i + 256, .. side by side, j ascending, each product and sum rounded on its own (build.py's
//                         default -ffp-contract=off); one workgroup argmax on the key (score, -|d|, d < 0):
//                         wh::sim_search (wh_simsearch.h), the search that wh_wsola.hip calls too.
//   psola_smarks_kernel   stage B, one wave per utterance: the synthesis marks are one sequential integer chain.  Per
//                         mark a 64-way search of the increasing list of analysis marks (three rounds for 10 s of
//                         speech), the flip rule and the step; the grain's centre and its two half widths go to scratch.
//   psola_ola_kernel      stage C, chip-wide: a tile of 256 output samples finds the grains that can reach it by two
//                         binary searches of the synthesis marks and gathers them, j ascending.
// The tracks are device data that no host check sees: a period is used only through eff() (0 or [pmin, 2048]), a source
// position is clamped to +- 2^62, a track index is clamped to the track, every chain is bounded by the capacity the host
// verified, and every read of x is range-tested.  No atomics.
// ================================================================================================
#include "wh_host.h"
#include "wh_simsearch.h"

#include <algorithm>

namespace {

constexpr int kPsMaxPeriod = 2048, kPsMaxTol = wh::kSimMaxTol, kPsMaxGrid = 4096, kPsMaxHop = 2048;
constexpr int kPsThreads = wh::kSimThreads;  // (the search's workgroup: wh_simsearch.h)
constexpr int kPsTile = 256;

struct PsUtt {
  int64_t x_off, n;              // the recording
  int64_t y_off, n_out;          // the output
  int64_t pa_off, ka;            // per_a: n / G + 1 entries
  int64_t ps_off, ks;            // per_s and src: n_out / G + 1 entries
  int64_t mark_off, mark_cap;    // the analysis marks and their capacity
  int64_t smark_off, smark_cap;  // the synthesis marks and their capacity
};

struct PsParams {
  int grid, hop, tol, pmin, smin, norm;
};

// x[i], 0.0 outside [0, n)
__device__ __forceinline__ double ps_read(const wh::ckp<const double>& xu, int64_t i, int64_t n) {
  return (i >= 0 && i < n) ? xu[(long long)i] : 0.0;
}

__device__ __forceinline__ int ps_eff(int p, int pmin) { return (p >= pmin && p <= kPsMaxPeriod) ? p : 0; }

template <int U>
__global__ __launch_bounds__(kPsThreads) void psola_marks_kernel(const PsUtt* __restrict__ meta, PsParams pr, int dmax,
                                                                 const double* __restrict__ x_, const int32_t* __restrict__ per_a_,
                                                                 int64_t* __restrict__ marks_, int32_t* __restrict__ period_,
                                                                 int32_t* __restrict__ n_marks_) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double s_score_[wh::kSimWaves];
  __shared__ int s_delta_[wh::kSimWaves];
  const PsUtt m = meta[blockIdx.x];
  const int tid = threadIdx.x;
  const wh::ckp<int32_t> n_marks = wh::ck_make(n_marks_, gridDim.x, wh::WH_CK_OUT);
  if (m.n == 0 || m.mark_cap == 0) {  // (uniform over the workgroup)
    if (tid == 0) n_marks[blockIdx.x] = 0;
    return;
  }
  // (wh::ckp<T> is T* in every shipped build; the bounds build checks each access against the range named here)
  const wh::ckp<double> tpl = wh::ck_make(reinterpret_cast<double*>(smem), kPsMaxPeriod, wh::WH_CK_LDS_MAIN);
  const wh::ckp<double> reg = wh::ck_make(reinterpret_cast<double*>(smem) + kPsMaxPeriod, kPsMaxPeriod + 2 * dmax, wh::WH_CK_LDS_AUX);
  const wh::ckp<double> s_score = wh::ck_make(s_score_, wh::kSimWaves, wh::WH_CK_LDS_SCRATCH);
  const wh::ckp<int> s_delta = wh::ck_make(s_delta_, wh::kSimWaves, wh::WH_CK_LDS_SCRATCH);
  const wh::ckp<const double> xu = wh::ck_make(x_ + m.x_off, m.n, wh::WH_CK_WAVEFORM);
  const wh::ckp<const int32_t> per_a = wh::ck_make(per_a_ + m.pa_off, m.ka, wh::WH_CK_IN);
  const wh::ckp<int64_t> marks = wh::ck_make(marks_ + m.mark_off, m.mark_cap, wh::WH_CK_OUT);
  const wh::ckp<int32_t> period = wh::ck_make(period_ + m.mark_off, m.mark_cap, wh::WH_CK_OUT);
  int64_t a = 0, count = m.mark_cap;  // (the capacity is never reached: every step is at least the contract's m)
#pragma unroll 1
  for (int64_t i = 0; i < m.mark_cap; ++i) {
    const int P = ps_eff(per_a[min(m.ka - 1, a / pr.grid)], pr.pmin);
    if (tid == 0) {
      marks[i] = a;
      period[i] = P;
    }
    if (a >= m.n) {  // the mark at or beyond the end belongs to the list
      count = i + 1;
      break;
    }
    if (P == 0) {
      a += pr.hop;
      continue;
    }
    const int h = P / 2, D = min(pr.tol, P / 4), R = P + 2 * D;
    const int64_t tb = a - h, rb = a + P - D - h;
    // (the mark before's readers are behind its second barrier)
    for (int j = tid; j < P; j += kPsThreads) tpl[j] = ps_read(xu, tb + j, m.n);
    for (int j = tid; j < R; j += kPsThreads) reg[j] = ps_read(xu, rb + j, m.n);
    __syncthreads();
    const int best_d = wh::sim_search<U>(tpl, reg, P, D, s_score, s_delta, tid);
    // (candidate 0 always exists, so |best_d| <= D <= P / 4; the slots are rewritten behind the next mark's first barrier)
    a += P + best_d;
  }
  if (tid == 0) n_marks[blockIdx.x] = (int32_t)count;
}

// The number of marks at or below c in the increasing list mk[0 .. Ma): a 64-way search by the lanes of one wave.
__device__ __forceinline__ int64_t ps_count_le(const wh::ckp<const int64_t>& mk, int64_t Ma, int64_t c, int lane) {
  int64_t lo = 0, hi = Ma;
  while (lo < hi) {
    const int64_t chunk = (hi - lo + WH_WAVE - 1) / WH_WAVE;
    const int64_t p = lo + lane * chunk;
    const bool le = p < hi && mk[p] <= c;
    const int cnt = __popcll(__ballot(le));  // (the list increases: the lanes that hold are the first cnt)
    if (cnt == 0) break;
    hi = min(hi, lo + cnt * chunk);
    lo = lo + (cnt - 1) * chunk + 1;
  }
  return lo;
}

__global__ __launch_bounds__(WH_WAVE) void psola_smarks_kernel(const PsUtt* __restrict__ meta, PsParams pr,
                                                               const int32_t* __restrict__ per_s_, const int64_t* __restrict__ src_,
                                                               const int64_t* __restrict__ marks_, const int32_t* __restrict__ period_,
                                                               const int32_t* __restrict__ n_marks_, int64_t* __restrict__ smarks_,
                                                               int32_t* __restrict__ sel_, uint8_t* __restrict__ flip_,
                                                               int32_t* __restrict__ n_smarks_, int64_t* __restrict__ centre_,
                                                               int32_t* __restrict__ lw_, int32_t* __restrict__ rw_,
                                                               int32_t* __restrict__ reach_) {
  const PsUtt m = meta[blockIdx.x];
  const int lane = threadIdx.x;
  const wh::ckp<const int32_t> n_marks = wh::ck_make(n_marks_, gridDim.x, wh::WH_CK_IN);
  const wh::ckp<int32_t> n_smarks = wh::ck_make(n_smarks_, gridDim.x, wh::WH_CK_OUT);
  const wh::ckp<int32_t> reach = wh::ck_make(reach_, 2 * (long long)gridDim.x, wh::WH_CK_OUT);
  const int64_t Ma = min((int64_t)max(n_marks[blockIdx.x], 0), m.mark_cap);
  if (m.n_out == 0 || Ma == 0 || m.smark_cap == 0) {  // (uniform over the wave)
    if (lane == 0) {
      n_smarks[blockIdx.x] = 0;
      reach[2 * blockIdx.x] = reach[2 * blockIdx.x + 1] = 0;
    }
    return;
  }
  const wh::ckp<const int32_t> per_s = wh::ck_make(per_s_ + m.ps_off, m.ks, wh::WH_CK_IN);
  const wh::ckp<const int64_t> src = wh::ck_make(src_ + m.ps_off, m.ks, wh::WH_CK_IN);
  const wh::ckp<const int64_t> marks = wh::ck_make(marks_ + m.mark_off, Ma, wh::WH_CK_IN);
  const wh::ckp<const int32_t> period = wh::ck_make(period_ + m.mark_off, Ma, wh::WH_CK_IN);
  const wh::ckp<int64_t> smarks = wh::ck_make(smarks_ + m.smark_off, m.smark_cap, wh::WH_CK_OUT);
  const wh::ckp<int32_t> sel = wh::ck_make(sel_ + m.smark_off, m.smark_cap, wh::WH_CK_OUT);
  const wh::ckp<uint8_t> flip = wh::ck_make(flip_ + m.smark_off, m.smark_cap, wh::WH_CK_OUT);
  const wh::ckp<int64_t> centre = wh::ck_make(centre_ + m.smark_off, m.smark_cap, wh::WH_CK_OUT);
  const wh::ckp<int32_t> lw = wh::ck_make(lw_ + m.smark_off, m.smark_cap, wh::WH_CK_OUT);
  const wh::ckp<int32_t> rw = wh::ck_make(rw_ + m.smark_off, m.smark_cap, wh::WH_CK_OUT);
  constexpr int64_t kFar = (int64_t)1 << 62;
  int64_t s = 0, count = m.smark_cap, prev_sel = -1;
  int prev_flip = 0, max_l = 0, max_r = 0;
#pragma unroll 1
  for (int64_t j = 0; j < m.smark_cap; ++j) {
    const int64_t k = min(m.ks - 1, s / pr.grid);
    const int64_t c = min(max(src[k], -kFar), kFar) + (s - k * pr.grid);
    // the nearest mark, the lower one on a tie: r marks lie at or below c
    const int64_t r = ps_count_le(marks, Ma, c, lane);
    int64_t i = r == 0 ? 0 : r - 1;
    if (r > 0 && r < Ma && marks[r] - c < c - marks[r - 1]) i = r;
    const int64_t a = marks[i];
    const int P = period[i];
    const int fb = P > 0 ? P : pr.hop;
    const int left = i > 0 ? (int)(a - marks[i - 1]) : fb;
    const int right = i + 1 < Ma ? (int)(marks[i + 1] - a) : fb;
    const int fl = (j >= 1 && P == 0 && i == prev_sel && prev_flip == 0) ? 1 : 0;
    if (lane == 0) {
      smarks[j] = s;
      sel[j] = (int32_t)i;
      flip[j] = (uint8_t)fl;
      centre[j] = a;
      lw[j] = left;
      rw[j] = right;
    }
    max_l = max(max_l, left), max_r = max(max_r, right);
    prev_sel = i, prev_flip = fl;
    if (s >= m.n_out) {  // the mark at or beyond the end belongs to the list
      count = j + 1;
      break;
    }
    const int Q = ps_eff(per_s[k], pr.pmin);
    int64_t step = pr.hop;
    if (Q > 0 && P > 0) {
      const int64_t sp = i + 1 < Ma ? (int64_t)right : (int64_t)P;
      step = max((int64_t)pr.smin, (sp * Q + P / 2) / P);
    }
    s += step;
  }
  if (lane == 0) {
    n_smarks[blockIdx.x] = (int32_t)count;
    reach[2 * blockIdx.x] = max_l;
    reach[2 * blockIdx.x + 1] = max_r;
  }
}

// the first j in [0, Ms) with sm[j] > v, Ms when there is none
__device__ __forceinline__ int64_t ps_first_above(const wh::ckp<const int64_t>& sm, int64_t Ms, int64_t v) {
  int64_t lo = 0, hi = Ms;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (sm[mid] > v) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// y[t] = sum over the grains j with -Lw < t - s_j < Rw, j ascending, of w x[a + (flip ? -tau : tau)], over max(W, 1) with norm.
// A grain reaches t only if t - max Rw < s_j < t + max Lw: the tile's candidates are one range of the increasing list.
__global__ __launch_bounds__(kPsTile) void psola_ola_kernel(const PsUtt* __restrict__ meta, int norm, const double* __restrict__ x_,
                                                            const int64_t* __restrict__ smarks_, const uint8_t* __restrict__ flip_,
                                                            const int32_t* __restrict__ n_smarks_, const int64_t* __restrict__ centre_,
                                                            const int32_t* __restrict__ lw_, const int32_t* __restrict__ rw_,
                                                            const int32_t* __restrict__ reach_, double* __restrict__ y_) {
  const PsUtt m = meta[blockIdx.y];
  const int64_t t0 = (int64_t)blockIdx.x * kPsTile, t = t0 + threadIdx.x;
  if (t0 >= m.n_out) return;  // (uniform over the workgroup)
  const wh::ckp<const int32_t> n_smarks = wh::ck_make(n_smarks_, gridDim.y, wh::WH_CK_IN);
  const wh::ckp<const int32_t> reach = wh::ck_make(reach_, 2 * (long long)gridDim.y, wh::WH_CK_IN);
  const int64_t Ms = min((int64_t)max(n_smarks[blockIdx.y], 0), m.smark_cap);
  const wh::ckp<const double> xu = wh::ck_make(x_ + m.x_off, m.n, wh::WH_CK_WAVEFORM);
  const wh::ckp<const int64_t> smarks = wh::ck_make(smarks_ + m.smark_off, Ms, wh::WH_CK_IN);
  const wh::ckp<const uint8_t> flip = wh::ck_make(flip_ + m.smark_off, Ms, wh::WH_CK_IN);
  const wh::ckp<const int64_t> centre = wh::ck_make(centre_ + m.smark_off, Ms, wh::WH_CK_IN);
  const wh::ckp<const int32_t> lw = wh::ck_make(lw_ + m.smark_off, Ms, wh::WH_CK_IN);
  const wh::ckp<const int32_t> rw = wh::ck_make(rw_ + m.smark_off, Ms, wh::WH_CK_IN);
  const wh::ckp<double> y = wh::ck_make(y_ + m.y_off, m.n_out, wh::WH_CK_OUT);
  const int64_t j0 = ps_first_above(smarks, Ms, t0 - reach[2 * blockIdx.y + 1]);
  const int64_t j1 = ps_first_above(smarks, Ms, t0 + (kPsTile - 2) + reach[2 * blockIdx.y]);
  double num = 0.0, wsum = 0.0;
#pragma unroll 1
  for (int64_t j = j0; j < j1; ++j) {  // (the grain's record is one address for the workgroup)
    const int64_t tau = t - smarks[j];
    const int left = lw[j], right = rw[j];
    if (tau > -(int64_t)left && tau < (int64_t)right) {
      const double u = (double)(tau < 0 ? -tau : tau) / (double)(tau < 0 ? left : right);
      const double w = 1.0 - (u * u) * (3.0 - 2.0 * u);
      const double v = ps_read(xu, centre[j] + (flip[j] ? -tau : tau), m.n);
      num = num + w * v;
      wsum = wsum + w;
    }
  }
  if (t < m.n_out) y[t] = norm ? num / (wsum > 1.0 ? wsum : 1.0) : num;
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace

extern "C" int wh_psola(wh_ctx* ctx, void* stream, int n_utt, const int64_t* h_x_off, const int64_t* h_y_off,
                        const int64_t* h_pa_off, const int64_t* h_ps_off, const int64_t* h_mark_off, const int64_t* h_smark_off,
                        int grid, int unvoiced_hop, int tol, int pmin, int smin, int norm, const double* x, const int32_t* per_a,
                        const int32_t* per_s, const int64_t* src, double* y, int64_t* marks, int32_t* mark_period,
                        int32_t* n_marks, int64_t* smarks, int32_t* sel, uint8_t* flip, int32_t* n_smarks) {
  const char* where = "wh_psola";
  if (!ctx) return wh::fail_msg(where, "null argument");
  WH_ENTER(ctx);
  if (n_utt < 0) return wh::fail_msg(where, "negative utterance count");
  if (n_utt > 65535) return wh::fail_msg(where, "at most 65535 utterances per call");
  if (grid < 1 || grid > kPsMaxGrid) return wh::fail_msg(where, "the grid must be in [1, 4096]");
  if (unvoiced_hop < 1 || unvoiced_hop > kPsMaxHop) return wh::fail_msg(where, "the unvoiced hop must be in [1, 2048]");
  if (tol < 0 || tol > kPsMaxTol) return wh::fail_msg(where, "the tolerance must be in [0, 512]");
  if (pmin < 2 || pmin > kPsMaxPeriod) return wh::fail_msg(where, "the smallest period must be in [2, 2048]");
  if (smin < 1 || smin > kPsMaxPeriod) return wh::fail_msg(where, "the smallest synthesis step must be in [1, 2048]");
  if (norm != 0 && norm != 1) return wh::fail_msg(where, "norm must be 0 or 1");
  if (n_utt == 0) return 0;
  if (!h_x_off || !h_y_off || !h_pa_off || !h_ps_off || !h_mark_off || !h_smark_off) return wh::fail_msg(where, "null argument");
  const int B = n_utt;
  // every analysis step is at least a_min samples, every synthesis step at least s_min
  const int64_t a_min = std::min(unvoiced_hop, pmin - std::min(tol, pmin / 4)), s_min = std::min(unvoiced_hop, smin);
  std::vector<PsUtt> meta(B);
  int64_t max_out = 0;
  for (int u = 0; u < B; ++u) {
    PsUtt& m = meta[u];
    if (!wh::utt_span(h_x_off, u, &m.x_off, &m.n) || !wh::utt_span(h_y_off, u, &m.y_off, &m.n_out) ||
        !wh::utt_span(h_pa_off, u, &m.pa_off, &m.ka) || !wh::utt_span(h_ps_off, u, &m.ps_off, &m.ks) ||
        !wh::utt_span(h_mark_off, u, &m.mark_off, &m.mark_cap) || !wh::utt_span(h_smark_off, u, &m.smark_off, &m.smark_cap))
      return wh::fail_msg(where, "offsets must start at or above 0 and be monotone");
    if (m.n > ((int64_t)1 << 40) || m.n_out > ((int64_t)1 << 40)) return wh::fail_msg(where, "an utterance is too long for one call");
    if (m.ka != m.n / grid + 1) return wh::fail_msg(where, "an utterance's analysis track must have n / grid + 1 entries");
    if (m.ks != m.n_out / grid + 1) return wh::fail_msg(where, "an utterance's target tracks must have n_out / grid + 1 entries");
    if (m.mark_cap < ceil_div(m.n, a_min) + 1 || m.mark_cap > 0x7fffffffLL)
      return wh::fail_msg(where, "an utterance's mark capacity must be at least ceil(n / min(U, pmin - min(tol, pmin / 4))) + 1");
    if (m.smark_cap < ceil_div(m.n_out, s_min) + 1 || m.smark_cap > 0x7fffffffLL)
      return wh::fail_msg(where, "an utterance's synthesis mark capacity must be at least ceil(n_out / min(U, smin)) + 1");
    max_out = std::max(max_out, m.n_out);
  }
  if (!per_a || !per_s || !src || (!x && h_x_off[B] > 0) || (!y && h_y_off[B] > 0)) return wh::fail_msg(where, "null argument");
  if (ceil_div(max_out, kPsTile) > 0x7fffffffLL) return wh::fail_msg(where, "an utterance is too long for one call");
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_mark = h_mark_off[B], n_smark = h_smark_off[B];
  wh::Carve carve;
  const auto r_marks = carve.take_if<int64_t>(!marks, n_mark);
  const auto r_period = carve.take_if<int32_t>(!mark_period, n_mark);
  const auto r_n_marks = carve.take_if<int32_t>(!n_marks, B);
  const auto r_smarks = carve.take_if<int64_t>(!smarks, n_smark);
  const auto r_sel = carve.take_if<int32_t>(!sel, n_smark);
  const auto r_flip = carve.take_if<uint8_t>(!flip, n_smark);
  const auto r_n_smarks = carve.take_if<int32_t>(!n_smarks, B);
  const auto r_centre = carve.take<int64_t>(n_smark);  // per grain: the analysis mark it is cut around,
  const auto r_lw = carve.take<int32_t>(n_smark);      // its left
  const auto r_rw = carve.take<int32_t>(n_smark);      // and right half widths;
  const auto r_reach = carve.take<int32_t>(2 * (int64_t)B);  // per utterance the greatest of each
  if (int rc = wh::ws_reserve(ctx, carve)) return rc;
  if (!marks) marks = r_marks.at(ctx->ws);
  if (!mark_period) mark_period = r_period.at(ctx->ws);
  if (!n_marks) n_marks = r_n_marks.at(ctx->ws);
  if (!smarks) smarks = r_smarks.at(ctx->ws);
  if (!sel) sel = r_sel.at(ctx->ws);
  if (!flip) flip = r_flip.at(ctx->ws);
  if (!n_smarks) n_smarks = r_n_smarks.at(ctx->ws);
  int64_t* d_centre = r_centre.at(ctx->ws);
  int32_t* d_lw = r_lw.at(ctx->ws);
  int32_t* d_rw = r_rw.at(ctx->ws);
  int32_t* d_reach = r_reach.at(ctx->ws);
  PsUtt* d_meta = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "ps.meta", meta, &d_meta)) return rc;
  const PsParams pr = {grid, unvoiced_hop, tol, pmin, smin, norm};
  // the template and the candidate region at the largest period (32 KB at D = 0, 40 KB at D = 512)
  const int dmax = std::min(tol, kPsMaxPeriod / 4);
  const size_t lds = sizeof(double) * (size_t)(2 * kPsMaxPeriod + 2 * dmax);
  // one instantiation per count of candidates that a thread runs side by side
  const int rc = wh::dispatch_sim_width(dmax, [&](auto u) {
    const auto kernel = psola_marks_kernel<decltype(u)::value>;
    if (int e = wh::allow_lds(kernel, lds)) return e;
    return wh::launch(ctx, st, "psola_marks_kernel", kernel, dim3((unsigned)B), dim3(kPsThreads), lds, d_meta, pr, dmax, x, per_a,
                      marks, mark_period, n_marks);
  });
  if (rc) return rc;
  WH_LAUNCH(ctx, st, "psola_smarks_kernel", psola_smarks_kernel, dim3((unsigned)B), dim3(WH_WAVE), 0, d_meta, pr, per_s, src,
            marks, mark_period, n_marks, smarks, sel, flip, n_smarks, d_centre, d_lw, d_rw, d_reach);
  if (max_out > 0)
    WH_LAUNCH(ctx, st, "psola_ola_kernel", psola_ola_kernel, dim3((unsigned)ceil_div(max_out, kPsTile), B), dim3(kPsTile), 0,
              d_meta, norm, x, smarks, flip, n_smarks, d_centre, d_lw, d_rw, d_reach, y);
  return 0;
}
