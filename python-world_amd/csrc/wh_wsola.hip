// ================================================================================================
// Waveform-similarity overlap-add (WSOLA): the timing of a recording changed without analysis and synthesis.  Frames of
// 2 H - 1 samples are copied from the input to an integer output hop H; every frame's input start may move by up to D
// samples from its nominal position to where the input continues the frame before best (normalised cross-correlation).
// Time-stretching by the f0 ratio and resampling back (wh_resample_poly) is Kobayashi and Toda's f0 transformation for
// vocoder-free conversion.  Contract: include/world_hip.h; tests/_wsola_reference.py is the same
// in NumPy, and both outputs (the shifts and y) are compared bit for bit.
//
//   wsola_search_kernel   one workgroup per utterance, a loop over its frames (frame m's template starts where frame
//                         m - 1 was taken from: the chain is sequential).  Per frame the template (L doubles) and the
//                         candidate region (L + 2 D doubles) are staged in LDS, zero-filled outside the utterance;
//                         thread i runs the two add chains of the candidates i, i + 256, .. side by side, j ascending,
//                         each product and sum rounded on its own (build.py's default -ffp-contract=off); one
//                         workgroup argmax on the key (score, -|d|, d < 0), a total order.  From the staged buffers
//                         to the winning shift this is wh::sim_search (wh_simsearch.h), shared with wh_psola.hip.
//   wsola_ola_kernel      every output sample from the list of frame starts: at most two terms, the earlier frame first.
// The only value-dependent index is the shift, confined to [-D, D] by construction; positions are added in unsigned
// arithmetic (any int64 is a legal position) and every read of x is range-tested.  No atomics.
// ================================================================================================
#include "wh_host.h"
#include "wh_simsearch.h"

#include <algorithm>

namespace {

constexpr int kWsMaxHop = 1024, kWsMaxTol = wh::kSimMaxTol;
constexpr int kWsThreads = wh::kSimThreads;  // (the search's workgroup: wh_simsearch.h)

struct WsUtt {
  int64_t x_off;    // first input sample
  int64_t n;        // input samples
  int64_t y_off;    // first output sample
  int64_t n_out;    // output samples
  int64_t pos_off;  // first frame in pos, c and delta
  int64_t n_frames; // M = ceil(n_out / H) + 1, or 0
};

// x[i] for a position in unsigned arithmetic: anything outside [0, n) — negative positions wrap beyond 2^63 — reads 0.0
__device__ __forceinline__ double ws_read(const wh::ckp<const double>& xu, uint64_t i, uint64_t n) { return i < n ? xu[(long long)i] : 0.0; }

template <int U>
__global__ __launch_bounds__(kWsThreads) void wsola_search_kernel(const WsUtt* __restrict__ meta, const int64_t* __restrict__ pos_,
                                                                  int hop, int tol, const double* __restrict__ x_,
                                                                  int64_t* __restrict__ c_, int32_t* __restrict__ delta_) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double s_score_[wh::kSimWaves];
  __shared__ int s_delta_[wh::kSimWaves];
  const WsUtt m = meta[blockIdx.x];
  if (m.n_frames == 0) return;  // (uniform over the workgroup)
  const int L = 2 * hop - 1, R = L + 2 * tol;
  const int tid = threadIdx.x;
  // (wh::ckp<T> is T* in every shipped build; the bounds build checks each access against the range named here)
  const wh::ckp<double> tpl = wh::ck_make(reinterpret_cast<double*>(smem), L, wh::WH_CK_LDS_MAIN);       // the template
  // (the region starts one double behind the template's odd length, on an even offset: with both LDS bases a multiple of 16
  // bytes apart the chain loop of wh::sim_search addresses them from one pointer without a negative displacement)
  const wh::ckp<double> reg = wh::ck_make(reinterpret_cast<double*>(smem) + L + 1, R, wh::WH_CK_LDS_AUX);  // x[pos - D ..]
  const wh::ckp<double> s_score = wh::ck_make(s_score_, wh::kSimWaves, wh::WH_CK_LDS_SCRATCH);
  const wh::ckp<int> s_delta = wh::ck_make(s_delta_, wh::kSimWaves, wh::WH_CK_LDS_SCRATCH);
  const wh::ckp<const double> xu = wh::ck_make(x_ + m.x_off, m.n, wh::WH_CK_WAVEFORM);
  const wh::ckp<const int64_t> pos = wh::ck_make(pos_ + m.pos_off, m.n_frames, wh::WH_CK_IN);
  const wh::ckp<int64_t> c = wh::ck_make(c_ + m.pos_off, m.n_frames, wh::WH_CK_OUT);
  const wh::ckp<int32_t> dl = wh::ck_make(delta_ ? delta_ + m.pos_off : delta_, delta_ ? m.n_frames : 0, wh::WH_CK_OUT);
  const uint64_t n = (uint64_t)m.n;
  uint64_t c_prev = (uint64_t)pos[0];  // delta_0 = 0
  if (tid == 0) {
    c[0] = (int64_t)c_prev;
    if (delta_) dl[0] = 0;
  }
#pragma unroll 1
  for (int64_t f = 1; f < m.n_frames; ++f) {
    const uint64_t p = (uint64_t)pos[f];
    const uint64_t tb = c_prev + (uint64_t)hop, rb = p - (uint64_t)tol;
    // (the last frame's readers are behind its second barrier)
    for (int j = tid; j < L; j += kWsThreads) tpl[j] = ws_read(xu, tb + (uint64_t)j, n);
    for (int i = tid; i < R; i += kWsThreads) reg[i] = ws_read(xu, rb + (uint64_t)i, n);
    __syncthreads();
    const int best_d = wh::sim_search<U>(tpl, reg, L, tol, s_score, s_delta, tid);
    // (candidate 0 always exists, so |best_d| <= D; the slots are rewritten behind the next frame's first barrier)
    c_prev = p + (uint64_t)(int64_t)best_d;
    if (tid == 0) {
      c[f] = (int64_t)c_prev;
      if (delta_) dl[f] = best_d;
    }
  }
}

// y[t] = sum over the frames m with 0 <= t - (m - 1) H < 2 H - 1, m ascending, of win[t - (m - 1) H] x[c_m + t - (m - 1) H]:
// frame t / H in its second half (not for its last sample, the window has 2 H - 1), then frame t / H + 1 in its first.
__global__ __launch_bounds__(256) void wsola_ola_kernel(const WsUtt* __restrict__ meta, const int64_t* __restrict__ c_, int hop,
                                                        const double* __restrict__ win_, const double* __restrict__ x_,
                                                        double* __restrict__ y_) {
  const WsUtt m = meta[blockIdx.y];
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= m.n_out) return;
  const wh::ckp<const double> xu = wh::ck_make(x_ + m.x_off, m.n, wh::WH_CK_WAVEFORM);
  const wh::ckp<const int64_t> c = wh::ck_make(c_ + m.pos_off, m.n_frames, wh::WH_CK_IN);
  const wh::ckp<const double> win = wh::ck_make(win_, 2 * hop - 1, wh::WH_CK_TABLE);
  const wh::ckp<double> y = wh::ck_make(y_ + m.y_off, m.n_out, wh::WH_CK_OUT);
  const uint64_t n = (uint64_t)m.n;
  const int64_t q = t / hop;
  const int r = (int)(t - q * hop);
  double acc = 0.0;
  if (r < hop - 1) acc = acc + win[r + hop] * ws_read(xu, (uint64_t)c[q] + (uint64_t)(r + hop), n);
  acc = acc + win[r] * ws_read(xu, (uint64_t)c[q + 1] + (uint64_t)r, n);
  y[t] = acc;
}

}  // namespace

extern "C" int wh_wsola(wh_ctx* ctx, void* stream, int n_utt, const int64_t* h_x_off, const int64_t* h_y_off,
                        const int64_t* h_pos_off, const int64_t* h_pos, int hop, int tol, const double* h_win, const double* x,
                        double* y, int32_t* delta) {
  const char* where = "wh_wsola";
  if (!ctx) return wh::fail_msg(where, "null argument");
  WH_ENTER(ctx);
  if (n_utt < 0) return wh::fail_msg(where, "negative utterance count");
  if (n_utt > 65535) return wh::fail_msg(where, "at most 65535 utterances per call");
  if (hop < 1 || hop > kWsMaxHop) return wh::fail_msg(where, "the hop must be in [1, 1024]");
  if (tol < 0 || tol > kWsMaxTol) return wh::fail_msg(where, "the tolerance must be in [0, 512]");
  if (n_utt == 0) return 0;
  if (!h_x_off || !h_y_off || !h_pos_off) return wh::fail_msg(where, "null argument");
  const int B = n_utt;
  std::vector<WsUtt> meta(B);
  int64_t max_out = 0;
  for (int u = 0; u < B; ++u) {
    WsUtt& m = meta[u];
    if (!wh::utt_span(h_x_off, u, &m.x_off, &m.n) || !wh::utt_span(h_y_off, u, &m.y_off, &m.n_out) ||
        !wh::utt_span(h_pos_off, u, &m.pos_off, &m.n_frames))
      return wh::fail_msg(where, "offsets must start at or above 0 and be monotone");
    const int64_t want = m.n_out > 0 ? (m.n_out + hop - 1) / hop + 1 : 0;
    if (m.n_frames != want)
      return wh::fail_msg(where, "an utterance's position list must have ceil(n_out / hop) + 1 entries (none when its output is empty)");
    max_out = std::max(max_out, m.n_out);
  }
  const int64_t n_pos = h_pos_off[B];
  if (h_y_off[B] == 0) return 0;
  if (!h_pos || !h_win || !y || (!x && h_x_off[B] > 0)) return wh::fail_msg(where, "null argument");
  if ((max_out + 255) / 256 > 0x7fffffffLL) return wh::fail_msg(where, "an utterance is too long for one call");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = wh::ws_reserve(ctx, sizeof(int64_t) * (size_t)(n_pos + 8))) return rc;
  int64_t* d_c = reinterpret_cast<int64_t*>(ctx->ws);  // every frame's input start: the search writes it, the overlap-add reads it
  WsUtt* d_meta = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "ws.meta", meta, &d_meta)) return rc;
  void* d_pos = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "ws.pos", h_pos, (size_t)n_pos * sizeof(int64_t), &d_pos)) return rc;
  void* d_win = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "ws.win", h_win, (size_t)(2 * hop - 1) * sizeof(double), &d_win)) return rc;
  // the template and the candidate region, sized from this call's hop and tolerance (5 KB at H = 128, D = 80; 41 KB at the limits)
  const size_t lds = sizeof(double) * (size_t)(2 * (2 * hop - 1) + 1 + 2 * tol);  // (+ 1: the pad between the two)
  // one instantiation per count of candidates that a thread runs side by side
  const int rc = wh::dispatch_sim_width(tol, [&](auto u) {
    const auto kernel = wsola_search_kernel<decltype(u)::value>;
    if (int e = wh::allow_lds(kernel, lds)) return e;
    return wh::launch(ctx, st, "wsola_search_kernel", kernel, dim3((unsigned)B), dim3(kWsThreads), lds, d_meta, d_pos, hop, tol,
                      x, d_c, delta);
  });
  if (rc) return rc;
  WH_LAUNCH(ctx, st, "wsola_ola_kernel", wsola_ola_kernel, dim3((unsigned)((max_out + 255) / 256), B), dim3(256), 0, d_meta, d_c,
            hop, (const double*)d_win, x, y);
  return 0;
}
