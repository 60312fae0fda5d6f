// Harvest F0 estimator, batched.  Replaces harvest() of the reference (world/harvest.py:17-54).
//
// This file: the C entry points, the plan of a call (geometry, run-time forms, workspace layout) and the stage sequence.
// Front end (wh_hv_front.hip):
//   hv_iir_fwd/bwd   : zero-phase Chebyshev-I decimation to ~8 kHz, SciPy filtfilt semantics (odd
//                      extension by 9, steady-state initial conditions), chunk-parallel with state warm-up
//                      (harvest.py:58-71,584-609)
//   band_events      : 152 band-pass channels + zero-crossing compaction (wh_bands.h): overlap-save FFT products
//                      (one forward transform per 4096-sample tile shared by all channels), direct FIR as fallback
//   hv_raw_kernel    : per (1 ms frame, channel) interpolation of the four interval-F0 trains (harvest.py:252-278),
//                      from (location, frequency) intervals staged per 128-frame tile
//   hv_detect_kernel : per frame: runs of >= 10 live channels -> candidate = mean (harvest.py:88-110)
//   hv_rawdet_kernel : the two in one transposed pass, for batches of kRawdetMinTiles tiles and more
// Refinement (wh_hv_refine.hip):
//   hv_refine_kernel : every overlapped candidate (+-3 frames, harvest.py:114-125) refined by instantaneous frequency
//                      at <= 6 harmonics.  The reference farms ~178 k two-FFT calls per 10 s utterance to a process
//                      pool (harvest.py:131-211); here two lanes per candidate accumulate only the harmonic bins as
//                      direct DFT sums — window pairs from a per-length table (the frame time cancels out of the
//                      reference's window argument), twiddles from an LDS table, samples from an LDS stage of the
//                      frames a workgroup takes; a 16-lane rotation form remains for f0 floors whose tables do not
//                      fit LDS.  The candidates of a frame that share window length and harmonic bins — mostly the seven
//                      overlapped copies of one pitch track — share ONE pass over the samples (equal-key classes), every
//                      member taking its own score from the class's spectra; 32 frames per workgroup
//   hv_prune_kernel  : neighbour-frame consistency test (harvest.py:215-248), 16 frames per workgroup
// Back end (wh_hv_contour.hip): contour tracking, smoothing, 5 ms pick.
#include <math.h>

#include <algorithm>

#include "wh_host.h"
#include "wh_device.h"  // WH_MAX_TWIDDLE
#include "wh_hv_types.h"

namespace {
using namespace wh;

// The transposed raw + detect kernel runs one wave per (utterance, 64-frame tile), each walking all channels: a handful of
// utterances is a few hundred waves with a 152-step chain each (one 4.6 s utterance: 74), where hv_raw_kernel spreads the
// same work over channels x utterances x segments workgroups — the reference's own benchmark, ONE encode of its test
// recording, went from 2.5 to 3.0 ms.  Below this many tiles in the batch the pair of kernels runs instead (~52 utterances
// of 10 s; measured: 1 / 8 / 32 / 64 utterances 0.46 / 0.46 / 0.96 / 1.54 ms fused against 0.15 / 0.29 / 0.82 / 1.52 ms for
// the pair).  WH_HV_RAWDET_MIN_TILES in the environment overrides it: tests run both forms on the same input.
constexpr int64_t kRawdetMinTiles = 8192;

const char kCapsMismatch[] = "wh_harvest_set_event_caps: one capacity per (utterance, channel) of THIS batch expected";

// Geometry of every utterance, totals, maxima and the run-time forms of one call.  Host only; nullptr: ok, else the
// error text.  `caps`: explicit list capacities, one per (utterance, channel), or empty; caps_worst: the bound no signal
// exceeds; want_map: the caller reads the [channel][frame] candidate map out.
const char* plan_harvest(const wh_batch* b, double fs, double f0_floor, int decimation_ratio, bool has_filter, int n_bands,
                         const double* h_band_f0, const int32_t* h_band_half, const std::vector<int64_t>& caps,
                         bool caps_worst, bool want_map, HvPlan& p) {
  const int B = p.B = b->n_utt;
  const int r = p.r = decimation_ratio < 1 ? 1 : decimation_ratio;
  p.n_bands = n_bands;
  // The anti-aliasing filter runs whenever fs > 8000 Hz — ALSO when the ratio rounds to 1 (8 kHz < fs < 12 kHz, e.g.
  // 11.025 kHz): the reference branches on `fs <= target_fs` (harvest.py:60) and then low-pass filters at 0.8 / r of
  // Nyquist with r = 1, keeping every sample.  The host says so by handing over the coefficients (a0 != 0).
  const bool filtered = p.filtered = r > 1 || has_filter;
  const double fs_d = p.fs_d = fs / r;
  p.ti.resize(n_bands * 3);
  for (int i = 0; i < n_bands; ++i) {
    const int lb = 2 * h_band_half[i] + 1;
    p.ti[i] = p.taps_total;
    p.ti[n_bands + i] = lb;
    p.ti[2 * n_bands + i] = h_band_half[i];  // filtered[(h+1) + g] == filtered[bias + 1 + g] with bias = h
    p.taps_total += lb;
    p.max_lb = std::max(p.max_lb, lb);
    p.h_max = std::max(p.h_max, (int)h_band_half[i]);
  }
  const int pad = p.pad = p.max_lb + 2;
  p.hmax = (int)ceil(3 * fs_d / f0_floor / 2) + 1;
  if (2 * p.hmax + 1 > WH_MAX_TWIDDLE / 2) return "f0_floor too low for the twiddle tables";
  if (!caps_worst && !caps.empty() && caps.size() != (size_t)B * n_bands) return kCapsMismatch;
  p.meta.resize(B);
  p.e_off.resize((size_t)B * n_bands);
  p.e_cap.resize((size_t)B * n_bands);
  p.tile_off.assign(B + 1, 0);
  for (int u = 0; u < B; ++u) {
    HvUtt& m = p.meta[u];
    m.x_off = b->h_x_off[u];
    m.n = b->h_x_off[u + 1] - b->h_x_off[u];
    if (m.n < 32) return "utterance shorter than 32 samples";
    if (filtered) {
      m.offset = (int64_t)ceil(140.0 / r) * r;
      m.nd = m.n + 2 * m.offset;
      const double n_out = ceil((double)m.nd / r);
      const int64_t n_beg = (int64_t)(r - (r * n_out - m.nd));
      const int64_t picks = (m.nd - (n_beg - 1) + r - 1) / r;
      m.ylen = picks - 2 * (m.offset / r);
      m.pick0 = (n_beg - 1) + (m.offset / r) * r;
    } else {
      m.offset = 0;
      m.nd = m.n;
      m.ylen = m.n;
      m.pick0 = 0;
    }
    m.t_off = p.t_tot;
    p.t_tot += m.nd + 2 * kFPad;
    m.y_off = p.y_tot;
    p.y_tot += m.ylen;
    m.z_off = p.z_tot;
    p.z_tot += m.ylen + 2 * pad;
    m.nf1 = (int64_t)(1000.0 * (double)m.n / fs / 1 + 1);
    m.f1_off = p.f1_tot;
    p.f1_tot += m.nf1;
    m.ntile = (m.nf1 + kRawTile - 1) / kRawTile;
    m.l_off = p.l_tot;
    p.l_tot += m.ntile * n_bands;
    m.f_off = b->h_frame_off[u];
    m.nf = b->h_frame_off[u + 1] - b->h_frame_off[u];
    for (int i = 0; i < n_bands; ++i) {
      // a band-limited channel centred on f crosses zero ~f times per second; 3x head-room + slack.  That is an
      // ESTIMATE: where the filtered signal is constant up to rounding (digital silence next to signal: the mean
      // removal of harvest.py:69 turns it into a DC level) the first difference changes sign at random, up to every
      // other sample.  Such a call raises WH_FLAG_EVENT_OVERFLOW, its counts stay exact (the walker counts on past a
      // full list), and the caller repeats it with them (wh_harvest_event_counts -> wh_harvest_set_event_caps) or with
      // the bound no signal exceeds, ylen / 2 + 2.
      int64_t cap = (int64_t)ceil((double)m.ylen / fs_d * h_band_f0[i] * 3.0) + 64;
      if (caps_worst) cap = m.ylen / 2 + 2;
      else if (!caps.empty()) cap = std::max<int64_t>(caps[(size_t)u * n_bands + i], 8);
      p.e_off[(size_t)u * n_bands + i] = p.e_tot;
      p.e_cap[(size_t)u * n_bands + i] = cap;
      p.e_tot += 4 * cap;
    }
    const int64_t tiles = (m.ylen + kOlsValid - 1) / kOlsValid;  // overlap-save tiles
    p.tile_off[u + 1] = p.tile_off[u] + tiles;
    p.max_tiles = std::max(p.max_tiles, tiles);
    p.max_len = std::max(p.max_len, m.nd + 2 * kFPad);
    p.max_ylen = std::max(p.max_ylen, m.ylen);
    p.max_nf1 = std::max(p.max_nf1, m.nf1);
    p.max_nf = std::max(p.max_nf, m.nf);
    p.max_ntile = std::max(p.max_ntile, m.ntile);
    p.batch_tiles += m.ntile;
  }
  // the block of kOlsN inputs must cover H + h + 1 + kOlsValid + 2 outputs for every channel
  p.use_ols = (2 * p.h_max + 1 + kOlsValid + 2 <= kOlsN) && pad >= p.h_max + 1;
  static const long rawdet_min_env = getenv("WH_HV_RAWDET_MIN_TILES") ? atol(getenv("WH_HV_RAWDET_MIN_TILES")) : -1;
  const int64_t rawdet_min = rawdet_min_env >= 0 ? rawdet_min_env : kRawdetMinTiles;
  p.use_rawdet = p.use_ols && p.batch_tiles >= rawdet_min;  // (its cursor hints come from the overlap-save walker)
  // the [channel][frame] candidate map (12 GB per 1024 x 10 s) and its bit map exist only where something reads them
  p.need_map = !p.use_rawdet || want_map;
  return nullptr;
}

// THE layout of the Harvest workspace: reserves it and points `d` at its regions, in carve order.  raw / live hold nothing
// without need_map, hint nothing without use_rawdet, the three spectra nothing without use_ols (a valid address all the same).
int carve_harvest(wh_ctx* ctx, const HvPlan& p, HvDev& d) {
  const int64_t B = p.B, nb = p.n_bands, f1 = p.f1_tot;
  const int64_t spec_bins = kOlsN / 2 + 1;
  wh::Carve c;
  const auto tmp = c.take<double>(p.t_tot);
  const auto y = c.take<double>(p.y_tot);
  const auto z = c.take<double>(p.z_tot);
  const auto mean = c.take<double>(B * (1 + kMeanParts));  // means, then the partial sums
  const auto e = c.take<double>(p.e_tot);
  const auto raw = c.take_if<double>(p.need_map, f1 * nb);
  const auto live = c.take_if<unsigned long long>(p.need_map, p.l_tot);
  const auto hint = c.take_if<int32_t>(p.use_rawdet, 4 * p.l_tot);
  const auto dc = c.take<double>(f1 * kMaxC);
  const auto dn = c.take<int32_t>(f1);
  const auto rf0 = c.take<double>(f1 * kRows);
  const auto rsc = c.take<double>(f1 * kRows);
  const auto keep = c.take<uint32_t>(4 * f1);
  const auto lst = c.take<int64_t>(f1);
  const auto ct = wh::hv_carve_contour(c, p);
  // overlap-save band filters: the channels' tap spectra, the tile spectra of every utterance, the real (zero-phase) tap spectra
  const auto tspec = c.take_if<double2>(p.use_ols, spec_bins * nb);
  const auto zspec = c.take_if<double2>(p.use_ols, spec_bins * p.tile_off[p.B]);
  const auto tre = c.take_if<double>(p.use_ols, spec_bins * nb);
  if (int rc = wh::ws_reserve(ctx, c)) return rc;
  void* ws = ctx->ws;
  d.tmp = tmp.at(ws); d.y = y.at(ws); d.z = z.at(ws); d.mean = mean.at(ws); d.e = e.at(ws);
  d.raw = raw.at(ws); d.live = live.at(ws); d.hint = hint.at(ws);
  d.dc = dc.at(ws); d.dn = dn.at(ws); d.rf0 = rf0.at(ws); d.rsc = rsc.at(ws); d.keep = keep.at(ws); d.lst = lst.at(ws);
  d.ct = ct.at(ws);
  d.tspec = tspec.at(ws); d.zspec = zspec.at(ws); d.tre = tre.at(ws);
  return 0;
}

}  // namespace

extern "C" int wh_harvest(wh_ctx* ctx, void* stream, const wh_batch* b, const double* x, const double* tp, double fs,
                          double f0_floor, double f0_ceil, double frame_period_ms, int decimation_ratio,
                          const double* h_ba, const double* h_zi, int n_bands, const double* h_band_f0,
                          const int32_t* h_band_half, const double* h_band_taps, double* f0_out, double* vuv_out,
                          double* dbg_y, double* dbg_raw, double* dbg_f0_1ms) {
  if (!ctx || !b || !x || !tp || !h_band_f0 || !h_band_half || !h_band_taps || !f0_out || !vuv_out)
    return wh::fail_msg("wh_harvest", "null argument");
  WH_ENTER(ctx);
  if (decimation_ratio > 1 && (!h_ba || !h_zi)) return wh::fail_msg("wh_harvest", "decimation filter missing");
  if (n_bands < 3 || n_bands > 1024) return wh::fail_msg("wh_harvest", "n_bands out of range");
  if (int rc = wh::tables_make_room(ctx)) return rc;
  hipStream_t st = (hipStream_t)stream;
  HvPlan p;
  if (const char* err = plan_harvest(b, fs, f0_floor, decimation_ratio, h_ba && h_zi && h_ba[4] != 0.0, n_bands, h_band_f0,
                                     h_band_half, ctx->hv_caps_next, ctx->hv_caps_worst, dbg_raw != nullptr, p)) {
    if (err == kCapsMismatch) ctx->hv_caps_next.clear();
    return wh::fail_msg("wh_harvest", err);
  }
  ctx->hv_caps_next.clear();  // explicit capacities serve one call
  HvDev d;
  if (int rc = carve_harvest(ctx, p, d)) return rc;
  {  // the lists' counts: a buffer of their own (wh_harvest_event_counts reads them after later stages have used the scratch)
    if (int rc = wh::persistent_scratch(ctx, "hv.counts", (size_t)p.B * n_bands * 4, &d.cnt)) return rc;
    ctx->hv_last_cnt = d.cnt;
    ctx->hv_last_cnt_lists = (int64_t)p.B * n_bands;
  }
  if (int rc = wh::hv_upload(ctx, st, p, h_band_taps, h_band_f0, d)) return rc;

  if (int rc = wh::hv_launch_decimate(ctx, st, p, x, h_ba, h_zi, d)) return rc;
  if (dbg_y) WH_CHECK(hipMemcpyAsync(dbg_y, d.y, sizeof(double) * p.y_tot, hipMemcpyDeviceToDevice, st));
  if (int rc = wh::hv_launch_band_events(ctx, st, p, d)) return rc;
  if (int rc = wh::hv_launch_raw_detect(ctx, st, p, f0_floor, f0_ceil, d, dbg_raw)) return rc;
  if (int rc = wh::hv_launch_refine(ctx, st, p, f0_floor, f0_ceil, d)) return rc;
  if (int rc = wh::hv_launch_prune(ctx, st, p, d)) return rc;
  return wh::hv_launch_contour(ctx, st, p, d, tp, f0_out, vuv_out, dbg_f0_1ms);
}

// Capacities of Harvest's zero-crossing lists (include/world_hip.h).  h_caps != NULL: one capacity per (utterance,
// channel) for the NEXT wh_harvest of this context (n = utterances x channels of that call); NULL with n == -1: every
// list sized for the bound no signal exceeds (ylen / 2 + 2) until reset; NULL with n == 0: back to the estimate.
extern "C" int wh_harvest_set_event_caps(wh_ctx* ctx, const int64_t* h_caps, int64_t n) {
  if (!ctx) return wh::fail_msg("wh_harvest_set_event_caps", "null context");
  if (h_caps) {
    if (n <= 0) return wh::fail_msg("wh_harvest_set_event_caps", "n must be utterances x channels");
    ctx->hv_caps_next.assign(h_caps, h_caps + n);
    return 0;
  }
  if (n != 0 && n != -1) return wh::fail_msg("wh_harvest_set_event_caps", "without capacities n is 0 (estimate) or -1 (bound)");
  ctx->hv_caps_next.clear();
  ctx->hv_caps_worst = n == -1;
  return 0;
}

// What the last wh_harvest of this context counted: h_caps_out[u * n_bands + i] = the longest of the four crossing
// trains of channel i of utterance u — exact also when the call overflowed its lists (WH_FLAG_EVENT_OVERFLOW), so a
// repeat with these capacities fits.  Waits for `stream`.
extern "C" int wh_harvest_event_counts(wh_ctx* ctx, void* stream, int64_t* h_caps_out, int64_t n) {
  if (!ctx || !h_caps_out) return wh::fail_msg("wh_harvest_event_counts", "null argument");
  WH_ENTER(ctx);
  if (!ctx->hv_last_cnt || n != ctx->hv_last_cnt_lists)
    return wh::fail_msg("wh_harvest_event_counts", "n is not utterances x channels of this context's last wh_harvest");
  std::vector<int32_t> cnt((size_t)n * 4);
  hipStream_t st = (hipStream_t)stream;
  WH_CHECK(hipMemcpyAsync(cnt.data(), ctx->hv_last_cnt, sizeof(int32_t) * cnt.size(), hipMemcpyDeviceToHost, st));
  WH_CHECK(hipStreamSynchronize(st));
  for (int64_t i = 0; i < n; ++i) {
    int32_t m = cnt[4 * i];
    for (int t = 1; t < 4; ++t) m = std::max(m, cnt[4 * i + t]);
    h_caps_out[i] = m;
  }
  return 0;
}
