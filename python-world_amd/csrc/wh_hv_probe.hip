// Test hook for Harvest's back end: wh_harvest_contour_probe runs hv_prune_kernel (wh_hv_refine.hip) and the contour
// kernels (wh_hv_contour.hip) on candidate pools and per-frame lists that the CALLER supplies, in the form hv_refine_kernel
// leaves them, through the launchers wh_harvest itself calls (hv_launch_prune, hv_launch_contour: the same grids, the same
// HcLayout), and reads the intermediate rows and the section table back.  Nothing in the library calls it
// (tests/test_hip_harvest_contour.py does).  Built unfused, like wh_hv_contour.hip.
#include <math.h>

#include <algorithm>

#include "wh_host.h"
#include "wh_hv_types.h"

extern "C" int wh_harvest_contour_probe(wh_ctx* ctx, void* stream, int mode, int n_utt, const int64_t* h_nf1,
                                        const int64_t* h_frame_off, const double* tp, const double* rf0, const double* rsc,
                                        int64_t pool_n, const int64_t* h_lst, uint32_t* keep, double* f0_out,
                                        double* vuv_out, double* rows, int32_t* h_nsec, int32_t* h_secs, int64_t sec_cap) {
  using namespace wh;
  const char* const me = "wh_harvest_contour_probe";
  if (!ctx || !h_nf1 || !h_frame_off || !tp || !f0_out || !vuv_out || !rows || !h_nsec || !h_secs)
    return fail_msg(me, "null argument");
  if (mode < 0 || mode > 2) return fail_msg(me, "mode is 0 (contour, caller's keep masks), 1 (prune + contour) or 2 (smoothing + pick)");
  if (mode != 2 && (!rf0 || !rsc || !h_lst || !keep)) return fail_msg(me, "null argument");
  if (n_utt < 1 || n_utt > 65535) return fail_msg(me, "n_utt out of range");
  if (pool_n < 0 || sec_cap < 0) return fail_msg(me, "negative capacity");
  WH_ENTER(ctx);
  hipStream_t st = (hipStream_t)stream;
  HvPlan p;  // only what the two stages read: B, meta[].f1_off / nf1 / f_off / nf, the maxima and the frame total
  p.B = n_utt;
  p.meta.resize(n_utt);
  for (int u = 0; u < n_utt; ++u) {
    HvUtt& m = p.meta[u];
    m = HvUtt{};
    if (h_nf1[u] < 1 || h_nf1[u] > (int64_t)1 << 24) return fail_msg(me, "nf1 must be at least 1 (and at most 2^24)");
    if (h_frame_off[u] < 0 || h_frame_off[u + 1] <= h_frame_off[u]) return fail_msg(me, "every utterance needs an output frame");
    m.nf1 = h_nf1[u];
    m.f1_off = p.f1_tot;
    p.f1_tot += m.nf1;
    m.f_off = h_frame_off[u];
    m.nf = h_frame_off[u + 1] - h_frame_off[u];
    p.max_nf1 = std::max(p.max_nf1, m.nf1);
    p.max_nf = std::max(p.max_nf, m.nf);
  }
  if (mode != 2)
    for (int64_t f = 0; f < p.f1_tot; ++f) {
      if (h_lst[f] < 0) return fail_msg(me, "a list leaves the pool");
      const int64_t slot = h_lst[f] >> 8, cnt = h_lst[f] & 255;
      if (cnt > kRows) return fail_msg(me, "a list holds more than kRows candidates");
      if (slot > pool_n || cnt > pool_n - slot) return fail_msg(me, "a list leaves the pool");
    }
  Carve c;
  const auto r_f0 = c.take<double>(pool_n), r_sc = c.take<double>(pool_n);
  const auto r_keep = c.take<uint32_t>(4 * p.f1_tot);
  const auto r_lst = c.take<int64_t>(p.f1_tot);
  const auto r_ct = hv_carve_contour(c, p);
  if (int rc = ws_reserve(ctx, c)) return rc;
  HvDev d{};
  d.rf0 = r_f0.at(ctx->ws);
  d.rsc = r_sc.at(ctx->ws);
  d.keep = r_keep.at(ctx->ws);
  d.lst = r_lst.at(ctx->ws);
  d.ct = r_ct.at(ctx->ws);
  if (int rc = persistent_upload(ctx, st, "hv.probe_meta", p.meta, &d.meta)) return rc;
  if (mode == 2) {
    if (int rc = hv_launch_smooth_pick(ctx, st, p, d, rows, tp, f0_out, vuv_out)) return rc;
    return hv_read_contour(st, p, d, rows, h_nsec, h_secs, sec_cap);
  }
  int64_t* d_lst = nullptr;  // (a persistent upload: the host list may be pageable memory that a failing call leaves early)
  {
    const std::vector<int64_t> lst(h_lst, h_lst + p.f1_tot);
    if (int rc = persistent_upload(ctx, st, "hv.probe_lst", lst, &d_lst)) return rc;
  }
  WH_CHECK(hipMemcpyAsync(d.lst, d_lst, sizeof(int64_t) * p.f1_tot, hipMemcpyDeviceToDevice, st));
  if (pool_n) {
    WH_CHECK(hipMemcpyAsync(d.rf0, rf0, sizeof(double) * pool_n, hipMemcpyDeviceToDevice, st));
    WH_CHECK(hipMemcpyAsync(d.rsc, rsc, sizeof(double) * pool_n, hipMemcpyDeviceToDevice, st));
  }
  if (mode == 0) {
    WH_CHECK(hipMemcpyAsync(d.keep, keep, sizeof(uint32_t) * 4 * p.f1_tot, hipMemcpyDeviceToDevice, st));
  } else {
    WH_CHECK(hipMemsetAsync(d.keep, 0xff, sizeof(uint32_t) * 4 * p.f1_tot, st));  // (a word the kernel left out would show)
    if (int rc = hv_launch_prune(ctx, st, p, d)) return rc;
  }
  if (int rc = hv_launch_contour(ctx, st, p, d, tp, f0_out, vuv_out, nullptr)) return rc;
  WH_CHECK(hipMemcpyAsync(keep, d.keep, sizeof(uint32_t) * 4 * p.f1_tot, hipMemcpyDeviceToDevice, st));
  return hv_read_contour(st, p, d, rows, h_nsec, h_secs, sec_cap);
}
