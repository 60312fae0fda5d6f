// What the Harvest units share (wh_harvest.hip, wh_hv_front.hip, wh_hv_refine.hip, wh_hv_contour.hip): the
// per-utterance record, the constants of the candidate map, the plan of one call, its device
// pointers, and the stage launchers that cross unit boundaries.  Include after wh_host.h.
#pragma once
#include <vector>

namespace wh {

constexpr int kMaxC = 15;          // int(152/10 + 0.5): candidate rows per frame before overlapping
constexpr int kRows = 7 * kMaxC;   // overlapped candidate rows (shift-major, candidate-minor)
constexpr int kFPad = 9;           // filtfilt padlen
constexpr int kHChunk = 256;       // filter outputs per lane of the chunked decimation IIR (+ warm-up before each chunk)
constexpr int kMeanParts = 32;     // partial sums per utterance of the mean removal (hv_mean_part_kernel)
// frames per tile of the raw-candidate kernels = threads per workgroup (one wave per workgroup: 1.56 ms at config 3 against
// 1.66 for 128 and 1.79 for 256; 23.3 against 25.0 ms at 1024 utterances); a tile's live bits are one wave ballot
constexpr int kRawTile = 64;
constexpr int kRawChunk = 2 * kRawTile;  // intervals staged per train and tile, at most
// overlap-save band filters (wh_bands.h): transform length, and outputs kept per block — 256 x 14 positions (+2 look-ahead
// samples); the longest filter (493 taps) leaves 4096 - 495 = 3601
constexpr int kOlsN = 4096;
constexpr int kOlsValid = 3584;

struct HvUtt {
  int64_t x_off, n;
  int64_t nd, offset;     // constant-padded length, pad amount
  int64_t t_off;          // pass-1 output (nd + 18)
  int64_t y_off, ylen;    // decimated + trimmed signal
  int64_t z_off;          // zero-padded, mean-removed copy: ylen + 2*pad
  int64_t pick0;          // index into the filtfilt output of y[0]
  int64_t f1_off, nf1;    // 1 ms frames
  int64_t l_off, ntile;   // live-candidate bit map: word l_off + channel * ntile + tile holds the tile's 64 frames
  int64_t f_off, nf;      // output frames
};

struct Tdf2 {
  double b0, b1, b2, b3, a1, a2, a3, zi0, zi1, zi2;
};

struct BandJob;  // wh_bands.h

// ---- host side ------------------------------------------------------------------------------------------------------
// One wh_harvest call: geometry of every utterance, totals and maxima over the batch, and the three run-time forms.
// Filled on the host from the batch, the rates and the band table; touches no device.
struct HvPlan {
  int B = 0, r = 1, n_bands = 0;
  bool filtered = false;  // the anti-aliasing filter runs (fs > 8000 Hz, also where the ratio rounds to 1)
  double fs_d = 0.0;      // decimated rate
  int max_lb = 0, taps_total = 0, h_max = 0;  // longest filter, all taps, largest half length
  int pad = 0;                                // zeros either side of z
  int hmax = 0;                               // half length of the longest refinement window (+ 1)
  std::vector<int32_t> ti;                    // [3][n_bands]: tap offset, tap count, half length (bias) of every channel
  std::vector<HvUtt> meta;
  std::vector<int64_t> e_off, e_cap;          // [B][n_bands]: the crossing lists of a channel, [4][cap] doubles at e_off
  std::vector<int64_t> tile_off;              // [B + 1]: overlap-save tiles in front of an utterance
  int64_t t_tot = 0, y_tot = 0, z_tot = 0, e_tot = 0, f1_tot = 0, l_tot = 0;
  int64_t max_len = 0, max_ylen = 0, max_nf1 = 0, max_nf = 0, max_ntile = 0, max_tiles = 0, batch_tiles = 0;
  bool use_ols = false;     // overlap-save band filters; false: the direct FIR (taps that exceed a tile)
  bool use_rawdet = false;  // hv_rawdet_kernel; false: hv_raw_kernel + hv_detect_kernel (below the tile threshold)
  bool need_map = false;    // the [channel][frame] candidate map and its bit map exist (the pair, or the debug read-out)
};

// Device pointers of one call: the workspace regions (wh_harvest.hip: carve_harvest) and the persistent uploads.
struct HvDev {
  HvUtt* meta = nullptr;
  BandJob* jobs = nullptr;
  double *taps = nullptr, *band_f0 = nullptr;
  int32_t* tapinfo = nullptr;  // ti of the plan
  int32_t* cnt = nullptr;      // [B][n_bands][4] crossing counts (a buffer of its own: wh_harvest_event_counts)
  double *tmp, *y, *z, *mean, *e, *raw;
  unsigned long long* live;
  int32_t* hint;  // [utterance][tile][channel][train]
  double* dc;
  int32_t* dn;
  double *rf0, *rsc;
  uint32_t* keep;
  int64_t* lst;
  char* ct;  // the contour back end's share
  double2* tspec;
  double2* zspec;
  double* tre;
};

// wh_hv_front.hip
int hv_upload(wh_ctx* ctx, hipStream_t st, const HvPlan& p, const double* h_band_taps, const double* h_band_f0, HvDev& d);
int hv_launch_decimate(wh_ctx* ctx, hipStream_t st, const HvPlan& p, const double* x, const double* h_ba,
                       const double* h_zi, const HvDev& d);
int hv_launch_band_events(wh_ctx* ctx, hipStream_t st, const HvPlan& p, const HvDev& d);
int hv_launch_raw_detect(wh_ctx* ctx, hipStream_t st, const HvPlan& p, double f0_floor, double f0_ceil, const HvDev& d,
                         double* dbg_raw);
// wh_hv_refine.hip
int hv_launch_refine(wh_ctx* ctx, hipStream_t st, const HvPlan& p, double f0_floor, double f0_ceil, const HvDev& d);
int hv_launch_prune(wh_ctx* ctx, hipStream_t st, const HvPlan& p, const HvDev& d);
// wh_hv_contour.hip
// the contour back end's share of the Harvest workspace, taken from `c`: exactly what hv_launch_contour carves from it
Region<char> hv_carve_contour(Carve& c, const HvPlan& p);
int hv_launch_contour(wh_ctx* ctx, hipStream_t st, const HvPlan& p, const HvDev& d, const double* tp, double* f0_out,
                      double* vuv_out, double* dbg_f0_1ms);
// test hooks (wh_hv_probe.hip): the smoothing and the pick alone on caller-supplied rows; the rows and the section table
// the back end left in its share (rows_out: DEVICE; h_nsec [B], h_secs [B][sec_cap][5] = (st, ed, r0, r1, kept): HOST)
int hv_launch_smooth_pick(wh_ctx* ctx, hipStream_t st, const HvPlan& p, const HvDev& d, const double* rows_in,
                          const double* tp, double* f0_out, double* vuv_out);
int hv_read_contour(hipStream_t st, const HvPlan& p, const HvDev& d, double* rows_out, int32_t* h_nsec, int32_t* h_secs,
                    int64_t sec_cap);

}  // namespace wh
