// Harvest front end (see wh_harvest.hip for the stage list): decimation, mean removal and padding; the 152 band-pass
// channels with their zero crossings (wh_bands.h); raw candidates and detection.  Built unfused like every F0 stage.
#include <math.h>
#include <hip/hip_runtime.h>

// The overlap-save walker loops over channel-tiles around an inlined inverse transform and needs the opaque thread index
// (wh_tid.h); the other kernels of this unit are compiled with it too.
#include "wh_tid.h"
#include "wh_bands.h"
#include "wh_device.h"
#include "wh_reduce.h"
#include "wh_host.h"
#include "wh_hv_types.h"
#include "wh_math.h"

namespace {
using namespace wh;

__device__ __forceinline__ double hv_xp(const double* __restrict__ x, const HvUtt& m, int64_t i) {
  int64_t k = i - m.offset;  // constant edge padding (harvest.py:66)
  k = k < 0 ? 0 : (k > m.n - 1 ? m.n - 1 : k);
  return x[k];
}
// odd extension by 9 samples of the constant-padded signal (scipy.signal.filtfilt, padtype='odd')
__device__ __forceinline__ double hv_ext(const double* __restrict__ x, const HvUtt& m, int64_t e) {
  if (e < kFPad) return 2 * hv_xp(x, m, 0) - hv_xp(x, m, kFPad - e);
  if (e < kFPad + m.nd) return hv_xp(x, m, e - kFPad);
  return 2 * hv_xp(x, m, m.nd - 1) - hv_xp(x, m, m.nd - 2 - (e - (kFPad + m.nd)));
}

#define TDF2_STEP(IN)                     \
  {                                       \
    const double xin = (IN);              \
    yv = z0 + c.b0 * xin;                 \
    z0 = z1 + xin * c.b1 - yv * c.a1;     \
    z1 = z2 + xin * c.b2 - yv * c.a2;     \
    z2 = xin * c.b3 - yv * c.a3;          \
  }

constexpr int kHBlock = 16;  // samples fetched together, a block ahead of the recurrence (wh::serial_run)

__global__ __launch_bounds__(64) void hv_iir_fwd_kernel(const double* __restrict__ x, const HvUtt* __restrict__ meta,
                                                        Tdf2 c, int warm, double* __restrict__ tmp) {
  const HvUtt m = meta[blockIdx.y];
  const int64_t len = m.nd + 2 * kFPad;
  const int64_t s = ((int64_t)blockIdx.x * 64 + threadIdx.x) * kHChunk;
  if (s >= len) return;
  const int64_t e = s + kHChunk < len ? s + kHChunk : len;
  const double* xu = x + m.x_off;
  double* out = tmp + m.t_off;
  double z0 = 0, z1 = 0, z2 = 0, yv = 0;
  int64_t i0 = s - warm;
  if (i0 <= 0) {  // the true start: steady-state initial conditions scaled by the first sample
    i0 = 0;
    const double x0 = hv_ext(xu, m, 0);
    z0 = c.zi0 * x0;
    z1 = c.zi1 * x0;
    z2 = c.zi2 * x0;
  }
  const int64_t lo = kFPad + m.offset, hi = kFPad + m.offset + m.n;  // extended indices that are plain samples of x
  wh::serial_run<kHBlock>(
      i0, e, [&](int64_t i) { return i >= lo && i + kHBlock <= hi; }, [&](int64_t i) { return xu[i - lo]; },
      [&](int64_t i) { return hv_ext(xu, m, i); },
      [&](int64_t i, double v) {
        TDF2_STEP(v);
        if (i >= s) out[i] = yv;
      });
}
// Second pass over the reversed pass-1 output; stores only the decimated picks p = pick0 + k*r of the filtfilt result
// (quotient and remainder of p - pick0 by r are carried along the walk instead of divided out per sample).
__global__ __launch_bounds__(64) void hv_iir_bwd_kernel(const HvUtt* __restrict__ meta, Tdf2 c, int warm, int r,
                                                        const double* __restrict__ tmp, double* __restrict__ y) {
  const HvUtt m = meta[blockIdx.y];
  const int64_t len = m.nd + 2 * kFPad;
  const int64_t s = ((int64_t)blockIdx.x * 64 + threadIdx.x) * kHChunk;
  if (s >= len) return;
  const int64_t e = s + kHChunk < len ? s + kHChunk : len;
  const double* in = tmp + m.t_off;
  double* yo = y + m.y_off;
  const int64_t ylen = m.ylen;
  double z0 = 0, z1 = 0, z2 = 0, yv = 0;
  int64_t i0 = s - warm;
  if (i0 <= 0) {
    i0 = 0;
    const double y0 = in[len - 1];
    z0 = c.zi0 * y0;
    z1 = c.zi1 * y0;
    z2 = c.zi2 * y0;
  }
  const int64_t d0 = (len - 1 - s) - kFPad - m.pick0;  // p - pick0 at i = s; falls by one per step
  int64_t k0 = d0 >= 0 ? d0 / r : -((-d0 + r - 1) / r);
  int r0 = (int)(d0 - k0 * r);
  wh::serial_run<kHBlock>(
      i0, e, [&](int64_t) { return true; }, [&](int64_t i) { return in[len - 1 - i]; },
      [&](int64_t i) { return in[len - 1 - i]; },
      [&](int64_t i, double v) {
        TDF2_STEP(v);
        if (i >= s) {
          if (r0 == 0 && k0 >= 0 && k0 < ylen) yo[k0] = yv;
          if (--r0 < 0) {
            r0 = r - 1;
            --k0;
          }
        }
      });
}

__global__ __launch_bounds__(256) void hv_copy_kernel(const double* __restrict__ x, const HvUtt* __restrict__ meta,
                                                      double* __restrict__ y) {
  const HvUtt m = meta[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < m.ylen) y[m.y_off + i] = x[m.x_off + i];
}

// mean of the decimated signal in two steps: kMeanParts partial sums per utterance (fixed association: the result does
// not depend on the launch), then their sum / length
__global__ __launch_bounds__(256) void hv_mean_part_kernel(const HvUtt* __restrict__ meta, const double* __restrict__ y,
                                                           double* __restrict__ part) {
  __shared__ double scratch[16];
  const HvUtt m = meta[blockIdx.y];
  const int64_t chunk = (m.ylen + kMeanParts - 1) / kMeanParts;
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < m.ylen ? begin + chunk : m.ylen;
  double s = 0.0;
  for (int64_t i = begin + threadIdx.x; i < end; i += 256) s += y[m.y_off + i];
  s = wh::block_sum(s, scratch);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * kMeanParts + blockIdx.x] = s;
}
__global__ __launch_bounds__(64) void hv_mean_kernel(const HvUtt* __restrict__ meta, const double* __restrict__ part,
                                                     int n_utt, double* __restrict__ mean) {
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= n_utt) return;
  double s = 0.0;
  for (int k = 0; k < kMeanParts; ++k) s += part[(int64_t)u * kMeanParts + k];
  mean[u] = s / (double)meta[u].ylen;
}

// z = [zeros(pad), y - mean, zeros(pad)]; also rewrites y itself mean-removed (the refinement reads it)
__global__ __launch_bounds__(256) void hv_pad_kernel(const HvUtt* __restrict__ meta, double* __restrict__ y,
                                                     const double* __restrict__ mean, int pad, double* __restrict__ z) {
  const HvUtt m = meta[blockIdx.y];
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m.ylen + 2 * pad) return;
  const int64_t i = j - pad;
  double v = 0.0;
  if (i >= 0 && i < m.ylen) {
    v = y[m.y_off + i] - mean[blockIdx.y];
    y[m.y_off + i] = v;
  }
  z[m.z_off + j] = v;
}

// One workgroup per (utterance, channel) walks the 1 ms frames in tiles of 256.  The four event trains are sorted
// and the frames ascending, so the events a tile can need are a window that only moves forward: the workgroup keeps
// a cursor per train and, per tile, turns the edges behind it into INTERVALS in LDS — location (e[i]+e[i+1])/2/fs and
// instantaneous frequency fs/(e[i+1]-e[i]), one thread per interval, coalesced loads — and every frame searches the
// locations of that window and interpolates between two staged intervals: one LDS read per search step and one divide
// per (frame, train), where the per-frame form re-derived both neighbouring intervals from four edges (two reads, an
// add and a multiply per step, three divides).  A band of centre f has ~1.1 f events per second at most, so the
// window staged for 256 ms is sized by the band (kRawChunk caps it).  A frame whose answer is not inside the staged
// window falls back to the search over the whole list in global memory (guarded, never taken for speech bands).
// Same arithmetic as wh::interp_four_trains, value for value.
__global__ __launch_bounds__(kRawTile) void hv_raw_kernel(const HvUtt* __restrict__ meta, const wh::BandJob* __restrict__ jobs,
                                                     const double* __restrict__ band_f0, int nb, double fs_d,
                                                     double f0_floor, double f0_ceil, double* __restrict__ raw,
                                                     unsigned long long* __restrict__ live, int dense) {
  static_assert(kRawTile == 64, "a tile's live bits are one wave ballot");
  __shared__ double2 iv[4][kRawChunk];  // (location, frequency) of interval start + i
  __shared__ int s_next[4];
  const HvUtt m = meta[blockIdx.y];
  const int b = blockIdx.x;
  const wh::BandJob job = jobs[(int64_t)blockIdx.y * nb + b];
  double* out = raw + m.f1_off * nb + (int64_t)b * m.nf1;
  // What hv_detect scans: ONE BIT per (channel, frame) — set where a candidate survived the range tests — as a 64-bit
  // word per (channel, 64-frame tile), the wave's ballot.  The candidate VALUES are written only where that bit is set
  // (round 6; `dense`: everywhere, for the debug read-out): hv_detect reads a value only inside a run of live channels,
  // and most of the [channel][frame] map is dead — it used to leave as 12.2 MB of doubles + 1.5 MB of bytes per 10 s
  // utterance, nearly all of it zeros nobody read.
  unsigned long long* lv = live + m.l_off + (int64_t)b * m.ntile;
  int cnt[4];
  bool usable = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    cnt[k] = job.counts[k];
    usable = usable && (cnt[k] - 1 >= 3);
  }
  if (!usable) {  // fewer than 3 intervals in a train: no candidate anywhere (dio.py:159-162)
    for (int64_t t = threadIdx.x; t < m.ntile; t += kRawTile) lv[t] = 0ull;
    if (dense)
      for (int64_t f = threadIdx.x; f < m.nf1; f += kRawTile) out[f] = 0.0;
    return;
  }
  const double bf = band_f0[b];
  const double half_inv_fs = 0.5 / fs_d;
  // intervals staged per tile: twice the ~1.1*bf*0.256 a band-limited signal can hold, plus the cursor's slack
  int need = 2 * (int)(bf * 1.1 * (kRawTile * 0.001) + 1.0) + 8;
  need = need > kRawChunk - 1 ? kRawChunk - 1 : need;  // (the last slot always holds the +inf sentinel of the search)
  int search_steps = 0;  // doubling steps that settle a lower_bound over [0, need]: 2^steps > need
  while ((1 << search_steps) < need + 1) ++search_steps;
  // blockIdx.z cuts the frames into gridDim.z segments of whole tiles, each with its own workgroup (the tile loop is a
  // chain of load -> barrier -> search -> barrier; more workgroups in flight hide it).  A segment's first cursors
  // are found by a search over the whole list.
  const int64_t tiles_all = (m.nf1 + kRawTile - 1) / kRawTile;
  const int64_t tiles_seg = (tiles_all + gridDim.z - 1) / gridDim.z;
  const int64_t f_begin = (int64_t)blockIdx.z * tiles_seg * kRawTile;
  const int64_t f_end = f_begin + tiles_seg * kRawTile < m.nf1 ? f_begin + tiles_seg * kRawTile : m.nf1;
  if (f_begin >= m.nf1) return;
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    const double* e = job.edges + (int64_t)k * job.cap;
    const double t = (double)f_begin * 1 / 1000;
    int lo = 0, hi = job.counts[k] - 1;
    if (f_begin == 0) hi = 0;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const double loc = (e[mid] + e[mid + 1]) * half_inv_fs;
      if (loc < t) lo = mid + 1; else hi = mid;
    }
    s_next[k] = lo;
  }
  __syncthreads();
  int pos[4];  // per train: number of interval locations before the current tile's first frame
#pragma unroll
  for (int k = 0; k < 4; ++k) pos[k] = s_next[k];
  __syncthreads();
  for (int64_t f0 = f_begin; f0 < f_end; f0 += kRawTile) {
    int start[4], nloc[4];
    double ea[4][2], eb[4][2];  // all of a tile's edge loads are issued before the first divide consumes one
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      start[k] = pos[k] - 2 > 0 ? pos[k] - 2 : 0;
      const int ni = cnt[k] - 1;
      nloc[k] = ni - start[k] < need ? ni - start[k] : need;  // intervals staged
      const double* e = job.edges + (int64_t)k * job.cap + start[k];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int i = threadIdx.x + r * kRawTile;
        ea[k][r] = i < nloc[k] ? e[i] : 0.0;
        eb[k][r] = i < nloc[k] ? e[i + 1] : 1.0;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int i = threadIdx.x + r * kRawTile;
        // (slots past the staged intervals hold +inf locations: the search below needs no bounds; written as a select —
        // as a branch that skips the second round's divide for the bands below ~400 Hz: 1.36 against 1.30 ms)
        iv[k][i] = i < nloc[k] ? make_double2((ea[k][r] + eb[k][r]) * half_inv_fs, wh::fdiv(fs_d, eb[k][r] - ea[k][r]))
                               : make_double2(INFINITY, 0.0);
      }
    __syncthreads();
    const int64_t f = f0 + threadIdx.x;
    int lo_g[4] = {0, 0, 0, 0};
    double cand = 0.0;
    if (f < f_end) {
      const double t = (double)f * 1 / 1000;  // basic_temporal_positions (harvest.py:21)
      double v[4];
      // lower_bound of t among the staged locations, the four trains in lockstep, as the branch-free DOUBLING search: the
      // position grows by a power of two whenever the element in front of the probe is still below t — add, read,
      // compare, select per step and train (the halving form carried a [lo, hi) pair and an activity flag: three times the
      // integer work of a kernel whose VALU is saturated and 22 % FP64).  The +inf sentinels behind the staged intervals
      // stand in for the bounds checks.
      int lo4[4] = {0, 0, 0, 0};
      for (int st = 1 << (search_steps - 1); st > 0; st >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int q = lo4[k] + st;
          lo4[k] = iv[k][q - 1].x < t ? q : lo4[k];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int ni = cnt[k] - 1;  // intervals of the whole train; location i = (e[i]+e[i+1])/2/fs
        const int lo = lo4[k];
        const bool inside = lo < nloc[k] || start[k] + nloc[k] == ni;
        const double* e = job.edges + (int64_t)k * job.cap;
        int g = start[k] + lo;  // count of locations < t over the whole train
        if (!inside) {          // the window ended before t: global search
          int l2 = g, h2 = ni;
          while (l2 < h2) {
            const int mid = (l2 + h2) >> 1;
            const double loc = (e[mid] + e[mid + 1]) * half_inv_fs;
            if (loc < t) l2 = mid + 1; else h2 = mid;
          }
          g = l2;
        }
        lo_g[k] = g;
        const int ih = g < 1 ? 1 : (g > ni - 1 ? ni - 1 : g);
        const int il = ih - 1;
        double x_lo, x_hi, y_lo, y_hi;
        if (il >= start[k] && ih < start[k] + nloc[k]) {
          const double2 a = iv[k][il - start[k]], c = iv[k][ih - start[k]];
          x_lo = a.x;
          y_lo = a.y;
          x_hi = c.x;
          y_hi = c.y;
        } else {
          const double e0 = e[il], e1 = e[il + 1], e2 = e[ih], e3 = e[ih + 1];
          x_lo = (e0 + e1) * half_inv_fs;
          x_hi = (e2 + e3) * half_inv_fs;
          y_lo = wh::fdiv(fs_d, e1 - e0);
          y_hi = wh::fdiv(fs_d, e3 - e2);
        }
        const double slope = wh::fdiv(y_hi - y_lo, x_hi - x_lo);
        v[k] = slope * (t - x_lo) + y_lo;
      }
      cand = (((v[0] + v[1]) + v[2]) + v[3]) / 4;
      if (cand > bf * 1.1 || cand < bf * 0.9 || cand > f0_ceil || cand < f0_floor) cand = 0.0;  // harvest.py:273-276
      if (dense || cand > 0) out[f] = cand;
    }
    {
      const unsigned long long bits = __ballot(cand > 0);  // (lanes behind the utterance's end: 0)
      if (threadIdx.x == 0) lv[f0 / kRawTile] = bits;
    }
    // the last frame of the tile hands its counts to the next tile as the new cursors
    const int64_t last = f0 + kRawTile - 1 < f_end - 1 ? f0 + kRawTile - 1 : f_end - 1;
    if (f == last) {
#pragma unroll
      for (int k = 0; k < 4; ++k) s_next[k] = lo_g[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) pos[k] = s_next[k];
  }
}

// ---- raw candidates AND detection in one pass (round 6) ---------------------------------------------------------------
// hv_raw_kernel walks the frames of ONE channel and leaves a [channel][frame] map for hv_detect_kernel, which walks the
// channels of one frame: 6 MB of candidate values written and 4.4 MB read back per 10 s utterance, plus the launch.  This
// kernel is the transpose: one wave per (utterance, tile of 64 frames) walks ALL channels in order, a lane per frame —
// the interpolation of hv_raw_kernel, value for value (same staging of (location, frequency) intervals in LDS, same
// doubling search, same window check with the search over the whole list as the way out) — and what DetectCandidates
// (harvest.py:88-110) needs of a frame's column is kept in the lane as it goes by: the length of the current run of live
// channels and the sum of its values, added channel after channel.  (np.mean adds them pairwise; hv_detect_kernel
// reproduces that association, this kernel does not: the values themselves agree with the reference's to ~1e-9 Hz —
// overlap-save filters against FFT products — so the 1e-16 of a summation order is not what parity rests on, and the
// eight accumulators + pending group of the pairwise form cost a wave per SIMD: 7.06 against 5.4 ms at 256 utterances.)
// A run of >= 10 channels that ends becomes a candidate.  Nothing but the 15 candidate slots per frame leaves the kernel.
//   Where a tile's search of a channel's four edge lists starts is the band walker's advice (emit_crossings_block's
// hints: crossings in front of the tile's first sample); the edges of the NEXT channel are fetched while the current
// one is searched.  Workgroup order: an utterance's tiles on one XCD, consecutive (neighbouring tiles read overlapping
// stretches of every list — from that XCD's L2 the second time).
struct RdMeta {  // what the edge loads of a channel are addressed by: fetched a channel ahead of them
  int4 h0, h1, c;  // the tile's hints, the next tile's, the trains' edge counts
  const double* e;
  int64_t cap;
  double bf;
};
struct RdStage {
  int start[4], nloc[4], ni[4];
  double ea[4][2];  // edge start + lane + 64 r of every train (the interval's other edge is the next lane's)
  const double* e;
  int64_t cap;
  double bf;
  int need, steps;
  bool usable;
};

constexpr int kRawdetMinWaves = 3;  // (12 KB of LDS per wave: 13 waves per CU whatever the registers)
__global__ __launch_bounds__(kRawTile, kRawdetMinWaves) void hv_rawdet_kernel(const HvUtt* __restrict__ meta, const wh::BandJob* __restrict__ jobs,
                                                             const double* __restrict__ band_f0,
                                                             const int32_t* __restrict__ hints, int nb, int n_utt, int n_xcd, int max_ntile,
                                                             double fs_d, double f0_floor, double f0_ceil,
                                                             double* __restrict__ dc, int32_t* __restrict__ dcount,
                                                             double* __restrict__ raw_dbg) {
  __shared__ double2 iv[4][kRawChunk];       // (location, frequency) of interval start + i
  const int xcd = blockIdx.x % n_xcd, local = blockIdx.x / n_xcd;  // (n_xcd: 8, or 1 for fewer than eight utterances)
  const int u = (local / max_ntile) * n_xcd + xcd;
  if (u >= n_utt) return;
  const HvUtt m = meta[u];
  const int64_t T = local % max_ntile;
  if (T >= m.ntile) return;
  const int lane = threadIdx.x;
  const int64_t f = T * kRawTile + lane;
  const bool live_f = f < m.nf1;
  const double t = (double)f * 1 / 1000;  // basic_temporal_positions (harvest.py:21)
  const double half_inv_fs = 0.5 / fs_d;
  const int32_t* hT = hints + (m.l_off + T * nb) * 4;          // [channel][train] of this tile
  const int32_t* cU = jobs[(int64_t)u * nb].counts;            // [channel][train] of this utterance (contiguous)

  // Two fetch stages run ahead of the channel being searched: the addressing data of channel b + 2 (hints, counts, list
  // base: uniform loads), then — from the data fetched one channel earlier — the edges of channel b + 1.  (With both in
  // one stage every channel waited a memory round trip for its hints before its edge loads could be issued.)
  auto fetch_meta = [&](int b, RdMeta& q) {
    b = b < nb ? b : nb - 1;  // (a surplus prefetch behind the last channel: harmless)
    typedef int v4i __attribute__((ext_vector_type(4)));
    typedef const v4i __attribute__((address_space(1))) * g4;
    const v4i a = *(g4)(hT + b * 4), c = *(g4)(cU + b * 4);
    const v4i n = T + 1 < m.ntile ? *(g4)(hT + (nb + b) * 4) : c;  // (behind the last tile: every edge)
    q.h0 = make_int4(a.x, a.y, a.z, a.w);
    q.h1 = make_int4(n.x, n.y, n.z, n.w);
    q.c = make_int4(c.x, c.y, c.z, c.w);
    const wh::BandJob* j = jobs + (int64_t)u * nb + b;
    q.e = j->edges;
    q.cap = j->cap;
    q.bf = band_f0[b];
  };
  auto fetch = [&](const RdMeta& q, RdStage& s) {
    s.e = q.e;
    s.cap = q.cap;
    s.bf = q.bf;
    const int cs[4] = {q.c.x, q.c.y, q.c.z, q.c.w}, h0s[4] = {q.h0.x, q.h0.y, q.h0.z, q.h0.w}, h1s[4] = {q.h1.x, q.h1.y, q.h1.z, q.h1.w};
    bool usable = true;
    int need = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = __builtin_amdgcn_readfirstlane(cs[k]);  // (uniform: kept in scalar registers)
      const int ni = c - 1;  // intervals of the whole train
      usable = usable && (ni >= 3);
      s.ni[k] = ni;
      // the hint counts EDGES in front of the tile's first sample; the locations in front of its first frame are that
      // many, give or take two: start four entries early (hv_raw_kernel starts two in front of the exact count) — and the
      // NEXT tile's hint says where this tile's edges end: the window is what the tile needs plus that slack, not a
      // worst-case budget (staged from a budget of twice the band's rate the tiles of an utterance read every list 2.2 times)
      const int h0 = __builtin_amdgcn_readfirstlane(h0s[k]);
      const int h1 = __builtin_amdgcn_readfirstlane(h1s[k]);
      int st = h0 - 4;
      st = st > ni - 1 ? ni - 1 : st;
      st = st < 0 ? 0 : st;
      s.start[k] = st;
      int n = h1 - st + 3;
      n = n > kRawChunk - 1 ? kRawChunk - 1 : n;  // (the last slot always holds the +inf sentinel of the search)
      n = n > ni - st ? ni - st : n;
      n = n < 1 ? 1 : n;
      s.nloc[k] = n;
      need = n > need ? n : need;
    }
    int steps = 0;
    while ((1 << steps) < need + 1) ++steps;
    s.need = need;
    s.steps = steps;
    s.usable = usable;
    if (!usable) return;  // fewer than 3 intervals in a train: no candidate anywhere in this channel (dio.py:159-162)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double* e = s.e + (int64_t)k * s.cap + s.start[k];
      {
        const int ic = lane <= s.nloc[k] ? lane : 0;  // entries 0 .. nloc (start + nloc <= ni: a valid edge); clamped, not skipped: no branch per load
        s.ea[k][0] = wh::ldg(e + ic);
      }
      if (s.need >= kRawTile) {  // (uniform; rare: more than 60 crossings of one kind in 64 ms)
        const int i = lane + kRawTile;
        const int ic = i <= s.nloc[k] ? i : 0;
        s.ea[k][1] = wh::ldg(e + ic);
      }
    }
  };

  // the lane's walk state: DetectCandidates of its frame
  double run_sum = 0.0;
  int idx = 0, count = 0;
  double* out = dc + (m.f1_off + f) * kMaxC;

  auto consume = [&](int b, const RdStage& s) {
    double cand = 0.0;
    if (s.usable) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // the interval's upper edge: the next lane's entry (lane 63 of the first round: lane 0 of the second)
        const double up0 = __shfl_down(s.ea[k][0], 1);
        if (s.need < kRawTile) {  // (uniform) one round: entries 0 .. 63, intervals 0 .. 62 at most
          iv[k][lane] = lane < s.nloc[k] ? make_double2((s.ea[k][0] + up0) * half_inv_fs, wh::fdiv(fs_d, up0 - s.ea[k][0]))
                                         : make_double2(INFINITY, 0.0);
        } else {
          const double up1 = __shfl_down(s.ea[k][1], 1);
          const double wrap = __shfl(s.ea[k][1], 0);
          const double eb[2] = {lane == kRawTile - 1 ? wrap : up0, up1};  // (entry 127 is never an interval: nloc <= 127)
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const int i = lane + r * kRawTile;
            iv[k][i] = i < s.nloc[k] ? make_double2((s.ea[k][r] + eb[r]) * half_inv_fs, wh::fdiv(fs_d, eb[r] - s.ea[k][r]))
                                     : make_double2(INFINITY, 0.0);
          }
        }
      }
      wh::sync<kRawTile>();
      if (live_f) {
        double v[4];
        int lo4[4] = {0, 0, 0, 0};
        for (int st = 1 << (s.steps - 1); st > 0; st >>= 1) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int q = lo4[k] + st;
            lo4[k] = iv[k][q - 1].x < t ? q : lo4[k];
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int ni = s.ni[k];
          const int lo = lo4[k];
          const double* e = s.e + (int64_t)k * s.cap;
          // the staged window holds the answer if a location >= t lies inside it (or the list ends in it) AND the count
          // did not stop at the window's first entry while locations lie in front of the window (the hint was late)
          const bool inside = (lo < s.nloc[k] || s.start[k] + s.nloc[k] == ni) && (lo > 0 || s.start[k] == 0);
          int g = s.start[k] + lo;  // count of locations < t over the whole train
          if (!inside) {            // search over the whole list
            int l2 = 0, h2 = ni;
            while (l2 < h2) {
              const int mid = (l2 + h2) >> 1;
              const double loc = (e[mid] + e[mid + 1]) * half_inv_fs;
              if (loc < t) l2 = mid + 1; else h2 = mid;
            }
            g = l2;
          }
          const int ih = g < 1 ? 1 : (g > ni - 1 ? ni - 1 : g);
          const int il = ih - 1;
          double x_lo, x_hi, y_lo, y_hi;
          if (il >= s.start[k] && ih < s.start[k] + s.nloc[k]) {
            const double2 a = iv[k][il - s.start[k]], c = iv[k][ih - s.start[k]];
            x_lo = a.x;
            y_lo = a.y;
            x_hi = c.x;
            y_hi = c.y;
          } else {
            const double e0 = e[il], e1 = e[il + 1], e2 = e[ih], e3 = e[ih + 1];
            x_lo = (e0 + e1) * half_inv_fs;
            x_hi = (e2 + e3) * half_inv_fs;
            y_lo = wh::fdiv(fs_d, e1 - e0);
            y_hi = wh::fdiv(fs_d, e3 - e2);
          }
          const double slope = wh::fdiv(y_hi - y_lo, x_hi - x_lo);
          v[k] = slope * (t - x_lo) + y_lo;
        }
        cand = (((v[0] + v[1]) + v[2]) + v[3]) / 4;
        if (cand > s.bf * 1.1 || cand < s.bf * 0.9 || cand > f0_ceil || cand < f0_floor) cand = 0.0;  // harvest.py:273-276
      }
      wh::sync<kRawTile>();  // (the next channel's intervals overwrite iv)
    }
    if (raw_dbg && live_f) raw_dbg[m.f1_off * nb + (int64_t)b * m.nf1 + f] = cand;
    // DetectCandidates (harvest.py:88-110): first and last channel count as dead; a run of >= 10 live channels that ends
    // gives the mean of its values
    const bool live = live_f && b >= 1 && b < nb - 1 && cand > 0;
    if (live) {
      run_sum += cand;
      ++idx;
    } else if (idx > 0) {
      if (idx >= 10 && count < kMaxC) out[count++] = run_sum / (double)idx;
      idx = 0;
      run_sum = 0.0;
    }
  };

  RdMeta qa, qb;
  RdStage sa, sb;
  fetch_meta(0, qa);
  fetch_meta(1, qb);
  fetch(qa, sa);
  for (int b = 0; b < nb; b += 2) {
    fetch(qb, sb);          // the edges of channel b + 1
    fetch_meta(b + 2, qa);
    consume(b, sa);
    fetch(qa, sa);          // ... of b + 2
    fetch_meta(b + 3, qb);
    if (b + 1 < nb) consume(b + 1, sb);
  }
  if (live_f) {
    for (int c = count; c < kMaxC; ++c) out[c] = 0.0;  // (hv_refine reads every slot)
    dcount[m.f1_off + f] = count;
  }
}

// NumPy's pairwise summation for n <= 128 (what np.mean does on the run of channel values)
__device__ __forceinline__ double np_sum_strided(const double* __restrict__ a, int64_t stride, int n) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += a[i * stride];
    return r;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = a[j * stride];
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += a[(i + j) * stride];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i * stride];
  return res;
}

// The channel walk reads hv_raw's byte map (1 = a candidate survived the band's range test) instead of the candidates
// themselves — an eighth of the bytes of a pass that runs at HBM speed — and fetches the values only for the runs that
// count.
__global__ __launch_bounds__(256) void hv_detect_kernel(const HvUtt* __restrict__ meta, int nb,
                                                        const double* __restrict__ raw,
                                                        const unsigned long long* __restrict__ live_map, double* __restrict__ dc,
                                                        int32_t* __restrict__ dcount) {
  const HvUtt m = meta[blockIdx.y];
  // the grid is sized by the longest utterance of the batch: blocks wholly behind this utterance's end leave at once
  // (also the nf1 == 0 case, where the clamp below would point in front of the column)
  if ((int64_t)blockIdx.x * 256 >= m.nf1) return;
  const int64_t f_raw = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live_f = f_raw < m.nf1;  // (the tail threads of the last block stay for its output pass)
  const int64_t f = live_f ? f_raw : m.nf1 - 1;
  const double* col = raw + m.f1_off * nb + f;  // element b at col[b * nf1]
  // the wave's 64 frames are one tile of hv_raw's bit map: ONE word per channel for the whole wave (a uniform address)
  const int64_t tile_w = ((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63)) / 64;
  const unsigned long long* lcol = live_map + m.l_off + (tile_w < m.ntile ? tile_w : m.ntile - 1);
  const int lane_w = threadIdx.x & 63;
  // Phase 1: the runs.  Phase 2 sums them run by run: every lane of the wave is then inside the same summation loop at
  // the same time (its loads in flight together), where summing a run the moment the walk finds its end made the wave
  // go through one summation — two or three dependent rounds of global loads — per distinct end position among its
  // 64 lanes.
  __shared__ unsigned short runs[kMaxC][256];  // (first live channel) << 8 | length
  int count = 0;
  int run_start = -1;  // 'st': index of the last dead channel before a live run
  bool prev = false;   // channel 0 is forced dead
  // the channel walk is a chain of dependent branches; its loads are not: eight channels are fetched together
  for (int b0 = 0; live_f && b0 < nb; b0 += 8) {
    unsigned v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = (unsigned)(lcol[(int64_t)(b0 + q < nb ? b0 + q : nb - 1) * m.ntile] >> lane_w) & 1u;  // clamped, not skipped: a
    // conditional load becomes a branch, and eight of them a chain of load-wait-load (the surplus values are not read)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int b = b0 + q;
      if (b < 1 || b >= nb) continue;
      const bool live = (b < nb - 1) && (v[q] > 0);  // last channel forced dead
      if (live && !prev) run_start = b - 1;
      if (!live && prev) {
        const int ed = b - 1;
        if (ed - run_start >= 10 && count < kMaxC) runs[count++][threadIdx.x] = (unsigned short)(((run_start + 1) << 8) | (ed - run_start));
      }
      prev = live;
    }
  }
  // The kMaxC slots of a frame are 120 bytes apart: written from the walk's lanes, every store instruction touched 64
  // cache lines.  They are collected in LDS (dense rows: an odd stride in doubles, conflict-free both ways) and leave as one
  // contiguous block per workgroup.
  __shared__ double s_out[256 * kMaxC];
  for (int c = 0; c < kMaxC; ++c) {
    double val = 0.0;
    if (live_f && c < count) {
      const int rr = runs[c][threadIdx.x];
      const int n = rr & 0xff;
      val = np_sum_strided(col + (int64_t)(rr >> 8) * m.nf1, m.nf1, n) / (double)n;
    }
    s_out[threadIdx.x * kMaxC + c] = val;
  }
  if (live_f) dcount[m.f1_off + f] = count;
  __syncthreads();
  const int64_t f_blk = (int64_t)blockIdx.x * 256;
  const int n_blk = (int)(m.nf1 - f_blk < 256 ? m.nf1 - f_blk : 256);
  double* ob = dc + (m.f1_off + f_blk) * kMaxC;
  for (int q = threadIdx.x; q < n_blk * kMaxC; q += 256) ob[q] = s_out[q];
}

double tdf2_pole_radius(double a1, double a2, double a3) {
  // max |root| of z^3 + a1 z^2 + a2 z + a3 (Durand-Kerner)
  double re[3] = {0.4, -0.2, 0.3}, im[3] = {0.9, 0.5, -0.7};
  for (int it = 0; it < 300; ++it)
    for (int i = 0; i < 3; ++i) {
      const double zr = re[i], zi = im[i];
      double pr = zr + a1, pi = zi;
      double tr = pr * zr - pi * zi + a2, ti = pr * zi + pi * zr;
      pr = tr * zr - ti * zi + a3;
      pi = tr * zi + ti * zr;
      double dr = 1, di = 0;
      for (int j = 0; j < 3; ++j)
        if (j != i) {
          const double ar = zr - re[j], ai = zi - im[j];
          const double nr = dr * ar - di * ai, ni = dr * ai + di * ar;
          dr = nr;
          di = ni;
        }
      const double den = dr * dr + di * di;
      if (den == 0) continue;
      re[i] -= (pr * dr + pi * di) / den;
      im[i] -= (pi * dr - pr * di) / den;
    }
  double r = 0;
  for (int i = 0; i < 3; ++i) r = fmax(r, hypot(re[i], im[i]));
  return r;
}

}  // namespace

namespace wh {

// The per-call tables: utterance records, the channels' jobs (their lists in the workspace), taps, centre frequencies and
// tap geometry.  Persistent device buffers, copied only when their content changed.
int hv_upload(wh_ctx* ctx, hipStream_t st, const HvPlan& p, const double* h_band_taps, const double* h_band_f0, HvDev& d) {
  const int B = p.B, n_bands = p.n_bands;
  std::vector<BandJob> jobs((size_t)B * n_bands);
  for (int u = 0; u < B; ++u)
    for (int i = 0; i < n_bands; ++i) {
      BandJob& j = jobs[(size_t)u * n_bands + i];
      j.z = d.z + p.meta[u].z_off;
      j.M = p.meta[u].ylen;
      j.edges = d.e + p.e_off[(size_t)u * n_bands + i];
      j.cap = p.e_cap[(size_t)u * n_bands + i];
      j.counts = d.cnt + ((int64_t)u * n_bands + i) * 4;
      if (p.use_rawdet) {
        j.hints = d.hint + (p.meta[u].l_off + i) * 4;
        j.hint_tiles = p.meta[u].ntile;
        j.hint_spt = kRawTile * p.fs_d / 1000.0;
        j.hint_inv_spt = 1.0 / j.hint_spt;
        j.hint_stride = n_bands * 4;
      }
    }
  std::vector<double> taps(h_band_taps, h_band_taps + p.taps_total), bf(h_band_f0, h_band_f0 + n_bands);
  if (int rc = persistent_upload(ctx, st, "hv.meta", p.meta, &d.meta)) return rc;
  if (int rc = persistent_upload(ctx, st, "hv.jobs", jobs, &d.jobs)) return rc;
  if (int rc = persistent_upload(ctx, st, "hv.taps", taps, &d.taps)) return rc;
  if (int rc = persistent_upload(ctx, st, "hv.band_f0", bf, &d.band_f0)) return rc;
  if (int rc = persistent_upload(ctx, st, "hv.tapinfo", p.ti, &d.tapinfo)) return rc;
  return 0;
}

// Decimation to ~8 kHz (or the plain copy), then the mean-removed signal and its zero-padded twin.
int hv_launch_decimate(wh_ctx* ctx, hipStream_t st, const HvPlan& p, const double* x, const double* h_ba,
                       const double* h_zi, const HvDev& d) {
  const int B = p.B;
  if (p.filtered) {
    Tdf2 c;
    c.b0 = h_ba[0]; c.b1 = h_ba[1]; c.b2 = h_ba[2]; c.b3 = h_ba[3];
    c.a1 = h_ba[5] / h_ba[4]; c.a2 = h_ba[6] / h_ba[4]; c.a3 = h_ba[7] / h_ba[4];
    if (h_ba[4] != 1.0) { c.b0 /= h_ba[4]; c.b1 /= h_ba[4]; c.b2 /= h_ba[4]; c.b3 /= h_ba[4]; }
    c.zi0 = h_zi[0]; c.zi1 = h_zi[1]; c.zi2 = h_zi[2];
    // warm-up of a chunk's filter state: |pole|^warm < 1e-20
    const double rad = tdf2_pole_radius(c.a1, c.a2, c.a3);
    int warm = 64;
    if (rad > 0 && rad < 1) warm = (int)ceil(-46.0 / log(rad));
    warm = ((warm + 63) / 64) * 64;
    if (!(rad < 0.9999)) warm = 1 << 30;
    const int chunks = (int)((p.max_len + kHChunk - 1) / kHChunk);
    dim3 gi((chunks + 63) / 64, B);
    WH_LAUNCH(ctx, st, "hv_iir_fwd_kernel", hv_iir_fwd_kernel, gi, dim3(64), 0, x, d.meta, c, warm, d.tmp);
    WH_LAUNCH(ctx, st, "hv_iir_bwd_kernel", hv_iir_bwd_kernel, gi, dim3(64), 0, d.meta, c, warm, p.r, d.tmp, d.y);
  } else {
    WH_LAUNCH(ctx, st, "hv_copy_kernel", hv_copy_kernel, dim3((unsigned)((p.max_ylen + 255) / 256), B), dim3(256), 0, x,
              d.meta, d.y);
  }
  WH_LAUNCH(ctx, st, "hv_mean_kernel", hv_mean_part_kernel, dim3(kMeanParts, B), dim3(256), 0, d.meta, d.y, d.mean + B);
  WH_LAUNCH(ctx, st, "hv_mean_kernel", hv_mean_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, d.meta, d.mean + B,
            B, d.mean);
  WH_LAUNCH(ctx, st, "hv_pad_kernel", hv_pad_kernel, dim3((unsigned)((p.max_ylen + 2 * p.pad + 255) / 256), B),
            dim3(256), 0, d.meta, d.y, d.mean, p.pad, d.z);
  return 0;
}

// 152 channels: FIR + crossings — overlap-save products, or the direct FIR where the taps exceed a tile.
int hv_launch_band_events(wh_ctx* ctx, hipStream_t st, const HvPlan& p, const HvDev& d) {
  const int n_bands = p.n_bands;
  if (!p.use_ols)
    return launch_band_events(ctx, st, d.jobs, n_bands, p.B, p.pad, d.taps, d.tapinfo, d.tapinfo + n_bands,
                              d.tapinfo + 2 * n_bands, p.max_lb, ctx->d_flags + WH_FLAG_EVENT_OVERFLOW);
  int64_t* d_tile_off = nullptr;
  if (int rc = persistent_upload(ctx, st, "hv.tile_off", p.tile_off, &d_tile_off)) return rc;
  return launch_band_events_ols(ctx, st, d.jobs, n_bands, p.B, p.pad, p.h_max, d.taps, d.tapinfo, d.tapinfo + n_bands,
                                d.tapinfo + 2 * n_bands, d_tile_off, p.max_tiles, d.tspec, d.tre, d.zspec,
                                ctx->d_flags + WH_FLAG_EVENT_OVERFLOW);
}

// Per-frame raw candidates and their detection: one transposed pass, or the pair of kernels for a small batch.
int hv_launch_raw_detect(wh_ctx* ctx, hipStream_t st, const HvPlan& p, double f0_floor, double f0_ceil, const HvDev& d,
                         double* dbg_raw) {
  const int B = p.B, n_bands = p.n_bands;
  if (p.use_rawdet) {
    const int rd_xcd = B >= 8 ? 8 : 1;
    WH_LAUNCH(ctx, st, "hv_rawdet_kernel", hv_rawdet_kernel,
              dim3((unsigned)((int64_t)((B + rd_xcd - 1) / rd_xcd) * rd_xcd * p.max_ntile)), dim3(kRawTile), 0, d.meta,
              d.jobs, d.band_f0, d.hint, n_bands, B, rd_xcd, (int)p.max_ntile, p.fs_d, f0_floor, f0_ceil, d.dc, d.dn,
              dbg_raw ? d.raw : nullptr);
    if (dbg_raw) WH_CHECK(hipMemcpyAsync(dbg_raw, d.raw, sizeof(double) * p.f1_tot * n_bands, hipMemcpyDeviceToDevice, st));
    return 0;
  }
  // frames of an (utterance, channel) cut into segments with a workgroup each while the grid is a few rounds of the chip
  // (2560 workgroups at ten per CU): 1.80 -> 1.70 ms at 64 utterances; large batches keep one (no second cursor search)
  const int raw_segs = (int64_t)n_bands * B < 16 * 2560 ? 4 : 1;
  WH_LAUNCH(ctx, st, "hv_raw_kernel", hv_raw_kernel, dim3(n_bands, B, raw_segs), dim3(kRawTile), 0, d.meta, d.jobs,
            d.band_f0, n_bands, p.fs_d, f0_floor, f0_ceil, d.raw, d.live, dbg_raw ? 1 : 0);
  if (dbg_raw) WH_CHECK(hipMemcpyAsync(dbg_raw, d.raw, sizeof(double) * p.f1_tot * n_bands, hipMemcpyDeviceToDevice, st));
  WH_LAUNCH(ctx, st, "hv_detect_kernel", hv_detect_kernel, dim3((unsigned)((p.max_nf1 + 255) / 256), B), dim3(256), 0,
            d.meta, n_bands, d.raw, d.live, d.dc, d.dn);
  return 0;
}

}  // namespace wh
