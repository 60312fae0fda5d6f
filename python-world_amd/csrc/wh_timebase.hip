// The time base of synthesis(): everything that depends on tp / f0 / vuv alone (world/synthesis.py:118-140, 144-152).
//
//   prep_kernel     : per output sample: f0/vuv linear interpolation at t_i, phase increment
//                     2*pi*f0/fs (synthesis.py:121-128).  Embarrassingly parallel.
//   phase scan      : per utterance: the cumulative phase is a SEQUENTIAL float64 sum in the reference
//                     (np.cumsum); reproduced bit for bit by an integer prefix sum per binade of the running
//                     sum (exact_cumsum_block), so the pulse positions derived from it are NumPy's.
//   pulse_*_kernel  : wrap phase, detect pulses (|d wrap| > pi), ordered compaction, 1-based sample index and
//                     fractional shift per pulse, noise-stream offsets (synthesis.py:129-138, 65): tile-parallel
//                     mark / scan / emit, then a per-utterance finish.
// Pulse positions are read off this arithmetic, which must round like the reference's: the unit is built with the
// library's -ffp-contract=off and holds no contraction pragma.
#include "wh_host.h"
#include "wh_tid.h"  // (the opaque thread index of the spectral units)
#include "wh_device.h"
#include "wh_math.h"  // (behind wh_tid.h: it includes wh_device.h)
#include "wh_reduce.h"
#include "wh_syn_types.h"

namespace {
using wh::SynUtt;
using wh::PulseRec;
using wh::lerp_segment;
using wh::lerp_on;
using wh::block_excl_scan_256;

// f0_low_limit > 0: f0 is the F0 stage's output and is read as World.encode leaves it after CheapTrick (unvoiced or
// below 3 fs / (fft - 3) -> 500 Hz, cheaptrick.py:26-27,32-33) and D4C (unvoiced -> 0, d4c.py:32): the time base can
// then be computed while those two kernels are still running.
__global__ __launch_bounds__(256) void prep_kernel(const SynUtt* __restrict__ meta, const double* __restrict__ tp,
                                                   const double* __restrict__ f0, const double* __restrict__ vuv,
                                                   double fs, double f0_low_limit, double* __restrict__ phase,
                                                   uint8_t* __restrict__ vuv_s) {
  const SynUtt m = meta[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m.ny) return;
  const double t = m.t0 + (double)i * m.dt;
  const double* tpu = tp + m.f_off;
  const int64_t ih = lerp_segment(tpu, m.nf, t);  // one search serves both interpolants
  double f_raw;
  if (f0_low_limit > 0.0) {
    const double* fu = f0 + m.f_off;
    const double* vu = vuv + m.f_off;
    auto final_f0 = [&](int64_t k) { return vu[k] == 0.0 ? 0.0 : (fu[k] < f0_low_limit ? 500.0 : fu[k]); };
    const int64_t il = ih - 1;
    const double slope = (final_f0(ih) - final_f0(il)) / (tpu[ih] - tpu[il]);
    f_raw = slope * (t - tpu[il]) + final_f0(il);
  } else {
    f_raw = lerp_on(tpu, f0 + m.f_off, ih, t);
  }
  const bool v = lerp_on(tpu, vuv + m.f_off, ih, t) > 0.5;
  double fi = f_raw * (v ? 1.0 : 0.0);
  if (fi == 0.0) fi = fi + 500.0;  // default_f0, synthesis.py:126
  phase[m.y_off + i] = 2 * M_PI * fi / fs;
  vuv_s[m.y_off + i] = v ? 1 : 0;
}

// In-place cumulative sum of NON-NEGATIVE doubles, bit-identical to the sequential float64 sum (np.cumsum: one
// rounding per sample, left to right) — without being sequential.
//
// While the running sum a stays inside one binade [2^k, 2^(k+1)) every partial sum is a multiple of the binade's
// ulp q = 2^(k-52), and fl(a + x) = a + RN_q(x): the rounding of each addend to a multiple of q does not depend on
// a (except for exact ties, which round to the even neighbour of a + x).  So inside a binade the sequence is an
// INTEGER prefix sum of r_j = RN(x_j / q), exact in any order.  One workgroup per utterance walks 2048-sample tiles:
//   * r_j for its 8 samples per thread, thread-local prefix, block scan  -> V_j = a/q + sum r;
//   * the first stop point of the pass — an exact tie, or V_j >= 2^53 (the sum leaves the binade) — is found with
//     min-reductions; everything before it is final (value V_j * q);
//   * the stop element itself is done as the true floating-point add, becomes the new carry, and the pass
//     repeats behind it.  There are ~17 binade crossings and ~1 tie per binade in a whole utterance, so a tile
//     takes one pass almost always.
// 5 ns per sample for the sequential add chain (tools/ubench/chain.hip) becomes ~0.5 ns.
constexpr int kXTile = 4096;
constexpr int kXThreads = 512;
constexpr int kXPer = kXTile / kXThreads;
constexpr int kXLds = kXTile + kXTile / kXPer;  // padded tile (xpad)
__device__ __forceinline__ int xpad(int i) { return i + i / kXPer; }  // thread-contiguous runs of kXPer: odd stride in doubles

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}

// p[0..n): in place.  xin / xout: kXLds doubles of LDS each; scr: 32 doubles.  One workgroup of kXThreads.
// All integer quantities (r_j, their prefix sums, V_j < 2^53) are carried as integer-valued doubles: exact, and
// the whole pass stays on the FP64 pipe.
// carry_in: the running sum in front of p[0] (0 at the start of a sequence); returns the running sum behind p[n-1].
// (wh::ckp<T>: T* in every shipped build, a range-checked pointer in the bounds build — wh_device.h)
__device__ __forceinline__ double exact_cumsum_block(wh::ckp<double> WH_RESTRICT p, int64_t n, wh::ckp<double> xin, wh::ckp<double> xout,
                                                     wh::ckp<double> scr, double carry_in = 0.0) {
  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  constexpr double kTop = 0x1p53;  // V reaches this: the sum has left the binade
  double carry = carry_in;         // the running sum before the current tile (uniform)
  double pre[kXPer];               // the next tile, in flight from global memory while this one is scanned
#pragma unroll
  for (int q = 0; q < kXPer; ++q) {
    const int64_t i = (int64_t)q * kXThreads + tid;
    pre[q] = i < n ? p[i] : 0.0;
  }
  for (int64_t base = 0; base < n; base += kXTile) {
    const int cnt = (int)(n - base < kXTile ? n - base : kXTile);
#pragma unroll
    for (int q = 0; q < kXPer; ++q) xin[xpad(q * kXThreads + tid)] = pre[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kXPer; ++q) {
      const int64_t i = base + kXTile + (int64_t)q * kXThreads + tid;
      pre[q] = i < n ? p[i] : 0.0;
    }
    double x[kXPer];
#pragma unroll
    for (int j = 0; j < kXPer; ++j) x[j] = xin[xpad(tid * kXPer + j)];
    int s = 0;  // first element of the tile that is not final yet (uniform)
    while (s < cnt) {
      const int ebits = (int)((__double_as_longlong(carry) >> 52) & 0x7ff);
      int jstop = s;  // carry == 0 (or subnormal): fl(carry + x) straight away
      if (ebits != 0) {
        const int sh = 52 - (ebits - 1023);     // x / q = x * 2^sh, exact
        const double c_int = ldexp(carry, sh);  // in [2^52, 2^53)
        double r[kXPer];
        double run = 0.0;
        int first_tie = kXTile;
#pragma unroll
        for (int j = 0; j < kXPer; ++j) {
          const int idx = tid * kXPer + j;
          double rj = 0.0;
          if (idx >= s && idx < cnt) {
            const double sc = fmin(ldexp(x[j], sh), 0x1p54);
            const double fl = floor(sc);
            const double fr = sc - fl;  // exact: sc has at most 53 significant bits
            rj = fl + (fr > 0.5 ? 1.0 : 0.0);
            if (fr == 0.5 && first_tie == kXTile) first_tie = idx;
          }
          run += rj;   // exact while < 2^53; beyond that only "it is >= 2^53" matters, and that it stays
          r[j] = run;  // thread-local inclusive prefix
        }
        double incl = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const double u = __shfl_up(incl, o, 64);
          if (lane >= o) incl += u;
        }
        if (lane == 63) scr[w] = incl;
        __syncthreads();
        // exclusive prefix from the lanes below only: incl - run would go through this thread's own run, which is
        // inexact (>= 2^53) once the thread lies behind a binade crossing — and would spoil lanes that do not
        double excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 0.0;
        double before = c_int + excl;  // V just before this thread's first element
        for (int i = 0; i < w; ++i) before += scr[i];
        int first_x = kXTile;
#pragma unroll
        for (int j = 0; j < kXPer; ++j) {
          const int idx = tid * kXPer + j;
          if (idx >= s && idx < cnt && before + r[j] >= kTop && first_x == kXTile) first_x = idx;
        }
        const int mine = wave_min_int(first_tie < first_x ? first_tie : first_x);
        const wh::ckp<int> iscr = wh::ck_as<int>(scr + 16);
        if (lane == 0) iscr[w] = mine;
        __syncthreads();
        jstop = iscr[0];
#pragma unroll
        for (int i = 1; i < kXThreads / 64; ++i) jstop = iscr[i] < jstop ? iscr[i] : jstop;
        if (jstop > cnt) jstop = cnt;
        const double q = ldexp(1.0, -sh);
#pragma unroll
        for (int j = 0; j < kXPer; ++j) {
          const int idx = tid * kXPer + j;
          if (idx >= s && idx < jstop) xout[xpad(idx)] = (before + r[j]) * q;  // V < 2^53 times a power of two: exact
        }
        __syncthreads();
      }
      if (jstop < cnt) {  // the stop element: the floating-point add itself
        const double a = jstop == s ? carry : xout[xpad(jstop - 1)];
        const double res = a + xin[xpad(jstop)];
        __syncthreads();  // everyone has read xout[jstop - 1] / scr before they change
        if (tid == 0) xout[xpad(jstop)] = res;
        carry = res;
        s = jstop + 1;
      } else {
        carry = xout[xpad(cnt - 1)];
        s = cnt;
      }
    }
    __syncthreads();
    for (int i = tid; i < cnt; i += kXThreads) p[base + i] = xout[xpad(i)];
    __syncthreads();
  }
  return carry;
}

// The same scan over (begin, end) pairs: pairs[2i] .. pairs[2i+1].
__global__ __launch_bounds__(kXThreads) void exact_cumsum_pairs_kernel(double* __restrict__ data,
                                                                       const int64_t* __restrict__ pairs) {
  __shared__ double xin[kXLds], xout[kXLds], scr[32];
  const int64_t n = pairs[2 * blockIdx.x + 1] - pairs[2 * blockIdx.x];
  exact_cumsum_block(wh::ck_make(data + pairs[2 * blockIdx.x], n, wh::WH_CK_OUT), n, wh::ck_make(xin, kXLds, wh::WH_CK_LDS_MAIN),
                     wh::ck_make(xout, kXLds, wh::WH_CK_LDS_AUX), wh::ck_make(scr, 32, wh::WH_CK_LDS_SCRATCH));
}

// ---- the same scan, tile-parallel -----------------------------------------------------------------------------------
// One workgroup per sequence leaves the chip idle for long sequences (60 s at 48 kHz after scale_duration(2): 5.76 M
// samples on each of 16 workgroups, 4.7 ms).  Inside a binade every partial sum is carry + q * (integer prefix of
// r_j = RN(x_j / q)), and r_j does not depend on the carry unless x_j / q is an exact tie — so a tile of kXTile samples
// that (i) lies inside one binade and (ii) holds no tie needs nothing from its predecessors but the carry, as an
// additive constant.  Five passes:
//   xs_tile_sum_kernel   : plain floating-point tile sums S_t                                  (all tiles in parallel)
//   xs_prefix_kernel     : their running sums A_t per sequence: the carry in front of tile t to ~1e-12, enough to name
//                          its binade unless it sits on a power of two                          (one lane per sequence)
//   xs_tile_total_kernel : with the binade of A_t: T_t = sum r_j (exact integer), tile flagged if a tie, an over-long
//                          step or a zero / subnormal carry shows                               (all tiles in parallel)
//   xs_carry_kernel      : per sequence, in order: a lane walks the unflagged tiles with EXACT carries — checking that
//                          the true carry has the assumed exponent and that carry/q + T_t stays below 2^53 — and
//                          stores each tile's carry; at a flagged tile, or one that fails the check, the whole
//                          workgroup runs the sequential-equivalent exact_cumsum_block on that tile with the exact
//                          carry (a few dozen tiles per sequence: the binade crossings and the ties)
//   xs_apply_kernel      : carry + q * (local integer prefix) for the tiles the walk accepted   (all tiles in parallel)
// Bit-identical to np.cumsum by the same argument as exact_cumsum_block; nothing is accepted on the approximate sums
// alone.
struct XsTile {
  double T;     // sum of r_j in units of q (integer-valued), valid when flag == 0
  int32_t sh;   // x / q = x * 2^sh for the assumed binade
  int32_t flag; // 0: candidate for the closed form, 1: needs the exact block scan, 2: done by xs_carry_kernel
};

__device__ __forceinline__ int xs_find_seq(const int64_t* __restrict__ tile_base, int n_seg, int64_t t) {
  int lo = 0, hi = n_seg;  // largest s with tile_base[s] <= t
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_base[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// pairs: sequence sq is data[pairs[2 sq] .. pairs[2 sq + 1]); tile_base[sq]: number of tiles in front of it.
__global__ __launch_bounds__(256) void xs_tile_sum_kernel(const double* __restrict__ data, const int64_t* __restrict__ pairs,
                                                          const int64_t* __restrict__ tile_base, int n_seg,
                                                          double* __restrict__ S) {
  __shared__ double red[8];
  const int64_t t = blockIdx.x;
  const int sq = xs_find_seq(tile_base, n_seg, t);
  const int64_t begin = pairs[2 * sq] + (t - tile_base[sq]) * kXTile;
  const int64_t end = begin + kXTile < pairs[2 * sq + 1] ? begin + kXTile : pairs[2 * sq + 1];
  double acc = 0.0;
  for (int64_t i = begin + threadIdx.x; i < end; i += 256) acc += data[i];
  acc = wh::block_sum<256>(acc, red);
  if (threadIdx.x == 0) S[t] = acc;
}

__global__ __launch_bounds__(64) void xs_prefix_kernel(const int64_t* __restrict__ tile_base, int n_seg,
                                                       double* __restrict__ S) {
  const int sq = blockIdx.x * 64 + threadIdx.x;
  if (sq >= n_seg) return;
  double run = 0.0;  // S[t] becomes the (approximate) carry in front of tile t
  wh::serial_run<16>(
      tile_base[sq], tile_base[sq + 1], [](int64_t) { return true; }, [&](int64_t t) { return S[t]; },
      [&](int64_t t) { return S[t]; },
      [&](int64_t t, double v) {
        S[t] = run;
        run += v;
      });
}

__global__ __launch_bounds__(256) void xs_tile_total_kernel(const double* __restrict__ data, const int64_t* __restrict__ pairs,
                                                            const int64_t* __restrict__ tile_base, int n_seg,
                                                            const double* __restrict__ A, XsTile* __restrict__ tiles) {
  __shared__ double red[8];
  __shared__ int bad_any;
  const int64_t t = blockIdx.x;
  const int sq = xs_find_seq(tile_base, n_seg, t);
  const int64_t begin = pairs[2 * sq] + (t - tile_base[sq]) * kXTile;
  const int64_t end = begin + kXTile < pairs[2 * sq + 1] ? begin + kXTile : pairs[2 * sq + 1];
  const double a = A[t];
  const int ebits = (int)((__double_as_longlong(a) >> 52) & 0x7ff);
  if (threadIdx.x == 0) bad_any = 0;
  __syncthreads();
  XsTile out;
  out.T = 0.0;
  out.sh = 0;
  out.flag = 1;
  if (ebits != 0 && ebits != 0x7ff && a > 0.0) {
    const int sh = 52 - (ebits - 1023);
    double acc = 0.0;
    bool bad = false;
    for (int64_t i = begin + threadIdx.x; i < end; i += 256) {
      const double x = data[i];
      const double sc = fmin(ldexp(x, sh), 0x1p54);
      const double fl = floor(sc);
      const double fr = sc - fl;
      bad = bad || fr == 0.5 || !(sc < 0x1p52) || !(x >= 0.0);  // a tie, a step of a whole binade, a negative / NaN addend
      acc += fl + (fr > 0.5 ? 1.0 : 0.0);
    }
    if (bad) bad_any = 1;
    acc = wh::block_sum<256>(acc, red);  // (two barriers: bad_any is visible behind them)
    out.T = acc;
    out.sh = sh;
    out.flag = (bad_any || !(acc < 0x1p52)) ? 1 : 0;  // partial sums below 2^52: every addition was exact
  }
  if (threadIdx.x == 0) tiles[t] = out;
}

__global__ __launch_bounds__(kXThreads) void xs_carry_kernel(double* __restrict__ data, const int64_t* __restrict__ pairs,
                                                             const int64_t* __restrict__ tile_base,
                                                             XsTile* __restrict__ tiles, double* __restrict__ C) {
  constexpr int kWin = 1024;  // tile records staged per round for the walking lane
  __shared__ double xin[kXLds], xout[kXLds], scr[32];
  __shared__ XsTile win[kWin];
  __shared__ long long sh_t;
  __shared__ double sh_a;
  const int sq = blockIdx.x;
  const int64_t t0 = tile_base[sq], t1 = tile_base[sq + 1];
  double a = 0.0;  // exact running sum in front of tile t (block-uniform)
  int64_t t = t0;
  while (t < t1) {
    const int nw = (int)(t1 - t < kWin ? t1 - t : kWin);
    for (int i = threadIdx.x; i < nw; i += kXThreads) win[i] = tiles[t + i];
    __syncthreads();
    if (threadIdx.x == 0) {
      int i = 0;
      double aa = a;
      for (; i < nw; ++i) {
        const XsTile cur = win[i];
        if (cur.flag != 0) break;
        const int ebits = (int)((__double_as_longlong(aa) >> 52) & 0x7ff);
        if (ebits == 0 || 52 - (ebits - 1023) != cur.sh) break;  // the true carry is not in the binade the tile assumed
        const double v = ldexp(aa, cur.sh) + cur.T;                // carry/q + T: both integers below 2^53, exact
        if (!(v < 0x1p53)) break;                                   // the tile would leave the binade
        C[t + i] = aa;
        aa = ldexp(v, -cur.sh);
      }
      sh_t = t + i;
      sh_a = aa;
    }
    __syncthreads();
    const int64_t tn = sh_t;
    a = sh_a;
    const bool stopped = tn < t + nw;  // inside the window: tile tn needs the sequential-equivalent scan
    t = tn;
    __syncthreads();
    if (stopped) {
      const int64_t begin = pairs[2 * sq] + (t - t0) * kXTile;
      const int64_t end = begin + kXTile < pairs[2 * sq + 1] ? begin + kXTile : pairs[2 * sq + 1];
      a = exact_cumsum_block(wh::ck_make(data + begin, end - begin, wh::WH_CK_OUT), end - begin, wh::ck_make(xin, kXLds, wh::WH_CK_LDS_MAIN),
                             wh::ck_make(xout, kXLds, wh::WH_CK_LDS_AUX), wh::ck_make(scr, 32, wh::WH_CK_LDS_SCRATCH), a);
      if (threadIdx.x == 0) tiles[t].flag = 2;
      ++t;
    }
  }
}

__global__ __launch_bounds__(256) void xs_apply_kernel(double* __restrict__ data, const int64_t* __restrict__ pairs,
                                                       const int64_t* __restrict__ tile_base, int n_seg,
                                                       const XsTile* __restrict__ tiles, const double* __restrict__ C) {
  constexpr int PER = kXTile / 256;
  __shared__ double buf[kXTile + kXTile / PER];  // thread-contiguous runs of PER at an odd stride (bank conflicts)
  __shared__ double wsum[4];
  auto pad = [](int i) { return i + i / PER; };
  const int64_t t = blockIdx.x;
  const XsTile tl = tiles[t];
  if (tl.flag != 0) return;
  const int sq = xs_find_seq(tile_base, n_seg, t);
  const int64_t begin = pairs[2 * sq] + (t - tile_base[sq]) * kXTile;
  const int64_t end = begin + kXTile < pairs[2 * sq + 1] ? begin + kXTile : pairs[2 * sq + 1];
  const int cnt = (int)(end - begin);
  const int sh = tl.sh;
  // coalesced in, thread-contiguous through LDS (the order of an integer prefix sum is free), coalesced out
  for (int i = threadIdx.x; i < cnt; i += 256) buf[pad(i)] = data[begin + i];
  __syncthreads();
  double r[PER];
  double run = 0.0;
  const int i0 = threadIdx.x * PER;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int idx = i0 + j;
    double rj = 0.0;
    if (idx < cnt) {
      const double sc = ldexp(buf[pad(idx)], sh);
      const double fl = floor(sc);
      rj = fl + (sc - fl > 0.5 ? 1.0 : 0.0);
    }
    run += rj;
    r[j] = run;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double incl = run;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  double before = ldexp(C[t], sh) + (incl - run);  // all integers below 2^53: exact
  for (int i = 0; i < w; ++i) before += wsum[i];
  const double q = ldexp(1.0, -sh);
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int idx = i0 + j;
    if (idx < cnt) buf[pad(idx)] = (before + r[j]) * q;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cnt; i += 256) data[begin + i] = buf[pad(i)];
}

// Host side of the scan: sequences of more than kXsMinTiles tiles take the tile-parallel passes (all of them in one
// set of launches), the rest the one-workgroup-per-sequence kernel (10 s at 16 kHz is 40 tiles, a dozen of which hold a
// binade crossing or a tie: 0.21 ms either way; 120 s at 48 kHz is 1407 tiles: 1.2 against 4.7 ms).
// h_off: n_seg + 1 offsets into d_data (HOST).
constexpr int kXsMinTiles = 64;
}  // namespace
int wh::exact_cumsum_segments(wh_ctx* ctx, hipStream_t st, double* d_data, const int64_t* h_off, int n_seg) {
  std::vector<int64_t> s_pairs, l_pairs, tb{0};
  for (int i = 0; i < n_seg; ++i) {
    const int64_t tiles = (h_off[i + 1] - h_off[i] + kXTile - 1) / kXTile;
    std::vector<int64_t>& dst = tiles > kXsMinTiles ? l_pairs : s_pairs;
    dst.push_back(h_off[i]);
    dst.push_back(h_off[i + 1]);
    if (tiles > kXsMinTiles) tb.push_back(tb.back() + tiles);
  }
  if (!s_pairs.empty()) {
    int64_t* d_sp = nullptr;
    if (int rc = wh::persistent_upload(ctx, st, "cumsum.short", s_pairs, &d_sp)) return rc;
    WH_LAUNCH(ctx, st, "phase_kernel", exact_cumsum_pairs_kernel, dim3((unsigned)(s_pairs.size() / 2)), dim3(kXThreads),
              0, d_data, d_sp);
  }
  if (l_pairs.empty()) return 0;
  const int ns = (int)(l_pairs.size() / 2);
  const int64_t nt = tb[ns];
  int64_t *d_lp = nullptr, *d_tb = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "cumsum.long", l_pairs, &d_lp)) return rc;
  if (int rc = wh::persistent_upload(ctx, st, "cumsum.tiles", tb, &d_tb)) return rc;
  wh::Carve c;  // per tile: S / A, C (doubles) and the tile record
  const auto r_S = c.take<double>(nt), r_C = c.take<double>(nt);
  const auto r_tiles = c.take<XsTile>(nt);
  if (!c.ok()) return wh::fail_msg("exact_cumsum_segments", "scratch size beyond size_t");
  char* d_scr = nullptr;
  if (int rc = wh::persistent_scratch(ctx, "cumsum.scratch", c.end(), &d_scr)) return rc;
  double *d_S = r_S.at(d_scr), *d_C = r_C.at(d_scr);
  XsTile* d_tiles = r_tiles.at(d_scr);
  WH_LAUNCH(ctx, st, "xs_tile_sum_kernel", xs_tile_sum_kernel, dim3((unsigned)nt), dim3(256), 0, d_data, d_lp, d_tb, ns,
            d_S);
  WH_LAUNCH(ctx, st, "xs_prefix_kernel", xs_prefix_kernel, dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, d_tb, ns,
            d_S);
  WH_LAUNCH(ctx, st, "xs_tile_total_kernel", xs_tile_total_kernel, dim3((unsigned)nt), dim3(256), 0, d_data, d_lp, d_tb,
            ns, d_S, d_tiles);
  WH_LAUNCH(ctx, st, "xs_carry_kernel", xs_carry_kernel, dim3((unsigned)ns), dim3(kXThreads), 0, d_data, d_lp, d_tb,
            d_tiles, d_C);
  WH_LAUNCH(ctx, st, "xs_apply_kernel", xs_apply_kernel, dim3((unsigned)nt), dim3(256), 0, d_data, d_lp, d_tb, ns,
            d_tiles, d_C);
  return 0;
}
namespace {

// Pulse detection (synthesis.py:129-138) in four launches, none of them serial in the utterance length:
//   pulse_mark_kernel   : one workgroup per 1024-sample tile: wrap the phase, mark |d wrap| > pi, count;
//   pulse_scan_kernel   : one workgroup per utterance: exclusive scan of its tile counts, pulse count;
//   pulse_emit_kernel   : one workgroup per tile: ordered compaction into the utterance's pulse slots;
//   pulse_finish_kernel : one workgroup per utterance: fractional shifts and the noise-stream offsets
//                         (exclusive prefix sum of max(3, noise_size), synthesis.py:65).
constexpr int kPTile = 1024;
constexpr int kPFinish = 1024;  // threads of pulse_finish_kernel (one workgroup per utterance)


__global__ __launch_bounds__(256) void pulse_mark_kernel(const SynUtt* __restrict__ meta, const double* __restrict__ phase,
                                                         int max_tiles, uint8_t* __restrict__ masks,
                                                         int32_t* __restrict__ tile_cnt) {
  __shared__ double wr[kPTile + 1];
  __shared__ int wsum[4];
  const SynUtt m = meta[blockIdx.y];
  const int64_t t0 = (int64_t)blockIdx.x * kPTile;
  if (t0 >= m.ny - 1) return;
  const double* ph = phase + m.y_off;
  const double two_pi = 2 * M_PI;
  for (int i = threadIdx.x; i < kPTile + 1; i += 256) {
    const int64_t g = t0 + i;
    wr[i] = g < m.ny ? fmod(ph[g], two_pi) : 0.0;  // np.remainder of a non-negative value
  }
  __syncthreads();
  unsigned mask = 0;  // 4 consecutive samples per thread
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = threadIdx.x * 4 + q;
    const int64_t g = t0 + i;
    if (g < m.ny - 1 && fabs(wr[i + 1] - wr[i]) > M_PI) mask |= 1u << q;
  }
  int total;
  (void)block_excl_scan_256(__popc(mask), wsum, &total);
  const int64_t slot = (int64_t)blockIdx.y * max_tiles + blockIdx.x;
  masks[slot * 256 + threadIdx.x] = (uint8_t)mask;
  if (threadIdx.x == 0) tile_cnt[slot] = total;
}

__global__ __launch_bounds__(256) void pulse_scan_kernel(const SynUtt* __restrict__ meta, int max_tiles,
                                                         int32_t* __restrict__ tile_cnt, int32_t* __restrict__ p_count,
                                                         int32_t* __restrict__ flags) {
  __shared__ int wsum[4];
  const SynUtt m = meta[blockIdx.x];
  const int tiles = m.ny > 1 ? (int)((m.ny - 1 + kPTile - 1) / kPTile) : 0;
  int32_t* tc = tile_cnt + (int64_t)blockIdx.x * max_tiles;
  int run = 0;
  for (int base = 0; base < tiles; base += 256) {
    const int i = base + threadIdx.x;
    const int c = i < tiles ? tc[i] : 0;
    int total;
    const int excl = block_excl_scan_256(c, wsum, &total);
    if (i < tiles) tc[i] = run + excl;
    run += total;
  }
  if (threadIdx.x == 0) {
    if (run > m.pcap) atomicOr(flags + WH_FLAG_PULSE_OVERFLOW, 1);
    if (run == 0) atomicOr(flags + WH_FLAG_NO_PULSE, 1);
    p_count[blockIdx.x] = run > m.pcap ? (int)m.pcap : run;
  }
}

__global__ __launch_bounds__(256) void pulse_emit_kernel(const SynUtt* __restrict__ meta, int max_tiles,
                                                         const uint8_t* __restrict__ masks,
                                                         const int32_t* __restrict__ tile_pos, double fs,
                                                         double* __restrict__ p_time, int64_t* __restrict__ p_idx) {
  __shared__ int wsum[4];
  const SynUtt m = meta[blockIdx.y];
  const int64_t t0 = (int64_t)blockIdx.x * kPTile;
  if (t0 >= m.ny - 1) return;
  const int64_t slot = (int64_t)blockIdx.y * max_tiles + blockIdx.x;
  const unsigned mask = masks[slot * 256 + threadIdx.x];
  int total;
  int pos = tile_pos[slot] + block_excl_scan_256(__popc(mask), wsum, &total);
  double* pt = p_time + m.p_off;
  int64_t* pi = p_idx + m.p_off;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (mask & (1u << q)) {
      if (pos < m.pcap) {
        const int64_t g = t0 + threadIdx.x * 4 + q;
        const double tt = m.t0 + (double)g * m.dt;
        pt[pos] = tt;
        pi[pos] = (int64_t)floor(tt * fs + 0.5) + 1;  // Decimal ROUND_HALF_UP then +1 (synthesis.py:132)
      }
      ++pos;
    }
  }
}

__global__ __launch_bounds__(kPFinish) void pulse_finish_kernel(const SynUtt* __restrict__ meta,
                                                                const double* __restrict__ phase, double fs,
                                                                const int64_t* __restrict__ p_idx,
                                                                const int32_t* __restrict__ p_count,
                                                                double* __restrict__ p_shift, int64_t* __restrict__ p_noff,
                                                                int32_t* __restrict__ flags) {
  __shared__ long long wsum64[kPFinish / 64];
  const SynUtt m = meta[blockIdx.x];
  const double* ph = phase + m.y_off;
  const int64_t* pi = p_idx + m.p_off;
  double* psh = p_shift + m.p_off;
  int64_t* pn = p_noff + m.p_off;
  const double two_pi = 2 * M_PI;
  const int count = p_count[blockIdx.x];
  long long run = 0;
  for (int base = 0; base < count; base += kPFinish) {
    const int i = base + threadIdx.x;
    long long d = 0;
    if (i < count) {
      int64_t id = pi[i];
      int64_t a = id - 1, b = id;  // wrap_phase[idx-1], wrap_phase[idx]
      a = a < 0 ? 0 : (a > m.ny - 1 ? m.ny - 1 : a);
      b = b < 0 ? 0 : (b > m.ny - 1 ? m.ny - 1 : b);
      const double y1 = fmod(ph[a], two_pi) - 2.0 * M_PI;
      const double y2 = fmod(ph[b], two_pi);
      psh[i] = (-y1 / (y2 - y1)) / fs;
      const int64_t nxt = pi[i + 1 < count ? i + 1 : count - 1];
      const int64_t ns = nxt - id;
      d = ns > 3 ? ns : 3;
    }
    long long incl = d;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long uu = __shfl_up(incl, o, 64);
      if (lane >= o) incl += uu;
    }
    __syncthreads();
    if (lane == 63) wsum64[threadIdx.x >> 6] = incl;
    __syncthreads();
    long long excl = incl - d, total = 0;
    for (int w = 0; w < kPFinish / 64; ++w) {
      if (w < (int)(threadIdx.x >> 6)) excl += wsum64[w];
      total += wsum64[w];
    }
    if (i < count) pn[i] = run + excl;
    run += total;
  }
  // (whether a host-supplied noise stream covers `run` draws is tested by wh_synthesis_render, which is the call that
  // knows the stream: noise_cover_kernel)
}

// Exclusive prefix of the per-utterance pulse counts → flat pulse numbering for the response grid.
__global__ void pulse_base_kernel(const int32_t* __restrict__ p_count, int n_utt, int64_t* __restrict__ base) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int64_t run = 0;
    for (int u = 0; u < n_utt; ++u) {
      base[u] = run;
      run += p_count[u];
    }
    base[n_utt] = run;
  }
}

// Per pulse: the two frames it interpolates between and the weight of the later one (synthesis.py:49-51,144-180).
// One thread per pulse here, so that the 256-thread response workgroups do not each walk the same 11-deep chain of
// dependent loads (binary search over the frame times) before they can start.
__global__ __launch_bounds__(256) void pulse_frames_kernel(const SynUtt* __restrict__ meta, const double* __restrict__ tp,
                                                           const double* __restrict__ p_time,
                                                           const int64_t* __restrict__ p_idx,
                                                           const double* __restrict__ p_shift,
                                                           const int64_t* __restrict__ p_noff,
                                                           const uint8_t* __restrict__ vuv_s,
                                                           const int32_t* __restrict__ p_count,
                                                           const int64_t* __restrict__ p_base,
                                                           PulseRec* __restrict__ p_rec) {
  const SynUtt m = meta[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int count = p_count[blockIdx.y];
  if (i >= count) return;
  const double* tpu = tp + m.f_off;
  const double ptime = p_time[m.p_off + i];
  // temporal_position_index = interp(tp -> 1..F)(time), clipped to [1, F]
  int64_t lo = 0, hi = m.nf;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (tpu[mid] < ptime) lo = mid + 1; else hi = mid;
  }
  const int64_t ih = lo < 1 ? 1 : (lo > m.nf - 1 ? m.nf - 1 : lo);
  const int64_t il = ih - 1;
  const double slope = ((double)(ih + 1) - (double)(il + 1)) / (tpu[ih] - tpu[il]);
  double pos = slope * (ptime - tpu[il]) + (double)(il + 1);
  pos = fmax(1.0, fmin((double)m.nf, pos));
  const int64_t flo = (int64_t)floor(pos) - 1;
  const int64_t fhi = (int64_t)ceil(pos) - 1;
  const double t1 = tpu[flo], t2 = tpu[fhi];
  const double xq = fmax(t1, fmin(t2, ptime));
  PulseRec r;
  r.pidx = p_idx[m.p_off + i];
  r.rows = (m.f_off + flo) | ((m.f_off + fhi) << 32);
  r.weight = (t1 == t2) ? -1.0 : (xq - t1) / (t2 - t1);
  r.shift = p_shift[m.p_off + i];
  r.noff = p_noff[m.p_off + i];
  r.u = blockIdx.y;
  r.noise_size = (int32_t)(p_idx[m.p_off + (i + 1 < count ? i + 1 : count - 1)] - r.pidx);
  int64_t vi = r.pidx - 1;
  vi = vi < 0 ? 0 : (vi > m.ny - 1 ? m.ny - 1 : vi);
  r.vuv = vuv_s[m.y_off + vi] != 0 ? 1 : 0;
  r.pad_[0] = r.pad_[1] = r.pad_[2] = 0;
  p_rec[p_base[blockIdx.y] + i] = r;  // flat pulse numbering: utterance by utterance, in time order
}

inline int pulse_tiles(int64_t max_ny) { return max_ny > 1 ? (int)((max_ny - 1 + kPTile - 1) / kPTile) : 1; }
}  // namespace

wh::TimeBaseLayout::TimeBaseLayout(Carve& c, int B, int64_t ny_tot, int64_t pulse_cap, int64_t max_ny) {
  const int64_t slots = B * pulse_cap, tiles = (int64_t)B * pulse_tiles(max_ny);
  phase = c.take<double>(ny_tot);
  vuv = c.take<uint8_t>(ny_tot);
  pt = c.take<double>(slots);
  pi = c.take<int64_t>(slots);
  ps = c.take<double>(slots);
  pn = c.take<int64_t>(slots);
  pc = c.take<int32_t>(B);
  masks = c.take<uint8_t>(tiles * 256);
  tile_cnt = c.take<int32_t>(tiles);
}

int wh::launch_pulses(wh_ctx* ctx, hipStream_t st, int B, int64_t max_ny, const SynUtt* d_meta, const double* tp,
                      const double* f0, const double* vuv, double fs, double f0_low_limit, const int64_t* h_y_off, void* ws,
                      const TimeBaseLayout& lay) {
  double *d_phase = lay.phase.at(ws), *d_pt = lay.pt.at(ws), *d_ps = lay.ps.at(ws);
  int64_t *d_pi = lay.pi.at(ws), *d_pn = lay.pn.at(ws);
  int32_t *d_pc = lay.pc.at(ws), *d_tc = lay.tile_cnt.at(ws);
  uint8_t *d_vuv = lay.vuv.at(ws), *d_masks = lay.masks.at(ws);
  WH_LAUNCH(ctx, st, "prep_kernel", prep_kernel, dim3((unsigned)((max_ny + 255) / 256), B), dim3(256), 0, d_meta, tp,
            f0, vuv, fs, f0_low_limit, d_phase, d_vuv);
  if (int rc = exact_cumsum_segments(ctx, st, d_phase, h_y_off, B)) return rc;
  const int mt = pulse_tiles(max_ny);
  WH_LAUNCH(ctx, st, "pulse_mark_kernel", pulse_mark_kernel, dim3(mt, B), dim3(256), 0, d_meta, d_phase, mt, d_masks,
            d_tc);
  WH_LAUNCH(ctx, st, "pulse_scan_kernel", pulse_scan_kernel, dim3(B), dim3(256), 0, d_meta, mt, d_tc, d_pc,
            ctx->d_flags);
  WH_LAUNCH(ctx, st, "pulse_emit_kernel", pulse_emit_kernel, dim3(mt, B), dim3(256), 0, d_meta, mt, d_masks, d_tc, fs,
            d_pt, d_pi);
  WH_LAUNCH(ctx, st, "pulse_finish_kernel", pulse_finish_kernel, dim3(B), dim3(kPFinish), 0, d_meta, d_phase, fs, d_pi,
            d_pc, d_ps, d_pn, ctx->d_flags);
  return 0;
}

int wh::fill_syn_meta(const char* who, const wh_batch* b, const int64_t* h_y_off, const double* h_t0, const double* h_dt,
                      int64_t pulse_cap, const double* noise, const int64_t* h_noise_off, std::vector<SynUtt>& meta,
                      int64_t* max_ny) {
  const int B = b->n_utt;
  meta.resize(B);
  *max_ny = 0;
  for (int u = 0; u < B; ++u) {
    SynUtt& m = meta[u];
    m.f_off = b->h_frame_off[u];
    m.nf = b->h_frame_off[u + 1] - b->h_frame_off[u];
    if (m.nf < 2) return wh::fail_msg(who, "an utterance has fewer than 2 frames");
    m.y_off = h_y_off[u];
    m.ny = h_y_off[u + 1] - h_y_off[u];
    m.p_off = (int64_t)u * pulse_cap;
    m.pcap = pulse_cap;
    m.noise_off = noise ? h_noise_off[u] : 0;
    m.noise_len = noise ? h_noise_off[u + 1] - h_noise_off[u] : -1;
    m.t0 = h_t0[u];
    m.dt = h_dt[u];
    *max_ny = std::max(*max_ny, m.ny);
  }
  return 0;
}

// Time base of synthesis(): everything that depends on tp / f0 / vuv alone (synthesis.py:118-140, 144-152) — phase
// increments, the exact cumulative phase, pulse positions and fractional shifts, noise offsets, per-pulse frame pairs.
// The results stay in ctx's workspace (ctx->timebase records where) until another call lays the workspace out again.
extern "C" int wh_synthesis_timebase(wh_ctx* ctx, void* stream, const wh_batch* b, const double* tp, const double* f0,
                                     const double* vuv, double fs, const int64_t* h_y_off, const double* h_t0,
                                     const double* h_dt, int64_t pulse_cap, double f0_low_limit) {
  if (!ctx || !b || !tp || !f0 || !vuv || !h_y_off || !h_t0 || !h_dt)
    return wh::fail_msg("wh_synthesis_timebase", "null argument");
  WH_ENTER(ctx);
  if (pulse_cap < 1) return wh::fail_msg("wh_synthesis_timebase", "pulse_cap must be >= 1");
  hipStream_t st = (hipStream_t)stream;
  const int B = b->n_utt;
  std::vector<SynUtt> meta;
  int64_t max_ny = 0;
  if (int rc = wh::fill_syn_meta("wh_synthesis_timebase", b, h_y_off, h_t0, h_dt, pulse_cap, nullptr, nullptr, meta, &max_ny)) return rc;
  const int64_t ny_tot = h_y_off[B];
  wh::Carve carve;
  const wh::TimeBaseLayout lay(carve, B, ny_tot, pulse_cap, max_ny);
  const auto r_pb = carve.take<int64_t>(B + 1);
  const auto r_rec = carve.take<PulseRec>(B * pulse_cap);
  if (int rc = wh::ws_reserve(ctx, carve)) return rc;
  ctx->timebase.valid = false;
  void* ws = ctx->ws;
  SynUtt* d_meta = nullptr;
  int64_t* d_pb = r_pb.at(ws);
  const int32_t* d_pc = lay.pc.at(ws);
  if (int rc = wh::persistent_upload(ctx, st, "syn.tbmeta", meta, &d_meta)) return rc;
  if (int rc = wh::launch_pulses(ctx, st, B, max_ny, d_meta, tp, f0, vuv, fs, f0_low_limit, h_y_off, ws, lay)) return rc;
  WH_LAUNCH(ctx, st, "pulse_base_kernel", pulse_base_kernel, dim3(1), dim3(64), 0, d_pc, B, d_pb);
  WH_LAUNCH(ctx, st, "pulse_frames_kernel", pulse_frames_kernel, dim3((unsigned)((pulse_cap + 255) / 256), B),
            dim3(256), 0, d_meta, tp, lay.pt.at(ws), lay.pi.at(ws), lay.ps.at(ws), lay.pn.at(ws), lay.vuv.at(ws), d_pc,
            d_pb, r_rec.at(ws));
  wh_ctx::TimeBase& t = ctx->timebase;
  t.valid = true;
  t.n_utt = B;
  t.pulse_cap = pulse_cap;
  t.ny_tot = ny_tot;
  t.frames = b->total_frames;
  t.phase = lay.phase; t.vuv = lay.vuv; t.pt = lay.pt; t.pi = lay.pi; t.ps = lay.ps; t.pn = lay.pn; t.pc = lay.pc;
  t.pb = r_pb;
  t.rec = r_rec;
  t.f_off.assign(b->h_frame_off.begin(), b->h_frame_off.begin() + B);
  return 0;
}

// What that call left, on the host (see world_hip.h): copies only — no launch, nothing in the workspace changes.
extern "C" int wh_synthesis_timebase_read(wh_ctx* ctx, void* stream, int n_utt, int64_t pulse_cap, int64_t n_samples,
                                          int32_t* h_count, int64_t* h_base, int64_t* h_pidx, double* h_time,
                                          double* h_shift, int64_t* h_noff, int32_t* h_noise_size, int32_t* h_vuv,
                                          int64_t* h_row_lo, int64_t* h_row_hi, double* h_weight, double* h_phase,
                                          uint8_t* h_vuv_s) {
  if (!ctx) return wh::fail_msg("wh_synthesis_timebase_read", "null ctx");
  const wh_ctx::TimeBase& t = ctx->timebase;
  if (!t.valid) return wh::fail_msg("wh_synthesis_timebase_read", "no time base (run wh_synthesis_timebase on this context, and nothing that uses its workspace since)");
  if (t.n_utt != n_utt || t.pulse_cap != pulse_cap || t.ny_tot != n_samples)
    return wh::fail_msg("wh_synthesis_timebase_read", "n_utt, pulse_cap or n_samples are not the time base's");
  WH_ENTER(ctx);
  WH_CHECK(hipStreamSynchronize((hipStream_t)stream));
  const void* ws = ctx->ws;
  const int B = t.n_utt;
  std::vector<int32_t> count((size_t)B);
  std::vector<int64_t> base((size_t)B + 1);
  WH_CHECK(hipMemcpy(count.data(), t.pc.at(ws), sizeof(int32_t) * B, hipMemcpyDeviceToHost));
  WH_CHECK(hipMemcpy(base.data(), t.pb.at(ws), sizeof(int64_t) * (B + 1), hipMemcpyDeviceToHost));
  for (int u = 0; u < B; ++u) {
    if (count[u] < 0 || count[u] > pulse_cap || base[0] != 0 || base[u + 1] - base[u] != count[u])
      return wh::fail_msg("wh_synthesis_timebase_read", "the pulse counts in the workspace are not a time base's");
    if (h_count) h_count[u] = count[u];
    if (h_base) h_base[u] = base[u];
  }
  if (h_base) h_base[B] = base[B];
  const int64_t total = base[B];
  if (total < 0 || total > (int64_t)B * pulse_cap)
    return wh::fail_msg("wh_synthesis_timebase_read", "the pulse counts in the workspace are not a time base's");
  std::vector<PulseRec> rec((size_t)total);
  if (total > 0) WH_CHECK(hipMemcpy(rec.data(), t.rec.at(ws), sizeof(PulseRec) * (size_t)total, hipMemcpyDeviceToHost));
  for (int64_t g = 0; g < total; ++g) {
    const PulseRec& r = rec[(size_t)g];
    const int64_t f0 = (r.u >= 0 && r.u < B) ? t.f_off[(size_t)r.u] : 0;
    if (h_pidx) h_pidx[g] = r.pidx;
    if (h_shift) h_shift[g] = r.shift;
    if (h_noff) h_noff[g] = r.noff;
    if (h_noise_size) h_noise_size[g] = r.noise_size;
    if (h_vuv) h_vuv[g] = r.vuv;
    if (h_row_lo) h_row_lo[g] = (r.rows & 0xffffffffll) - f0;
    if (h_row_hi) h_row_hi[g] = ((r.rows >> 32) & 0xffffffffll) - f0;
    if (h_weight) h_weight[g] = r.weight;
  }
  if (h_time) {  // p_time lies in pulse slots: pulse i of utterance u at u * pulse_cap + i
    for (int u = 0; u < B; ++u) {
      if (count[u] > 0)
        WH_CHECK(hipMemcpy(h_time + base[u], t.pt.at(ws) + (size_t)u * (size_t)pulse_cap,
                           sizeof(double) * (size_t)count[u], hipMemcpyDeviceToHost));
    }
  }
  if (h_phase && n_samples > 0) WH_CHECK(hipMemcpy(h_phase, t.phase.at(ws), sizeof(double) * (size_t)n_samples, hipMemcpyDeviceToHost));
  if (h_vuv_s && n_samples > 0) WH_CHECK(hipMemcpy(h_vuv_s, t.vuv.at(ws), (size_t)n_samples, hipMemcpyDeviceToHost));
  return 0;
}

// In-place exact sequential cumulative sum of n_seg independent segments of NON-NEGATIVE doubles
// (h_off[n_seg + 1] element offsets into d_data) — the routine behind the phase accumulator, exposed so that its
// bit-for-bit agreement with np.cumsum can be tested directly.
extern "C" int wh_cumsum_exact(wh_ctx* ctx, void* stream, double* d_data, const int64_t* h_off, int n_seg) {
  if (!ctx || !d_data || !h_off || n_seg < 0) return wh::fail_msg("wh_cumsum_exact", "bad argument");
  WH_ENTER(ctx);
  if (n_seg == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  return wh::exact_cumsum_segments(ctx, st, d_data, h_off, n_seg);
}

// Pulse bookkeeping only (no responses): per-utterance pulse count and total noise draws
// sum(max(3, noise_size)) — lets a host draw EXACTLY the reference's number of randn samples.
extern "C" int wh_synthesis_plan(wh_ctx* ctx, void* stream, const wh_batch* b, const double* tp, const double* f0,
                                 const double* vuv, double fs, const int64_t* h_y_off, const double* h_t0,
                                 const double* h_dt, int64_t pulse_cap, int32_t* h_pulse_count,
                                 int64_t* h_noise_total) {
  if (!ctx || !b || !tp || !f0 || !vuv || !h_y_off || !h_t0 || !h_dt || !h_pulse_count || !h_noise_total)
    return wh::fail_msg("wh_synthesis_plan", "null argument");
  WH_ENTER(ctx);
  hipStream_t st = (hipStream_t)stream;
  const int B = b->n_utt;
  std::vector<SynUtt> meta;
  int64_t max_ny = 0;
  if (int rc = wh::fill_syn_meta("wh_synthesis_plan", b, h_y_off, h_t0, h_dt, pulse_cap, nullptr, nullptr, meta, &max_ny)) return rc;
  wh::Carve carve;
  const wh::TimeBaseLayout lay(carve, B, h_y_off[B], pulse_cap, max_ny);
  if (int rc = wh::ws_reserve(ctx, carve)) return rc;
  void* ws = ctx->ws;
  SynUtt* d_meta = nullptr;
  const int64_t* d_pn = lay.pn.at(ws);
  const int32_t* d_pc = lay.pc.at(ws);
  if (int rc = wh::persistent_upload(ctx, st, "syn.meta", meta, &d_meta)) return rc;
  ctx->timebase.valid = false;  // (this call lays the workspace out its own way)
  if (int rc = wh::launch_pulses(ctx, st, B, max_ny, d_meta, tp, f0, vuv, fs, 0.0, h_y_off, ws, lay)) return rc;
  WH_CHECK(hipMemcpyAsync(h_pulse_count, d_pc, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
  WH_CHECK(hipStreamSynchronize(st));
  // total draws = noff[last] + max(3, 0)
  for (int u = 0; u < B; ++u) {
    int64_t total = 0;
    if (h_pulse_count[u] > 0) {
      int64_t last_off = 0;
      WH_CHECK(hipMemcpy(&last_off, d_pn + (int64_t)u * pulse_cap + h_pulse_count[u] - 1, sizeof(int64_t),
                         hipMemcpyDeviceToHost));
      total = last_off + 3;
    }
    h_noise_total[u] = total;
  }
  return 0;
}
