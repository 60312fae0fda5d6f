// Harvest refinement and pruning (see wh_harvest.hip for the stage list): hv_refine_kernel with its DPP row helpers and
// equal-key classes, hv_prune_kernel, and the host builders of the rotation and window tables.  Built unfused.
#include <math.h>
#include <hip/hip_runtime.h>

#include "wh_tid.h"  // (the opaque thread index the old single Harvest unit was compiled with)
#include "wh_device.h"
#include "wh_host.h"
#include "wh_hv_types.h"
#include "wh_math.h"

namespace {
using namespace wh;

// ---- candidate refinement ------------------------------------------------------------------------
// GetRefinedF0 (harvest.py:169-211) for one (frame, candidate), evaluated by a 16-lane DPP row; a wave
// refines four candidates at once.  No FFT: the Blackman-windowed frame and its derivative-windowed twin are
// accumulated directly into the <= 6 harmonic bins the reference reads from its two zero-padded FFTs, and the
// 24 partial sums are reduced inside the row with DPP lane permutes (no LDS, no cross-row traffic).
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  // every control used here reads a live lane of the same row for every lane: no "old" value is needed
  lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, true);
  hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// sum over the RL lanes (a power of two up to 16, aligned) that work on one candidate, result in every lane of the group: xor-1, xor-2
// quad permutes, then the mirror of the half row and, for 16, of the row
template <int RL>
__device__ __forceinline__ double row_sum(double v) {
  static_assert(RL == 16 || RL == 8 || RL == 4 || RL == 2 || RL == 1, "group of a DPP row");
  if (RL >= 2) v += dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
  if (RL >= 4) v += dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
  if (RL >= 8) v += dpp_f64<0x141>(v);   // row_half_mirror
  if (RL == 16) v += dpp_f64<0x140>(v);  // row_mirror
  return v;
}

// TWL: the twiddles come from the workgroup's LDS copy (tw_lds, at a compile-time offset of the dynamic LDS block, so
// that a look-up is one ds_read_b128 whose address register is the running byte offset itself); else from the global
// tables through tw_base.
// WTAB: the Blackman window and its derivative twin depend on the window length alone (the frame time cancels out of the
// reference's window argument, see the tabulated loop) — (w(j), dw(j)) come from a per-call table (win_tab, row hwl at
// offset hwl*(hwl+2), a zero pair at either end) instead of being re-derived per sample by rotation + DPP neighbour exchange.
// Window half length, transform length, harmonic count and the six rounded harmonic bins of a candidate
// (harvest.py:171-174,203), and their packed form: two candidates with the same key have the same two spectra at the
// same bins (hv_refine_kernel's classes), and the key is all the sample loop needs to know about the candidate.
struct RefineGeom {
  int hwl, nfft, nh, bins[6];
};
__device__ __forceinline__ int refine_nfft(int hwl) {
  const int L = 2 * hwl + 1;
  int e = 0;
  while ((1 << e) < L) ++e;
  return 1 << (e + 1);
}
__device__ __forceinline__ RefineGeom refine_geom(double f0c, double fs) {
  RefineGeom g;
  g.hwl = (int)ceil(3 * fs / f0c / 2);
  g.nfft = refine_nfft(g.hwl);
  g.nh = (int)fmin(floor(fs / 2 / f0c), 6.0);
#pragma unroll
  for (int h = 0; h < 6; ++h) g.bins[h] = (int)(f0c * g.nfft / fs * (double)(h + 1) + 0.5);
  return g;
}
// the first bin is within a few units of 1.5 * nfft / hwl (f0c lies in (1.5 fs / hwl, 1.5 fs / (hwl - 1)]): any
// deterministic function of (hwl, nfft) serves as the base it is stored against
__device__ __forceinline__ int refine_bin_base(int hwl, int nfft) { return (int)(1.5f * (float)nfft / (float)hwl) - 1; }
// [0,9) hwl; [9,11) bins[0] - base; [11,14) nh; [14,16), [16,19), [19,22), [22,25), [25,28): bins[h] - (h+1)*bins[0], which is
// within +-(h+2)/2, offset to be non-negative.  -1: a value outside these ranges (not expected; the item is then a class
// of its own and the sample loop derives everything from the candidate).
__device__ __forceinline__ int refine_pack(const RefineGeom& g) {
  const int b0 = g.bins[0] - refine_bin_base(g.hwl, g.nfft);
  const int d1 = g.bins[1] - 2 * g.bins[0] + 1, d2 = g.bins[2] - 3 * g.bins[0] + 3, d3 = g.bins[3] - 4 * g.bins[0] + 3;
  const int d4 = g.bins[4] - 5 * g.bins[0] + 3, d5 = g.bins[5] - 6 * g.bins[0] + 3;
  const bool fits = (unsigned)d1 < 4u && (unsigned)d2 < 8u && (unsigned)d3 < 8u && (unsigned)d4 < 8u && (unsigned)d5 < 8u &&
                    (unsigned)b0 < 4u && (unsigned)g.hwl < 512u && (unsigned)g.nh < 8u;
  return fits ? (g.hwl | (b0 << 9) | (g.nh << 11) | (d1 << 14) | (d2 << 16) | (d3 << 19) | (d4 << 22) | (d5 << 25)) : -1;
}
__device__ __forceinline__ RefineGeom refine_unpack(int key) {
  RefineGeom g;
  g.hwl = key & 511;
  g.nfft = refine_nfft(g.hwl);
  g.nh = (key >> 11) & 7;
  const int b0 = refine_bin_base(g.hwl, g.nfft) + ((key >> 9) & 3);
  g.bins[0] = b0;
  g.bins[1] = 2 * b0 + ((key >> 14) & 3) - 1;
  g.bins[2] = 3 * b0 + ((key >> 16) & 7) - 3;
  g.bins[3] = 4 * b0 + ((key >> 19) & 7) - 3;
  g.bins[4] = 5 * b0 + ((key >> 22) & 7) - 3;
  g.bins[5] = 6 * b0 + ((key >> 25) & 7) - 3;
  return g;
}
__device__ __forceinline__ bool rotation_path_ok(bool wtab, double a0, double a0_frac) {
  return !wtab && a0 > 1.0 && a0_frac > 1e-6 && a0_frac < 1.0 - 1e-6;
}
// RL: lanes per candidate.  The set-up before and the reductions after the sample loop are per wave instruction,
// whatever the number of candidates in the wave, and with the tabulated windows they outweigh the loop (233 + 391
// against 40 instructions per 16 samples): eight lanes per candidate — eight candidates per wave — halve their share
// and drop one of the four reduction steps.  The rotation path needs the 16-lane row rotates.
// `members(eval)`: the caller runs eval(f0c_m, &f0, &score) for every candidate of the frame that shares this one's
// window length and harmonic bins (hv_refine_kernel: the seven overlapped copies of a slowly moving pitch track mostly
// do) — the spectra at the harmonic bins are the same for all of them, only the score looks at the candidate itself.
template <bool TWL, bool WTAB, int RL, class Members>
__device__ __forceinline__ void hv_refine_row(wh::ckp<const double> WH_RESTRICT yl, int64_t ybase, int64_t ylen, double fs,
                                              double t0, double f0c, int pkey, double f0_floor, double f0_ceil,
                                              const double2* __restrict__ tw_base, const char* tw_lds, int tw_n,
                                              wh::ckp<const double2> WH_RESTRICT rot_tab, wh::ckp<const double2> WH_RESTRICT win_tab,
                                              Members members) {
  static_assert(WTAB || RL == 16, "the rotation path exchanges window values with 16-lane row rotates");
  const int l16 = threadIdx.x & (RL - 1);  // lane within the candidate's group
  // pkey >= 0: the candidate's packed geometry (refine_pack), computed when the classes were built
  const RefineGeom geo = pkey >= 0 ? refine_unpack(pkey) : refine_geom(f0c, fs);
  const int hwl = geo.hwl;
  const double hwl_d = (double)hwl;
  const int L = 2 * hwl + 1;
  const double wlit = (2 * hwl_d + 1) / fs;
  const int nfft = geo.nfft;
  const int nh = geo.nh;
  // twiddles exp(-2*pi*i*k/nfft): from the workgroup's LDS copy of the largest table any of its candidates can
  // need (the smaller tables are its subsamples, bit for bit), else from the global table
  const char* tw = TWL ? tw_lds : reinterpret_cast<const char*>(tw_base + nfft);
  const int tw_sh = (TWL ? (__ffs(tw_n) - __ffs(nfft)) : 0) + 4;  // table subsampling, and elements -> bytes
  auto twiddle = [&](int byte_off) -> double2 {
    if constexpr (TWL) {  // the table sits at LDS address 0 (checked by the kernel): the offset IS the address
#if WH_BOUNDS
      if ((unsigned)byte_off + 16u > (unsigned)tw_n * 16u || (byte_off & 15)) wh::oob_report(wh::WH_CK_TWIDDLE, byte_off >> 4, tw_n);
#endif
      typedef double v2d __attribute__((ext_vector_type(2)));
      typedef const v2d __attribute__((address_space(3))) * lds_tw_t;
      const v2d w = *(lds_tw_t)(size_t)(uint32_t)byte_off;
      return make_double2(w.x, w.y);
    } else {
      return *reinterpret_cast<const double2*>(tw + byte_off);
    }
  };
  int bins[6];
#pragma unroll
  for (int h = 0; h < 6; ++h) bins[h] = geo.bins[h];
  const double inv_fs = 1.0 / fs;  // the sample index below is floor(integer + 0.501 +- 1e-12): an ulp cannot move it
  auto idx_raw_at = [&](int j) -> double {
    const double v = (t0 + (double)(j - hwl) * inv_fs) * fs + 0.001;  // "first-aid treatment", harvest.py:178
    return v > 0 ? v + 0.5 : v - 0.5;                               // round_matlab does not truncate (Q1)
  };
  // window phase: 2*common = pi*xw, xw advances by dx per unit step of idx_raw (steps are 1, or 2 where the
  // +-0.5 offset flips sign at negative times)
  const double dx = 2.0 / (fs * wlit);
  double sd1 = 0.0, cd1 = 1.0, sd2 = 0.0, cd2 = 1.0;  // step rotations of the general path (set there)
  double xr[6], xi[6], dr[6], di[6];
#pragma unroll
  for (int h = 0; h < 6; ++h) xr[h] = xi[h] = dr[h] = di[h] = 0.0;
  // one sample of the frame: (s2, c2) = sin/cos(pi*xw(j)); two_next / two_prev: the index step to the neighbour is 2
  auto sample = [&](int j, double ir, double s2, double c2, bool two_next, bool two_prev) {
    const double mj = 0.42 + 0.5 * c2 + 0.08 * (2 * c2 * c2 - 1);  // cos(4c) = 2cos^2(2c) - 1
    double mn = 0.0, mp = 0.0;
    if (j + 1 < L) {
      const double c = two_next ? c2 * cd2 - s2 * sd2 : c2 * cd1 - s2 * sd1;  // cos(2c + step*pi*dx)
      mn = 0.42 + 0.5 * c + 0.08 * (2 * c * c - 1);
    }
    if (j > 0) {
      const double c = two_prev ? c2 * cd2 + s2 * sd2 : c2 * cd1 + s2 * sd1;
      mp = 0.42 + 0.5 * c + 0.08 * (2 * c * c - 1);
    }
    double dw;
    if (j == 0) dw = -mn / 2;
    else if (j == L - 1) dw = mp / 2;
    else dw = -((mn - mj) + (mj - mp)) / 2;
    const double irc = fmax(1.0, fmin((double)ylen, ir)) - 1;
    const double smp = yl[(int64_t)irc - ybase];
    const double a = smp * mj, d = smp * dw;
#pragma unroll
    for (int h = 0; h < 6; ++h) {
      if (h < nh) {
        const double2 w = twiddle(((bins[h] * j) & (nfft - 1)) << tw_sh);
        xr[h] = fma(a, w.x, xr[h]);
        xi[h] = fma(a, w.y, xi[h]);
        dr[h] = fma(d, w.x, dr[h]);
        di[h] = fma(d, w.y, di[h]);
      }
    }
  };
  // The sample index of j is floor(idx_raw_at(j)) = floor(A + j) with A = t0*fs - hwl + 0.501: it steps by exactly one
  // per j as long as A's fraction stays clear of 0 and 1 by more than the rounding of the expression (~1e-9 at 60 s),
  // which the 0.501 guarantees for every decimated rate that is a multiple of 50 Hz; checked here (row-uniform), and
  // a frame that fails the check takes the general path below.
  const double a0 = idx_raw_at(0);
  const double a0_frac = a0 - floor(a0);
  if (WTAB && a0 > 1.0 && a0_frac > 1e-6 && a0_frac < 1.0 - 1e-6) {
    // index_raw(j) = t0*fs + (j - hwl) + 0.501 is never truncated before it enters the window argument
    // (index_raw - 1)/fs - t0 = (j - hwl - 0.499)/fs: the frame time cancels, whatever its position between two
    // samples, and the window pair of row hwl applies as tabulated (only the sample PICK floor(index_raw) depends on
    // the frame, through i_first below).  The loop is the 24 FMAs, the six twiddle gathers and one table read
    // (fetched an iteration ahead).
    // (Advancing some of the six twiddles by a rotation instead of gathering them — 4 more FP64 operations per harmonic and
    // iteration, one LDS gather less — is slower: 2.32 ... 2.48 against 2.28 ms; the loop is bound by VALU issue, not LDS.)
    // The sums run over the sample PAIRS (hwl + m, hwl - m), m = 1..hwl, around the window's centre: the twiddle of
    // bin b at -m is the conjugate of the one at +m, so with a = x*w and d = x*dw
    //   sum_j a_j e^{-i th (j - hwl)} = a_0 + sum_m (a_m + a_-m) cos(th m) - i (a_m - a_-m) sin(th m)
    // — one twiddle gather and four FMAs per harmonic and PAIR instead of per sample (half the gathers, half the FMAs of
    // the loop: 3.19 -> 2.57 ms at config 3).  Referring the phase to the centre multiplies both spectra by the same unit
    // factor e^{i th hwl}: the power |X|^2 and the cross term Im(conj(X) D) that the instantaneous frequency is made of do
    // not see it.  (The window is NOT symmetric — its argument is (j - hwl - 0.499)/fs — so both window pairs are read.)
    // Row hwl of the table has a zero entry in front of and behind its 2*hwl + 1 pairs, and a lane past the window's end
    // (m > hwl in the last iteration) reads those: no predicate and no select inside the loop; the staged signal
    // replicates the utterance's edge samples, so the sample index needs no clamp either.
    const wh::ckp<const double2> wt = win_tab + (hwl * (hwl + 2) + (hwl + 1));  // the centre pair
    int tix[6], tstep[6];  // byte offsets into the twiddle table (see the rotation path below)
    const int tmask = ((nfft - 1) << tw_sh);
#pragma unroll
    for (int h = 0; h < 6; ++h) {
      tix[h] = ((bins[h] * (1 + l16)) & (nfft - 1)) << tw_sh;
      tstep[h] = ((bins[h] * RL) & (nfft - 1)) << tw_sh;
    }
    const int n_it = (hwl + RL - 1) / RL;
    const wh::ckp<const double> yc = yl + ((int)((int64_t)a0 - 1 - ybase) + hwl);  // the centre sample in the staged signal
    if (l16 == 0) {  // the centre sample: cos = 1 for every bin
      const double2 wc = wt[0];
      const double smp = yc[0];
#pragma unroll
      for (int h = 0; h < 6; ++h) {
        xr[h] = smp * wc.x;
        dr[h] = smp * wc.y;
      }
    }
    const int m_end = hwl + 1;  // the zero pair
    int m = 1 + l16;            // (<= hwl + 1: RL <= 4 ... hwl >= RL is not required, the clamp covers it)
    m = m < m_end ? m : m_end;
    double2 cur_p = wt[m], cur_m = wt[-m];
    for (int it = 0; it < n_it; ++it) {
      int mn = m + RL;
      mn = mn < m_end ? mn : m_end;
      const double sp = yc[m], sm = yc[-m];
      const double ap = sp * cur_p.x, am = sm * cur_m.x, dp = sp * cur_p.y, dm = sm * cur_m.y;
      const double ea = ap + am, oa = ap - am, ed = dp + dm, od = dp - dm;
      double2 wv[6];  // all six gathers in flight before the first FMA needs one
#pragma unroll
      for (int h = 0; h < 6; ++h) wv[h] = twiddle(tix[h]);
      cur_p = wt[mn];  // the next iteration's window pairs, in flight under this one's FMAs
      cur_m = wt[-mn];
      // (without the fence the compiler folds the loop-carried pair into "load the current pair at the top of the
      // iteration", and every iteration waits for a global round trip)
      asm volatile("" ::: "memory");
#pragma unroll
      for (int h = 0; h < 6; ++h) {
        const double2 w = wv[h];
        xr[h] = fma(ea, w.x, xr[h]);
        xi[h] = fma(oa, w.y, xi[h]);
        dr[h] = fma(ed, w.x, dr[h]);
        di[h] = fma(od, w.y, di[h]);
        tix[h] = (tix[h] + tstep[h]) & tmask;
      }
      m = mn;
    }
  } else if (rotation_path_ok(WTAB, a0, a0_frac)) {
    if constexpr (!WTAB) {
    // Every index of the frame is positive (all frames but the first few of an utterance): idx_raw, and with it the
    // window phase xw, is linear in j, so this lane's samples j = l16 + 16 i are a fixed rotation of 16*pi*dx apart —
    // one sincospi to start, a 6-flop rotation per sample after that (<= 24 steps: error growth ~1e-15; the rotation
    // constants of every window length come from a small per-call table).
    // The derivative window needs the Blackman values of samples j-1 and j+1: those are what the neighbouring lanes
    // of the row hold in the same iteration (lane 0's left neighbour is lane 15's value of the previous iteration,
    // lane 15's right neighbour lane 0's value of the next one, which is therefore computed one iteration ahead), so
    // they are fetched with two DPP row rotates each instead of being recomputed (2 x (rotation + Blackman) = 26
    // FP64 operations per sample in a kernel that is VALU-bound).  All 16 lanes of a row run the same number of
    // iterations (validity is a predicate), which keeps every source lane of the rotates alive.  The twiddle offset
    // (bin*j mod nfft) advances by a constant per iteration: an add and a mask instead of a 32-bit multiply.
    // (A lane-contiguous layout, j = l*nb + i, needs no cross-lane traffic at all but multiplies the lane stride of
    // the twiddle gathers by nb: their LDS bank conflicts made it 20 % slower, measured.)
    const double2 rot = rot_tab[hwl];  // (sin, cos)(16*pi*dx)
    const double s16 = rot.x, c16 = rot.y;
    double s2, c2;
    {
      const double ir0 = idx_raw_at(l16);
      sincospi(2 * ((ir0 - 1) / fs - t0) / wlit, &s2, &c2);
    }
    auto blackman = [](double c) { return 0.42 + 0.5 * c + 0.08 * (2 * c * c - 1); };  // cos(4c) = 2cos^2(2c) - 1
    // twiddle look-ups as byte offsets into the table in use, already scaled by its subsampling shift: the
    // offset of harmonic h advances by (16*bin_h mod nfft) << shift per iteration.  All six harmonics are accumulated
    // whatever nh is (the surplus ones, for candidates above fs/12, are simply not read afterwards): no per-harmonic
    // predication inside the loop.
    int tix[6], tstep[6];
    const int tmask = ((nfft - 1) << tw_sh);
#pragma unroll
    for (int h = 0; h < 6; ++h) {
      tix[h] = ((bins[h] * l16) & (nfft - 1)) << tw_sh;
      tstep[h] = ((bins[h] * 16) & (nfft - 1)) << tw_sh;
    }
    double m_prev = 0.0, m_cur = blackman(c2);
    const int n_it = (L + 15) >> 4;
    int j = l16;
    // staged-signal index of sample j: clamp(floor(A) + j, 1, ylen) - 1 - ybase, carried as an int
    const int64_t i_first = (int64_t)a0;
    const int i_lo = (int)(0 - ybase), i_hi = (int)(ylen - 1 - ybase);
    int si = (int)(i_first - 1 - ybase) + l16;
    for (int it = 0; it < n_it; ++it, j += 16) {
      const double cn = c2 * c16 - s2 * s16;  // phase of sample j + 16
      s2 = s2 * c16 + c2 * s16;
      c2 = cn;
      const double m_next = blackman(c2);
      const double right = dpp_f64<0x12F>(m_cur), right_wrap = dpp_f64<0x12F>(m_next);  // lane l <- lane l+1 (15 <- 0)
      const double left = dpp_f64<0x121>(m_cur), left_wrap = dpp_f64<0x121>(m_prev);     // lane l <- lane l-1 (0 <- 15)
      const double mn = j + 1 < L ? (l16 == 15 ? right_wrap : right) : 0.0;
      const double mp = j > 0 ? (l16 == 0 ? left_wrap : left) : 0.0;
      const double mj = m_cur;
      double dw;
      if (j == 0) dw = -mn / 2;
      else if (j == L - 1) dw = mp / 2;
      else dw = -((mn - mj) + (mj - mp)) / 2;
      double smp = 0.0;
      if (j < L) smp = yl[si < i_lo ? i_lo : (si > i_hi ? i_hi : si)];
      si += 16;
      const double a = smp * mj, d = smp * dw;
#pragma unroll
      for (int h = 0; h < 6; ++h) {
        const double2 w = twiddle(tix[h]);
        xr[h] = fma(a, w.x, xr[h]);
        xi[h] = fma(a, w.y, xi[h]);
        dr[h] = fma(d, w.x, dr[h]);
        di[h] = fma(d, w.y, di[h]);
        tix[h] = (tix[h] + tstep[h]) & tmask;
      }
      m_prev = m_cur;
      m_cur = m_next;
    }
    }
  } else {
    sincospi(dx, &sd1, &cd1);
    sincospi(2 * dx, &sd2, &cd2);
    for (int j = l16; j < L; j += RL) {
      const double ir = idx_raw_at(j);
      const double xw = 2 * ((ir - 1) / fs - t0) / wlit;
      double s2, c2;
      sincospi(xw, &s2, &c2);  // sin/cos(2*common)
      const bool two_next = (j + 1 < L) && (idx_raw_at(j + 1) - ir > 1.5);
      const bool two_prev = (j > 0) && (ir - idx_raw_at(j - 1) > 1.5);
      sample(j, ir, s2, c2, two_next, two_prev);
    }
  }
  // The four sums of every harmonic go round the row; lane h then evaluates harmonic h alone — instantaneous
  // frequency, amplitude, deviation: five FP64 divides and a square root, ~85 instructions that all sixteen lanes used
  // to repeat for each of the six harmonics — and three more row sums collect the totals.  (Folding the 24 partial sums
  // once by DPP and finishing through an LDS scratch needs a third of the instructions but its 24 KB cost a workgroup
  // per CU: 9.5 against 8.0 ms, measured.)
  constexpr int P = (6 + RL - 1) / RL;  // harmonics per lane: lane l takes l, l + RL, ...
  double sa[P], sb[P], sc_[P], sd[P];
  int my_bin[P];
#pragma unroll
  for (int q = 0; q < P; ++q) {
    sa[q] = sb[q] = sc_[q] = sd[q] = 0.0;
    my_bin[q] = 0;
  }
#pragma unroll
  for (int h = 0; h < 6; ++h) {
    const double a = row_sum<RL>(xr[h]), b = row_sum<RL>(xi[h]), c = row_sum<RL>(dr[h]), d = row_sum<RL>(di[h]);
    if (l16 == h % RL) {
      sa[h / RL] = a;
      sb[h / RL] = b;
      sc_[h / RL] = c;
      sd[h / RL] = d;
      my_bin[h / RL] = bins[h];
    }
  }
  // per harmonic of this lane: instantaneous frequency and amplitude (harvest.py:193-203) — functions of the spectra
  // alone; numerator / denominator / variation are summed per candidate below, over ITS harmonics
  double inst_q[P], amp_q[P];
#pragma unroll
  for (int q = 0; q < P; ++q) {
    const double p = sa[q] * sa[q] + sb[q] * sb[q];
    const double nm = sa[q] * sd[q] - sb[q] * sc_[q];
    // bin / nfft is exact (power of two), and so is the halving
    // (the quotients of this epilogue — seventeen per lane — go through wh::fdiv: they were two thirds of its instructions)
    inst_q[q] = ((double)my_bin[q] * (1.0 / (double)nfft) + wh::fdiv(wh::fdiv(nm, p) * 0.5, M_PI)) * fs;
    amp_q[q] = sqrt(p);
  }
  // numerator and denominator run over the harmonics below nh — the same for every member (nh is part of the class key)
  double t_num = 0.0, t_den = 0.0, a_q[P];
#pragma unroll
  for (int q = 0; q < P; ++q) {
    const int h = l16 + q * RL;
    a_q[q] = wh::fdiv(inst_q[q], (double)(h + 1));
    if (h < nh) {
      t_num += amp_q[q] * inst_q[q];
      t_den += amp_q[q] * (double)(h + 1);
    }
  }
  const double num = row_sum<RL>(t_num), den = row_sum<RL>(t_den);
  const double rf_all = wh::fdiv(num, den);
  // (scoring four members at a time, one per lane, was measured and is no faster: 3.51 against 3.53 ms)
  members([&](double f0m, double* out_f0, double* out_sc) {
    double t_var = 0.0;
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const int h = l16 + q * RL;
      if (h < nh) t_var += fabs(wh::fdiv(a_q[q] - f0m, f0m));
    }
    const double var = row_sum<RL>(t_var);
    double rf = rf_all;
    double sc = wh::fdiv(1.0, 0.000000000001 + wh::fdiv(var, (double)nh));
    if (rf < f0_floor || rf > f0_ceil || sc < 2.5) {
      rf = 0.0;
      sc = 0.0;
    }
    *out_f0 = rf;
    *out_sc = sc;
  });
}

constexpr int kRefineMinWaves = 3;  // waves per SIMD the tabulated variant is compiled for (2: 5.07 ms against 4.09 at config 3)
// lanes per candidate of the tabulated variant (round 6, 512 x 10 s: 8 lanes 22.1 ms, 4: 17.7, 2: 16.5, 1: 18.6; 64 x 10 s:
// 4: 2.30, 2: 2.15, 1: 2.49)
constexpr int kRefineRowLanes = 2;
// its frames per workgroup (round 6, with two lanes per candidate: 32 frames 16.36 ms against 16.50 for 24 at 512 x 10 s;
// round 4, four lanes: the list building is per block and a wave pass takes 16 classes whatever it holds; config 3:
// 16 frames 3.81 ms, 24: 3.34, 32: 3.37, 48: 4.79 — 52.3 against 59.7 ms at 1024 utterances)
constexpr int kRefineTabFrames = 32;
constexpr int kRefineItemCap = 1344;  // work-list slots in LDS; a block whose frames hold more takes them in several rounds of whole frames
// lanes per candidate and frames per workgroup of the two refinement variants
constexpr int refine_lanes(bool wtab) { return wtab ? kRefineRowLanes : 16; }
constexpr int refine_frames(bool wtab) { return wtab ? kRefineTabFrames : 4; }
constexpr int refine_item_cap(bool wtab) { return refine_frames(wtab) * kRows < kRefineItemCap ? refine_frames(wtab) * kRows : kRefineItemCap; }

template <bool TWL, bool WTAB>
__global__ __launch_bounds__(256, WTAB ? kRefineMinWaves : 1) void hv_refine_kernel(const HvUtt* __restrict__ meta, const double* __restrict__ y,
                                                        const double* __restrict__ dc, const int32_t* __restrict__ dcount,
                                                        double fs, double f0_floor, double f0_ceil, int hmax, int seglen,
                                                        const double2* __restrict__ tw_base, int tw_n,
                                                        const double2* __restrict__ rot_tab,
                                                        const double2* __restrict__ win_tab,
                                                        double* __restrict__ rf0, double* __restrict__ rsc,
                                                        int64_t* __restrict__ lst, int item_cap) {
  // All of the kernel's LDS is the dynamic block, so that it starts at LDS address 0 and the twiddle table's byte
  // offsets are LDS addresses as they stand (hv_refine_lds_bytes mirrors this layout).
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int RL = refine_lanes(WTAB);
  constexpr int kFramesPerBlock = refine_frames(WTAB);
  constexpr int kBuckets = 64;
  const HvUtt m = meta[blockIdx.y];
  const int64_t f_first = (int64_t)blockIdx.x * kFramesPerBlock;
  if (f_first >= m.nf1) return;
  // LDS: the twiddle table of the largest transform length first (tw_n points; TWL false: none, the global tables are
  // read) — every sample of every refinement gathers 6 twiddles at scattered indices, LDS serves those, the L1 does
  // not — then the staged signal around the block's frames.
  // (wh::ckp<T>: T* in every shipped build, range-checked in the bounds build — wh_device.h)
  const wh::ckp<double2> twl = wh::ck_make(reinterpret_cast<double2*>(smem), TWL ? tw_n : 0, wh::WH_CK_TWIDDLE);
  if (TWL && (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem != 0u) __builtin_trap();
  constexpr int kItems = refine_item_cap(WTAB);                // (>= kRows: a single frame always fits)
  const int seg_pad = (seglen + 1) & ~1;
  double* yl_raw = reinterpret_cast<double*>(smem + (TWL ? sizeof(double2) * (size_t)tw_n : 0));
  const wh::ckp<double> yl = wh::ck_make(yl_raw, seg_pad, wh::WH_CK_LDS_MAIN);
  const wh::ckp<double> cl_val = wh::ck_make(yl_raw + seg_pad, kItems, wh::WH_CK_LDS_AUX);  // kItems
  int* ints_raw = reinterpret_cast<int*>(yl_raw + seg_pad + kItems);
  const wh::ckp<int> cl_meta = wh::ck_make(ints_raw, kItems, wh::WH_CK_LDS_OTHER);               // kItems
  const wh::ckp<int> order = wh::ck_make(ints_raw + kItems, kItems, wh::WH_CK_LDS_OTHER);        // kItems
  const wh::ckp<int> key_s = wh::ck_make(ints_raw + 2 * kItems, kItems, wh::WH_CK_LDS_OTHER);    // kItems: packed geometry of an item (refine_pack)
  const wh::ckp<int> bucket = wh::ck_make(ints_raw + 3 * kItems, kBuckets + 1, wh::WH_CK_LDS_SCRATCH);  // kBuckets (+ the class count)
  int& cl_n = bucket[kBuckets];
  const wh::ckp<uint32_t> nzmask = wh::ck_make(reinterpret_cast<uint32_t*>(ints_raw + 3 * kItems + kBuckets + 1), kFramesPerBlock * 4,
                                               wh::WH_CK_LDS_SCRATCH);  // [kFramesPerBlock][4]: rows of a frame that hold a candidate
  const wh::ckp<int> foff = wh::ck_make(ints_raw + 3 * kItems + kBuckets + 1 + kFramesPerBlock * 4, kFramesPerBlock + 1,
                                        wh::WH_CK_LDS_SCRATCH);  // [kFramesPerBlock + 1]: first list slot of a frame
  for (int i = threadIdx.x; i < kFramesPerBlock * 4; i += 256) nzmask[i] = 0;
  if (TWL)
    for (int i = threadIdx.x; i < tw_n; i += 256) twl[i] = tw_base[tw_n + i];
  const int64_t centre0 = (int64_t)floor(((double)f_first * 1 / 1000) * fs + 0.5);
  // (may be negative: the staged signal replicates the utterance's first and last sample beyond its ends, which is what
  // the reference's index clamp reads there, harvest.py:179)
  const int64_t ybase = centre0 - hmax - 3;
  const wh::ckp<const double> yu = wh::ck_make(y + m.y_off, m.ylen, wh::WH_CK_WAVEFORM);
  // the utterance's share of the global arrays: candidate slots in, result pool and list heads out, the window tables
  const wh::ckp<const double> dc_u = wh::ck_make(dc + m.f1_off * kMaxC, m.nf1 * kMaxC, wh::WH_CK_IN) - m.f1_off * kMaxC;
  const wh::ckp<double> rf0_u = wh::ck_make(rf0 + m.f1_off * kRows, m.nf1 * kRows, wh::WH_CK_OUT) - m.f1_off * kRows;
  const wh::ckp<double> rsc_u = wh::ck_make(rsc + m.f1_off * kRows, m.nf1 * kRows, wh::WH_CK_OUT) - m.f1_off * kRows;
  const wh::ckp<int64_t> lst_u = wh::ck_make(lst + m.f1_off, m.nf1, wh::WH_CK_OUT) - m.f1_off;
  const wh::ckp<const double2> win_ck = wh::ck_make(win_tab, win_tab ? (long long)(hmax + 2) * (hmax + 4) : 0, wh::WH_CK_TABLE);
  const wh::ckp<const double2> rot_ck = wh::ck_make(rot_tab, hmax + 2, wh::WH_CK_TABLE);
  for (int i = threadIdx.x; i < seglen; i += 256) {
    const int64_t g = ybase + i;
    yl[i] = yu[g < 0 ? 0 : (g > m.ylen - 1 ? m.ylen - 1 : g)];
  }
  if (threadIdx.x == 0) cl_n = 0;
  __syncthreads();
  // gather the overlapped candidates of the block's frames (+-3 frames, harvest.py:114-125) and compact the
  // non-zero ones into a work list.  The reference's [frame][105] candidate map is ~17 % occupied; what the later stages
  // need from it is the ORDER of a frame's candidates (first-index / last-index tie rules), not the row numbers, so the
  // results are stored as per-frame lists in row order: the block's frames share one contiguous pool region (at the place
  // the dense rows of its first frame would start), lst[frame] = (first pool slot << 8) | count.
  // A thread's (up to 7) candidate slots are fetched in one round of unconditional loads from clamped source frames —
  // hv_detect writes every one of a frame's kMaxC slots, zeros past its count, so the count itself is not needed; as
  // `if (in range && c < dcount[src]) cand = dc[..]` every slot was two dependent round trips, one slot after the other.
  constexpr int kGather = (kFramesPerBlock * kRows + 255) / 256;
  double cv[kGather];
#pragma unroll
  for (int it = 0; it < kGather; ++it) {
    const int q = threadIdx.x + it * 256;
    const int qc = q < kFramesPerBlock * kRows ? q : 0;
    const int fl = qc / kRows, e = qc % kRows;
    int64_t src = f_first + fl + (e / kMaxC - 3);
    src = src < 0 ? 0 : (src > m.nf1 - 1 ? m.nf1 - 1 : src);
    cv[it] = dc_u[(m.f1_off + src) * kMaxC + e % kMaxC];
  }
  // The work list is written in LIST-SLOT order (the rank of a row among its frame's rows: the order the results are
  // stored in), so a frame's items are contiguous and an item's index is its result slot: a first pass marks the rows
  // that hold a candidate, a second, behind the per-frame offsets, places them.
  bool live_q[kGather];
#pragma unroll
  for (int it = 0; it < kGather; ++it) {
    const int q = threadIdx.x + it * 256;
    live_q[it] = false;
    if (q >= kFramesPerBlock * kRows) continue;
    const int fl = q / kRows, e = q % kRows;
    const int64_t f = f_first + fl;
    if (f >= m.nf1) continue;
    const int64_t src = f + (e / kMaxC - 3);
    double cand = (src >= 0 && src < m.nf1) ? cv[it] : 0.0;
    if (e == 0 && f < 3) cand = dc_u[(m.f1_off + f) * kMaxC + 6];  // stray seeding of row 0 (harvest.py:119)
    cv[it] = cand;
    if (cand != 0.0 && ceil(3 * fs / cand / 2) <= (double)hmax) {
      live_q[it] = true;
      atomicOr(&nzmask[fl * 4 + (e >> 5)], 1u << (e & 31));
    }
  }
  __syncthreads();
  const int64_t pool_base = (m.f1_off + f_first) * kRows;
  static_assert(kFramesPerBlock <= 64, "one lane per frame below");
  // the work-list encoding: a 5-bit frame index and an 11-bit successor link in cl_meta, a 6-bit sort key
  static_assert(kFramesPerBlock <= 32 && kItems < 2048 && kBuckets <= 64, "field widths of the hv_refine work list");
  if (threadIdx.x < 64) {  // per-frame counts -> list offsets: one lane per frame, a wave scan (one lane walking the frames
                           // was a chain of dependent LDS round trips with the other 255 threads at the barrier)
    const int fl = threadIdx.x;
    const int c = fl < kFramesPerBlock
                      ? __popc(nzmask[fl * 4]) + __popc(nzmask[fl * 4 + 1]) + __popc(nzmask[fl * 4 + 2]) + __popc(nzmask[fl * 4 + 3])
                      : 0;
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (fl >= o) incl += up;
    }
    if (fl < kFramesPerBlock) {
      foff[fl] = incl - c;
      if (f_first + fl < m.nf1) lst_u[m.f1_off + f_first + fl] = ((pool_base + (incl - c)) << 8) | (int64_t)c;
    }
    if (fl == 63) foff[kFramesPerBlock] = incl;
  }
  __syncthreads();
  // Rounds of whole frames whose candidates fit the work list (kItems slots; the 32 frames of a block hold ~400 candidates
  // on speech-like input, 3360 at most): normally one.  The first round is placed from the registers of the gather above
  // (which die here: inside the loop they would stay alive across the refinement passes), a further round fetches its
  // rows again.
  auto round_end = [&](int fa) {
    if (foff[kFramesPerBlock] - foff[fa] <= item_cap) return (int)kFramesPerBlock;  // the usual case: all that is left
    int fb = fa + 1;  // (walking the frames costs a dependent LDS read each, on every thread)
    while (fb < kFramesPerBlock && foff[fb + 1] - foff[fa] <= item_cap) ++fb;  // (item_cap <= kItems: the LDS slots)
    return fb;
  };
  auto slot_of = [&](int fl, int e, int s0) {
    const wh::ckp<const uint32_t> mw = nzmask + fl * 4;
    int slot = foff[fl] - s0 + __popc(mw[e >> 5] & ((1u << (e & 31)) - 1u));  // rank of row e among the round's rows
    for (int w = 0; w < (e >> 5); ++w) slot += __popc(mw[w]);
    return slot;
  };
  int fa = 0, fb = round_end(0);
#pragma unroll
  for (int it = 0; it < kGather; ++it) {
    if (!live_q[it]) continue;
    const int q = threadIdx.x + it * 256;
    const int fl = q / kRows, e = q % kRows;
    if (fl >= fb) continue;
    const int slot = slot_of(fl, e, 0);
    cl_val[slot] = cv[it];
    cl_meta[slot] = fl;
  }
  while (true) {
    const int s0 = foff[fa];
    const int n_items = foff[fb] - s0;
    // EQUAL-KEY CLASSES.  What a refinement costs — the two windowed spectra at the harmonic bins — depends on the
    // candidate only through its window half length and its six rounded bins (harvest.py:171-174,203): the seven overlapped
    // copies of a slowly moving pitch track that meet in one frame mostly share them (measured on the benchmark input: 178 k
    // work items per 10 s, 121 k distinct keys; the reference's own test recording: 83 k / 66 k).  One item of a class does the
    // sums; every member gets its own score from them (it is the score that looks at the candidate's value,
    // harvest.py:205-206) — same arithmetic, same results, a third less work.
    // cl_meta fields: [0,5) frame; [5,11) iteration count (the counting sort's key); [17,28) successor in the class + 1,
    // bit 28: not the class's first item.  key_s: the packed geometry, which IS the class key.
    __syncthreads();
    // the keys, one thread per PLACED item (every lane busy; inside the gather loop above the same arithmetic ran seven
    // times per wave with a tenth of the lanes)
    for (int i = threadIdx.x; i < n_items; i += 256) {
      const RefineGeom g = refine_geom(cl_val[i], fs);
      const int key = refine_pack(g);
      // iteration count of the sample loop: the counting sort's key
      int skey = WTAB ? (g.hwl + RL - 1) / RL : (2 * g.hwl + 1 + RL - 1) / RL;
      skey = skey > kBuckets - 1 ? kBuckets - 1 : skey;
      key_s[i] = key >= 0 ? key : (int)(0x80000000u | (unsigned)i);  // (unpackable: a class of its own)
      cl_meta[i] = cl_meta[i] | (skey << 5);
    }
    __syncthreads();
    if (threadIdx.x < kBuckets) bucket[threadIdx.x] = 0;  // (for the counting sort below: one barrier less)
    constexpr int kClassScan = (kItems + 255) / 256;
    int link[kClassScan];  // per item of this thread: (successor + 1) | not-first flag << 11
  #pragma unroll
    for (int r = 0; r < kClassScan; ++r) {
      const int i = threadIdx.x + r * 256;
      link[r] = 0;
      if (i < n_items) {
        const int ka = key_s[i], fl = cl_meta[i] & 31;
        const int lo = foff[fl] - s0, hi = foff[fl + 1] - s0;  // the frame's items
        bool has_pred = false;
        int succ = 0;
        for (int j = lo; j < i; ++j) has_pred = has_pred || key_s[j] == ka;
        for (int j = hi - 1; j > i; --j) succ = key_s[j] == ka ? j + 1 : succ;
        link[r] = succ | (has_pred ? 1 << 11 : 0);
      }
    }
    __syncthreads();
  #pragma unroll
    for (int r = 0; r < kClassScan; ++r) {
      const int i = threadIdx.x + r * 256;
      if (i < n_items) cl_meta[i] = (cl_meta[i] & 0x7ff) | (link[r] << 17);
    }
    // A wave refines 64 / RL classes at once, one per group of RL lanes, and runs as long as its longest one: the
    // window length goes with 1/f0 (31 ... 340 samples at 8 kHz), and a frame's candidates are typically an f0 with its
    // octave neighbours.  Counting sort of the classes' first items by iteration count, so that the groups of a wave
    // (consecutive entries) carry windows of the same length class.
    {
      // (the buckets were zeroed in front of the class scan's barrier; a thread counts the items whose links it wrote)
      for (int i = threadIdx.x; i < n_items; i += 256)
        if (!(cl_meta[i] >> 28 & 1)) atomicAdd(&bucket[(cl_meta[i] >> 5) & 63], 1);  // the classes' first items
      __syncthreads();
      static_assert(kBuckets == 64, "one lane per bucket");
      if (threadIdx.x < 64) {  // exclusive scan of the counts, longest first (the long items start the block's schedule)
        const int k = kBuckets - 1 - threadIdx.x;
        const int c = bucket[k];
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int up = __shfl_up(incl, o, 64);
          if ((int)threadIdx.x >= o) incl += up;
        }
        bucket[k] = incl - c;
        if (threadIdx.x == 63) cl_n = incl;  // classes
      }
      __syncthreads();
        const int n_lead = cl_n;
      for (int i = threadIdx.x; i < n_items; i += 256)
        if (!(cl_meta[i] >> 28 & 1)) order[atomicAdd(&bucket[(cl_meta[i] >> 5) & 63], 1)] = i;
      __syncthreads();
      for (int it = threadIdx.x / RL; it < n_lead; it += 256 / RL) {
        const int src = order[it];
        const int64_t f = f_first + (cl_meta[src] & 31);
        hv_refine_row<TWL, WTAB, RL>(
            yl, ybase, m.ylen, fs, (double)f * 1 / 1000, cl_val[src], key_s[src], f0_floor, f0_ceil, tw_base, smem, tw_n, rot_ck, win_ck,
            [&](auto eval) {
              int p = src;
              while (true) {
                double r0, r1;
                eval(cl_val[p], &r0, &r1);
                if ((threadIdx.x & (RL - 1)) == 0) {
                  rf0_u[pool_base + s0 + p] = r0;  // (an item's index is its slot in the round's part of the block's pool region)
                  rsc_u[pool_base + s0 + p] = r1;
                }
                const int nx = (cl_meta[p] >> 17) & 0x7ff;
                if (!nx) break;
                p = nx - 1;
              }
            });
      }
    }
    fa = fb;
    if (fa >= kFramesPerBlock) break;
    fb = round_end(fa);
    __syncthreads();  // (this round's lists have been consumed)
    for (int q = threadIdx.x; q < kFramesPerBlock * kRows; q += 256) {  // the next round's rows, fetched again (rare path)
      const int fl = q / kRows, e = q % kRows;
      if (fl < fa || fl >= fb || !((nzmask[fl * 4 + (e >> 5)] >> (e & 31)) & 1u)) continue;
      const int64_t f = f_first + fl;
      const int64_t src = f + (e / kMaxC - 3);
      const double cand = (e == 0 && f < 3) ? dc_u[(m.f1_off + f) * kMaxC + 6] : dc_u[(m.f1_off + src) * kMaxC + e % kMaxC];
      const int slot = slot_of(fl, e, foff[fa]);
      cl_val[slot] = cand;
      cl_meta[slot] = fl;
    }
  }
}

// RemoveUnreliableCandidates (harvest.py:215-234): a candidate survives if some candidate of frame j-1
// or j+1 lies within 5 %.  A workgroup takes kPruneFrames consecutive frames: the candidate lists of those frames and
// their two outer neighbours are fetched once (half a wave per frame), their non-zero entries compacted into LDS (ballot
// ranks), then every list entry is tested against the non-zero entries of its two neighbours.  (One 128-thread workgroup
// per frame — 640 k of them for 64 x 10 s — was bound by the rate at which workgroups can be launched, and read every
// frame three times.)
constexpr int kPruneFrames = 16;

// The result is a 128-bit keep mask per frame (bit k: entry k of the frame's list survives, i.e. is non-zero and passed
// the test): the contour kernels read the refined lists through it (wh_hv_contour.hip), which spares this pass the
// score array and pruned copies.
__global__ __launch_bounds__(256) void hv_prune_kernel(const HvUtt* __restrict__ meta, const double* __restrict__ rf0,
                                                       const int64_t* __restrict__ lst, uint32_t* __restrict__ keep) {
  constexpr int kRowPad = 128;                              // a row of nzl: the non-zero entries, then +inf
  __shared__ double nzl[kPruneFrames + 2][kRowPad];         // non-zero candidates of frames f_first-1 .. f_first+16
  __shared__ int ln[kPruneFrames + 2];
  static_assert(kRows <= kRowPad, "row padding");
  const HvUtt m = meta[blockIdx.y];
  const int64_t f_first = (int64_t)blockIdx.x * kPruneFrames;
  if (f_first >= m.nf1) return;
  // HALF a wave per frame: a list holds ~17 entries on speech-like input (105 at most), so with a whole wave per frame
  // three lanes in four idled through the neighbour loops; a half-wave takes entries l32 + 32 * pass, and a pass that
  // neither of the wave's two frames reaches is skipped.  The eight half-waves take rows hw, hw + 8, hw + 16 of the 18.
  const int lane = threadIdx.x & 63, half = lane >> 5, l32 = lane & 31;
  const int hw = (threadIdx.x >> 6) * 2 + half;
  constexpr int kPer = (kPruneFrames + 2 + 7) / 8;
  constexpr int kPass = (kRows + 31) / 32;
  for (int i = threadIdx.x; i < (kPruneFrames + 2) * kRowPad; i += 256) (&nzl[0][0])[i] = INFINITY;
  // the list heads first, then every list — independent loads in flight before the first ballot needs one.  Entry k of
  // a list sits on lane k & 31 of its half (pass k >> 5) and stays there: the half-wave that fetched a frame also tests it.
  int64_t ent[kPer];
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int fr = hw + 8 * i;
    const int64_t f = f_first - 1 + fr;
    const bool ok = fr < kPruneFrames + 2 && f >= 0 && f < m.nf1;
    ent[i] = ok ? lst[m.f1_off + f] : 0;
  }
  double val[kPer][kPass];
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const double* src = rf0 + (ent[i] >> 8);
    const int n = (int)(ent[i] & 255);
#pragma unroll
    for (int pass = 0; pass < kPass; ++pass) {
      const int e = l32 + 32 * pass;
      val[i][pass] = e < n ? src[e] : 0.0;
    }
  }
  __syncthreads();  // (the +inf fill is complete)
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int fr = hw + 8 * i;
    const bool row = fr < kPruneFrames + 2;
    int n = 0;
#pragma unroll
    for (int pass = 0; pass < kPass; ++pass) {
      const double a = val[i][pass];
      const unsigned long long nz64 = __ballot(a != 0.0);  // zeros can never be the nearest candidate
      const uint32_t nz = (uint32_t)(nz64 >> (32 * half));
      if (row && a != 0.0) nzl[fr][n + __popc(nz & ((1u << l32) - 1u))] = a;
      n += __popc(nz);
    }
    if (row && l32 == 0) ln[fr] = n;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int fr = hw + 8 * i;
    const int64_t f = f_first - 1 + fr;
    const bool valid = fr >= 1 && fr <= kPruneFrames && f < m.nf1;  // rows 0 and 17 are neighbours only
    const bool inner = valid && f >= 1 && f <= m.nf1 - 2;
    const int n_prev = valid ? ln[fr - 1] : 0, n_next = valid ? ln[fr + 1] : 0;
    const double* nb_prev = nzl[valid ? fr - 1 : 0];
    const double* nb_next = nzl[valid ? fr + 1 : 0];
    // loop bounds and the pass count of the wave: the larger of its two halves' (a half that reads past its own row's
    // entries reads +inf, which no minimum takes)
    const int cnt = valid ? (int)(ent[i] & 255) : 0;
    const int t_next = max(__builtin_amdgcn_readlane(n_next, 0), __builtin_amdgcn_readlane(n_next, 32));
    const int t_prev = max(__builtin_amdgcn_readlane(n_prev, 0), __builtin_amdgcn_readlane(n_prev, 32));
    const int t_cnt = max(__builtin_amdgcn_readlane(cnt, 0), __builtin_amdgcn_readlane(cnt, 32));
#pragma unroll
    for (int pass = 0; pass < kPass; ++pass) {
      double v = val[i][pass];
      if (32 * pass < t_cnt) {
        if (inner && v != 0.0) {
          double e1 = 1.0, e2 = 1.0;  // SelectBestF0 with allowed_range = 1 (a zero candidate gives exactly 1)
          // min_k |v - nb_k| / v == (min_k |v - nb_k|) / v bit for bit (division by v > 0 is monotone): one divide per
          // neighbour frame instead of one per neighbour candidate
          double d1 = INFINITY, d2 = INFINITY;
          for (int k = 0; k < t_next; ++k) d1 = fmin(d1, fabs(v - nb_next[k]));
          for (int k = 0; k < t_prev; ++k) d2 = fmin(d2, fabs(v - nb_prev[k]));
          if (n_next > 0) e1 = fmin(e1, d1 / v);
          if (n_prev > 0) e2 = fmin(e2, d2 / v);
          if (fmin(e1, e2) > 0.05) v = 0.0;
        }
      }
      const unsigned long long kept = __ballot(v != 0.0);
      if (valid && l32 == 0) keep[(m.f1_off + f) * 4 + pass] = (uint32_t)(kept >> (32 * half));
    }
  }
}

// 16-sample rotation (sin, cos)(16*pi*dx) of the window phase for every half length (hv_refine_row, rotation path)
int upload_rotation_table(wh_ctx* ctx, hipStream_t st, double fs_d, int hmax, double2** d_rot) {
  std::vector<double2> rot(hmax + 2);
  for (int h = 0; h <= hmax + 1; ++h) {
    const double wlit = (2 * (double)h + 1) / fs_d;
    const double dx = 2.0 / (fs_d * wlit);
    rot[h] = make_double2(sin(M_PI * (16 * dx)), cos(M_PI * (16 * dx)));
  }
  return persistent_upload(ctx, st, "hv.rot", rot, d_rot);
}

// (w(j), dw(j)) of every window length, row hwl at offset hwl*(hwl+2) between two zero pairs (hv_refine_row, WTAB).  Built
// once per (rate, longest window) and kept on the device.
int window_table(wh_ctx* ctx, double fs_d, int hmax, const double2** d_wtab) {
  char key[96];
  snprintf(key, sizeof key, "hv.wtab2:%.17g:%d", fs_d, hmax);
  auto it = ctx->tables.find(key);
  if (it != ctx->tables.end()) {
    *d_wtab = reinterpret_cast<const double2*>(it->second);
    return 0;
  }
  // row h at offset h*(h+2): a zero pair, the 2h+1 window pairs, a zero pair
  std::vector<double> tab((size_t)2 * (hmax + 2) * (hmax + 4), 0.0);
  std::vector<double> mw;
  for (int h = 0; h <= hmax + 1; ++h) {
    const int Lh = 2 * h + 1;
    const double wlit = (2 * (double)h + 1) / fs_d;
    mw.assign(Lh, 0.0);
    for (int j = 0; j < Lh; ++j) {
      // index_raw keeps round_matlab's +0.5 and the +0.001 "first-aid" (harvest.py:178, Q1): the window is
      // evaluated 0.501 samples late
      const double c = cos(M_PI * (2 * (((double)(j - h) + (0.001 + 0.5) - 1.0) / fs_d) / wlit));
      mw[j] = 0.42 + 0.5 * c + 0.08 * (2 * c * c - 1);
    }
    double* row = tab.data() + 2 * ((size_t)h * (h + 2) + 1);
    for (int j = 0; j < Lh; ++j) {
      double dw;
      if (j == 0) dw = Lh > 1 ? -mw[1] / 2 : 0.0;
      else if (j == Lh - 1) dw = mw[j - 1] / 2;
      else dw = -((mw[j + 1] - mw[j]) + (mw[j] - mw[j - 1])) / 2;
      row[2 * j] = mw[j];
      row[2 * j + 1] = dw;
    }
  }
  const double* d = nullptr;
  if (int rc = const_table(ctx, key, tab, &d)) return rc;
  *d_wtab = reinterpret_cast<const double2*>(d);
  return 0;
}

// One launch of hv_refine_kernel<TWL, WTAB>: LDS twiddles with tabulated windows, or the global-twiddle rotation form.
template <bool TWL, bool WTAB>
int launch_refine_form(wh_ctx* ctx, hipStream_t st, const HvPlan& p, double f0_floor, double f0_ceil, const HvDev& d, int tw_n,
                       const double2* d_rot, const double2* d_wtab) {
  const int fpb = refine_frames(WTAB);
  const int seglen = 2 * p.hmax + 8 + (fpb - 1) * ((int)ceil(p.fs_d / 1000.0) + 1);
  const size_t lds = sizeof(double2) * (size_t)tw_n + sizeof(double) * (size_t)((seglen + 1) & ~1) +
                     (sizeof(double) + 3 * sizeof(int)) * (size_t)refine_item_cap(WTAB) + sizeof(int) * (72 + 5 * fpb + 1);
  const dim3 grid((unsigned)((p.max_nf1 + fpb - 1) / fpb), p.B);
  // slots of the work list a round may fill: all of them, unless WH_HV_ITEM_CAP_RT (tests: the several-rounds path,
  // which real input reaches only with > ~70 candidates per frame over a whole block) says fewer
  static const int cap_env = getenv("WH_HV_ITEM_CAP_RT") ? atoi(getenv("WH_HV_ITEM_CAP_RT")) : 0;
  int item_cap = refine_item_cap(WTAB);
  if (cap_env >= kRows && cap_env < item_cap) item_cap = cap_env;
  if (int rc = allow_lds(&hv_refine_kernel<TWL, WTAB>, lds)) return rc;
  WH_LAUNCH(ctx, st, "hv_refine_kernel", hv_refine_kernel<TWL, WTAB>, grid, dim3(256), lds, d.meta, d.y, d.dc, d.dn,
            p.fs_d, f0_floor, f0_ceil, p.hmax, seglen, ctx->d_twiddle, tw_n, d_rot, d_wtab, d.rf0, d.rsc, d.lst,
            item_cap);
  return 0;
}

}  // namespace

namespace wh {

int hv_launch_refine(wh_ctx* ctx, hipStream_t st, const HvPlan& p, double f0_floor, double f0_ceil, const HvDev& d) {
  int tw_n = 1;  // transform length of the longest window (harvest.py:171-172): 2 * 2^ceil(log2(2*hmax+1))
  while (tw_n < 2 * p.hmax + 1) tw_n <<= 1;
  tw_n <<= 1;
  if (tw_n > 2048) tw_n = 0;  // 32 KB of LDS at most for the table; beyond that gather from the global tables
  double2* d_rot = nullptr;
  if (int rc = upload_rotation_table(ctx, st, p.fs_d, p.hmax, &d_rot)) return rc;
  if (tw_n) {
    const double2* d_wtab = nullptr;
    if (int rc = window_table(ctx, p.fs_d, p.hmax, &d_wtab)) return rc;
    return launch_refine_form<true, true>(ctx, st, p, f0_floor, f0_ceil, d, tw_n, d_rot, d_wtab);
  }
  return launch_refine_form<false, false>(ctx, st, p, f0_floor, f0_ceil, d, 0, d_rot, nullptr);
}

int hv_launch_prune(wh_ctx* ctx, hipStream_t st, const HvPlan& p, const HvDev& d) {
  WH_LAUNCH(ctx, st, "hv_prune_kernel", hv_prune_kernel,
            dim3((unsigned)((p.max_nf1 + kPruneFrames - 1) / kPruneFrames), p.B), dim3(256), 0, d.meta, d.rf0, d.lst,
            d.keep);
  return 0;
}

}  // namespace wh
