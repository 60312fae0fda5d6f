// D4C's analysis windows: the per-frame set-up table (win_setup / win_load / win_thread_phase) and the two forms of the
// windowed, DC-removed pitch-synchronous frame — d4c_window (through LDS) and d4c_window_regs (register-fed, N = 8 FT).
// The two are kept as two routines on purpose: one shared helper moved 15 of the unit's 28 functions.
// Include after wh_d4c_types.h.
#pragma once
#include "wh_reduce.h"

namespace wh {

constexpr int kKeepW = 4;  // rows of a register-fed window whose window values survive from the first walk to the second

// Per-frame set-up of one analysis window, evaluated ONCE per workgroup by a single lane (win_setup) and read back by
// every thread through LDS broadcasts: window length, clamped sample range, rotation constants and the start phase are
// the same for all threads, yet as straight-line code each of the four waves spent ~280 instructions per window on
// them (five FP64 divides, two sincospi, the 64-bit clamps) — a fifth of this kernel's instruction stream.
// The per-thread start phase is base * E[tid]: E = exp(i*pi*delta*tid) costs one sincospi per thread and is shared by
// the windows that have the same f0 and length (the Hann frame and the two centroid frames).
struct WinSetup {
  int hwl, L, rlo, rhi;
  long long centre;
  double rot_s, rot_c, base_s, base_c, delta, inv_span, phase, cf;
};
__device__ __forceinline__ void win_setup(wh::ckp<double> tab, long long xn, double fs, double cf, double pos, double half_length,
                                          int ft) {
  const int hwl = (int)(half_length * fs / cf + 0.5);
  const long long centre = wh::frame_centre(pos, fs);
  const double phase = (pos * fs - (double)(long long)(pos * fs + 0.5)) / fs;
  // per-frame constants are inverted once and multiplied in: an FP64 divide is ~12 instructions with a long
  // dependency chain, and the per-sample ones were a fifth of this kernel's instruction count (results move by an ulp)
  const double inv_span = 1.0 / fs / half_length;
  // sample index relative to the centre, clamped to the utterance (d4c.py:98): x[centre - 1 + rel]
  const long long rel_min = 1 - centre, rel_max = xn - centre;
  const int rlo = (int)(rel_min < -(1 << 30) ? -(1 << 30) : (rel_min > (1 << 30) ? (1 << 30) : rel_min));
  const int rhi = (int)(rel_max > (1 << 30) ? (1 << 30) : (rel_max < -(1 << 30) ? -(1 << 30) : rel_max));
  double rot_s, rot_c, base_s, base_c;
  sincospi((double)ft * inv_span * cf, &rot_s, &rot_c);                 // rotation by FT samples
  sincospi(((double)(0 - hwl) * inv_span + phase) * cf, &base_s, &base_c);  // phase of sample 0
  tab[0] = (double)hwl;
  tab[1] = (double)(2 * hwl + 1);
  tab[2] = (double)rlo;
  tab[3] = (double)rhi;
  tab[4] = (double)centre;  // |centre| < 2^53
  tab[5] = rot_s;
  tab[6] = rot_c;
  tab[7] = base_s;
  tab[8] = base_c;
  tab[9] = inv_span * cf;
  tab[10] = inv_span;
  tab[11] = phase;
  tab[12] = cf;
}
__device__ __forceinline__ WinSetup win_load(wh::ckp<const double> tab) {
  WinSetup w;
  w.hwl = (int)tab[0];
  w.L = (int)tab[1];
  w.rlo = (int)tab[2];
  w.rhi = (int)tab[3];
  w.centre = (long long)tab[4];
  w.rot_s = tab[5];
  w.rot_c = tab[6];
  w.base_s = tab[7];
  w.base_c = tab[8];
  w.delta = tab[9];
  w.inv_span = tab[10];
  w.phase = tab[11];
  w.cf = tab[12];
  return w;
}
// E[tid] = exp(i*pi*delta*tid) as (sin, cos)
__device__ __forceinline__ double2 win_thread_phase(double delta) {
  double s, c;
  sincospi(delta * (double)threadIdx.x, &s, &c);
  return make_double2(s, c);
}

// Windowed, DC-removed pitch-synchronous frame (world/d4c.py:92-110).  emit(j, value) is called for every sample
// j = tid + q*FT < N (zero beyond the window; rows longer than N are cropped like np.fft.fft(x, n), Q7) — the callers
// store straight into the transform buffer, so no per-thread output array exists.  ENERGY: the values are divided by
// the frame's norm sqrt(sum(wave^2)) over the FULL window (d4c.py:147).  BLACKMAN selects window type 2, else Hann.
//
// Two walks, one reduction, no per-thread arrays: the first walk accumulates the sums, the second fetches the
// samples again (L1/L2 hits) and emits the DC-removed values.  Keeping x*w and w in registers between the walks (the
// first version) made this routine the kernel's register peak (~95 VGPRs on its own).  The window is re-derived
// cheaply in both walks because cos(pi*f0*t_j) advances from j to j + FT by a fixed rotation (one sincospi per
// thread and 4 flops per sample instead of one cospi per sample).  The energy of the DC-removed frame comes out of
// the same block reduction as the two means:
//   sum (xw - w*dc)^2 = sum (xw)^2 - 2*dc*sum (xw*w) + dc^2 * sum w^2
// (three more partial sums, no second pass over the data and no second pair of barriers).  The expansion loses
// log10((DC/AC)^2) digits to cancellation — nothing for speech-like input (DC << AC), and still 1e-10 relative for a
// DC offset 1000x the signal.
// slot / STRIDE: sample j is parked at slot[j * STRIDE] (LDS) between the gather and the second walk — the place emit()
// overwrites with the final value, so the park costs no extra memory.
template <bool BLACKMAN, int N, bool ENERGY, int STRIDE, int FT_ = 0, class Emit>
__device__ __forceinline__ void d4c_window(wh::ckp<const double> WH_RESTRICT xu, wh::ckp<const double> tab, double2 e_tid,
                                           wh::ckp<double> scratch, wh::ckp<double> slot, Emit emit) {
  constexpr int FT = FT_ ? FT_ : ft_of(N);
  constexpr int Q = N / FT;
  const WinSetup ws = win_load(tab);
  const int hwl = ws.hwl, L = ws.L, rlo = ws.rlo, rhi = ws.rhi;
  const double inv_span = ws.inv_span, phase = ws.phase, cf = ws.cf;
  auto shape = [](double c1) -> double {
    return BLACKMAN ? (0.08 * (2 * c1 * c1 - 1) + 0.5 * c1 + 0.42) : (0.5 * c1 + 0.5);  // cos(2a) = 2cos^2(a)-1
  };
  auto win = [&](int j) -> double { return shape(cospi(((double)(j - hwl) * inv_span + phase) * cf)); };
  const wh::ckp<const double> xb = xu + (ws.centre - 1);  // (re-derived from laundered bits before the second walk)
  auto sample = [&](int j) -> double {
    int rel = j - hwl;
    rel = rel < rlo ? rlo : rel;
    rel = rel > rhi ? rhi : rel;
    return xb[rel];
  };
  const double rot_s = ws.rot_s, rot_c = ws.rot_c;
  // phase of this thread's first sample: base * E[tid]
  const double c0 = ws.base_c * e_tid.y - ws.base_s * e_tid.x;
  const double s0 = ws.base_s * e_tid.y + ws.base_c * e_tid.x;
  double s_sw = 0.0, s_w = 0.0, s_swsw = 0.0, s_sww = 0.0, s_ww = 0.0;
  // The gather is ONE round: all Q loads of the thread are issued together and parked in LDS as they arrive (each
  // thread only ever touches its own slots, so no barrier is involved).  Both walks then read LDS.  Gathering inside
  // the walks — in chunks of four, twice — put four dependent global-memory round trips (~3.5 k cycles each on the
  // loaded chip) into every window: 15 k of a window's 20 k cycles; carrying the samples in registers across the
  // reduction instead was the register peak of the kernel.
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int j = threadIdx.x + q * FT;
    slot[j * STRIDE] = sample(j);  // clamped: always a valid address
  }
  {
    double c = c0, sn = s0;
#pragma unroll 2
    for (int q = 0; q < Q; ++q) {
      const int j = threadIdx.x + q * FT;
      if (j < L) {
        const double w = shape(c);
        const double sw = slot[j * STRIDE] * w;
        s_sw += sw;
        s_w += w;
        if (ENERGY) {
          s_swsw += sw * sw;
          s_sww += sw * w;
          s_ww += w * w;
        }
      }
      const double cn = c * rot_c - sn * rot_s;
      sn = sn * rot_c + c * rot_s;
      c = cn;
    }
    for (int j = N + threadIdx.x; j < L; j += FT) {  // rows longer than N: cropped, but they count in the sums
      const double w = win(j);
      const double sw = sample(j) * w;
      s_sw += sw;
      s_w += w;
      if (ENERGY) {
        s_swsw += sw * sw;
        s_sww += sw * w;
        s_ww += w * w;
      }
    }
  }
  STAGE_MARK(kStWinWalk)
  if (ENERGY) wh::block_sum5<FT>(s_sw, s_w, s_swsw, s_sww, s_ww, scratch);
  else wh::block_sum2<FT>(s_sw, s_w, scratch);
  STAGE_MARK(kStWinReduce)
  const double dc = s_sw / s_w;  // = mean(x w) / mean(w): the two divisions by L cancel (two FP64 divides less per window)
  const double inv_nrm = ENERGY ? 1.0 / sqrt((s_swsw - 2.0 * dc * s_sww) + dc * dc * s_ww) : 1.0;
  {
    double c = c0, sn = s0;
#pragma unroll 2
    for (int q = 0; q < Q; ++q) {
      const int j = threadIdx.x + q * FT;
      double val = 0.0;
      if (j < L) {
        const double w = shape(c);
        val = slot[j * STRIDE] * w - w * dc;
        if (ENERGY) val *= inv_nrm;
      }
      emit(j, val);
      const double cn = c * rot_c - sn * rot_s;
      sn = sn * rot_c + c * rot_s;
      c = cn;
    }
  }
}

// The register-fed form (N = 8 * FT: the lengths D4C runs at from 16 kHz up).  A thread's Q = N / FT samples
// j = tid + q*FT are exactly the operands of its radix-8 butterfly in the FIRST pass of the transform that follows, so
// the windowed frame never exists in LDS: one round of global loads into registers, walk 1 (the sums) and walk 2 (the
// DC-removed, normalised values) over those registers, and out[q] goes straight into wh::fft_lds_from_regs.  Against
// d4c_window this removes, per frame and window, the parking store (2048 x 8 B), both walks' LDS reads, the emit of
// 2048 complex values and the first pass's read of them — stores are what an FFT pass costs on this LDS (~80 B/clk per
// CU, MI355X_MICROARCH.md) — and the walks stop at the window's end: rows q >= ceil(L / FT) are zeros (a window spans
// 4 pitch periods, ~640 of the 2048 samples at 100 Hz), uniformly for the workgroup.
template <bool BLACKMAN, int N, bool ENERGY, int FT_ = 0>
__device__ __forceinline__ void d4c_window_regs(wh::ckp<const double> WH_RESTRICT xu, wh::ckp<const double> tab, double2 e_tid,
                                                wh::ckp<double> scratch, double (&out)[N / (FT_ ? FT_ : ft_of(N))]) {
  constexpr int FT = FT_ ? FT_ : ft_of(N);
  constexpr int Q = N / FT;
  const WinSetup ws = win_load(tab);
  const int hwl = ws.hwl, L = ws.L, rlo = ws.rlo, rhi = ws.rhi;
  const double inv_span = ws.inv_span, phase = ws.phase, cf = ws.cf;
  auto shape = [](double c1) -> double {
    return BLACKMAN ? (0.08 * (2 * c1 * c1 - 1) + 0.5 * c1 + 0.42) : (0.5 * c1 + 0.5);  // cos(2a) = 2cos^2(a)-1
  };
  auto win = [&](int j) -> double { return shape(cospi(((double)(j - hwl) * inv_span + phase) * cf)); };
  const wh::ckp<const double> xb = xu + (ws.centre - 1);
  auto sample = [&](int j) -> double {
    int rel = j - hwl;
    rel = rel < rlo ? rlo : rel;
    rel = rel > rhi ? rhi : rel;
    return xb[rel];
  };
  // rows that hold window samples: workgroup-uniform, and said so (a scalar: the row tests below are scalar branches)
  const int nq = __builtin_amdgcn_readfirstlane(L >= N ? Q : (L + FT - 1) / FT);
  // All loads of a round are issued unconditionally (the index is clamped: always a valid address; rows past the window
  // read its last sample, one line for the whole wave) and the rows past nq zeroed by a select.  Written as `if (q < nq)
  // out[q] = sample(..)` the compiler made a chain of conditional blocks, each WAITING for its load before the next block's
  // and copying the whole array between them: nq dependent global round trips and ~25 register moves per row.
  // Two rounds to choose from, each straight-line: a window of at most Q / 2 rows (every pitch above 62.5 Hz at N = 2048)
  // loads Q / 2 rows and its upper rows are plain zeros — no clamp, address, load or select for them.
  if (nq <= Q / 2) {
#pragma unroll
    for (int q = 0; q < Q / 2; ++q) out[q] = sample(threadIdx.x + q * FT);
#pragma unroll
    for (int q = 0; q < Q / 2; ++q) out[q] = q < nq ? out[q] : 0.0;
#pragma unroll
    for (int q = Q / 2; q < Q; ++q) out[q] = 0.0;
  } else {
#pragma unroll
    for (int q = 0; q < Q; ++q) out[q] = sample(threadIdx.x + q * FT);
#pragma unroll
    for (int q = 0; q < Q; ++q) out[q] = q < nq ? out[q] : 0.0;
  }
  const double rot_s = ws.rot_s, rot_c = ws.rot_c;
  const double c0 = ws.base_c * e_tid.y - ws.base_s * e_tid.x;  // phase of this thread's first sample: base * E[tid]
  const double s0 = ws.base_s * e_tid.y + ws.base_c * e_tid.x;
  double s_sw = 0.0, s_w = 0.0, s_swsw = 0.0, s_sww = 0.0, s_ww = 0.0;
  // The window values of the first KEEPQ rows are kept for the second walk (rows beyond that — windows longer than
  // KEEPQ * FT samples, f0 below ~62 Hz at N = 2048 — re-derive theirs by the rotation, as every row used to).
  constexpr int KEEPQ = N >= 4096 ? 0 : (kKeepW < Q ? kKeepW : Q);  // (N = 4096: 26 ... 276 spilled registers)
  double wk[KEEPQ > 0 ? KEEPQ : 1];
  {
    double c = c0, sn = s0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      if (q < nq) {
        const int j = threadIdx.x + q * FT;
        double w = 0.0;
        if (j < L) {
          w = shape(c);
          const double sw = out[q] * w;
          s_sw += sw;
          s_w += w;
          if (ENERGY) {
            s_swsw += sw * sw;
            s_sww += sw * w;
            s_ww += w * w;
          }
        }
        if (q < KEEPQ) wk[q] = w;
        const double cn = c * rot_c - sn * rot_s;
        sn = sn * rot_c + c * rot_s;
        c = cn;
      }
    }
    for (int j = N + threadIdx.x; j < L; j += FT) {  // rows longer than N: cropped, but they count in the sums
      const double w = win(j);
      const double sw = sample(j) * w;
      s_sw += sw;
      s_w += w;
      if (ENERGY) {
        s_swsw += sw * sw;
        s_sww += sw * w;
        s_ww += w * w;
      }
    }
  }
  STAGE_MARK(kStWinWalk)
  if (ENERGY) wh::block_sum5<FT>(s_sw, s_w, s_swsw, s_sww, s_ww, scratch);
  else wh::block_sum2<FT>(s_sw, s_w, scratch);
  STAGE_MARK(kStWinReduce)
  const double dc = s_sw / s_w;  // = mean(x w) / mean(w): the two divisions by L cancel (two FP64 divides less per window)
  const double inv_nrm = ENERGY ? 1.0 / sqrt((s_swsw - 2.0 * dc * s_sww) + dc * dc * s_ww) : 1.0;
  {
    double c = c0, sn = s0;
    if (KEEPQ < Q && nq > KEEPQ) {  // phase of row KEEPQ for the rows that re-derive their window value
#pragma unroll
      for (int q = 0; q < KEEPQ; ++q) {
        const double cn = c * rot_c - sn * rot_s;
        sn = sn * rot_c + c * rot_s;
        c = cn;
      }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      if (q < nq) {
        const int j = threadIdx.x + q * FT;
        double val = 0.0;
        if (q < KEEPQ) {
          const double w = wk[q];  // 0 past the window's end
          val = out[q] * w - w * dc;
          if (ENERGY) val *= inv_nrm;
          if (!(j < L)) val = 0.0;
        } else {
          if (j < L) {
            const double w = shape(c);
            val = out[q] * w - w * dc;
            if (ENERGY) val *= inv_nrm;
          }
          const double cn = c * rot_c - sn * rot_s;
          sn = sn * rot_c + c * rot_s;
          c = cn;
        }
        out[q] = val;
      }
    }
  }
}

}  // namespace wh
