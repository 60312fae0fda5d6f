// D4C's rank selection: the sum of the m smallest of K band powers without a sort (sum_smallest) and its wave-level
// counting helpers.  d4c_frame's band stage calls it; wh_d4c_select_probe (wh_d4c_probe.hip) runs it on caller data.
// Include after wh_d4c_types.h.
#pragma once
#include "wh_reduce.h"

namespace wh {

// Exponents per round of sum_smallest: WIN = 1 << DB, 4 as built.  On speech the K - m (~22) largest bins lie within 4
// octaves of the maximum on average, 7 at most (measured on the oracle's spectra), so a second round is nothing unusual;
// the loop slides on as far as the values reach (tests/test_hip_d4c_select.py: ten rounds).
// Long spectra (K = 2049 at 48 kHz: 65 bins dropped, spread over more octaves, hundreds of values in the threshold bin)
// have a DB of their own, kSelDbLong: more exponents per round and mantissa bits per refinement level mean fewer rounds,
// barrier pairs and count exchanges for more counters per round.  Both are 2 as built.
constexpr int kSelDb = 2;
constexpr int kSelDbLong = 2;  // K > 1100

// 64-lane sum of a 32-bit integer on the VALU (the DPP ladder of wh::wave_sum), result uniform
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
  v += (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
  v += (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
  v += (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, true);  // row_half_mirror
  v += (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xF, 0xF, true);  // row_mirror
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// mine[e] = number of slots in the wave whose digit (0 .. WIN-1, or < 0: not counted) is e.  Packed form: every lane
// counts its own slots into 16-bit fields (two digit values per register) and the registers are summed over the wave
// by DPP — VALU only; the ballot form is a v_cmp, an s_bcnt1 and an s_add per (digit value, slot), each SALU instruction
// waiting for the VALU-written mask.
template <int WIN, int PER, class Digit>
__device__ __forceinline__ void wave_digit_counts(Digit digit, int (&mine)[WIN]) {
  static_assert(WIN % 2 == 0, "two digit values per register");
  unsigned c[WIN / 2];
#pragma unroll
  for (int j = 0; j < WIN / 2; ++j) c[j] = 0;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int d = digit(q);
#pragma unroll
    for (int j = 0; j < WIN / 2; ++j) c[j] += (d >> 1) == j ? (1u << (16 * (d & 1))) : 0u;
  }
#pragma unroll
  for (int j = 0; j < WIN / 2; ++j) {
    const unsigned ssum = wave_sum_u32(c[j]);
    mine[2 * j] = (int)(ssum & 0xFFFF);
    mine[2 * j + 1] = (int)(ssum >> 16);
  }
}

// Sum of the m smallest of K non-negative values and their total, without sorting and without LDS atomics.
// The reference sorts the K powers and prefix-sums them (world/d4c.py:206-208); only the VALUES of the m smallest
// enter the sum, and m = K - (boundary + 1) is close to K, so the kernel finds the few LARGE values to leave out:
//   (1) per wave, the maximum IEEE exponent (shuffles) and the population counts of the WIN = 1 << kSelDb = 4
//       exponents at and below it (packed counters summed by DPP); counts AND the wave's maximum go through LDS
//       together, so one hop yields the block maximum and the block's counts; the window slides further down, WIN
//       exponents per round, while the K - m largest span more than that;
//   (2) the one exponent bin that holds the threshold is compacted into a list at offsets derived from the same
//       ballots (no atomic counter) and its members are ranked against each other (~11 on speech); equal values are
//       interchangeable in a sum, so ties need no index rule.
// Each thread then adds its own kept elements in a fixed order -> deterministic sums.
// x[q], q < PER: the thread's share of the K values (bit q of `valid` set where the slot is used — any assignment of the
// values to threads will do).  work: >= 80 ints + K doubles of free
// LDS; scratch: 32 doubles.  Four barrier phases.
template <int K, int FT, int PER>
__device__ __forceinline__ void sum_smallest(const double (&x)[PER], unsigned valid, int m, wh::ckp<double> work, wh::ckp<double> scratch,
                                             double* s_small, double* s_total) {
  constexpr int NW = FT / 64;
  constexpr int DB = K > 1100 ? kSelDbLong : kSelDb;   // mantissa bits per refinement level
  constexpr int WIN = 1 << DB;           // exponents per round = values of a mantissa digit
  const wh::ckp<int> cnts = wh::ck_as<int>(work);               // [NW][WIN + 1]: counts per exponent, then the wave's top
  const wh::ckp<double> list = work + (NW * (WIN + 1) + (NW * (WIN + 1) & 1)) / 2;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int key[PER];
  int kmax = 0;
  double t = 0.0;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const bool in = (valid >> q) & 1u;  // slot q of this thread holds one of the K values
    key[q] = in ? (int)((__double_as_longlong(x[q]) >> 52) & 0x7FF) : -1;
    if (in) t += x[q];
    kmax = key[q] > kmax ? key[q] : kmax;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(kmax, o, 64);
    kmax = u > kmax ? u : kmax;
  }
  const int drop = K - m;  // how many of the largest values are left out (>= 1)
  // Round 0 counts below the WAVE's own maximum and publishes that maximum next to the counts: one LDS hop gives every
  // thread the block maximum and all counts (a wave whose maximum is lower has nothing above its own window, and its
  // window reaches at least as far down as the block's).  Further rounds (rare) count below the common `top`.
  int top = kmax;          // exponent at the top of this wave's current window
  int above = 0;           // elements with an exponent above the window
  int tbin = -1, wave_before = 0, in_bin = 0;
  bool first = true;
  while (true) {
    int mine[WIN];
    wave_digit_counts<WIN, PER>([&](int q) {  // digit e = exponent top - e; padding slots (key -1) and the rest: none
      const int d = top - key[q];
      return (key[q] >= 0 && d >= 0 && d < WIN) ? d : -1;
    }, mine);
    wh::sync<FT>();  // the work area is free (previous round's counts have been read by everyone)
    if (lane <= WIN) {
      int c = top;
#pragma unroll
      for (int e = 0; e < WIN; ++e) c = lane == e ? mine[e] : c;
      cnts[w * (WIN + 1) + lane] = c;
    }
    wh::sync<FT>();
    int gtop = top;
    if (first) {
#pragma unroll
      for (int i = 0; i < NW; ++i) gtop = cnts[i * (WIN + 1) + WIN] > gtop ? cnts[i * (WIN + 1) + WIN] : gtop;
    }
    // lane e sums the waves' counts of offset e (and what the waves in front of this one hold of it); the WIN results
    // come back through readlane as uniform values — WIN LDS reads per wave in WIN lanes instead of in every lane
    int tot_l = 0, bef_l = 0;
    if (lane < WIN) {
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        // wave i counted exponent gtop - e at its own offset e - (gtop - top_i)
        const int sh = first ? gtop - cnts[i * (WIN + 1) + WIN] : 0;
        const int c = lane - sh >= 0 ? cnts[i * (WIN + 1) + (lane - sh)] : 0;
        bef_l += i < w ? c : 0;
        tot_l += c;
      }
    }
    int run = above;
#pragma unroll
    for (int e = 0; e < WIN; ++e) {  // e: offset below the BLOCK's top
      const int tot = __builtin_amdgcn_readlane(tot_l, e), before = __builtin_amdgcn_readlane(bef_l, e);
      if (tbin < 0 && run + tot >= drop) {
        tbin = gtop - e;
        above = run;
        wave_before = before;
        in_bin = tot;
      }
      run += tot;
    }
    if (tbin >= 0 || gtop - WIN < 0) break;
    above = run;
    top = gtop - WIN;  // every wave continues below the common window
    first = false;
  }
  // tbin < 0 cannot happen (every element has an exponent in [0, kmax]); guard anyway: drop nothing more
  int need = tbin >= 0 ? drop - above : 0;  // members of the threshold bin that belong to the large set
  double a = 0.0;
#pragma unroll
  for (int q = 0; q < PER; ++q)
    if (key[q] >= 0 && key[q] < tbin) a += x[q];  // everything below the threshold bin is kept
  // The members of the threshold bin are ranked against each other below, in_bin^2 / FT comparisons: fine for the ~11
  // members a 2048-point band spectrum leaves there (22 bins dropped of 1025), not for the hundreds of a 4096-point one
  // (65 of 2049: 41 % of the whole kernel at 48 kHz).  While the bin holds more than 32 values it is split by the next
  // DB mantissa bits — the same packed counts, WIN digits, one LDS hop — and only the digit that holds the
  // threshold stays a candidate: larger digits are dropped whole, smaller ones kept whole.
  unsigned cand = 0;  // bit q: slot q is a member of the current threshold set
#pragma unroll
  for (int q = 0; q < PER; ++q) cand |= (key[q] == tbin ? 1u : 0u) << q;
  int shift = 52;
  while (in_bin > 32 && shift >= DB) {  // (uniform)
    shift -= DB;
    int dig[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) dig[q] = ((cand >> q) & 1u) ? (int)((__double_as_longlong(x[q]) >> shift) & (WIN - 1)) : -1;
    int mine[WIN];
    wave_digit_counts<WIN, PER>([&](int q) { return dig[q] >= 0 ? WIN - 1 - dig[q] : -1; }, mine);  // e counts down from the largest digit
    wh::sync<FT>();
    if (lane < WIN) {
      int c = 0;
#pragma unroll
      for (int e = 0; e < WIN; ++e) c = lane == e ? mine[e] : c;
      cnts[w * (WIN + 1) + lane] = c;
    }
    wh::sync<FT>();
    int tot_l = 0, bef_l = 0;
    if (lane < WIN) {
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        const int c = cnts[i * (WIN + 1) + lane];
        bef_l += i < w ? c : 0;
        tot_l += c;
      }
    }
    int run = 0, td = -1, bef = 0, tot_d = 0, run_at = 0;
#pragma unroll
    for (int e = 0; e < WIN; ++e) {
      const int tot = __builtin_amdgcn_readlane(tot_l, e), before = __builtin_amdgcn_readlane(bef_l, e);
      if (td < 0 && run + tot >= need) {
        td = WIN - 1 - e;
        run_at = run;
        bef = before;
        tot_d = tot;
      }
      run += tot;
    }
    // (td >= 0 always: the set holds at least `need` members)
    need -= run_at;
    wave_before = bef;
    in_bin = tot_d;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      if (dig[q] >= 0 && dig[q] < td) a += x[q];  // below the threshold digit: kept
      if (dig[q] != td) cand &= ~(1u << q);
    }
  }
  // compaction of the threshold set: wave offset from the per-wave counts, lane offset from the ballots
  {
    int pos = wave_before;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const bool mem = (cand >> q) & 1u;
      const unsigned long long mk = __ballot(mem);
      if (mem) list[pos + __popcll(mk & ((1ull << lane) - 1ull))] = x[q];
      pos += __popcll(mk);
    }
  }
  wh::sync<FT>();
  // the threshold bin: list entry i is kept unless it is one of the `need` largest (ties: list order).  One entry
  // per thread, so the ranking costs in_bin LDS reads per thread whatever the distribution of the bin over threads.
  for (int i = threadIdx.x; i < in_bin; i += FT) {
    const double v = list[i];
    int ahead = 0;
    for (int j = 0; j < in_bin; ++j) {
      const double o = list[j];
      ahead += (o > v || (o == v && j < i)) ? 1 : 0;
    }
    if (ahead >= need) a += v;
  }
  wh::block_sum2<FT>(a, t, scratch);
  *s_small = a;
  *s_total = t;
}

}  // namespace wh
