// One pulse of a run of response_kernel (wh_synthesis.hip): log spectra, noise run, minimum-phase chains, noise
// convolution, DC removal and overlap-add into the run's ring — and noise_conv_groups, the convolution as response_pair
// runs it.  Include after wh_math.h, wh_reduce.h, wh_philox.h, wh_resp_types.h and wh_resp_ring.h.
#pragma once

namespace {

// response_pulse's noise convolution of R <= 4 outputs per thread (the shift-free form described there) for response_pair:
// acc[q] += sum_{j < cnt} nzb[j] * ra[mb0 + q - j], mb0 = m0 - j0, ra the padded response (rap_index), nzb the zero-mean noise,
// zero-padded to a multiple of 2R.  The same loads and the same FMAs in the same order: the same bits.
template <int R>
__device__ __forceinline__ void noise_conv_groups(wh::ckp<double> rap, wh::ckp<double> nzb, int cnt, int m0, int64_t j0, double (&acc)[R]) {
#pragma clang fp contract(fast)
  auto load_group = [&](int base, double (&g)[R]) {  // base is a multiple of R: a group is all-valid or all before the start
#pragma unroll
    for (int t = 0; t < R; t += 2) {
      double2 v = make_double2(0.0, 0.0);
      if (base >= 0) v = wh::ck_as<const double2>(rap + rap_index(base + t))[0];
      g[t] = v.x;
      g[t + 1] = v.y;
    }
  };
  auto block = [&](int j, const double (&hi)[R], const double (&lo)[R]) {
    double n[R];
#pragma unroll
    for (int t = 0; t < R; t += 2) {
      const double2 v = wh::ck_as<const double2>(nzb + (j + t))[0];
      n[t] = v.x;
      n[t + 1] = v.y;
    }
#pragma unroll
    for (int sft = 0; sft < R; ++sft)
#pragma unroll
      for (int q = 0; q < R; ++q) acc[q] = fma(n[sft], q - sft >= 0 ? hi[q - sft] : lo[R + q - sft], acc[q]);
  };
  double ga[R], gb[R];
  const int mb0 = m0 - (int)j0;
  load_group(mb0, ga);
  load_group(mb0 - R, gb);
  const int steps = ((cnt + 2 * R - 1) / (2 * R)) * (2 * R);  // the noise is zero-padded up to a multiple of 2R
  for (int j = 0; j < steps; j += 2 * R) {
    block(j, ga, gb);
    load_group(mb0 - j - 2 * R, ga);
    block(j + R, gb, ga);
    load_group(mb0 - j - 3 * R, gb);
  }
}

// One pulse of a run.
template <int N>
__device__ __forceinline__ void response_pulse(const RespArgs& A, const PulseRec& rec, char* smem, wh::ckp<double> ring, RunState& rs,
                                               wh::ckp<double> WH_RESTRICT row,
                                               const double (&dcw)[N / ft_syn(N) <= 4 ? N / ft_syn(N) : 1]) {
#pragma clang fp contract(fast)
  const SynUtt* __restrict__ meta = A.meta;
  const double* __restrict__ spectrogram = A.spectrogram;
  const double* __restrict__ aperiodicity = A.aperiodicity;
  const double fs = A.fs;
  const double* __restrict__ noise = A.noise;
  const uint64_t seed = A.seed;
  const double* __restrict__ dc_base = A.dc_base;
  const double2* __restrict__ tw_raw = A.tw_base;
  asm volatile("" : "+s"(tw_raw));  // per pulse: no twiddle address / value of one pulse survives into the next
  const wh::ckp<const double2> tw_base = wh::ck_make(tw_raw, WH_TWIDDLE_ENTRIES, wh::WH_CK_TWIDDLE);
  const double* __restrict__ mt_raw = A.math_tab;
  asm volatile("" : "+s"(mt_raw));  // (likewise)
  const wh::ckp<const double> mt = wh::ck_make(mt_raw, wh::kMtEntries, wh::WH_CK_TABLE);
  constexpr int FT = ft_syn(N);
  constexpr int K = N / 2 + 1;
  constexpr int NZ = kRespNoise;
  constexpr int NZC = resp_conv8<N>() ? 252 : NZ;  // noise samples per chunk (the eight-output form walks them twelve at a time)
  constexpr int R = N / FT;  // consecutive output samples per thread
  static_assert(R % 2 == 0 && NZ % (2 * R) == 0, "pairwise reads; whole blocks of 2R noise samples");
  constexpr int GT = FT >= 256 ? FT / 2 : FT;  // threads per chain: the periodic and aperiodic chains run side by side
  constexpr int NG = FT / GT;
  // (wh::ckp<T> is T* in every shipped build; the bounds build checks each access against the range named here)
  using L = RespLds<N>;
  static_assert(NZ == L::kNoiseLen, "the noise block of the layout is the chunk this function stages");
  const wh::ckp<double> lds_all = wh::ck_make(reinterpret_cast<double*>(smem), L::kPulse, wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> zrA = wh::ck_sub(lds_all, L::kChainA, L::kChainLen, wh::WH_CK_LDS_MAIN);  // N/2+1 complex: aperiodic chain
  const wh::ckp<double2> zbA = wh::ck_as<double2>(zrA);
  const wh::ckp<double> zrP = wh::ck_sub(lds_all, L::kChainP, L::kChainLen, wh::WH_CK_LDS_AUX);   // N/2+1 complex: periodic chain
  const wh::ckp<double2> zbP = wh::ck_as<double2>(zrP);
  const wh::ckp<double> rap = wh::ck_sub(lds_all, L::kRap, L::kRapLen, wh::WH_CK_LDS_OTHER);  // padded aperiodic response
  const wh::ckp<double> nz = wh::ck_sub(lds_all, L::kNoise, L::kNoiseLen, wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> scratch = wh::ck_sub(lds_all, L::kScratch, L::kScratchLen, wh::WH_CK_LDS_SCRATCH);

  RSTAGE_BEGIN
  wh::sync<FT>();
  const int u = rec.u;
  const SynUtt m = meta[u];  // (output / noise offsets: not needed before the noise fetch and the overlap-add)
  const int64_t pidx = rec.pidx;
  const double shift = rec.shift;
  const int64_t noise_size = rec.noise_size;

  // ---- spectral parameters of this pulse (synthesis.py:49-51,144-180) -------------------------
  // the two neighbouring frames and the interpolation weight, from pulse_frames_kernel
  const int64_t row_lo = rec.rows & 0xffffffffll, row_hi = rec.rows >> 32;
  const double bw = rec.weight;
  const bool same = bw < 0.0;
  const double b = same ? 0.0 : bw;
  const double a = 1 - b;
  const double* s_lo = spectrogram + row_lo * K;
  const double* s_hi = spectrogram + row_hi * K;
  const double* a_lo = aperiodicity + row_lo * K;
  const double* a_hi = aperiodicity + row_hi * K;
  // a thread's bins k = tid + q FT: all of their row loads are issued before the first log (a call: nothing is moved
  // across it), one global round trip per pulse instead of one per bin
  constexpr int KQ = (K + FT - 1) / FT;
  double rsl[KQ], rsh[KQ], ral[KQ], rah[KQ];
  const bool need_ap = rec.vuv != 0;  // (workgroup-uniform, known from the record)
#pragma unroll
  for (int q = 0; q < KQ; ++q) {
    const int k = WH_TID + q * FT;
    const int kc = k < K ? k : K - 1;  // (clamped: always a valid address; the surplus slot is not used)
    rsl[q] = s_lo[kc];
    rsh[q] = s_hi[kc];
    if constexpr (resp_skip_ap<N>()) {
      ral[q] = rah[q] = 0.0;
    } else {
      ral[q] = a_lo[kc];
      rah[q] = a_hi[kc];
    }
  }
  // aperiodic_slice[0] decides voicing (synthesis.py:69); its two loads ride with the rows' (issued first, they put
  // two more dependent round trips in front of the rows: the compiler waited for each before going on)
  double ap0_lo, ap0_hi;
  if constexpr (resp_skip_ap<N>()) {
    ap0_lo = ap0_hi = 0.0;
    if (need_ap) {
#pragma unroll
      for (int q = 0; q < KQ; ++q) {
        const int k = WH_TID + q * FT;
        const int kc = k < K ? k : K - 1;
        ral[q] = a_lo[kc];
        rah[q] = a_hi[kc];
      }
      ap0_lo = a_lo[0];
      ap0_hi = a_hi[0];
    }
  } else {
    ap0_lo = a_lo[0];
    ap0_hi = a_hi[0];
  }
  asm volatile("" : "+v"(ap0_lo), "+v"(ap0_hi));  // (both issued here: else the second is sunk behind the test of `same`)
  double aper0;
  {
    const double al = ap0_lo * ap0_lo, ah = ap0_hi * ap0_hi;
    aper0 = same ? al : a * al + b * ah;
  }
  const bool voiced = (rec.vuv != 0) && (aper0 <= 0.999);
  RSTAGE_COUNT(voiced ? kRsNVoiced : (rec.vuv == 0 ? kRsNUnvoicedVuv : kRsNUnvoicedRows))
  RSTAGE_COUNT(kRsNPulses)
#pragma unroll
  for (int q = 0; q < KQ; ++q) {
    const int k = WH_TID + q * FT;
    if (k >= K) break;
    const double sl = rsl[q], sh = rsh[q];
    double v, w;
    auto spectra = [&]() {
      double al = ral[q] * ral[q], ah = rah[q] * rah[q];
      // (behind the voiced test the compiler fuses each square into its 1 - x, one rounding less than the reference's
      // aperiodicity ** 2 and than this code took before the test: the squares stay values of their own)
      if constexpr (resp_skip_ap<N>()) asm volatile("" : "+v"(al), "+v"(ah));
      const double pl = fmax(0.001, 1 - al), ph = fmax(0.001, 1 - ah);
      const double sp = same ? sl : a * sl + b * sh;
      const double pe = same ? pl : a * pl + b * ph;
      const double ap = same ? al : a * al + b * ah;
      v = sp * pe;  // periodic spectrum
      if (v == 0.0) v = 2.220446049250313e-16;
      w = voiced ? sp * ap : sp;  // aperiodic spectrum
    };
    if constexpr (resp_skip_ap<N>()) {  // (an unvoiced pulse uses neither product: at the 16 kHz shape it skips the squares too)
      v = 0.0;
      w = same ? sl : a * sl + b * sh;
      if (voiced) spectra();
    } else {
      spectra();
    }
    if (w == 0.0) w = 2.220446049250313e-16;
    // log|.| / 2 of the Hermitian-mirrored spectrum (synthesis.py:103-105), written where the chain's first
    // transform reads it: no amplitude arrays, no separate log and mirror passes
    // (a voiced pulse's two logarithms through one call, like the pair of complex exponentials in min_phase_response)
    double2 lg;
    if (voiced) lg = log_pair_call(fabs(w), fabs(v));
    else lg = make_double2(log_call(fabs(w)), 0.0);
    const double lw = lg.x / 2;
    zrA[k] = lw;
    if (k > 0 && k < N / 2) zrA[N - k] = lw;
    if (voiced) {
      const double lv = lg.y / 2;
      zrP[k] = lv;
      if (k > 0 && k < N / 2) zrP[N - k] = lv;
    }
  }
  RSTAGE_MARK(kRsSetup)
  // ---- noise for this pulse: max(3, noise_size) samples, zero-mean (synthesis.py:93-95) -----------
  const int64_t nd = noise_size > 3 ? noise_size : 3;
  const int64_t noff = rec.noff;
  auto noise_at = [&](int64_t j) -> double {
    if (noise) {
      const int64_t q = noff + j;
      return q < m.noise_len ? noise[m.noise_off + q] : 0.0;
    }
    return normal_at(philox_key(seed, (uint64_t)u), (uint64_t)(noff + j));
  };
  // Where a chain's transforms run on one wave of its group (resp_wave_fft), the group's other waves have nothing to do
  // during them: a device-stream run that fits nz (the usual case) is generated THERE, by the waves that idle through the
  // first transform of the chains, and its mean is taken behind the chains — nothing reads either before the convolution.
  constexpr bool ROLES = resp_wave_fft<N>();  // (in front of the chains instead: DESIGN.md §4 round 10)
  static_assert(!ROLES || NZ / 2 + 1 <= FT, "a run that fits nz is at most one Philox block per thread");
  const bool side_noise = ROLES && noise == nullptr && nd <= NZ;  // (workgroup-uniform)
  // Thread i of the n side threads takes Philox block (noff >> 1) + i like thread i of the workgroup does in front of the
  // chains, so a side wave holds the partial sums of one wave of block_sum's tree: it leaves their sum in scratch[that
  // wave] (the chains do not touch scratch either), and the mean behind the chains adds the wave sums in wave order.
  auto noise_side = [&](int i, int n) {
    if (!side_noise) return;
    const uint64_t key = philox_key(seed, (uint64_t)u);
    const int lane = i & 63;
    const int64_t blk0 = noff >> 1, b1 = (noff + nd - 1) >> 1;
    for (int c = __builtin_amdgcn_readfirstlane(i - lane); blk0 + c <= b1; c += n) {  // (wave-uniform: wave_sum wants every lane)
      const int64_t blk = blk0 + c + lane;
      double part = 0.0;
      if (blk <= b1) {
        const double2 z = normal_pair(key, (uint64_t)blk);
        const int64_t j = 2 * blk - noff;  // -1 .. nd-1, nd <= NZ
        if (j >= 0) {
          part += z.x;
          nz[j] = z.x;
        }
        if (j + 1 < nd) {
          part += z.y;
          nz[j + 1] = z.y;
        }
      }
      part = wh::wave_sum(part);
      if (lane == 0) scratch[c >> 6] = part;
    }
  };
  double mean = 0.0;
  if (side_noise) {
    wh::sync<FT>();  // the log spectra are visible
  } else {
    double part = 0.0;
    if (noise) {
      for (int64_t j = WH_TID; j < nd; j += FT) {
        const double v = noise_at(j);
        part += v;
        if (j < NZ) nz[j] = v;  // the usual case nd <= NZ: generate / fetch each sample once
      }
    } else {
      // device stream: sample q of the utterance is one half of Philox block q >> 1 — walk the blocks the run touches
      const uint64_t key = philox_key(seed, (uint64_t)u);
      const int64_t b1 = (noff + nd - 1) >> 1;
      for (int64_t blk = (noff >> 1) + WH_TID; blk <= b1; blk += FT) {
        const double2 z = normal_pair(key, (uint64_t)blk);
        const int64_t j = 2 * blk - noff;  // index of the block's first half within this pulse's run (-1 .. nd-1)
        if (j >= 0) {
          part += z.x;
          if (j < NZ) nz[j] = z.x;
        }
        if (j + 1 < nd) {
          part += z.y;
          if (j + 1 < NZ) nz[j + 1] = z.y;
        }
      }
    }
    mean = wh::block_sum<FT>(part, scratch) / (double)nd;  // barriers: the log spectra and nz are visible
  }

  RSTAGE_MARK(kRsNoise)
  // ---- minimum-phase responses (synthesis.py:86-116): aperiodic chain on thread group 0, periodic chain on
  //      group 1, advancing through the same barrier phases (with a single group: one after the other) --------
  const double coef_pi = 2.0 * fs / N;  // coefficient = 2*pi*fs/N (synthesis.py:59), kept in units of pi
  if constexpr (ROLES) {
    // (one wave per chain transforms: waves 1 and 3 of a voiced pulse, waves 1 - 3 of an unvoiced one take the noise run)
    if (NG == 2 && voiced) {
      const int g = WH_TID / GT;
      min_phase_response<N, GT, true, resp_table_cis<N>()>(g == 0 ? zbA : zbP, tw_base, mt, g == 0 ? 0.0 : coef_pi * shift, SpectrumIdentity(), noise_side);
    } else {
      min_phase_response<N, FT, true, resp_table_cis<N>()>(zbA, tw_base, mt, 0.0, SpectrumIdentity(), noise_side);
      if (voiced) min_phase_response<N, FT, true, resp_table_cis<N>()>(zbP, tw_base, mt, coef_pi * shift);
    }
  } else if (NG == 2 && voiced) {
    const int g = WH_TID / GT;
    min_phase_response<N, GT, false, resp_table_cis<N>()>(g == 0 ? zbA : zbP, tw_base, mt, g == 0 ? 0.0 : coef_pi * shift);
  } else {
    // an unvoiced pulse has no periodic response (synthesis.py:69-75): one chain, on all the threads — 40 % of the
    // pulses of speech-like input (the 500 Hz default rate of unvoiced stretches) do half the transform work
    min_phase_response<N, FT, false, resp_table_cis<N>()>(zbA, tw_base, mt, 0.0);
    if (voiced) min_phase_response<N, FT, false, resp_table_cis<N>()>(zbP, tw_base, mt, coef_pi * shift);
  }
  RSTAGE_MARK(voiced ? kRsChainsVoiced : kRsChainsUnvoiced)
  if (side_noise) {
    // the mean of the run in block_sum's order: the wave sums the side waves left (visible behind the chains' last
    // barrier), added in wave order.  (A wave whose threads are all behind the run's last block adds 0.0 there: skipped.)
    const int n_blk = (int)(((noff + nd - 1) >> 1) - (noff >> 1)) + 1;
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < (NZ / 2 + 1 + 63) / 64; ++w)
      if (w * 64 < n_blk) t += scratch[w];
    mean = t / (double)nd;
  }
  // zrA[n] = N * aperiodic response, zrP[n] = N * periodic response (both before fftshift)
  for (int n = WH_TID; n < N; n += FT) rap[rap_index(n)] = zrA[(n + N / 2) & (N - 1)] / N;
  wh::sync<FT>();

  // y[m] = sum_j nz[j] * ra[m-j], m < N: each thread owns R consecutive outputs and slides an R-wide
  // register window over the response, two noise samples (one 16-byte LDS read each side) per step.
  double acc[R];
#pragma unroll
  for (int q = 0; q < R; ++q) acc[q] = 0.0;
  double acc8[resp_conv8<N>() ? 8 : 1];
#pragma unroll
  for (int q = 0; q < (resp_conv8<N>() ? 8 : 1); ++q) acc8[q] = 0.0;
  const int m0 = WH_TID * R;
  for (int64_t j0 = 0; j0 < nd; j0 += NZC) {
    const int cnt = (int)(nd - j0 < NZC ? nd - j0 : NZC);
    wh::sync<FT>();
    for (int j = WH_TID; j < NZ; j += FT) {
      double v = 0.0;
      if (j < cnt) v = (j0 == 0 ? nz[j] : noise_at(j0 + j)) - mean;
      nz[j] = v;  // zero padded to an even count
    }
    wh::sync<FT>();
    if constexpr (resp_conv8<N>()) {
      // EIGHT outputs per thread, the noise range of the chunk split over the two halves of the workgroup (round 6).
      // With four outputs per thread a block of 4 noise samples is 16 FMAs against four 16-byte LDS reads (two for the
      // noise, two for the new response group): 32 LDS cycles per 64 FMA cycles of a wave, and the CU's four SIMDs share ONE
      // LDS pipe (MI355X_MICROARCH.md) — twice what it can feed.  At 48 kHz, where a pulse's noise run is ~100-200 samples
      // against a 2048-sample response, the convolution was a third of the kernel (tools/resp_stage_timer.py 48000 16 60
      // 1.5 2.0) and LDS-bound.  Eight outputs per thread: the same four reads feed 32 FMAs.  Half h of the workgroup
      // takes the outputs m = 8 t .. 8 t + 7 (t = tid mod FT/2) over ITS half of the noise samples; the two partial sums
      // meet in LDS behind the loop.  Response samples travel as aligned groups of four through a ring of three register
      // groups: nothing is shifted.
      constexpr int HT = FT / 2;
      const int half_id = WH_TID / HT, t8 = WH_TID - half_id * HT;
      const int c_all = ((cnt + 11) / 12) * 12;              // (<= NZC = 252; nz is zero-padded to NZ)
      const int c_mid = ((c_all / 12 + 1) / 2) * 12;          // half 0: [0, c_mid), half 1: [c_mid, c_all)
      const int jb = half_id == 0 ? 0 : c_mid, je = half_id == 0 ? c_mid : c_all;
      auto load4 = [&](int base, double (&g)[4]) {  // base is a multiple of 4: all four valid or all in front of the response
        double2 v0 = make_double2(0.0, 0.0), v1 = make_double2(0.0, 0.0);
        if (base >= 0) {
          v0 = wh::ck_as<const double2>(rap + rap_index(base))[0];
          v1 = wh::ck_as<const double2>(rap + rap_index(base + 2))[0];
        }
        g[0] = v0.x; g[1] = v0.y; g[2] = v1.x; g[3] = v1.y;
      };
      // outputs q = 0..7 at noise step s = 0..3 read ra[mb + q - s]: hi = ra[mb+4 .. mb+7], mid = ra[mb .. mb+3], lo = ra[mb-4 .. mb-1]
      auto block4 = [&](int j, const double (&hi)[4], const double (&mid)[4], const double (&lo)[4]) {
#pragma unroll
        for (int sp = 0; sp < 4; sp += 2) {  // two noise samples at a time: one 16-byte read
          const double2 nn = wh::ck_as<const double2>(nz + (j + sp))[0];
#pragma unroll
          for (int sft = sp; sft < sp + 2; ++sft)
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              const int idx = q - sft;  // -3 .. 7
              acc8[q] = fma(sft == sp ? nn.x : nn.y, idx >= 4 ? hi[idx - 4] : (idx >= 0 ? mid[idx] : lo[idx + 4]), acc8[q]);
            }
        }
      };
      // Three register groups in a ring (a fourth, fetched a block ahead, cost 28 spilled registers and 26 GB of scratch
      // traffic per config-5 step): the group a block has finished with receives the next block's lowest samples.
      const int mb0 = t8 * 8 - (int)j0 - jb;  // response index of output 0 at the half's first noise sample
      double g0[4], g1[4], g2[4];
      load4(mb0 + 4, g0);
      load4(mb0, g1);
      load4(mb0 - 4, g2);
      for (int j = jb; j < je; j += 12) {
        const int mb = t8 * 8 - (int)j0 - j;
        block4(j, g0, g1, g2);
        load4(mb - 8, g0);
        block4(j + 4, g1, g2, g0);
        load4(mb - 12, g1);
        block4(j + 8, g2, g0, g1);
        load4(mb - 16, g2);
      }
    } else if constexpr (R <= 4) {
      // Aligned groups of R response samples around the thread's outputs: hi = ra[mb .. mb+R-1], lo = ra[mb-R .. mb-1],
      // mb = m0 - j0 - j.  A block of R noise samples needs exactly these two groups (output q at step s reads
      // ra[mb + q - s]); for the next block lo becomes hi and ONE new group is fetched — into the registers of the group
      // that just died, so nothing is ever shifted (the two-step version moved 2(R-1) doubles per pair of steps).
      // (response_pair runs the same form from noise_conv_groups; moving this copy there reschedules response_kernel<512>)
      auto load_group = [&](int base, double (&g)[R]) {  // base is a multiple of R: a group is all-valid or all before the start
  #pragma unroll
        for (int t = 0; t < R; t += 2) {
          double2 v = make_double2(0.0, 0.0);
          if (base >= 0) v = wh::ck_as<const double2>(rap + rap_index(base + t))[0];
          g[t] = v.x;
          g[t + 1] = v.y;
        }
      };
      auto block = [&](int j, const double (&hi)[R], const double (&lo)[R]) {
        double n[R];
  #pragma unroll
        for (int t = 0; t < R; t += 2) {
          const double2 v = wh::ck_as<const double2>(nz + (j + t))[0];
          n[t] = v.x;
          n[t + 1] = v.y;
        }
  #pragma unroll
        for (int sft = 0; sft < R; ++sft)
  #pragma unroll
          for (int q = 0; q < R; ++q) acc[q] = fma(n[sft], q - sft >= 0 ? hi[q - sft] : lo[R + q - sft], acc[q]);
      };
      double ga[R], gb[R];
      const int mb0 = m0 - (int)j0;
      load_group(mb0, ga);
      load_group(mb0 - R, gb);
      const int steps = ((cnt + 2 * R - 1) / (2 * R)) * (2 * R);  // nz is zero-padded up to NZ, a multiple of 2R
      for (int j = 0; j < steps; j += 2 * R) {
        block(j, ga, gb);
        load_group(mb0 - j - 2 * R, ga);
        block(j + R, gb, ga);
        load_group(mb0 - j - 3 * R, gb);
      }
    } else {
      // (R = 8, fft size 4096: the 64-FMA blocks of the shift-free form do not fit the register budget)
      double r[R];
  #pragma unroll
      for (int q = 0; q < R; ++q) {
        const int idx = m0 + q - (int)j0;
        r[q] = idx >= 0 ? rap[rap_index(idx)] : 0.0;
      }
      const int steps = (cnt + 1) & ~1;
      for (int j = 0; j < steps; j += 2) {
        const double2 nn = wh::ck_as<const double2>(nz + j)[0];
        const int inew = m0 - (int)j0 - j - 2;  // even: (ra[inew], ra[inew+1]) is an aligned pair
        double2 fresh = make_double2(0.0, 0.0);
        if (inew >= 0) fresh = wh::ck_as<const double2>(rap + rap_index(inew))[0];
  #pragma unroll
        for (int q = 0; q < R; ++q) acc[q] = fma(nn.x, r[q], acc[q]);
  #pragma unroll
        for (int q = R - 1; q > 0; --q) r[q] = r[q - 1];
        r[0] = fresh.y;  // ra[m0 - g - 1]
  #pragma unroll
        for (int q = 0; q < R; ++q) acc[q] = fma(nn.y, r[q], acc[q]);
  #pragma unroll
        for (int q = R - 1; q > 0; --q) r[q] = r[q - 1];
        r[0] = fresh.x;  // ra[m0 - g - 2]
      }
    }
  }

  if constexpr (resp_conv8<N>()) {
    // the two halves' partial sums meet: half 0 parks its eight outputs in the aperiodic chain's buffer, half 1 in the
    // padded response's (both free now), and every thread collects the four outputs the overlap-add expects of it
    constexpr int HT = FT / 2;
    const int half_id = WH_TID / HT, t8 = WH_TID - half_id * HT;
    wh::sync<FT>();  // every thread is done reading rap
    const wh::ckp<double> park = half_id == 0 ? zrA : rap;
#pragma unroll
    for (int q = 0; q < 8; q += 2) wh::ck_as<double2>(park + (t8 * 8 + q))[0] = make_double2(acc8[q], acc8[q + 1]);
    wh::sync<FT>();
#pragma unroll
    for (int q = 0; q < R; q += 2) {
      const double2 a = wh::ck_as<const double2>(zrA + (m0 + q))[0], b2 = wh::ck_as<const double2>(rap + (m0 + q))[0];
      acc[q] = a.x + b2.x;
      acc[q + 1] = a.y + b2.y;
    }
  }
  RSTAGE_MARK(kRsConv)
  // ---- DC removal of the periodic response (synthesis.py:72-73) ------------------------------------
  double dc_total = 0.0;
  const double gain = sqrt((double)(noise_size > 1 ? noise_size : 1));
  if (voiced) {
    double part = 0.0;
    for (int n = WH_TID; n < N; n += FT) part += zrP[n] / N;
    dc_total = wh::block_sum<FT>(part, scratch);
  }

  // ---- overlap-add with the reference's clipped fancy-index semantics (Q8), through the run's ring ----------
  const int64_t s1 = pidx - N / 2 + 1;  // 1-based index of this pulse's first tap
  ring_advance<N>(ring, rs, row, s1, m.ny);
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const int mm = m0 + q;
    const int64_t tgt = s1 + mm;
    double v = acc[q];
    // (the eight-output form reads the weight where it uses it: four values held across the convolution were registers it lacked)
    if (voiced) v += (zrP[(mm + N / 2) & (N - 1)] / N + (R <= 4 && !resp_conv8<N>() ? dcw[R <= 4 ? q : 0] : dc_base[mm]) * -dc_total) * gain;
    if (tgt < 1) continue;                    // clipped to 1 and overwritten by the in-range tap
    if (tgt < m.ny) ring[(int)(tgt & (N - 1))] += v;    // this thread is the only writer of its R slots
    else if (mm == N - 1) rs.last += v;                 // last duplicate wins on the high side: the last sample's share
  }
  RSTAGE_MARK(kRsOverlapAdd)
}

}  // namespace
