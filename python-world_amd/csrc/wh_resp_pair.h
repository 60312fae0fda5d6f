// Two consecutive unvoiced pulses of a run through the two chain buffers side by side (resp_pairs<N>(), wh_resp_types.h).
// Kept apart from response_pulse on purpose: a shared helper moved every instance of the kernel.
// Include after wh_resp_pulse.h (noise_conv_groups).
#pragma once

namespace {

// Whether two consecutive pulses of a run share the chains (response_pair): decided from their records alone, the same
// for every thread of the workgroup.
__device__ __forceinline__ bool resp_pairable(const RespArgs& A, int vuv0, int noise_size0, int vuv1, int noise_size1) {
  const int nd0 = noise_size0 > 3 ? noise_size0 : 3, nd1 = noise_size1 > 3 ? noise_size1 : 3;
  return vuv0 == 0 && vuv1 == 0 && A.noise == nullptr && nd0 + nd1 <= kRespNoise;
}

// Two consecutive UNVOICED pulses of a run (both records say vuv == 0, device-stream noise, both noise runs fit nz together)
// through the machinery of one voiced pulse.  An unvoiced pulse has the aperiodic chain only: alone, one of the workgroup's
// four waves transforms and the periodic chain's buffer lies idle — and the reference places unvoiced pulses every 2 ms, in
// long runs.  Here r0's chain runs in zbA on thread group 0 and r1's in zbP on group 1, in lockstep like a voiced pulse's
// two; waves 1 and 3 generate the two noise runs under the first transform.  Each chain is the plan it is alone (8-8-8 on
// one wave, the same bins per expression), each run takes the Philox blocks and forms its mean in the order it does alone,
// and the ring receives r0's taps, then r1's: the output has the bits of the one-by-one path.  The spectrogram rows are
// fetched once where both pulses interpolate the same pair of frames (the usual case: pulses 2 ms apart, frames 5 ms),
// the aperiodicity rows not at all.
template <int N>
__device__ __forceinline__ void response_pair(const RespArgs& A, const PulseRec& r0, const PulseRec& r1, char* smem, wh::ckp<double> ring,
                                              RunState& rs, wh::ckp<double> WH_RESTRICT row) {
#pragma clang fp contract(fast)
  const double* __restrict__ spectrogram = A.spectrogram;
  const double2* __restrict__ tw_raw = A.tw_base;
  asm volatile("" : "+s"(tw_raw));  // per pulse: no twiddle address / value of one pulse survives into the next
  const wh::ckp<const double2> tw_base = wh::ck_make(tw_raw, WH_TWIDDLE_ENTRIES, wh::WH_CK_TWIDDLE);
  const double* __restrict__ mt_raw = A.math_tab;
  asm volatile("" : "+s"(mt_raw));  // (likewise)
  const wh::ckp<const double> mt = wh::ck_make(mt_raw, wh::kMtEntries, wh::WH_CK_TABLE);
  constexpr int FT = ft_syn(N);
  constexpr int K = N / 2 + 1;
  constexpr int NZ = kRespNoise;
  constexpr int R = N / FT;
  constexpr int GT = FT / 2;
  static_assert(GT == 2 * WH_WAVE && R <= 4 && 2 * NZ <= N, "one side wave per chain; the staged noise fits the first chain's buffer");
  using L = RespLds<N>;
  static_assert(NZ == L::kNoiseLen, "the noise block of the layout is the chunk this function stages");
  const wh::ckp<double> lds_all = wh::ck_make(reinterpret_cast<double*>(smem), L::kPulse, wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> zrA = wh::ck_sub(lds_all, L::kChainA, L::kChainLen, wh::WH_CK_LDS_MAIN);  // r0's chain
  const wh::ckp<double2> zbA = wh::ck_as<double2>(zrA);
  const wh::ckp<double> zrP = wh::ck_sub(lds_all, L::kChainP, L::kChainLen, wh::WH_CK_LDS_AUX);   // r1's chain
  const wh::ckp<double2> zbP = wh::ck_as<double2>(zrP);
  const wh::ckp<double> rap = wh::ck_sub(lds_all, L::kRap, L::kRapLen, wh::WH_CK_LDS_OTHER);  // padded aperiodic response
  const wh::ckp<double> nz = wh::ck_sub(lds_all, L::kNoise, L::kNoiseLen, wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> scratch = wh::ck_sub(lds_all, L::kScratch, L::kScratchLen, wh::WH_CK_LDS_SCRATCH);

  RSTAGE_BEGIN
  wh::sync<FT>();
  const int u = r0.u;
  const int64_t ny = A.meta[u].ny;
  RSTAGE_COUNT(kRsNUnvoicedVuv) RSTAGE_COUNT(kRsNUnvoicedVuv) RSTAGE_COUNT(kRsNPairs) RSTAGE_COUNT(kRsNPulses) RSTAGE_COUNT(kRsNPulses)
  {  // ---- log spectra: the rows' registers die here, in front of the chains
    const bool same_rows = r0.rows == r1.rows;  // (workgroup-uniform)
    const double* s_lo0 = spectrogram + (r0.rows & 0xffffffffll) * K;
    const double* s_hi0 = spectrogram + (r0.rows >> 32) * K;
    const double* s_lo1 = spectrogram + (r1.rows & 0xffffffffll) * K;
    const double* s_hi1 = spectrogram + (r1.rows >> 32) * K;
    const bool same0 = r0.weight < 0.0, same1 = r1.weight < 0.0;
    const double b0 = same0 ? 0.0 : r0.weight, b1 = same1 ? 0.0 : r1.weight;
    const double a0 = 1 - b0, a1 = 1 - b1;
    constexpr int KQ = (K + FT - 1) / FT;
    double rl0[KQ], rh0[KQ], rl1[KQ], rh1[KQ];
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      const int k = WH_TID + q * FT;
      const int kc = k < K ? k : K - 1;  // (clamped: always a valid address; the surplus slot is not used)
      rl0[q] = s_lo0[kc];
      rh0[q] = s_hi0[kc];
    }
    if (same_rows) {
#pragma unroll
      for (int q = 0; q < KQ; ++q) {
        rl1[q] = rl0[q];
        rh1[q] = rh0[q];
      }
    } else {
#pragma unroll
      for (int q = 0; q < KQ; ++q) {
        const int k = WH_TID + q * FT;
        const int kc = k < K ? k : K - 1;
        rl1[q] = s_lo1[kc];
        rh1[q] = s_hi1[kc];
      }
    }
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      const int k = WH_TID + q * FT;
      if (k >= K) break;
      // an unvoiced pulse's aperiodic spectrum is the spectrogram's.  response_pulse's `a * sl + b * sh` is contracted to
      // fma(a, sl, b * sh); written as a sum here, the second pulse's came out as fma(b, sh, a * sl) — an ulp apart in a few
      // bins (1e-16 in the output) — so the form is spelled out
      double w0 = same0 ? rl0[q] : fma(a0, rl0[q], b0 * rh0[q]);
      double w1 = same1 ? rl1[q] : fma(a1, rl1[q], b1 * rh1[q]);
      if (w0 == 0.0) w0 = 2.220446049250313e-16;
      if (w1 == 0.0) w1 = 2.220446049250313e-16;
      const double2 lg = log_pair_call(fabs(w0), fabs(w1));  // (the two pulses' logarithms like a voiced pulse's two)
      const double l0 = lg.x / 2, l1 = lg.y / 2;
      zrA[k] = l0;
      zrP[k] = l1;
      if (k > 0 && k < N / 2) {
        zrA[N - k] = l0;
        zrP[N - k] = l1;
      }
    }
  }
  RSTAGE_MARK(kRsSetup)
  // ---- the two noise runs: r0's on wave 1 into nz[0, nd0), r1's on wave 3 into nz[nd0, nd0 + nd1); wave sums of the 64-block
  //      chunks in scratch[c / 64] and scratch[4 + c / 64] (response_pulse's noise_side: the same blocks, lanes and sums)
  const int nd0 = r0.noise_size > 3 ? r0.noise_size : 3, nd1 = r1.noise_size > 3 ? r1.noise_size : 3;  // nd0 + nd1 <= NZ
  const int64_t noff0 = r0.noff, noff1 = r1.noff;
  const uint64_t seed = A.seed;
  auto noise_side = [&](int i, int) {
    const uint64_t key = philox_key(seed, (uint64_t)u);
    const int lane = i & 63;
    const int p = __builtin_amdgcn_readfirstlane(i - lane) >> 6;  // the chain this side wave belongs to
    const int64_t noff = p == 0 ? noff0 : noff1;
    const int nd = p == 0 ? nd0 : nd1, at = p == 0 ? 0 : nd0;
    const int64_t blk0 = noff >> 1, b1 = (noff + nd - 1) >> 1;
    for (int c = 0; blk0 + c <= b1; c += 64) {
      const int64_t blk = blk0 + c + lane;
      double part = 0.0;
      if (blk <= b1) {
        const double2 z = normal_pair(key, (uint64_t)blk);
        const int j = (int)(2 * blk - noff);  // -1 .. nd-1
        if (j >= 0) {
          part += z.x;
          nz[at + j] = z.x;
        }
        if (j + 1 < nd) {
          part += z.y;
          nz[at + j + 1] = z.y;
        }
      }
      part = wh::wave_sum(part);
      if (lane == 0) scratch[4 * p + (c >> 6)] = part;
    }
  };
  wh::sync<FT>();  // the log spectra are visible
  RSTAGE_MARK(kRsNoise)
  {
    const int g = WH_TID / GT;
    min_phase_response<N, GT, true, resp_table_cis<N>()>(g == 0 ? zbA : zbP, tw_base, mt, 0.0, SpectrumIdentity(), noise_side);
  }
  RSTAGE_MARK(kRsChainsPair)
  // the means, each from its run's wave sums in wave order (response_pulse behind the chains)
  double mean0, mean1;
  {
    const int nb0 = (int)(((noff0 + nd0 - 1) >> 1) - (noff0 >> 1)) + 1, nb1 = (int)(((noff1 + nd1 - 1) >> 1) - (noff1 >> 1)) + 1;
    double t0 = 0.0, t1 = 0.0;
#pragma unroll
    for (int w = 0; w < (NZ / 2 + 1 + 63) / 64; ++w) {
      if (w * 64 < nb0) t0 += scratch[w];
      if (w * 64 < nb1) t1 += scratch[4 + w];
    }
    mean0 = t0 / (double)nd0;
    mean1 = t1 / (double)nd1;
  }
  // zrA[n] = N * r0's response, zrP[n] = N * r1's (both before fftshift).  r0's goes to the padded buffer; zrA is free then
  // and takes both zero-mean runs, each zero-padded to NZ: r0's at zrA[0, NZ), r1's at zrA[NZ, 2 NZ)
  for (int n = WH_TID; n < N; n += FT) rap[rap_index(n)] = zrA[(n + N / 2) & (N - 1)] / N;
  wh::sync<FT>();
  for (int j = WH_TID; j < NZ; j += FT) {
    zrA[j] = j < nd0 ? nz[j] - mean0 : 0.0;
    zrA[NZ + j] = j < nd1 ? nz[nd0 + j] - mean1 : 0.0;
  }
  wh::sync<FT>();
  const int m0 = WH_TID * R;
  // convolution and overlap-add, r0 then r1: the ring sees the additions in the order of the one-by-one path
  auto excite_and_add = [&](wh::ckp<double> nzb, int nd, int64_t pidx) {
    double acc[R];
#pragma unroll
    for (int q = 0; q < R; ++q) acc[q] = 0.0;
    noise_conv_groups<R>(rap, nzb, nd, m0, 0, acc);
    const int64_t s1 = pidx - N / 2 + 1;  // 1-based index of this pulse's first tap
    ring_advance<N>(ring, rs, row, s1, ny);
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int mm = m0 + q;
      const int64_t tgt = s1 + mm;
      if (tgt < 1) continue;                                   // clipped to 1 and overwritten by the in-range tap
      if (tgt < ny) ring[(int)(tgt & (N - 1))] += acc[q];      // this thread is the only writer of its R slots
      else if (mm == N - 1) rs.last += acc[q];                 // last duplicate wins on the high side: the last sample's share
    }
  };
  excite_and_add(zrA, nd0, r0.pidx);
  RSTAGE_MARK(kRsConv)
  wh::sync<FT>();  // every thread is done with r0's response; its taps are in the ring
  for (int n = WH_TID; n < N; n += FT) rap[rap_index(n)] = zrP[(n + N / 2) & (N - 1)] / N;
  wh::sync<FT>();
  excite_and_add(zrA + NZ, nd1, r1.pidx);
  RSTAGE_MARK(kRsOverlapAdd)
}

}  // namespace
