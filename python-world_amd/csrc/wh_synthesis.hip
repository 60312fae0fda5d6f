// Pulse-by-pulse overlap-add synthesis, batched: the spectral half.  Replaces synthesis() (world/synthesis.py:21-82) together
// with the time base (wh_timebase.hip: phase, pulse positions, per-pulse records).
//
//   response_kernel : one workgroup per pulse: interpolate the two neighbouring frames, build the
//                     minimum-phase periodic and aperiodic responses with six LDS FFTs
//                     (synthesis.py:86-116,144-180), excite the aperiodic one with zero-mean noise
//                     (direct convolution == the reference's truncated fftfilt), and scatter-add into
//                     y with the reference's clipped-index semantics.
#include "wh_host.h"
#include "wh_math.h"
// response_kernel walks a run of pulses in a loop and reads the thread index opaquely (wh_tid.h): with the plain index
// every per-thread LDS / twiddle address of the ~15 transform passes in the loop body is hoisted in front of the loop and
// kept alive across it (248 VGPRs, 2 waves per SIMD); the few integer instructions that are recomputed cost nothing
// next to 128 spare registers.
#include "wh_tid.h"
#include "wh_device.h"
#include "wh_syn_types.h"
#include "wh_minphase.h"

// -DWH_RESP_STAGE_TIMER: per-stage shader-clock cycles of response_kernel (thread 0 of every workgroup), read with
// wh_debug_resp_stages (tools/resp_stage_timer.py).
#ifdef WH_RESP_STAGE_TIMER
// Slots 0 - 5: stage cycles (2: the chains of voiced pulses); 6: the chains of unvoiced pulses, 7: those of pairs;
// 8 - 13 count pulses: voiced, unvoiced with vuv == 0, unvoiced by the aperiodicity rows only, vuv == 0 pulses whose
// successor in the run could share the chains with them (RSTAGE_COUNT in response_kernel), pairs taken, pulses in all.
__device__ unsigned long long g_resp_stage[16];
#define RSTAGE_BEGIN unsigned long long _t0 = __builtin_readcyclecounter();
#define RSTAGE_MARK(i) { __syncthreads(); if (threadIdx.x == 0) { const unsigned long long _t = __builtin_readcyclecounter(); atomicAdd(&g_resp_stage[i], _t - _t0); _t0 = _t; } }
#define RSTAGE_COUNT(i) { if (threadIdx.x == 0) atomicAdd(&g_resp_stage[i], 1ull); }
#else
#define RSTAGE_BEGIN
#define RSTAGE_MARK(i)
#define RSTAGE_COUNT(i)
#endif
namespace {
using wh::SynUtt;
using wh::PulseRec;
using wh::block_excl_scan_256;
using wh::first_pulse_at;

#ifndef WH_RESP_PAIR
#define WH_RESP_PAIR 1  // two consecutive unvoiced pulses of a run through the two chain buffers side by side (response_pair); 0: one by one
#endif
// The noise convolution with eight outputs per thread (see response_pulse), where it pays: the long noise runs of 44.1 / 48 kHz (config 5: response_kernel 41.8 -> 39.6 ms).  At 16 kHz a pulse's run
// is ~64 samples — two 16-sample rounds per half — and the prologue and the merge cost more than the reads they save
// (config 2: 3.43 -> 3.58 ms), so N = 1024 keeps four outputs per thread.
template <int N>
constexpr bool resp_conv8() { return N / ft_syn(N) == 4 && N >= 2048; }

// ---- counter-based normal generator (Philox-4x32-10 + Box-Muller) for the no-host-noise mode ----
__device__ __forceinline__ void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
  c1 = (uint32_t)p1;
  c3 = (uint32_t)p0;
  c0 = n0;
  c2 = n2;
}
__device__ __attribute__((noinline)) double normal_at(uint64_t seed, uint64_t q) {  // a call: see log_call, wh_minphase.h
  uint32_t c0 = (uint32_t)(q >> 1), c1 = (uint32_t)((q >> 1) >> 32), c2 = 0x9E3779B9u, c3 = 0x243F6A88u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const double u1 = ((double)c0 * 4294967296.0 + (double)c1 + 0.5) * (1.0 / 18446744073709551616.0);
  const double u2 = ((double)c2 * 4294967296.0 + (double)c3 + 0.5) * (1.0 / 18446744073709551616.0);
  const double rr = sqrt(-2.0 * log(u1));
  double s, c;
  sincospi(2 * u2, &s, &c);  // sin/cos(2*pi*u2) without the large-argument reduction path
  return (q & 1) ? rr * s : rr * c;
}

// Both normals of one Philox block (normal_at(seed, 2*blk) and normal_at(seed, 2*blk + 1), bit for bit): the pulse's
// noise run is generated block-wise, one Box-Muller evaluation per pair instead of one per sample.
__device__ __attribute__((noinline)) double2 normal_pair(uint64_t seed, uint64_t blk) {
  uint32_t c0 = (uint32_t)blk, c1 = (uint32_t)(blk >> 32), c2 = 0x9E3779B9u, c3 = 0x243F6A88u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const double u1 = ((double)c0 * 4294967296.0 + (double)c1 + 0.5) * (1.0 / 18446744073709551616.0);
  const double u2 = ((double)c2 * 4294967296.0 + (double)c3 + 0.5) * (1.0 / 18446744073709551616.0);
  const double rr = sqrt(-2.0 * log(u1));
  double s, c;
  sincospi(2 * u2, &s, &c);
  return make_double2(rr * c, rr * s);
}

// The stream key of utterance u under `seed` (response_kernel derives the same one).
__device__ __host__ __forceinline__ uint64_t philox_key(uint64_t seed, uint64_t u) {
  return seed * 0x9E3779B97F4A7C15ull + u * 0xD1B54A32D192ED03ull + 1;
}
// out[i] = sample q0 + i of utterance u's stream: what wh_philox_normals exposes, so that the device-noise decode can be
// checked sample by sample (tests/test_hip_synthesis.py: the dumped stream fed back as host noise, and to the oracle).
__global__ __launch_bounds__(256) void philox_dump_kernel(uint64_t seed, int32_t u, int64_t q0, int64_t n,
                                                          double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = normal_at(philox_key(seed, (uint64_t)u), (uint64_t)(q0 + i));
}
// Host-supplied noise must cover every draw of the utterance: the last pulse's offset + its run (synthesis.py:93).
__global__ __launch_bounds__(64) void noise_cover_kernel(const SynUtt* __restrict__ meta, const PulseRec* __restrict__ rec,
                                                         const int64_t* __restrict__ p_base, int n_utt,
                                                         int32_t* __restrict__ flags) {
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= n_utt) return;
  const int64_t count = p_base[u + 1] - p_base[u];
  if (count < 1) return;
  const PulseRec& r = rec[p_base[u] + count - 1];
  const int64_t need = r.noff + (r.noise_size > 3 ? r.noise_size : 3);
  if (meta[u].noise_len >= 0 && need > meta[u].noise_len) atomicOr(flags + WH_FLAG_NOISE_SHORT, 1);
}

// The chains' transforms on one wave each (mp_fft, wh_minphase.h): the 16 kHz shape.
template <int N>
constexpr bool resp_wave_fft() { return N == 1024; }
// A pulse whose record says vuv == 0 is unvoiced whatever the aperiodicity rows hold (synthesis.py:69), and an unvoiced
// pulse's aperiodic spectrum is the spectrogram's: at the 16 kHz shape such a pulse does not fetch the two aperiodicity
// rows.  The other lengths keep the code they had (they were not measured with it).
template <int N>
constexpr bool resp_skip_ap() { return resp_wave_fft<N>(); }

// padded index of the aperiodic response for the register-tiled convolution: 2 doubles of padding every 32
// keep the 16-byte pair reads of lanes that are 4..8 samples apart on different LDS banks
__device__ __forceinline__ int rap_index(int i) { return i + 2 * (i >> 5); }

// Everything one pulse needs (kernel arguments bundled so that the per-pulse body can be a real function).
struct RespArgs {
  const SynUtt* meta;
  const double* tp;
  const double* spectrogram;
  const double* aperiodicity;
  double fs;
  const PulseRec* p_rec;
  const int64_t* p_base;
  int n_utt;
  const double* noise;
  uint64_t seed;
  const double* dc_base;
  const double2* tw_base;
  double* rows;             // overlap-add rows of the runs (response_gather_kernel sums them into y)
  const int64_t* row_base;  // [B + 1]: where every utterance's region of `rows` begins (sized from ITS sample count)
  const int64_t* run_base;  // [n_utt + 1] first run of every utterance (pulse_run_base_kernel)
  const int64_t* row_off;   // [n_utt][runs_cap] where run r's row begins in the utterance's region (pulse_rows_kernel)
  int64_t runs_cap;
};

// Overlap-add of a workgroup's run of consecutive pulses OF ONE UTTERANCE: the run's contributions are accumulated, in
// pulse order, in an N-sample LDS ring that covers the window of the current pulse; when the window moves on, the
// samples that leave it are final for this run and go to the run's ROW (plain stores, zeros included) — row r of an
// utterance holds the sum of run r over the samples its pulses cover, and response_gather_kernel adds the rows that
// cover an output sample in run order.  No atomics anywhere: the decode is the same from run to run, and the same
// whether an utterance is decoded alone, in a batch or on another rank (runs are numbered per utterance).  The
// reference adds pulse after pulse into y (synthesis.py:67-81); summing runs of pulses first is another association
// of the same sum (1e-17 relative).
// Row layout (per utterance a region of row_base[u + 1] - row_base[u] doubles): the rows lie one behind the other, row r at row_off[r]
// (pulse_rows_kernel: an exclusive scan of the row lengths, which follow from the pulse positions); slot 0 = what the
// run adds to the LAST sample (Q8, below), slot 1 + (t - start_r) = its sum at the 1-based sample t < ny, start_r =
// max(1, first tap of the run's first pulse).  A region holds 12 doubles per output sample (a mean f0 up to ~fs / 16 at
// N = 1024); an utterance that needs more raises WH_FLAG_PULSE_OVERFLOW like one that runs out of pulse slots, and the
// retry with the safe pulse capacity sizes the region for it.
struct RunState {
  bool any;           // a pulse has been accumulated (the ring holds something)
  int64_t win_start;  // 1-based output index of the first sample of the ring's window
  int64_t row_start;  // start_r
  double last;        // thread FT-1: the run's contribution to the utterance's last sample
};
#ifndef WH_RESP_RUN
#define WH_RESP_RUN 0  // pulses per workgroup; 0: by transform length (resp_run below)
#endif

// Samples [a, b) (1-based, within the ring's current window) are final for this run: to the row, clear the ring.
template <int N>
__device__ __forceinline__ void ring_flush(wh::ckp<double> ring, int64_t a, int64_t b, wh::ckp<double> WH_RESTRICT row, int64_t row_start,
                                           int64_t ny) {
  constexpr int FT = ft_syn(N);
  a = a < 1 ? 1 : a;
  b = b > ny ? ny : b;
  for (int64_t tgt = a + WH_TID; tgt < b; tgt += FT) {
    const int slot = (int)(tgt & (N - 1));
    row[1 + (tgt - row_start)] = ring[slot];
    ring[slot] = 0.0;
  }
}

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

// The ring's window moves on to the pulse whose first tap is s1: what it leaves behind goes to the row.
template <int N>
__device__ __forceinline__ void ring_advance(wh::ckp<double> ring, RunState& rs, wh::ckp<double> WH_RESTRICT row, int64_t s1, int64_t ny) {
  constexpr int FT = ft_syn(N);
  if (rs.any) {
    const int64_t e = s1 < rs.win_start + N ? s1 : rs.win_start + N;  // the samples the window leaves behind
    ring_flush<N>(ring, rs.win_start, e, row, rs.row_start, ny);
    // (pulses more than N samples apart — f0 below fs / N: the samples between the two windows belong to the row too)
    for (int64_t tgt = rs.win_start + N + WH_TID; tgt < (s1 < ny ? s1 : ny); tgt += FT) row[1 + (tgt - rs.row_start)] = 0.0;
    wh::sync<FT>();
  } else {
    rs.row_start = s1 < 1 ? 1 : s1;
  }
  rs.any = true;
  rs.win_start = s1;
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
  constexpr int FT = ft_syn(N);
  constexpr int K = N / 2 + 1;
  constexpr int NZ = 256;
  constexpr int NZC = resp_conv8<N>() ? 252 : NZ;  // noise samples per chunk (the eight-output form walks them twelve at a time)
  constexpr int R = N / FT;  // consecutive output samples per thread
  static_assert(R % 2 == 0 && NZ % (2 * R) == 0, "pairwise reads; whole blocks of 2R noise samples");
  constexpr int GT = FT >= 256 ? FT / 2 : FT;  // threads per chain: the periodic and aperiodic chains run side by side
  constexpr int NG = FT / GT;
  // (wh::ckp<T> is T* in every shipped build; the bounds build checks each access against the range named here)
  const wh::ckp<double> lds_all = wh::ck_make(reinterpret_cast<double*>(smem), 2 * (N + 2) + (N + N / 16 + 2) + NZ + 32, wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> zrA = wh::ck_sub(lds_all, 0, N + 2, wh::WH_CK_LDS_MAIN);       // N/2+1 complex: aperiodic chain
  const wh::ckp<double2> zbA = wh::ck_as<double2>(zrA);
  const wh::ckp<double> zrP = wh::ck_sub(lds_all, N + 2, N + 2, wh::WH_CK_LDS_AUX);    // N/2+1 complex: periodic chain
  const wh::ckp<double2> zbP = wh::ck_as<double2>(zrP);
  const wh::ckp<double> rap = wh::ck_sub(lds_all, 2 * (N + 2), N + N / 16 + 2, wh::WH_CK_LDS_OTHER);  // padded aperiodic response
  const wh::ckp<double> nz = wh::ck_sub(lds_all, 2 * (N + 2) + (N + N / 16 + 2), NZ, wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> scratch = wh::ck_sub(lds_all, 2 * (N + 2) + (N + N / 16 + 2) + NZ, 32, wh::WH_CK_LDS_SCRATCH);

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
  RSTAGE_COUNT(voiced ? 8 : (rec.vuv == 0 ? 9 : 10))
  RSTAGE_COUNT(13)
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
  RSTAGE_MARK(5)
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

  RSTAGE_MARK(0)
  // ---- minimum-phase responses (synthesis.py:86-116): aperiodic chain on thread group 0, periodic chain on
  //      group 1, advancing through the same barrier phases (with a single group: one after the other) --------
  const double coef_pi = 2.0 * fs / N;  // coefficient = 2*pi*fs/N (synthesis.py:59), kept in units of pi
  if constexpr (ROLES) {
    // (one wave per chain transforms: waves 1 and 3 of a voiced pulse, waves 1 - 3 of an unvoiced one take the noise run)
    if (NG == 2 && voiced) {
      const int g = WH_TID / GT;
      min_phase_response<N, GT, true>(g == 0 ? zbA : zbP, tw_base, g == 0 ? 0.0 : coef_pi * shift, SpectrumIdentity(), noise_side);
    } else {
      min_phase_response<N, FT, true>(zbA, tw_base, 0.0, SpectrumIdentity(), noise_side);
      if (voiced) min_phase_response<N, FT, true>(zbP, tw_base, coef_pi * shift);
    }
  } else if (NG == 2 && voiced) {
    const int g = WH_TID / GT;
    min_phase_response<N, GT>(g == 0 ? zbA : zbP, tw_base, g == 0 ? 0.0 : coef_pi * shift);
  } else {
    // an unvoiced pulse has no periodic response (synthesis.py:69-75): one chain, on all the threads — 40 % of the
    // pulses of speech-like input (the 500 Hz default rate of unvoiced stretches) do half the transform work
    min_phase_response<N, FT>(zbA, tw_base, 0.0);
    if (voiced) min_phase_response<N, FT>(zbP, tw_base, coef_pi * shift);
  }
  RSTAGE_MARK(voiced ? 2 : 6)
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
  RSTAGE_MARK(3)
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
  RSTAGE_MARK(4)
}

// Whether two consecutive pulses of a run share the chains (response_pair): decided from their records alone, the same
// for every thread of the workgroup.
template <int N>
constexpr bool resp_pairs() { return WH_RESP_PAIR && resp_wave_fft<N>() && ft_syn(N) == 256; }
__device__ __forceinline__ bool resp_pairable(const RespArgs& A, int vuv0, int noise_size0, int vuv1, int noise_size1) {
  const int nd0 = noise_size0 > 3 ? noise_size0 : 3, nd1 = noise_size1 > 3 ? noise_size1 : 3;
  return vuv0 == 0 && vuv1 == 0 && A.noise == nullptr && nd0 + nd1 <= 256;
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
  constexpr int FT = ft_syn(N);
  constexpr int K = N / 2 + 1;
  constexpr int NZ = 256;
  constexpr int R = N / FT;
  constexpr int GT = FT / 2;
  static_assert(GT == 2 * WH_WAVE && R <= 4 && 2 * NZ <= N, "one side wave per chain; the staged noise fits the first chain's buffer");
  // (the LDS layout of response_pulse)
  const wh::ckp<double> lds_all = wh::ck_make(reinterpret_cast<double*>(smem), 2 * (N + 2) + (N + N / 16 + 2) + NZ + 32, wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> zrA = wh::ck_sub(lds_all, 0, N + 2, wh::WH_CK_LDS_MAIN);     // r0's chain
  const wh::ckp<double2> zbA = wh::ck_as<double2>(zrA);
  const wh::ckp<double> zrP = wh::ck_sub(lds_all, N + 2, N + 2, wh::WH_CK_LDS_AUX);  // r1's chain
  const wh::ckp<double2> zbP = wh::ck_as<double2>(zrP);
  const wh::ckp<double> rap = wh::ck_sub(lds_all, 2 * (N + 2), N + N / 16 + 2, wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> nz = wh::ck_sub(lds_all, 2 * (N + 2) + (N + N / 16 + 2), NZ, wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> scratch = wh::ck_sub(lds_all, 2 * (N + 2) + (N + N / 16 + 2) + NZ, 32, wh::WH_CK_LDS_SCRATCH);

  RSTAGE_BEGIN
  wh::sync<FT>();
  const int u = r0.u;
  const int64_t ny = A.meta[u].ny;
  RSTAGE_COUNT(9) RSTAGE_COUNT(9) RSTAGE_COUNT(12) RSTAGE_COUNT(13) RSTAGE_COUNT(13)
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
  RSTAGE_MARK(5)
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
  RSTAGE_MARK(0)
  {
    const int g = WH_TID / GT;
    min_phase_response<N, GT, true>(g == 0 ? zbA : zbP, tw_base, 0.0, SpectrumIdentity(), noise_side);
  }
  RSTAGE_MARK(7)
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
  RSTAGE_MARK(3)
  wh::sync<FT>();  // every thread is done with r0's response; its taps are in the ring
  for (int n = WH_TID; n < N; n += FT) rap[rap_index(n)] = zrP[(n + N / 2) & (N - 1)] / N;
  wh::sync<FT>();
  excite_and_add(zrA + NZ, nd1, r1.pidx);
  RSTAGE_MARK(4)
}

// Pulses per workgroup: 6 up to N = 1024, 8 beyond (measured with the pulse record prefetch in place: 4 / 5 / 6 / 7 / 8 /
// 12 / 16 pulses 3.414 / 3.416 / 3.417 / 3.449 / 3.46 / 3.51 / 3.59 ms at config 2; at 48 kHz, N = 2048, 5 pulses 42.5
// against 41.6 ms for 8: the flush of the longer ring is what a short run does not amortise).
constexpr int resp_run(int n) { return WH_RESP_RUN > 0 ? WH_RESP_RUN : (n <= 1024 ? 6 : 8); }

// First run of every utterance: runs never straddle utterances, so that what a run sums does not depend on the
// utterance's position in the batch.
__global__ void pulse_run_base_kernel(const int32_t* __restrict__ p_count, int n_utt, int run, int64_t* __restrict__ base) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int64_t at = 0;
    for (int u = 0; u < n_utt; ++u) {
      base[u] = at;
      at += (p_count[u] + run - 1) / run;
    }
    base[n_utt] = at;
  }
}

// Where every run's row begins in its utterance's region: row r holds 1 + (end_r - start_r) doubles (RunState), the rows
// lie one behind the other.  One workgroup per utterance scans its runs in chunks of 256.  A row that does not fit the
// region gets offset -1 (its run is skipped, its samples are not gathered) and raises WH_FLAG_PULSE_OVERFLOW.
template <int N>
__global__ __launch_bounds__(256) void pulse_rows_kernel(const SynUtt* __restrict__ meta, const int64_t* __restrict__ p_idx,
                                                         const int32_t* __restrict__ p_count, int64_t runs_cap,
                                                         const int64_t* __restrict__ row_base, int64_t* __restrict__ row_off,
                                                         int32_t* __restrict__ flags) {
  constexpr int RUN = resp_run(N);
  __shared__ int wsum[4];
  const SynUtt m = meta[blockIdx.x];
  const int count = p_count[blockIdx.x];
  const int64_t* pi = p_idx + m.p_off;
  const int n_runs = (count + RUN - 1) / RUN;
  int64_t* out = row_off + (int64_t)blockIdx.x * runs_cap;
  int64_t carry = 0;
  bool over = false;
  const int64_t room = row_base[blockIdx.x + 1] - row_base[blockIdx.x];
  for (int base = 0; base < n_runs; base += 256) {
    const int r = base + threadIdx.x;
    int len = 0;
    if (r < n_runs) {
      const int kf = r * RUN;
      const int kl = (kf + RUN < count ? kf + RUN : count) - 1;
      int64_t start = pi[kf] - N / 2 + 1, end = pi[kl] + N / 2 + 1;
      start = start < 1 ? 1 : start;
      end = end < m.ny ? end : m.ny;
      len = 1 + (int)(end > start ? end - start : 0);
    }
    int total;
    const int excl = block_excl_scan_256(len, wsum, &total);
    if (r < n_runs) {
      const int64_t at = carry + excl;
      const bool fits = at + len <= room;
      out[r] = fits ? at : -1;
      over = over || !fits;
    }
    carry += total;
    __syncthreads();  // wsum is reused by the next chunk
  }
  if (over) atomicOr(flags + WH_FLAG_PULSE_OVERFLOW, 1);
}

// One workgroup per RUN of resp_run(N) consecutive pulses of one utterance (runs numbered utterance by utterance, in
// time order).  The grid is sized from the host's pulse capacity; the runs that exist (device-side pulse counts) are
// dealt to the XCDs in contiguous ranges, so that the spectrogram / aperiodicity rows neighbouring pulses share are
// fetched into one L2 — the surplus workgroups exit at once.
template <int N>
__global__ __launch_bounds__(ft_syn(N), 4) void response_kernel(RespArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int FT = ft_syn(N);
  constexpr int RUN = resp_run(N);
  const int64_t n_runs = A.run_base[A.n_utt];
  const int64_t run = wh::xcd_unit(blockIdx.x, n_runs);
  if (run >= n_runs) return;
  int u = 0;
  {  // the utterance of this run: last u with run_base[u] <= run (scalar loads, block-uniform)
    int lo = 0, hi = A.n_utt;  // run_base[lo] <= run < run_base[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (A.run_base[mid] <= run) lo = mid; else hi = mid;
    }
    u = lo;
  }
  const int64_t r_in_utt = run - A.run_base[u];
  const wh::ckp<double> ring = wh::ck_make(reinterpret_cast<double*>(smem) + (2 * (N + 2) + (N + N / 16 + 2) + 256 + 32), N, wh::WH_CK_LDS_OTHER);
  for (int i = threadIdx.x; i < N; i += FT) ring[i] = 0.0;
  RunState rs{false, 0, 1, 0.0};
  const int64_t gp0 = A.p_base[u] + r_in_utt * RUN;
  const int64_t gp1 = gp0 + RUN < A.p_base[u + 1] ? gp0 + RUN : A.p_base[u + 1];
  const int64_t my_off = A.row_off[(int64_t)u * A.runs_cap + r_in_utt];
  if (my_off < 0) return;  // the utterance's row region is full (flagged by pulse_rows_kernel)
  // slot i of the row at row[i]; what is left of the utterance's region behind the row's start is the range it may touch
  const wh::ckp<double> row = wh::ck_make(A.rows + A.row_base[u] + my_off, A.row_base[u + 1] - A.row_base[u] - my_off, wh::WH_CK_OUT);
  // A pulse's record travels as ONE dword per lane (lane i & 15 holds dword i) and is turned into scalars by
  // v_readlane at the top of the pulse that uses it — a pulse after its load was issued.  Fetched as a struct the
  // compiler made scalars of it (readfirstlane) right behind the load: the "prefetch" was waited for at once.
  auto fetch_rec = [&](int64_t gp) -> uint32_t {
    return reinterpret_cast<const uint32_t*>(A.p_rec + gp)[threadIdx.x & 15];
  };
  auto unpack_rec = [&](uint32_t word) -> PulseRec {
    uint32_t d[16];
#pragma unroll
    for (int i = 0; i < 13; ++i) d[i] = (uint32_t)__builtin_amdgcn_readlane((int)word, i);
    PulseRec r;
    r.pidx = (int64_t)(((uint64_t)d[1] << 32) | d[0]);
    r.rows = (int64_t)(((uint64_t)d[3] << 32) | d[2]);
    r.weight = __hiloint2double((int)d[5], (int)d[4]);
    r.shift = __hiloint2double((int)d[7], (int)d[6]);
    r.noff = (int64_t)(((uint64_t)d[9] << 32) | d[8]);
    r.u = (int32_t)d[10];
    r.noise_size = (int32_t)d[11];
    r.vuv = (int32_t)d[12];
    r.pad_[0] = r.pad_[1] = r.pad_[2] = 0;
    return r;
  };
  uint32_t cur_w = fetch_rec(gp0);
  // the DC-removal weights of this thread's R output samples are the same for every pulse: read once per run (R <= 4;
  // beyond that they would cost the registers the convolution needs)
  constexpr int R = N / FT;
  double dcw[R <= 4 ? R : 1];
  if constexpr (R <= 4) {
#pragma unroll
    for (int q = 0; q < R; ++q) dcw[q] = A.dc_base[threadIdx.x * R + q];
  } else {
    dcw[0] = 0.0;
  }
  // the row's first sample is known from the run's first pulse: max(1, its first tap)
  int64_t row_start;
  {
    const int64_t pidx0 = reinterpret_cast<const int64_t*>(A.p_rec + gp0)[0];
    row_start = pidx0 - N / 2 + 1;
    row_start = row_start < 1 ? 1 : row_start;
  }
  (void)row_start;
  if constexpr (resp_pairs<N>()) {
    // Two records travel: the pulse's own and its successor's, whose vuv and noise_size decide — with the pulse's — whether
    // the two go through the chains together (response_pair).  A pair fetches the records two and three pulses ahead, a
    // single pulse the one two ahead: every record is still read out a pulse or more after its load was issued.
    uint32_t nxt_w = fetch_rec(gp0 + 1 < gp1 ? gp0 + 1 : gp0);
#pragma unroll 1
    for (int64_t gp = gp0; gp < gp1;) {
      const PulseRec cur = unpack_rec(cur_w);
      const int64_t last = gp1 - 1;
      bool pair = false;
      if (gp + 1 < gp1)
        pair = resp_pairable(A, cur.vuv, cur.noise_size, __builtin_amdgcn_readlane((int)nxt_w, 12), __builtin_amdgcn_readlane((int)nxt_w, 11));
      if (pair) {
        const PulseRec nxt = unpack_rec(nxt_w);
        const uint32_t w2 = fetch_rec(gp + 2 < last ? gp + 2 : last), w3 = fetch_rec(gp + 3 < last ? gp + 3 : last);
        response_pair<N>(A, cur, nxt, smem, ring, rs, row);
        cur_w = w2;
        nxt_w = w3;
        gp += 2;
      } else {
        const uint32_t w2 = fetch_rec(gp + 2 < last ? gp + 2 : last);
        response_pulse<N>(A, cur, smem, ring, rs, row, dcw);
        cur_w = nxt_w;
        nxt_w = w2;
        gp += 1;
      }
    }
  } else {
#pragma unroll 1
    for (int64_t gp = gp0; gp < gp1; ++gp) {
      const PulseRec cur = unpack_rec(cur_w);
      const uint32_t nxt_w = fetch_rec(gp + 1 < gp1 ? gp + 1 : gp);  // in flight under this whole pulse
#ifdef WH_RESP_STAGE_TIMER
      if (gp + 1 < gp1 && resp_pairable(A, cur.vuv, cur.noise_size, __builtin_amdgcn_readlane((int)nxt_w, 12), __builtin_amdgcn_readlane((int)nxt_w, 11)))
        RSTAGE_COUNT(11)
#endif
      response_pulse<N>(A, cur, smem, ring, rs, row, dcw);
      cur_w = nxt_w;
    }
  }
  wh::sync<FT>();
  if (rs.any) ring_flush<N>(ring, rs.win_start, rs.win_start + N, row, rs.row_start, A.meta[u].ny);
  if (threadIdx.x == FT - 1) row[0] = rs.last;
}

// y[t] = sum of the rows that cover t, in run order (see RunState): one thread per output sample.  The runs whose
// pulses reach a tile of 256 samples follow from the utterance's ascending pulse indices (the wave search of the
// Requiem excitation); a run's extent from its first and last pulse.  The utterance's LAST sample receives, of every
// pulse whose window reaches it or beyond, the last tap only (the reference's clipped fancy-index assignment keeps the
// last of the duplicates, Q8): the rows' slot 0.
#ifndef WH_GATHER_PER
#define WH_GATHER_PER 4
#endif
constexpr int kGatherTile = 256 * WH_GATHER_PER;  // output samples per workgroup: one pulse search for all of them
template <int N>
__global__ __launch_bounds__(256) void response_gather_kernel(const SynUtt* __restrict__ meta,
                                                              const int64_t* __restrict__ p_idx,
                                                              const int32_t* __restrict__ p_count,
                                                              const double* __restrict__ rows, const int64_t* __restrict__ row_base,
                                                              const int64_t* __restrict__ row_off, int64_t runs_cap,
                                                              double* __restrict__ y) {
  constexpr int RUN = resp_run(N);
  constexpr int PER = WH_GATHER_PER;
  const SynUtt m = meta[blockIdx.y];
  const int64_t n0 = (int64_t)blockIdx.x * kGatherTile;
  if (n0 >= m.ny) return;
  const int count = p_count[blockIdx.y];
  const int64_t* pi = p_idx + m.p_off;
  const double* ru = rows + row_base[blockIdx.y];
  const int64_t* ro = row_off + (int64_t)blockIdx.y * runs_cap;
  // pulses whose window [pidx - N/2 + 1, pidx + N/2] reaches the tile's samples n0 + 1 .. n0 + kGatherTile
  const int k0 = first_pulse_at(pi, count, n0 + 1 - N / 2);
  const int n_runs = (count + RUN - 1) / RUN;
  double sum[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) sum[q] = 0.0;
  const int64_t t0 = n0 + 1 + threadIdx.x;  // this thread's samples: t0 + 256 q (1-based)
  for (int r = k0 / RUN; r < n_runs; ++r) {
    const int kf = r * RUN;
    const int kl = (kf + RUN < count ? kf + RUN : count) - 1;
    const int64_t s1f = pi[kf] - N / 2 + 1;
    if (s1f > n0 + kGatherTile) break;
    const int64_t start = s1f < 1 ? 1 : s1f;
    int64_t end = pi[kl] + N / 2 + 1;  // one behind the last tap of the run's last pulse ...
    end = end < m.ny ? end : m.ny;     // ... and the last sample takes the rows' slot 0 only (below)
    const int64_t off = ro[r];
    if (off < 0) continue;  // (dropped: the region was full — flagged)
    const double* rr = ru + off + 1 - start;  // sample t of the run at rr[t]: slot 1 + (t - start)
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int64_t tgt = t0 + 256 * q;
      if (tgt >= start && tgt < end) sum[q] += rr[tgt];
    }
  }
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int64_t tgt = t0 + 256 * q;
    if (tgt < m.ny) y[m.y_off + tgt - 1] = sum[q];
  }
  if (n0 + kGatherTile >= m.ny) {  // the tile that holds the utterance's last sample: block-uniform
    const int k_end = first_pulse_at(pi, count, m.ny - N / 2);  // first pulse whose last tap reaches the last sample
    if (threadIdx.x == 0) {
      double last = 0.0;
      for (int r = k_end / RUN; r < n_runs; ++r) {
        const int64_t off = ro[r];
        if (off >= 0) last += ru[off];
      }
      y[m.y_off + m.ny - 1] = last;
    }
  }
}


template <int N>
int launch_resp(wh_ctx* ctx, hipStream_t st, int B, int64_t pcap_max, int64_t max_ny, const std::vector<int64_t>& h_ny, const SynUtt* d_meta, const double* tp,
                const double* spec, const double* ap, double fs, const PulseRec* p_rec, const int64_t* p_base,
                const int64_t* p_idx, const int32_t* p_count, const double* noise, uint64_t seed, double* y) {
  std::vector<double> dc(N);
  double sum = 0.0;
  for (int n = 0; n < N; ++n) {  // hanning(N+2)[1:-1] normalised (synthesis.py:57-58)
    dc[n] = 0.5 - 0.5 * cos(2.0 * M_PI * (double)(n + 1) / (double)(N + 1));
    sum += dc[n];
  }
  for (int n = 0; n < N; ++n) dc[n] /= sum;
  const double* d_dc = nullptr;
  if (int rc = wh::const_table(ctx, "dc_base:" + std::to_string(N), dc, &d_dc)) return rc;
  const size_t lds = sizeof(double) * (2 * (N + 2) + (N + N / 16 + 2) + 256 + 32 + N);  // ... + the overlap-add ring
  if (int rc = wh::allow_lds(&response_kernel<N>, lds)) return rc;
  // overlap-add rows (RunState): per utterance ceil(pcap / RUN) rows of N + 1 slots laid along the time axis.  Held in a
  // buffer of its own, not in the arena: the render reserves no workspace (the time base may live in this context's)
  const int64_t runs_cap = (pcap_max + resp_run(N) - 1) / resp_run(N);
  // doubles per output sample in an utterance's row region: 12 with the default pulse capacity (ny / 8) — the rows take
  // 6.2 where the reference places its 500 Hz unvoiced pulses at 16 kHz, 5 at a voiced 400 Hz, 12 at ~1 kHz — up to 48 with
  // the safe capacity of the retry (ny / 2: f0 up to fs / 4 at N = 1024)
  int64_t per_sample = (96 * pcap_max + max_ny - 1) / (max_ny > 0 ? max_ny : 1);
  per_sample = per_sample < 12 ? 12 : (per_sample > 48 ? 48 : per_sample);
  // every utterance's region from ITS OWN sample count (sized from the longest utterance a ragged batch held
  // max_ny per utterance, ~1 GB per 64 x 10 s whatever the other lengths were)
  std::vector<int64_t> row_base((size_t)B + 1, 0);
  for (int u = 0; u < B; ++u) row_base[u + 1] = row_base[u] + per_sample * h_ny[u] + 4 * (N + 1);
  int64_t* d_row_base = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "syn.row_base", row_base, &d_row_base)) return rc;
  void* d_rows = nullptr;
  void* d_rb = nullptr;
  void* d_ro = nullptr;
  if (int rc = wh::persistent_scratch(ctx, "syn.ola_rows", sizeof(double) * (size_t)row_base[B], &d_rows)) return rc;
  if (int rc = wh::persistent_scratch(ctx, "syn.run_base", sizeof(int64_t) * ((size_t)B + 1), &d_rb)) return rc;
  if (int rc = wh::persistent_scratch(ctx, "syn.row_off", sizeof(int64_t) * (size_t)runs_cap * B, &d_ro)) return rc;
  { wh::KernelTimer _kt(ctx, st, "pulse_run_base_kernel"); hipLaunchKernelGGL(pulse_run_base_kernel, dim3(1), dim3(64), 0, st, p_count, B, resp_run(N), reinterpret_cast<int64_t*>(d_rb)); }
  WH_LAUNCH_CHECK("pulse_run_base_kernel");
  { wh::KernelTimer _kt(ctx, st, "pulse_rows_kernel"); hipLaunchKernelGGL(pulse_rows_kernel<N>, dim3(B), dim3(256), 0, st, d_meta, p_idx, p_count, runs_cap, d_row_base, reinterpret_cast<int64_t*>(d_ro), ctx->d_flags); }
  WH_LAUNCH_CHECK("pulse_rows_kernel");
  // one workgroup per run of resp_run(N) pulse slots; runs past the real pulse count exit at once
  const int64_t grid = wh::xcd_grid(runs_cap * B);
  { wh::KernelTimer _kt(ctx, st, "response_kernel"); RespArgs ra{d_meta, tp, spec, ap, fs, p_rec, p_base, B, noise, seed, d_dc, ctx->d_twiddle, reinterpret_cast<double*>(d_rows), d_row_base, reinterpret_cast<const int64_t*>(d_rb), reinterpret_cast<const int64_t*>(d_ro), runs_cap};
  hipLaunchKernelGGL(response_kernel<N>, dim3((unsigned)grid), dim3(ft_syn(N)), lds, st, ra); }
  WH_LAUNCH_CHECK("response_kernel");
  { wh::KernelTimer _kt(ctx, st, "response_gather_kernel"); hipLaunchKernelGGL(response_gather_kernel<N>, dim3((unsigned)((max_ny + kGatherTile - 1) / kGatherTile), B), dim3(256), 0, st, d_meta, p_idx, p_count, reinterpret_cast<const double*>(d_rows), d_row_base, reinterpret_cast<const int64_t*>(d_ro), runs_cap, y); }
  WH_LAUNCH_CHECK("response_gather_kernel");
  return 0;
}


}  // namespace

// The spectral part: one response per pulse of the time base held by `timebase_ctx` (this context or another one of the
// same device), overlap-added into y.  Stream order (or an event the caller waits on) must put it behind that time base.
extern "C" int wh_synthesis_render(wh_ctx* ctx, void* stream, const wh_batch* b, const wh_ctx* timebase_ctx,
                                   const double* tp, const double* spectrogram, const double* aperiodicity, double fs,
                                   int fft_size, const int64_t* h_y_off, const double* h_t0, const double* h_dt,
                                   int64_t pulse_cap, const double* noise, const int64_t* h_noise_off, uint64_t seed,
                                   double* y, int32_t* pulse_count_out) {
  if (!ctx || !b || !timebase_ctx || !tp || !spectrogram || !aperiodicity || !h_y_off || !h_t0 || !h_dt || !y)
    return wh::fail_msg("wh_synthesis_render", "null argument");
  WH_ENTER(ctx);
  if (noise && !h_noise_off) return wh::fail_msg("wh_synthesis_render", "noise given without h_noise_off");
  hipStream_t st = (hipStream_t)stream;
  const int B = b->n_utt;
  const wh_ctx::TimeBase& t = timebase_ctx->timebase;
  if (!t.valid || t.n_utt != B || t.pulse_cap != pulse_cap || t.ny_tot != h_y_off[B] || t.frames != b->total_frames ||
      timebase_ctx->device != ctx->device)
    return wh::fail_msg("wh_synthesis_render", "no matching time base in timebase_ctx (run wh_synthesis_timebase on it "
                                               "with the same batch, lengths and pulse_cap, and nothing else since)");
  std::vector<SynUtt> meta;
  int64_t max_ny = 0;
  if (int rc = wh::fill_syn_meta("wh_synthesis_render", b, h_y_off, h_t0, h_dt, pulse_cap, noise, h_noise_off, meta, &max_ny)) return rc;
  const char* ws = reinterpret_cast<const char*>(timebase_ctx->ws);
  SynUtt* d_meta = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "syn.meta", meta, &d_meta)) return rc;
  const int64_t* d_pb = reinterpret_cast<const int64_t*>(ws + t.o_pb);
  const int64_t* d_pi = reinterpret_cast<const int64_t*>(ws + t.o_pi);
  const PulseRec* d_rec = reinterpret_cast<const PulseRec*>(ws + t.o_rec);
  const int32_t* d_pc = reinterpret_cast<const int32_t*>(ws + t.o_pc);
  if (noise) {  // (the time base knows nothing about the noise stream: the cover test belongs to the call that is given one)
    wh::KernelTimer _kt(ctx, st, "noise_cover_kernel");
    hipLaunchKernelGGL(noise_cover_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, d_meta, d_rec, d_pb, B, ctx->d_flags);
  }
  WH_LAUNCH_CHECK("noise_cover_kernel");
  std::vector<int64_t> h_ny((size_t)B);
  for (int u = 0; u < B; ++u) h_ny[u] = meta[u].ny;
  int rc = 0;
  if (!wh::dispatch_fft_size(fft_size, [&](auto n) {
        rc = launch_resp<decltype(n)::value>(ctx, st, B, pulse_cap, max_ny, h_ny, d_meta, tp, spectrogram, aperiodicity, fs, d_rec, d_pb, d_pi, d_pc, noise, seed, y);
      }))
    return wh::fail_msg("wh_synthesis_render", "fft_size must be a power of two in [512, 4096]");
  if (rc) return rc;
  if (pulse_count_out) WH_CHECK(hipMemcpyAsync(pulse_count_out, d_pc, sizeof(int32_t) * B, hipMemcpyDeviceToDevice, st));
  return 0;
}

extern "C" int wh_synthesis(wh_ctx* ctx, void* stream, const wh_batch* b, const double* tp, const double* f0,
                            const double* vuv, const double* spectrogram, const double* aperiodicity, double fs,
                            int fft_size, const int64_t* h_y_off, const double* h_t0, const double* h_dt,
                            int64_t pulse_cap, const double* noise, const int64_t* h_noise_off, uint64_t seed, double* y,
                            int32_t* pulse_count_out) {
  if (!ctx || !b || !tp || !f0 || !vuv || !spectrogram || !aperiodicity || !h_y_off || !h_t0 || !h_dt || !y)
    return wh::fail_msg("wh_synthesis", "null argument");
  if (noise && !h_noise_off) return wh::fail_msg("wh_synthesis", "noise given without h_noise_off");
  if (!wh::dispatch_fft_size(fft_size, [](auto) {}))
    return wh::fail_msg("wh_synthesis", "fft_size must be a power of two in [512, 4096]");
  if (int rc = wh_synthesis_timebase(ctx, stream, b, tp, f0, vuv, fs, h_y_off, h_t0, h_dt, pulse_cap, 0.0)) return rc;
  return wh_synthesis_render(ctx, stream, b, ctx, tp, spectrogram, aperiodicity, fs, fft_size, h_y_off, h_t0, h_dt, pulse_cap,
                             noise, h_noise_off, seed, y, pulse_count_out);
}

// Samples [q0, q0 + n) of the normal stream that the device-noise decode (noise == NULL) reads for utterance `utt`
// under `seed`: pulse i of that utterance consumes samples noff_i .. noff_i + max(3, noise_size_i) of it, exactly as it
// would consume a host-supplied stream.  Feeding the dump back as `noise` therefore reproduces the seeded decode.
extern "C" int wh_philox_normals(wh_ctx* ctx, void* stream, uint64_t seed, int utt, int64_t q0, int64_t n, double* out) {
  if (!ctx || !out || utt < 0 || q0 < 0 || n < 0) return wh::fail_msg("wh_philox_normals", "bad argument");
  WH_ENTER(ctx);
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  { wh::KernelTimer _kt(ctx, st, "philox_dump_kernel"); hipLaunchKernelGGL(philox_dump_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, seed, (int32_t)utt, q0, n, out); }
  WH_LAUNCH_CHECK("philox_dump_kernel");
  return 0;
}

// ---- peak normalisation of decode(): y /= max|y| where it exceeds 1 (world/main.py:209-212), per utterance ----
// Non-negative doubles order like their bit patterns, so the maximum is an integer atomicMax.
__global__ __launch_bounds__(256) void peak_max_kernel(const double* __restrict__ y, const int64_t* __restrict__ off,
                                                       unsigned long long* __restrict__ peak_bits) {
  __shared__ unsigned long long wmax[4];
  const int u = blockIdx.y;
  const int64_t s = off[u], n = off[u + 1] - s;
  unsigned long long m = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(y[s + i]));
    m = b > m ? b : m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long v = (unsigned long long)__shfl_xor((long long)m, o, 64);
    m = v > m ? v : m;
  }
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) m = wmax[w] > m ? wmax[w] : m;
    atomicMax(peak_bits + u, m);
  }
}
__global__ __launch_bounds__(256) void peak_scale_kernel(double* __restrict__ y, const int64_t* __restrict__ off,
                                                         const unsigned long long* __restrict__ peak_bits) {
  const int u = blockIdx.y;
  const double peak = __longlong_as_double((long long)peak_bits[u]);
  if (!(peak > 1.0)) return;  // world/main.py:210: only when the maximum exceeds 1 (a NaN peak leaves y alone)
  const int64_t s = off[u], n = off[u + 1] - s;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[s + i] = y[s + i] / peak;
}

extern "C" int wh_peak_normalise(wh_ctx* ctx, void* stream, double* y, const int64_t* h_y_off, int n_utt) {
  if (!ctx || !y || !h_y_off || n_utt < 0) return wh::fail_msg("wh_peak_normalise", "bad argument");
  WH_ENTER(ctx);
  if (n_utt == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  std::vector<int64_t> off(h_y_off, h_y_off + n_utt + 1);
  int64_t* d_off = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "peak.off", off, &d_off)) return rc;
  int64_t max_n = 0;
  for (int u = 0; u < n_utt; ++u) max_n = std::max(max_n, off[u + 1] - off[u]);
  if (int rc = wh::ws_reserve(ctx, sizeof(unsigned long long) * (size_t)n_utt)) return rc;
  unsigned long long* d_peak = reinterpret_cast<unsigned long long*>(ctx->ws);
  WH_CHECK(hipMemsetAsync(d_peak, 0, sizeof(unsigned long long) * (size_t)n_utt, st));
  const unsigned gx = (unsigned)std::min<int64_t>(64, (max_n + 4 * 256 - 1) / (4 * 256) + 1);
  { wh::KernelTimer _kt(ctx, st, "peak_max_kernel"); hipLaunchKernelGGL(peak_max_kernel, dim3(gx, n_utt), dim3(256), 0, st, y, d_off, d_peak); }
  WH_LAUNCH_CHECK("peak_max_kernel");
  { wh::KernelTimer _kt(ctx, st, "peak_scale_kernel"); hipLaunchKernelGGL(peak_scale_kernel, dim3(gx, n_utt), dim3(256), 0, st, y, d_off, d_peak); }
  WH_LAUNCH_CHECK("peak_scale_kernel");
  return 0;
}

#ifdef WH_RESP_STAGE_TIMER
extern "C" int wh_debug_resp_stages(unsigned long long* out16, int reset) {
  (void)hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_resp_stage), sizeof(unsigned long long) * 16);
  if (reset) {
    unsigned long long z[16] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_resp_stage), z, sizeof(z));
  }
  return 0;
}
#endif
