// What the pieces of the response stage share (wh_synthesis.hip through wh_resp_ring.h, wh_resp_pulse.h and
// wh_resp_pair.h): the stage timer, the shape predicates, the kernel's argument bundle, the state of a run and the ONE
// definition of response_kernel's LDS layout, read by the device functions, the kernel and its launcher alike.
// Include after wh_tid.h, wh_device.h and wh_syn_types.h.
#pragma once
#include "wh_minphase.h"  // ft_syn

// -DWH_RESP_STAGE_TIMER: per-stage shader-clock cycles of response_kernel (thread 0 of every workgroup), read with
// wh_debug_resp_stages (tools/resp_stage_timer.py).  The counters are per translation unit (static, like the bounds
// record of wh_device.h): wh_debug_resp_stages lives in wh_synthesis.hip and reads the copy response_kernel writes.
enum RespStage {  // index into g_resp_stage[16]; 0 - 7: cycles of what ENDS at the mark, 8 - 13: pulse counts
  kRsNoise = 0,           // the noise run and its mean in front of the chains (from the logs to the chains)
  kRsChainsVoiced = 2,    // minimum-phase chains of a voiced pulse (two side by side)
  kRsConv = 3,            // response reorder + noise convolution
  kRsOverlapAdd = 4,      // DC sum + overlap-add into the run's ring
  kRsSetup = 5,           // pulse look-up, spectral rows, interpolation, logs
  kRsChainsUnvoiced = 6,  // the one chain of an unvoiced pulse
  kRsChainsPair = 7,      // the chains of two unvoiced pulses side by side (response_pair)
  kRsNVoiced = 8,         // pulses: voiced
  kRsNUnvoicedVuv = 9,    //         unvoiced with vuv == 0
  kRsNUnvoicedRows = 10,  //         unvoiced by the aperiodicity rows only
  kRsNPartner = 11,       //         vuv == 0 pulses whose successor in the run could share the chains (shapes without pairs)
  kRsNPairs = 12,         //         pairs taken
  kRsNPulses = 13         //         all
};
#ifdef WH_RESP_STAGE_TIMER
static __device__ unsigned long long g_resp_stage[16];
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

// The noise convolution with eight outputs per thread (see response_pulse), where it pays: the long noise runs of
// 44.1 / 48 kHz (config 5: response_kernel 41.8 -> 39.6 ms).  At 16 kHz a pulse's run is ~64 samples — two 16-sample rounds per half — and the prologue and the merge cost more than the reads they save
// (config 2: 3.43 -> 3.58 ms), so N = 1024 keeps four outputs per thread.
template <int N>
constexpr bool resp_conv8() { return N / ft_syn(N) == 4 && N >= 2048; }

// The chains' transforms on one wave each (mp_fft, wh_minphase.h): the 16 kHz shape.
template <int N>
constexpr bool resp_wave_fft() { return N == 1024; }
// A pulse whose record says vuv == 0 is unvoiced whatever the aperiodicity rows hold (synthesis.py:69), and an unvoiced
// pulse's aperiodic spectrum is the spectrogram's: at the 16 kHz shape such a pulse does not fetch the two aperiodicity
// rows.  The other lengths keep the code they had (they were not measured with it).
template <int N>
constexpr bool resp_skip_ap() { return resp_wave_fft<N>(); }
// Whether two consecutive unvoiced pulses of a run may go through the two chain buffers side by side (response_pair,
// wh_resp_pair.h): the 16 kHz shape.  (One by one: config 2 at 8.975 - 9.010 ms per step against 8.767 - 8.789 with pairs)
template <int N>
constexpr bool resp_pairs() { return resp_wave_fft<N>() && ft_syn(N) == 256; }

// The chains' complex exponentials through the table-driven forms (cis_pair_tab_call, wh_minphase.h) from N = 1024 on:
// response_kernel 2.73 -> 2.66 ms at config 2, 35.6 -> 34.9 ms at config 5, at the registers the kernels had.  N = 512 keeps
// the library call: the table form's live values take response_kernel<512> from 92 to 107 VGPRs and a wave per SIMD.
template <int N>
constexpr bool resp_table_cis() { return N >= 1024; }

// Pulses per workgroup: 6 up to N = 1024, 8 beyond (measured with the pulse record prefetch in place: 4 / 5 / 6 / 7 / 8 /
// 12 / 16 pulses 3.414 / 3.416 / 3.417 / 3.449 / 3.46 / 3.51 / 3.59 ms at config 2; at 48 kHz, N = 2048, 5 pulses 42.5
// against 41.6 ms for 8: the flush of the longer ring is what a short run does not amortise).
constexpr int resp_run(int n) { return n <= 1024 ? 6 : 8; }

// padded index of the aperiodic response for the register-tiled convolution: 2 doubles of padding every 32
// keep the 16-byte pair reads of lanes that are 4..8 samples apart on different LDS banks
__device__ __forceinline__ int rap_index(int i) { return i + 2 * (i >> 5); }

// ---- LDS layout of response_kernel<N>, in doubles: the device functions carve it, the launcher asks for it ----------
constexpr int kRespNoise = 256;  // noise samples staged per chunk of a pulse's run (what response_pulse calls NZ)
template <int N>
struct RespLds {
  static constexpr int kChainLen = N + 2;                // N/2 + 1 complex values
  static constexpr int kChainA = 0;                      // aperiodic chain (response_pair: the first pulse's)
  static constexpr int kChainP = kChainA + kChainLen;    // periodic chain (response_pair: the second pulse's)
  static constexpr int kRap = kChainP + kChainLen;       // the aperiodic response, padded (rap_index)
  static constexpr int kRapLen = N + N / 16 + 2;
  static constexpr int kNoise = kRap + kRapLen;          // the noise block
  static constexpr int kNoiseLen = kRespNoise;
  static constexpr int kScratch = kNoise + kNoiseLen;    // reduction scratch (block_sum at 8 waves: 24; the side waves' sums)
  static constexpr int kScratchLen = 32;
  static constexpr int kPulse = kScratch + kScratchLen;  // what one pulse (or pair) touches: everything in front of the ring
  static constexpr int kRing = kPulse;                   // the run's overlap-add ring (RunState)
  static constexpr int kRingLen = N;
  static constexpr int kTotal = kRing + kRingLen;
};

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
  const double* math_tab;   // wh_math.h's table (wh::math_table)
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

}  // namespace
