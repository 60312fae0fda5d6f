// Pulse-by-pulse overlap-add synthesis, batched: the spectral half.  Replaces synthesis() (world/synthesis.py:21-82) together
// with the time base (wh_timebase.hip: phase, pulse positions, per-pulse records).
//
//   response_kernel : one workgroup per pulse: interpolate the two neighbouring frames, build the
//                     minimum-phase periodic and aperiodic responses with six LDS FFTs
//                     (synthesis.py:86-116,144-180), excite the aperiodic one with zero-mean noise
//                     (direct convolution == the reference's truncated fftfilt), and scatter-add into
//                     y with the reference's clipped-index semantics.
#include "wh_host.h"
// response_kernel walks a run of pulses in a loop and reads the thread index opaquely (wh_tid.h): with the plain index
// every per-thread LDS / twiddle address of the ~15 transform passes in the loop body is hoisted in front of the loop and
// kept alive across it (248 VGPRs, 2 waves per SIMD); the few integer instructions that are recomputed cost nothing
// next to 128 spare registers.
#include "wh_tid.h"
#include "wh_device.h"
#include "wh_math.h"  // (behind wh_tid.h: it includes wh_device.h)
#include "wh_reduce.h"
#include "wh_syn_types.h"
#include "wh_minphase.h"
#include "wh_philox.h"
#include "wh_resp_types.h"
#include "wh_resp_ring.h"
#include "wh_resp_pulse.h"
#include "wh_resp_pair.h"

namespace {
using wh::block_excl_scan_256;
using wh::first_pulse_at;

// (the test hook of wh_philox.h stays in this unit: with its kernel in a unit of its own normal_at is scheduled
// differently here)
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
  const wh::ckp<double> ring = wh::ck_make(reinterpret_cast<double*>(smem) + RespLds<N>::kRing, RespLds<N>::kRingLen, wh::WH_CK_LDS_OTHER);
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
        RSTAGE_COUNT(kRsNPartner)
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
constexpr int kGatherPer = 4;                   // output samples per thread
constexpr int kGatherTile = 256 * kGatherPer;  // output samples per workgroup: one pulse search for all of them
template <int N>
__global__ __launch_bounds__(256) void response_gather_kernel(const SynUtt* __restrict__ meta,
                                                              const int64_t* __restrict__ p_idx,
                                                              const int32_t* __restrict__ p_count,
                                                              const double* __restrict__ rows, const int64_t* __restrict__ row_base,
                                                              const int64_t* __restrict__ row_off, int64_t runs_cap,
                                                              double* __restrict__ y) {
  constexpr int RUN = resp_run(N);
  constexpr int PER = kGatherPer;
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

// What one render hands the launcher (device pointers but for h_ny).
struct RespCall {
  int B;
  int64_t pcap_max, max_ny;
  const std::vector<int64_t>* h_ny;
  const SynUtt* d_meta;
  const double* tp;
  const double* spec;
  const double* ap;
  double fs;
  const PulseRec* p_rec;
  const int64_t* p_base;
  const int64_t* p_idx;
  const int32_t* p_count;
  const double* noise;
  uint64_t seed;
  double* y;
};

template <int N>
int launch_resp(wh_ctx* ctx, hipStream_t st, const RespCall& c) {
  const int B = c.B;
  const int64_t pcap_max = c.pcap_max, max_ny = c.max_ny;
  const std::vector<int64_t>& h_ny = *c.h_ny;
  const SynUtt* d_meta = c.d_meta;
  const int64_t* p_idx = c.p_idx;
  const int32_t* p_count = c.p_count;
  std::vector<double> dc(N);
  double sum = 0.0;
  for (int n = 0; n < N; ++n) {  // hanning(N+2)[1:-1] normalised (synthesis.py:57-58)
    dc[n] = 0.5 - 0.5 * cos(2.0 * M_PI * (double)(n + 1) / (double)(N + 1));
    sum += dc[n];
  }
  for (int n = 0; n < N; ++n) dc[n] /= sum;
  const double* d_dc = nullptr;
  if (int rc = wh::const_table(ctx, "dc_base:" + std::to_string(N), dc, &d_dc)) return rc;
  const double* d_mt = nullptr;
  if (int rc = wh::math_table(ctx, &d_mt)) return rc;
  const size_t lds = sizeof(double) * RespLds<N>::kTotal;
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
  double* d_rows = nullptr;
  int64_t *d_rb = nullptr, *d_ro = nullptr;
  if (int rc = wh::persistent_scratch(ctx, "syn.ola_rows", (size_t)row_base[B], &d_rows)) return rc;
  if (int rc = wh::persistent_scratch(ctx, "syn.run_base", (size_t)B + 1, &d_rb)) return rc;
  if (int rc = wh::persistent_scratch(ctx, "syn.row_off", (size_t)runs_cap * B, &d_ro)) return rc;
  WH_LAUNCH(ctx, st, "pulse_run_base_kernel", pulse_run_base_kernel, dim3(1), dim3(64), 0, p_count, B, resp_run(N), d_rb);
  WH_LAUNCH(ctx, st, "pulse_rows_kernel", pulse_rows_kernel<N>, dim3(B), dim3(256), 0, d_meta, p_idx, p_count, runs_cap,
            d_row_base, d_ro, ctx->d_flags);
  // one workgroup per run of resp_run(N) pulse slots; runs past the real pulse count exit at once
  const int64_t grid = wh::xcd_grid(runs_cap * B);
  const RespArgs ra{d_meta, c.tp, c.spec, c.ap, c.fs, c.p_rec, c.p_base, B, c.noise, c.seed, d_dc, ctx->d_twiddle, d_mt,
                    d_rows, d_row_base, d_rb, d_ro, runs_cap};
  WH_LAUNCH(ctx, st, "response_kernel", response_kernel<N>, dim3((unsigned)grid), dim3(ft_syn(N)), lds, ra);
  WH_LAUNCH(ctx, st, "response_gather_kernel", response_gather_kernel<N>,
            dim3((unsigned)((max_ny + kGatherTile - 1) / kGatherTile), B), dim3(256), 0, d_meta, p_idx, p_count,
            d_rows, d_row_base, d_ro, runs_cap, c.y);
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
  const void* ws = timebase_ctx->ws;
  SynUtt* d_meta = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "syn.meta", meta, &d_meta)) return rc;
  const int64_t* d_pb = t.pb.at(ws);
  const int64_t* d_pi = t.pi.at(ws);
  const PulseRec* d_rec = t.rec.at(ws);
  const int32_t* d_pc = t.pc.at(ws);
  if (noise)  // (the time base knows nothing about the noise stream: the cover test belongs to the call that is given one)
    WH_LAUNCH(ctx, st, "noise_cover_kernel", noise_cover_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, d_meta,
              d_rec, d_pb, B, ctx->d_flags);
  std::vector<int64_t> h_ny((size_t)B);
  for (int u = 0; u < B; ++u) h_ny[u] = meta[u].ny;
  const RespCall call{B, pulse_cap, max_ny, &h_ny, d_meta, tp, spectrogram, aperiodicity, fs, d_rec, d_pb, d_pi, d_pc, noise, seed, y};
  int rc = 0;
  if (!wh::dispatch_fft_size(fft_size, [&](auto n) { rc = launch_resp<decltype(n)::value>(ctx, st, call); }))
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
  WH_LAUNCH(ctx, st, "philox_dump_kernel", philox_dump_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, seed,
            (int32_t)utt, q0, n, out);
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
