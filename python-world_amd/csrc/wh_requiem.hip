// ================================================================================================
// Requiem synthesis (world/synthesisRequiem.py:12-141): excitation = band-weighted seed noise +
// band-mixed seed pulses, then frame-wise minimum-phase filtering with overlap-add.
// ================================================================================================
#include "wh_host.h"
#include "wh_tid.h"  // (the opaque thread index of the spectral units)
#include "wh_device.h"
#include "wh_math.h"  // (behind wh_tid.h: it includes wh_device.h)
#include "wh_fft.h"
#include "wh_syn_types.h"
#include "wh_minphase.h"

namespace {
using wh::SynUtt;
using wh::lerp_segment;
using wh::first_pulse_at;

struct ReqUtt {
  int64_t hop;        // int((tp[1]-tp[0])*fs), host-evaluated
  int64_t cursor[8];  // per-band start position in the circular noise seed
  int64_t row_off;    // first overlap-add row of the utterance (req_filter_kernel), in doubles
  int64_t n_runs;     // its runs of frames
};

__global__ __launch_bounds__(256) void req_linap_kernel(const double* __restrict__ band_db, int64_t count,
                                                        double* __restrict__ lin) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) lin[i] = pow(10.0, band_db[i] / 10);  // synthesisRequiem.py:125
}

// bracketing frames of time t (SciPy interp1d linear + extrapolate)
__device__ __forceinline__ void bracket(const double* __restrict__ tp, int64_t nf, double t, int64_t* il, int64_t* ih) {
  *ih = lerp_segment(tp, nf, t);  // guess from the grid's mean step, checked; bisection otherwise
  *il = *ih - 1;
}

// Per pulse: the gain sqrt(max(1, next index - this one)) — 0 for a pulse the reference skips (unvoiced at its sample, or
// lowest-band aperiodicity above 0.999, synthesisRequiem.py:55) — and the band weights 1 - ap_b at the pulse's sample
// (synthesisRequiem.py:57-60,66-71).  One thread per pulse: the chain of dependent look-ups (pulse index, voicing,
// bracketing frames, band rows) is paid once per pulse here, with no atomics behind it.
__global__ __launch_bounds__(256) void req_pulse_weights_kernel(const SynUtt* __restrict__ meta, const double* __restrict__ tp,
                                                                const double* __restrict__ lin, int nb,
                                                                const int64_t* __restrict__ p_idx,
                                                                const int32_t* __restrict__ p_count,
                                                                const uint8_t* __restrict__ vuv_s,
                                                                double* __restrict__ p_gain, double* __restrict__ p_w) {
  const SynUtt m = meta[blockIdx.y];
  const int count = p_count[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int64_t pidx = p_idx[m.p_off + i];
  int64_t p = pidx - 1;
  p = p < 0 ? 0 : (p > m.ny - 1 ? m.ny - 1 : p);
  double gain = 0.0;
  if (vuv_s[m.y_off + p] != 0) {
    const double t = m.t0 + (double)p * m.dt;
    const double* tpu = tp + m.f_off;
    int64_t il, ih;
    bracket(tpu, m.nf, t, &il, &ih);
    const double dx = tpu[ih] - tpu[il];
    double w0 = 0.0;
    for (int b = 0; b < nb; ++b) {
      const double y_lo = lin[(m.f_off + il) * nb + b], y_hi = lin[(m.f_off + ih) * nb + b];
      const double w = (y_hi - y_lo) / dx * (t - tpu[il]) + y_lo;
      if (b == 0) w0 = w;
      p_w[(m.p_off + i) * nb + b] = 1 - w;
    }
    if (!(w0 > 0.999)) {
      const int64_t nxt = p_idx[m.p_off + (i + 1 < count ? i + 1 : count - 1)];
      const int64_t ns = nxt - pidx;
      gain = sqrt((double)(ns > 1 ? ns : 1));
    }
  }
  p_gain[m.p_off + i] = gain;
}

// The excitation signal (synthesisRequiem.py:27-63), one thread per output sample: the aperiodic component (band noises
// weighted by the interpolated aperiodicities) plus the periodic one GATHERED from the pulses whose 512-tap band-mixed
// seed covers the sample, in pulse order — the order in which the reference accumulates them, so the sum is the
// reference's, bit for bit, and the same from run to run.  (The scatter form, one wave per pulse adding its taps with
// atomics on top of the noise, was bound by the rate of those atomics: 5.4 + 1.2 ms for the two kernels at 1024
// utterances.)  The reference's clipped fancy-index assignment (Q8) keeps, of the taps that fall before the first or
// behind the last sample, only the LAST one written: taps before sample 1 are dropped (the in-range tap of index 1 is
// written after them), and the last sample receives the last tap of every pulse that reaches it or beyond.
__global__ __launch_bounds__(256) void req_excite_kernel(const SynUtt* __restrict__ meta, const ReqUtt* __restrict__ rq,
                                                         const double* __restrict__ tp, const double* __restrict__ lin,
                                                         int nb, const double* __restrict__ noise_seed, int64_t nlen,
                                                         const double* __restrict__ pulse_seed, int pfft,
                                                         const int64_t* __restrict__ p_idx, const int32_t* __restrict__ p_count,
                                                         const double* __restrict__ p_gain, const double* __restrict__ p_w,
                                                         double* __restrict__ exc) {
  const SynUtt m = meta[blockIdx.y];
  const int64_t n0 = (int64_t)blockIdx.x * 256;
  if (n0 >= m.ny) return;
  const int count = p_count[blockIdx.y];
  const int64_t* pi = p_idx + m.p_off;
  const double* pg = p_gain + m.p_off;
  const double* pw = p_w + m.p_off * nb;
  // pulses whose taps reach this tile: index in [first sample - pfft/2, last sample + pfft/2 - 1] (1-based)
  const int64_t lo = n0 + 1 - pfft / 2, hi = n0 + 256 + pfft / 2 - 1;
  const int k0 = first_pulse_at(pi, count, lo);
  const int k_end = first_pulse_at(pi, count, m.ny - pfft / 2);  // first pulse whose last tap reaches the last sample
  const int64_t i = n0 + threadIdx.x;
  if (i >= m.ny) return;
  const int64_t tgt = i + 1;
  double periodic = 0.0;
  // (the pulse records are read with scalar loads, the same for every thread of the tile; staging the tile's pulses in
  // LDS first — one round of coalesced loads, two barriers — is slower: 3.77 against 3.45 ms at 1024 utterances)
  if (tgt < m.ny) {
    for (int k = k0; k < count; ++k) {
      const int64_t pidx = pi[k];
      if (pidx > hi) break;
      const double gain = pg[k];
      if (gain == 0.0) continue;
      const int64_t mm = tgt - pidx + pfft / 2 - 1;
      if (mm >= 0 && mm < pfft) {
        double r = 0.0;
        for (int b = 0; b < nb; ++b) r += pulse_seed[mm * nb + b] * pw[(int64_t)k * nb + b];
        periodic += r * gain;
      }
    }
  } else {
    for (int k = k_end; k < count; ++k) {
      const double gain = pg[k];
      if (gain == 0.0) continue;
      double r = 0.0;
      for (int b = 0; b < nb; ++b) r += pulse_seed[(int64_t)(pfft - 1) * nb + b] * pw[(int64_t)k * nb + b];
      periodic += r * gain;
    }
  }
  const double t = m.t0 + (double)i * m.dt;
  const double* tpu = tp + m.f_off;
  int64_t il, ih;
  bracket(tpu, m.nf, t, &il, &ih);
  const double dx = tpu[ih] - tpu[il];
  double aperiodic = 0.0;
  const bool nlen_pow2 = (nlen & (nlen - 1)) == 0;
  for (int b = 0; b < nb; ++b) {
    const double y_lo = lin[(m.f_off + il) * nb + b], y_hi = lin[(m.f_off + ih) * nb + b];
    const double ap = (y_hi - y_lo) / dx * (t - tpu[il]) + y_lo;
    const int64_t at = rq[blockIdx.y].cursor[b] + i;  // circular read of the band's noise seed (synthesisRequiem.py:131-141)
    const int64_t pos = nlen_pow2 ? (at & (nlen - 1)) : at % nlen;  // (the default table lengths are powers of two)
    aperiodic += noise_seed[pos * nb + b] * ap;
  }
  exc[m.y_off + i] = periodic + aperiodic;  // synthesisRequiem.py:62
}

// The Hanning window of the Requiem frames, hanning(2 hop + 1)[1:-1] (synthesisRequiem.py:84-86): the same for every frame of
// every utterance with that hop.  Evaluated on the device with req_filter_kernel's own expression (bitwise what the kernel
// computes in place), cached per context and window length.
__global__ void req_hann_kernel(double* __restrict__ w, int wlen) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < wlen) w[j] = 0.5 - 0.5 * cospi(2.0 * (double)(j + 1) / (double)(wlen + 1));
}

// frames per run of req_filter_kernel: 4 up to N = 1024 — measured at config 4 (filter + gather) with the run's sums in
// LDS: 1 frame 1.40 + 0.22 ms, 4 frames 1.57 + 0.08, 8 frames 1.70 + 0.06, 16 frames 1.96 + 0.05; one frame per row
// beyond (no benchmark config decodes Requiem there).  At the north-star size (1024 x 10 s, round 6): 1 frame 23.4 + 3.2 ms
// (nine workgroups per CU instead of six: -7 % for +50 % of the waves — the kernel is not waiting for occupancy), 2 frames
// 25.3 + 2.0, 4 frames 25.1 + 1.2, 8 frames 27.0 + 0.9
constexpr int req_runf(int n) { return n <= 1024 ? 4 : 1; }

// Frame-wise minimum-phase filtering of the excitation with overlap-add (synthesisRequiem.py:74-101), WITHOUT atomics:
// a workgroup takes a run of RUNF consecutive frames of one utterance, adds their responses — in frame order — into an
// LDS accumulator that spans the run ((RUNF - 1) hop + N samples), and writes it as the run's ROW; req_gather_kernel
// then adds, per output sample, the two or three rows that cover it, in run order.  The same sum from launch to launch
// and wherever the utterance sits in a batch (runs are numbered per utterance); the reference adds frame after frame
// into y — runs of frames first is another association of that sum.  Row r of an utterance: W = (RUNF - 1) hop + N + 1
// doubles at row_off + r W; slot 0 = the run's share of the utterance's LAST sample (Q8: of the taps clipped onto it
// only the last one written survives — the last tap of every frame whose response reaches it or beyond), slot 1 + j =
// the sum at the 1-based sample a_r + j, a_r = r RUNF hop + 1.  RUNF = 1 (long transforms, long hops): the row is the
// frame's own response, written straight from the transform buffer.  Rows instead of atomics take the 1.07 GB of
// read-modify-write traffic per 64 utterances down to a 0.33 GB row write + as much read by the gather.
template <int N, int RUNF>
__global__ __launch_bounds__(ft_syn(N), 1) void req_filter_kernel(const SynUtt* __restrict__ meta, const ReqUtt* __restrict__ rq,
                                                        const double* __restrict__ spectrogram,
                                                        const double* __restrict__ exc,
                                                        const double2* __restrict__ tw_base_arg, double* rows,
                                                        const double* __restrict__ hann) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int FT = ft_syn(N);
  constexpr int K = N / 2 + 1;
  const double2* tw_raw = tw_base_arg;
  const SynUtt m = meta[blockIdx.y];
  const ReqUtt q = rq[blockIdx.y];
  // (wh::ckp<T> is T* in every shipped build; the bounds build checks each access against the range named here)
  const wh::ckp<double> zr = wh::ck_make(reinterpret_cast<double*>(smem), N + 2, wh::WH_CK_LDS_MAIN);  // minimum-phase half spectrum (N/2+1 complex)
  const wh::ckp<double2> zb = wh::ck_as<double2>(zr);
  const wh::ckp<double> sr = wh::ck_make(reinterpret_cast<double*>(smem) + (N + 2), N + 2, wh::WH_CK_LDS_AUX);  // windowed excitation frame / its half spectrum
  const wh::ckp<double2> sb = wh::ck_as<double2>(sr);
  // RUNF > 1: the run's sums, (RUNF - 1) hop + N doubles
  const wh::ckp<double> acc = wh::ck_make(reinterpret_cast<double*>(smem) + 2 * (N + 2), RUNF > 1 ? (RUNF - 1) * q.hop + N : 0, wh::WH_CK_LDS_OTHER);
  if ((int64_t)blockIdx.x >= q.n_runs) return;
  const int64_t hop = q.hop;
  int64_t wlen = 2 * hop - 1;
  const int64_t i0 = (int64_t)blockIdx.x * RUNF + 2;  // frames 2 .. F-2  (synthesisRequiem.py:83)
  const int64_t i1 = i0 + RUNF - 1 < m.nf - 2 ? i0 + RUNF - 1 : m.nf - 2;
  const int64_t a_r = (i0 - 2) * hop + 1;  // 1-based sample of the run's first tap (= the first frame's origin)
  const int64_t W = (RUNF - 1) * hop + N + 1;
  const wh::ckp<double> row = wh::ck_make(rows + q.row_off + (int64_t)blockIdx.x * W, W, wh::WH_CK_OUT);
  const int span = (int)(W - 1);
  if (RUNF > 1) {
    for (int j = threadIdx.x; j < span; j += FT) acc[j] = 0.0;  // (ordered before the first add by the chain's barriers)
  }
  double last = 0.0;  // (thread FT-1: tap N-1 of every frame whose response reaches the utterance's last sample)
  const wh::ckp<const double> eu = wh::ck_make(exc + m.y_off, m.ny, wh::WH_CK_WAVEFORM);
#pragma unroll 1
  for (int64_t i = i0; i <= i1; ++i) {
    const int64_t origin = (i - 1) * hop - (hop - 1);  // 1-based
    // per frame: neither the twiddles nor the window values of one frame are parked in registers for the next (both are
    // the same for every frame, and hoisted out of this loop they cost a wave per SIMD)
    asm volatile("" : "+s"(tw_raw));
    const wh::ckp<const double2> tw_base = wh::ck_make(tw_raw, WH_TWIDDLE_ENTRIES, wh::WH_CK_TWIDDLE);
    {
      int hop_s = __builtin_amdgcn_readfirstlane((int)hop);  // (uniform by construction; said so for the constraint)
      asm volatile("" : "+s"(hop_s));
      wlen = 2 * (int64_t)hop_s - 1;
    }
    for (int j = WH_TID; j < N; j += FT) {
      double v = 0.0;
      if (j < wlen) {
        int64_t g = origin + j;
        g = g > m.ny ? m.ny : g;
        g = g < 1 ? 1 : g;
        // hanning(wlen+2)[1:-1] — from the launch's table when every utterance has this hop (req_hann_kernel: the same
        // expression, evaluated once instead of per frame: a cospi and a divide per sample were ~5 % of the kernel's
        // instructions), else in place
        const double wv = hann ? hann[j] : 0.5 - 0.5 * cospi(2.0 * (double)(j + 1) / (double)(wlen + 1));
        v = eu[g - 1] * wv;
      }
      sr[j] = v;
    }
    const wh::ckp<const double> sp = wh::ck_make(spectrogram + (m.f_off + (i - 1)) * K, K, wh::WH_CK_IN);
    for (int k = WH_TID; k < K; k += FT) {  // log|S| / 2, Hermitian-mirrored: the input of the chain's first transform
      const double lw = log_call(fabs(sp[k])) / 2;  // (two bins per call: measured, no gain here — 24.0 ms either way)
      zr[k] = lw;
      if (k > 0 && k < N / 2) zr[N - k] = lw;
    }
    wh::sync<FT>();
    wh::rfft_lds<N, FT>(sb, tw_base);
    // minimum-phase spectrum x excitation spectrum (both Hermitian, so is the product), straight into the inverse
    // transform: the fused chain of the pulse responses with the product applied to the register-held bin pairs
    min_phase_response<N, FT>(zb, tw_base, wh::ckp<const double>(), 0.0, [&](int k, double2 e) { return wh::cmul(e, sb[k]); });
    // The run's sums live in LDS and go to the row ONCE, at the end of the run.  (Kept in the row itself — read, add,
    // write back per frame — the kernel is 3 % faster, 1.52 against 1.57 ms at config 4: the accumulator's 10 KB cost two
    // of its eight workgroups per CU; but every frame's 8 KB then travel to HBM and the kernel moves 2.2 GB per 64
    // utterances where this form moves ~1 GB.  Register-held sums spill: 90 VGPRs.)
    const int shift = (int)(origin - a_r);  // (i - i0) * hop: where this frame's tap 0 falls in the run
    for (int mm = WH_TID; mm < N; mm += FT) {
      const double v = origin + mm < m.ny ? zr[mm] / N : 0.0;  // (origin + mm >= 1 always)
      if (RUNF > 1) acc[shift + mm] += v;  // one writer per slot and frame; frames are separated by barriers
      else row[1 + mm] = v;
    }
    if (WH_TID == FT - 1 && origin + (N - 1) >= m.ny) last += zr[N - 1] / N;
    if (RUNF > 1) wh::sync<FT>();  // zr is free for the next frame, this frame's adds are visible to its successor
  }
  if (RUNF > 1) {
    for (int j = threadIdx.x; j < span; j += FT) row[1 + j] = acc[j];  // (zeros behind a short last run's frames)
  }
  if (threadIdx.x == FT - 1) row[0] = last;
}

// y[t] = sum of the rows of req_filter_kernel that cover t, in run order; the last sample: the rows' slot 0.
template <int N, int RUNF>
__global__ __launch_bounds__(256) void req_gather_kernel(const SynUtt* __restrict__ meta, const ReqUtt* __restrict__ rq,
                                                         const double* __restrict__ rows, double* __restrict__ y) {
  const SynUtt m = meta[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m.ny) return;
  const ReqUtt q = rq[blockIdx.y];
  const int64_t adv = RUNF * q.hop;               // samples from one run's first tap to the next run's
  const int64_t W = (RUNF - 1) * q.hop + N + 1;
  const double* ru = rows + q.row_off;
  const int64_t tgt = i + 1;
  double sum = 0.0;
  if (tgt < m.ny) {
    // run r covers the samples a_r .. a_r + W - 2, a_r = r adv + 1
    int64_t r_hi = (tgt - 1) / adv;
    r_hi = r_hi > q.n_runs - 1 ? q.n_runs - 1 : r_hi;
    int64_t r_lo = tgt - (W - 1) <= 0 ? 0 : (tgt - (W - 1) - 1) / adv + 1;  // first r with a_r + W - 2 >= tgt
    for (int64_t r = r_lo; r <= r_hi; ++r) sum += ru[r * W + 1 + (tgt - (r * adv + 1))];  // (rows are written in full)
  } else {
    // frames whose last tap reaches the last sample live in the runs from (ny - N) / adv - 1 on; the others hold 0 there
    int64_t r_lo = (m.ny - N) / adv - 1;
    r_lo = r_lo < 0 ? 0 : r_lo;
    for (int64_t r = r_lo; r < q.n_runs; ++r) sum += ru[r * W];
  }
  y[m.y_off + i] = sum;
}

template <int N>
int launch_req_filter(wh_ctx* ctx, hipStream_t st, int B, int64_t max_nf, int64_t max_ny, int64_t max_hop, bool runs,
                      const SynUtt* d_meta, const ReqUtt* d_rq, const double* spec, const double* exc, double* rows,
                      double* y, int64_t uniform_hop) {
  constexpr int RUNF = req_runf(N);
  const double* d_hann = nullptr;
  if (uniform_hop > 0 && 2 * uniform_hop - 1 <= N) {
    const int wlen = (int)(2 * uniform_hop - 1);
    const std::string key = "req.hann:" + std::to_string(wlen);
    auto it = ctx->tables.find(key);
    if (it == ctx->tables.end()) {
      double* d = nullptr;
      WH_CHECK(hipMalloc((void**)&d, sizeof(double) * (size_t)wlen));
      WH_LAUNCH_UNTIMED(st, "req_hann_kernel", req_hann_kernel, dim3((unsigned)((wlen + 255) / 256)), dim3(256), 0, d,
                        wlen);
      ctx->tables[key] = d;
      ctx->table_bytes += sizeof(double) * (size_t)wlen;
      d_hann = d;
    } else {
      d_hann = it->second;
    }
  }
  const size_t lds = sizeof(double2) * 2 * (N / 2 + 1) + 64;  // the chain's buffer and the excitation frame's
  const bool run = runs && RUNF > 1;
  if (max_nf >= 4) {
    const size_t lds_k = run ? lds + sizeof(double) * (size_t)((RUNF - 1) * max_hop + N) : lds;  // + the run's sums
    const auto k = run ? req_filter_kernel<N, RUNF> : req_filter_kernel<N, 1>;
    if (int rc = wh::allow_lds(k, lds_k)) return rc;
    WH_LAUNCH(ctx, st, "req_filter_kernel", k, dim3((unsigned)(run ? (max_nf - 3 + RUNF - 1) / RUNF : max_nf - 3), B),
              dim3(ft_syn(N)), lds_k, d_meta, d_rq, spec, exc, ctx->d_twiddle, rows, d_hann);
  }
  WH_LAUNCH(ctx, st, "req_gather_kernel", run ? req_gather_kernel<N, RUNF> : req_gather_kernel<N, 1>,
            dim3((unsigned)((max_ny + 255) / 256), B), dim3(256), 0, d_meta, d_rq, rows, y);
  return 0;
}

}  // namespace

extern "C" int wh_synthesis_requiem(wh_ctx* ctx, void* stream, const wh_batch* b, const double* tp, const double* f0,
                                    const double* vuv, const double* spectrogram, const double* band_aperiodicity,
                                    double fs, int fft_size, const int64_t* h_y_off, const double* h_t0, const double* h_dt,
                                    const int64_t* h_hop, int64_t pulse_cap, const double* pulse_seed, int pulse_fft,
                                    const double* noise_seed, int64_t noise_len, int n_bands, const int64_t* h_cursor,
                                    double* y) {
  if (!ctx || !b || !tp || !f0 || !vuv || !spectrogram || !band_aperiodicity || !h_y_off || !h_t0 || !h_dt || !h_hop ||
      !pulse_seed || !noise_seed || !h_cursor || !y)
    return wh::fail_msg("wh_synthesis_requiem", "null argument");
  WH_ENTER(ctx);
  if (n_bands < 1 || n_bands > 8) return wh::fail_msg("wh_synthesis_requiem", "n_bands must be in [1, 8]");
  if (pulse_cap < 1 || noise_len < 1) return wh::fail_msg("wh_synthesis_requiem", "bad pulse_cap / noise_len");
  hipStream_t st = (hipStream_t)stream;
  const int B = b->n_utt;
  std::vector<SynUtt> meta;
  std::vector<ReqUtt> rq(B);
  int64_t max_ny = 0, max_nf = 0, max_hop = 0, uniform_hop = 0;  // (uniform_hop: the hop every utterance has, or 0)
  if (int rc = wh::fill_syn_meta("wh_synthesis_requiem", b, h_y_off, h_t0, h_dt, pulse_cap, nullptr, nullptr, meta, &max_ny)) return rc;
  for (int u = 0; u < B; ++u) {
    rq[u].hop = h_hop[u];
    if (rq[u].hop < 1) return wh::fail_msg("wh_synthesis_requiem", "frame hop below one sample");
    max_hop = std::max(max_hop, rq[u].hop);
    if (u == 0) uniform_hop = rq[u].hop;
    else if (rq[u].hop != uniform_hop) uniform_hop = 0;
    for (int k = 0; k < 8; ++k) rq[u].cursor[k] = k < n_bands ? ((h_cursor[(int64_t)u * n_bands + k] % noise_len) + noise_len) % noise_len : 0;
    max_nf = std::max(max_nf, meta[u].nf);
  }
  const int64_t ny_tot = h_y_off[B];
  const int64_t F = b->total_frames;
  // overlap-add rows of req_filter_kernel: runs of frames (one row per frame beyond N = 1024 and for long hops)
  int runf = 1;
  if (!wh::dispatch_fft_size(fft_size, [&](auto n) { runf = req_runf(n); }))
    return wh::fail_msg("wh_synthesis_requiem", "fft_size must be a power of two in [512, 4096]");
  // (the run's sums are an LDS accumulator of (RUNF - 1) hop + N doubles: at most 2 N, i.e. 16 KB at N = 1024)
  const bool runs = runf > 1 && (runf - 1) * max_hop <= (int64_t)fft_size;
  if (!runs) runf = 1;
  int64_t rows_tot = 0;
  for (int u = 0; u < B; ++u) {
    const int64_t frames = meta[u].nf >= 4 ? meta[u].nf - 3 : 0;  // frames 2 .. F-2
    rq[u].n_runs = (frames + runf - 1) / runf;
    rq[u].row_off = rows_tot;
    rows_tot += rq[u].n_runs * ((runf - 1) * rq[u].hop + fft_size + 1);
  }
  wh::Carve carve;
  const wh::TimeBaseLayout lay(carve, B, ny_tot, pulse_cap, max_ny);
  const auto r_lin = carve.take<double>(F * n_bands);
  const auto r_exc = carve.take<double>(ny_tot);
  const auto r_pw = carve.take<double>(B * pulse_cap * n_bands);  // band weights per pulse (the gains reuse lay.pt)
  const auto r_rows = carve.take<double>(rows_tot + 8);
  if (int rc = wh::ws_reserve(ctx, carve)) return rc;
  void* ws = ctx->ws;
  SynUtt* d_meta = nullptr;
  ReqUtt* d_rq = nullptr;
  double* d_pt = lay.pt.at(ws);  // (pulse times; then the pulse gains)
  const uint8_t* d_vuv = lay.vuv.at(ws);
  const int64_t* d_pi = lay.pi.at(ws);
  const int32_t* d_pc = lay.pc.at(ws);
  double *d_lin = r_lin.at(ws), *d_exc = r_exc.at(ws), *d_pw = r_pw.at(ws), *d_rows = r_rows.at(ws);
  if (int rc = wh::persistent_upload(ctx, st, "syn.meta", meta, &d_meta)) return rc;
  if (int rc = wh::persistent_upload(ctx, st, "syn.req", rq, &d_rq)) return rc;
  if (int rc = wh::launch_pulses(ctx, st, B, max_ny, d_meta, tp, f0, vuv, fs, 0.0, h_y_off, ws, lay)) return rc;
  WH_LAUNCH(ctx, st, "req_linap_kernel", req_linap_kernel, dim3((unsigned)((F * n_bands + 255) / 256)), dim3(256), 0,
            band_aperiodicity, F * n_bands, d_lin);
  WH_LAUNCH(ctx, st, "req_pulse_weights_kernel", req_pulse_weights_kernel, dim3((unsigned)((pulse_cap + 255) / 256), B),
            dim3(256), 0, d_meta, tp, d_lin, n_bands, d_pi, d_pc, d_vuv, d_pt, d_pw);
  WH_LAUNCH(ctx, st, "req_excite_kernel", req_excite_kernel, dim3((unsigned)((max_ny + 255) / 256), B), dim3(256), 0,
            d_meta, d_rq, tp, d_lin, n_bands, noise_seed, noise_len, pulse_seed, pulse_fft, d_pi, d_pc, d_pt, d_pw,
            d_exc);
  int rc = 0;
  wh::dispatch_fft_size(fft_size, [&](auto n) {
    rc = launch_req_filter<decltype(n)::value>(ctx, st, B, max_nf, max_ny, max_hop, runs, d_meta, d_rq, spectrogram, d_exc, d_rows, y, uniform_hop);
  });
  return rc;
}
