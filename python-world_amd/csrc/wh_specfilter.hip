// ================================================================================================
// A per-frame spectral gain applied to an existing waveform: Hanning windows on an integer hop, each window's spectrum
// multiplied by the minimum-phase spectrum of a log-gain row, overlap-add without atomics.  The vocoder-free
// ("differential") voice conversion filters the source recording by converted over source envelope this way.
// Contract: include/world_hip.h; tests/_specfilter_reference.py is the same in NumPy.
//
// The chain (window -> rfft_lds (through rfft_frame_lds) -> min_phase_response with the product lambda -> the run's sums in LDS -> one row per run
// -> a gather in run order) is req_filter_kernel's (wh_requiem.hip), with another geometry and another gain:
//   * windows w = 0 .. W-1, W = ceil(ny / hop) + 1, window w starts at the 0-based sample (w - 1) hop; taps and window
//     samples outside [0, ny) are DROPPED at both ends (nothing is clipped onto an end sample, no "last sample" slot);
//   * window w takes gain row map[w] of its utterance (a host list, checked by the entry);
//   * the half log-gain h[k] is formed in the chain's buffer straight from one or two rows: two spectrogram rows
//     (kind 0), or two rows [log E, x_1 .. x_p] of line spectral frequencies in the cosine domain (kind 1) whose
//     envelopes are evaluated in product form per bin, exactly as lsf_distortion_kernel forms A2 (wh_lsf_chain.hip) —
//     neither envelope is ever in memory;
//   * or (kind 2, the entry wh_melcep_filter) the rows are mel-cepstra on an all-pass warped axis, whose
//     difference IS the exponent of a minimum-phase spectrum: per bin one Clenshaw recurrence, then exponent_response —
//     the tail of the chain alone, without h, the logarithms and the fold's two transforms.
// Built like wh_requiem.hip: build.py's default -ffp-contract=off (the products of kind 1 are rounded one by one, as
// the contract states them); only min_phase_response, exponent_response and kind 2's recurrence fuse, by their own pragmas.
// ================================================================================================
#include "wh_host.h"
#include "wh_tid.h"  // (the opaque thread index of the spectral units)
#include "wh_device.h"
#include "wh_math.h"
#include "wh_fft.h"
#include "wh_minphase.h"

#include <algorithm>

namespace {

constexpr int kSfMaxOrder = 64;
constexpr int kSfKindSpectrum = 0, kSfKindLsf = 1, kSfKindMelcep = 2;
// kind 2: the window's row difference d[0 .. order] has LDS of its own (order + 1 <= 65 doubles, padded to 16 bytes):
// the segment's buffer is being read by the product while the bins run their recurrences over d
constexpr int kSfDiffSlots = 66;

struct SfUtt {
  int64_t x_off;    // first sample of the utterance in x and y
  int64_t ny;       // its samples
  int64_t f_off;    // its first gain row
  int64_t map_off;  // its first window in the map
  int64_t n_win;    // its windows
  int64_t hop;
  int64_t row_off;  // its first overlap-add row, in doubles
  int64_t n_runs;   // its runs of windows
  int64_t runf;     // windows per run: a property of the utterance alone (sf_runf_of), whatever else is in the batch
};

// windows per run: req_filter_kernel's measured choice (wh_requiem.hip, req_runf) — the chain and the accumulator are the same
constexpr int sf_runf(int n) { return n <= 1024 ? 4 : 1; }
// ... as long as the run's accumulator, (RUNF - 1) hop + N doubles, stays within 2 N (as in wh_synthesis_requiem); a longer
// hop takes one row per window.  Decided per UTTERANCE from its own hop: the two forms associate the overlapping
// responses differently, so the form must not depend on the other utterances of the call.
inline int sf_runf_of(int n, int64_t hop) { return sf_runf(n) > 1 && (sf_runf(n) - 1) * hop <= (int64_t)n ? sf_runf(n) : 1; }

// A workgroup takes a run of RUNF consecutive windows of one utterance, adds their responses — in window order — into
// an LDS accumulator that spans the run ((RUNF - 1) hop + N samples) and writes it as the run's ROW.  Row r of an
// utterance: (RUNF - 1) hop + N doubles at row_off + r * that; slot j = the run's sum at the 0-based sample
// a_r + j, a_r = (r RUNF - 1) hop (negative for the first run: those slots hold 0, as do the slots at or behind ny).
// Runs are numbered per utterance and the form is the utterance's own (SfUtt::runf: an instantiation passes over the
// utterances of the other form), so an utterance's sums are the same alone and inside any batch.  RUNF = 1 (long
// transforms, long hops): the row is the window's own response, written straight from the transform buffer.
// Kind lsf stages the doubled roots in the segment's buffer, which is free until h is built: no LDS of their own.
// Kind 2 (wh_melcep_filter): the rows are mel-cepstra c[0 .. p] on the all-pass warped axis whose cosines and sines the
// table holds (cos_[k] = cos beta_k, cos_[K + k] = sin beta_k).  exp(sum_j d[j] z~^-j) is minimum phase as it stands, so
// the thread that owns the pair of bins (k, N/2 - k) evaluates both exponents itself — one Clenshaw recurrence each over
// d = num - den, read from LDS at one address by every lane (a broadcast) — and goes straight to exponent_response:
// no logarithm, no h in LDS, and the chain's first two transforms with their barriers are absent.
template <int N, int RUNF, int KIND>
__global__ __launch_bounds__(ft_syn(N), 1) void specfilter_kernel(const SfUtt* __restrict__ meta, const int32_t* __restrict__ map_,
                                                                  long long n_map, const double* __restrict__ num_, long long ldn,
                                                                  const double* __restrict__ den_, long long ldd, int p,
                                                                  long long n_rows, const double* __restrict__ cos_,
                                                                  const double* __restrict__ x_,
                                                                  const double2* __restrict__ tw_base_arg, double* rows_) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int FT = ft_syn(N);
  constexpr int K = N / 2 + 1;
  const double2* tw_raw = tw_base_arg;
  const SfUtt m = meta[blockIdx.y];
  // (wh::ckp<T> is T* in every shipped build; the bounds build checks each access against the range named here)
  const wh::ckp<double> zr = wh::ck_make(reinterpret_cast<double*>(smem), N + 2, wh::WH_CK_LDS_MAIN);  // h mirrored -> minimum-phase half spectrum -> response
  const wh::ckp<double2> zb = wh::ck_as<double2>(zr);
  const wh::ckp<double> sr = wh::ck_make(reinterpret_cast<double*>(smem) + (N + 2), N + 2, wh::WH_CK_LDS_AUX);  // windowed segment / its half spectrum
  const wh::ckp<double2> sb = wh::ck_as<double2>(sr);
  // kind 1: the doubled roots of the numerator's and the denominator's row, in the segment's buffer until h is built
  const wh::ckp<double> xa = wh::ck_make(reinterpret_cast<double*>(smem) + (N + 2), kSfMaxOrder, wh::WH_CK_LDS_SCRATCH);
  const wh::ckp<double> xb = wh::ck_make(reinterpret_cast<double*>(smem) + (N + 2) + kSfMaxOrder, kSfMaxOrder, wh::WH_CK_LDS_SCRATCH);
  // RUNF > 1: the run's sums, (RUNF - 1) hop + N doubles
  constexpr int DL = KIND == kSfKindMelcep ? kSfDiffSlots : 0;  // kind 2: d[0 .. p] between the segment and the sums
  const wh::ckp<double> dl = wh::ck_make(reinterpret_cast<double*>(smem) + 2 * (N + 2), DL, wh::WH_CK_LDS_SCRATCH);
  const wh::ckp<double> acc = wh::ck_make(reinterpret_cast<double*>(smem) + 2 * (N + 2) + DL,
                                          RUNF > 1 ? (RUNF - 1) * m.hop + N : 0, wh::WH_CK_LDS_OTHER);
  if (m.runf != RUNF || (int64_t)blockIdx.x >= m.n_runs) return;  // (uniform over the workgroup)
  const int64_t hop = m.hop;
  int64_t wlen = 2 * hop - 1;
  const int64_t w0 = (int64_t)blockIdx.x * RUNF;
  const int64_t w1 = w0 + RUNF - 1 < m.n_win - 1 ? w0 + RUNF - 1 : m.n_win - 1;
  const int64_t a_r = (w0 - 1) * hop;  // 0-based sample of the run's first tap
  const int64_t W = (RUNF - 1) * hop + N;
  const wh::ckp<double> row = wh::ck_make(rows_ + m.row_off + (int64_t)blockIdx.x * W, W, wh::WH_CK_OUT);
  const int span = (int)W;
  if (RUNF > 1) {
    for (int j = threadIdx.x; j < span; j += FT) acc[j] = 0.0;  // (ordered before the first add by the chain's barriers)
  }
  const wh::ckp<const double> xu = wh::ck_make(x_ + m.x_off, m.ny, wh::WH_CK_WAVEFORM);
  const wh::ckp<const int32_t> map = wh::ck_make(map_, n_map, wh::WH_CK_IN);
  const long long cols = KIND == kSfKindSpectrum ? K : p + 1;
  const wh::ckp<const double> num = wh::ck_make(num_, (n_rows - 1) * ldn + cols, wh::WH_CK_IN);
  const wh::ckp<const double> den = wh::ck_make(den_, den_ ? (n_rows - 1) * ldd + cols : 0, wh::WH_CK_IN);
  const wh::ckp<const double> ctab = wh::ck_make(cos_, KIND == kSfKindLsf ? K : KIND == kSfKindMelcep ? 2 * K : 0, wh::WH_CK_TABLE);
#pragma unroll 1
  for (int64_t w = w0; w <= w1; ++w) {
    const int64_t s = (w - 1) * hop;                       // 0-based sample of the window's first tap
    const int64_t r = m.f_off + (int64_t)map[m.map_off + w];  // (inside the utterance's rows: checked on the host)
    // per window: neither the twiddles nor the window values of one window are parked in registers for the next
    // (req_filter_kernel: hoisted out of this loop they cost a wave per SIMD)
    asm volatile("" : "+s"(tw_raw));
    const wh::ckp<const double2> tw_base = wh::ck_make(tw_raw, WH_TWIDDLE_ENTRIES, wh::WH_CK_TWIDDLE);
    {
      int hop_s = __builtin_amdgcn_readfirstlane((int)hop);  // (uniform by construction; said so for the constraint)
      asm volatile("" : "+s"(hop_s));
      wlen = 2 * (int64_t)hop_s - 1;
    }
    if (KIND == kSfKindLsf) {
      // (the buffer is free: the last window's product read it in front of its chain's last barriers)
      const int j = WH_TID;
      if (j < p) {
        xa[j] = 2.0 * num[r * ldn + 1 + j];
        if (den_) xb[j] = 2.0 * den[r * ldd + 1 + j];
      }
      wh::sync<FT>();
      const double g = den_ ? num[r * ldn] - den[r * ldd] : num[r * ldn];  // log E_n - log E_d
      for (int k = WH_TID; k < K; k += FT) {
        const double c = ctab[k];
        const double tc = 2.0 * c;
        double ua = 1.0, va = 1.0, ub = 1.0, vb = 1.0;
        for (int i = 0; i < p; i += 2) {
          ua = ua * (tc - xa[i]);
          va = va * (tc - xa[i + 1]);
          if (den_) {
            ub = ub * (tc - xb[i]);
            vb = vb * (tc - xb[i + 1]);
          }
        }
        const double fp = 2.0 * (1.0 + c), fm = 2.0 * (1.0 - c);
        const double a2n = 0.25 * (fp * (ua * ua) + fm * (va * va));
        const double a2d = 0.25 * (fp * (ub * ub) + fm * (vb * vb));
        const double t = log_call(den_ ? a2n / a2d : a2n);
        const double h = (g - t) / 2;
        zr[k] = h;
        if (k > 0 && k < N / 2) zr[N - k] = h;
      }
      wh::sync<FT>();  // every bin has read the roots: the buffer takes the segment
    }
    for (int j = WH_TID; j < N; j += FT) {
      double v = 0.0;
      const int64_t g = s + j;
      if (j < wlen && g >= 0 && g < m.ny) {
        // hanning(wlen + 2)[1:-1], req_filter_kernel's own expression (wlen + 1 = 2 hop)
        const double wv = 0.5 - 0.5 * cospi(2.0 * (double)(j + 1) / (double)(wlen + 1));
        v = xu[g] * wv;
      }
      sr[j] = v;
    }
    if (KIND == kSfKindMelcep) {
      // (free: the last window's bins read it in front of their inverse transform's barriers)
      const int j = WH_TID;
      if (j <= p) dl[j] = den_ ? num[r * ldn + j] - den[r * ldd + j] : num[r * ldn + j];
    }
    if (KIND == kSfKindSpectrum) {
      const wh::ckp<const double> nr = num + r * ldn;
      const wh::ckp<const double> dr = den_ ? den + r * ldd : den;  // (no arithmetic on a null pointer)
      for (int k = WH_TID; k < K; k += FT) {  // Hermitian-mirrored: the input of the chain's first transform
        double h;
        if (den_) {
          const double2 l = log_pair_call(fabs(nr[k]), fabs(dr[k]));
          h = (l.x - l.y) / 2;
        } else {
          h = log_call(fabs(nr[k])) / 2;
        }
        zr[k] = h;
        if (k > 0 && k < N / 2) zr[N - k] = h;
      }
    }
    wh::sync<FT>();
    wh::rfft_frame_lds<N, FT>(sb, tw_base);  // (rfft_lds at the Requiem filter's shapes: wh_fft.h)
    if constexpr (KIND == kSfKindMelcep) {
      // exp(sum_j d[j] cos(j beta) - i sum_j d[j] sin(j beta)) x segment spectrum: Clenshaw, b_j = d[j] + 2 cos(beta) b_{j+1}
      // - b_{j+2}, j = p .. 1; the sums are d[0] + cos(beta) b_1 - b_2 and sin(beta) b_1.  Two bins side by side: their
      // chains are independent, and one read of d[j] serves both.  (zb is free: the last window's taps were read in front
      // of a barrier — the run form's own, or this window's transform's.)
      exponent_response<N, FT>(
          zb, tw_base,
          [&](int k0, int k1) {
#pragma clang fp contract(fast)
            const double c0 = ctab[k0], c1 = ctab[k1];
            const double t0 = 2.0 * c0, t1 = 2.0 * c1;
            double u1 = 0.0, u2 = 0.0, v1 = 0.0, v2 = 0.0;  // b_{j+1}, b_{j+2} of either bin
#pragma unroll 4
            for (int j = p; j >= 1; --j) {
              const double dj = dl[j];
              const double u0 = dj + t0 * u1 - u2, v0 = dj + t1 * v1 - v2;
              u2 = u1;
              u1 = u0;
              v2 = v1;
              v1 = v0;
            }
            const double d0 = dl[0];
            return make_double4(d0 + c0 * u1 - u2, ctab[K + k0] * u1, d0 + c1 * v1 - v2, ctab[K + k1] * v1);
          },
          [&](int k, double2 e) { return wh::cmul(e, sb[k]); });
    } else {
      // minimum-phase spectrum of h x segment spectrum (both Hermitian, so is the product), straight into the inverse transform
      min_phase_response<N, FT>(zb, tw_base, wh::ckp<const double>(), 0.0, [&](int k, double2 e) { return wh::cmul(e, sb[k]); });
    }
    const int shift = (int)(s - a_r);  // (w - w0) * hop: where this window's tap 0 falls in the run
    for (int mm = WH_TID; mm < N; mm += FT) {
      const int64_t t = s + mm;
      const double v = t >= 0 && t < m.ny ? zr[mm] / N : 0.0;  // taps outside the utterance are dropped
      if (RUNF > 1) acc[shift + mm] += v;  // one writer per slot and window; windows are separated by barriers
      else row[mm] = v;
    }
    if (RUNF > 1) wh::sync<FT>();  // zr is free for the next window, this window's adds are visible to its successor
  }
  if (RUNF > 1) {
    for (int j = threadIdx.x; j < span; j += FT) row[j] = acc[j];  // (zeros behind a short last run's windows)
  }
}

// y[t] = sum of the rows of specfilter_kernel that cover t, in run order.
template <int N>
__global__ __launch_bounds__(256) void specfilter_gather_kernel(const SfUtt* __restrict__ meta, const double* __restrict__ rows_,
                                                                long long n_rows_doubles, double* __restrict__ y_) {
  const SfUtt m = meta[blockIdx.y];
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= m.ny) return;
  const wh::ckp<const double> rows = wh::ck_make(rows_, n_rows_doubles, wh::WH_CK_IN);
  const wh::ckp<double> y = wh::ck_make(y_ + m.x_off, m.ny, wh::WH_CK_OUT);
  const int64_t adv = m.runf * m.hop;  // samples from one run's first tap to the next run's
  const int64_t W = (m.runf - 1) * m.hop + N;
  // run r covers the samples a_r .. a_r + W - 1, a_r = r adv - hop
  int64_t r_hi = (t + m.hop) / adv;
  r_hi = r_hi > m.n_runs - 1 ? m.n_runs - 1 : r_hi;
  const int64_t lo = t + m.hop - W + 1;  // first r with r adv >= lo
  const int64_t r_lo = lo <= 0 ? 0 : (lo + adv - 1) / adv;
  double sum = 0.0;
  for (int64_t r = r_lo; r <= r_hi; ++r) sum += rows[m.row_off + r * W + (t - (r * adv - m.hop))];  // (rows are written in full)
  y[t] = sum;
}

// max_runs / max_hop: [0] over the utterances of the run form, [1] over those with one row per window
template <int N, int KIND>
int launch_specfilter(wh_ctx* ctx, hipStream_t st, int B, const int64_t* max_runs, int64_t max_ny, const int64_t* max_hop,
                      const SfUtt* d_meta, const int32_t* d_map, int64_t n_map, const double* num, int64_t ldn,
                      const double* den, int64_t ldd, int p, int64_t n_rows, const double* d_cos, const double* x,
                      double* rows, int64_t rows_tot, double* y) {
  constexpr int RUNF = sf_runf(N);
  // the chain's buffer and the segment's (+ kind 2's row difference)
  const size_t lds = sizeof(double) * (2 * (N + 2) + (KIND == kSfKindMelcep ? kSfDiffSlots : 0)) + 64;
  if constexpr (RUNF > 1) {
    if (max_runs[0] > 0) {
      const size_t lds_k = lds + sizeof(double) * (size_t)((RUNF - 1) * max_hop[0] + N);  // + the run's sums
      if (int rc = wh::allow_lds(specfilter_kernel<N, RUNF, KIND>, lds_k)) return rc;
      WH_LAUNCH(ctx, st, "specfilter_kernel", specfilter_kernel<N, RUNF, KIND>, dim3((unsigned)max_runs[0], B),
                dim3(ft_syn(N)), lds_k, d_meta, d_map, n_map, num, ldn, den, ldd, p, n_rows, d_cos, x, ctx->d_twiddle, rows);
    }
  }
  if (max_runs[1] > 0) {
    if (int rc = wh::allow_lds(specfilter_kernel<N, 1, KIND>, lds)) return rc;
    WH_LAUNCH(ctx, st, "specfilter_kernel", specfilter_kernel<N, 1, KIND>, dim3((unsigned)max_runs[1], B), dim3(ft_syn(N)),
              lds, d_meta, d_map, n_map, num, ldn, den, ldd, p, n_rows, d_cos, x, ctx->d_twiddle, rows);
  }
  if (max_ny > 0)
    WH_LAUNCH(ctx, st, "specfilter_gather_kernel", specfilter_gather_kernel<N>, dim3((unsigned)((max_ny + 255) / 256), B),
              dim3(256), 0, d_meta, rows, rows_tot, y);
  return 0;
}

// Both entries: `where` names the caller in the messages; `kind` has been admitted by it.  Kind 2 takes two HOST tables
// of K entries (h_cos, h_sin: the warped axis), kind 1 one, kind 0 none.
int spectral_filter(const char* where, wh_ctx* ctx, void* stream, int n_utt, const int64_t* h_x_off, const int64_t* h_frame_off,
                    const int64_t* h_map_off, const int32_t* h_map, const int64_t* h_hop, int kind, const double* num,
                    int64_t ldn, const double* den, int64_t ldd, int p_or_kbins, const double* h_cos, const double* h_sin,
                    int fft_size, const double* x, double* y) {
  if (n_utt < 0) return wh::fail_msg(where, "negative utterance count");
  if (n_utt > 65535) return wh::fail_msg(where, "at most 65535 utterances per call");
  if (!wh::dispatch_fft_size(fft_size, [](auto) {}))
    return wh::fail_msg(where, "fft_size must be a power of two in [512, 4096]");
  const int K = fft_size / 2 + 1;
  int p = 0;
  if (kind == kSfKindLsf) {
    p = p_or_kbins;
    if (p < 2 || p > kSfMaxOrder || (p & 1)) return wh::fail_msg(where, "the order p must be even and in [2, 64]");
    if (!h_cos) return wh::fail_msg(where, "null argument");
  } else if (kind == kSfKindMelcep) {
    p = p_or_kbins;
    if (p < 1 || p > kSfMaxOrder) return wh::fail_msg(where, "the order must be in [1, 64]");
    if (!h_cos || !h_sin) return wh::fail_msg(where, "null table of the warped axis");
  } else if (p_or_kbins != K) {
    return wh::fail_msg(where, "kind spectrum: the rows must have fft_size / 2 + 1 bins");
  }
  const int64_t cols = kind == kSfKindSpectrum ? K : p + 1;
  if (ldn < cols) return wh::fail_msg(where, "ldn is smaller than a row");
  if (den && ldd < cols) return wh::fail_msg(where, "ldd is smaller than a row");
  if (n_utt == 0) return 0;
  if (!h_x_off || !h_frame_off || !h_map_off || !h_hop) return wh::fail_msg(where, "null argument");
  const int B = n_utt;
  std::vector<SfUtt> meta(B);
  int64_t max_ny = 0;
  for (int u = 0; u < B; ++u) {
    SfUtt& m = meta[u];
    m.hop = h_hop[u];
    int64_t nf = 0;
    if (!wh::utt_span(h_x_off, u, &m.x_off, &m.ny) || !wh::utt_span(h_frame_off, u, &m.f_off, &nf) ||
        !wh::utt_span(h_map_off, u, &m.map_off, &m.n_win))
      return wh::fail_msg(where, "offsets must start at or above 0 and be monotone");
    if (m.hop < 1) return wh::fail_msg(where, "hop below one sample");
    if (2 * m.hop - 1 > (int64_t)fft_size) return wh::fail_msg(where, "the window of 2 hop - 1 samples is longer than fft_size");
    const int64_t want = m.ny > 0 ? (m.ny + m.hop - 1) / m.hop + 1 : 0;
    if (m.n_win != want) return wh::fail_msg(where, "an utterance's map must have ceil(ny / hop) + 1 entries (none when it is empty)");
    if (m.n_win > 0 && !h_map) return wh::fail_msg(where, "null argument");
    for (int64_t w = 0; w < m.n_win; ++w) {
      const int32_t r = h_map[m.map_off + w];
      if (r < 0 || r >= nf) return wh::fail_msg(where, "a map entry is outside the utterance's gain rows");
    }
    max_ny = std::max(max_ny, m.ny);
  }
  const int64_t n_map = h_map_off[B], n_rows = h_frame_off[B], ny_tot = h_x_off[B];
  if (ny_tot == 0) return 0;
  if (!num || !x || !y) return wh::fail_msg(where, "null argument");
  int64_t rows_tot = 0, max_runs[2] = {0, 0}, max_hop[2] = {0, 0};
  for (int u = 0; u < B; ++u) {
    const int runf = sf_runf_of(fft_size, meta[u].hop);  // the utterance's own form
    meta[u].runf = runf;
    meta[u].n_runs = (meta[u].n_win + runf - 1) / runf;
    meta[u].row_off = rows_tot;
    rows_tot += meta[u].n_runs * ((runf - 1) * meta[u].hop + fft_size);
    const int form = runf > 1 ? 0 : 1;
    max_runs[form] = std::max(max_runs[form], meta[u].n_runs);
    max_hop[form] = std::max(max_hop[form], meta[u].hop);
  }
  if (std::max(max_runs[0], max_runs[1]) > 0x7fffffffLL || (max_ny + 255) / 256 > 0x7fffffffLL) return wh::fail_msg(where, "an utterance is too long for one call");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = wh::ws_reserve(ctx, sizeof(double) * (size_t)(rows_tot + 8))) return rc;
  double* d_rows = reinterpret_cast<double*>(ctx->ws);
  SfUtt* d_meta = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "sf.meta", meta, &d_meta)) return rc;
  void* d_map = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "sf.map", h_map, (size_t)n_map * sizeof(int32_t), &d_map)) return rc;
  void* d_cos = nullptr;
  if (kind == kSfKindLsf)
    if (int rc = wh::persistent_upload(ctx, st, "sf.bins", h_cos, (size_t)K * sizeof(double), &d_cos)) return rc;
  if (kind == kSfKindMelcep) {  // [cos beta_k | sin beta_k], one upload
    std::vector<double> warp(h_cos, h_cos + K);
    warp.insert(warp.end(), h_sin, h_sin + K);
    if (int rc = wh::persistent_upload(ctx, st, "sf.warp", warp.data(), warp.size() * sizeof(double), &d_cos)) return rc;
  }
  int rc = 0;
  wh::dispatch_fft_size(fft_size, [&](auto n) {
    constexpr int N = decltype(n)::value;
    auto go = [&](auto k) {
      return launch_specfilter<N, decltype(k)::value>(ctx, st, B, max_runs, max_ny, max_hop, d_meta, (const int32_t*)d_map, n_map,
                                                      num, ldn, den, ldd, p, n_rows, (const double*)d_cos, x, d_rows, rows_tot, y);
    };
    rc = kind == kSfKindLsf      ? go(std::integral_constant<int, kSfKindLsf>())
         : kind == kSfKindMelcep ? go(std::integral_constant<int, kSfKindMelcep>())
                                 : go(std::integral_constant<int, kSfKindSpectrum>());
  });
  return rc;
}

}  // namespace

extern "C" int wh_spectral_filter(wh_ctx* ctx, void* stream, int n_utt, const int64_t* h_x_off, const int64_t* h_frame_off,
                                  const int64_t* h_map_off, const int32_t* h_map, const int64_t* h_hop, int kind,
                                  const double* num, int64_t ldn, const double* den, int64_t ldd, int p_or_kbins,
                                  const double* h_cos, int fft_size, const double* x, double* y) {
  const char* where = "wh_spectral_filter";
  if (!ctx) return wh::fail_msg(where, "null argument");
  WH_ENTER(ctx);
  // (mel-cepstral rows have an entry of their own, wh_melcep_filter: they need a second table)
  if (kind != kSfKindSpectrum && kind != kSfKindLsf) return wh::fail_msg(where, "kind must be 0 (spectrum) or 1 (lsf)");
  return spectral_filter(where, ctx, stream, n_utt, h_x_off, h_frame_off, h_map_off, h_map, h_hop, kind, num, ldn, den, ldd,
                         p_or_kbins, h_cos, nullptr, fft_size, x, y);
}

extern "C" int wh_melcep_filter(wh_ctx* ctx, void* stream, int n_utt, const int64_t* h_x_off, const int64_t* h_frame_off,
                                const int64_t* h_map_off, const int32_t* h_map, const int64_t* h_hop, const double* num,
                                int64_t ldn, const double* den, int64_t ldd, int order, const double* h_cos_beta,
                                const double* h_sin_beta, int fft_size, const double* x, double* y) {
  const char* where = "wh_melcep_filter";
  if (!ctx) return wh::fail_msg(where, "null argument");
  WH_ENTER(ctx);
  return spectral_filter(where, ctx, stream, n_utt, h_x_off, h_frame_off, h_map_off, h_map, h_hop, kSfKindMelcep, num, ldn, den,
                         ldd, order, h_cos_beta, h_sin_beta, fft_size, x, y);
}
