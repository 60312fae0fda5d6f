// D4C / D4C-Requiem band aperiodicity.
//   love_train_kernel : VUV gate, one workgroup per frame, one FFT          (world/d4c.py:68-88)
//   d4c_kernel        : per gated frame, everything in LDS: two Blackman frames packed as
//                       x + j*n*x into ONE complex FFT each (spectrum and time-weighted spectrum
//                       are separated by Hermitian symmetry), Hann frame FFT, three sliding-window
//                       smoothings, then per 3 kHz band: Nuttall-windowed group delay → FFT →
//                       rank-select of the smallest-energy bins → energy ratio      (world/d4c.py:114-209)
// Replaces d4c() (world/d4c.py:10-64) and d4cRequiem() (world/d4cRequiem.py:9-44).
// The pieces that can be read on their own live in headers: wh_d4c_types.h (thread counts, LDS layouts, fences, stage
// timer), wh_d4c_window.h (the analysis windows), wh_d4c_select.h (the rank selection), wh_d4c_runs.h (the run-resident
// spectral helpers).  Every transform call of D4C is in this file.
#include "wh_d4c_types.h"
#include "wh_fft.h"
#include "wh_reduce.h"
#include "wh_d4c_window.h"
#include "wh_d4c_select.h"
#include "wh_d4c_runs.h"
#include "wh_apbands.h"

namespace {
using namespace wh;

// Every transform of d4c_kernel runs the radix-8 plan, at every length (the register-fed windows feed a radix-8 first
// pass); so does the gate kernel's one real transform.
constexpr int kLoveMaxR = 8;

template <int NLT>
__global__ __launch_bounds__(ft_love(NLT)) void love_train_kernel(
    const double* __restrict__ x, const int64_t* __restrict__ x_off, const int32_t* __restrict__ frame_utt,
    const double* __restrict__ tp, double* __restrict__ f0_io, const double* __restrict__ vuv, double fs,
    double threshold, const double2* __restrict__ tw_base, int32_t* __restrict__ gate, long long n_frames) {
  constexpr int FT = ft_love(NLT);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // (wh::ckp<T> is T* in every shipped build; the bounds build checks each access against the range named here)
  const wh::ckp<double> lds_all = wh::ck_make(reinterpret_cast<double*>(smem), love_lds_doubles(NLT), wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> zr = wh::ck_sub(lds_all, 0, NLT + 2, wh::WH_CK_LDS_MAIN);  // the NLT real samples, then the half spectrum (NLT + 2 doubles)
  const wh::ckp<double2> zb = wh::ck_as<double2>(zr);                               // NLT/2+1 complex after the real FFT
  const wh::ckp<double> scratch = wh::ck_sub(lds_all, NLT + 2, 48, wh::WH_CK_LDS_SCRATCH);
  const wh::ckp<double> wtab = wh::ck_sub(lds_all, NLT + 2 + 48, kWinTab, wh::WH_CK_LDS_AUX);  // window set-up table (kWinTab doubles)
  const wh::ckp<const double2> tw = wh::ck_make(tw_base, WH_TWIDDLE_ENTRIES, wh::WH_CK_TWIDDLE);
  const int64_t f = wh::xcd_unit(blockIdx.x, n_frames);
  if (f >= n_frames) return;
  double f0 = f0_io[f];
  if (vuv[f] == 0.0) f0 = 0.0;  // d4c.py:32 — written back (Q6)
  if (threadIdx.x == 0) f0_io[f] = f0;
  if (f0 == 0.0) {
    if (threadIdx.x == 0) gate[f] = 0;
    return;
  }
  const int u = frame_utt[f];
  const long long xn = x_off[u + 1] - x_off[u];
  const wh::ckp<const double> xu = wh::ck_make(x + x_off[u], xn, wh::WH_CK_WAVEFORM);
  const double cf = fmax(f0, 40.0);
  if (threadIdx.x == 0) win_setup(wtab, xn, fs, cf, tp[f], 1.5, FT);
  wh::sync<FT>();
  {
    // the frame's samples stay in registers from the gather through both walks (round 6): parked in LDS between them, the
    // window cost a store and two reads per sample on an LDS pipe this kernel keeps busy all the time
    double v[NLT / FT];
    d4c_window_regs<true, NLT, false, FT>(xu, wtab, win_thread_phase(wtab[9]), scratch, v);
#pragma unroll
    for (int q = 0; q < NLT / FT; ++q) zr[WH_TID + q * FT] = v[q];
  }
  wh::sync<FT>();
  wh::rfft_lds<NLT, FT, FT, kLoveMaxR>(zb, tw);  // (66 VGPRs here: the radix-8 plan fits, unlike in d4c_kernel)
  const int b0 = (int)(ceil(100.0 / (fs / NLT)) + 1);
  const int b1 = (int)(ceil(4000.0 / (fs / NLT)) + 1);
  const int b2 = (int)(ceil(7900.0 / (fs / NLT)) + 1);
  double s1 = 0.0, s2 = 0.0;
  {
    // the voicing decision s1 / s2 > 0.85 (d4c.py:86): powers, sums and ratio stay unfused, like NumPy's (ADVICE r5 — the
    // translation unit is compiled with contraction for its transforms; what feeds a discrete decision is not)
#pragma clang fp contract(off)
    for (int k = b0 + threadIdx.x; k < b2 && k < NLT; k += FT) {
      const double2 z = zb[k <= NLT / 2 ? k : NLT - k];  // |X[k]|^2 is even about NLT/2
      const double p = z.x * z.x + z.y * z.y;
      s2 += p;
      if (k < b1) s1 += p;
    }
  }
  wh::block_sum2<FT>(s1, s2, scratch);
  if (threadIdx.x == 0) gate[f] = (s1 / s2 > threshold) ? 1 : 0;
}

// Group-delay centroid of one Blackman frame, added into the run-resident cent (d4c.py:146-153).
// x and n*x (two real sequences) share ONE complex FFT: z = x + i*n*x, separated afterwards by symmetry.
template <int N>
__device__ __forceinline__ void add_centroid(wh::ckp<const double> xu, wh::ckp<const double> wtab, double2 e_tid,
                                             wh::ckp<double2> buf, double (&cent)[Runs<N>::KR], bool first,
                                             wh::ckp<const double2> tw_base, wh::ckp<double> scratch) {
  constexpr int FT = Runs<N>::FT, K = Runs<N>::K, KR = Runs<N>::KR;
  // z[j] = x[j] + i*(j+1)*x[j] (n is 1-based), normalised frame
  if constexpr (d4c_regfed<N>()) {
    double val[N / FT];
    d4c_window_regs<true, N, true>(xu, wtab, e_tid, scratch, val);
    double2 zin[N / FT];
#pragma unroll
    for (int q = 0; q < N / FT; ++q) zin[q] = make_double2(val[q], val[q] * (double)(WH_TID + q * FT + 1));
    wh::fft_lds_from_regs<N, false, FT, 8>(zin, buf, fresh_table(tw_base) + N);
  } else {
    // written straight into the transform buffer
    d4c_window<true, N, true, 2>(xu, wtab, e_tid, scratch, wh::ck_as<double>(buf),
                                 [&](int j, double val) { buf[j] = make_double2(val, val * (double)(j + 1)); });
    wh::sync<FT>();
    wh::fft_lds<N, false, FT, FT, 8>(buf, fresh_table(tw_base) + N);
  }
  const int k0 = threadIdx.x * KR;
#pragma unroll
  for (int r = 0; r < KR; ++r) {
    const int k = k0 + r;
    if (k < K) {
      const double2 a = buf[k];
      const double2 b = buf[(N - k) & (N - 1)];
      // S = (Z[k]+conj(Z[N-k]))/2 ; T = (Z[k]-conj(Z[N-k]))/(2i)
      const double sr = 0.5 * (a.x + b.x), si = 0.5 * (a.y - b.y);
      const double tr = 0.5 * (a.y + b.y), ti = -0.5 * (a.x - b.x);
      const double c = tr * sr + si * ti;  // -Im(W)Re(S)+Im(S)Re(W) with W = -i*T
      cent[r] = first ? c : cent[r] + c;
    }
  }
  wh::sync<FT>();  // buf is free again
}

// FUSED (love-train FFT size == D4C FFT size, the case at 16/22.05/44.1/48 kHz for d4c()): the VUV gate's
// Blackman frame and the Hann frame of the smoothed power spectrum are two real sequences → ONE complex FFT,
// separated by Hermitian symmetry; the separate love_train_kernel launch and one transform disappear.
template <int N, bool FUSED>
__device__ __forceinline__ void d4c_frame(
    const double* __restrict__ x, const int64_t* __restrict__ x_off, const int32_t* __restrict__ frame_utt,
    const double* __restrict__ tp, double* __restrict__ f0_io, const double* __restrict__ vuv,
    const int32_t* __restrict__ gate, double threshold, double fs, int nap, int interval,
    const double* __restrict__ window, int wlen, const double2* __restrict__ tw_base,
    int k_spec,                       // >0: dense amplitude output [F][k_spec]; 0: Requiem band output [F][nap+2]
    double* __restrict__ out, double* __restrict__ coarse_dbg, long long n_frames, const D4cLaunchConst& lc, int64_t f) {
  constexpr int FT = Runs<N>::FT, K = Runs<N>::K, KR = Runs<N>::KR;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // (wh::ckp<T> is T* in every shipped build; the bounds build checks each access against the range named here)
  const wh::ckp<double> lds_all = wh::ck_make(reinterpret_cast<double*>(smem), d4c_lds_doubles(N), wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> zr = wh::ck_sub(lds_all, 0, 2 * N, wh::WH_CK_LDS_MAIN);  // 2N doubles: real buffers, mirrored spectra, scratch
  const wh::ckp<double2> buf = wh::ck_as<double2>(zr);   // the same as N complex (centroid FFT) / N/2+1 complex (real FFTs)
  const wh::ckp<double> scratch = wh::ck_sub(lds_all, 2 * N, 40, wh::WH_CK_LDS_SCRATCH);  // 40 (block_sum5 at 8 waves)
  const wh::ckp<double> band = wh::ck_sub(lds_all, 2 * N + 40, 8, wh::WH_CK_LDS_AUX);     // nap (<= 8)
  const wh::ckp<double> wtab = wh::ck_sub(lds_all, 2 * N + 48, 4 * kWinTab, wh::WH_CK_LDS_AUX);  // 4 windows x kWinTab: gate, power, centroid +, centroid -
  constexpr int KPAD = (K + 1) & ~1;
  const wh::ckp<double> td = zr + (2 * N - KPAD);        // band stage: the shaped group delay, above the real-FFT buffer
  const wh::ckp<const double2> tw = wh::ck_make(tw_base, WH_TWIDDLE_ENTRIES, wh::WH_CK_TWIDDLE);  // the table of size n at offset n
  const wh::ckp<const double> win_tab = wh::ck_make(window, wlen, wh::WH_CK_TABLE);

  STAGE_TIMER_BEGIN
  if (f >= n_frames) return;
  const int u = frame_utt[f];
  const long long xn = x_off[u + 1] - x_off[u];
  const wh::ckp<const double> xu = wh::ck_make(x + x_off[u], xn, wh::WH_CK_WAVEFORM);
  const double pos = tp[f];
  double f0v = f0_io[f];
  bool voiced;
  if (FUSED) {
    if (vuv[f] == 0.0) f0v = 0.0;  // d4c.py:32 — written back (Q6)
    if (threadIdx.x == 0) f0_io[f] = f0v;
    voiced = f0v != 0.0;
  } else {
    voiced = gate[f] != 0;
  }
  const double cf = fmax(47.0, f0v);
  const int k0 = threadIdx.x * KR;
  double pw[KR], cent[KR];  // run-resident per-bin arrays
#pragma unroll
  for (int r = 0; r < KR; ++r) pw[r] = cent[r] = 0.0;
  // the four windows of the frame are set up by four lanes at once (win_setup); the three that share f0 and length
  // also share the per-thread phase factor e_frame
  if (voiced && threadIdx.x < 4) {
    const int wdx = threadIdx.x;
    const double wcf = wdx == 0 ? fmax(f0v, 40.0) : cf;
    const double wpos = wdx == 2 ? pos + 1 / cf / 4 : (wdx == 3 ? pos - 1 / cf / 4 : pos);
    win_setup(wtab + wdx * kWinTab, xn, fs, wcf, wpos, wdx == 0 ? 1.5 : 2.0, FT);
  }
  wh::sync<FT>();
  double2 e_frame = make_double2(0.0, 1.0);
  if (voiced) e_frame = win_thread_phase(wtab[kWinTab + 9]);
  if (FUSED && voiced) {
    // love-train frame (Blackman, 3*T0, f0 floored at 40 Hz) and smoothed-power frame (Hann, 4*T0) in one FFT
    if constexpr (d4c_regfed<N>()) {
      double va[N / FT], vb[N / FT];
      d4c_window_regs<true, N, false>(xu, wtab, win_thread_phase(wtab[9]), scratch, va);
      d4c_window_regs<false, N, false>(xu, wtab + kWinTab, e_frame, scratch, vb);
      STAGE_MARK(kStWindows)
      double2 zin[N / FT];
#pragma unroll
      for (int q = 0; q < N / FT; ++q) zin[q] = make_double2(va[q], vb[q]);
      wh::fft_lds_from_regs<N, false, FT, 8>(zin, buf, fresh_table(tw) + N);
    } else {
      d4c_window<true, N, false, 2>(xu, wtab, win_thread_phase(wtab[9]), scratch, zr, [&](int j, double val) { zr[2 * j] = val; });
      d4c_window<false, N, false, 2>(xu, wtab + kWinTab, e_frame, scratch, zr + 1, [&](int j, double val) { zr[2 * j + 1] = val; });
      STAGE_MARK(kStWindows)
      wh::sync<FT>();
      wh::fft_lds<N, false, FT, FT, 8>(buf, fresh_table(tw) + N);
    }
    STAGE_MARK(kStGateFft)
    const int b0 = lc.b0, b1 = lc.b1, b2 = lc.b2;
    double s1 = 0.0, s2 = 0.0;
    {
    // (the love-train powers feed the voicing decision below: unfused, see love_train_kernel)
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      const int k = k0 + r;
      if (k < K) {
        const double2 a = buf[k], b = buf[(N - k) & (N - 1)];
        const double ar = 0.5 * (a.x + b.x), ai = 0.5 * (a.y - b.y);   // love-train spectrum A[k]
        const double br = 0.5 * (a.y + b.y), bi = -0.5 * (a.x - b.x);  // Hann-frame spectrum B[k]
        pw[r] = br * br + bi * bi;
        const double pa = ar * ar + ai * ai;  // |A[k]|^2 = |A[N-k]|^2: bins k and N-k of the full power spectrum
        if (k >= b0 && k < b2) {
          s2 += pa;
          if (k < b1) s1 += pa;
        }
        const int km = N - k;  // mirrored bin (only reached when 7.9 kHz lies above fs/2)
        if (k > 0 && k < N / 2 && km >= b0 && km < b2) {
          s2 += pa;
          if (km < b1) s1 += pa;
        }
      }
    }
    }
    wh::block_sum2<FT>(s1, s2, scratch);  // (its barriers also free buf for the next stage)
    voiced = s1 / s2 > threshold;  // d4c.py:86
  }
  if (!voiced) {
    if (k_spec > 0) {
      const wh::ckp<double> o = wh::ck_make(out + f * (int64_t)k_spec, k_spec, wh::WH_CK_OUT);
      for (int k = threadIdx.x; k < k_spec; k += FT) o[k] = 1 - 0.000000000001;
      if (coarse_dbg) for (int b = threadIdx.x; b < nap; b += FT) coarse_dbg[f * nap + b] = 0.0;
    } else {
      const wh::ckp<double> o = wh::ck_make(out + f * (int64_t)(nap + 2), nap + 2, wh::WH_CK_OUT);
      for (int b = threadIdx.x; b < nap + 2; b += FT) o[b] = -0.000000000001;
    }
    return;
  }

  STAGE_MARK(kStGateFold)
  // ---- static centroid from two frames at +-T0/4 (d4c.py:132-142) ---------------------------------------
  // (one rolled copy of the centroid frame's code, run twice, lost: DESIGN.md §4 round 5)
  add_centroid<N>(xu, wtab + 2 * kWinTab, e_frame, buf, cent, true, tw, scratch);
  STAGE_MARK(kStCentroidA)
  add_centroid<N>(xu, wtab + 3 * kWinTab, e_frame, buf, cent, false, tw, scratch);
  STAGE_MARK(kStCentroidB)
  low_band_replica_runs<N>(cent, zr, fs, cf, 1.2 * cf);
  STAGE_MARK(kStReplica)

  // ---- smoothed power spectrum (d4c.py:157-161) ----------------------------------------------
  if (!FUSED) {
    d4c_window<false, N, false, 1>(xu, wtab + kWinTab, e_frame, scratch, zr, [&](int j, double val) { zr[j] = val; });
    wh::sync<FT>();
    wh::rfft_lds<N, FT, FT, 8>(buf, fresh_table(tw));
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      if (k0 + r < K) {
        const double2 z = buf[k0 + r];
        pw[r] = z.x * z.x + z.y * z.y;
      }
    }
    wh::sync<FT>();
  }
  const wh::ckp<double> cum = zr;  // the FFT buffer is idle during the smoothing steps (low-band scratch, then the mirrored spectra)
  const double inv_cf = 1.0 / cf;
  low_band_replica_runs<N>(pw, cum, fs, cf, 1.2 * cf);
  // the three rectangular smoothings as sliding windowed sums (wh_spectral.h: BandWindow) over the owned runs
  double bandv[KR];
  wh::BandWindow bw;
  fill_mirrored_runs<N>(pw, cum, fs);
  bw.init(cum, N, fs, cf / 2);
  bw.run<KR>(k0, K, bandv);
#pragma unroll
  for (int r = 0; r < KR; ++r) cent[r] = cent[r] / (bandv[r] * inv_cf);  // T_g = centroid / smoothed power (d4c.py:169; no zero guard, Q14)
  wh::sync<FT>();
  // ---- group-delay shaping (d4c.py:165-174) --------------------------------------------------
  fill_mirrored_runs<N>(cent, cum, fs);
  {
    const double w2 = cf / 2;
    const double inv_w2 = 1.0 / w2;
    bw.init(cum, N, fs, w2 / 2);
    bw.run<KR>(k0, K, bandv);
#pragma unroll
    for (int r = 0; r < KR; ++r) pw[r] = bandv[r] * inv_w2;  // T_gs
  }
  wh::sync<FT>();
  fill_mirrored_runs<N>(pw, cum, fs);
  bw.init(cum, N, fs, cf / 2);
  bw.run<KR>(k0, K, bandv);
  wh::sync<FT>();  // everyone is done with the mirrored spectrum before td (inside the same buffer) is written
#pragma unroll
  for (int r = 0; r < KR; ++r)
    if (k0 + r < K) td[k0 + r] = pw[r] - bandv[r] * inv_cf;  // T_D = T_gs - T_gb
  wh::sync<FT>();

  STAGE_MARK(kStSmooth)
  // ---- band-wise aperiodicity (d4c.py:192-209) -----------------------------------------------
  const int boundary = lc.boundary;
  const int half = wlen / 2;
  // The band window (Nuttall, wlen <= N / 2 + 1 taps: 2 * floor(interval / (fs / N)) + 1) is the same for every band: a
  // thread's taps j = tid + q FT are fetched ONCE, together, in front of the band loop.  Read inside the fill loop they
  // were one dependent global round trip per tap and band — the fill was 24 % of the N = 4096 instance's latency (five
  // bands at 48 kHz: 62.7 k of 258.7 k cycles per frame, tools/d4c_stage_timer.py 48000), more than the bands' transforms.
  constexpr int WQ = (N / 2 + 1 + FT - 1) / FT;
  double wv[WQ];
#pragma unroll
  for (int q = 0; q < WQ; ++q) {
    const int j = threadIdx.x + q * FT;
    wv[q] = win_tab[j < wlen ? j : 0];  // (clamped, not skipped: no branch per load)
  }
  for (int b = 0; b < nap; ++b) {
    const int centre = lc.centre[b];
#pragma unroll
    for (int q = 0; q < N / FT; ++q) {
      const int j = threadIdx.x + q * FT;
      double val = 0.0;
      if (j < wlen) {
        int idx = centre - half + j;          // index into the mirrored full group delay
        idx = idx < 0 ? -idx : idx;
        idx = idx > N / 2 ? N - idx : idx;
        val = td[idx] * (q < WQ ? wv[q < WQ ? q : 0] : win_tab[j]);
      }
      zr[j] = val;
    }
    wh::sync<FT>();
    STAGE_MARK(kStBandFill)
    // real transform of the windowed segment = half-size complex transform of its sample pairs + post-pass; only
    // |X[k]|^2 is needed, so the post-pass goes from the pair of bins (k, N/2 - k) straight to the two powers in the
    // thread's registers (the selection below takes its values in any distribution over the threads)
    constexpr int MB = N / 2;
    constexpr int PJ = (MB / 2 + 1 + FT - 1) / FT;  // pair jobs per thread
    double px[2 * PJ];
    unsigned pvalid = 0;
    {
      const wh::ckp<const double2> twb = fresh_table(tw);
      wh::fft_lds<MB, false, FT, FT, 8>(buf, twb + MB);
      const wh::ckp<const double2> WH_RESTRICT wpost = twb + N;
#pragma unroll
      for (int i = 0; i < PJ; ++i) {
        const int k = threadIdx.x + i * FT;
        px[2 * i] = px[2 * i + 1] = 0.0;
        if (k <= MB / 2) {
          const double2 a = buf[k], b = buf[MB - k];
          if (k == 0) {
            px[0] = (a.x + a.y) * (a.x + a.y);
            px[1] = (a.x - a.y) * (a.x - a.y);
            pvalid |= 3u;
          } else {
            const double er = 0.5 * (a.x + b.x), ei = 0.5 * (a.y - b.y);
            const double dr = 0.5 * (a.x - b.x), di = 0.5 * (a.y + b.y);
            const double2 wk = wh::ldg2(wpost + k);
            const double tr = fma(wk.x, di, wk.y * dr);
            const double ti = fma(wk.y, di, -(wk.x * dr));
            const double xr = er + tr, xi = ei + ti, yr = er - tr, yi = ti - ei;
            px[2 * i] = xr * xr + xi * xi;
            pvalid |= 1u << (2 * i);
            if (k != MB - k) {  // (the middle bin pairs with itself)
              px[2 * i + 1] = yr * yr + yi * yi;
              pvalid |= 2u << (2 * i);
            }
          }
        }
      }
    }
    STAGE_MARK(kStBandFft)
    wh::sync<FT>();  // the spectrum has been read: the lower part of the buffer becomes the selection's work area
    STAGE_MARK(kStBandPower)
    double s_small, s_total;
    sum_smallest<K, FT, 2 * PJ>(px, pvalid, N / 2 - boundary, zr, scratch, &s_small, &s_total);
    if (threadIdx.x == 0) band[b] = -10 * log10(s_small / s_total);
    wh::sync<FT>();
  }

  STAGE_MARK(kStSelect)
  // ---- outputs (d4c.py:56-59 / d4cRequiem.py:40) ---------------------------------------------
  const double tilt = (cf - 100) * 2 / 100;
  if (k_spec > 0) {
    if (coarse_dbg) for (int b = threadIdx.x; b < nap; b += FT) coarse_dbg[f * nap + b] = -fmax(0.0, band[b] - tilt);
    const wh::ckp<double> o = wh::ck_make(out + f * (int64_t)k_spec, k_spec, wh::WH_CK_OUT);
    // the interpolation over the coarse axis lives in wh_apbands.h, shared with ap_from_bands_kernel (wh_apbands.hip)
    const wh::ApAxis ax = wh::ap_axis(fs, nap, interval, k_spec);
    for (int k = threadIdx.x; k < k_spec; k += FT)
      o[k] = wh::ap_from_bands(ax, k, [&](int b) { return -fmax(0.0, band[b] - tilt); });
  } else {
    const wh::ckp<double> o = wh::ck_make(out + f * (int64_t)(nap + 2), nap + 2, wh::WH_CK_OUT);
    for (int b = threadIdx.x; b < nap + 2; b += FT)
      o[b] = b == 0 ? -60.0 : (b == nap + 1 ? -0.000000000001 : -fmax(0.0, band[b - 1] - tilt));
  }
  STAGE_MARK(kStOutput)
}

template <int N, bool FUSED>
__global__ __launch_bounds__(ft_of(N), minblk_of(N)) void d4c_kernel(
    const double* __restrict__ x, const int64_t* __restrict__ x_off, const int32_t* __restrict__ frame_utt,
    const double* __restrict__ tp, double* __restrict__ f0_io, const double* __restrict__ vuv,
    const int32_t* __restrict__ gate, double threshold, double fs, int nap, int interval,
    const double* __restrict__ window, int wlen, const double2* __restrict__ tw_base, int k_spec,
    double* __restrict__ out, double* __restrict__ coarse_dbg, long long n_frames, D4cLaunchConst lc) {
  d4c_frame<N, FUSED>(x, x_off, frame_utt, tp, f0_io, vuv, gate, threshold, fs, nap, interval, window, wlen, tw_base, k_spec, out,
                      coarse_dbg, n_frames, lc, wh::xcd_unit(blockIdx.x, n_frames));
}

int pow2_at_least(double v) { return (int)llround(pow(2.0, ceil(log2(v)))); }

// Nuttall window of (possibly float-valued) length n, world/d4c.py:237-245.
std::vector<double> nuttall(int n) {
  std::vector<double> w(n);
  for (int i = 0; i < n; ++i) {
    const double t = (double)i * 2 * M_PI / (double)(n - 1);
    w[i] = 0.355768 * cos(0 * t) + -0.487396 * cos(t) + 0.144232 * cos(2 * t) + -0.012604 * cos(3 * t);
  }
  return w;
}

// What the launchers of one wh_d4c / wh_d4c_requiem call share.
struct D4cCall {
  wh_ctx* ctx;
  hipStream_t st;
  const wh_batch* b;
  const double *x, *tp;
  double* f0;
  const double* vuv;
  double fs, thr;
  int32_t* gate;  // [F], the workspace
  int nap, interval;
  const double* win;  // the band window, wlen taps
  int wlen, k_spec;
  double *out, *coarse;
};

template <int NLT>
int launch_lt(const D4cCall& a) {
  const size_t lds = sizeof(double) * love_lds_doubles(NLT);
  if (int rc = wh::allow_lds(&love_train_kernel<NLT>, lds)) return rc;
  WH_LAUNCH(a.ctx, a.st, "love_train_kernel", love_train_kernel<NLT>, dim3((unsigned)wh::xcd_grid(a.b->total_frames)),
            dim3(ft_love(NLT)), lds, a.x, a.b->d_x_off, a.b->d_frame_utt, a.tp, a.f0, a.vuv, a.fs, a.thr,
            a.ctx->d_twiddle, a.gate, a.b->total_frames);
  return 0;
}

template <int N, bool FUSED>
int launch_main(const D4cCall& a) {
  const size_t lds = sizeof(double) * d4c_lds_doubles(N);
  if (int rc = wh::allow_lds(&d4c_kernel<N, FUSED>, lds)) return rc;
  WH_LAUNCH(a.ctx, a.st, "d4c_kernel", d4c_kernel<N, FUSED>, dim3((unsigned)wh::xcd_grid(a.b->total_frames)),
            dim3(ft_of(N)), lds, a.x, a.b->d_x_off, a.b->d_frame_utt, a.tp, a.f0, a.vuv, a.gate, a.thr, a.fs, a.nap,
            a.interval, a.win, a.wlen, a.ctx->d_twiddle, a.k_spec, a.out, a.coarse, a.b->total_frames,
            d4c_launch_const(a.fs, N, a.wlen, a.interval, a.nap));
  return 0;
}

int d4c_common(wh_ctx* ctx, void* stream, const wh_batch* b, const double* x, const double* tp, double* f0,
               const double* vuv, double fs, double threshold, int nfft, int interval, int k_spec, double* out,
               double* coarse) {
  if (b->total_frames == 0) return 0;
  const int nap = (int)floor(fmin(15000.0, fs / 2 - interval) / interval);
  if (nap <= 0) return wh::fail_msg("wh_d4c", "sampling rate too low: no aperiodicity band (reference asserts, d4c.py:35)");
  if (nap > 8) return wh::fail_msg("wh_d4c", "more than 8 aperiodicity bands unsupported");
  const int nlt = pow2_at_least(3 * fs / 40.0 + 1);
  const int wlen = (int)(floor(interval / (fs / nfft)) * 2 + 1);
  // workspace: gate[F]; the band window is a cached constant table
  if (int rc = wh::ws_reserve(ctx, (size_t)b->total_frames * sizeof(int32_t))) return rc;
  const double* d_win = nullptr;
  if (int rc = wh::const_table(ctx, "nuttall:" + std::to_string(wlen), nuttall(wlen), &d_win)) return rc;
  const D4cCall a = {ctx, (hipStream_t)stream, b, x, tp, f0, vuv, fs, threshold, reinterpret_cast<int32_t*>(ctx->ws),
                     nap, interval, d_win, wlen, k_spec, out, coarse};
  int rc = 0;
  const bool fused = nlt == nfft;  // fused love-train + D4C
  if (!fused) {
    if (!wh::dispatch_fft_size<8192>(nlt, [&](auto n) { rc = launch_lt<decltype(n)::value>(a); }))
      return wh::fail_msg("wh_d4c", "love-train FFT size outside [512, 8192] (fs must be <= ~109 kHz)");
    if (rc) return rc;
  }
  if (!wh::dispatch_fft_size<8192>(nfft, [&](auto n) {
        rc = fused ? launch_main<decltype(n)::value, true>(a) : launch_main<decltype(n)::value, false>(a);
      }))
    return wh::fail_msg("wh_d4c", "D4C FFT size outside [512, 8192]");
  return rc;
}

}  // namespace

#ifdef WH_D4C_STAGE_TIMER
extern "C" int wh_debug_d4c_stages(unsigned long long* out16, int reset) {
  (void)hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_d4c_stage), sizeof(unsigned long long) * 16);
  if (reset) {
    unsigned long long z[16] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_d4c_stage), z, sizeof(z));
  }
  return 0;
}
#endif

extern "C" int wh_d4c_bands(double fs, int requiem) {
  const int interval = (!requiem && fs < 16000) ? 2000 : 3000;
  return (int)floor(fmin(15000.0, fs / 2 - interval) / interval);
}

extern "C" int wh_d4c(wh_ctx* ctx, void* stream, const wh_batch* b, const double* x, const double* tp, double* f0,
                      const double* vuv, double fs, double threshold, int fft_size_for_spectrum, double* aperiodicity,
                      double* coarse_ap) {
  if (!ctx || !b || !x || !tp || !f0 || !vuv || !aperiodicity) return wh::fail_msg("wh_d4c", "null argument");
  WH_ENTER(ctx);
  if (fft_size_for_spectrum < 2) return wh::fail_msg("wh_d4c", "fft_size_for_spectrum must be >= 2");
  const int nfft = pow2_at_least(4 * fs / 47.0 + 1);
  const int interval = fs < 16000 ? 2000 : 3000;
  return d4c_common(ctx, stream, b, x, tp, f0, vuv, fs, threshold, nfft, interval, fft_size_for_spectrum / 2 + 1,
                    aperiodicity, coarse_ap);
}

extern "C" int wh_d4c_requiem(wh_ctx* ctx, void* stream, const wh_batch* b, const double* x, const double* tp,
                              double* f0, const double* vuv, double fs, double threshold, int fft_size,
                              double* band_aperiodicity) {
  if (!ctx || !b || !x || !tp || !f0 || !vuv || !band_aperiodicity) return wh::fail_msg("wh_d4c_requiem", "null argument");
  WH_ENTER(ctx);
  const int nfft = fft_size > 0 ? fft_size : pow2_at_least(3 * fs / 47.0 + 1);
  return d4c_common(ctx, stream, b, x, tp, f0, vuv, fs, threshold, nfft, 3000, 0, band_aperiodicity, nullptr);
}
