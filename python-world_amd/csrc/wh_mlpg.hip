// Dynamic features and maximum-likelihood parameter generation (MLPG): what a statistical model of WORLD parameters is
// trained on — static, delta and delta-delta rows — and what turns its predicted means and variances back into a track:
// per utterance and feature column the banded symmetric positive definite system (sum_w W_w' P_w W_w) c = sum_w W_w' P_w mu_w.
// The arithmetic is a contract (include/world_hip.h; tests/_mlpg_reference.py is the same contract in
// NumPy and the results agree bit for bit): every sum starts from 0.0 and is unfused, every product is rounded on its own
// and grouped as written, a precision is one correctly rounded division, the factorisation is a sequential banded LDL'
// with one reciprocal per pivot and every subtraction running from the farthest predecessor to the nearest.
//
// delta_features_kernel: one thread per output element; a tap that reaches outside the frame's own utterance is skipped.
// mlpg_kernel<B> (B = 2L = 0, 2, 4): one lane per system, systems numbered u * d + column, 64 consecutive systems per
// wave — with d >= 64 the lanes read consecutive doubles of one frame row, with d = 1 (log-f0) 64 utterances share a
// wave; a lane is predicated off past its own T and the wave runs to its longest.  The forward sweep ingests frame
// s = t + L and solves row t: the last 2L + 1 frames of precisions and means slide through registers, R's row and r[t]
// are summed from them, the previous B rows of multipliers and reciprocals stay in registers.  A frame outside the
// utterance enters the window as precision 0 and mean 0: its terms are +-0.0, and a sum that starts from +0.0 in round
// to nearest is never -0.0, so adding them changes no bit — the edges need no branch.  The raw variances and means of
// the kMlpgAhead frames after the one being ingested are in flight in a register ring (a slot is refilled as soon as it
// has been consumed), so the loads are issued far ahead of the chain mul - mul - sub - reciprocal that a step waits on.
// The multipliers go to the context's scratch laid out [frame][k][column] (B doubles per element, coalesced like the rows),
// y[t] = z[t] * q[t] goes to `out`, and the backward sweep reads both back from T - 1 down, again through a ring.
// No atomics except the flag; no LDS; a system's result does not depend on the batch it is in.
#include <math.h>

#include "wh_device.h"
#include "wh_host.h"

namespace {

constexpr int kMlpgMaxWin = 4;
constexpr int kMlpgMaxTaps = 5;
constexpr int kMlpgAhead = 4;  // frames in flight ahead of the chain, forward and backward

struct MlpgWindows {
  double w[kMlpgMaxWin][kMlpgMaxTaps];  // [window][tap a + L]; taps beyond 2L and windows beyond n_win are 0
};

__global__ __launch_bounds__(WH_BLOCK) void delta_features_kernel(const int64_t* __restrict__ frame_off_, int n_utt,
                                                                  const int32_t* __restrict__ frame_utt_, long long frames,
                                                                  const double* __restrict__ x_, long long ldx, long long len_x,
                                                                  int d, int n_win, int half, MlpgWindows win,
                                                                  double* __restrict__ out_, long long ldo, long long len_o) {
  const wh::ckp<const int64_t> frame_off = wh::ck_make(frame_off_, (long long)n_utt + 1, wh::WH_CK_TABLE);
  const wh::ckp<const int32_t> frame_utt = wh::ck_make(frame_utt_, frames, wh::WH_CK_TABLE);
  const wh::ckp<const double> x = wh::ck_make(x_, len_x, wh::WH_CK_IN);
  const wh::ckp<double> out = wh::ck_make(out_, len_o, wh::WH_CK_OUT);
  const long long width = (long long)n_win * d;
  const long long e = (long long)blockIdx.x * WH_BLOCK + threadIdx.x;
  if (e >= frames * width) return;
  const long long f = e / width;
  const int col = (int)(e - f * width), w = col / d, c = col - w * d;
  const int u = frame_utt[f];
  const long long f0 = frame_off[0], lo = frame_off[u] - f0, hi = frame_off[u + 1] - f0;  // the utterance's rows
  double acc = 0.0;
  for (int a = -half; a <= half; ++a) {
    const long long g = f + a;
    if (g >= lo && g < hi) acc = acc + win.w[w][a + half] * x[g * ldx + c];
  }
  out[f * ldo + col] = acc;
}

// Forward sweep and backward sweep of every system.  L = B / 2.
template <int B>
__global__ __launch_bounds__(WH_WAVE) void mlpg_kernel(const int64_t* __restrict__ frame_off_, int n_utt, long long frames,
                                                       const double* __restrict__ mean_, long long ldm, long long len_m,
                                                       const double* __restrict__ var_, long long ldv, long long len_v,
                                                       int d, int n_win, MlpgWindows win, double* __restrict__ out_,
                                                       long long ldo, long long len_o, double* __restrict__ mult_,
                                                       long long len_l, double* __restrict__ piv_, int32_t* flags) {
  constexpr int L = B / 2, NT = 2 * L + 1, PF = kMlpgAhead, NW = kMlpgMaxWin;
  const wh::ckp<const int64_t> frame_off = wh::ck_make(frame_off_, (long long)n_utt + 1, wh::WH_CK_TABLE);
  const wh::ckp<const double> mean = wh::ck_make(mean_, len_m, wh::WH_CK_IN);
  const wh::ckp<const double> var = wh::ck_make(var_, len_v, wh::WH_CK_IN);
  const wh::ckp<double> out = wh::ck_make(out_, len_o, wh::WH_CK_OUT);
  const wh::ckp<double> mult = wh::ck_make(mult_, len_l, wh::WH_CK_LDS_SCRATCH);
  const wh::ckp<double> piv = wh::ck_make(piv_, piv_ ? frames * d : 0, wh::WH_CK_OUT);
  const long long g = (long long)blockIdx.x * WH_WAVE + threadIdx.x;  // the system: u * d + column
  const bool act = g < (long long)n_utt * d;
  const long long u = act ? g / d : 0;
  const int c = act ? (int)(g - u * d) : 0;
  const long long fb = frame_off[0];
  const long long f0 = frame_off[u] - fb;                    // the utterance's first row
  const long long T = act ? frame_off[u + 1] - fb - f0 : 0;  // its frames; an idle lane has none

  // ---- forward: ingest frame s, solve row t = s - L ------------------------------------------------------------------
  double rv[PF][NW], rm[PF][NW];  // the ring: raw variances and means of frames s .. s + PF - 1
  auto fetch = [&](int slot, long long s) {
    const bool ok = s < T;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      if (w < n_win) {
        rv[slot][w] = ok ? var[(f0 + s) * ldv + (long long)w * d + c] : 1.0;
        rm[slot][w] = ok ? mean[(f0 + s) * ldm + (long long)w * d + c] : 0.0;
      }
    }
  };
  double p[NW][NT], mu[NW][NT];  // the window: slot i holds frame t - L + i
#pragma unroll
  for (int w = 0; w < NW; ++w)
#pragma unroll
    for (int i = 0; i < NT; ++i) p[w][i] = mu[w][i] = 0.0;
  double lp[B > 0 ? B : 1][B > 0 ? B : 1];  // lp[n - 1][k - 1]: multiplier k of row t - n
  double qp[B > 0 ? B : 1], zp[B > 0 ? B : 1];  // q and z of rows t - 1 .. t - B
#pragma unroll
  for (int n = 0; n < (B > 0 ? B : 1); ++n) {
    qp[n] = zp[n] = 0.0;
#pragma unroll
    for (int k = 0; k < (B > 0 ? B : 1); ++k) lp[n][k] = 0.0;
  }
  bool bad = false;
#pragma unroll
  for (int i = 0; i < PF; ++i) fetch(i, i);
  for (long long s0 = 0; __any(s0 < T + L); s0 += PF) {
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const long long s = s0 + i, t = s - L;
      // the window moves on by one frame; the newest is frame s (absent past the end: precision 0, mean 0)
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        if (w < n_win) {
#pragma unroll
          for (int j = 0; j + 1 < NT; ++j) {
            p[w][j] = p[w][j + 1];
            mu[w][j] = mu[w][j + 1];
          }
          p[w][NT - 1] = s < T ? 1.0 / rv[i][w] : 0.0;
          mu[w][NT - 1] = rm[i][w];
        }
      }
      fetch(i, s + PF);
      // R[t-k][t], k = 0 .. B, and r[t]: w ascending, then the frames ascending
      double R[B + 1], r = 0.0;
#pragma unroll
      for (int k = 0; k <= B; ++k) R[k] = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        if (w < n_win) {
#pragma unroll
          for (int j = 0; j < NT; ++j) {
#pragma unroll
            for (int k = 0; k <= B; ++k)
              if (j + k < NT) R[k] = R[k] + (win.w[w][NT - 1 - j - k] * p[w][j]) * win.w[w][NT - 1 - j];
            r = r + (win.w[w][NT - 1 - j] * p[w][j]) * mu[w][j];
          }
        }
      }
      // row t of the factorisation: v[k] = l[t][k] d[t-k], farthest column first
      double v[B + 1], l[B + 1];
#pragma unroll
      for (int k = B; k >= 1; --k) {
        double a = R[k];
#pragma unroll
        for (int n = B; n > k; --n) a = a - v[n] * lp[k - 1][n - k - 1];
        v[k] = t >= k ? a : 0.0;  // a column in front of the utterance does not exist
        l[k] = v[k] * qp[k - 1];
      }
      double dd = R[0], z = r;
#pragma unroll
      for (int k = B; k >= 1; --k) dd = dd - v[k] * l[k];
#pragma unroll
      for (int k = B; k >= 1; --k) z = z - l[k] * zp[k - 1];
      const double q = 1.0 / dd;
      const bool live = t >= 0 && t < T;
      if (live) {
        if (!(dd > 0.0 && dd < __builtin_inf())) bad = true;
        const long long f = f0 + t;
        out[f * ldo + c] = z * q;
#pragma unroll
        for (int k = 1; k <= B; ++k) mult[(f * B + (k - 1)) * d + c] = l[k];
        if (piv_) piv[f * d + c] = dd;
        // rows t - 1 .. t - B move on by one.  In front of the utterance they hold zeros: the contract's sums stop at
        // m = min(B, t), and the terms beyond are +0.0 * x subtracted from a value that is never -0.0 — no bit changes
#pragma unroll
        for (int n = B - 1; n >= 1; --n) {
          qp[n] = qp[n - 1];
          zp[n] = zp[n - 1];
#pragma unroll
          for (int k = 0; k < B; ++k) lp[n][k] = lp[n - 1][k];
        }
        if (B > 0) {
          qp[0] = q;
          zp[0] = z;
#pragma unroll
          for (int k = 1; k <= B; ++k) lp[0][k - 1] = l[k];
        }
      }
    }
  }
  if (bad) atomicOr(flags + WH_FLAG_MLPG_PIVOT, 1);
  if (B == 0) return;  // diagonal systems: y is the solution

  // ---- backward: c[t] = y[t] - sum l[t+k][k] c[t+k], k from the farthest to the nearest, t from T - 1 down ----------
  // step j handles t = T - 1 - j of the lane's own utterance; what it loads was stored by this lane
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double ry[PF], rl[PF][B > 0 ? B : 1];  // y[t] and l[t+k][k], k = 1 .. B
  auto fetch_b = [&](int slot, long long j) {
    const long long t = T - 1 - j;
    const bool ok = t >= 0;
    ry[slot] = ok ? out[(f0 + t) * ldo + c] : 0.0;
#pragma unroll
    for (int k = 1; k <= B; ++k) rl[slot][k - 1] = (ok && t + k < T) ? mult[((f0 + t + k) * B + (k - 1)) * d + c] : 0.0;
  };
  double cp[B > 0 ? B : 1];  // c[t+1] .. c[t+B]
#pragma unroll
  for (int k = 0; k < B; ++k) cp[k] = 0.0;
#pragma unroll
  for (int i = 0; i < PF; ++i) fetch_b(i, i);
  for (long long j0 = 0; __any(j0 < T); j0 += PF) {
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const long long j = j0 + i, t = T - 1 - j;
      double cc = ry[i];
      double lk[B > 0 ? B : 1];
#pragma unroll
      for (int k = 0; k < B; ++k) lk[k] = rl[i][k];
      fetch_b(i, j + PF);
#pragma unroll
      for (int k = B; k >= 1; --k) cc = cc - lk[k - 1] * cp[k - 1];
      if (t >= 0) {
        out[(f0 + t) * ldo + c] = cc;
#pragma unroll
        for (int k = B - 1; k >= 1; --k) cp[k] = cp[k - 1];
        cp[0] = cc;
      }
    }
  }
}

int mlpg_windows(const char* where, int n_win, int half, const double* h_win, MlpgWindows* out) {
  if (n_win < 1 || n_win > kMlpgMaxWin) return wh::fail_msg(where, "n_win must be in [1, 4]");
  if (half < 0 || half > 2) return wh::fail_msg(where, "the windows' half-width must be 0, 1 or 2");
  if (!h_win) return wh::fail_msg(where, "null argument");
  const int nt = 2 * half + 1;
  for (int w = 0; w < kMlpgMaxWin; ++w)
    for (int a = 0; a < kMlpgMaxTaps; ++a) out->w[w][a] = (w < n_win && a < nt) ? h_win[w * nt + a] : 0.0;
  for (int a = 0; a < nt; ++a)
    if (!(h_win[a] == (a == half ? 1.0 : 0.0)))
      return wh::fail_msg(where, "window 0 must be the static window: centre tap 1.0, every other tap 0.0");
  return 0;
}

}  // namespace

extern "C" int wh_delta_features(wh_ctx* ctx, void* stream, const wh_batch* b, const double* x, int64_t ldx, int d, int n_win,
                                 int half, const double* h_win, double* out, int64_t ldo) {
  if (!ctx || !b) return wh::fail_msg("wh_delta_features", "null argument");
  WH_ENTER(ctx);
  MlpgWindows win;
  if (int rc = mlpg_windows("wh_delta_features", n_win, half, h_win, &win)) return rc;
  if (d < 1) return wh::fail_msg("wh_delta_features", "d must be >= 1");
  if (ldx < d) return wh::fail_msg("wh_delta_features", "ldx must be at least d");
  if (ldo < (int64_t)n_win * d) return wh::fail_msg("wh_delta_features", "ldo must be at least n_win * d");
  const long long frames = b->total_frames;
  if (frames == 0) return 0;
  if (!x || !out) return wh::fail_msg("wh_delta_features", "null argument");
  const long long width = (long long)n_win * d, total = frames * width;
  const long long blocks = (total + WH_BLOCK - 1) / WH_BLOCK;
  if (blocks > 0x7fffffffLL) return wh::fail_msg("wh_delta_features", "too many output elements for one call");
  hipStream_t st = (hipStream_t)stream;
  WH_LAUNCH(ctx, st, "delta_features_kernel", delta_features_kernel, dim3((unsigned)blocks), dim3(WH_BLOCK), 0,
            b->d_frame_off, b->n_utt, b->d_frame_utt, frames, x, ldx, (frames - 1) * ldx + d, d, n_win, half, win, out,
            ldo, (frames - 1) * ldo + width);
  return 0;
}

extern "C" int wh_mlpg(wh_ctx* ctx, void* stream, const wh_batch* b, const double* mean, int64_t ldm, const double* var,
                       int64_t ldv, int d, int n_win, int half, const double* h_win, double* out, int64_t ldo,
                       double* pivots_out) {
  if (!ctx || !b) return wh::fail_msg("wh_mlpg", "null argument");
  WH_ENTER(ctx);
  MlpgWindows win;
  if (int rc = mlpg_windows("wh_mlpg", n_win, half, h_win, &win)) return rc;
  if (d < 1) return wh::fail_msg("wh_mlpg", "d must be >= 1");
  const long long width = (long long)n_win * d;
  if (ldm < width) return wh::fail_msg("wh_mlpg", "ldm must be at least n_win * d");
  if (ldv != 0 && ldv < width) return wh::fail_msg("wh_mlpg", "ldv must be 0 (one row for every frame) or at least n_win * d");
  if (ldo < d) return wh::fail_msg("wh_mlpg", "ldo must be at least d");
  const long long frames = b->total_frames;
  for (int u = 0; u < b->n_utt; ++u)
    if (b->h_frame_off[u + 1] - b->h_frame_off[u] > 0x7fffffffLL) return wh::fail_msg("wh_mlpg", "an utterance has too many frames");
  if (frames == 0) return 0;
  if (!mean || !var || !out) return wh::fail_msg("wh_mlpg", "null argument");
  const long long systems = (long long)b->n_utt * d, waves = (systems + WH_WAVE - 1) / WH_WAVE;
  if (waves > 0x7fffffffLL) return wh::fail_msg("wh_mlpg", "too many systems for one call");
  hipStream_t st = (hipStream_t)stream;
  const int B = 2 * half;
  const long long len_l = frames * B * d;
  double* mult = nullptr;
  if (B > 0)
    if (int rc = wh::persistent_scratch(ctx, "mlpg.scratch", (size_t)len_l, &mult)) return rc;
  const long long len_m = (frames - 1) * ldm + width, len_v = ldv ? (frames - 1) * ldv + width : width;
  const long long len_o = (frames - 1) * ldo + d;
  WH_LAUNCH(ctx, st, "mlpg_kernel", B == 0 ? mlpg_kernel<0> : B == 2 ? mlpg_kernel<2> : mlpg_kernel<4>,
            dim3((unsigned)waves), dim3(WH_WAVE), 0, b->d_frame_off, b->n_utt, frames, mean, ldm, len_m, var, ldv,
            len_v, d, n_win, win, out, ldo, len_o, mult, len_l, pivots_out, ctx->d_flags);
  return 0;
}
