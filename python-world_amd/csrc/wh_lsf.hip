// Line spectral frequencies: the all-pole code of a spectral envelope that is valid at every sampling rate.  Per frame and
// independent: autocorrelation lags (wh_feature_matmul with a cosine table, no kernel here) -> Levinson-Durbin
// (lpc_levinson_kernel) -> the roots of the two Chebyshev series of P and Q in the cosine domain x = cos w
// (lsf_from_lpc_kernel) and back: rows [E, x_1 .. x_p] -> power spectrum in product form (lsf_envelope_kernel).
// The arithmetic is a contract (include/world_hip.h; tests/_lsf_reference.py is the same contract in
// NumPy and the results agree bit for bit): every sum is sequential and unfused (this unit is compiled with build.py's
// default -ffp-contract=off), every product is rounded on its own and grouped as written, and no kernel calls a
// transcendental — the only trigonometry is the two host tables the entries are handed.
//
// lpc_levinson_kernel: one lane per frame, 64 frames per workgroup.  A lane's r[0..p] and a[0..p] live in LDS laid out
//   [index][lane] (a dynamically indexed private array would go to scratch; with the lane as the fastest index every
//   access of a wave is conflict-free), the order-n update runs in place from both ends.
// lsf_from_lpc_kernel<LPF>: one wave per frame (LPF = 64), or two frames per wave on its two halves while a frame's roots
//   fit 32 lanes (p <= 32, LPF = 32); four waves per workgroup.  Lanes over the grid points: the 2 (m + 1) series
//   coefficients are LDS reads of one address per frame (broadcast), a ballot gives the sign pattern of LPF points at a
//   time and the lane that owns a sign change files its bracket under the root's ordinal; then one lane per root bisects
//   its bracket, P's roots on the even lanes' slots and Q's on the odd ones.  The level loop runs while any frame of the
//   wave is short of brackets; a frame that has them keeps them.  The bits do not depend on LPF.
// lsf_envelope_kernel: kEnvFrames frames per workgroup, the doubled roots and E in LDS, one thread per bin.
#include <math.h>

#include "wh_device.h"
#include "wh_host.h"

namespace {

constexpr int kLsfMaxOrder = 64;
constexpr int kLsfMaxHalf = kLsfMaxOrder / 2;
constexpr int kLsfGridMin = 256;
constexpr int kLsfGridMax = 4096;
constexpr int kLsfMaxBisect = 60;
constexpr int kLsfWaves = 4;   // frames per workgroup of lsf_from_lpc_kernel
constexpr int kEnvFrames = 8;  // frames per workgroup of lsf_envelope_kernel
constexpr int kEnvThreads = 256;

// ---- b. Levinson-Durbin ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WH_WAVE) void lpc_levinson_kernel(const double* __restrict__ r_, long long n_frames,
                                                               long long ldr, int p, double* __restrict__ a_,
                                                               long long lda, double* __restrict__ e_,
                                                               double* __restrict__ k_, long long ldk, int32_t* flags) {
  extern __shared__ double s_lev[];
  const long long f = (long long)blockIdx.x * WH_WAVE + threadIdx.x;
  const bool act = f < n_frames;
  const int lane = threadIdx.x, n1 = p + 1;
  const wh::ckp<const double> r = wh::ck_make(r_, (n_frames - 1) * ldr + n1, wh::WH_CK_IN);
  const wh::ckp<double> a = wh::ck_make(a_, (n_frames - 1) * lda + n1, wh::WH_CK_OUT);
  const wh::ckp<double> e_out = wh::ck_make(e_, n_frames, wh::WH_CK_OUT);
  const wh::ckp<double> refl = wh::ck_make(k_, k_ ? (n_frames - 1) * ldk + p : 0, wh::WH_CK_OUT);
  const wh::ckp<double> sr = wh::ck_make(s_lev, (long long)n1 * WH_WAVE, wh::WH_CK_LDS_MAIN);
  const wh::ckp<double> sa = wh::ck_make(s_lev + n1 * WH_WAVE, (long long)n1 * WH_WAVE, wh::WH_CK_LDS_AUX);
  for (int i = 0; i < n1; ++i) {
    sr[i * WH_WAVE + lane] = act ? r[f * ldr + i] : 1.0;
    sa[i * WH_WAVE + lane] = i == 0 ? 1.0 : 0.0;
  }
  double e = sr[lane];
  const bool zero = e == 0.0;
  bool bad = !zero && !(e > 0.0 && e < __builtin_inf());
  for (int n = 1; n <= p; ++n) {
    double acc = sr[n * WH_WAVE + lane];
    for (int i = 1; i < n; ++i) acc = acc + sa[i * WH_WAVE + lane] * sr[(n - i) * WH_WAVE + lane];
    const double k = -(acc / e);
    for (int i = 1; i <= n / 2; ++i) {
      const double ai = sa[i * WH_WAVE + lane], aj = sa[(n - i) * WH_WAVE + lane];
      sa[i * WH_WAVE + lane] = ai + k * aj;
      sa[(n - i) * WH_WAVE + lane] = aj + k * ai;
    }
    sa[n * WH_WAVE + lane] = k;
    if (k_ && act) refl[f * ldk + n - 1] = k;
    e = e * (1.0 - k * k);
    if (!zero && !(e > 0.0 && e < __builtin_inf())) bad = true;
  }
  if (!act) return;
  const double nan = __builtin_nan("");
  for (int i = 0; i < n1; ++i) a[f * lda + i] = bad ? nan : zero ? (i == 0 ? 1.0 : 0.0) : sa[i * WH_WAVE + lane];
  e_out[f] = bad ? nan : zero ? 0.0 : e;
  if (k_ && (bad || zero))
    for (int i = 0; i < p; ++i) refl[f * ldk + i] = bad ? nan : 0.0;
  if (bad) atomicOr(flags + WH_FLAG_LSF, 1);
}

// ---- c. the roots of the two series ------------------------------------------------------------------------------------
// sum c[k] T_k(x) by Clenshaw's recurrence; c is laid out with stride 2 (P's and Q's coefficients interleaved)
__device__ __forceinline__ double lsf_clenshaw(const wh::ckp<const double>& c, int m, double x) {
  const double tx = 2.0 * x;
  double b1 = 0.0, b2 = 0.0;
  for (int k = m; k >= 1; --k) {
    const double b0 = (tx * b1 - b2) + c[2 * k];
    b2 = b1;
    b1 = b0;
  }
  return (x * b1 - b2) + c[0];
}

// LPF lanes per frame: 64 (one frame per wave) or, for p <= 32, 32 (two frames per wave, each on its own half)
template <int LPF>
__global__ __launch_bounds__(kLsfWaves* WH_WAVE) void lsf_from_lpc_kernel(const double* __restrict__ a_, long long n_frames,
                                                                          long long lda, int p,
                                                                          const double* __restrict__ grid_,
                                                                          double* __restrict__ x_, long long ldx,
                                                                          int32_t* __restrict__ level_, int32_t* flags) {
  constexpr int FPW = WH_WAVE / LPF;                                 // frames per wave
  constexpr unsigned long long kMask = ~0ull >> (WH_WAVE - LPF);     // the LPF sign bits of a frame's round
  __shared__ double s_g[kLsfWaves * FPW][2 * (kLsfMaxHalf + 1)];  // the deflated halves g (P) and h (Q), interleaved
  __shared__ double s_c[kLsfWaves * FPW][2 * (kLsfMaxHalf + 1)];  // the series' coefficients, interleaved
  __shared__ int s_b[kLsfWaves * FPW][kLsfMaxOrder];              // brackets: 2 j + (f(x_(j-1)) < 0), slot 2 i P's, 2 i + 1 Q's
  const int wave = threadIdx.x / WH_WAVE, lane = threadIdx.x % WH_WAVE;
  const int grp = lane / LPF, gl = lane % LPF, slot = wave * FPW + grp;
  const long long f_first = ((long long)blockIdx.x * kLsfWaves + wave) * FPW;
  if (f_first >= n_frames) return;  // (wave-uniform; the waves of a workgroup share nothing and meet at no barrier)
  // a half without a frame of its own (the last wave of an odd count) repeats the last frame and writes nothing
  const bool act = f_first + grp < n_frames;
  const long long f = act ? f_first + grp : n_frames - 1;
  const int m = p / 2, n1 = p + 1;
  const wh::ckp<const double> a = wh::ck_make(a_, (n_frames - 1) * lda + n1, wh::WH_CK_IN);
  const wh::ckp<const double> grid = wh::ck_make(grid_, kLsfGridMax + 1, wh::WH_CK_TABLE);
  const wh::ckp<double> x = wh::ck_make(x_, (n_frames - 1) * ldx + p, wh::WH_CK_OUT);
  const wh::ckp<int32_t> level = wh::ck_make(level_, level_ ? n_frames : 0, wh::WH_CK_OUT);
  const wh::ckp<double> g = wh::ck_make(&s_g[slot][0], 2 * (kLsfMaxHalf + 1), wh::WH_CK_LDS_MAIN);
  const wh::ckp<double> c = wh::ck_make(&s_c[slot][0], 2 * (kLsfMaxHalf + 1), wh::WH_CK_LDS_AUX);
  const wh::ckp<int> br = wh::ck_make(&s_b[slot][0], kLsfMaxOrder, wh::WH_CK_LDS_OTHER);
  // the deflation is a sequential recurrence: the frame's lane 0 runs P's, lane 1 Q's
  if (gl < 2) {
    double prev = a[f * lda];
    g[gl] = prev;
    for (int i = 1; i <= m; ++i) {
      const double lo = a[f * lda + i], hi = a[f * lda + n1 - i];
      prev = gl == 0 ? (lo + hi) - prev : (lo - hi) + prev;
      g[2 * i + gl] = prev;
    }
  }
  wh::sync<WH_WAVE>();
  for (int i = gl; i < 2 * (m + 1); i += LPF) {
    const int k = i >> 1, s = i & 1;
    c[i] = k == 0 ? g[2 * m + s] : 2.0 * g[2 * (m - k) + s];
  }
  wh::sync<WH_WAVE>();
  const wh::ckp<const double> cp = wh::ckp<const double>(c), cq = wh::ckp<const double>(c + 1);
  int found = 0;
  for (int G = kLsfGridMin; G <= kLsfGridMax && __any(found == 0); G *= 2) {  // (every lane runs the rounds: the ballots)
    const bool open = found == 0;  // a frame that has its brackets keeps them
    const int stride = kLsfGridMax / G;
    int n_p = 0, n_q = 0;
    unsigned long long last_p = 0, last_q = 0;  // the sign bit of the point in front of the round's first
    for (int j0 = 0; j0 <= G; j0 += LPF) {
      const int j = j0 + gl < G ? j0 + gl : G;  // (the last round is the point G alone: every lane repeats it)
      const double xj = grid[j * stride];
      const unsigned long long mp = (__ballot(lsf_clenshaw(cp, m, xj) < 0.0) >> (grp * LPF)) & kMask;
      const unsigned long long mq = (__ballot(lsf_clenshaw(cq, m, xj) < 0.0) >> (grp * LPF)) & kMask;
      if (j0 == 0) {
        last_p = mp & 1ull;
        last_q = mq & 1ull;
      }
      const unsigned long long before_p = ((mp << 1) | last_p) & kMask, before_q = ((mq << 1) | last_q) & kMask;
      const unsigned long long ch_p = mp ^ before_p, ch_q = mq ^ before_q;
      const unsigned long long below = (1ull << gl) - 1ull;
      if (open && ((ch_p >> gl) & 1ull)) {
        const int ord = n_p + __popcll(ch_p & below);
        if (ord < m) br[2 * ord] = 2 * j + (int)((before_p >> gl) & 1ull);
      }
      if (open && ((ch_q >> gl) & 1ull)) {
        const int ord = n_q + __popcll(ch_q & below);
        if (ord < m) br[2 * ord + 1] = 2 * j + (int)((before_q >> gl) & 1ull);
      }
      n_p += __popcll(ch_p);
      n_q += __popcll(ch_q);
      last_p = (mp >> (LPF - 1)) & 1ull;
      last_q = (mq >> (LPF - 1)) & 1ull;
    }
    if (open && n_p >= m && n_q >= m) found = G;
  }
  wh::sync<WH_WAVE>();
  if (level_ && act && gl == 0) level[f] = found;
  if (!found && act) {
    if (gl < p) x[f * ldx + gl] = __builtin_nan("");
    if (gl == 0) atomicOr(flags + WH_FLAG_LSF, 1);
  }
  if (!__any(found != 0)) return;
  // one lane per root: slot `gl` is root gl / 2 of P (even) or Q (odd) — the interlaced order of the output
  const bool own = found != 0 && gl < p;
  const int stride = kLsfGridMax / (found ? found : kLsfGridMax);
  const int code = own ? br[gl] : 2;
  const int j = code >> 1;
  const bool n_hi = code & 1;
  double lo = grid[j * stride], hi = grid[(j - 1) * stride];
  const wh::ckp<const double> cs = wh::ckp<const double>(c + (gl & 1));
  for (int it = 0; it < kLsfMaxBisect; ++it) {
    const double mid = 0.5 * (lo + hi);
    const bool live = own && mid != lo && mid != hi;
    if (!__any(live)) break;
    const bool same = (lsf_clenshaw(cs, m, mid) < 0.0) == n_hi;
    if (live && same) hi = mid;
    if (live && !same) lo = mid;
  }
  if (own && act) x[f * ldx + gl] = 0.5 * (lo + hi);
}

// ---- d. rows [E, x_1 .. x_p] -> power spectrum ---------------------------------------------------------------------------
__global__ __launch_bounds__(kEnvThreads) void lsf_envelope_kernel(const double* __restrict__ rows_, long long n_frames,
                                                                   long long ldr, int p, const double* __restrict__ cos_,
                                                                   int k_bins, double* __restrict__ out_, long long ldo) {
  __shared__ double s_x[kEnvFrames][kLsfMaxOrder];  // 2 x_i
  __shared__ double s_e[kEnvFrames];
  const wh::ckp<const double> rows = wh::ck_make(rows_, (n_frames - 1) * ldr + p + 1, wh::WH_CK_IN);
  const wh::ckp<const double> ctab = wh::ck_make(cos_, k_bins, wh::WH_CK_TABLE);
  const wh::ckp<double> out = wh::ck_make(out_, (n_frames - 1) * ldo + k_bins, wh::WH_CK_OUT);
  const wh::ckp<double> sx = wh::ck_make(&s_x[0][0], kEnvFrames * kLsfMaxOrder, wh::WH_CK_LDS_MAIN);
  const wh::ckp<double> se = wh::ck_make(s_e, kEnvFrames, wh::WH_CK_LDS_AUX);
  const long long f0 = (long long)blockIdx.x * kEnvFrames;
  const int nf = (int)(n_frames - f0 < kEnvFrames ? n_frames - f0 : kEnvFrames);
  for (int i = threadIdx.x; i < nf * (p + 1); i += kEnvThreads) {
    const int fr = i / (p + 1), col = i - fr * (p + 1);
    const double v = rows[(f0 + fr) * ldr + col];
    if (col == 0) se[fr] = v;
    else sx[fr * kLsfMaxOrder + col - 1] = 2.0 * v;
  }
  __syncthreads();
  const int n_el = nf * k_bins;
  for (int e = threadIdx.x; e < n_el; e += kEnvThreads) {
    const int fr = e / k_bins, k = e - fr * k_bins;
    const double c = ctab[k], tc = 2.0 * c;
    double u = 1.0, v = 1.0;
    for (int i = 0; i < p; i += 2) {
      u = u * (tc - sx[fr * kLsfMaxOrder + i]);
      v = v * (tc - sx[fr * kLsfMaxOrder + i + 1]);
    }
    const double a2 = 0.25 * ((2.0 * (1.0 + c)) * (u * u) + (2.0 * (1.0 - c)) * (v * v));
    out[(f0 + fr) * ldo + k] = se[fr] / a2;  // (64-bit: 2 049 024 frames x 513 bins x 8 B is beyond 2^31 bytes)
  }
}

int lsf_check_order(const char* where, int p) {
  if (p < 2 || p > kLsfMaxOrder || (p & 1)) return wh::fail_msg(where, "the order p must be even and in [2, 64]");
  return 0;
}

}  // namespace

extern "C" int wh_lpc_levinson(wh_ctx* ctx, void* stream, const double* r, int64_t n_frames, int64_t ldr, int p, double* a,
                               int64_t lda, double* e, double* refl, int64_t ldk) {
  if (!ctx) return wh::fail_msg("wh_lpc_levinson", "null argument");
  WH_ENTER(ctx);
  if (p < 1 || p > kLsfMaxOrder) return wh::fail_msg("wh_lpc_levinson", "the order p must be in [1, 64]");
  if (n_frames < 0) return wh::fail_msg("wh_lpc_levinson", "negative frame count");
  if (ldr < p + 1) return wh::fail_msg("wh_lpc_levinson", "ldr must be at least p + 1");
  if (lda < p + 1) return wh::fail_msg("wh_lpc_levinson", "lda must be at least p + 1");
  if (refl && ldk < p) return wh::fail_msg("wh_lpc_levinson", "ldk must be at least p");
  if (n_frames == 0) return 0;
  if (!r || !a || !e) return wh::fail_msg("wh_lpc_levinson", "null argument");
  const long long blocks = (n_frames + WH_WAVE - 1) / WH_WAVE;
  if (blocks > 0x7fffffffLL) return wh::fail_msg("wh_lpc_levinson", "too many frames for one call");
  const size_t lds = (size_t)2 * (p + 1) * WH_WAVE * sizeof(double);
  if (int rc = wh::allow_lds(lpc_levinson_kernel, lds)) return rc;
  hipStream_t st = (hipStream_t)stream;
  WH_LAUNCH(ctx, st, "lpc_levinson_kernel", lpc_levinson_kernel, dim3((unsigned)blocks), dim3(WH_WAVE), lds, r,
            n_frames, ldr, p, a, lda, e, refl, ldk, ctx->d_flags);
  return 0;
}

extern "C" int wh_lsf_from_lpc(wh_ctx* ctx, void* stream, const double* a, int64_t n_frames, int64_t lda, int p,
                               const double* h_grid, int n_grid, double* x, int64_t ldx, int32_t* level_out) {
  if (!ctx) return wh::fail_msg("wh_lsf_from_lpc", "null argument");
  WH_ENTER(ctx);
  if (int rc = lsf_check_order("wh_lsf_from_lpc", p)) return rc;
  if (n_frames < 0) return wh::fail_msg("wh_lsf_from_lpc", "negative frame count");
  if (lda < p + 1) return wh::fail_msg("wh_lsf_from_lpc", "lda must be at least p + 1");
  if (ldx < p) return wh::fail_msg("wh_lsf_from_lpc", "ldx must be at least p");
  if (n_grid != kLsfGridMax + 1) return wh::fail_msg("wh_lsf_from_lpc", "the grid table must hold 4097 abscissae");
  if (!h_grid) return wh::fail_msg("wh_lsf_from_lpc", "null argument");
  if (n_frames == 0) return 0;
  if (!a || !x) return wh::fail_msg("wh_lsf_from_lpc", "null argument");
  const int per_block = p <= 32 ? 2 * kLsfWaves : kLsfWaves;  // two frames per wave while a frame's roots fit half a wave
  const long long blocks = (n_frames + per_block - 1) / per_block;
  if (blocks > 0x7fffffffLL) return wh::fail_msg("wh_lsf_from_lpc", "too many frames for one call");
  hipStream_t st = (hipStream_t)stream;
  void* d_grid = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "lsf.grid", h_grid, (size_t)n_grid * sizeof(double), &d_grid)) return rc;
  WH_LAUNCH(ctx, st, "lsf_from_lpc_kernel", p <= 32 ? lsf_from_lpc_kernel<32> : lsf_from_lpc_kernel<64>,
            dim3((unsigned)blocks), dim3(kLsfWaves * WH_WAVE), 0, a, n_frames, lda, p,
            reinterpret_cast<const double*>(d_grid), x, ldx, level_out, ctx->d_flags);
  return 0;
}

extern "C" int wh_lsf_envelope(wh_ctx* ctx, void* stream, const double* rows, int64_t n_frames, int64_t ldr, int p,
                               const double* h_cos, int k_bins, double* out, int64_t ldo) {
  if (!ctx) return wh::fail_msg("wh_lsf_envelope", "null argument");
  WH_ENTER(ctx);
  if (int rc = lsf_check_order("wh_lsf_envelope", p)) return rc;
  if (n_frames < 0) return wh::fail_msg("wh_lsf_envelope", "negative frame count");
  if (k_bins < 2 || k_bins > 16385) return wh::fail_msg("wh_lsf_envelope", "k_bins out of range");
  if (ldr < p + 1) return wh::fail_msg("wh_lsf_envelope", "ldr must be at least p + 1");
  if (ldo < k_bins) return wh::fail_msg("wh_lsf_envelope", "ldo must be at least k_bins");
  if (!h_cos) return wh::fail_msg("wh_lsf_envelope", "null argument");
  if (n_frames == 0) return 0;
  if (!rows || !out) return wh::fail_msg("wh_lsf_envelope", "null argument");
  const long long blocks = (n_frames + kEnvFrames - 1) / kEnvFrames;
  if (blocks > 0x7fffffffLL) return wh::fail_msg("wh_lsf_envelope", "too many frames for one call");
  hipStream_t st = (hipStream_t)stream;
  void* d_cos = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "lsf.bins", h_cos, (size_t)k_bins * sizeof(double), &d_cos)) return rc;
  WH_LAUNCH(ctx, st, "lsf_envelope_kernel", lsf_envelope_kernel, dim3((unsigned)blocks), dim3(kEnvThreads), 0, rows,
            n_frames, ldr, p, reinterpret_cast<const double*>(d_cos), k_bins, out, ldo);
  return 0;
}
