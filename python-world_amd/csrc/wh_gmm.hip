// Joint-density Gaussian mixtures for voice conversion (Toda, Black and Tokuda 2007): the three frame-proportional
// computations of EM and of the conversion, each a dense FP64 product per row and component on the matrix cores
// (wh_mfma.h: operand layout, strip geometry, pipeline).  The per-component algebra — a d x d Cholesky factor, its
// inverse, the regression matrices — is tiny and is done on the host (world/gmm.py).  Contract: include/world_hip.h,
// DESIGN section 16; tests/_gmm_reference.py is the same contract in NumPy (the results agree within derived bounds, and
// bit for bit where every partial sum is exact).
//
// gmm_rows_kernel<MODE>: a workgroup of four waves takes 128 rows and ALL columns (up to 160: ten 16-column tiles, each
// wave 32 rows x 160 = 2 x 10 accumulator tiles), and loops over the components m.  Per component it is one run of the
// staged pipeline over 16-wide k strips of (x - mu_m) (the centring applied on the way in) and of the component's matrix,
// read as it lies in memory ([k][n] row-major); what lies beyond k or n enters as 0.0.
//   MODE 0 (E-step): the matrix is the upper triangular whitening W_m, so strip s needs the column tiles t >= s only (the
//     others are structural zeros and are neither fetched nor multiplied); ll[row][m] = logc[m] - 0.5 sum_j z_j^2, the sum
//     over a lane's tiles ascending and then over the 16 lanes of the row by a butterfly, goes to an LDS tile
//     [128][M + 1], and after the last component one thread per row reduces over m ascending (max, sum of exp, log).
//   MODE 1 (conversion): ONE accumulation over all components, m ascending — the A operand of component m is
//     g[row][m] (x - mu_x[m]) (MMSE), or (x - mu_x[m]) where best[row] == m and 0.0 elsewhere (a select, not a product),
//     and the accumulators are not reset between components; a last pass of k = 0 .. M-1 with A = g[row][k] (or the
//     indicator of best[row] == k) and B = mu_y adds sum_m g_m mu_y[m].  No per-component epilogue and no second set of
//     accumulators: with one (res += g * (mu_y + acc) per component) the kernel spilled 99 VGPRs.
// A row's result depends on no other row.  No index or trip count depends on a value.
//
// gmm_stats_kernel: s2 = sum_n gamma (x - mu)(x - mu)' is a product whose k runs over the ROWS.  With a column of ones
// appended to the centred row, e~ = [x - mu_m, 1], the one product e~' diag(gamma) e~ holds s2, s1 (its last column) and s0
// (its last entry).  Workgroup (m, split): the rows [split * 4096, ...) in strips of 16 through the same pipeline
// ([row][column], with gamma beside it); A = gamma * e~ (multiplied as the operand is read), B = e~.  Only the tile pairs
// ti <= tj are computed (at most 66), dealt to the workgroup's eight waves round-robin, and of a diagonal tile only i <= j is kept: the
// lower triangle is the MIRROR of the upper one, bit for bit.  Partials [split][m][d + 1][d + 1] go to the context's
// scratch; gmm_combine_kernel adds the splits in ascending order (one thread per entry) and writes both triangles.
// No atomics: the split is a function of n_rows alone, so the same input gives the same bits on every run.
#include <math.h>

#include "wh_device.h"
#include "wh_host.h"
#include "wh_mfma.h"

namespace {

constexpr int kGmmMaxD = 160;  // the joint vector of 39 static + 39 delta coefficients per speaker: 156, padded
constexpr int kGmmMaxM = 64;
constexpr int kGmmRowTile = 128;     // rows per workgroup of gmm_rows_kernel
constexpr int kGmmSplitRows = 4096;  // rows per partial sum of gmm_stats_kernel

constexpr int kGmmNT = kGmmMaxD / 16;             // column tiles of a row tile
constexpr int kGmmST = (kGmmMaxD + 1 + 15) / 16;  // column tiles of the stats strip: d + 1 columns
using GmmStrip = wh::mfma_strip<kGmmNT>;
constexpr int kGmmKS = GmmStrip::KS, kGmmAS = GmmStrip::AS, kGmmBS = GmmStrip::BS;
constexpr int kGmmES = wh::mfma_strip<kGmmST>::BS;  // the stats strip is a B strip: [row = k][column]
constexpr int kGmmStatsWaves = 8;                // waves of a statistics workgroup
constexpr int kGmmSlots = (kGmmST * (kGmmST + 1) / 2 + kGmmStatsWaves - 1) / kGmmStatsWaves;  // tile pairs per wave
constexpr int kGmmEPer = kGmmES / 32;           // strip columns a thread stages: column t % 32 + 32 i of row t / 32

template <int MODE>
__global__ __launch_bounds__(256) void gmm_rows_kernel(
    const double* __restrict__ x_, long long n_rows, long long ldx, long long len_x, int ka, int nb, int M,
    const double* __restrict__ mu_, const double* __restrict__ bm_, const double* __restrict__ logc_,
    const double* __restrict__ muy_, const int32_t* __restrict__ best_in_, const double* __restrict__ g_, long long ldg,
    long long len_g, double* __restrict__ o0_, long long ld0, long long len_0, double* __restrict__ o1_, long long ld1,
    long long len_1, double* __restrict__ rowll_, int32_t* __restrict__ best_out_) {
  // MODE 0: o0 = ll, o1 = gamma.  MODE 1: o0 = out.
  const wh::ckp<const double> x = wh::ck_make(x_, len_x, wh::WH_CK_IN);
  const wh::ckp<const double> mu = wh::ck_make(mu_, (long long)M * ka, wh::WH_CK_TABLE);
  const wh::ckp<const double> bm = wh::ck_make(bm_, (long long)M * ka * nb, wh::WH_CK_TABLE);
  const wh::ckp<const double> logc = wh::ck_make(logc_, logc_ ? M : 0, wh::WH_CK_TABLE);
  const wh::ckp<const double> muy = wh::ck_make(muy_, muy_ ? (long long)M * nb : 0, wh::WH_CK_TABLE);
  const wh::ckp<const int32_t> best_in = wh::ck_make(best_in_, best_in_ ? n_rows : 0, wh::WH_CK_IN);
  const wh::ckp<const double> g = wh::ck_make(g_, len_g, wh::WH_CK_IN);
  const wh::ckp<double> o0 = wh::ck_make(o0_, len_0, wh::WH_CK_OUT);
  const wh::ckp<double> o1 = wh::ck_make(o1_, len_1, wh::WH_CK_OUT);
  const wh::ckp<double> rowll = wh::ck_make(rowll_, rowll_ ? n_rows : 0, wh::WH_CK_OUT);
  const wh::ckp<int32_t> best_out = wh::ck_make(best_out_, best_out_ ? n_rows : 0, wh::WH_CK_OUT);

  extern __shared__ double gmm_lds[];
  double* const As = gmm_lds;                                // [2][kGmmRowTile * kGmmAS]
  double* const Bs = As + 2 * kGmmRowTile * kGmmAS;          // [2][kGmmKS * kGmmBS]
  double* const Ls = Bs + 2 * kGmmKS * kGmmBS;               // MODE 0: [kGmmRowTile][M + 1]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long f0 = (long long)blockIdx.x * kGmmRowTile;
  const int ntiles = (nb + 15) / 16;
  // staging roles: thread t fetches 8 consecutive k of A row t/2 and the columns t%16 + 16 i of matrix row t/16
  const int ar = threadIdx.x >> 1, ak = (threadIdx.x & 1) * 8;
  const int bk = threadIdx.x >> 4, bc = threadIdx.x & 15;
  const long long arow = f0 + ar;
  const bool a_ok = arow < n_rows;
  const bool by_best = MODE == 1 && best_in_ != nullptr;
  const int32_t abest = (by_best && a_ok) ? best_in[arow] : -1;  // the staged row's component

  wh::double4_t acc[2][kGmmNT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int t = 0; t < kGmmNT; ++t) acc[mt][t] = wh::double4_t{0.0, 0.0, 0.0, 0.0};

  const int passes = MODE == 0 ? M : M + 1;  // MODE 1: the last pass adds sum_m g_m mu_y[m]
  for (int m = 0; m < passes; ++m) {
    const bool tail = MODE == 1 && m == M;
    const int kdim = tail ? M : ka;
    const int steps = (kdim + kGmmKS - 1) / kGmmKS;
    if (MODE == 0) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int t = 0; t < kGmmNT; ++t) acc[mt][t] = wh::double4_t{0.0, 0.0, 0.0, 0.0};
    }
    double gm = 1.0;  // MODE 1, MMSE: the staged row's weight of this component
    if (MODE == 1 && !tail && !by_best) gm = a_ok ? g[arow * ldg + m] : 0.0;
    double areg[8], breg[kGmmNT];
    auto fetch = [&](int st) {
      const int kc = st * kGmmKS;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = kc + ak + i;
        double v = 0.0;
        if (a_ok && k < kdim) {
          if (tail) {
            v = by_best ? (abest == k ? 1.0 : 0.0) : g[arow * ldg + k];
          } else {
            v = x[arow * ldx + k] - mu[(long long)m * ka + k];
            if (MODE == 1) v = by_best ? (abest == m ? v : 0.0) : gm * v;
          }
        }
        areg[i] = v;
      }
      const int k = kc + bk;
#pragma unroll
      for (int i = 0; i < kGmmNT; ++i) {
        const int n = bc + 16 * i;
        double v = 0.0;
        if (i < ntiles && (MODE != 0 || i >= st) && k < kdim && n < nb)
          v = tail ? muy[(long long)k * nb + n] : bm[((long long)m * ka + k) * nb + n];
        breg[i] = v;
      }
    };
    auto stage = [&](int buf) {
      double* a = As + buf * (kGmmRowTile * kGmmAS);
      double* b = Bs + buf * (kGmmKS * kGmmBS);
#pragma unroll
      for (int i = 0; i < 8; ++i) a[ar * kGmmAS + ak + i] = areg[i];
#pragma unroll
      for (int i = 0; i < kGmmNT; ++i) b[bk * kGmmBS + bc + 16 * i] = breg[i];
    };
    // wh_mfma.h's pipeline, written out as it always was: this kernel's schedule (412 VGPRs) follows the text, and the
    // forms that did not compile to the same code measured 0.7 % slower on the E-step
    fetch(0);
    stage(0);
    __syncthreads();
    for (int st = 0; st < steps; ++st) {
      const int buf = st & 1;
      if (st + 1 < steps) fetch(st + 1);  // in flight under this step's MFMAs
      const double* as = As + buf * (kGmmRowTile * kGmmAS) + (32 * w + (lane & 15)) * kGmmAS + (lane >> 4);
      const double* bs = Bs + buf * (kGmmKS * kGmmBS) + (lane >> 4) * kGmmBS + (lane & 15);
#pragma unroll
      for (int kk = 0; kk < kGmmKS / 4; ++kk) {
        const double a0 = as[4 * kk], a1 = as[16 * kGmmAS + 4 * kk];
#pragma unroll
        for (int t = 0; t < kGmmNT; ++t) {
          if (t < ntiles && (MODE != 0 || t >= st)) {
            const double b = bs[4 * kk * kGmmBS + 16 * t];
            wh::mfma_pair(acc[0][t], acc[1][t], a0, a1, b);
          }
        }
      }
      if (st + 1 < steps) stage(buf ^ 1);  // the other buffer was last read a step ago, before the barrier below
      __syncthreads();
    }
    if (MODE == 0) {  // the component's epilogue: ll of the tile's rows
      const double lc = logc[m];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double s = 0.0;
#pragma unroll
          for (int t = 0; t < kGmmNT; ++t) {
            if (t < ntiles) {
              const double v = acc[mt][t][r];
              s = s + ((16 * t + (lane & 15)) < nb ? v * v : 0.0);
            }
          }
          s = s + __shfl_xor(s, 1);
          s = s + __shfl_xor(s, 2);
          s = s + __shfl_xor(s, 4);
          s = s + __shfl_xor(s, 8);
          if ((lane & 15) == 0) Ls[(32 * w + 16 * mt + 4 * r + (lane >> 4)) * (M + 1) + m] = lc - 0.5 * s;
        }
    }
  }

  if (MODE == 0) {
    __syncthreads();
    const long long f = f0 + threadIdx.x;
    if (threadIdx.x < kGmmRowTile && f < n_rows) {
      const double* l = Ls + threadIdx.x * (M + 1);
      double mx = l[0];
      int32_t bi = 0;
      for (int m = 1; m < M; ++m) {
        const double v = l[m];
        if (v > mx || (v != v && mx == mx)) {  // the first maximum; a NaN takes over and stays
          mx = v;
          bi = m;
        }
      }
      double s = 0.0;
      for (int m = 0; m < M; ++m) s = s + exp(l[m] - mx);
      if (o0_)
        for (int m = 0; m < M; ++m) o0[f * ld0 + m] = l[m];
      if (o1_)
        for (int m = 0; m < M; ++m) o1[f * ld1 + m] = exp(l[m] - mx) / s;
      if (rowll_) rowll[f] = mx + log(s);
      if (best_out_) best_out[f] = bi;
    }
  } else {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int t = 0; t < kGmmNT; ++t) {
        const int n = 16 * t + (lane & 15);
        if (t < ntiles && n < nb) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const long long f = f0 + 32 * w + 16 * mt + 4 * r + (lane >> 4);
            if (f < n_rows) o0[f * ld0 + n] = acc[mt][t][r];
          }
        }
      }
  }
}

__global__ __launch_bounds__(64 * kGmmStatsWaves) void gmm_stats_kernel(
    const double* __restrict__ x_, long long n_rows, long long ldx, long long len_x, int d, int M,
    const double* __restrict__ gamma_, long long ldg, long long len_g, const double* __restrict__ mu_,
    double* __restrict__ part_, long long len_p) {
  const wh::ckp<const double> x = wh::ck_make(x_, len_x, wh::WH_CK_IN);
  const wh::ckp<const double> gamma = wh::ck_make(gamma_, len_g, wh::WH_CK_IN);
  const wh::ckp<const double> mu = wh::ck_make(mu_, (long long)M * d, wh::WH_CK_TABLE);
  const wh::ckp<double> part = wh::ck_make(part_, len_p, wh::WH_CK_LDS_SCRATCH);
  __shared__ double Es[2][kGmmKS * kGmmES];
  __shared__ double Gs[2][kGmmKS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int m = blockIdx.x;
  const long long sp = blockIdx.y;
  const long long r0 = sp * kGmmSplitRows;
  const long long r1 = r0 + kGmmSplitRows < n_rows ? r0 + kGmmSplitRows : n_rows;
  const int d1 = d + 1, nt = (d1 + 15) / 16, npairs = nt * (nt + 1) / 2;
  // this wave's tile pairs: pair p = kGmmStatsWaves s + w of the list (0,0) (0,1) .. (0,nt-1) (1,1) ..
  int ti[kGmmSlots], tj[kGmmSlots];
  wh::double4_t acc[kGmmSlots];
#pragma unroll
  for (int s = 0; s < kGmmSlots; ++s) {
    int a = 0, rem = kGmmStatsWaves * s + w;
    const bool ok = rem < npairs;
    if (!ok) rem = 0;
    for (int i = 0; i < kGmmST; ++i)
      if (rem >= nt - a) {
        rem -= nt - a;
        ++a;
      }
    ti[s] = ok ? a : -1;
    tj[s] = a + rem;
    acc[s] = wh::double4_t{0.0, 0.0, 0.0, 0.0};
  }
  const int rk = threadIdx.x >> 5, rc = threadIdx.x & 31;
  double ereg[kGmmEPer], greg = 0.0;
  auto fetch = [&](long long row0) {
    const long long row = row0 + rk;
    const bool ok = row < r1;
#pragma unroll
    for (int i = 0; i < kGmmEPer; ++i) {
      const int c = rc + 32 * i;
      double v = 0.0;
      if (c < 16 * nt && ok) {
        if (c < d) v = x[row * ldx + c] - mu[(long long)m * d + c];
        else if (c == d) v = 1.0;
      }
      ereg[i] = v;
    }
    greg = (ok && rc == 0) ? gamma[row * ldg + m] : 0.0;
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kGmmEPer; ++i) Es[buf][rk * kGmmES + rc + 32 * i] = ereg[i];
    if (rc == 0) Gs[buf][rk] = greg;
  };
  const long long steps = (r1 - r0 + kGmmKS - 1) / kGmmKS;
  wh::mfma_pipeline(steps, [&](long long st) { fetch(r0 + st * kGmmKS); }, stage, [&](long long, int buf) {
#pragma unroll
    for (int kk = 0; kk < kGmmKS / 4; ++kk) {
      const int kr = 4 * kk + (lane >> 4);
      const double* e = &Es[buf][kr * kGmmES + (lane & 15)];
      const double gk = Gs[buf][kr];
#pragma unroll
      for (int s = 0; s < kGmmSlots; ++s) {
        if (ti[s] >= 0) wh::mfma_acc(acc[s], gk * e[16 * ti[s]], e[16 * tj[s]]);
      }
    }
  });
  const long long base = (sp * M + m) * (long long)d1 * d1;
#pragma unroll
  for (int s = 0; s < kGmmSlots; ++s) {
    if (ti[s] >= 0) {
      const int j = 16 * tj[s] + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * ti[s] + 4 * r + (lane >> 4);
        if (i <= j && j < d1) part[base + (long long)i * d1 + j] = acc[s][r];
      }
    }
  }
}

__global__ __launch_bounds__(WH_BLOCK) void gmm_combine_kernel(const double* __restrict__ part_, long long len_p,
                                                               long long splits, int d, int M, double* __restrict__ s0_,
                                                               double* __restrict__ s1_, double* __restrict__ s2_) {
  const wh::ckp<const double> part = wh::ck_make(part_, len_p, wh::WH_CK_LDS_SCRATCH);
  const wh::ckp<double> s0 = wh::ck_make(s0_, M, wh::WH_CK_OUT);
  const wh::ckp<double> s1 = wh::ck_make(s1_, (long long)M * d, wh::WH_CK_OUT);
  const wh::ckp<double> s2 = wh::ck_make(s2_, (long long)M * d * d, wh::WH_CK_OUT);
  const int d1 = d + 1;
  const long long per = (long long)d1 * d1;
  const long long e = (long long)blockIdx.x * WH_BLOCK + threadIdx.x;
  if (e >= (long long)M * per) return;
  const int m = (int)(e / per);
  const int i = (int)((e - m * per) / d1), j = (int)(e - m * per - (long long)i * d1);
  if (i > j) return;
  double v = 0.0;
  for (long long sp = 0; sp < splits; ++sp) v = v + part[(sp * M + m) * per + (long long)i * d1 + j];
  if (j < d) {
    s2[((long long)m * d + i) * d + j] = v;
    s2[((long long)m * d + j) * d + i] = v;
  } else if (i < d) {
    s1[(long long)m * d + i] = v;
  } else {
    s0[m] = v;
  }
}

long long gmm_splits(long long n_rows) { return (n_rows + kGmmSplitRows - 1) / kGmmSplitRows; }

size_t gmm_rows_lds(int mode, int M) {
  size_t n = 2 * (size_t)kGmmRowTile * kGmmAS + 2 * (size_t)kGmmKS * kGmmBS;
  if (mode == 0) n += (size_t)kGmmRowTile * (M + 1);
  return n * sizeof(double);
}

int gmm_check_rows(const char* where, int64_t n_rows, int64_t ldx, int d) {
  if (n_rows < 0) return wh::fail_msg(where, "n_rows must be >= 0");
  if (ldx < d) return wh::fail_msg(where, "ldx must be at least the row width");
  if ((n_rows + kGmmRowTile - 1) / kGmmRowTile > 0x7fffffffLL) return wh::fail_msg(where, "too many rows for one call");
  return 0;
}

}  // namespace

extern "C" int64_t wh_gmm_workspace_bytes(int64_t n_rows, int d, int M) {
  if (n_rows < 0 || d < 1 || d > kGmmMaxD || M < 1 || M > kGmmMaxM) return -1;
  return (int64_t)(gmm_splits(n_rows) * M * (long long)(d + 1) * (d + 1) * (long long)sizeof(double));
}

extern "C" int wh_gmm_estep(wh_ctx* ctx, void* stream, const double* x, int64_t n_rows, int64_t ldx, int d, int M,
                            const double* mu, const double* whiten, const double* logc, double* ll, int64_t ldl,
                            double* gamma, int64_t ldg, double* rowll, int32_t* best) {
  if (!ctx) return wh::fail_msg("wh_gmm_estep", "null argument");
  WH_ENTER(ctx);
  if (d < 1 || d > kGmmMaxD) return wh::fail_msg("wh_gmm_estep", "d must be in [1, 160]");
  if (M < 1 || M > kGmmMaxM) return wh::fail_msg("wh_gmm_estep", "M must be in [1, 64]");
  if (int rc = gmm_check_rows("wh_gmm_estep", n_rows, ldx, d)) return rc;
  if ((ll && ldl < M) || (gamma && ldg < M)) return wh::fail_msg("wh_gmm_estep", "ldl and ldg must be at least M");
  if (n_rows == 0) return 0;
  if (!x || !mu || !whiten || !logc) return wh::fail_msg("wh_gmm_estep", "null argument");
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = gmm_rows_lds(0, M);
  if (int rc = wh::allow_lds(gmm_rows_kernel<0>, lds)) return rc;
  const long long blocks = (n_rows + kGmmRowTile - 1) / kGmmRowTile;
  WH_LAUNCH(ctx, st, "gmm_estep_kernel", gmm_rows_kernel<0>, dim3((unsigned)blocks), dim3(256), lds, x, n_rows, ldx,
            (n_rows - 1) * ldx + d, d, d, M, mu, whiten, logc, nullptr, nullptr, nullptr, 0LL, 0LL, ll, ldl,
            ll ? (n_rows - 1) * ldl + M : 0LL, gamma, ldg, gamma ? (n_rows - 1) * ldg + M : 0LL, rowll, best);
  return 0;
}

extern "C" int wh_gmm_stats(wh_ctx* ctx, void* stream, const double* x, int64_t n_rows, int64_t ldx, int d, int M,
                            const double* gamma, int64_t ldg, const double* mu, double* s0, double* s1, double* s2) {
  if (!ctx) return wh::fail_msg("wh_gmm_stats", "null argument");
  WH_ENTER(ctx);
  if (d < 1 || d > kGmmMaxD) return wh::fail_msg("wh_gmm_stats", "d must be in [1, 160]");
  if (M < 1 || M > kGmmMaxM) return wh::fail_msg("wh_gmm_stats", "M must be in [1, 64]");
  if (int rc = gmm_check_rows("wh_gmm_stats", n_rows, ldx, d)) return rc;
  if (ldg < M) return wh::fail_msg("wh_gmm_stats", "ldg must be at least M");
  if (n_rows == 0) return 0;
  if (!x || !gamma || !mu || !s0 || !s1 || !s2) return wh::fail_msg("wh_gmm_stats", "null argument");
  hipStream_t st = (hipStream_t)stream;
  const long long splits = gmm_splits(n_rows);
  if (splits > 65535) return wh::fail_msg("wh_gmm_stats", "too many rows for one call");
  const long long per = (long long)(d + 1) * (d + 1), len_p = splits * M * per;
  double* part = nullptr;
  if (int rc = wh::persistent_scratch(ctx, "gmm.partials", (size_t)len_p, &part)) return rc;
  WH_LAUNCH(ctx, st, "gmm_stats_kernel", gmm_stats_kernel, dim3((unsigned)M, (unsigned)splits),
            dim3(64 * kGmmStatsWaves), 0, x, n_rows, ldx, (n_rows - 1) * ldx + d, d, M, gamma, ldg,
            (n_rows - 1) * ldg + M, mu, part, len_p);
  const long long total = (long long)M * per;
  WH_LAUNCH(ctx, st, "gmm_combine_kernel", gmm_combine_kernel, dim3((unsigned)((total + WH_BLOCK - 1) / WH_BLOCK)),
            dim3(WH_BLOCK), 0, part, len_p, splits, d, M, s0, s1, s2);
  return 0;
}

extern "C" int wh_gmm_convert(wh_ctx* ctx, void* stream, const double* x, int64_t n_rows, int64_t ldx, int dx, int dy, int M,
                              const double* mu_x, const double* a, const double* mu_y, const int32_t* best, const double* g,
                              int64_t ldg, double* out, int64_t ldo) {
  if (!ctx) return wh::fail_msg("wh_gmm_convert", "null argument");
  WH_ENTER(ctx);
  if (dx < 1 || dy < 1 || (long long)dx + dy > kGmmMaxD)
    return wh::fail_msg("wh_gmm_convert", "dx and dy must be >= 1 and dx + dy at most 160");
  if (M < 1 || M > kGmmMaxM) return wh::fail_msg("wh_gmm_convert", "M must be in [1, 64]");
  if (int rc = gmm_check_rows("wh_gmm_convert", n_rows, ldx, dx)) return rc;
  if ((best != nullptr) == (g != nullptr)) return wh::fail_msg("wh_gmm_convert", "exactly one of best and g must be given");
  if (g && ldg < M) return wh::fail_msg("wh_gmm_convert", "ldg must be at least M");
  if (ldo < dy) return wh::fail_msg("wh_gmm_convert", "ldo must be at least dy");
  if (n_rows == 0) return 0;
  if (!x || !mu_x || !a || !mu_y || !out) return wh::fail_msg("wh_gmm_convert", "null argument");
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = gmm_rows_lds(1, M);
  if (int rc = wh::allow_lds(gmm_rows_kernel<1>, lds)) return rc;
  const long long blocks = (n_rows + kGmmRowTile - 1) / kGmmRowTile;
  WH_LAUNCH(ctx, st, "gmm_convert_kernel", gmm_rows_kernel<1>, dim3((unsigned)blocks), dim3(256), lds, x, n_rows, ldx,
            (n_rows - 1) * ldx + dx, dx, dy, M, mu_x, a, nullptr, mu_y, best, g, ldg, g ? (n_rows - 1) * ldg + M : 0LL,
            out, ldo, (n_rows - 1) * ldo + dy, nullptr, 0LL, 0LL, nullptr, nullptr);
  return 0;
}
