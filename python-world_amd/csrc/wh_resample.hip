// Polyphase resampling: scipy.signal.resample_poly(x, up, down) with its defaults (window=('kaiser', 5.0),
// padtype='constant', cval=None) over a ragged batch, bit for bit — the step the reference's callers run in front of
// the analysis (example/prosody.py:16-19).  The host designs the padded FIR (firwin, the pre/post zero pads of
// resample_poly); this file turns it into scipy's phase table h_trans_flip[up][P] and evaluates upfirdn's loop:
//
//   output j of upfirdn:  t = (j*down) % up,  xi = (j*down) / up,  acc = 0.0;
//                         for k = xi-P+1 .. xi, k in [0, n_in):  acc = acc + x[k] * h_trans_flip[t][k - (xi-P+1)]
//
// with each product rounded on its own (the TU stays at the build's -ffp-contract=off) and resample_poly keeping
// j = i + n_pre_remove, i < n_out.  Taps of k outside the signal are skipped, not multiplied by zero, so a non-finite
// tap or sample gives what scipy gives.
//
// Layout.  A tile is up*G*R consecutive outputs of one utterance, its first output a multiple of `up`: output
// i0 + o + up*(g + G*r) has phase t(o) = ((o + n_pre_remove) * down) % up whatever the tile, so a thread that owns the
// phase slot o (and group g) reads ONE filter row for all its outputs.  The tile's input span (tile * down / up + P
// samples) is staged into LDS with coalesced loads; the row is held in registers (P <= 64, the rates of the 16 kHz
// analysis: a variant per 24 / 32 / 48 / 64 taps, the row behind zero taps) or read through L1 (longer filters).  Per
// tap a lane then issues one LDS read, one multiply and one add, with no branch between the taps.
#include <math.h>
#include <string.h>

#include <numeric>
#include <string>
#include <vector>

#include "wh_device.h"
#include "wh_host.h"

namespace {

constexpr int kRsThreads = 256;
constexpr int kRsLds = 6144;  // staged input samples per tile (48 KiB: three workgroups per CU)
constexpr int kRsMaxRate = 4096;

struct RsUtt {
  long long in_off, n_in, out_off, n_out, pre_remove, tab_off;
  int up, down, P, nph, G, R, xg, pad;  // xg: the span does not fit LDS, samples are read from global memory
};
struct RsTile {
  long long i0;
  int u, pad;
};

__device__ __forceinline__ long long rs_xi(long long i, const RsUtt& U) {
  return ((i + U.pre_remove) * (long long)U.down) / U.up;
}

// One output the general way: guarded tap range, samples from LDS (span origin k_first) or global memory, taps through L1.
// The table of an utterance is tap-major, element (phase t, tap m) at m * up + t: the lanes of a wave hold different
// phases of one tap, and their loads share cache lines.
template <bool LDS>
__device__ __forceinline__ double rs_one(long long k0, const RsUtt& U, wh::ckp<const double> xin, wh::ckp<const double> xs,
                                         long long k_first, wh::ckp<const double> htab, int t) {
  const long long m_lo = k0 < 0 ? -k0 : 0;
  const long long m_hi = (U.n_in - k0) < U.P ? (U.n_in - k0) : U.P;
  double acc = 0.0;
  for (long long m = m_lo; m < m_hi; ++m) {
    const double xv = LDS ? xs[k0 + m - k_first] : xin[k0 + m];
    acc = acc + xv * htab[m * U.up + t];
  }
  return acc;
}

// The LDS span allows three workgroups per CU, so three waves per SIMD is all the register budget has to allow: the
// 64-tap row (128 VGPRs) with two chains, the shorter rows with four.
template <int PMAX>
__global__ __launch_bounds__(kRsThreads, 3) void resample_kernel(const double* __restrict__ x_raw, long long x_n,
                                                              double* __restrict__ y_raw, long long y_n,
                                                              const RsUtt* __restrict__ utts, int n_utt,
                                                              const RsTile* __restrict__ tiles, long long n_tiles,
                                                              const double* __restrict__ tab_raw, long long tab_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const long long unit = wh::xcd_unit(blockIdx.x, n_tiles);
  if (unit >= n_tiles) return;
  const wh::ckp<const double> x = wh::ck_make(x_raw, x_n, wh::WH_CK_WAVEFORM);
  const wh::ckp<double> y = wh::ck_make(y_raw, y_n, wh::WH_CK_OUT);
  const wh::ckp<const double> tab = wh::ck_make(tab_raw, tab_n, wh::WH_CK_TABLE);
  const wh::ckp<const RsTile> tl = wh::ck_make(tiles, n_tiles, wh::WH_CK_IN);
  const RsTile T = tl[unit];
  const wh::ckp<const RsUtt> ut = wh::ck_make(utts, (long long)n_utt, wh::WH_CK_IN);
  const RsUtt U = ut[T.u];
  const wh::ckp<double> xs = wh::ck_make(reinterpret_cast<double*>(smem), (long long)kRsLds, wh::WH_CK_LDS_MAIN);
  const wh::ckp<const double> xin = wh::ck_sub(x, U.in_off, U.n_in, wh::WH_CK_WAVEFORM);
  const wh::ckp<double> yout = wh::ck_sub(y, U.out_off, U.n_out, wh::WH_CK_OUT);

  const long long tile_out = (long long)U.up * U.G * U.R;
  const long long i0 = T.i0;
  const long long i1 = i0 + tile_out < U.n_out ? i0 + tile_out : U.n_out;
  // the fast path runs PMAX taps per output: the row behind pad = PMAX - P zero taps, i.e. pad more (older) samples in front
  // of each window.  With acc starting at +0.0, a finite sample times a zero tap adds +-0 and leaves acc +0.0, so that is
  // the same sum bit for bit — as long as those samples are finite: a span holding a non-finite sample takes the exact path.
  const int pad = PMAX > U.P ? PMAX - U.P : 0;
  const long long k_first = rs_xi(i0, U) - U.P + 1 - pad;
  int nonfinite = 0;
  if (!U.xg) {  // stage the span [k_first, xi(i1-1)]: zeros outside the signal (never read: the taps there are skipped)
    const long long span = rs_xi(i1 - 1, U) - k_first + 1;
    for (long long s0 = threadIdx.x; s0 < span; s0 += 4 * kRsThreads) {
      double v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const long long k = k_first + s0 + c * kRsThreads;
        v[c] = (s0 + c * kRsThreads < span && k >= 0 && k < U.n_in) ? xin[k] : 0.0;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (s0 + c * kRsThreads < span) xs[s0 + c * kRsThreads] = v[c];
        nonfinite |= !isfinite(v[c]);
      }
    }
    nonfinite = __syncthreads_or(nonfinite);
  }
  constexpr int CH = 2;  // outputs per thread and pass (independent accumulation chains)
  const int q = threadIdx.x;
  if (q >= U.nph * U.G) return;
  const int slot = q % U.nph, g = q / U.nph;
  const long long pr = U.pre_remove % U.up;
  for (int o = slot; o < U.up; o += U.nph) {
    const int t = (int)(((o + pr) * (long long)U.down) % U.up);
    const wh::ckp<const double> htab = wh::ck_sub(tab, U.tab_off, (long long)U.up * U.P, wh::WH_CK_TABLE);
    double hr[PMAX > 0 ? PMAX : 1];
    if constexpr (PMAX > 0) {
#pragma unroll
      for (int m = 0; m < PMAX; ++m) hr[m] = m < pad ? 0.0 : htab[(long long)(m - pad) * U.up + t];
    }
    for (int r0 = 0; r0 < U.R; r0 += CH) {
      long long i[CH], kk[CH];  // kk: the first tap's sample k0 = xi - P + 1, relative to k_first
      bool valid[CH];
      bool fast = !U.xg && (PMAX == 0 || !nonfinite);
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        i[c] = i0 + o + (long long)U.up * (g + (long long)U.G * (r0 + c));
        valid[c] = r0 + c < U.R && i[c] < i1;
        const long long k0 = rs_xi(valid[c] ? i[c] : i0, U) - U.P + 1;  // (a lane without output c uses a window of the tile)
        const bool inside = k0 - pad >= 0 && k0 + U.P <= U.n_in;
        fast = fast && (!valid[c] || inside);
        kk[c] = (valid[c] || inside) ? k0 - k_first : -1;
      }
      if (!valid[0]) continue;  // (outputs are in ascending r: none left for this phase)
#pragma unroll
      for (int c = 1; c < CH; ++c)
        if (kk[c] < 0) kk[c] = kk[0];
      if (fast) {  // interior outputs: CH independent chains over the staged span, no branch between the taps
        double a[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) a[c] = 0.0;
        if constexpr (PMAX > 0) {  // the row from registers
          int b[CH];
#pragma unroll
          for (int c = 0; c < CH; ++c) b[c] = (int)kk[c] - pad;
#pragma unroll
          for (int m = 0; m < PMAX; ++m) {
            const double h = hr[m];
#pragma unroll
            for (int c = 0; c < CH; ++c) a[c] = a[c] + xs[b[c] + m] * h;
          }
        } else {  // the row through L1
          for (int m = 0; m < U.P; ++m) {
            const double h = htab[(long long)m * U.up + t];
#pragma unroll
            for (int c = 0; c < CH; ++c) a[c] = a[c] + xs[kk[c] + m] * h;
          }
        }
#pragma unroll
        for (int c = 0; c < CH; ++c)
          if (valid[c]) yout[i[c]] = a[c];
      } else {  // the edges of an utterance, or a span beyond LDS / holding a non-finite sample
        for (int c = 0; c < CH; ++c) {
          if (!valid[c]) continue;
          const long long k0 = rs_xi(i[c], U) - U.P + 1;
          yout[i[c]] = U.xg ? rs_one<false>(k0, U, xin, xs, k_first, htab, t) : rs_one<true>(k0, U, xin, xs, k_first, htab, t);
        }
      }
    }
  }
}

// content key of the filters: one multiply-xorshift step per 64-bit word
uint64_t mix64(uint64_t h, uint64_t w) {
  h = (h ^ w) * 0x9e3779b97f4a7c15ull;
  return h ^ (h >> 29);
}

// Phase slots per tile and groups of them.  Up to 256 phases a thread owns one (its row is loaded once per tile; 160
// phases: 160 slots, two and a half waves busy); beyond, the split of the 256 threads over `up` phases that leaves the
// fewest idle (a thread owns ceil(up / nph) phases).
void rs_split(int up, int* nph, int* G) {
  if (up <= kRsThreads) {
    *nph = up;
    *G = kRsThreads / up;
    return;
  }
  double best = -1.0;
  for (int k = 1; k <= 16; ++k) {
    const int n = (up + k - 1) / k;
    if (n > kRsThreads) continue;
    const int g = kRsThreads / n;
    const double util = (double)up * g / ((double)kRsThreads * k);
    if (util > best + 1e-9) {
      best = util;
      *nph = n;
      *G = g;
    }
    if (n == 1) break;
  }
}

}  // namespace

extern "C" int wh_resample_poly(wh_ctx* ctx, void* stream, int n_utt, const int64_t* h_in_off, const int64_t* h_out_off,
                                const int32_t* h_up, const int32_t* h_down, const int64_t* h_filt_off,
                                const int64_t* h_filt_len, const int64_t* h_pre_remove, const double* h_filters,
                                int64_t n_filters, const double* x, double* y) {
  const char* W = "wh_resample_poly";
  if (!ctx || !h_in_off || !h_out_off || !h_up || !h_down || !h_filt_off || !h_filt_len || !h_pre_remove || !h_filters)
    return wh::fail_msg(W, "null argument");
  WH_ENTER(ctx);
  if (n_utt < 0 || n_filters < 0) return wh::fail_msg(W, "negative count");
  if (n_utt == 0) return 0;
  if (h_in_off[0] < 0 || h_out_off[0] < 0) return wh::fail_msg(W, "negative offset");
  for (int u = 0; u < n_utt; ++u)
    if (h_in_off[u + 1] < h_in_off[u] || h_out_off[u + 1] < h_out_off[u])
      return wh::fail_msg(W, "offset tables must be monotone");
  const long long x_n = h_in_off[n_utt], y_n = h_out_off[n_utt];
  if (y_n > 0 && (!x || !y)) return wh::fail_msg(W, "null device pointer");
  hipStream_t st = (hipStream_t)stream;
  // the phase tables of the distinct filters of this call, one device table keyed by their content
  std::vector<RsUtt> utt(n_utt);
  struct Seen {
    long long fo, L, up, P, off;
  };
  std::vector<Seen> seen;  // the distinct (filter, up) of the call and their offsets in the table
  long long tab_n = 0;
  uint64_t key = 1469598103934665603ull;
  for (int u = 0; u < n_utt; ++u) {
    const long long n_in = h_in_off[u + 1] - h_in_off[u], n_out = h_out_off[u + 1] - h_out_off[u];
    const int up = h_up[u], down = h_down[u];
    if (up < 1 || down < 1) return wh::fail_msg(W, "rates must be positive integers");
    if (up > kRsMaxRate || down > kRsMaxRate)
      return wh::fail_msg(W, "reduced up / down beyond 4096 (the filter would span more than 81921 taps)");
    const long long L = h_filt_len[u], fo = h_filt_off[u], npr = h_pre_remove[u];
    if (L < 1 || fo < 0 || fo + L > n_filters) return wh::fail_msg(W, "filter outside h_filters");
    if (npr < 0) return wh::fail_msg(W, "negative n_pre_remove");
    if (n_out != (n_in * up + down - 1) / down) return wh::fail_msg(W, "output length is not ceil(n_in * up / down)");
    const long long P = (L + up - 1) / up;
    if (P > (1 << 30)) return wh::fail_msg(W, "filter too long");
    RsUtt& U = utt[u];
    U.in_off = h_in_off[u];
    U.n_in = n_in;
    U.out_off = h_out_off[u];
    U.n_out = n_out;
    U.pre_remove = npr;
    U.up = up;
    U.down = down;
    U.P = (int)P;
    U.pad = 0;
    long long off = -1;
    for (auto& e : seen)
      if (e.fo == fo && e.L == L && e.up == up) off = e.off;
    if (off < 0) {
      off = tab_n;
      seen.push_back({fo, L, (long long)up, P, off});
      tab_n += P * up;
      key = mix64(key, (uint64_t)up);
      key = mix64(key, (uint64_t)L);
      for (long long k = 0; k < L; ++k) {
        uint64_t w;
        memcpy(&w, h_filters + fo + k, sizeof w);
        key = mix64(key, w);
      }
    }
    U.tab_off = off;
    rs_split(up, &U.nph, &U.G);
  }
  if (y_n == 0) return 0;
  if (int rc = wh::tables_make_room(ctx)) return rc;
  // the tables are built only when the cache does not hold them already
  const std::string tab_key = "resample:" + std::to_string(tab_n) + ":" + std::to_string(key);
  const double* d_tab = nullptr;
  auto hit = ctx->tables.find(tab_key);
  if (hit != ctx->tables.end()) {
    d_tab = hit->second;
  } else {
    std::vector<double> tab((size_t)tab_n, 0.0);
    for (const Seen& e : seen)
      // h_trans_flip (h padded to P*up, reshaped (P, up), transposed, each row reversed), stored tap-major: [m][t]
      for (long long t = 0; t < e.up; ++t)
        for (long long m = 0; m < e.P; ++m) {
          const long long src = (e.P - 1 - m) * e.up + t;
          tab[(size_t)(e.off + m * e.up + t)] = src < e.L ? h_filters[e.fo + src] : 0.0;
        }
    if (int rc = wh::const_table(ctx, tab_key, tab, &d_tab)) return rc;
  }
  // tiles, one list per kernel variant: rows in registers (P <= 24 / 32 / 48 / 64 taps) or through L1
  constexpr int kVariants = 5;
  static const int pmax[kVariants] = {24, 32, 48, 64, 0};
  std::vector<RsTile> tl[kVariants];
  for (int u = 0; u < n_utt; ++u) {
    RsUtt& U = utt[u];
    if (U.n_out == 0) {
      U.R = 1;
      U.xg = 0;
      continue;
    }
    const long long per = (long long)U.up * U.G;  // outputs per r
    const long long need = (U.n_out + per - 1) / per;
    long long R = 16;
    const long long taps = U.P > 64 ? U.P : 64;  // (the register variants stage up to 64 - P samples more per span)
    while (R > 1 && (R > need || ((per * R - 1) * U.down) / U.up + 1 + taps + 1 > kRsLds)) --R;
    U.R = (int)R;
    U.xg = ((per * R - 1) * U.down) / U.up + 1 + taps + 1 > kRsLds ? 1 : 0;
    int v = kVariants - 1;
    if (!U.xg)
      for (int k = kVariants - 2; k >= 0; --k)
        if (U.P <= pmax[k]) v = k;
    for (long long i0 = 0; i0 < U.n_out; i0 += per * R) tl[v].push_back({i0, u, 0});
  }
  RsUtt* d_utt = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "resample.utt", utt, &d_utt)) return rc;
  static const char* slots[kVariants] = {"resample.tiles24", "resample.tiles32", "resample.tiles48", "resample.tiles64",
                                         "resample.tilesL1"};
  static const char* names[kVariants] = {"resample_kernel<24>", "resample_kernel<32>", "resample_kernel<48>",
                                         "resample_kernel<64>", "resample_kernel<0>"};
  static decltype(&resample_kernel<0>) const kernels[kVariants] = {resample_kernel<24>, resample_kernel<32>,
                                                                   resample_kernel<48>, resample_kernel<64>,
                                                                   resample_kernel<0>};
  const size_t lds = sizeof(double) * kRsLds;
  for (int v = 0; v < kVariants; ++v) {
    if (tl[v].empty()) continue;
    RsTile* d_tiles = nullptr;
    if (int rc = wh::persistent_upload(ctx, st, slots[v], tl[v], &d_tiles)) return rc;
    const long long n = (long long)tl[v].size();
    WH_LAUNCH(ctx, st, names[v], kernels[v], dim3((unsigned)wh::xcd_grid(n)), dim3(kRsThreads), lds, x, x_n, y, y_n,
              d_utt, n_utt, d_tiles, n, d_tab, tab_n);
  }
  return 0;
}
