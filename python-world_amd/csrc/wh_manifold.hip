// The manifold vocoder's networks on the device: a stack of Dense layers run over many rows in one launch.  Replaces
// the Keras `encoder.predict` / `decoder.predict` of World.encode_vae (world/main.py:367-384) together with the glue
// around them: the `Xc -= mean` shift and get_context on the way in, the kept column window and `Yc += mean` on the way
// out.  The reference's networks are 39 -> 256 -> 256 -> 256 -> 12 (encoder) and 12 -> 256 -> 256 -> 256 -> 39
// (decoder), ReLU on the hidden layers, linear at the latent and the output.
//
// dense_stack_kernel: a workgroup of four waves owns a tile of 32 rows for the whole stack.  The tile's activations live in
// one LDS buffer (32 rows x 273 doubles, 68 KiB: the row stride is 17 mod 32 doubles so that the 16 rows x 4 k of an A
// operand fall on distinct bank pairs); each layer reads it as its A operand, waits at a barrier, and writes its output
// back over it.  Single buffering costs one barrier per layer and lets two workgroups share a CU's 160 KiB (eight waves,
// two per SIMD).  Wave w computes the output column tiles 4w .. 4w+3 of every layer — 2 x 4 accumulator tiles, 64 VGPRs
// (wh_mfma.h: the tile type, the MFMA pair, the operand layout) — with its weight k-strips loaded from L2 straight into
// registers one 16-k step ahead of the MFMAs (each wave reads only its own columns, so the weights never pass through
// LDS; that is why this kernel does not run wh_mfma.h's LDS-staged pipeline).  Layer 0 stages its input
// into the same tile, up to 256 columns at a time (the input may be up to 2048 wide), with the context gather and the
// input shift applied on the load.  The tap layer's and the last layer's outputs leave through the tile as contiguous
// row stores; keeping per-row global addresses in registers instead made the kernel spill.
//
// Tile height: the padded weights of the TIMIT pair are 2.36 MB (FP64), read from L2 once per tile: at 32 rows that is
// 74 KB per frame against 576.5 kFLOP, 7.8 FLOP/B, while an MI355X CU issues 128 FP64 matrix FLOP/clk against 64 B/clk
// of L1 fill — so 32 rows keep the weight stream at a quarter of what the matrix pipe could consume.  64 rows would halve
// that but take 136 KiB of LDS per workgroup (one per CU, one wave per SIMD) and double the accumulators.
//
// Every output element is one MFMA accumulation chain over k in ascending 4-steps, identical for every row of the tile:
// a row's result does not depend on which other rows share its launch or tile.
#include <math.h>

#include <string>
#include <vector>

#include "wh_device.h"
#include "wh_host.h"
#include "wh_mfma.h"

namespace {

constexpr int kDsRows = 32;      // rows per workgroup tile
constexpr int kDsMaxW = 256;     // widest layer (units) the LDS tile holds
constexpr int kDsMaxL = 16;      // layers per stack
constexpr int kDsMaxIn = 2048;   // widest input row (after context stacking)
constexpr int kDsS = kDsMaxW + 17;  // LDS row stride in doubles (273 = 17 mod 32)
constexpr int kDsKS = 16;        // k per pipeline step: 4 MFMA k-slices
constexpr int kDsNT = 4;         // 16-column tiles per wave

enum { kActLinear = 0, kActRelu = 1, kActTanh = 2, kActSigmoid = 3 };

struct DsLayer {
  long long w_off;  // offset of the layer's [kpad][npad] k-major weights in the weight buffer
  int b_off;        // offset of its npad biases
  int kpad;         // input width padded to a multiple of 16
  int npad;         // output width padded to a multiple of 16
  int units;        // real output width
  int act;
};

__device__ __forceinline__ double ds_act(double v, int act) {
  switch (act) {
    case kActRelu: return v > 0.0 ? v : 0.0;
    case kActTanh: return tanh(v);
    case kActSigmoid: return 1.0 / (1.0 + exp(-v));
    default: return v;
  }
}

__global__ __launch_bounds__(256, 2) void dense_stack_kernel(
    const double* __restrict__ x_raw, long long x_n, long long n_rows, int d, long long ldx, int d_in,
    const long long* __restrict__ seg_raw, int n_seg, int window, const double* __restrict__ ishift_raw,
    const DsLayer* __restrict__ plan_raw, int n_layers, int tap_layer, int tap_f32,
    const double* __restrict__ w_raw, long long w_n, const double* __restrict__ b_raw, long long b_n,
    double* __restrict__ tap_raw, long long tap_n, long long ld_tap, const double* __restrict__ oshift_raw,
    double* __restrict__ out_raw, long long out_n, long long ldo) {
  __shared__ double act_lds[kDsRows * kDsS];
  const long long n_tiles = (n_rows + kDsRows - 1) / kDsRows;
  const long long unit = wh::xcd_unit(blockIdx.x, n_tiles);
  if (unit >= n_tiles) return;
  const wh::ckp<const double> x = wh::ck_make(x_raw, x_n, wh::WH_CK_IN);
  const wh::ckp<const long long> seg = wh::ck_make(seg_raw, (long long)n_seg + 1, wh::WH_CK_IN);
  const wh::ckp<const double> ishift = wh::ck_make(ishift_raw, (long long)d, wh::WH_CK_TABLE);
  const wh::ckp<const double> wt = wh::ck_make(w_raw, w_n, wh::WH_CK_TABLE);
  const wh::ckp<const double> bias = wh::ck_make(b_raw, b_n, wh::WH_CK_TABLE);
  const wh::ckp<double> tap = wh::ck_make(tap_raw, tap_n, wh::WH_CK_OUT);
  const wh::ckp<double> out = wh::ck_make(out_raw, out_n, wh::WH_CK_OUT);
  const wh::ckp<double> A = wh::ck_make(act_lds, (long long)kDsRows * kDsS, wh::WH_CK_LDS_MAIN);
  const wh::ckp<const DsLayer> plan = wh::ck_make(plan_raw, (long long)n_layers, wh::WH_CK_TABLE);
  const DsLayer Llast = plan[n_layers - 1];
  const wh::ckp<const double> oshift = wh::ck_make(oshift_raw, (long long)Llast.units, wh::WH_CK_TABLE);

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const long long r0 = unit * kDsRows;

  // the segment [lo, hi) of each row of the tile: context never crosses it
  __shared__ long long seg_lds[2 * kDsRows];
  const wh::ckp<long long> sl = wh::ck_make(seg_lds, 2LL * kDsRows, wh::WH_CK_LDS_AUX);
  if (threadIdx.x < kDsRows) {
    const long long r = r0 + threadIdx.x;
    int lo = 0, hi = n_seg;  // the last u with seg[u] <= r (the last segment for the padding rows past n_rows)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (seg[mid] <= r) lo = mid;
      else hi = mid;
    }
    sl[2 * threadIdx.x] = seg[lo];
    sl[2 * threadIdx.x + 1] = seg[lo + 1];
  }
  __syncthreads();

  for (int l = 0; l < n_layers; ++l) {
    const DsLayer L = plan[l];
    const int t0 = kDsNT * w;
    const int nt = L.npad / 16 - t0;
    const int nt_here = nt < 0 ? 0 : (nt > kDsNT ? kDsNT : nt);
    wh::double4_t acc[2][kDsNT] = {};
    // this wave's weight column li of tile t0 at k row lk: the k step and tile are uniform offsets from here
    const wh::ckp<const double> wl =
        wh::ck_sub(wt, L.w_off, (long long)L.kpad * L.npad, wh::WH_CK_TABLE) + ((long long)lk * L.npad + 16 * t0 + li);
    // a wave with fewer than four tiles in a narrow layer repeats its last one (branch-free MFMAs; results not stored)
    int tc[kDsNT];
#pragma unroll
    for (int t = 0; t < kDsNT; ++t) tc[t] = t < nt_here ? t : nt_here - 1;
    // k rows [kc, kc + kn) of the layer against LDS columns [0, kn)
    auto mma = [&](int kc, int kn) {
      const int steps = kn / kDsKS;
      double bnext[4][kDsNT];
      auto fetch = [&](int k0) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int t = 0; t < kDsNT; ++t)
            bnext[kk][t] = wl[(long long)(kc + k0 + 4 * kk) * L.npad + 16 * tc[t]];
      };
      fetch(0);
#pragma unroll 1
      for (int st = 0; st < steps; ++st) {
        double bcur[4][kDsNT];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int t = 0; t < kDsNT; ++t) bcur[kk][t] = bnext[kk][t];
        if (st + 1 < steps) fetch((st + 1) * kDsKS);  // in flight under this step's MFMAs
        const int k0 = st * kDsKS;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const double a0 = A[li * kDsS + k0 + 4 * kk + lk];
          const double a1 = A[(16 + li) * kDsS + k0 + 4 * kk + lk];
#pragma unroll
          for (int t = 0; t < kDsNT; ++t) wh::mfma_pair(acc[0][t], acc[1][t], a0, a1, bcur[kk][t]);
        }
      }
    };
    if (l > 0) {
      if (nt_here > 0) mma(0, L.kpad);
    } else {
      // layer 0 stages its input into the tile, up to 256 columns at a time: thread t gathers row t / 8, columns
      // kc + t % 8 + 8 i, as x[clamp(r + j - window)][c] - shift[c] with k = j d + c (main.py:362-369)
      const int row = threadIdx.x >> 3;
      const long long r = r0 + row, lo = sl[2 * row], hi = sl[2 * row + 1];
      for (int kc = 0; kc < L.kpad; kc += kDsMaxW) {
        const int kn = L.kpad - kc < kDsMaxW ? L.kpad - kc : kDsMaxW;
        for (int kq = threadIdx.x & 7; kq < kn; kq += 8) {
          const int k = kc + kq;
          double v = 0.0;
          if (r < n_rows && k < d_in) {
            const int j = k / d, c = k - j * d;
            long long src = r + j - window;
            src = src < lo ? lo : (src > hi - 1 ? hi - 1 : src);
            v = x[src * ldx + c];
            if (ishift_raw) v = v - ishift[c];
          }
          A[row * kDsS + kq] = v;
        }
        __syncthreads();
        if (nt_here > 0) mma(kc, kn);
        if (kc + kn < L.kpad) __syncthreads();  // the next chunk overwrites the tile
      }
    }
    __syncthreads();  // every wave has read this layer's input: its output may overwrite the buffer
    const bool last = l == n_layers - 1;
#pragma unroll
    for (int t = 0; t < kDsNT; ++t) {
      if (t >= nt_here) continue;
      const int col = 16 * (t0 + t) + li;
      const double bv = bias[L.b_off + col];
      const double sh = last && oshift_raw && col < L.units ? oshift[col] : 0.0;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double v = col < L.units ? ds_act(acc[mt][t][r] + bv, L.act) : 0.0;  // padding columns stay zero
          if (last && oshift_raw) v = v + sh;
          if (l == tap_layer && tap_f32) v = (double)(float)v;  // Keras hands the latent on in float32
          A[(16 * mt + 4 * r + lk) * kDsS + col] = v;
        }
    }
    __syncthreads();
    // the tap layer's and the last layer's outputs leave the tile row by row (contiguous stores)
    if (l == tap_layer || last) {
      const wh::ckp<double> dst = last ? out : tap;
      const long long ld = last ? ldo : ld_tap;
      for (int row = w; row < kDsRows && r0 + row < n_rows; row += 4)
        for (int c = lane; c < L.units; c += 64) dst[(r0 + row) * ld + c] = A[row * kDsS + c];
    }
  }
}

}  // namespace

extern "C" int wh_dense_stack(wh_ctx* ctx, void* stream, const double* x, int64_t n_rows, int d, int64_t ldx,
                              const int64_t* h_seg_off, int n_seg, int window, const double* h_in_shift, int n_layers,
                              const int* h_units, const int* h_act, const double* h_w, const double* h_b, int out_col0,
                              int n_out, int tap_layer, double* tap_out, int64_t ld_tap, int tap_f32,
                              const double* h_out_shift, double* out, int64_t ldo, uint64_t table_tag) {
  static const char* kWhere = "wh_dense_stack";
  if (!ctx || !h_units || !h_act || !h_w || !h_b) return wh::fail_msg(kWhere, "null argument");
  WH_ENTER(ctx);
  if (n_layers < 1 || n_layers > kDsMaxL) return wh::fail_msg(kWhere, "n_layers must be 1 .. 16");
  if (d < 1 || window < 0 || ldx < d) return wh::fail_msg(kWhere, "bad input shape (d >= 1, window >= 0, ldx >= d)");
  const long long d_in_ll = (long long)(2 * (long long)window + 1) * d;
  if (d_in_ll > kDsMaxIn) return wh::fail_msg(kWhere, "input width (2 window + 1) d exceeds the limit of 2048");
  const int d_in = (int)d_in_ll;
  for (int l = 0; l < n_layers; ++l) {
    if (h_units[l] < 1) return wh::fail_msg(kWhere, "every layer needs at least one unit");
    if (l < n_layers - 1 && h_units[l] > kDsMaxW) return wh::fail_msg(kWhere, "layer width exceeds the limit of 256 units");
    if (h_act[l] < kActLinear || h_act[l] > kActSigmoid)
      return wh::fail_msg(kWhere, "activation must be 0 (linear), 1 (relu), 2 (tanh) or 3 (sigmoid)");
  }
  const int u_last = h_units[n_layers - 1];
  if (out_col0 < 0 || n_out < 1 || (long long)out_col0 + n_out > u_last)
    return wh::fail_msg(kWhere, "kept output columns [out_col0, out_col0 + n_out) must lie inside the last layer");
  if (n_out > kDsMaxW) return wh::fail_msg(kWhere, "kept output width exceeds the limit of 256 columns");
  if (ldo < n_out) return wh::fail_msg(kWhere, "ldo < n_out");
  if (tap_layer >= 0) {
    if (tap_layer >= n_layers - 1) return wh::fail_msg(kWhere, "tap_layer must name a layer before the last");
    if (!tap_out || ld_tap < h_units[tap_layer]) return wh::fail_msg(kWhere, "tap output missing or ld_tap too small");
  } else {
    tap_layer = -1;
  }
  if (n_rows < 0) return wh::fail_msg(kWhere, "n_rows < 0");
  if (n_seg < 1 || !h_seg_off) return wh::fail_msg(kWhere, "at least one segment is needed");
  if (h_seg_off[0] != 0 || h_seg_off[n_seg] != n_rows)
    return wh::fail_msg(kWhere, "segment offsets must run from 0 to n_rows");
  for (int u = 0; u < n_seg; ++u)
    if (h_seg_off[u + 1] < h_seg_off[u]) return wh::fail_msg(kWhere, "segment offsets must not decrease");
  if (n_rows == 0) return 0;
  if (!x || !out) return wh::fail_msg(kWhere, "null argument");

  // the plan: per layer its padded shape and offsets; the last layer keeps only columns [out_col0, out_col0 + n_out)
  std::vector<DsLayer> P((size_t)n_layers);
  long long w_total = 0, b_total = 0;
  std::string shape = std::to_string(d_in);
  for (int l = 0; l < n_layers; ++l) {
    const int kin = l == 0 ? d_in : h_units[l - 1];
    const int nu = l == n_layers - 1 ? n_out : h_units[l];
    DsLayer& L = P[l];
    L.kpad = ((kin + kDsKS - 1) / kDsKS) * kDsKS;
    L.npad = ((nu + 15) / 16) * 16;
    L.units = nu;
    L.act = h_act[l];
    L.w_off = w_total;
    L.b_off = (int)b_total;
    w_total += (long long)L.kpad * L.npad;
    b_total += L.npad;
    shape += "." + std::to_string(h_units[l]) + "a" + std::to_string(h_act[l]);
  }
  shape += ".c" + std::to_string(out_col0) + "n" + std::to_string(n_out);
  hipStream_t st = (hipStream_t)stream;
  double* d_w = nullptr;
  double* d_b = nullptr;
  const std::string wslot = table_tag ? "dense.t." + std::to_string(table_tag) + "." + shape + ".w" : "dense.w";
  const std::string bslot = table_tag ? "dense.t." + std::to_string(table_tag) + "." + shape + ".b" : "dense.b";
  if (table_tag) {  // a tagged stack that is already resident: a pointer look-up
    d_w = reinterpret_cast<double*>(wh::persistent_resident(ctx, wslot, (size_t)w_total * sizeof(double)));
    d_b = reinterpret_cast<double*>(wh::persistent_resident(ctx, bslot, (size_t)b_total * sizeof(double)));
  }
  if (!d_w || !d_b) {
    // zero padding: surplus k rows and n columns contribute nothing, padded biases are zero
    std::vector<double> wp((size_t)w_total, 0.0), bp((size_t)b_total, 0.0);
    size_t hw = 0, hb = 0;
    for (int l = 0; l < n_layers; ++l) {
      const DsLayer& L = P[l];
      const int kin = l == 0 ? d_in : h_units[l - 1];
      const int nfull = h_units[l];
      const int c0 = l == n_layers - 1 ? out_col0 : 0;
      for (int k = 0; k < kin; ++k)
        for (int n = 0; n < L.units; ++n) {
          const double v = h_w[hw + (size_t)k * nfull + c0 + n];
          if (!isfinite(v)) return wh::fail_msg(kWhere, "non-finite weight");
          wp[(size_t)L.w_off + (size_t)k * L.npad + n] = v;
        }
      for (int n = 0; n < L.units; ++n) {
        const double v = h_b[hb + c0 + n];
        if (!isfinite(v)) return wh::fail_msg(kWhere, "non-finite bias");
        bp[(size_t)L.b_off + n] = v;
      }
      hw += (size_t)kin * nfull;
      hb += (size_t)nfull;
    }
    if (int rc = wh::persistent_upload(ctx, st, wslot, wp, &d_w)) return rc;
    if (int rc = wh::persistent_upload(ctx, st, bslot, bp, &d_b)) return rc;
  }
  DsLayer* d_plan = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "dense.plan", P, &d_plan)) return rc;
  std::vector<long long> segv(h_seg_off, h_seg_off + n_seg + 1);
  long long* d_seg = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "dense.seg", segv, &d_seg)) return rc;
  double* d_is = nullptr;
  double* d_os = nullptr;
  if (h_in_shift) {
    std::vector<double> v(h_in_shift, h_in_shift + d);
    if (int rc = wh::persistent_upload(ctx, st, "dense.ishift", v, &d_is)) return rc;
  }
  if (h_out_shift) {
    std::vector<double> v(h_out_shift, h_out_shift + n_out);
    if (int rc = wh::persistent_upload(ctx, st, "dense.oshift", v, &d_os)) return rc;
  }
  const long long n_tiles = (n_rows + kDsRows - 1) / kDsRows;
  const long long x_n = (n_rows - 1) * ldx + d;
  const long long tap_n = tap_layer >= 0 ? (n_rows - 1) * ld_tap + h_units[tap_layer] : 0;
  const long long out_n = (n_rows - 1) * ldo + n_out;
  WH_LAUNCH(ctx, st, "dense_stack_kernel", dense_stack_kernel, dim3((unsigned)wh::xcd_grid(n_tiles)), dim3(256), 0, x,
            x_n, n_rows, d, ldx, d_in, d_seg, n_seg, window, d_is, d_plan, n_layers, tap_layer, tap_f32 ? 1 : 0, d_w,
            w_total, d_b, b_total, tap_layer >= 0 ? tap_out : nullptr, tap_n, ld_tap, d_os, out, out_n, ldo);
  return 0;
}
