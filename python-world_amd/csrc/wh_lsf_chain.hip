// The two per-frame steps a chain over line spectral frequencies needs besides csrc/wh_lsf.hip's coding: the repair of a
// track that a model produced (lsf_repair_kernel) and the log-spectral distortion of two rows' all-pole envelopes on
// aligned frames, in product form, without either envelope in memory (lsf_distortion_kernel).  Contracts:
// include/world_hip.h; tests/_lsf_chain_reference.py is the same in NumPy.  Built like wh_lsf.hip:
// build.py's default -ffp-contract=off, every product and sum rounded on its own.
//
// lsf_repair_kernel: one lane per frame, 64 frames per workgroup of one wave.  The tile of 64 rows is read with
//   consecutive lanes on consecutive addresses and kept in LDS as [index][lane] with a row pitch of 65 doubles (the
//   transposing write lands on 64 different bank pairs, the lane's own column is conflict-free); the forward and the
//   backward scan walk a lane's column, and the tile goes out the way it came in.  The whole tile is in LDS before the
//   first store, so out == w is allowed.  `changed` re-reads the input next to the store (same thread, same address).
// lsf_distortion_kernel: one wave per pair, four pairs per workgroup; the waves share nothing and meet at no barrier.
//   The doubled roots of both rows are staged once in the wave's LDS; a lane carries kDistBins bins at a time (a root is
//   one broadcast LDS read for kDistBins factors), the two sums are kept per lane over its bins in ascending order and
//   finished by wh::wave_sum: a fixed order that does not depend on the other pairs of the call.
#include <math.h>

#include "wh_device.h"
#include "wh_host.h"
#include "wh_reduce.h"

namespace {

constexpr int kLsfMaxOrder = 64;
constexpr int kRepairPitch = WH_WAVE + 1;  // doubles between two indices of the LDS tile
constexpr int kDistWaves = 4;              // pairs per workgroup of lsf_distortion_kernel
constexpr int kDistBins = 4;               // bins a lane carries side by side

// torch's maximum / minimum: a NaN operand gives that NaN (fmax / fmin would drop it)
__device__ __forceinline__ double max_nan(double a, double b) { return a != a ? a : b != b ? b : a > b ? a : b; }
__device__ __forceinline__ double min_nan(double a, double b) { return a != a ? a : b != b ? b : a < b ? a : b; }

// ---- a. repair ---------------------------------------------------------------------------------------------------------
// (w_ and out_ may be the same buffer: no __restrict__)
__global__ __launch_bounds__(WH_WAVE) void lsf_repair_kernel(const double* w_, long long n_frames, long long ldw, int p,
                                                             double gap, double hi, double* out_, long long ldo,
                                                             int32_t* changed_) {
  extern __shared__ double s_rep[];
  const wh::ckp<const double> w = wh::ck_make(w_, (n_frames - 1) * ldw + p, wh::WH_CK_IN);
  const wh::ckp<double> out = wh::ck_make(out_, (n_frames - 1) * ldo + p, wh::WH_CK_OUT);
  const wh::ckp<int32_t> changed = wh::ck_make(changed_, changed_ ? n_frames : 0, wh::WH_CK_OUT);
  const wh::ckp<double> s = wh::ck_make(s_rep, (long long)p * kRepairPitch, wh::WH_CK_LDS_MAIN);
  const int lane = threadIdx.x;
  const long long f0 = (long long)blockIdx.x * WH_WAVE;
  const int nf = (int)(n_frames - f0 < WH_WAVE ? n_frames - f0 : WH_WAVE);
  const int n_el = nf * p;
  // element e = fr * p + col of the tile: one division per lane, then (fr, col) walk on by 64 = step_fr * p + step_col
  const int fr0 = lane / p, col0 = lane - fr0 * p, step_fr = WH_WAVE / p, step_col = WH_WAVE - step_fr * p;
  for (int e = lane, fr = fr0, col = col0; e < n_el; e += WH_WAVE) {
    s[col * kRepairPitch + fr] = w[(f0 + fr) * ldw + col];
    fr += step_fr;
    col += step_col;
    if (col >= p) {
      col -= p;
      ++fr;
    }
  }
  __syncthreads();
  if (lane < nf) {
    double prev = min_nan(max_nan(s[lane], gap), hi);
    s[lane] = prev;
    for (int i = 1; i < p; ++i) {
      const double x = max_nan(min_nan(max_nan(s[i * kRepairPitch + lane], gap), hi), prev + gap);
      s[i * kRepairPitch + lane] = x;
      prev = x;
    }
    prev = min_nan(prev, hi);
    s[(p - 1) * kRepairPitch + lane] = prev;
    for (int i = p - 2; i >= 0; --i) {
      const double x = min_nan(s[i * kRepairPitch + lane], prev - gap);
      s[i * kRepairPitch + lane] = x;
      prev = x;
    }
  }
  __syncthreads();
  for (int e = lane, fr = fr0, col = col0; e < n_el; e += WH_WAVE) {
    const double x = s[col * kRepairPitch + fr];
    if (changed_) {
      const double old = w[(f0 + fr) * ldw + col];
      s[col * kRepairPitch + fr] = __double_as_longlong(old) != __double_as_longlong(x) ? 1.0 : 0.0;
    }
    out[(f0 + fr) * ldo + col] = x;
    fr += step_fr;
    col += step_col;
    if (col >= p) {
      col -= p;
      ++fr;
    }
  }
  if (!changed_) return;
  __syncthreads();
  if (lane < nf) {
    int n = 0;
    for (int i = 0; i < p; ++i) n += s[i * kRepairPitch + lane] != 0.0;
    changed[f0 + lane] = n;
  }
}

// ---- b. log-spectral distortion of two rows ------------------------------------------------------------------------------
__global__ __launch_bounds__(kDistWaves* WH_WAVE) void lsf_distortion_kernel(
    const double* __restrict__ rows_a_, long long n_rows_a, long long lda, const double* __restrict__ rows_b_,
    long long n_rows_b, long long ldb, int p, const long long* __restrict__ idx_a_, const long long* __restrict__ idx_b_,
    long long n_pairs, const double* __restrict__ cos_, int k_bins, double* __restrict__ out_) {
  __shared__ double s_x[kDistWaves][2][kLsfMaxOrder];  // 2 x_i of side a and of side b
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WH_WAVE), lane = threadIdx.x % WH_WAVE;
  const long long n = (long long)blockIdx.x * kDistWaves + wave;
  if (n >= n_pairs) return;  // (wave-uniform)
  const wh::ckp<const double> rows_a = wh::ck_make(rows_a_, (n_rows_a - 1) * lda + p + 1, wh::WH_CK_IN);
  const wh::ckp<const double> rows_b = wh::ck_make(rows_b_, (n_rows_b - 1) * ldb + p + 1, wh::WH_CK_IN);
  const wh::ckp<const long long> idx_a = wh::ck_make(idx_a_, idx_a_ ? n_pairs : 0, wh::WH_CK_IN);
  const wh::ckp<const long long> idx_b = wh::ck_make(idx_b_, idx_b_ ? n_pairs : 0, wh::WH_CK_IN);
  const wh::ckp<const double> ctab = wh::ck_make(cos_, k_bins, wh::WH_CK_TABLE);
  const wh::ckp<double> out = wh::ck_make(out_, 2 * n_pairs, wh::WH_CK_OUT);
  const wh::ckp<double> xa = wh::ck_make(&s_x[wave][0][0], kLsfMaxOrder, wh::WH_CK_LDS_MAIN);
  const wh::ckp<double> xb = wh::ck_make(&s_x[wave][1][0], kLsfMaxOrder, wh::WH_CK_LDS_AUX);
  const long long ia = idx_a_ ? idx_a[n] : n, ib = idx_b_ ? idx_b[n] : n;
  if (ia < 0 || ia >= n_rows_a || ib < 0 || ib >= n_rows_b) {  // (wave-uniform: every lane read the same two indices)
    if (lane < 2) out[2 * n + lane] = __builtin_nan("");
    return;
  }
  if (lane < p) {
    xa[lane] = 2.0 * rows_a[ia * lda + 1 + lane];
    xb[lane] = 2.0 * rows_b[ib * ldb + 1 + lane];
  }
  wh::sync<WH_WAVE>();
  double s1 = 0.0, s2 = 0.0;
  for (int k0 = 0; k0 < k_bins; k0 += kDistBins * WH_WAVE) {
    double tc[kDistBins], ua[kDistBins], va[kDistBins], ub[kDistBins], vb[kDistBins];
#pragma unroll
    for (int j = 0; j < kDistBins; ++j) {
      const int k = k0 + j * WH_WAVE + lane;
      tc[j] = 2.0 * ctab[k < k_bins ? k : k_bins - 1];  // (a lane past the last bin repeats it and adds nothing)
      ua[j] = va[j] = ub[j] = vb[j] = 1.0;
    }
    for (int i = 0; i < p; i += 2) {
      const double a0 = xa[i], a1 = xa[i + 1], b0 = xb[i], b1 = xb[i + 1];
#pragma unroll
      for (int j = 0; j < kDistBins; ++j) {
        ua[j] = ua[j] * (tc[j] - a0);
        va[j] = va[j] * (tc[j] - a1);
        ub[j] = ub[j] * (tc[j] - b0);
        vb[j] = vb[j] * (tc[j] - b1);
      }
    }
#pragma unroll
    for (int j = 0; j < kDistBins; ++j) {
      const double c = 0.5 * tc[j];
      const double fp = 2.0 * (1.0 + c), fm = 2.0 * (1.0 - c);
      const double a2a = 0.25 * (fp * (ua[j] * ua[j]) + fm * (va[j] * va[j]));
      const double a2b = 0.25 * (fp * (ub[j] * ub[j]) + fm * (vb[j] * vb[j]));
      const double t = log(a2a / a2b);
      if (k0 + j * WH_WAVE + lane < k_bins) {
        s1 = s1 + t;
        s2 = s2 + t * t;
      }
    }
  }
  s1 = wh::wave_sum(s1);
  s2 = wh::wave_sum(s2);
  if (lane == 0) {
    out[2 * n] = s1;  // (64-bit: n_pairs is not bounded by 2^31 / 16)
    out[2 * n + 1] = s2;
  }
}

int chain_check_order(const char* where, int p) {
  if (p < 2 || p > kLsfMaxOrder) return wh::fail_msg(where, "the order p must be in [2, 64]");
  return 0;
}

}  // namespace

extern "C" int wh_lsf_repair(wh_ctx* ctx, void* stream, const double* w, int64_t n_frames, int64_t ldw, int p, double gap,
                             double hi, double* out, int64_t ldo, int32_t* changed) {
  if (!ctx) return wh::fail_msg("wh_lsf_repair", "null argument");
  WH_ENTER(ctx);
  if (int rc = chain_check_order("wh_lsf_repair", p)) return rc;
  if (n_frames < 0) return wh::fail_msg("wh_lsf_repair", "negative frame count");
  if (ldw < p) return wh::fail_msg("wh_lsf_repair", "ldw must be at least p");
  if (ldo < p) return wh::fail_msg("wh_lsf_repair", "ldo must be at least p");
  if (!(gap > 0.0) || !(hi >= gap)) return wh::fail_msg("wh_lsf_repair", "gap must be positive and hi at least gap");
  if (n_frames == 0) return 0;
  if (!w || !out) return wh::fail_msg("wh_lsf_repair", "null argument");
  const long long blocks = (n_frames + WH_WAVE - 1) / WH_WAVE;
  if (blocks > 0x7fffffffLL) return wh::fail_msg("wh_lsf_repair", "too many frames for one call");
  const size_t lds = (size_t)p * kRepairPitch * sizeof(double);
  hipStream_t st = (hipStream_t)stream;
  WH_LAUNCH(ctx, st, "lsf_repair_kernel", lsf_repair_kernel, dim3((unsigned)blocks), dim3(WH_WAVE), lds, w, n_frames,
            ldw, p, gap, hi, out, ldo, changed);
  return 0;
}

extern "C" int wh_lsf_distortion(wh_ctx* ctx, void* stream, const double* rows_a, int64_t n_rows_a, int64_t lda,
                                 const double* rows_b, int64_t n_rows_b, int64_t ldb, int p, const int64_t* idx_a,
                                 const int64_t* idx_b, int64_t n_pairs, const double* h_cos, int k_bins, double* out) {
  if (!ctx) return wh::fail_msg("wh_lsf_distortion", "null argument");
  WH_ENTER(ctx);
  if (p < 2 || p > kLsfMaxOrder || (p & 1)) return wh::fail_msg("wh_lsf_distortion", "the order p must be even and in [2, 64]");
  if (n_rows_a < 0 || n_rows_b < 0 || n_pairs < 0) return wh::fail_msg("wh_lsf_distortion", "negative count");
  if (k_bins < 2 || k_bins > 16385) return wh::fail_msg("wh_lsf_distortion", "k_bins out of range");
  if (lda < p + 1) return wh::fail_msg("wh_lsf_distortion", "lda must be at least p + 1");
  if (ldb < p + 1) return wh::fail_msg("wh_lsf_distortion", "ldb must be at least p + 1");
  if (!h_cos) return wh::fail_msg("wh_lsf_distortion", "null argument");
  if (n_pairs == 0) return 0;
  if (!out || (n_rows_a > 0 && !rows_a) || (n_rows_b > 0 && !rows_b)) return wh::fail_msg("wh_lsf_distortion", "null argument");
  const long long blocks = (n_pairs + kDistWaves - 1) / kDistWaves;
  if (blocks > 0x7fffffffLL) return wh::fail_msg("wh_lsf_distortion", "too many pairs for one call");
  hipStream_t st = (hipStream_t)stream;
  void* d_cos = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "lsf.bins", h_cos, (size_t)k_bins * sizeof(double), &d_cos)) return rc;
  WH_LAUNCH(ctx, st, "lsf_distortion_kernel", lsf_distortion_kernel, dim3((unsigned)blocks), dim3(kDistWaves * WH_WAVE),
            0, rows_a, n_rows_a, lda, rows_b, n_rows_b, ldb, p, reinterpret_cast<const long long*>(idx_a),
            reinterpret_cast<const long long*>(idx_b), n_pairs, reinterpret_cast<const double*>(d_cos), k_bins, out);
  return 0;
}
