// What World.set_pitch leaves open (world/main.py:164-168: "need to resample to set values at given temporal positions
// (which are presumably shared with the spectrogram)"): a pitch contour from outside interpolated onto a batch's frame
// times (wh_interp_contour), and a resident encoding's frame-major tensors moved to another frame grid (wh_regrid_rows).
// Both are np.interp, bit for bit — the arithmetic modify_duration_kernel and warp_spectrum_kernel (wh_modify.hip)
// reproduce, with a binary search for knot lists of thousands of points and NumPy's retry where the result is NaN.
#include <math.h>

#include "wh_device.h"
#include "wh_host.h"

namespace {

// np.interp's search for one query point over the n knots xp (strictly increasing): j = the knot whose value is read
// first.  den == 0 marks the cases in which NumPy returns fp[j] itself — beyond either end (the end values), the last
// knot, an exact hit; otherwise den = xp[j+1] - xp[j], dx = x - xp[j] and dx2 = x - xp[j+1] (the retry's abscissa).
struct Located {
  long long j;
  double dx, den, dx2;
};

__device__ __forceinline__ Located np_interp_locate(const wh::ckp<const double>& xp, long long n, double x) {
#pragma clang fp contract(off)
  Located r = {0, 0.0, 0.0, 0.0};
  if (x > xp[n - 1]) {
    r.j = n - 1;
    return r;
  }
  if (!(x > xp[0])) return r;  // below the first knot, or on it
  long long lo = 0, hi = n - 1;  // xp[lo] <= x <= xp[hi]: the last j with xp[j] <= x by bisection
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (xp[mid] <= x) lo = mid;
    else hi = mid;
  }
  if (xp[hi] <= x) lo = hi;  // (on the last knot of the bracket)
  r.j = lo;
  if (lo == n - 1 || xp[lo] == x) return r;
  r.den = xp[lo + 1] - xp[lo];
  r.dx = x - xp[lo];
  r.dx2 = x - xp[lo + 1];
  return r;
}

// NumPy's value between two knots (compiled_base.c, arr_interp): the slope form, the same from the other knot where
// that is NaN (an infinite value on one side), and the common value where both are NaN and the two values agree
__device__ __forceinline__ double np_interp_value(double a, double b, double dx, double den, double dx2) {
#pragma clang fp contract(off)
  const double slope = (b - a) / den;
  double v = slope * dx + a;
  if (v != v) {
    v = slope * dx2 + b;
    if (v != v && a == b) v = a;
  }
  return v;
}

// ---- wh_interp_contour: one thread per frame ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void interp_contour_kernel(const double* __restrict__ tp_, const int32_t* __restrict__ frame_utt_,
                                                             long long n_frames, const int64_t* __restrict__ knot_off_,
                                                             int n_utt, const double* __restrict__ kt_,
                                                             const double* __restrict__ kv_, long long n_knots, int voiced_rule,
                                                             double* __restrict__ out_, double* __restrict__ vuv_) {
  const wh::ckp<const double> tp = wh::ck_make(tp_, n_frames, wh::WH_CK_IN);
  const wh::ckp<const int32_t> frame_utt = wh::ck_make(frame_utt_, n_frames, wh::WH_CK_IN);
  const wh::ckp<const int64_t> knot_off = wh::ck_make(knot_off_, n_utt + 1, wh::WH_CK_TABLE);
  const wh::ckp<double> out = wh::ck_make(out_, n_frames, wh::WH_CK_OUT);
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= n_frames) return;
  const int u = frame_utt[f];
  const long long k0 = knot_off[u], n = knot_off[u + 1] - k0;
  const wh::ckp<const double> xp = wh::ck_sub(wh::ck_make(kt_, n_knots, wh::WH_CK_TABLE), k0, n, wh::WH_CK_TABLE);
  const wh::ckp<const double> fp = wh::ck_sub(wh::ck_make(kv_, n_knots, wh::WH_CK_TABLE), k0, n, wh::WH_CK_TABLE);
  const double x = tp[f];
  double r;
  bool voiced;
  if (x != x) {  // NumPy hands a NaN query back
    r = x;
    voiced = false;
  } else {
    const Located p = np_interp_locate(xp, n, x);
    const double a = fp[p.j];
    if (p.den == 0.0) {
      r = a;
      voiced = a > 0.0;
    } else {
      const double b = fp[p.j + 1];
      r = np_interp_value(a, b, p.dx, p.den, p.dx2);
      voiced = a > 0.0 && b > 0.0;
    }
  }
  if (voiced_rule) {
    out[f] = voiced ? r : 0.0;
    if (vuv_) wh::ck_make(vuv_, n_frames, wh::WH_CK_OUT)[f] = voiced ? 1.0 : 0.0;
  } else {
    out[f] = r;
  }
}

// ---- wh_regrid_rows ------------------------------------------------------------------------------------------------
// The search is done once per DESTINATION FRAME by regrid_plan_kernel (one thread each): the source row to read first as
// an index into the whole source tensor, and the three abscissa terms.  32 B per frame, against k_bins * 8 B per row
// moved.
__global__ __launch_bounds__(256) void regrid_plan_kernel(const double* __restrict__ tp_src_, const double* __restrict__ tp_dst_,
                                                          const int64_t* __restrict__ src_off_, const int32_t* __restrict__ dst_utt_,
                                                          int n_utt, long long n_src, long long n_dst,
                                                          long long* __restrict__ pj_, double* __restrict__ pdx_,
                                                          double* __restrict__ pden_, double* __restrict__ pdx2_) {
  const wh::ckp<const double> tp_dst = wh::ck_make(tp_dst_, n_dst, wh::WH_CK_IN);
  const wh::ckp<const int64_t> src_off = wh::ck_make(src_off_, n_utt + 1, wh::WH_CK_TABLE);
  const wh::ckp<const int32_t> dst_utt = wh::ck_make(dst_utt_, n_dst, wh::WH_CK_IN);
  const wh::ckp<long long> pj = wh::ck_make(pj_, n_dst, wh::WH_CK_OUT);
  const wh::ckp<double> pdx = wh::ck_make(pdx_, n_dst, wh::WH_CK_OUT);
  const wh::ckp<double> pden = wh::ck_make(pden_, n_dst, wh::WH_CK_OUT);
  const wh::ckp<double> pdx2 = wh::ck_make(pdx2_, n_dst, wh::WH_CK_OUT);
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= n_dst) return;
  const int u = dst_utt[f];
  const long long s0 = src_off[u], n = src_off[u + 1] - s0;  // (n >= 1: checked on the host)
  const wh::ckp<const double> xp = wh::ck_sub(wh::ck_make(tp_src_, n_src, wh::WH_CK_IN), s0, n, wh::WH_CK_IN);
  const Located p = np_interp_locate(xp, n, tp_dst[f]);
  pj[f] = s0 + p.j;
  pdx[f] = p.dx;
  pden[f] = p.den;
  pdx2[f] = p.dx2;
}

// The row kernel is memory-bound: per output row one or two source rows in, one row out.  A workgroup owns `rows`
// consecutive destination frames (an even number), takes their plan entries to LDS and walks the group's bins as PAIRS
// of the flat output, as ap_from_bands_kernel does (wh_apbands.hip): K is odd for the dense tensors, so a single row is
// not 16-byte aligned, but an even number of rows is — every pair is one 16-byte store whichever rows its two bins
// belong to.  The source side of a pair that lies inside one row is one 16-byte load where its address allows
// (rows of odd K alternate) and two 8-byte loads of the same 16 bytes where it does not.  The scalar instantiation
// serves an output that does not start on a 16-byte boundary.
constexpr int kRgThreads = 256;
constexpr int kRgMaxRows = 256;

struct RowPlan {
  long long s;  // flat index of the first source element read: (source row) * k_bins + bin
  double dx, den, dx2;
};

__device__ __forceinline__ double regrid_one(double a, double b, const RowPlan& p, int positive) {
  const double v = np_interp_value(a, b, p.dx, p.den, p.dx2);
  return (positive && !(a > 0.0 && b > 0.0)) ? 0.0 : v;
}

__device__ __forceinline__ double regrid_copy(double a, int positive) { return (positive && !(a > 0.0)) ? 0.0 : a; }

// one bin
__device__ __forceinline__ double regrid_bin(const wh::ckp<const double>& in, int k_bins, const RowPlan& p, int positive) {
  const double a = in[p.s];
  if (p.den == 0.0) return regrid_copy(a, positive);
  return regrid_one(a, in[p.s + k_bins], p, positive);
}

// elements s and s + 1 of the source
__device__ __forceinline__ void regrid_load2(const wh::ckp<const double>& in, long long s, double& v0, double& v1) {
#if WH_BOUNDS
  v0 = in[s];
  v1 = in[s + 1];
#else
  const double* q = in + s;
  if ((reinterpret_cast<uintptr_t>(q) & 15) == 0) {
    const double2 t = wh::ldg2(reinterpret_cast<const double2*>(q));
    v0 = t.x;
    v1 = t.y;
  } else {
    v0 = wh::ldg(q);
    v1 = wh::ldg(q + 1);
  }
#endif
}

template <bool VEC>
__global__ __launch_bounds__(kRgThreads) void regrid_rows_kernel(const double* __restrict__ in_, double* __restrict__ out_,
                                                                 const long long* __restrict__ pj_,
                                                                 const double* __restrict__ pdx_,
                                                                 const double* __restrict__ pden_,
                                                                 const double* __restrict__ pdx2_, long long n_src,
                                                                 long long n_dst, int k_bins, int rows, int positive) {
  __shared__ long long s_j[kRgMaxRows];
  __shared__ double s_dx[kRgMaxRows], s_den[kRgMaxRows], s_dx2[kRgMaxRows];
  const wh::ckp<long long> lj = wh::ck_make(s_j, kRgMaxRows, wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> ldx = wh::ck_make(s_dx, kRgMaxRows, wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> lden = wh::ck_make(s_den, kRgMaxRows, wh::WH_CK_LDS_OTHER);
  const wh::ckp<double> ldx2 = wh::ck_make(s_dx2, kRgMaxRows, wh::WH_CK_LDS_OTHER);
  const wh::ckp<const long long> pj = wh::ck_make(pj_, n_dst, wh::WH_CK_TABLE);
  const wh::ckp<const double> pdx = wh::ck_make(pdx_, n_dst, wh::WH_CK_TABLE);
  const wh::ckp<const double> pden = wh::ck_make(pden_, n_dst, wh::WH_CK_TABLE);
  const wh::ckp<const double> pdx2 = wh::ck_make(pdx2_, n_dst, wh::WH_CK_TABLE);
  const wh::ckp<const double> in = wh::ck_make(in_, n_src * k_bins, wh::WH_CK_IN);
  const wh::ckp<double> out = wh::ck_make(out_, n_dst * k_bins, wh::WH_CK_OUT);
  const long long f0 = (long long)blockIdx.x * rows;
  const int nf = (int)(n_dst - f0 < rows ? n_dst - f0 : rows);
  for (int i = threadIdx.x; i < nf; i += kRgThreads) {
    lj[i] = pj[f0 + i];
    ldx[i] = pdx[f0 + i];
    lden[i] = pden[f0 + i];
    ldx2[i] = pdx2[f0 + i];
  }
  __syncthreads();
  const auto plan = [&](int fr, int k) {
    RowPlan p;
    p.s = lj[fr] * k_bins + k;  // (64-bit: 2 049 024 frames x 513 bins x 8 B is beyond 2^31 bytes)
    p.dx = ldx[fr];
    p.den = lden[fr];
    p.dx2 = ldx2[fr];
    return p;
  };
  const int n_el = nf * k_bins;  // (at most 256 rows x 16385 bins)
  const long long e0 = f0 * k_bins;
  if constexpr (VEC) {
    const wh::ckp<double2> out2 = wh::ck_as<double2>(out);  // f0 * k_bins is even: rows is
    for (int e = 2 * threadIdx.x; e < n_el; e += 2 * kRgThreads) {
      const int fr = e / k_bins;
      const int k = e - fr * k_bins;
      const RowPlan p = plan(fr, k);
      if (k + 1 < k_bins) {  // both bins in row fr
        double a0, a1, v0, v1;
        regrid_load2(in, p.s, a0, a1);
        if (p.den == 0.0) {
          v0 = regrid_copy(a0, positive);
          v1 = regrid_copy(a1, positive);
        } else {
          double b0, b1;
          regrid_load2(in, p.s + k_bins, b0, b1);
          v0 = regrid_one(a0, b0, p, positive);
          v1 = regrid_one(a1, b1, p, positive);
        }
        out2[(e0 + e) >> 1] = make_double2(v0, v1);
      } else {
        const double v0 = regrid_bin(in, k_bins, p, positive);
        if (e + 1 < n_el) {  // the pair straddles two rows
          out2[(e0 + e) >> 1] = make_double2(v0, regrid_bin(in, k_bins, plan(fr + 1, 0), positive));
        } else {
          out[e0 + e] = v0;  // the last bin of a batch with an odd number of elements
        }
      }
    }
  } else {
    for (int e = threadIdx.x; e < n_el; e += kRgThreads) {
      const int fr = e / k_bins;
      out[e0 + e] = regrid_bin(in, k_bins, plan(fr, e - fr * k_bins), positive);
    }
  }
}

// destination frames per workgroup: even (the pairs' alignment), about 4096 bins' worth, 8 for the dense tensors
int regrid_rows_per_group(int k_bins) {
  int rows = (4096 + k_bins - 1) / k_bins;
  rows += rows & 1;
  return rows < 8 ? 8 : (rows > kRgMaxRows ? kRgMaxRows : rows);
}

}  // namespace

extern "C" int wh_interp_contour(wh_ctx* ctx, void* stream, const wh_batch* b, const double* tp, const int64_t* h_knot_off,
                                 const double* h_time, const double* h_value, int voiced_rule, double* out,
                                 double* vuv_out) {
  if (!ctx || !b || !h_knot_off || !h_time || !h_value) return wh::fail_msg("wh_interp_contour", "null argument");
  WH_ENTER(ctx);
  // the knot lists, before anything reaches a kernel
  if (h_knot_off[0] != 0) return wh::fail_msg("wh_interp_contour", "h_knot_off must start at 0");
  for (int u = 0; u < b->n_utt; ++u) {
    if (h_knot_off[u + 1] <= h_knot_off[u]) return wh::fail_msg("wh_interp_contour", "every utterance needs at least one knot");
    for (int64_t i = h_knot_off[u]; i < h_knot_off[u + 1]; ++i) {
      if (!isfinite(h_time[i])) return wh::fail_msg("wh_interp_contour", "knot times must be finite");
      if (i > h_knot_off[u] && !(h_time[i] > h_time[i - 1]))
        return wh::fail_msg("wh_interp_contour", "knot times must be strictly increasing");
    }
  }
  if (b->total_frames == 0) return 0;
  if (!tp || !out) return wh::fail_msg("wh_interp_contour", "null argument");
  if (out == tp || (vuv_out && (vuv_out == tp || vuv_out == out))) return wh::fail_msg("wh_interp_contour", "outputs must not alias");
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_knots = h_knot_off[b->n_utt];
  std::vector<int64_t> off(h_knot_off, h_knot_off + b->n_utt + 1);
  std::vector<double> kt(h_time, h_time + n_knots), kv(h_value, h_value + n_knots);
  int64_t* d_off = nullptr;
  double *d_kt = nullptr, *d_kv = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "contour.off", off, &d_off)) return rc;
  if (int rc = wh::persistent_upload(ctx, st, "contour.time", kt, &d_kt)) return rc;
  if (int rc = wh::persistent_upload(ctx, st, "contour.value", kv, &d_kv)) return rc;
  const long long blocks = (b->total_frames + 255) / 256;
  if (blocks > 0x7fffffffLL) return wh::fail_msg("wh_interp_contour", "too many frames for one launch");
  WH_LAUNCH(ctx, st, "interp_contour_kernel", interp_contour_kernel, dim3((unsigned)blocks), dim3(256), 0, tp,
            b->d_frame_utt, b->total_frames, d_off, b->n_utt, d_kt, d_kv, n_knots, voiced_rule, out,
            voiced_rule ? vuv_out : nullptr);
  return 0;
}

extern "C" int wh_regrid_rows(wh_ctx* ctx, void* stream, const wh_batch* src, const wh_batch* dst, const double* tp_src,
                              const double* tp_dst, const double* in, double* out, int k_bins, int positive_rule) {
  if (!ctx || !src || !dst) return wh::fail_msg("wh_regrid_rows", "null argument");
  WH_ENTER(ctx);
  if (src->n_utt != dst->n_utt) return wh::fail_msg("wh_regrid_rows", "the two grids must describe the same utterances");
  if (k_bins < 1 || k_bins > 16385) return wh::fail_msg("wh_regrid_rows", "k_bins out of range");
  for (int u = 0; u < dst->n_utt; ++u)
    if (dst->h_frame_off[u + 1] > dst->h_frame_off[u] && src->h_frame_off[u + 1] <= src->h_frame_off[u])
      return wh::fail_msg("wh_regrid_rows", "an utterance with destination frames has no source frame");
  const long long n_src = src->total_frames, n_dst = dst->total_frames;
  if (n_dst == 0) return 0;
  if (!tp_src || !tp_dst || !in || !out) return wh::fail_msg("wh_regrid_rows", "null argument");
  {
    const char *a0 = (const char*)in, *a1 = a0 + (size_t)n_src * k_bins * 8, *b0 = (const char*)out,
               *b1 = b0 + (size_t)n_dst * k_bins * 8;
    if (a0 < b1 && b0 < a1) return wh::fail_msg("wh_regrid_rows", "out must not overlap in");
  }
  hipStream_t st = (hipStream_t)stream;
  long long* pj = nullptr;  // per frame: the source row, then three doubles
  if (int rc = wh::persistent_scratch(ctx, "regrid.plan", (size_t)n_dst * 4, &pj)) return rc;
  double* pdx = reinterpret_cast<double*>(pj + n_dst);
  double* pden = pdx + n_dst;
  double* pdx2 = pden + n_dst;
  const long long pblocks = (n_dst + 255) / 256;
  const int rows = regrid_rows_per_group(k_bins);
  const long long groups = (n_dst + rows - 1) / rows;
  if (pblocks > 0x7fffffffLL || groups > 0x7fffffffLL) return wh::fail_msg("wh_regrid_rows", "too many frames for one launch");
  WH_LAUNCH(ctx, st, "regrid_plan_kernel", regrid_plan_kernel, dim3((unsigned)pblocks), dim3(256), 0, tp_src, tp_dst,
            src->d_frame_off, dst->d_frame_utt, dst->n_utt, n_src, n_dst, pj, pdx, pden, pdx2);
  const bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  WH_LAUNCH(ctx, st, "regrid_rows_kernel", vec ? regrid_rows_kernel<true> : regrid_rows_kernel<false>,
            dim3((unsigned)groups), dim3(kRgThreads), 0, in, out, pj, pdx, pden, pdx2, n_src, n_dst, k_bins, rows,
            positive_rule);
  return 0;
}
