// ================================================================================================
// Exemplar-based conversion (frame selection): the K nearest database rows of every query row by brute force, and one
// candidate per frame by a Viterbi pass that trades closeness against the continuity of the chosen target frames.
// Contract: include/world_hip.h; tests/_exemplar_reference.py is the same in NumPy, and every output
// (idx, dist, sel, slot, total, the accumulated costs) is compared bit for bit.
//
//   knn_tile_kernel      a workgroup owns kKnnTileQ queries and one consecutive range of database rows (the cut:
//                        blockIdx.y).  Database tiles of kKnnTileR rows pass through LDS in strips of kKnnStrip columns,
//                        both sides transposed ([column][row]); a thread keeps a 4 x 4 block of pair sums, sixteen
//                        independent add chains whose column order is fixed: each difference, product and sum rounded on
//                        its own (build.py's default -ffp-contract=off; the zero columns behind d add +0.0 to a sum that
//                        is never -0.0).  A finished tile's keys (NaN -> +inf) go to LDS over the strips, and the first
//                        wave, one lane per query, offers them to the query's sorted K-list in LDS: a candidate below
//                        the list's last entry under (key, row) is inserted by K compare-selects — no address and no
//                        trip count depends on a value.
//   knn_merge_kernel     more than one range: one thread per query offers every range's list to one list, same order.
//   frame_sources_kernel the rows a frame's slots stand for, range-tested once: y row of slot k, y row of its successor
//                        (-1: invalid).
//   frame_select_kernel  one workgroup per utterance, a loop over its frames.  The 2 K rows of the next frame are gathered
//                        from global memory into registers while this frame's K x K chains run out of LDS, and stored
//                        behind them (their indices wait in LDS, fetched two frames ahead); thread k then takes the minimum over j in the contract's order (a literal scan), and
//                        the back-pointers (one byte per frame and slot) go to the context's scratch.  The walk back reads
//                        them through LDS in pieces of kFsChunk frames.
// The order of the K-lists is total, so neither the tiling nor the cut shows in a result.  No atomics.
// ================================================================================================
#include <math.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "wh_device.h"
#include "wh_host.h"

namespace {

// (world/exemplar.py exports the same numbers to the tests: tests/test_exemplar_host.py compares them with this file)
constexpr int kKnnTileQ = 64;
constexpr int kKnnTileR = 64;
constexpr int kKnnStrip = 16;
constexpr int kKnnMaxD = 160;
constexpr int kKnnMaxK = 32;
constexpr int kKnnThreads = 256;
constexpr int kKnnLd = 68;  // row stride of the transposed strips and of the key tile (16-byte aligned reads of 4)
constexpr int kKnnEmpty = std::numeric_limits<int>::max();  // row of an empty list entry: behind every row (n_db <= 2^31 - 1)
constexpr int kFsMaxK = 32;
constexpr int kFsMaxDy = 64;
constexpr int kFsThreads = 256;
constexpr int kFsChunk = 256;  // frames per piece of the walk back
constexpr int kFsPre = 2 * kFsMaxK / (kFsThreads / 64);  // 16 rows of the gather per wave, one column per lane
constexpr int kFsPairs = (kFsMaxK * kFsMaxK + kFsThreads - 1) / kFsThreads;     // 4 chains per thread
static_assert(kKnnTileQ == 64 && kKnnTileR == 64 && kKnnThreads == 256, "the 4 x 4 blocks of 16 x 16 threads");
static_assert(2 * kKnnStrip <= kKnnTileR, "the key tile lies over both strips");

// (key, row) of a is in front of (key, row) of b; keys are never NaN here
__device__ __forceinline__ bool knn_less(double ka, int ia, double kb, int ib) { return ka < kb || (ka == kb && ia < ib); }

// Offer (key, row) to column `col` of a sorted list kept as [K][64] in LDS; (tk, ti) is the list's last entry, kept in
// registers.  K compare-selects from the end: entry j becomes the old entry j - 1 where the candidate is in front of that,
// else the candidate where it is in front of the old entry j.
__device__ __forceinline__ void knn_offer(const wh::ckp<double>& lk, const wh::ckp<int>& li, int K, int col, double key, int row,
                                          double& tk, int& ti) {
  if (!knn_less(key, row, tk, ti)) return;
  double ck = tk;  // the old entry j
  int ci = ti;
  for (int j = K - 1; j >= 1; --j) {
    const double pk = lk[(j - 1) * 64 + col];
    const int pi = li[(j - 1) * 64 + col];
    const bool before_prev = knn_less(key, row, pk, pi), before_cur = knn_less(key, row, ck, ci);
    lk[j * 64 + col] = before_prev ? pk : (before_cur ? key : ck);
    li[j * 64 + col] = before_prev ? pi : (before_cur ? row : ci);
    ck = pk, ci = pi;
  }
  const bool before_cur = knn_less(key, row, ck, ci);
  lk[col] = before_cur ? key : ck;
  li[col] = before_cur ? row : ci;
  tk = lk[(K - 1) * 64 + col];
  ti = li[(K - 1) * 64 + col];
}

__global__ __launch_bounds__(kKnnThreads) void knn_tile_kernel(const double* __restrict__ q_, long long n_q, long long ldq,
                                                               const double* __restrict__ db_, long long n_db, long long lddb,
                                                               int d, int K, const int32_t* __restrict__ excl_lo_,
                                                               const int32_t* __restrict__ excl_hi_, long long per,
                                                               int32_t* __restrict__ out_idx_, double* __restrict__ out_key_) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ __attribute__((aligned(16))) double s_buf_[kKnnTileR * kKnnLd];
  // (wh::ckp<T> is T* in every shipped build; the bounds build checks each access against the range named here)
  const wh::ckp<double> sq = wh::ck_make(s_buf_, kKnnStrip * kKnnLd, wh::WH_CK_LDS_MAIN);
  const wh::ckp<double> sdb = wh::ck_make(s_buf_ + kKnnStrip * kKnnLd, kKnnStrip * kKnnLd, wh::WH_CK_LDS_AUX);
  const wh::ckp<double> tile = wh::ck_make(s_buf_, kKnnTileR * kKnnLd, wh::WH_CK_LDS_OTHER);  // [row][query], over the strips
  const wh::ckp<double> lk = wh::ck_make(reinterpret_cast<double*>(smem), K * 64, wh::WH_CK_LDS_SCRATCH);
  const wh::ckp<int> li = wh::ck_make(reinterpret_cast<int*>(smem + sizeof(double) * K * 64), K * 64, wh::WH_CK_LDS_SCRATCH);
  const wh::ckp<const double> q = wh::ck_make(q_, (n_q - 1) * ldq + d, wh::WH_CK_IN);
  const wh::ckp<const double> db = wh::ck_make(db_, n_db > 0 ? (n_db - 1) * lddb + d : 0, wh::WH_CK_IN);
  const wh::ckp<const int32_t> excl_lo = wh::ck_make(excl_lo_, excl_lo_ ? n_q : 0, wh::WH_CK_TABLE);
  const wh::ckp<const int32_t> excl_hi = wh::ck_make(excl_hi_, excl_hi_ ? n_q : 0, wh::WH_CK_TABLE);
  const long long n_out = (long long)gridDim.y * n_q * K;
  const wh::ckp<int32_t> out_idx = wh::ck_make(out_idx_, n_out, wh::WH_CK_OUT);
  const wh::ckp<double> out_key = wh::ck_make(out_key_, n_out, wh::WH_CK_OUT);
  const double inf = __builtin_inf();
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const long long q0 = (long long)blockIdx.x * kKnnTileQ;
  const long long r_lo = (long long)blockIdx.y * per, r_hi = r_lo + per < n_db ? r_lo + per : n_db;
  for (int e = tid; e < K * 64; e += kKnnThreads) {
    lk[e] = inf;
    li[e] = kKnnEmpty;
  }
  // the scanning lane's query: its exclusion range and the last entry of its list
  const bool active = tid < kKnnTileQ && q0 + tid < n_q;
  long long ex_lo = 0, ex_hi = 0;
  if (active && excl_lo_) {
    ex_lo = excl_lo[q0 + tid];
    ex_hi = excl_hi[q0 + tid];
  }
  double tk = inf;
  int ti = kKnnEmpty;
  const int lrow = tid >> 2, lcol = (tid & 3) * 4;  // the loader: four consecutive columns of one row
  const long long qrow = q0 + lrow;
  for (long long r0 = r_lo; r0 < r_hi; r0 += kKnnTileR) {
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    const long long drow = r0 + lrow;
    for (int c0 = 0; c0 < d; c0 += kKnnStrip) {
      double vq[4], vd[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = c0 + lcol + i;
        vq[i] = (qrow < n_q && c < d) ? q[qrow * ldq + c] : 0.0;
        vd[i] = (drow < r_hi && c < d) ? db[drow * lddb + c] : 0.0;
      }
      __syncthreads();  // (the strip before, or the key tile, has been read)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sq[(lcol + i) * kKnnLd + lrow] = vq[i];
        sdb[(lcol + i) * kKnnLd + lrow] = vd[i];
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < kKnnStrip; ++c) {
        double a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[i] = sq[c * kKnnLd + ty * 4 + i];
          b[i] = sdb[c * kKnnLd + tx * 4 + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double e = a[i] - b[j];
            acc[i][j] = acc[i][j] + e * e;
          }
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double s = acc[i][j];
        tile[(tx * 4 + j) * kKnnLd + ty * 4 + i] = s != s ? inf : s;
      }
    __syncthreads();
    if (tid < kKnnTileQ) {
      for (int r = 0; r < kKnnTileR; ++r) {
        const long long rg = r0 + r;
        const double key = tile[r * kKnnLd + tid];
        if (active && rg < r_hi && !(rg >= ex_lo && rg < ex_hi)) knn_offer(lk, li, K, tid, key, (int)rg, tk, ti);
      }
    }
  }
  __syncthreads();
  if (active) {
    const long long o = ((long long)blockIdx.y * n_q + q0 + tid) * K;
    for (int k = 0; k < K; ++k) {
      const int i = li[k * 64 + tid];
      out_idx[o + k] = i == kKnnEmpty ? -1 : i;
      out_key[o + k] = lk[k * 64 + tid];
    }
  }
}

__global__ __launch_bounds__(64) void knn_merge_kernel(const int32_t* __restrict__ part_idx_, const double* __restrict__ part_key_,
                                                       long long n_q, int K, int splits, int32_t* __restrict__ idx_,
                                                       double* __restrict__ dist_) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const wh::ckp<double> lk = wh::ck_make(reinterpret_cast<double*>(smem), K * 64, wh::WH_CK_LDS_SCRATCH);
  const wh::ckp<int> li = wh::ck_make(reinterpret_cast<int*>(smem + sizeof(double) * K * 64), K * 64, wh::WH_CK_LDS_SCRATCH);
  const wh::ckp<const int32_t> part_idx = wh::ck_make(part_idx_, (long long)splits * n_q * K, wh::WH_CK_IN);
  const wh::ckp<const double> part_key = wh::ck_make(part_key_, (long long)splits * n_q * K, wh::WH_CK_IN);
  const wh::ckp<int32_t> idx = wh::ck_make(idx_, n_q * K, wh::WH_CK_OUT);
  const wh::ckp<double> dist = wh::ck_make(dist_, n_q * K, wh::WH_CK_OUT);
  const int tid = threadIdx.x;
  const long long n = (long long)blockIdx.x * 64 + tid;
  for (int k = 0; k < K; ++k) {  // (a thread's own column: no barrier)
    lk[k * 64 + tid] = __builtin_inf();
    li[k * 64 + tid] = kKnnEmpty;
  }
  if (n >= n_q) return;
  double tk = __builtin_inf();
  int ti = kKnnEmpty;
  for (int s = 0; s < splits; ++s) {
    const long long o = ((long long)s * n_q + n) * K;
    for (int k = 0; k < K; ++k) {
      const int i = part_idx[o + k];
      const double key = part_key[o + k];
      if (i >= 0) knn_offer(lk, li, K, tid, key, i, tk, ti);
    }
  }
  for (int k = 0; k < K; ++k) {
    const int i = li[k * 64 + tid];
    idx[n * K + k] = i == kKnnEmpty ? -1 : i;
    dist[n * K + k] = lk[k * 64 + tid];
  }
}

// src[f][k] = the y row of slot k of frame f, src[f][K + k] = the y row of its successor; -1 where the slot's index or the
// successor is outside [0, n_db)
__global__ __launch_bounds__(256) void frame_sources_kernel(const int32_t* __restrict__ idx_, long long n_slots, int K,
                                                            long long n_db, const int32_t* __restrict__ succ_,
                                                            int32_t* __restrict__ src_) {
  const wh::ckp<const int32_t> idx = wh::ck_make(idx_, n_slots, wh::WH_CK_IN);
  const wh::ckp<const int32_t> succ = wh::ck_make(succ_, n_db, wh::WH_CK_TABLE);
  const wh::ckp<int32_t> src = wh::ck_make(src_, 2 * n_slots, wh::WH_CK_OUT);
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_slots) return;
  const long long f = e / K;
  const int k = (int)(e - f * K);
  const long long i = idx[e];
  const bool ok = i >= 0 && i < n_db;
  long long s = -1;
  if (ok) s = succ[i];
  src[f * 2 * K + k] = ok ? (int32_t)i : -1;
  src[f * 2 * K + K + k] = (ok && s >= 0 && s < n_db) ? (int32_t)s : -1;
}

__global__ __launch_bounds__(kFsThreads) void frame_select_kernel(const int64_t* __restrict__ frame_off_, int n_utt,
                                                                  long long total_frames, const int32_t* __restrict__ idx_,
                                                                  const double* __restrict__ tc_, int K,
                                                                  const double* __restrict__ y_, long long n_db, long long ldy,
                                                                  int dy, double weight, const int32_t* __restrict__ src_,
                                                                  uint8_t* __restrict__ bp_, int32_t* __restrict__ sel_,
                                                                  int32_t* __restrict__ slot_, double* __restrict__ total_,
                                                                  double* __restrict__ acc_) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int s_ks_[1];
  const int dyp = dy | 1;                  // (an odd row stride: the lanes' rows on different banks)
  const int buf = 2 * K * dyp;             // one frame's rows: K of its slots, K of their successors
  double* const base = reinterpret_cast<double*>(smem);
  const wh::ckp<double> rows = wh::ck_make(base, 2 * buf, wh::WH_CK_LDS_MAIN);
  const wh::ckp<double> V = wh::ck_make(base + 2 * buf, K * K, wh::WH_CK_LDS_AUX);
  const wh::ckp<double> A = wh::ck_make(base + 2 * buf + K * K, 2 * K, wh::WH_CK_LDS_SCRATCH);
  int* const ibase = reinterpret_cast<int*>(base + 2 * buf + K * K + 2 * K);
  const wh::ckp<int> ok = wh::ck_make(ibase, 4 * K, wh::WH_CK_LDS_OTHER);  // [buffer][2 K]: the row was gathered
  const wh::ckp<int> s_src = wh::ck_make(ibase + 4 * K, 4 * K, wh::WH_CK_LDS_OTHER);  // [frame parity][2 K]: the rows to gather
  const wh::ckp<int> s_slot = wh::ck_make(ibase + 8 * K, kFsChunk, wh::WH_CK_LDS_OTHER);
  const wh::ckp<uint8_t> s_bp = wh::ck_make(reinterpret_cast<uint8_t*>(ibase + 8 * K + kFsChunk), kFsChunk * K, wh::WH_CK_LDS_OTHER);
  const wh::ckp<int> s_ks = wh::ck_make(s_ks_, 1, wh::WH_CK_LDS_OTHER);
  const wh::ckp<const int64_t> frame_off = wh::ck_make(frame_off_, (long long)n_utt + 1, wh::WH_CK_TABLE);
  const int u = blockIdx.x, tid = threadIdx.x;
  const long long F0 = frame_off[u], F = frame_off[u + 1] - F0;
  const wh::ckp<double> total = wh::ck_make(total_, n_utt, wh::WH_CK_OUT);
  if (F <= 0) {  // (uniform over the workgroup)
    if (tid == 0) total[u] = 0.0;
    return;
  }
  const wh::ckp<const int32_t> idx = wh::ck_make(idx_ + F0 * K, F * K, wh::WH_CK_IN);
  const wh::ckp<const double> tc = wh::ck_make(tc_ + F0 * K, F * K, wh::WH_CK_IN);
  const wh::ckp<const int32_t> src = wh::ck_make(src_ + F0 * 2 * K, F * 2 * K, wh::WH_CK_IN);
  const wh::ckp<const double> y = wh::ck_make(y_, n_db > 0 ? (n_db - 1) * ldy + dy : 0, wh::WH_CK_IN);
  const wh::ckp<uint8_t> bp = wh::ck_make(bp_ + F0 * K, F * K, wh::WH_CK_OUT);
  const wh::ckp<int32_t> sel = wh::ck_make(sel_ + F0, F, wh::WH_CK_OUT);
  const wh::ckp<int32_t> slot = wh::ck_make(slot_ ? slot_ + F0 : slot_, slot_ ? F : 0, wh::WH_CK_OUT);
  const wh::ckp<double> acc = wh::ck_make(acc_ ? acc_ + F0 * K : acc_, acc_ ? F * K : 0, wh::WH_CK_OUT);
  const double inf = __builtin_inf();
  const int KK = K * K;
  // this thread's chains (j, k), fixed over the frames; of a frame's gather it takes column tid % 64 of the rows
  // tid / 64 + 4 e (a wave reads one row's consecutive columns)
  int pj[kFsPairs], pk[kFsPairs];
#pragma unroll
  for (int e = 0; e < kFsPairs; ++e) {
    const int p = tid + kFsThreads * e;
    pj[e] = p < KK ? p / K : -1;
    pk[e] = p < KK ? p - pj[e] * K : 0;
  }
  const int pcol = tid & 63, prow0 = tid >> 6;
  double pre[kFsPre];
  int pre_ok = 0;
  auto gather = [&](int sb) {  // the rows that s_src's half sb names, into registers
#pragma unroll
    for (int e = 0; e < kFsPre; ++e) {
      const int r = min(prow0 + 4 * e, 2 * K - 1);  // (behind the last row: that row again, the same value to the same place)
      pre[e] = 0.0;
      if (pcol < dy) {
        const long long s = s_src[sb * 2 * K + r];
        if (s >= 0) pre[e] = y[s * ldy + pcol];
      }
    }
    if (tid < 2 * K) pre_ok = s_src[sb * 2 * K + tid] >= 0;
  };
  auto stage = [&](int b) {  // ... and from there into buffer b
#pragma unroll
    for (int e = 0; e < kFsPre; ++e) {
      const int r = min(prow0 + 4 * e, 2 * K - 1);
      if (pcol < dy) rows[b * buf + r * dyp + pcol] = pre[e];
    }
    if (tid < 2 * K) ok[b * 2 * K + tid] = pre_ok;
  };
  // The row indices are fetched two frames ahead and wait in LDS, the rows themselves one frame ahead: a frame's gather
  // is then ONE global load deep, issued in front of the chains of the frame before.
  if (tid < 2 * K) {
    s_src[tid] = src[tid];
    if (F > 1) s_src[2 * K + tid] = src[2 * K + tid];
  }
  __syncthreads();
#pragma unroll 1
  for (int t = 0; t < 2 && t < F; ++t) {  // (frames 0 and 1 have nothing in flight yet)
    gather(t);
    stage(t);
  }
  __syncthreads();
  if (tid < 2 * K && F > 2) s_src[tid] = src[2 * 2 * K + tid];
  double tcn = (tid < K && F > 1) ? tc[K + tid] : 0.0;  // tc of the next frame, one frame ahead as well
  if (tid < K) {
    const double a = ok[tid] ? tc[tid] : inf;
    A[tid] = a;
    bp[tid] = 0;
    if (acc_) acc[tid] = a;
  }
  __syncthreads();
#pragma unroll 1
  for (long long t = 1; t < F; ++t) {
    const int b = (int)(t & 1), bo = b ^ 1;
    if (t + 1 < F) gather(bo);
    const double tcv = tcn;
    int nsrc = -1;
    if (tid < 2 * K && t + 2 < F) nsrc = src[(t + 2) * 2 * K + tid];
    if (tid < K && t + 1 < F) tcn = tc[(t + 1) * K + tid];
#pragma unroll
    for (int e = 0; e < kFsPairs; ++e) {
      if (pj[e] >= 0) {
        const int j = pj[e], k = pk[e];
        double v = inf;
        if (ok[b * 2 * K + k] && ok[bo * 2 * K + K + j]) {
          double cc = 0.0;
          for (int c = 0; c < dy; ++c) {
            const double df = rows[b * buf + k * dyp + c] - rows[bo * buf + (K + j) * dyp + c];
            cc = cc + df * df;
          }
          v = A[bo * K + j] + weight * cc;
        }
        V[j * K + k] = v;
      }
    }
    __syncthreads();
    if (tid < K) {
      double best = V[tid];
      int bj = 0;
      for (int j = 1; j < K; ++j) {
        const double v = V[j * K + tid];
        if (v < best) best = v, bj = j;
      }
      const bool valid = ok[b * 2 * K + tid] != 0;
      const double a = valid ? tcv + best : inf;
      A[b * K + tid] = a;
      bp[t * K + tid] = (uint8_t)(valid ? bj : 0);
      if (acc_) acc[t * K + tid] = a;
    }
    if (t + 1 < F) stage(bo);  // (frame t - 1's rows have been read: the barrier above)
    if (tid < 2 * K) s_src[b * 2 * K + tid] = nsrc;  // (frame t + 2's; frame t's indices were read a frame ago)
    __syncthreads();
  }
  // the end: the smallest k whose accumulated cost is strictly smallest
  if (tid == 0) {
    const int b = (int)((F - 1) & 1);
    double best = A[b * K];
    int kb = 0;
    for (int k = 1; k < K; ++k) {
      const double a = A[b * K + k];
      if (a < best) best = a, kb = k;
    }
    total[u] = best;
    s_ks[0] = kb;
  }
  // the walk back, kFsChunk frames at a time: the piece's back-pointers into LDS, one thread walks, all write
  for (long long f1 = F; f1 > 0; f1 -= kFsChunk) {
    const long long f0 = f1 > kFsChunk ? f1 - kFsChunk : 0;
    const int nf = (int)(f1 - f0);
    __syncthreads();  // (the back-pointers of this workgroup's own threads, and the piece before has been written out)
    for (int e = tid; e < nf * K; e += kFsThreads) s_bp[e] = bp[f0 * K + e];
    __syncthreads();
    if (tid == 0) {
      int ks = s_ks[0];
      for (int f = nf - 1; f >= 0; --f) {
        s_slot[f] = ks;
        ks = s_bp[f * K + ks];  // (frame 0 holds zeros; what it gives is not used)
      }
      s_ks[0] = ks;
    }
    __syncthreads();
    for (int f = tid; f < nf; f += kFsThreads) {
      const int ks = s_slot[f];
      sel[f0 + f] = idx[(f0 + f) * K + ks];
      if (slot_) slot[f0 + f] = ks;
    }
  }
}

size_t fs_lds_bytes(int K, int dy) {
  const size_t doubles = (size_t)2 * 2 * K * (dy | 1) + (size_t)K * K + 2 * K;
  return doubles * sizeof(double) + sizeof(int) * (size_t)(8 * K + kFsChunk) + (size_t)kFsChunk * K;
}

}  // namespace

extern "C" int wh_knn(wh_ctx* ctx, void* stream, const double* q, int64_t n_q, int64_t ldq, const double* db, int64_t n_db,
                      int64_t lddb, int d, int K, const int32_t* excl_lo, const int32_t* excl_hi, int splits, int32_t* idx,
                      double* dist) {
  const char* where = "wh_knn";
  if (!ctx) return wh::fail_msg(where, "null argument");
  WH_ENTER(ctx);
  if (d < 1 || d > kKnnMaxD) return wh::fail_msg(where, "d must be in [1, 160]");
  if (K < 1 || K > kKnnMaxK) return wh::fail_msg(where, "K must be in [1, 32]");
  if (n_q < 0 || n_db < 0) return wh::fail_msg(where, "negative row count");
  if (n_db > 0x7fffffffLL) return wh::fail_msg(where, "at most 2^31 - 1 database rows");
  if (ldq < d || lddb < d) return wh::fail_msg(where, "row strides must be at least d");
  if ((excl_lo == nullptr) != (excl_hi == nullptr)) return wh::fail_msg(where, "excl_lo and excl_hi come together");
  if (splits < 0 || splits > 65535) return wh::fail_msg(where, "splits must be in [0, 65535]");
  if (n_q == 0) return 0;
  if (!q || !idx || !dist || (!db && n_db > 0)) return wh::fail_msg(where, "null argument");
  const int64_t q_tiles = (n_q + kKnnTileQ - 1) / kKnnTileQ;
  if (q_tiles > 0x7fffffffLL) return wh::fail_msg(where, "too many queries for one call");
  if (splits == 0) {
    // enough workgroups for four per compute unit, as long as a range keeps eight tiles of rows
    const int64_t want = (1024 + q_tiles - 1) / q_tiles, room = n_db / (8 * kKnnTileR);
    splits = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, room), 65535));
  }
  const int64_t per = (n_db + splits - 1) / splits;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)K * 64 * (sizeof(double) + sizeof(int));
  int32_t* o_idx = idx;
  double* o_key = dist;
  if (splits > 1) {
    wh::Carve carve;
    const auto r_key = carve.take<double>((int64_t)splits * n_q * K);
    const auto r_idx = carve.take<int32_t>((int64_t)splits * n_q * K);
    if (int rc = wh::ws_reserve(ctx, carve)) return rc;
    o_key = r_key.at(ctx->ws);
    o_idx = r_idx.at(ctx->ws);
  }
  WH_LAUNCH(ctx, st, "knn_tile_kernel", knn_tile_kernel, dim3((unsigned)q_tiles, (unsigned)splits), dim3(kKnnThreads), lds, q,
            n_q, ldq, db, n_db, lddb, d, K, excl_lo, excl_hi, per, o_idx, o_key);
  if (splits > 1)
    WH_LAUNCH(ctx, st, "knn_merge_kernel", knn_merge_kernel, dim3((unsigned)q_tiles), dim3(64), lds, o_idx, o_key, n_q, K,
              splits, idx, dist);
  return 0;
}

extern "C" int wh_frame_select(wh_ctx* ctx, void* stream, const wh_batch* b, const int32_t* idx, const double* tc, int K,
                               const double* y, int64_t n_db, int64_t ldy, int dy, const int32_t* succ, double weight,
                               int32_t* sel, int32_t* slot, double* total, double* acc_out) {
  const char* where = "wh_frame_select";
  if (!ctx || !b) return wh::fail_msg(where, "null argument");
  WH_ENTER(ctx);
  if (K < 1 || K > kFsMaxK) return wh::fail_msg(where, "K must be in [1, 32]");
  if (dy < 1 || dy > kFsMaxDy) return wh::fail_msg(where, "dy must be in [1, 64]");
  if (ldy < dy) return wh::fail_msg(where, "the row stride must be at least dy");
  if (n_db < 0 || n_db > 0x7fffffffLL) return wh::fail_msg(where, "the database must have 0 .. 2^31 - 1 rows");
  if (!(weight >= 0.0) || !std::isfinite(weight)) return wh::fail_msg(where, "the weight must be finite and >= 0");
  if (b->n_utt == 0) return 0;
  const int64_t frames = b->total_frames;
  if (!total || (frames > 0 && (!idx || !tc || !sel)) || (frames > 0 && n_db > 0 && (!y || !succ)))
    return wh::fail_msg(where, "null argument");
  hipStream_t st = (hipStream_t)stream;
  wh::Carve carve;
  const auto r_src = carve.take<int32_t>(frames * 2 * K);
  const auto r_bp = carve.take<uint8_t>(frames * K);
  if (int rc = wh::ws_reserve(ctx, carve)) return rc;
  int32_t* src = r_src.at(ctx->ws);
  uint8_t* bp = r_bp.at(ctx->ws);
  const int64_t n_slots = frames * K;
  if ((n_slots + 255) / 256 > 0x7fffffffLL) return wh::fail_msg(where, "too many frames for one call");
  if (n_slots > 0)
    WH_LAUNCH(ctx, st, "frame_sources_kernel", frame_sources_kernel, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, idx,
              n_slots, K, n_db, succ, src);
  const size_t lds = fs_lds_bytes(K, dy);
  if (int rc = wh::allow_lds(frame_select_kernel, lds)) return rc;
  WH_LAUNCH(ctx, st, "frame_select_kernel", frame_select_kernel, dim3((unsigned)b->n_utt), dim3(kFsThreads), lds,
            b->d_frame_off, b->n_utt, frames, idx, tc, K, y, n_db, ldy, dy, weight, src, bp, sel, slot, total, acc_out);
  return 0;
}
