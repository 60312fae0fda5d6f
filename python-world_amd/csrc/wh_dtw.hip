// Frame alignment of parallel utterances: batched dynamic time warping over feature rows (mel-cepstra), the step in
// front of every voice-conversion mapping between two speakers' recordings of the same sentences and of the aligned
// mel-cepstral distortion.  The arithmetic is a contract (include/world_hip.h; tests/_dtw_reference.py
// is the same contract in NumPy and the results agree bit for bit): the local cost is a sequential unfused sum and a
// correctly rounded sqrt, the predecessor is chosen diagonal, then (i-1,j), then (i,j-1) by strict <.
//
// dtw_recurrence_kernel: one wave per pair.  The rows of `a` are cut into strips of kDtwStripRows; a lane owns
// kDtwRowsPerLane consecutive rows and keeps them in registers (2 DP VGPRs each, DP = d rounded up to 8: the zero
// columns add +0.0 to a non-negative sum and change nothing).  The lanes run skewed: at step t lane l is at column
// t - l, so D(i-1, .) of a lane's first row is what the lane below it computed one step earlier (one wave shift per
// step), and the two rows of a lane are two independent add chains.  The rows of `b` are staged through a ring in LDS,
// kDtwChunkCols at a time — the skew keeps 64 of them live per wave; the row stride DP + 2 doubles puts the 16-byte
// reads of 16 consecutive lanes on 16 different slots of the bank row (an odd multiple of 16 bytes).  A strip's last row
// goes to the next strip through a line buffer in global memory, in place: a strip writes column t - 63 and has read
// everything up to t.  Under a band a (strip, chunk) rectangle that lies outside it is not computed.
// Back-pointers: two bits per cell, 16 cells per word, rows padded to whole words; a lane fills a word in a register
// and stores it once.
// dtw_backtrack_kernel: one thread per pair walks the back-pointers and writes the path in walking order and both frame
// maps; dtw_reverse_kernel turns every path round and adds the frame offsets.  No atomics anywhere: a pair's result
// does not depend on the batch around it.
#include <math.h>

#include "wh_device.h"
#include "wh_host.h"

namespace {

// (world/align.py exports the same three numbers to the tests: tests/test_align_host.py compares them with this file)
constexpr int kDtwRowsPerLane = 2;
constexpr int kDtwStripRows = WH_WAVE * kDtwRowsPerLane;
constexpr int kDtwChunkCols = 32;
constexpr int kDtwRing = 96;  // staged rows alive: the chunk and the 63 columns the skew still needs, + 1
static_assert(kDtwRing >= kDtwChunkCols + WH_WAVE - 1 && kDtwChunkCols < WH_WAVE, "ring / in-place line buffer");
constexpr int kDtwPairWords = 8;  // per pair: a0, b0, N, M, back-pointer word offset, line offset, path offset, acc offset

struct DtwPair {
  long long a0, b0, n, m, bp, line, path, acc;
};

__device__ __forceinline__ DtwPair dtw_pair(const wh::ckp<const int64_t>& pairs, long long u) {
  DtwPair p;
  p.a0 = pairs[u * kDtwPairWords + 0];
  p.b0 = pairs[u * kDtwPairWords + 1];
  p.n = pairs[u * kDtwPairWords + 2];
  p.m = pairs[u * kDtwPairWords + 3];
  p.bp = pairs[u * kDtwPairWords + 4];
  p.line = pairs[u * kDtwPairWords + 5];
  p.path = pairs[u * kDtwPairWords + 6];
  p.acc = pairs[u * kDtwPairWords + 7];
  return p;
}

// best of the three predecessors in the contract's order; code 0 diagonal, 1 (i-1,j), 2 (i,j-1)
__device__ __forceinline__ double dtw_best(double diag, double up, double left, int& code) {
  double best = diag;
  code = 0;
  if (up < best) {
    best = up;
    code = 1;
  }
  if (left < best) {
    best = left;
    code = 2;
  }
  return best;
}

template <int DP>
__global__ __launch_bounds__(WH_WAVE) void dtw_recurrence_kernel(const int64_t* __restrict__ pairs_, int n_pairs,
                                                                 const double* __restrict__ xa_, long long lda,
                                                                 long long len_a, const double* __restrict__ xb_,
                                                                 long long ldb, long long len_b, int d, long long radius,
                                                                 uint32_t* bp_, long long bp_words, double* line_,
                                                                 long long line_len, double* __restrict__ total_,
                                                                 double* __restrict__ acc_, long long acc_len) {
  constexpr int C = kDtwChunkCols, RING = kDtwRing, LD = DP + 2;
  __shared__ __attribute__((aligned(16))) double s_b[RING * LD];
  __shared__ double s_top[C];
  const wh::ckp<double> sb = wh::ck_make(s_b, RING * LD, wh::WH_CK_LDS_MAIN);
  const wh::ckp<double> top = wh::ck_make(s_top, C, wh::WH_CK_LDS_AUX);
  const wh::ckp<const int64_t> pairs = wh::ck_make(pairs_, (long long)n_pairs * kDtwPairWords, wh::WH_CK_TABLE);
  const int lane = threadIdx.x;
  const long long u = blockIdx.x;
  const DtwPair pr = dtw_pair(pairs, u);
  const long long N = pr.n, M = pr.m;
  const long long rw = (M + 15) >> 4;  // back-pointer words per row
  const wh::ckp<const double> xa = wh::ck_sub(wh::ck_make(xa_, len_a, wh::WH_CK_IN), pr.a0 * lda, (N - 1) * lda + d, wh::WH_CK_IN);
  const wh::ckp<const double> xb = wh::ck_sub(wh::ck_make(xb_, len_b, wh::WH_CK_IN), pr.b0 * ldb, (M - 1) * ldb + d, wh::WH_CK_IN);
  const wh::ckp<uint32_t> bp = wh::ck_sub(wh::ck_make(bp_, bp_words, wh::WH_CK_OUT), pr.bp, N * rw, wh::WH_CK_OUT);
  const wh::ckp<double> line = wh::ck_sub(wh::ck_make(line_, line_len, wh::WH_CK_LDS_SCRATCH), pr.line, M, wh::WH_CK_LDS_SCRATCH);
  const wh::ckp<double> total = wh::ck_make(total_, n_pairs, wh::WH_CK_OUT);
  const wh::ckp<double> acc = wh::ck_sub(wh::ck_make(acc_, acc_len, wh::WH_CK_OUT), acc_ ? pr.acc : 0, acc_ ? N * M : 0, wh::WH_CK_OUT);
  const double inf = __builtin_inf();
  const long long mx = (N > M ? N : M) - 1;
  const bool banded = radius > 0 && radius < mx;  // (radius >= max(N-1, M-1): every cell is inside)
  const long long lim = banded ? radius * mx : 0;
  const long long n_chunks = (M + WH_WAVE - 1 + C - 1) / C;  // steps t = 0 .. M + 62

  for (long long i0 = 0; i0 < N; i0 += kDtwStripRows) {
    const long long r0 = i0 + 2 * lane, r1 = r0 + 1;
    const bool has_next = i0 + kDtwStripRows < N;
    double a_0[DP], a_1[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      a_0[k] = (k < d && r0 < N) ? xa[r0 * lda + k] : 0.0;
      a_1[k] = (k < d && r1 < N) ? xa[r1 * lda + k] : 0.0;
    }
    double d0p = inf, d1p = inf, upp = inf;  // D(r0, j-1), D(r1, j-1), D(r0-1, j-1)
    uint32_t w0 = 0, w1 = 0;                 // the back-pointer words being filled
    for (long long c = 0; c < n_chunks; ++c) {
      const long long t0 = c * C;
      wh::sync<WH_WAVE>();  // (the slots overwritten here were last read 64 steps ago)
      for (int e = lane; e < C * DP; e += WH_WAVE) {
        const int rr = e / DP, k = e - rr * DP;
        const long long j = t0 + rr;
        sb[(int)(j % RING) * LD + k] = (j < M && k < d) ? xb[j * ldb + k] : 0.0;
      }
      if (i0 > 0 && lane < C) top[lane] = t0 + lane < M ? line[t0 + lane] : inf;
      wh::sync<WH_WAVE>();
      bool skip = false;
      if (banded) {  // the rectangle of cells this chunk computes: outside the band iff it lies wholly on one side
        const long long ra = i0, rb = (i0 + kDtwStripRows < N ? i0 + kDtwStripRows : N) - 1;
        const long long ja = t0 - (WH_WAVE - 1) > 0 ? t0 - (WH_WAVE - 1) : 0, jb = t0 + C - 1 < M - 1 ? t0 + C - 1 : M - 1;
        const long long vmax = jb * (N - 1) - ra * (M - 1), vmin = ja * (N - 1) - rb * (M - 1);
        skip = vmin > lim || vmax < -lim;
      }
      if (skip) {
        const long long jp = t0 - 1 - lane;  // a word left unfinished by the chunk before
        if (jp >= 0 && jp < M - 1 && (jp & 15) != 15) {
          if (r0 < N) bp[r0 * rw + (jp >> 4)] = w0;
          if (r1 < N) bp[r1 * rw + (jp >> 4)] = w1;
        }
        w0 = w1 = 0;
        d0p = d1p = upp = inf;
        if (has_next && lane < C) {
          const long long jj = t0 - (WH_WAVE - 1) + lane;
          if (jj >= 0 && jj < M) line[jj] = inf;
        }
        if (acc_) {
          for (int ts = 0; ts < C; ++ts) {
            const long long j = t0 + ts - lane;
            if (j >= 0 && j < M) {
              if (r0 < N) acc[r0 * M + j] = inf;
              if (r1 < N) acc[r1 * M + j] = inf;
            }
          }
        }
        continue;
      }
      int slot = (int)(((t0 - lane) % RING + RING) % RING);
      long long v0 = (t0 - lane) * (N - 1) - r0 * (M - 1);  // j (N-1) - i (M-1) of (r0, j)
      for (int ts = 0; ts < C; ++ts) {
        const long long j = t0 + ts - lane;
        double up = __shfl_up(d1p, 1, WH_WAVE);  // D(r0-1, j): the lane below was at column j one step ago
        if (lane == 0) up = i0 > 0 ? top[ts] : inf;
        if (j >= 0 && j < M) {
          double s0 = 0.0, s1 = 0.0;
#pragma unroll
          for (int k = 0; k < DP; ++k) {
            const double bk = sb[slot * LD + k];
            const double e0 = a_0[k] - bk, e1 = a_1[k] - bk;
            s0 = s0 + e0 * e0;
            s1 = s1 + e1 * e1;
          }
          const double c0 = sqrt(s0), c1 = sqrt(s1);
          const long long v1 = v0 - (M - 1);
          const bool in0 = !banded || (v0 <= lim && v0 >= -lim), in1 = !banded || (v1 <= lim && v1 >= -lim);
          int code0, code1;
          double best0, best1;
          // on row 0 and on column 0 the only predecessor that exists, whatever the values
          if (r0 == 0) {
            best0 = j == 0 ? 0.0 : d0p;
            code0 = 2;
          } else if (j == 0) {
            best0 = up;
            code0 = 1;
          } else {
            best0 = dtw_best(upp, up, d0p, code0);
          }
          double d0 = (r0 == 0 && j == 0) ? c0 : c0 + best0;
          if (!in0) d0 = inf;
          if (j == 0) {
            best1 = d0;
            code1 = 1;
          } else {
            best1 = dtw_best(d0p, d0, d1p, code1);
          }
          double d1 = c1 + best1;
          if (!in1) d1 = inf;
          w0 |= (uint32_t)code0 << (2 * (int)(j & 15));
          w1 |= (uint32_t)code1 << (2 * (int)(j & 15));
          if ((j & 15) == 15 || j == M - 1) {
            if (r0 < N) bp[r0 * rw + (j >> 4)] = w0;
            if (r1 < N) bp[r1 * rw + (j >> 4)] = w1;
            w0 = w1 = 0;
          }
          if (acc_) {
            if (r0 < N) acc[r0 * M + j] = d0;
            if (r1 < N) acc[r1 * M + j] = d1;
          }
          if (j == M - 1) {
            if (r0 == N - 1) total[u] = d0;
            if (r1 == N - 1) total[u] = d1;
          }
          if (has_next && lane == WH_WAVE - 1) line[j] = d1;
          upp = up;
          d0p = d0;
          d1p = d1;
        }
        slot = slot + 1 == RING ? 0 : slot + 1;
        v0 += N - 1;
      }
    }
    wh::sync<WH_WAVE>();  // the line this strip wrote is the next strip's top row
  }
}

__global__ __launch_bounds__(WH_WAVE) void dtw_backtrack_kernel(const int64_t* __restrict__ pairs_, int n_pairs,
                                                                const uint32_t* __restrict__ bp_, long long bp_words,
                                                                int64_t* __restrict__ path_a_, int64_t* __restrict__ path_b_,
                                                                long long path_total, int64_t* __restrict__ path_len_,
                                                                int64_t* __restrict__ map_a2b_, long long frames_a,
                                                                int64_t* __restrict__ map_b2a_, long long frames_b) {
  const wh::ckp<const int64_t> pairs = wh::ck_make(pairs_, (long long)n_pairs * kDtwPairWords, wh::WH_CK_TABLE);
  const long long u = (long long)blockIdx.x * WH_WAVE + threadIdx.x;
  if (u >= n_pairs) return;
  const DtwPair pr = dtw_pair(pairs, u);
  const long long N = pr.n, M = pr.m, rw = (M + 15) >> 4;
  const wh::ckp<const uint32_t> bp = wh::ck_sub(wh::ck_make(bp_, bp_words, wh::WH_CK_IN), pr.bp, N * rw, wh::WH_CK_IN);
  const wh::ckp<int64_t> pa = wh::ck_sub(wh::ck_make(path_a_, path_total, wh::WH_CK_OUT), pr.path, N + M - 1, wh::WH_CK_OUT);
  const wh::ckp<int64_t> pb = wh::ck_sub(wh::ck_make(path_b_, path_total, wh::WH_CK_OUT), pr.path, N + M - 1, wh::WH_CK_OUT);
  const wh::ckp<int64_t> a2b = wh::ck_sub(wh::ck_make(map_a2b_, frames_a, wh::WH_CK_OUT), pr.a0, N, wh::WH_CK_OUT);
  const wh::ckp<int64_t> b2a = wh::ck_sub(wh::ck_make(map_b2a_, frames_b, wh::WH_CK_OUT), pr.b0, M, wh::WH_CK_OUT);
  const wh::ckp<int64_t> path_len = wh::ck_make(path_len_, n_pairs, wh::WH_CK_OUT);
  long long i = N - 1, j = M - 1, p = 0;
  long long i_hi = i, j_hi = j;  // where the walk entered the current column / row: the run's upper end
  for (;;) {
    pa[p] = i;  // walking order and pair-local indices: dtw_reverse_kernel finishes both
    pb[p] = j;
    ++p;
    if (i == 0 && j == 0) break;
    int code;
    if (i == 0) code = 2;
    else if (j == 0) code = 1;
    else code = (int)((bp[i * rw + (j >> 4)] >> (2 * (int)(j & 15))) & 3u);
    const long long ni = code == 2 ? i : i - 1, nj = code == 1 ? j : j - 1;
    if (nj != j) {  // the cells i .. i_hi share column j
      b2a[j] = pr.a0 + ((i + i_hi) >> 1);
      i_hi = ni;
    }
    if (ni != i) {
      a2b[i] = pr.b0 + ((j + j_hi) >> 1);
      j_hi = nj;
    }
    i = ni;
    j = nj;
  }
  b2a[0] = pr.a0 + (i_hi >> 1);
  a2b[0] = pr.b0 + (j_hi >> 1);
  path_len[u] = p;
}

__global__ __launch_bounds__(WH_BLOCK) void dtw_reverse_kernel(const int64_t* __restrict__ pairs_, int n_pairs,
                                                               int64_t* __restrict__ path_a_, int64_t* __restrict__ path_b_,
                                                               long long path_total, const int64_t* __restrict__ path_len_) {
  const wh::ckp<const int64_t> pairs = wh::ck_make(pairs_, (long long)n_pairs * kDtwPairWords, wh::WH_CK_TABLE);
  const long long u = blockIdx.x;
  const DtwPair pr = dtw_pair(pairs, u);
  const wh::ckp<int64_t> pa = wh::ck_sub(wh::ck_make(path_a_, path_total, wh::WH_CK_OUT), pr.path, pr.n + pr.m - 1, wh::WH_CK_OUT);
  const wh::ckp<int64_t> pb = wh::ck_sub(wh::ck_make(path_b_, path_total, wh::WH_CK_OUT), pr.path, pr.n + pr.m - 1, wh::WH_CK_OUT);
  const long long len = wh::ck_make(path_len_, n_pairs, wh::WH_CK_IN)[u];
  for (long long p = threadIdx.x; 2 * p < len; p += WH_BLOCK) {
    const long long q = len - 1 - p;
    const long long ai = pa[p], aq = pa[q], bi = pb[p], bq = pb[q];
    pa[p] = aq + pr.a0;
    pb[p] = bq + pr.b0;
    if (q != p) {
      pa[q] = ai + pr.a0;
      pb[q] = bi + pr.b0;
    }
  }
}

// dtw_recurrence_kernel<DP> by DP / 8 - 1: the feature dimension padded to a multiple of 8
decltype(&dtw_recurrence_kernel<8>) const kDtwRecurrence[8] = {
    dtw_recurrence_kernel<8>,  dtw_recurrence_kernel<16>, dtw_recurrence_kernel<24>, dtw_recurrence_kernel<32>,
    dtw_recurrence_kernel<40>, dtw_recurrence_kernel<48>, dtw_recurrence_kernel<56>, dtw_recurrence_kernel<64>};

}  // namespace

extern "C" int wh_dtw(wh_ctx* ctx, void* stream, const wh_batch* a, const wh_batch* b, const double* xa, int64_t lda,
                      const double* xb, int64_t ldb, int d, int64_t radius, const int64_t* h_path_off, int64_t* path_a,
                      int64_t* path_b, int64_t* path_len, double* total_cost, int64_t* map_a2b, int64_t* map_b2a,
                      double* acc_out, const int64_t* h_acc_off) {
  if (!ctx || !a || !b || !h_path_off) return wh::fail_msg("wh_dtw", "null argument");
  WH_ENTER(ctx);
  if (a->n_utt != b->n_utt) return wh::fail_msg("wh_dtw", "the two batches must hold the same number of utterances");
  if (d < 1 || d > 64) return wh::fail_msg("wh_dtw", "d must be in [1, 64]");
  if (lda < d || ldb < d) return wh::fail_msg("wh_dtw", "row strides must be at least d");
  if (acc_out && !h_acc_off) return wh::fail_msg("wh_dtw", "acc_out needs h_acc_off");
  const int n = a->n_utt;
  std::vector<int64_t> pairs((size_t)n * kDtwPairWords);
  long long line_len = 0, bp_words = 0, acc_len = 0;
  for (int u = 0; u < n; ++u) {
    const int64_t N = a->h_frame_off[u + 1] - a->h_frame_off[u], M = b->h_frame_off[u + 1] - b->h_frame_off[u];
    if (N < 1 || M < 1) return wh::fail_msg("wh_dtw", "an utterance has no frames");
    if (N > 0x7fffffffLL || M > 0x7fffffffLL) return wh::fail_msg("wh_dtw", "an utterance has too many frames");
    if (h_path_off[u] < 0 || h_path_off[u + 1] - h_path_off[u] < N + M - 1)
      return wh::fail_msg("wh_dtw", "h_path_off must leave every pair N + M - 1 entries");
    if (acc_out && (h_acc_off[u] < 0 || h_acc_off[u + 1] - h_acc_off[u] < N * M))
      return wh::fail_msg("wh_dtw", "h_acc_off must leave every pair N * M entries");
    int64_t* p = &pairs[(size_t)u * kDtwPairWords];
    p[0] = a->h_frame_off[u];
    p[1] = b->h_frame_off[u];
    p[2] = N;
    p[3] = M;
    p[4] = bp_words;
    p[5] = line_len;
    p[6] = h_path_off[u];
    p[7] = acc_out ? h_acc_off[u] : 0;
    bp_words += N * ((M + 15) >> 4);
    line_len += M;
    if (acc_out) acc_len = h_acc_off[u + 1];
  }
  if (n == 0) return 0;
  if (!xa || !xb || !path_a || !path_b || !path_len || !total_cost || !map_a2b || !map_b2a)
    return wh::fail_msg("wh_dtw", "null argument");
  hipStream_t st = (hipStream_t)stream;
  int64_t* d_pairs = nullptr;
  if (int rc = wh::persistent_upload(ctx, st, "dtw.pairs", pairs, &d_pairs)) return rc;
  wh::Carve carve;
  const auto r_line = carve.take<double>(line_len);
  const auto r_bp = carve.take<uint32_t>(bp_words);
  if (!carve.ok()) return wh::fail_msg("wh_dtw", "scratch size beyond size_t");
  char* scratch = nullptr;
  if (int rc = wh::persistent_scratch(ctx, "dtw.scratch", carve.end(), &scratch)) return rc;
  double* line = r_line.at(scratch);
  uint32_t* bp = r_bp.at(scratch);
  const long long len_a = (a->total_frames - 1) * lda + d, len_b = (b->total_frames - 1) * ldb + d;
  const long long path_total = h_path_off[n];
  WH_LAUNCH(ctx, st, "dtw_recurrence_kernel", kDtwRecurrence[(d + 7) / 8 - 1], dim3((unsigned)n), dim3(WH_WAVE), 0,
            d_pairs, n, xa, lda, len_a, xb, ldb, len_b, d, radius, bp, bp_words, line, line_len, total_cost, acc_out,
            acc_len);
  WH_LAUNCH(ctx, st, "dtw_backtrack_kernel", dtw_backtrack_kernel, dim3((unsigned)((n + WH_WAVE - 1) / WH_WAVE)),
            dim3(WH_WAVE), 0, d_pairs, n, bp, bp_words, path_a, path_b, path_total, path_len, map_a2b, a->total_frames,
            map_b2a, b->total_frames);
  WH_LAUNCH(ctx, st, "dtw_reverse_kernel", dtw_reverse_kernel, dim3((unsigned)n), dim3(WH_BLOCK), 0, d_pairs, n, path_a,
            path_b, path_total, path_len);
  return 0;
}
