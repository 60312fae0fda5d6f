// The overlap-add ring of a run of pulses (RunState, wh_resp_types.h): what leaves the ring's window goes to the run's row.
// Include after wh_resp_types.h.
#pragma once

namespace {

// Samples [a, b) (1-based, within the ring's current window) are final for this run: to the row, clear the ring.
template <int N>
__device__ __forceinline__ void ring_flush(wh::ckp<double> ring, int64_t a, int64_t b, wh::ckp<double> WH_RESTRICT row, int64_t row_start,
                                           int64_t ny) {
  constexpr int FT = ft_syn(N);
  a = a < 1 ? 1 : a;
  b = b > ny ? ny : b;
  for (int64_t tgt = a + WH_TID; tgt < b; tgt += FT) {
    const int slot = (int)(tgt & (N - 1));
    row[1 + (tgt - row_start)] = ring[slot];
    ring[slot] = 0.0;
  }
}

// The ring's window moves on to the pulse whose first tap is s1: what it leaves behind goes to the row.
template <int N>
__device__ __forceinline__ void ring_advance(wh::ckp<double> ring, RunState& rs, wh::ckp<double> WH_RESTRICT row, int64_t s1, int64_t ny) {
  constexpr int FT = ft_syn(N);
  if (rs.any) {
    const int64_t e = s1 < rs.win_start + N ? s1 : rs.win_start + N;  // the samples the window leaves behind
    ring_flush<N>(ring, rs.win_start, e, row, rs.row_start, ny);
    // (pulses more than N samples apart — f0 below fs / N: the samples between the two windows belong to the row too)
    for (int64_t tgt = rs.win_start + N + WH_TID; tgt < (s1 < ny ? s1 : ny); tgt += FT) row[1 + (tgt - rs.row_start)] = 0.0;
    wh::sync<FT>();
  } else {
    rs.row_start = s1 < 1 ? 1 : s1;
  }
  rs.any = true;
  rs.win_start = s1;
}

}  // namespace
