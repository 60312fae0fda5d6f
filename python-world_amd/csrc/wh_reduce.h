// Wave and workgroup reductions (gfx950, wave64): wave_sum on the VALU by DPP, block_sum* = wave sums plus one LDS hop
// across the waves, wave_scan_incl.  The thread index is WH_TID (wh_device.h): a unit that defines it opaquely
// (wh_tid.h, wh_d4c_types.h) does so before this header is read.
#pragma once
#include "wh_device.h"

namespace wh {

// Sum over the 64 lanes of a wave, result in every lane.  DPP form: butterflies inside the rows of 16 lanes by
// quad permutes and row mirrors, then row_bcast:15 / row_bcast:31 carry the row totals up to lane 63, whose value is
// broadcast through the scalar unit — 12 v_mov_dpp + 6 v_add_f64 + 2 v_readlane, all on the VALU.  The shuffle form it
// replaced (six __shfl_xor steps) was 12 ds_bpermute_b32 through the LDS crossbar with a wait in front of every add; the
// window reductions of d4c_kernel run five of these sums four times per frame.  (tools/ubench/wave_sum_check.hip)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_or_zero(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xF, false);  // lanes outside the mask / without a source: 0
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xF, false);
  return __hiloint2double(hi, lo);
}
// a permutation inside the rows of 16 lanes: every lane has a source, so there is no "old" value to prepare (with
// update_dpp(0, ..) each of these steps carried two v_mov_b32 v, 0 in front of its two v_mov_b32_dpp)
template <int CTRL>
__device__ __forceinline__ double dpp_row_perm(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, true);
  hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// the tree without the broadcast: the total in lane 63 only
__device__ __forceinline__ double wave_sum_lane63(double v) {
  v += dpp_row_perm<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_row_perm<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_row_perm<0x141>(v);  // row_half_mirror
  v += dpp_row_perm<0x140>(v);  // row_mirror: every lane holds its row's total
  v += dpp_or_zero<0x142, 0xA>(v);  // row_bcast:15 into rows 1 and 3
  return v + dpp_or_zero<0x143, 0xC>(v);  // row_bcast:31 into rows 2 and 3: lane 63 holds the wave's total
}
__device__ __forceinline__ double wave_sum(double v) {
  v = wave_sum_lane63(v);
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63), hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
  return __hiloint2double(hi, lo);
}

// Sum over the whole 256-thread block; result broadcast to every thread.
// `scratch` must hold >= 3*NT/64 doubles of LDS (24 for the largest block used, 512).  Contains two barriers.
template <int NT = WH_BLOCK>
__device__ __forceinline__ double block_sum(double v, ckp<double> scratch) {
  v = wave_sum(v);
  if constexpr (NT <= WH_WAVE) {
    sync<NT>();
    return v;
  }
  const int w = WH_TID >> 6;
  __syncthreads();
  if ((WH_TID & 63) == 0) scratch[w] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < NT / WH_WAVE; ++i) t += scratch[i];
  return t;
}

// ---- several values through one tree ---------------------------------------------------------------------------------
// wave_sum is a balanced butterfly: lane l adds its partner l^1, then l^2, the other quad of its half row, the other half of
// its row, the other row of its pair, the other half of the wave — every lane of a group holds the same bits, because a + b
// and b + a are the same double.  Reducing K values one after the other repeats all six levels K times although from the
// first level on half of the lanes hold copies.  The packed forms keep, per lane, HALF of the values at level 1 (chosen by
// a lane bit: the lane hands its partner the values it drops and adds the partner's copy of those it keeps) and half
// again at level 2 (K = 4), so that from then on one register pair per lane runs through the remaining levels and every
// quad holds all K totals side by side.  Every node adds the two operands wave_sum adds there, possibly in the other
// order: the totals are wave_sum's bit for bit (tests/test_hip_reduce.py against wave_sum and against a model of the tree).
// The lanes of a quad hold different values, so the levels across rows cannot broadcast one lane (row_bcast): they swap
// rows and halves of a register with a copy of itself (v_permlane16_swap_b32, v_permlane32_swap_b32: one output holds the
// even rows' or lower half's value in every row, the other the odd rows' or upper half's) and add the two.  Every lane
// ends with a total, and no v_readlane is needed.  The lane-bit selects read constant scalar masks.
// Per wave: four values 39 VALU instructions (four wave_sum: 96), two values 26 (48).  (tools/ubench/wave_sum_packed_check.hip)
__device__ __forceinline__ bool lane_bit0() { return __builtin_amdgcn_inverse_ballot_w64(0xAAAAAAAAAAAAAAAAull); }
__device__ __forceinline__ bool lane_bit1() { return __builtin_amdgcn_inverse_ballot_w64(0xCCCCCCCCCCCCCCCCull); }
// every lane: the value of lane ^ 4 (no DPP control swaps the quads of a half row in place — row_half_mirror also
// reverses the lanes inside them —, so: quads 0 and 2 of a row read four lanes up, quads 1 and 3 four lanes down)
__device__ __forceinline__ double dpp_xor4(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  int tlo = __builtin_amdgcn_mov_dpp(lo, 0x104, 0xF, 0x5, false);  // row_shl:4, banks 0 and 2
  int thi = __builtin_amdgcn_mov_dpp(hi, 0x104, 0xF, 0x5, false);
  tlo = __builtin_amdgcn_update_dpp(tlo, lo, 0x114, 0xF, 0xA, false);  // row_shr:4, banks 1 and 3; the others keep theirs
  thi = __builtin_amdgcn_update_dpp(thi, hi, 0x114, 0xF, 0xA, false);
  return __hiloint2double(thi, tlo);
}
// v + (the value of the lane in the other row of the pair | the other half of the wave), in every lane
template <bool HALVES>
__device__ __forceinline__ double add_swapped(double v) {
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  const auto l = HALVES ? __builtin_amdgcn_permlane32_swap(lo, lo, false, false) : __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto h = HALVES ? __builtin_amdgcn_permlane32_swap(hi, hi, false, false) : __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
}
// Two values: the wave's total of a in lanes 0 and 3 of every quad, of b in lanes 1 and 2 (a layout the row mirrors of
// levels 3 and 4 keep).
__device__ __forceinline__ double wave_sum2_packed(double a, double b) {
  const bool inner = lane_bit0() != lane_bit1();
  double v = inner ? b : a;
  v += dpp_row_perm<0xB1>(inner ? a : b);  // quad_perm [1,0,3,2]: the partner's copy of the value this lane keeps
  v += dpp_row_perm<0x1B>(v);   // quad_perm [3,2,1,0]: the other pair of the quad
  v += dpp_row_perm<0x141>(v);  // row_half_mirror
  v += dpp_row_perm<0x140>(v);  // row_mirror
  v = add_swapped<false>(v);
  return add_swapped<true>(v);
}
// Four values: the wave's total of the (lane & 3)-th in every lane.
__device__ __forceinline__ double wave_sum4_packed(double a, double b, double c, double d) {
  const bool odd = lane_bit0(), up = lane_bit1();
  double p = odd ? b : a, q = odd ? d : c;  // even lanes keep (a, c), odd lanes (b, d)
  p += dpp_row_perm<0xB1>(odd ? a : b);
  q += dpp_row_perm<0xB1>(odd ? c : d);
  double v = up ? q : p;  // lanes 0 and 1 of a quad keep a | b, lanes 2 and 3 c | d
  v += dpp_row_perm<0x4E>(up ? p : q);  // quad_perm [2,3,0,1]
  v += dpp_xor4(v);
  v += dpp_row_perm<0x128>(v);  // row_ror:8 = the lane ^ 8 of a row of 16
  v = add_swapped<false>(v);
  return add_swapped<true>(v);
}

// Two sums at once (saves barriers).  The wave totals go from the lanes that hold them straight into scratch[k * NW + w];
// the combine across the waves is block_sum's: ascending from 0.0.
template <int NT = WH_BLOCK>
__device__ __forceinline__ void block_sum2(double& a, double& b, ckp<double> scratch) {
  if constexpr (NT <= WH_WAVE) {
    a = wave_sum(a);
    b = wave_sum(b);
    sync<NT>();
    return;
  } else {
    constexpr int NW = NT / WH_WAVE;
    const double v = wave_sum2_packed(a, b);
    const int w = WH_TID >> 6, lane = WH_TID & 63;
    __syncthreads();
    if (lane < 2) scratch[lane * NW + w] = v;
    __syncthreads();
    double ta = 0.0, tb = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      ta += scratch[i];
      tb += scratch[NW + i];
    }
    a = ta;
    b = tb;
  }
}

// (three values ride the tree of four: its fourth sums zeros)
template <int NT = WH_BLOCK>
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c, ckp<double> scratch) {
  if constexpr (NT <= WH_WAVE) {
    a = wave_sum(a);
    b = wave_sum(b);
    c = wave_sum(c);
    sync<NT>();
    return;
  } else {
    constexpr int NW = NT / WH_WAVE;
    const double v = wave_sum4_packed(a, b, c, 0.0);
    const int w = WH_TID >> 6, lane = WH_TID & 63;
    __syncthreads();
    if (lane < 3) scratch[lane * NW + w] = v;
    __syncthreads();
    double ta = 0.0, tb = 0.0, tc = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      ta += scratch[i];
      tb += scratch[NW + i];
      tc += scratch[2 * NW + i];
    }
    a = ta;
    b = tb;
    c = tc;
  }
}

// Five sums at once (the D4C window: two means and the three second moments of its energy, one pair of barriers): a
// tree of four and a single one.  `scratch` must hold >= 5*NT/64 doubles.
template <int NT = WH_BLOCK>
__device__ __forceinline__ void block_sum5(double& a, double& b, double& c, double& d, double& e, ckp<double> scratch) {
  if constexpr (NT <= WH_WAVE) {
    a = wave_sum(a);
    b = wave_sum(b);
    c = wave_sum(c);
    d = wave_sum(d);
    e = wave_sum(e);
    sync<NT>();
    return;
  } else {
    constexpr int NW = NT / WH_WAVE;
    const double v = wave_sum4_packed(a, b, c, d);
    const double ve = wave_sum_lane63(e);
    const int w = WH_TID >> 6, lane = WH_TID & 63;
    __syncthreads();
    if (lane < 4) scratch[lane * NW + w] = v;
    if (lane == 63) scratch[4 * NW + w] = ve;
    __syncthreads();
    double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < NW; ++i)
#pragma unroll
      for (int k = 0; k < 5; ++k) t[k] += scratch[k * NW + i];
    a = t[0];
    b = t[1];
    c = t[2];
    d = t[3];
    e = t[4];
  }
}

__device__ __forceinline__ double wave_scan_incl(double v) {
  const int lane = WH_TID & 63;
#pragma unroll
  for (int o = 1; o < WH_WAVE; o <<= 1) {
    double u = __shfl_up(v, o, WH_WAVE);
    if (lane >= o) v += u;
  }
  return v;
}

}  // namespace wh
