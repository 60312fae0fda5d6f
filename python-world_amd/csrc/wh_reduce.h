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
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_row_perm<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_row_perm<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_row_perm<0x141>(v);  // row_half_mirror
  v += dpp_row_perm<0x140>(v);  // row_mirror: every lane holds its row's total
  v += dpp_or_zero<0x142, 0xA>(v);  // row_bcast:15 into rows 1 and 3
  v += dpp_or_zero<0x143, 0xC>(v);  // row_bcast:31 into rows 2 and 3: lane 63 holds the wave's total
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

// Two sums at once (saves barriers).
template <int NT = WH_BLOCK>
__device__ __forceinline__ void block_sum2(double& a, double& b, ckp<double> scratch) {
  a = wave_sum(a);
  b = wave_sum(b);
  if constexpr (NT <= WH_WAVE) {
    sync<NT>();
    return;
  }
  const int w = WH_TID >> 6;
  __syncthreads();
  if ((WH_TID & 63) == 0) {
    scratch[w] = a;
    scratch[NT / WH_WAVE + w] = b;
  }
  __syncthreads();
  double ta = 0.0, tb = 0.0;
#pragma unroll
  for (int i = 0; i < NT / WH_WAVE; ++i) {
    ta += scratch[i];
    tb += scratch[NT / WH_WAVE + i];
  }
  a = ta;
  b = tb;
}

template <int NT = WH_BLOCK>
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c, ckp<double> scratch) {
  a = wave_sum(a);
  b = wave_sum(b);
  c = wave_sum(c);
  if constexpr (NT <= WH_WAVE) {
    sync<NT>();
    return;
  }
  const int w = WH_TID >> 6;
  __syncthreads();
  if ((WH_TID & 63) == 0) {
    scratch[w] = a;
    scratch[NT / WH_WAVE + w] = b;
    scratch[2 * (NT / WH_WAVE) + w] = c;
  }
  __syncthreads();
  double ta = 0.0, tb = 0.0, tc = 0.0;
#pragma unroll
  for (int i = 0; i < NT / WH_WAVE; ++i) {
    ta += scratch[i];
    tb += scratch[NT / WH_WAVE + i];
    tc += scratch[2 * (NT / WH_WAVE) + i];
  }
  a = ta;
  b = tb;
  c = tc;
}

// Five sums at once (the D4C window: two means and the three second moments of its energy, one pair of barriers).
// `scratch` must hold >= 5*NT/64 doubles.
template <int NT = WH_BLOCK>
__device__ __forceinline__ void block_sum5(double& a, double& b, double& c, double& d, double& e, ckp<double> scratch) {
  a = wave_sum(a);
  b = wave_sum(b);
  c = wave_sum(c);
  d = wave_sum(d);
  e = wave_sum(e);
  if constexpr (NT <= WH_WAVE) {
    sync<NT>();
    return;
  }
  constexpr int NW = NT / WH_WAVE;
  const int w = WH_TID >> 6;
  __syncthreads();
  if ((WH_TID & 63) == 0) {
    scratch[w] = a;
    scratch[NW + w] = b;
    scratch[2 * NW + w] = c;
    scratch[3 * NW + w] = d;
    scratch[4 * NW + w] = e;
  }
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
