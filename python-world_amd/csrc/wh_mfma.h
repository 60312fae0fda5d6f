// The FP64 matrix cores (gfx950, wave64), shared by wh_features.hip, wh_manifold.hip and wh_gmm.hip.  v_mfma_f64_16x16x4_f64:
// a wave multiplies a 16 x 4 slice of A by a 4 x 16 slice of B into a 16 x 16 tile D, four registers per lane.
// Operand layout (measured, tools/ubench/mfma_check.hip): A[i][k] in lane 16k+i, B[k][j] in lane 16k+j,
// D[4r + l/16][l%16] in register r of lane l.  A wave's accumulators are acc[2][NT]: two 16-row tiles by NT 16-column tiles;
// every output element is one accumulation chain over k in ascending 4-steps.
#pragma once
#include "wh_device.h"

namespace wh {

typedef double double4_t __attribute__((ext_vector_type(4)));  // one accumulator tile

// c += a b.  (Through a reference: a RETURNED tile is `noundef` wherever this is inlined, which alone moved the code of
// gmm_rows_kernel<0>.)
__device__ __forceinline__ void mfma_acc(double4_t& c, double a, double b) {
  c = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
// one B operand against the A operands of both row tiles: an A operand feeds NT MFMAs, a B operand two
__device__ __forceinline__ void mfma_pair(double4_t& c0, double4_t& c1, double a0, double a1, double b) {
  mfma_acc(c0, a0, b);
  mfma_acc(c1, a1, b);
}

// The LDS strips of one stage of the pipeline below, for NT column tiles: A as [row][k], B as [k][column]
template <int NT>
struct mfma_strip {
  static constexpr int KS = 16;            // k step staged per pipeline stage: 4 MFMA k-slices
  static constexpr int AS = KS + 1;        // row stride of the A strip in doubles: 16 rows x 4 k land on distinct banks
  static constexpr int BS = 16 * NT + 16;  // row stride of the B strip: k rows 32 banks apart
};

// The double-buffered pipeline over `steps` strips (int or long long).  fetch(st) loads strip st from global memory into
// registers ONE STEP AHEAD, stage(buf) stores those registers to LDS buffer buf, step(st, buf) runs strip st's MFMAs out of
// buffer buf: the matrix pipe waits neither for HBM nor for L2.  One barrier per step.
template <class Index, class Fetch, class Stage, class Step>
__device__ __forceinline__ void mfma_pipeline(Index steps, Fetch fetch, Stage stage, Step step) {
  fetch((Index)0);
  stage(0);
  __syncthreads();
  for (Index st = 0; st < steps; ++st) {
    const int buf = (int)(st & 1);
    if (st + 1 < steps) fetch(st + 1);  // in flight under this step's MFMAs
    step(st, buf);
    if (st + 1 < steps) stage(buf ^ 1);  // the other buffer was last read a step ago, before the barrier below
    __syncthreads();
  }
}

}  // namespace wh
