// The thread index as an opaque value.  A kernel that LOOPS over units around an inlined transform (the overlap-save band
// walker, the response kernels, the Requiem frames) turns every per-thread LDS / twiddle address of the passes into a
// loop invariant when it reads the plain index: LLVM hoists them all and keeps them alive across the loop (the walker:
// ~310 VGPRs against 169).  An opaque read makes each use its own value.  Include BEFORE wh_device.h, wh_reduce.h
// and wh_fft.h: wh_device.h sets the default WH_TID, the helpers of the other two take their index from it.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned wh_opaque_tid() {
  unsigned t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}
#define WH_TID wh_opaque_tid()
