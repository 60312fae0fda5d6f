// What the D4C units share (wh_d4c.hip and its test hooks in wh_d4c_probe.hip, through wh_d4c_window.h, wh_d4c_select.h
// and wh_d4c_runs.h): the opaque thread index, the two compiler fences, threads and occupancy per transform length, the
// ownership of bins by threads, the per-launch constants, the one definition of each LDS layout and the stage timer.
// Include FIRST: the thread index has to be defined before wh_device.h is read, so this header does the including.
#pragma once
#include <hip/hip_runtime.h>

// The thread index as the FFT / reduction helpers of wh_fft.h / wh_reduce.h see it: an opaque read.  d4c_kernel runs four
// transforms and four windows per frame through the same helpers; with the plain threadIdx.x the compiler recognises
// the per-thread LDS addresses (eight swizzled store addresses and eight load addresses per radix-8 pass), twiddle
// offsets and index-to-double conversions as common subexpressions of all of them, computes them once and parks them
// in registers for the whole kernel (193 VGPRs wanted where four workgroups per CU allow 128).  Re-deriving them per
// use costs a few integer instructions.
// (Several frames per workgroup with the three fences lifted — this one, fresh_table, stage_fence — lost: DESIGN.md §4 round 6.)
// (a copy of its own, returning int: with the unsigned index of wh_tid.h the d4c_kernel instances compile differently)
__device__ __forceinline__ int wh_opaque_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}
#define WH_TID wh_opaque_tid()

#include "wh_host.h"
#include "wh_spectral.h"

// -DWH_D4C_STAGE_TIMER: thread 0 of every workgroup adds the shader-clock cycles between stage boundaries to
// g_d4c_stage[] (read with wh_debug_d4c_stages, tools/d4c_stage_timer.py) — the per-stage latencies quoted in DESIGN.md.
// The counters are per translation unit (static, like the bounds record of wh_device.h): wh_debug_d4c_stages lives in
// wh_d4c.hip and reads the copy d4c_kernel writes, whichever other unit sees this header.
enum D4cStage {  // index into g_d4c_stage[16]: what ENDS at the mark (tools/d4c_stage_timer.py prints them in kernel order)
  kStGateFold = 0,    // gate reduction + power fold
  kStCentroidA = 1,   // centroid frame at +T0/4: window + FFT + fold
  kStCentroidB = 2,   // centroid frame at -T0/4
  kStReplica = 3,     // low-band replica of the centroid
  kStSmooth = 4,      // power replica + the three sliding windows
  kStSelect = 5,      // the bands' rank selection (from the last kStBandPower mark to the end of the band loop)
  kStOutput = 6,      // outputs
  kStWindows = 7,     // start-up + the two stage-1 windows
  kStGateFft = 8,     // fused gate / power FFT
  kStBandPower = 9,   // band: powers read, buffer released
  kStWinWalk = 10,    // (inside every window: set-up + first walk)
  kStWinReduce = 11,  // (inside every window: the reduction)
  kStBandFill = 12,   // band: shaped group delay x Nuttall window -> buffer
  kStBandFft = 13     // band: real FFT + post-pass to powers
};
#ifdef WH_D4C_STAGE_TIMER
static __device__ unsigned long long g_d4c_stage[16];
// (the running time stamp of a workgroup lives in global memory so that device functions can mark stages too)
static __device__ unsigned long long g_d4c_t0[1 << 20];
#define STAGE_TIMER_BEGIN { if (threadIdx.x == 0) g_d4c_t0[blockIdx.x & ((1 << 20) - 1)] = __builtin_readcyclecounter(); }
#define STAGE_MARK(i) { __syncthreads(); if (threadIdx.x == 0) { const unsigned long long _t = __builtin_readcyclecounter(); atomicAdd(&g_d4c_stage[i], _t - g_d4c_t0[blockIdx.x & ((1 << 20) - 1)]); g_d4c_t0[blockIdx.x & ((1 << 20) - 1)] = _t; } }
#else
#define STAGE_TIMER_BEGIN
#define STAGE_MARK(i)
#endif

namespace wh {

// The kernel runs four transforms through the same twiddle table.  Left alone, the compiler recognises the repeated
// read-only loads and address arithmetic, computes them once and keeps them in registers across the whole kernel
// (203 VGPRs); passing the table pointer through an empty asm before each transform makes every instance re-derive
// what it needs from L1/L2-resident data.
__device__ __forceinline__ const double2* fresh_table(const double2* p) {
  asm volatile("" : "+s"(p));
  return p;
}
#if WH_BOUNDS
__device__ __forceinline__ wh::ckp<const double2> fresh_table(wh::ckp<const double2> p) {
  asm volatile("" : "+s"(p.p));
  return p;
}
#endif
// Stage fence for a per-frame scalar: everything a stage derives from the returned value (window phase, sample
// addresses, rotation constants ...) can only be computed after this point, i.e. the compiler cannot start the next
// stage's loads and transcendental set-up underneath the current stage's transform (which it does otherwise, and
// pays for with ~60 VGPRs of values parked across the FFT).
__device__ __forceinline__ double stage_fence(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

// Threads cooperating on one frame: 256 up to N = 2048; 512 at N = 4096 (48 kHz), where the 96 KB of LDS per frame
// leave one workgroup per CU and the thread count is the only occupancy there is.
// At N = 1024 (D4C-Requiem at 16 kHz) 128 threads make N = 8 * FT, the shape of the register-fed windows.
constexpr int kFtD4c = 256;
constexpr int kFtD4c1024 = 128;
constexpr int kFtD4c4096 = 512;  // (1024 threads, staged windows: 62.9 ms at config 5 — 50.8 compiled for 8 waves per SIMD
                                 // with 164 spilled registers — against 31.8: occupancy is what this instance lacks, but
                                 // LDS (66 KB) and registers (111) both stop it at 4 waves)
constexpr int ft_of(int n) { return n >= 8192 ? 2 * kFtD4c : n >= 4096 ? kFtD4c4096 : (n == 1024 ? kFtD4c1024 : kFtD4c); }
// Waves per SIMD the register allocation must leave room for (HIP's second __launch_bounds__ argument is
// MIN_WAVES_PER_EU).  LDS per frame is the 2N-double transform buffer (33 KB at N = 2048: 4 workgroups of 4 waves
// per CU, 66 KB at N = 4096: 2 workgroups of 8 waves), i.e. 4 waves per SIMD either way -> 128 VGPRs.
constexpr int kMinBlk = 4;
constexpr int kMinBlk4096 = 4;
// N = 1024 (D4C-Requiem at 16 kHz), register-fed, two waves per frame: the radix-8 butterflies need the 128-register
// budget; eight workgroups per CU.
constexpr int kMinBlk1024 = 4;
// (N = 8192, 96 kHz material: 131 KB of LDS per frame -> one 512-thread workgroup per CU, 256 registers per thread)
constexpr int minblk_of(int n) { return n >= 8192 ? 1 : n >= 4096 ? kMinBlk4096 : (n == 1024 ? kMinBlk1024 : (n < 1024 ? 5 : kMinBlk)); }
template <int N>
constexpr bool d4c_regfed() { return N == 8 * ft_of(N); }

// Threads per frame of the stand-alone gate kernel: its one transform is real (N/2 complex points), so N/16 threads are
// one radix-8 butterfly each — half of d4c_kernel's count.
constexpr int kFtLoveDiv = 2;
constexpr int ft_love(int n) { return ft_of(n) / kFtLoveDiv < 64 ? 64 : ft_of(n) / kFtLoveDiv; }

// ---- thread-owned runs of bins ---------------------------------------------------------------------------------
// From the first spectrum to the band stage the K = N/2+1 per-bin quantities of a frame (smoothed power, group-delay
// centroid and what the smoothings make of them) live in REGISTERS: thread t owns the bins [t*KR, (t+1)*KR).  LDS then
// holds nothing but the 2N-double transform buffer (32 KB at N = 2048 -> 4 workgroups per CU instead of 3 with the
// two 8 KB per-bin arrays of the first version), and the smoothings (BandWindow, wh_spectral.h) read and write the
// same runs.
template <int N>
struct Runs {
  static constexpr int FT = ft_of(N);
  static constexpr int K = N / 2 + 1;
  static constexpr int KR = (K + FT - 1) / FT;
};

// Quantities of a launch that depend on the sampling rate and the transform length alone, evaluated once on the host
// with the reference's expressions (d4c.py:78-80, 197-199) instead of by every wave of every frame (FP64 divides and
// ceil / floor: ~60 VALU instructions per frame that no lane needs to repeat).
struct D4cLaunchConst {
  int b0, b1, b2;      // love-train band edges: ceil(100 | 4000 | 7900 / (fs / N)) + 1
  int boundary;        // int(N / wlen * 8 + 0.5)
  int centre[8];       // per band: floor(interval * (b + 1) / (fs / N))
};
inline D4cLaunchConst d4c_launch_const(double fs, int n, int wlen, int interval, int nap) {
  D4cLaunchConst c;
  c.b0 = (int)(ceil(100.0 / (fs / n)) + 1);
  c.b1 = (int)(ceil(4000.0 / (fs / n)) + 1);
  c.b2 = (int)(ceil(7900.0 / (fs / n)) + 1);
  c.boundary = (int)((double)n / wlen * 8 + 0.5);
  for (int b = 0; b < 8; ++b) c.centre[b] = b < nap ? (int)floor((double)interval * (b + 1) / (fs / n)) : 0;
  return c;
}

// ---- LDS layouts, in doubles: the kernels carve them, the launchers ask for them -------------------------------------
constexpr int kWinTab = 16;  // doubles per window in the set-up table (wh_d4c_window.h: win_setup fills 13 of them)
// the front of a frame's block: the 2N-double transform buffer (real buffers, mirrored spectra, the selection's work area)
// and 40 doubles of reduction scratch (block_sum5 at 8 waves) — all the test hooks of wh_d4c_probe.hip need
constexpr int d4c_lds_front(int n) { return 2 * n + 40; }
// d4c_kernel: the front, 8 band values (nap <= 8), 4 window tables (gate, power, centroid +, centroid -)
constexpr int d4c_lds_doubles(int n) { return d4c_lds_front(n) + 8 + 4 * kWinTab; }
// love_train_kernel: NLT real samples / the half spectrum (NLT + 2), 48 doubles of reduction scratch, one window table
// (17 KB at 2048: the 66 VGPRs, not LDS, set the occupancy)
constexpr int love_lds_doubles(int nlt) { return nlt + 2 + 48 + kWinTab; }

}  // namespace wh
