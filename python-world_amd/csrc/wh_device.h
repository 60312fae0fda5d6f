// Device-side core shared by every WORLD kernel (gfx950 / CDNA4, wave64): the global-memory accessors, the checked
// pointer of the bounds build, the barriers, the workgroup id -> unit mapping that keeps neighbouring units on one XCD
// (one L2), the blocked fetch of the serial recurrences and the geometry of the context's twiddle tables.
// The wave / workgroup reductions are in wh_reduce.h, the FFT engine in wh_fft.h; both include this header.
//
// All arithmetic is FP64: the reference is float64 end to end and the F0 stages take discrete
// decisions on it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define WH_BLOCK 256
#define WH_WAVE 64
// Thread index as the FFT / reduction helpers see it.  A translation unit whose kernel LOOPS over units may define
// WH_TID as an opaque read of threadIdx.x (see wh_synthesis.hip): the helpers' per-thread addresses then stop being
// loop invariants that the compiler hoists and keeps in registers across the whole loop body.
#ifndef WH_TID
#define WH_TID threadIdx.x
#endif

#define WH_MAX_FFT 8192  // longest in-LDS transform (CheapTrick / synthesis stop at 4096, D4C / love-train / SWIPE' at 8192)
// The twiddle tables go further: StoneMask and the Harvest refinement evaluate a handful of bins of a transform of
// 2^(2 + floor(log2(window))) points directly (stonemask.py:33-35) — no transform is run, only exp(-2 pi i k / n) is
// looked up — and a 3-period window at a low floor and a high rate asks for 16384 or 32768 (96 kHz below 70 Hz, 48 kHz
// below 35 Hz: the fft_size override).  1 MB per context.
#define WH_MAX_TWIDDLE 32768

namespace wh {

// Loads that are known to address global memory, said so to the compiler.  Kernel-argument pointers are inferred as
// global on their own, but not once they have been laundered through an empty asm (fresh_table, stage fences), selected
// at run time, or read out of a by-value argument struct: loads through those compile to flat_load, which ticks BOTH
// the vector-memory and the LDS counter — every s_waitcnt lgkmcnt(0) in front of an LDS read then also waits for the
// twiddle fetch that was issued early precisely to overlap with it.
__device__ __forceinline__ double2 ldg2(const double2* p) {
  typedef double v2d __attribute__((ext_vector_type(2)));
  const v2d v = *(const v2d __attribute__((address_space(1)))*)p;
  return make_double2(v.x, v.y);
}
__device__ __forceinline__ double ldg(const double* p) { return *(const double __attribute__((address_space(1)))*)p; }
#if WH_BOUNDS
template <class T> struct ckp;
__device__ __forceinline__ double2 ldg2(const ckp<const double2>& p);
__device__ __forceinline__ double ldg(const ckp<const double>& p);
#endif
// The same for stores (a pointer read out of a job record is generic to the compiler: flat_store), plain and non-temporal.
__device__ __forceinline__ void stg(double* p, double v) { *(double __attribute__((address_space(1)))*)p = v; }
__device__ __forceinline__ void stg_nt(double* p, double v) {
  __builtin_nontemporal_store(v, (double __attribute__((address_space(1)))*)p);
}

// ------------------------------------------------------------------------------------------
// Checked pointers: the bounds build (-DWH_BOUNDS=1, tools/build_variants.py; never shipped)
// ------------------------------------------------------------------------------------------
// This image cannot run device AddressSanitizer (no instrumented ROCm runtime, XNACK off), and round 5's attempt left an
// abort of the instrumented cheaptrick_kernel that could not be read.  The deterministic replacement: wh::ckp<T> is T*
// in every normal build — the alias, so the shipped code is the code without it, instruction for instruction — and in
// the bounds build a pointer that carries the element range it may touch.  Every [] / * through it is compared with that
// range; the first access outside is recorded (buffer tag, element index, range size) in a device word that
// wh_take_flags reads: WH_FLAG_OOB with the record behind wh_bounds_last(), and the access itself is redirected to the
// range's first element, so the kernel runs on instead of faulting.  The kernels that are covered name their buffers with
// ck_make / ck_sub / ck_as; helpers take ckp<T> parameters; a raw pointer handed to such a helper converts implicitly
// to an UNCHECKED ckp (kernels not yet converted keep compiling).
#ifndef WH_BOUNDS
#define WH_BOUNDS 0
#endif
enum {  // buffer tags of the record
  WH_CK_LDS_MAIN = 1, WH_CK_LDS_AUX = 2, WH_CK_LDS_SCRATCH = 3, WH_CK_TWIDDLE = 4, WH_CK_WAVEFORM = 5, WH_CK_OUT = 6,
  WH_CK_TABLE = 7, WH_CK_LDS_OTHER = 8, WH_CK_IN = 9
};
#if WH_BOUNDS
#define WH_RESTRICT
// first out-of-range access by this translation unit's kernels since the last read: count, tag, index, size
static __device__ unsigned long long g_oob[4];
__device__ __forceinline__ void oob_report(int tag, long long index, long long size) {
  if (atomicAdd(&g_oob[0], 1ull) == 0ull) {
    g_oob[1] = (unsigned long long)tag;
    g_oob[2] = (unsigned long long)index;
    g_oob[3] = (unsigned long long)size;
  }
}
template <class T>
struct ckp {
  T* p = nullptr;
  T* base = nullptr;  // element 0 of the range
  long long n = -1;   // elements in the range; < 0: unchecked
  int tag = 0;
  __host__ __device__ ckp() {}
  __host__ __device__ ckp(T* q) : p(q), base(q), n(-1), tag(0) {}  // a raw pointer: unchecked
  __host__ __device__ ckp(T* q, T* b, long long nn, int tg) : p(q), base(b), n(nn), tag(tg) {}
  template <class U, class = decltype(static_cast<T*>(static_cast<U*>(nullptr)))>
  __host__ __device__ ckp(const ckp<U>& o) : p(o.p), base(o.base), n(o.n), tag(o.tag) {}  // T* -> const T*
  __device__ __forceinline__ T* at(long long i) const {
    if (n >= 0) {
      const long long k = (p - base) + i;
      if (k < 0 || k >= n) {
        oob_report(tag, k, n);
        return base;
      }
    }
    return p + i;
  }
  __device__ __forceinline__ T& operator[](long long i) const { return *at(i); }
  __device__ __forceinline__ T& operator*() const { return *at(0); }
  __host__ __device__ ckp operator+(long long k) const { return ckp(p + k, base, n, tag); }
  __host__ __device__ ckp operator-(long long k) const { return ckp(p - k, base, n, tag); }
  __host__ __device__ explicit operator bool() const { return p != nullptr; }
};
template <class T>
__host__ __device__ __forceinline__ ckp<T> ck_make(T* q, long long n, int tag) { return ckp<T>(q, q, n, tag); }
// elements [off, off + n) of p's range as a range of its own
template <class T>
__host__ __device__ __forceinline__ ckp<T> ck_sub(ckp<T> p, long long off, long long n, int tag) {
  return ckp<T>(p.p + off, p.p + off, n, tag);
}
// the same bytes seen as U (the range is re-expressed in elements of U)
template <class U, class T>
__host__ __device__ __forceinline__ ckp<U> ck_as(ckp<T> p) {
  U* b = reinterpret_cast<U*>(p.base);
  const long long n = p.n < 0 ? -1 : (long long)((p.n * (long long)sizeof(T)) / (long long)sizeof(U));
  return ckp<U>(reinterpret_cast<U*>(p.p), b, n, p.tag);
}
template <class T>
__host__ __device__ __forceinline__ T* ck_raw(ckp<T> p) { return p.p; }
// host side: this translation unit's record, read and cleared (registered with wh_api.hip at load time)
int bounds_register(int (*reader)(unsigned long long*));
static int bounds_reader_tu(unsigned long long* out4) {
  const unsigned long long z[4] = {0ull, 0ull, 0ull, 0ull};
  if (hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_oob), sizeof z) != hipSuccess) return 1;
  if (out4[0] && hipMemcpyToSymbol(HIP_SYMBOL(g_oob), z, sizeof z) != hipSuccess) return 1;
  return 0;
}
static const int bounds_registered_tu = bounds_register(&bounds_reader_tu);
__device__ __forceinline__ double2 ldg2(const ckp<const double2>& p) { return ldg2(static_cast<const double2*>(p.at(0))); }
__device__ __forceinline__ double ldg(const ckp<const double>& p) { return ldg(static_cast<const double*>(p.at(0))); }
#else
#define WH_RESTRICT __restrict__
template <class T>
using ckp = T*;
template <class T>
__host__ __device__ __forceinline__ T* ck_make(T* q, long long, int) { return q; }
template <class T>
__host__ __device__ __forceinline__ T* ck_sub(T* p, long long off, long long, int) { return p + off; }
template <class U, class T>
__host__ __device__ __forceinline__ U* ck_as(T* p) { return reinterpret_cast<U*>(p); }
template <class T>
__host__ __device__ __forceinline__ T* ck_raw(T* p) { return p; }
#endif

// Workgroup-wide synchronisation for NT cooperating threads.  A single-wave group (NT == 64) needs no
// hardware barrier: its lanes run in lockstep, so a compiler-level wavefront fence is enough to order the
// LDS traffic.  This is what lets the per-frame kernels run as one wave per frame with zero s_barrier.
template <int NT>
__device__ __forceinline__ void sync() {
  if constexpr (NT <= WH_WAVE) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

// Workgroups are dealt to the 8 XCDs of the MI355X round-robin by linear id, and every XCD has its own L2.  The
// per-frame / per-pulse kernels read overlapping neighbourhoods (a 5 ms hop against 20-40 ms analysis windows; the
// two spectrogram rows a pulse interpolates are its neighbour's too), so unit u = consecutive ids would put every
// neighbourhood into all eight L2s.  This mapping gives XCD x the contiguous range [x*ceil(n/8), (x+1)*ceil(n/8)).
// Returns n (out of range) for the padding ids of the last rows.
__device__ __forceinline__ long long xcd_unit(long long id, long long n) {
  constexpr int kXcds = 8;
  const long long per = (n + kXcds - 1) / kXcds;
  const long long u = (id % kXcds) * per + id / kXcds;
  return (id / kXcds < per && u < n) ? u : n;
}
__host__ __device__ __forceinline__ long long xcd_grid(long long n) { return ((n + 7) / 8) * 8; }

// Barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory counter, so a global load
// issued before it (the FFT passes fetch their twiddles ahead of the barrier) would have to land before any wave
// may pass; with the fences restricted to the local address space the load stays in flight across the barrier.
// Only valid where the threads hand each other LDS contents and nothing else.
template <int NT>
__device__ __forceinline__ void sync_lds() {
  if constexpr (NT <= WH_WAVE) {
    sync<NT>();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
  }
}

// A lane-private serial recurrence over the samples [i0, i1) (the chunked IIR passes): the recurrence itself costs
// ~40 cycles per sample, a dependent global load per sample ~1500, and the lanes of a wave sit a whole chunk apart so
// nothing coalesces.  The samples are therefore fetched in blocks of B independent loads, one block ahead of the
// block the recurrence is consuming.  interior(i) says that fast(i) .. fast(i + B - 1) are plain loads (no edge
// extension); edge blocks go through slow().  body(i, v) runs in ascending i.
template <int B, class Interior, class Fast, class Slow, class Body>
__device__ __forceinline__ void serial_run(int64_t i0, int64_t i1, Interior interior, Fast fast, Slow slow, Body body) {
  double cur[B], nxt[B];
  auto fetch = [&](double (&v)[B], int64_t i) {
    if (i + B > i1) return;
    if (interior(i)) {
#pragma unroll
      for (int k = 0; k < B; ++k) v[k] = fast(i + k);
    } else {
#pragma unroll
      for (int k = 0; k < B; ++k) v[k] = slow(i + k);
    }
  };
  int64_t i = i0;
  fetch(cur, i);
  for (; i + B <= i1; i += B) {
    fetch(nxt, i + B);
#pragma unroll
    for (int k = 0; k < B; ++k) body(i + k, cur[k]);
#pragma unroll
    for (int k = 0; k < B; ++k) cur[k] = nxt[k];
  }
  for (; i < i1; ++i) body(i, slow(i));
}

// Geometry of the context's twiddle tables (d_twiddle, filled by wh_api.hip; read by the passes of wh_fft.h).
// Pass twiddles.  The context's table of size n lives at [n, 2n) of d_twiddle (wh_api.hip); behind those tables (0.56 MB),
// from 2 * WH_MAX_TWIDDLE on, every radix R in {2, 4, 8} has one table per pass span M = NS * R <= WH_MAX_FFT, laid out
// [k][r]: entry k * (R - 1) + r - 1 = exp(-2 pi i k r / M), k < M / R, 1 <= r < R.  A butterfly's R - 1 twiddles are then
// R - 1 consecutive entries: one address per butterfly and immediate offsets, where the size-N table needed R - 1
// products (k r N / M) & (N - 1).  The entries are copies of the size-M table's entry k r, which is the size-N table's
// entry k r N / M bit for bit (the host computes exp(-2 pi i k / n) as -2 pi k / n in long double: scaling k and n by
// the same power of two scales the rounded angle exactly), so the transforms' results do not change.
constexpr int fft_ptw_count(int R) { return (2 * WH_MAX_FFT / R - 1) * (R - 1); }  // entries of radix R's tables
constexpr int fft_ptw_offset(int M, int R) {                                       // table (M, R), from d_twiddle
  return 2 * WH_MAX_TWIDDLE + (R >= 4 ? fft_ptw_count(2) : 0) + (R >= 8 ? fft_ptw_count(4) : 0) + (M / R - 1) * (R - 1);
}
#define WH_TWIDDLE_ENTRIES (2 * WH_MAX_TWIDDLE + wh::fft_ptw_count(2) + wh::fft_ptw_count(4) + wh::fft_ptw_count(8))

}  // namespace wh
