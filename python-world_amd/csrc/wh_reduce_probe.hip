// Test hook for the packed workgroup reductions of wh_reduce.h: wh_reduce_probe runs block_sum2 / block_sum3 / block_sum5 on
// caller data in one workgroup of NT threads and, next to them, the routine they replaced — one wave_sum per value, lane 0
// of every wave to scratch[k * NW + w], the waves' totals added in ascending order from 0.0.  Nothing in the library calls
// it (tests/test_hip_reduce.py does).  Compiled with wh_d4c.hip's flags (build.py), behind D4C's opaque thread index: the
// reductions as d4c_kernel compiles them.
#include "wh_d4c_types.h"
#include "wh_reduce.h"

namespace {

// in: K rows of NT doubles (value k of thread t at in[k * NT + t]).  out: per thread 2 K doubles, the packed totals and
// then the sequential routine's (every thread writes its own copy: a total that did not reach a lane shows).
template <int NT, int K>
__global__ __launch_bounds__(NT) void reduce_probe_kernel(const double* __restrict__ in, double* __restrict__ out) {
  __shared__ double lds[5 * 8];
  const wh::ckp<double> scratch = wh::ck_make(&lds[0], 5 * 8, wh::WH_CK_LDS_SCRATCH);
  const int tid = threadIdx.x;
  double v[K], p[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < K; ++k) p[k] = v[k] = in[k * NT + tid];
  if constexpr (K == 2) wh::block_sum2<NT>(p[0], p[1], scratch);
  else if constexpr (K == 3) wh::block_sum3<NT>(p[0], p[1], p[2], scratch);
  else wh::block_sum5<NT>(p[0], p[1], p[2], p[3], p[4], scratch);
#pragma unroll
  for (int k = 0; k < K; ++k) out[(long long)tid * 2 * K + k] = p[k];
  // the routine block_sum2 / 3 / 5 were before the packed tree
  constexpr int NW = NT / WH_WAVE;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wh::wave_sum(v[k]);
  __syncthreads();
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) scratch[k * NW + (tid >> 6)] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double t = 0.0;
    if constexpr (NW > 1) {
#pragma unroll
      for (int i = 0; i < NW; ++i) t += scratch[k * NW + i];
    } else {
      t = v[k];  // (a one-wave group never went through scratch)
    }
    out[(long long)tid * 2 * K + K + k] = t;
  }
}

template <int NT>
int launch_reduce_probe(hipStream_t st, int k, const double* in, double* out) {
  if (k == 2) return wh::launch_untimed(st, "reduce_probe_kernel", reduce_probe_kernel<NT, 2>, dim3(1), dim3(NT), 0, in, out);
  if (k == 3) return wh::launch_untimed(st, "reduce_probe_kernel", reduce_probe_kernel<NT, 3>, dim3(1), dim3(NT), 0, in, out);
  return wh::launch_untimed(st, "reduce_probe_kernel", reduce_probe_kernel<NT, 5>, dim3(1), dim3(NT), 0, in, out);
}

}  // namespace

extern "C" {

int wh_reduce_probe(wh_ctx* ctx, void* stream, int nt, int k, const double* in, double* out) {
  if (!ctx || !in || !out || (k != 2 && k != 3 && k != 5) || (nt != 64 && nt != 128 && nt != 256 && nt != 512))
    return wh::fail_msg("wh_reduce_probe", "bad argument: nt is 64, 128, 256 or 512 and k is 2, 3 or 5");
  WH_ENTER(ctx);
  const hipStream_t st = (hipStream_t)stream;
  switch (nt) {
    case 64: return launch_reduce_probe<64>(st, k, in, out);
    case 128: return launch_reduce_probe<128>(st, k, in, out);
    case 256: return launch_reduce_probe<256>(st, k, in, out);
    default: return launch_reduce_probe<512>(st, k, in, out);
  }
}

}  // extern "C"
