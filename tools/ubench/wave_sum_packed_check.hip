// Lane semantics the packed reductions of wh_reduce.h rest on, checked on the device the way wave_sum_check.hip and
// dpp_check.hip check the DPP controls:
//   * v_permlane16_swap_b32 / v_permlane32_swap_b32 of a register with a copy of itself: the two outputs hold, in every
//     lane, the value of the same lane of the even | odd row of its pair, and of the lower | upper half of the wave;
//   * dpp_xor4 (row_shl:4 on banks 0 and 2, row_shr:4 on banks 1 and 3) reads lane ^ 4, row_ror:8 reads lane ^ 8;
//   * wave_sum2_packed / wave_sum4_packed give wave_sum's bits in the lanes that are documented to hold each value.
// hipcc --offload-arch=gfx950 -O2 wave_sum_packed_check.hip -o wave_sum_packed_check.bin && ./wave_sum_packed_check.bin
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include "../../python-world_amd/csrc/wh_reduce.h"

// out rows of 64: 0/1 permlane16_swap outputs, 2/3 permlane32_swap outputs, 4 dpp_xor4, 5 row_ror:8 (all on the lane id);
// 6 wave_sum2_packed, 7 wave_sum4_packed, 8 ... 11 wave_sum of the four values
__global__ void k(const double* in, double* out) {
  const int l = threadIdx.x;
  const unsigned id = (unsigned)l;
  const auto s16 = __builtin_amdgcn_permlane16_swap(id, id, false, false);
  const auto s32 = __builtin_amdgcn_permlane32_swap(id, id, false, false);
  out[0 * 64 + l] = (double)s16[0];
  out[1 * 64 + l] = (double)s16[1];
  out[2 * 64 + l] = (double)s32[0];
  out[3 * 64 + l] = (double)s32[1];
  out[4 * 64 + l] = wh::dpp_xor4((double)l);
  out[5 * 64 + l] = wh::dpp_row_perm<0x128>((double)l);
  const double a = in[l], b = in[64 + l], c = in[128 + l], d = in[192 + l];
  out[6 * 64 + l] = wh::wave_sum2_packed(a, b);
  out[7 * 64 + l] = wh::wave_sum4_packed(a, b, c, d);
  out[8 * 64 + l] = wh::wave_sum(a);
  out[9 * 64 + l] = wh::wave_sum(b);
  out[10 * 64 + l] = wh::wave_sum(c);
  out[11 * 64 + l] = wh::wave_sum(d);
}
static bool same_bits(double x, double y) { return std::memcmp(&x, &y, sizeof x) == 0; }
int main() {
  double h[256], o[12 * 64], *d_in, *d_out;
  for (int i = 0; i < 256; ++i) h[i] = (i % 3 == 0 ? 1e16 : i % 3 == 1 ? -1e16 : 1.0) * (1 + i / 64) + 1.0 / (i + 1);
  if (hipMalloc(&d_in, sizeof h) != hipSuccess || hipMalloc(&d_out, sizeof o) != hipSuccess) return 2;
  hipMemcpy(d_in, h, sizeof h, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, d_in, d_out);
  if (hipMemcpy(o, d_out, sizeof o, hipMemcpyDeviceToHost) != hipSuccess) return 2;
  int bad[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int l = 0; l < 64; ++l) {
    // one output is the even row's lane, the other the odd row's (which is which is not relied on: the two are added)
    const double e16 = (double)(l & ~16), o16 = (double)(l | 16), lo32 = (double)(l & ~32), hi32 = (double)(l | 32);
    bad[0] += !((o[l] == e16 && o[64 + l] == o16) || (o[l] == o16 && o[64 + l] == e16));
    bad[1] += !((o[128 + l] == lo32 && o[192 + l] == hi32) || (o[128 + l] == hi32 && o[192 + l] == lo32));
    bad[2] += o[4 * 64 + l] != (double)(l ^ 4);
    bad[3] += o[5 * 64 + l] != (double)(l ^ 8);
    const int q = l & 3;
    bad[4] += !same_bits(o[6 * 64 + l], o[(8 + ((q == 1 || q == 2) ? 1 : 0)) * 64 + l]);
    bad[5] += !same_bits(o[7 * 64 + l], o[(8 + q) * 64 + l]);
  }
  printf("lanes off: permlane16_swap %d  permlane32_swap %d  dpp_xor4 %d  row_ror:8 %d  wave_sum2_packed %d  wave_sum4_packed %d\n",
         bad[0], bad[1], bad[2], bad[3], bad[4], bad[5]);
  printf("lane 5: swap16 (%g, %g) swap32 (%g, %g) xor4 %g ror8 %g\n", o[5], o[64 + 5], o[128 + 5], o[192 + 5], o[4 * 64 + 5], o[5 * 64 + 5]);
  printf("lane 21: swap16 (%g, %g)  lane 37: swap32 (%g, %g)\n", o[21], o[64 + 21], o[128 + 37], o[192 + 37]);
  int all = 0;
  for (int i = 0; i < 6; ++i) all += bad[i];
  return all != 0;
}
