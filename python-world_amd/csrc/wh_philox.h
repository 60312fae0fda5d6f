// The counter-based normal generator of the no-host-noise decode (Philox-4x32-10 + Box-Muller) and the stream key of an
// utterance.  response_pulse / response_pair (wh_resp_pulse.h, wh_resp_pair.h) draw from it; wh_philox_normals
// (wh_synthesis.hip) dumps the same stream sample by sample.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// ---- counter-based normal generator (Philox-4x32-10 + Box-Muller) for the no-host-noise mode ----
__device__ __forceinline__ void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
  c1 = (uint32_t)p1;
  c3 = (uint32_t)p0;
  c0 = n0;
  c2 = n2;
}
__device__ __attribute__((noinline)) double normal_at(uint64_t seed, uint64_t q) {  // a call: see log_call, wh_minphase.h
  uint32_t c0 = (uint32_t)(q >> 1), c1 = (uint32_t)((q >> 1) >> 32), c2 = 0x9E3779B9u, c3 = 0x243F6A88u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const double u1 = ((double)c0 * 4294967296.0 + (double)c1 + 0.5) * (1.0 / 18446744073709551616.0);
  const double u2 = ((double)c2 * 4294967296.0 + (double)c3 + 0.5) * (1.0 / 18446744073709551616.0);
  const double rr = sqrt(-2.0 * log(u1));
  double s, c;
  sincospi(2 * u2, &s, &c);  // sin/cos(2*pi*u2) without the large-argument reduction path
  return (q & 1) ? rr * s : rr * c;
}

// Both normals of one Philox block (normal_at(seed, 2*blk) and normal_at(seed, 2*blk + 1), bit for bit): the pulse's
// noise run is generated block-wise, one Box-Muller evaluation per pair instead of one per sample.
__device__ __attribute__((noinline)) double2 normal_pair(uint64_t seed, uint64_t blk) {
  uint32_t c0 = (uint32_t)blk, c1 = (uint32_t)(blk >> 32), c2 = 0x9E3779B9u, c3 = 0x243F6A88u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const double u1 = ((double)c0 * 4294967296.0 + (double)c1 + 0.5) * (1.0 / 18446744073709551616.0);
  const double u2 = ((double)c2 * 4294967296.0 + (double)c3 + 0.5) * (1.0 / 18446744073709551616.0);
  const double rr = sqrt(-2.0 * log(u1));
  double s, c;
  sincospi(2 * u2, &s, &c);
  return make_double2(rr * c, rr * s);
}

// The stream key of utterance u under `seed` (response_kernel derives the same one).
__device__ __host__ __forceinline__ uint64_t philox_key(uint64_t seed, uint64_t u) {
  return seed * 0x9E3779B97F4A7C15ull + u * 0xD1B54A32D192ED03ull + 1;
}

}  // namespace
