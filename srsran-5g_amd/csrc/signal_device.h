// Device helpers shared by the signal kernels (estimator, demodulator, modulators, PDCCH, PUCCH, PRACH, OFDM, UCI):
// the bf16 grid word, complex arithmetic on cpx, std::isnormal, the butterfly wave reductions and the job-descriptor
// copy into LDS. Everything is force-inlined; a kernel file includes this and defines none of it again.
#pragma once

#include "common.h"
#include "cpx.h"

namespace srsgpu {

/// float -> bf16 bits, round to nearest even (adt/bf16.h). The integer form on purpose: every grid and estimate word
/// the kernels store is held bit-exact to the reference's, which rounds with exactly this arithmetic. The hardware
/// packing conversion was tried in its place and rejected: that change did not pass the project's checks. This is
/// the only copy of the rule; a kernel that stores bf16 calls it.
__device__ __forceinline__ uint32_t bf16_bits(float v)
{
  const uint32_t u = __float_as_uint(v);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

/// A grid or estimate word (re in the low half, im in the high half, both bf16) as two floats.
__device__ __forceinline__ cpx bf16c(uint32_t u)
{
  return {__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)};
}
__device__ __forceinline__ uint32_t to_bf16c(cpx v)
{
  return bf16_bits(v.x) | (bf16_bits(v.y) << 16);
}

// Products in the including file's default contraction mode (a pragma there that follows this header does not reach
// them); where the rounding must not depend on it, cmul_fused (common.h).
__device__ __forceinline__ cpx cmul(cpx a, cpx b)
{
  return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
}
/// a * conj(b)
__device__ __forceinline__ cpx cmulc(cpx a, cpx b)
{
  return {a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y};
}
__device__ __forceinline__ float norm2(cpx a)
{
  return a.x * a.x + a.y * a.y;
}

/// std::isnormal without the library: neither zero, subnormal, infinite nor NaN.
__device__ __forceinline__ bool is_normal(float v)
{
  const uint32_t e = (__float_as_uint(v) >> 23) & 0xffu;
  return e != 0u && e != 0xffu;
}

// Wave reductions by butterfly exchange (__shfl_xor with 32, 16, ... 1): every lane ends with the result. The float
// sum adds in butterfly order; the estimator's DPP sums (pusch_chest.hip, wave_sum_dpp) add in another order, so the
// two differ in the last bit and are not interchangeable. The int wave_max is in common.h.
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    v += __shfl_xor(v, m);
  }
  return v;
}
__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    v += __shfl_xor(v, m);
  }
  return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    v = fmaxf(v, __shfl_xor(v, m));
  }
  return v;
}

/// Copies one job descriptor into LDS by 32-bit words, thread tid of nthreads taking every nthreads-th word (one
/// coalesced read instead of dependent scalar loads of its fields). The caller orders it against the readers.
template <typename T>
__device__ __forceinline__ void copy_words(T* lds_dst, const T* src, uint32_t tid, uint32_t nthreads)
{
  static_assert(sizeof(T) % 4 == 0, "the descriptor is copied by words");
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
  uint32_t*       d = reinterpret_cast<uint32_t*>(lds_dst);
  for (uint32_t i = tid; i < sizeof(T) / 4u; i += nthreads) {
    d[i] = s[i];
  }
}

} // namespace srsgpu
