// Shared device-side helpers for the srsgpu PHY kernels (gfx950 / CDNA4, wave64).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>
#include <utility>

namespace srsgpu {

constexpr int WAVE = 64;

/// Compile-time loop: calls f(std::integral_constant<int, I>{}) for I = 0 .. N-1 (fully unrolled, static indices).
template <typename F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>)
{
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f)
{
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// Cross-lane reductions on DPP (VALU lane permutations: no LDS round trip, which __shfl_xor's ds_bpermute costs per
// step). Within a 16-lane row: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror, after which every
// lane of the row holds the row's result (each step pairs lanes symmetrically, so all lanes compute identical bits).
// Across rows: row_bcast:15 into rows 1 and 3 (ROW_MASK 0xa; the 32-lane halves: lanes 31 / 63 hold them) and
// row_bcast:31 into rows 2 and 3 (ROW_MASK 0xc; lane 63 holds the wave's), read back with readlane.
constexpr int DPP_XOR1 = 0xb1, DPP_XOR2 = 0x4e, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;
constexpr int DPP_BCAST15 = 0x142, DPP_BCAST31 = 0x143;

/// v permuted by CTRL within the rows of ROW_MASK; old in the other rows and where the source lane is out of range.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_f(float old, float v)
{
  return __int_as_float(
      __builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int dpp_i(int old, int v)
{
  return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ float readlane_f(float v, int lane)
{
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

/// One DPP step of a wave reduction: v ^ (v permuted by CTRL within the enabled rows; 0 elsewhere).
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_xor(uint32_t v)
{
  return v ^ static_cast<uint32_t>(dpp_i<CTRL, ROW_MASK>(0, static_cast<int>(v)));
}

/// XOR of v over the 64 lanes (all lanes must be active), returned to every lane: the six steps above.
__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
  v = dpp_xor<DPP_XOR1>(v);
  v = dpp_xor<DPP_XOR2>(v);
  v = dpp_xor<DPP_HALF_MIRROR>(v);
  v = dpp_xor<DPP_MIRROR>(v);
  v = dpp_xor<DPP_BCAST15, 0xa>(v);
  v = dpp_xor<DPP_BCAST31, 0xc>(v);
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 63));
}

/// One DPP step of an OR reduction.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_or(uint32_t v)
{
  return v | static_cast<uint32_t>(dpp_i<CTRL, ROW_MASK>(0, static_cast<int>(v)));
}

/// OR of v over the 64 lanes (all lanes active), returned to every lane; the steps of wave_xor.
__device__ __forceinline__ uint32_t wave_or(uint32_t v)
{
  v = dpp_or<DPP_XOR1>(v);
  v = dpp_or<DPP_XOR2>(v);
  v = dpp_or<DPP_HALF_MIRROR>(v);
  v = dpp_or<DPP_MIRROR>(v);
  v = dpp_or<DPP_BCAST15, 0xa>(v);
  v = dpp_or<DPP_BCAST31, 0xc>(v);
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 63));
}

__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    int w = __shfl_xor(v, o, WAVE);
    v     = v > w ? v : w;
  }
  return v;
}

/// Integer clamp; lowers to a single v_med3_i32.
__device__ __forceinline__ int clamp_i(int v, int lo, int hi)
{
  return v < lo ? lo : (v > hi ? hi : v);
}

/// (ax + j ay)(bx + j by) with both fused multiply-adds explicit and nothing left to contract, so the rounding does
/// not depend on the compiler's contraction choices in context: the estimator's per-symbol CFO rotation of its
/// estimates and the demodulator's rotation of the compact estimate row must agree bit for bit.
__device__ __forceinline__ void cmul_fused(float ax, float ay, float bx, float by, float& rx, float& ry)
{
#pragma clang fp contract(off)
  const float pyy = ay * by;
  const float pyx = ay * bx;
  rx              = __builtin_fmaf(ax, bx, -pyy);
  ry              = __builtin_fmaf(ax, by, pyx);
}

} // namespace srsgpu
