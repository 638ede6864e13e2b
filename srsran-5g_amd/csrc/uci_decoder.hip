// UCI decoder for short blocks (1..11 message bits) on gfx950: one wavefront per field, every field of a plan in one
// launch. Restates short_block_detector_impl::detect exactly (integers only): the validation on the count of non-zero
// LLRs, the rate dematching with its saturating per-block sum, the sign decision (1 bit), the four-codeword search
// (2 bits) and the maximum-likelihood search over the (32, A) code of TS 38.212 section 5.3.3.3 with the GLRT validity
// test (3..11 bits).
//
// Reference (behaviour, not code): lib/phy/upper/channel_coding/short/short_block_detector_impl.cpp:186 (detect), :60
// (validate_spans), :160 (rate_dematch), :89 (detect_2), :129 (detect_3_11); the LLR sum as the AVX2 build computes it,
// lib/phy/upper/log_likelihood_ratio.cpp:432 (int8 saturating add, then the clamp to +-120).
//
// Rate dematching: position p of the N-long block receives LLRs p, p + N, p + 2N, ... and the sum saturates after
// every one of them, so it is no plain sum: 100, 100, -100 gives 20. Each step is a map x -> min(max(x + a, lo), hi);
// these maps are closed under composition (apply (a1, lo1, hi1), then (a2, lo2, hi2): a = a1 + a2, lo = clamp(lo1 + a2,
// lo2, hi2), hi = clamp(hi1 + a2, lo2, hi2)) and composition is associative. The wave's 64 lanes are S segments x N
// positions (S the largest power of two with S N <= 64): each lane composes the steps of a contiguous run of blocks,
// a log2(S)-step tree composes the segments in order, and the result is applied to 0. Since x stays in [-120, 120] and
// the bounds too, `a` may itself be clamped to +-240 without changing the map there, which keeps it from overflowing.
//
// 3..11 bits: codeword k (message 2k) is the XOR of basis words 1..10 by the bits of k. Words 1..5 are, position by
// position, the 32 distinct 5-bit numbers (a permuted first-order Reed-Muller code; checked below), so for the low
// five bits of k the 32 correlations are one 32-point Walsh-Hadamard transform of the dematched LLRs taken in that
// order, and the high bits of k select one of 2^(A-6) sign masks (XORs of words 6..10) applied before it. Each half of
// the wave transforms one mask at a time, five butterfly stages through cross-lane shuffles, no LDS. Byte traffic: E
// LLR bytes read per field, three bytes written.
#include "signal_device.h"
#include "srsgpu_internal.h"
#include "uci_basis_words.h"

namespace srsgpu {
namespace {

constexpr int UCI_THREADS         = 256;
constexpr int UCI_FIELDS_PER_BLOCK = UCI_THREADS / 64;
constexpr int LLR_LIMIT           = 120;  // log_likelihood_ratio LLR_MAX

/// Walsh-Hadamard input index of codeword position n: bit i - 1 = M_{n,i}, i = 1..5.
constexpr uint32_t uci_hadamard_index(uint32_t n)
{
  uint32_t idx = 0;
  for (uint32_t i = 1; i <= 5; ++i) {
    idx |= ((kUciBasisWords[i] >> n) & 1u) << (i - 1);
  }
  return idx;
}

constexpr bool uci_hadamard_index_is_permutation()
{
  uint32_t seen = 0;
  for (uint32_t n = 0; n < 32; ++n) {
    seen |= 1u << uci_hadamard_index(n);
  }
  return seen == 0xffffffffu;
}

/// Bit plane `bit` of the inverse permutation: bit q of the result = bit `bit` of the position n with index q.
constexpr uint32_t uci_position_plane(uint32_t bit)
{
  uint32_t w = 0;
  for (uint32_t n = 0; n < 32; ++n) {
    w |= ((n >> bit) & 1u) << uci_hadamard_index(n);
  }
  return w;
}

// The odd messages are the complements of the even ones (bit 0 comes from the metric's sign) ...
static_assert(kUciBasisWords[0] == 0xffffffffu, "basis word 0 must be all ones");
// ... and words 1..5 enumerate the 32 Walsh functions.
static_assert(uci_hadamard_index_is_permutation(), "basis words 1..5 must take 32 distinct values over the positions");

constexpr uint32_t kUciPositionPlanes[5] = {uci_position_plane(0), uci_position_plane(1), uci_position_plane(2),
                                            uci_position_plane(3), uci_position_plane(4)};

/// min(max()), not common.h's clamp_i: the ternary form gives the same integers but compiles differently here.
__device__ inline int clamp_int(int x, int lo, int hi)
{
  return min(max(x, lo), hi);
}

__global__ __launch_bounds__(UCI_THREADS) void uci_decoder_kernel(const uci_field_desc* __restrict__ descs,
                                                                  uint32_t                          nof_fields,
                                                                  const int8_t* __restrict__        src0,
                                                                  const int8_t* __restrict__        src1,
                                                                  const int8_t* __restrict__        src2,
                                                                  uint16_t* __restrict__            msgs,
                                                                  uint8_t* __restrict__             status)
{
  // One field per wavefront: everything derived from the descriptor is wave-uniform, and so is every branch on it.
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t f    = blockIdx.x * UCI_FIELDS_PER_BLOCK + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (f >= nof_fields) {
    return;
  }
  const uci_field_desc d    = descs[f];
  const uint32_t       A    = d.nof_bits;
  const uint32_t       qm   = d.qm;
  const uint32_t       E    = d.nof_enc;
  const int8_t*        llrs = (d.source == 0 ? src0 : d.source == 1 ? src1 : src2) + d.llr_offset;

  // Rate dematching into N positions (see the head of the file), counting the non-zero LLRs on the way.
  const uint32_t N    = A == 1 ? qm : A == 2 ? 3u * qm : 32u;
  const uint32_t S    = 1u << (31 - __builtin_clz(64u / N));
  const uint32_t seg  = lane / N;
  const uint32_t p    = lane - seg * N;
  const uint32_t nblk = (E + N - 1u) / N;
  const uint32_t per  = (nblk + S - 1u) / S;
  const uint32_t b0   = seg < S ? min(seg * per, nblk) : 0u;
  const uint32_t b1   = seg < S ? min(b0 + per, nblk) : 0u;
  int            a = 0, lo = -LLR_LIMIT, hi = LLR_LIMIT, nonzero = 0;
  // A position past the end of a partial last block adds 0, which leaves the map as it is. Unrolled so that a lane has
  // four loads in flight.
#pragma unroll 4
  for (uint32_t b = b0; b < b1; ++b) {
    const uint32_t i = b * N + p;
    const int      v = i < E ? llrs[i] : 0;
    nonzero += v != 0;
    a  = clamp_int(a + v, -2 * LLR_LIMIT, 2 * LLR_LIMIT);
    lo = clamp_int(lo + v, -LLR_LIMIT, LLR_LIMIT);
    hi = clamp_int(hi + v, -LLR_LIMIT, LLR_LIMIT);
  }
  for (uint32_t st = 1; st < S; st <<= 1) {
    // Segment seg (a multiple of 2 st) takes in segment seg + st, which follows it. The other lanes compute values
    // that nobody reads.
    const int from = static_cast<int>(lane + st * N);
    const int a2 = __shfl(a, from), lo2 = __shfl(lo, from), hi2 = __shfl(hi, from);
    lo = clamp_int(lo + a2, lo2, hi2);
    hi = clamp_int(hi + a2, lo2, hi2);
    a  = clamp_int(a + a2, -2 * LLR_LIMIT, 2 * LLR_LIMIT);
  }
  const int t = lane < N ? clamp_int(a, lo, hi) : 0;  // dematched LLR of position `lane`
  nonzero     = wave_sum(nonzero);

  uint32_t value = 0;
  bool     valid = false;
  if (nonzero < static_cast<int>(d.min_nonzero) || (A <= 2 && E < qm)) {
    value = (1u << A) - 1u;
  } else if (A == 1) {
    value = __shfl(t, 0) > 0 ? 0u : 1u;
    valid = true;
  } else if (A == 2) {
    int x0 = __shfl(t, 0), x1 = __shfl(t, 1), x2 = __shfl(t, 2);
    if (qm > 1) {
      x0 += __shfl(t, static_cast<int>(qm + 1));
      x1 += __shfl(t, static_cast<int>(2 * qm));
      x2 = __shfl(t, static_cast<int>(qm)) + __shfl(t, static_cast<int>(2 * qm + 1));
    }
    // Codewords (1, 1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, 1): the first strictly greater metric wins, starting
    // from "nothing beats 0". The reference's 2 m^2 / (3 n - m^2) > 0 in double holds exactly when that metric is
    // positive (m = 0 gives 0 or, with every value 0, 0 / 0).
    const int metric[4] = {x0 + x1 + x2, -x0 + x1 - x2, x0 - x1 - x2, -x0 - x1 + x2};
    int       best      = 0;
    for (uint32_t i = 0; i < 4; ++i) {
      if (metric[i] > best) {
        best  = metric[i];
        value = i;
      }
    }
    valid = best > 0;
  } else {
    // Lane (h, q): Walsh index q of half h. It takes the LLR and the mask column of the position with that index.
    const uint32_t q = lane & 31u, h = lane >> 5;
    uint32_t       n = 0, column = 0;
    for (uint32_t i = 0; i < 5; ++i) {
      n |= ((kUciPositionPlanes[i] >> q) & 1u) << i;
    }
    for (uint32_t i = 0; i < 5; ++i) {
      column |= ((kUciBasisWords[6 + i] >> n) & 1u) << i;
    }
    const int      tq        = __shfl(t, static_cast<int>(n));
    const uint32_t nof_masks = A > 6 ? 1u << (A - 6) : 1u;
    const uint32_t nof_walsh = A > 6 ? 32u : 1u << (A - 1);
    // key = |metric| << 11 | (1023 - k) << 1 | (metric < 0): its maximum is the largest |metric| of the lowest k, the
    // reference's first strictly greater one (|metric| <= 32 * 120 < 2^12).
    int best = -1;
    for (uint32_t m0 = 0; m0 < nof_masks; m0 += 2) {
      const uint32_t m = m0 + h;
      int            y = (__popc(column & m) & 1) != 0 ? -tq : tq;
      for (uint32_t bit = 1; bit < 32; bit <<= 1) {
        const int other = __shfl_xor(y, static_cast<int>(bit));
        y               = (q & bit) != 0 ? other - y : y + other;
      }
      const uint32_t k   = m * 32u + q;
      const int      key = static_cast<int>((static_cast<uint32_t>(abs(y)) << 11) | ((1023u - k) << 1) | (y < 0 ? 1u : 0u));
      best               = (m < nof_masks && q < nof_walsh) ? max(best, key) : best;
    }
    best                = wave_max(best);
    const int64_t m     = best >> 11;
    value               = 2u * (1023u - ((static_cast<uint32_t>(best) >> 1) & 1023u)) + (static_cast<uint32_t>(best) & 1u);
    const int64_t norm2 = wave_sum(t * t);
    // The reference tests 31 m^2 / (32 n - m^2) > T in double. Every operand is an integer below 2^53, hence exact
    // there, and Cauchy-Schwarz keeps the denominator >= 0 (0 with m > 0: +inf, valid; m = 0: 0 or 0 / 0, invalid).
    // The exact quotient is either equal to the integer T or at least 1 / (32 n) > 2^-24 away from it, far more than
    // the rounding of one division, so this integer comparison decides the same. No double on the device.
    valid = m > 0 && 31 * m * m > static_cast<int64_t>(d.threshold) * (32 * norm2 - m * m);
  }
  if (lane == 0) {
    msgs[f]   = static_cast<uint16_t>(value);
    status[f] = valid ? 1 : 0;
  }
}

} // namespace

void launch_uci_decode(const uci_field_desc* d_desc,
                       uint32_t              nof_fields,
                       const int8_t*         d_src0,
                       const int8_t*         d_src1,
                       const int8_t*         d_src2,
                       uint16_t*             d_msgs,
                       uint8_t*              d_status,
                       hipStream_t           stream)
{
  if (nof_fields == 0) {
    return;
  }
  const unsigned blocks = (nof_fields + UCI_FIELDS_PER_BLOCK - 1) / UCI_FIELDS_PER_BLOCK;
  hipLaunchKernelGGL(uci_decoder_kernel, dim3(blocks), dim3(UCI_THREADS), 0, stream, d_desc, nof_fields, d_src0, d_src1,
                     d_src2, d_msgs, d_status);
}

} // namespace srsgpu
