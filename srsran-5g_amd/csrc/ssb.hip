// SS/PBCH blocks on gfx950: PBCH payload generation, both scramblings, CRC24C, polar encoding, rate matching, QPSK and
// RE mapping with the PBCH DM-RS, the PSS and the SSS of every block of a batch of slots in one launch, one workgroup
// per block, into the bf16 resource grids of the PDSCH modulator's layout.
//
// Reference (behaviour, not code): lib/phy/upper/channel_processors/ssb/ssb_processor_impl.cpp:29 (process),
// pbch_encoder_impl.cpp:41 (payload) / :80 (first scrambling) / :121 (CRC) / :138 (interleaving, allocation, encoding)
// / :155 (rate matching), pbch_modulator_impl.cpp:30 (second scrambling) / :42 (QPSK) / :52 (RE pattern),
// signal_processors/dmrs_pbch_processor_impl.cpp:41 (sequence) / :50 (RE pattern), pss_processor_impl.cpp:32,
// sss_processor_impl.cpp:32, the sequence generators' scaling and product (pss_sequence_generator.h:68,
// sss_sequence_generator.h:91), adt/bf16.h:39.
//
// Work decomposition, after pdcch_kernel's. Wave 0 encodes: lanes 0-31 form a_i from the 28 bits read from device
// memory and the bits the plan fixes; a ballot makes a one word, two of its bits select the first scrambling's mask
// (four per block, built on the host), the CRC24C is a xor of per-position weights, and the 56 bits of c are one
// wave-uniform 64-bit mask. The encoder input u is formed 64 positions at a time by a ballot over one table lookup per
// position, which leaves u as 16 words, one per lane; u G_512 is five shift-and-mask stages inside each word and four
// lane exchanges across words. Meanwhile waves 1-3 evaluate the 27 Gold words of the second scrambling (chunks 0-3 of
// the sequence of N_id) and the 9 of the DM-RS. After one barrier every lane takes REs of the block's four symbols in
// grid order, consecutive lanes on consecutive subcarriers, and stores each rounded word once per listed port. Only the
// REs the reference writes are written: symbol 0 outside the PSS and the gaps beside the SSS stay as they are.
//
// Floating point follows the reference exactly: every product term is rounded separately (no contraction).
#include "gold_device.h"
#include "signal_device.h"
#include "srsgpu_internal.h"
#include "ssb_host.h"

#pragma clang fp contract(off)

namespace srsgpu {
namespace {

constexpr uint32_t SSB_THREADS    = 256;
constexpr uint32_t SSB_DATA_WORDS = SSB_PBCH_BITS / 32;  // 27
constexpr uint32_t SSB_DMRS_WORDS = 9;                   // 144 values of two bits

__global__ __launch_bounds__(SSB_THREADS) void ssb_kernel(const ssb_desc* __restrict__ descs,
                                                           const ssb_tables* __restrict__ tables,
                                                           const uint8_t* __restrict__ payloads,
                                                           uint32_t* __restrict__ grids,
                                                           const uint32_t* __restrict__ x1,
                                                           const uint32_t* __restrict__ x2_jump,
                                                           const uint32_t* __restrict__ x2_lane)
{
  __shared__ uint32_t x_words[SSB_POLAR_N / 32];  // the encoded bits d, bit q at word q / 32, bit q % 32
  __shared__ uint32_t gold_data[SSB_DATA_WORDS];
  __shared__ uint32_t gold_dmrs[SSB_DMRS_WORDS];

  const ssb_desc& d   = descs[blockIdx.x];
  const uint32_t  tid = threadIdx.x, lane = tid & 63u;

  if (tid < 64) {
    // a: the payload's 24 bits and the SFN's four LSBs from device memory, the rest fixed in the plan.
    const uint8_t* p   = payloads + d.payload_offset;
    const uint32_t dyn = (static_cast<uint32_t>(p[0]) << 20) | (static_cast<uint32_t>(p[1]) << 12) |
                         (static_cast<uint32_t>(p[2]) << 4) | (p[3] & 15u);  // dynamic bit t at bit 27 - t
    uint32_t bit = 0;
    if (lane < 32) {
      const uint32_t src = tables->dyn_source[lane];
      bit                = src == SSB_DYNAMIC_NONE ? (d.a_const >> lane) & 1u : (dyn >> (27u - src)) & 1u;
    }
    const uint32_t a = static_cast<uint32_t>(__ballot(bit != 0));
    // First scrambling, advanced by M v with v the SFN's 3rd and 2nd LSB, and the CRC24C of the 32 scrambled bits.
    const uint32_t v       = 2u * ((a >> tables->v_hi) & 1u) + ((a >> tables->v_lo) & 1u);
    const uint32_t a_prime = a ^ d.scramble[v];
    uint32_t       crc     = (lane < 32 && ((a_prime >> lane) & 1u) != 0) ? tables->crc_weights[31u - lane] : 0u;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      crc ^= __shfl_xor(crc, m);
    }
    // c: bit i < 32 is a'_i, bit 32 + j is parity bit j (the CRC's MSB first).
    const uint64_t c = a_prime | (static_cast<uint64_t>(__builtin_bitreverse32(crc) >> 8) << 32);
    // u: position q takes c[u_source[q]] (input interleaver and allocation), frozen positions 0. Lane j keeps word j.
    uint32_t w = 0;
#pragma unroll
    for (uint32_t r = 0; r < SSB_POLAR_N / 64; ++r) {
      const uint32_t src = tables->u_source[64u * r + lane];
      const uint64_t u   = __ballot(src < SSB_PBCH_K && ((c >> (src & 63u)) & 1u) != 0);
      w = lane == 2u * r ? static_cast<uint32_t>(u) : lane == 2u * r + 1u ? static_cast<uint32_t>(u >> 32) : w;
    }
    // d = u G_N: d[i] ^= d[i + t] for the i with bit t clear, t = 1 .. N / 2.
    w ^= (w >> 1) & 0x55555555u;
    w ^= (w >> 2) & 0x33333333u;
    w ^= (w >> 4) & 0x0f0f0f0fu;
    w ^= (w >> 8) & 0x00ff00ffu;
    w ^= (w >> 16) & 0x0000ffffu;
#pragma unroll
    for (uint32_t t = 1; t < 16; t <<= 1) {
      const uint32_t other = __shfl_down(w, t);
      w ^= (lane & t) == 0 ? other : 0u;
    }
    if (lane < 16) {
      x_words[lane] = w;
    }
  } else {
    for (uint32_t i = tid - 64u; i < SSB_DATA_WORDS + SSB_DMRS_WORDS; i += SSB_THREADS - 64u) {
      if (i < SSB_DATA_WORDS) {
        const uint32_t w = d.data_word0 + i;
        gold_data[i]     = gold_word(d.c_init_data, w, w >> 6, x1, x2_jump, x2_lane);
      } else {
        gold_dmrs[i - SSB_DATA_WORDS] = gold_word(d.c_init_dmrs, i - SSB_DATA_WORDS, 0, x1, x2_jump, x2_lane);
      }
    }
  }
  __syncthreads();

  const uint32_t v    = d.v, P = d.nof_ports;
  const float    qpsk = 0.70710678118654752440f;  // float(M_SQRT1_2)
  // Item t: symbol s of the block, subcarrier k of its 240.
  for (uint32_t t = tid; t < 4u * 240u; t += SSB_THREADS) {
    const uint32_t s = t / 240u, k = t - 240u * s;
    const bool     sync = k >= 56u && k < 183u;  // the PSS's and the SSS's subcarriers
    float          re, im;
    if (s == 0u || (s == 2u && k >= 48u && k < 192u)) {
      if (!sync) {
        continue;
      }
      const uint32_t n = k - 56u;
      if (s == 0u) {
        // PSS: (d, 0) scaled by the amplitude.
        const float dn = ((d.pss[n >> 5] >> (n & 31u)) & 1u) ? -1.f : 1.f;
        re             = dn * d.pss_amplitude;
        im             = 0.f * d.pss_amplitude;
      } else {
        // SSS: (d0, 0) scaled by 1, times (d1, 0) as complex numbers.
        const float d0 = ((d.sss0[n >> 5] >> (n & 31u)) & 1u) ? -1.f : 1.f;
        const float d1 = ((d.sss1[n >> 5] >> (n & 31u)) & 1u) ? -1.f : 1.f;
        const float ar = d0 * 1.f, ai = 0.f * 1.f;
        re             = ar * d1 - ai * 0.f;
        im             = ar * 0.f + ai * d1;
      }
    } else {
      // PBCH and its DM-RS: symbols 1 and 3 whole, symbol 2 on RBs 0-3 and 16-19.
      const uint32_t rb = k / 12u, j = k - 12u * rb;
      const uint32_t rb_rank = s == 1u ? rb : s == 3u ? rb + 28u : rb < 4u ? rb + 20u : rb + 8u;  // of the 48 PBCH RBs
      uint32_t       word, n;
      if ((j & 3u) == v) {
        n    = 2u * (3u * rb_rank + (j >> 2));
        word = gold_dmrs[n >> 5];
      } else {
        const uint32_t rank = j - (j > v ? 1u : 0u) - (j > v + 4u ? 1u : 0u) - (j > v + 8u ? 1u : 0u);
        const uint32_t r    = 9u * rb_rank + rank;
        const uint32_t g    = tables->gather[r];
        const uint32_t q0 = g & 0xffffu, q1 = g >> 16;
        n    = 2u * r;
        word = gold_data[n >> 5] ^ (((x_words[q0 >> 5] >> (q0 & 31u)) & 1u) << (31u - (n & 31u))) ^
               (((x_words[q1 >> 5] >> (q1 & 31u)) & 1u) << (30u - (n & 31u)));
      }
      const uint32_t sh = 31u - (n & 31u);
      re                = ((word >> sh) & 1u) ? -qpsk : qpsk;
      im                = ((word >> (sh - 1u)) & 1u) ? -qpsk : qpsk;
    }
    const uint32_t e    = d.grid_base + s * d.nsc + k;
    const uint32_t word = bf16_bits(re) | (bf16_bits(im) << 16);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (p < static_cast<int>(P)) {
        grids[e + static_cast<uint32_t>(d.ports[p]) * d.port_stride] = word;
      }
    }
  }
}

} // namespace

void launch_ssb(const ssb_desc*   d_descs,
                uint32_t          nof_blocks,
                const ssb_tables* d_tables,
                const uint8_t*    d_payloads,
                uint32_t*         d_grids,
                const uint32_t*   d_x1,
                const uint32_t*   d_x2_jump,
                const uint32_t*   d_x2_lane,
                hipStream_t       stream)
{
  if (nof_blocks == 0) {
    return;
  }
  hipLaunchKernelGGL(ssb_kernel, dim3(nof_blocks), dim3(SSB_THREADS), 0, stream, d_descs, d_tables, d_payloads, d_grids,
                     d_x1, d_x2_jump, d_x2_lane);
}

} // namespace srsgpu
