// PDCCH on gfx950: DCI encoding, scrambling, QPSK, precoding, RE mapping and DM-RS of every DCI of a batch of slots in
// one launch, one workgroup per DCI, into the bf16 resource grids of the PDSCH modulator's layout.
//
// Reference (behaviour, not code): lib/phy/upper/channel_processors/pdcch/pdcch_processor_impl.cpp:79 (process),
// pdcch_encoder_impl.cpp:33 (CRC attachment) / :63 (interleaving, allocation, encoding) / :79 (rate matching),
// pdcch_modulator_impl.cpp:32 (scrambling) / :45 (QPSK and scaling) / :59 (RE pattern),
// signal_processors/dmrs_pdcch_processor_impl.cpp:32 (c_init) / :40 (sequence) / :52 (RE pattern),
// support/resource_grid_mapper_impl.cpp:140 (RE order), channel_precoder_generic.cpp:27 (precoding), adt/bf16.h:39.
//
// Work decomposition. Wave 0 encodes: lanes read the payload bits from device memory and fold the CRC24C as a xor of
// per-position weights; the K bits of c live in three wave-uniform 64-bit masks; the encoder input u is formed 64
// positions at a time by a ballot over one table lookup per position (input interleaver and allocation composed on
// the host), which leaves u as 16 words, one per lane; u G_N is five shift-and-mask stages inside each word and four
// lane exchanges across words. Meanwhile waves 1-3 evaluate the Gold sequence words of the scrambler and of the DM-RS
// of every CORESET symbol (gold_device.h; every sequence lies in chunk 0) and stage the PRB list. After one barrier
// every lane takes REs of the DCI's PRBs in grid order, consecutive lanes on consecutive subcarriers: k = 1, 5, 9 are
// DM-RS, the other nine carry the rate-matched (one gather table, sub-block interleaver and bit selection composed),
// scrambled, QPSK-mapped bits. Each RE is one complex product per port, rounded once to bf16, one 4-byte vector store.
//
// Floating point follows the reference exactly: every product term is rounded separately (no contraction).
#include "gold_device.h"
#include "signal_device.h"
#include "srsgpu_internal.h"

#pragma clang fp contract(off)

namespace srsgpu {
namespace {

constexpr int PDCCH_THREADS = 256;

__global__ __launch_bounds__(PDCCH_THREADS) void pdcch_kernel(const pdcch_desc* __restrict__ descs,
                                                               const pdcch_code_desc* __restrict__ codes,
                                                               const uint8_t* __restrict__ u_source,
                                                               const uint32_t* __restrict__ gather,
                                                               const uint16_t* __restrict__ prbs,
                                                               const uint32_t* __restrict__ crc_weights,
                                                               const uint8_t* __restrict__ payloads,
                                                               uint32_t* __restrict__ grids,
                                                               const uint32_t* __restrict__ x1,
                                                               const uint32_t* __restrict__ x2_jump,
                                                               const uint32_t* __restrict__ x2_lane)
{
  __shared__ uint32_t x_words[16];  // the encoded bits d, bit q at word q / 32, bit q % 32
  __shared__ uint32_t gold_data[PDCCH_MAX_DATA_WORDS];
  __shared__ uint32_t gold_dmrs[3][PDCCH_MAX_DMRS_WORDS];
  __shared__ uint16_t prb_list[PDCCH_MAX_PRBS];

  const pdcch_desc&      d    = descs[blockIdx.x];
  const pdcch_code_desc& code = codes[d.code];
  const uint32_t         tid = threadIdx.x, lane = tid & 63u;
  const uint32_t         nof_prb = d.nof_prb, duration = d.duration;

  if (tid < 64) {
    // c = payload, then the CRC24C parity of (24 ones, payload) with the RNTI on its last 16 bits.
    const uint32_t A = d.nof_payload_bits, K = code.K, N = 1u << code.n;
    uint32_t       payload_bit[2];
    uint32_t       crc = 0;
#pragma unroll
    for (uint32_t r = 0; r < 2; ++r) {
      const uint32_t i = 64u * r + lane;
      uint32_t       b = 0;
      if (i < A) {
        b = (payloads[d.payload_offset + (i >> 3)] >> (7u - (i & 7u))) & 1u;
        crc ^= b != 0 ? crc_weights[A - 1u - i] : 0u;
      }
      payload_bit[r] = b;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      crc ^= __shfl_xor(crc, m);
    }
    crc ^= d.crc_init;
    uint64_t c[3];
#pragma unroll
    for (uint32_t r = 0; r < 3; ++r) {
      const uint32_t i = 64u * r + lane;
      uint32_t       b = r < 2 ? payload_bit[r] : 0u;
      if (i >= A && i < K) {
        b = (crc >> (23u - (i - A))) & 1u;
      }
      c[r] = __ballot(b != 0);
    }
    // u: position q takes c[u_source[q]] (input interleaver and allocation), frozen positions 0. Lane j keeps word j.
    uint32_t w = 0;
    for (uint32_t r = 0; 64u * r < N; ++r) {
      const uint32_t q   = 64u * r + lane;
      const uint32_t src = q < N ? u_source[code.u_source_offset + q] : 0xffu;
      const uint64_t m   = src < 64u ? c[0] : src < 128u ? c[1] : c[2];
      const uint64_t u   = __ballot(src != 0xffu && ((m >> (src & 63u)) & 1u) != 0);
      w = lane == 2u * r ? static_cast<uint32_t>(u) : lane == 2u * r + 1u ? static_cast<uint32_t>(u >> 32) : w;
    }
    // d = u G_N: d[i] ^= d[i + t] for the i with bit t clear, t = 1 .. N / 2. Words past N / 32 are zero, so the
    // cross-word stages past N leave the words unchanged.
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
    // Gold sequence words: the scrambler's, then the DM-RS words of each CORESET symbol that the DCI's PRBs read.
    const uint32_t nw_data = (18u * nof_prb * duration + 31u) >> 5;  // E: nine REs of two bits per PRB and symbol
    const uint32_t nw_dmrs = d.dmrs_nof_words;
    for (uint32_t i = tid - 64u; i < nw_data + duration * nw_dmrs; i += PDCCH_THREADS - 64u) {
      if (i < nw_data) {
        gold_data[i] = gold_word(d.c_init_data, i, 0, x1, x2_jump, x2_lane);
      } else {
        const uint32_t j = i - nw_data, s = j / nw_dmrs, k = j - s * nw_dmrs;
        gold_dmrs[s][k]  = gold_word(d.c_init_dmrs[s], d.dmrs_word0 + k, 0, x1, x2_jump, x2_lane);
      }
    }
    for (uint32_t i = tid - 64u; i < nof_prb; i += PDCCH_THREADS - 64u) {
      prb_list[i] = prbs[d.prb_offset + i];
    }
  }
  __syncthreads();

  const uint32_t P = d.nof_ports;
  const float    a = d.data_amplitude, ad = d.dmrs_amplitude;
  float          wr[4], wi[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    wr[p] = d.w[p][0];
    wi[p] = d.w[p][1];
  }
  // Item t: symbol s, the DCI's PRB number i, subcarrier k of the PRB.
  for (uint32_t t = tid; t < 12u * nof_prb * duration; t += PDCCH_THREADS) {
    const uint32_t pi  = t / 12u, k = t - 12u * pi;
    const uint32_t s   = pi / nof_prb, i = pi - s * nof_prb;
    const uint32_t prb = prb_list[i];
    float          re, im;
    if ((k & 3u) == 1u) {
      // DM-RS: pilot k / 4 of the PRB, sequence bits 2 m and 2 m + 1 with m counted from the reference PRB.
      const uint32_t n    = 2u * (3u * (prb - d.reference_rb) + (k >> 2)) - 32u * d.dmrs_word0;
      const uint32_t word = gold_dmrs[s][n >> 5];
      const uint32_t sh   = 31u - (n & 31u);
      re                  = ((word >> sh) & 1u) ? -ad : ad;
      im                  = ((word >> (sh - 1u)) & 1u) ? -ad : ad;
    } else {
      // Data: RE r of the DCI in symbol-major, ascending subcarrier order carries rate-matched bits 2 r and 2 r + 1.
      const uint32_t rank = k - (k > 1u ? 1u : 0u) - (k > 5u ? 1u : 0u) - (k > 9u ? 1u : 0u);
      const uint32_t r    = (s * nof_prb + i) * 9u + rank;
      const uint32_t g    = gather[code.gather_offset + r];
      const uint32_t q0 = g & 0xffffu, q1 = g >> 16;
      const uint32_t word = gold_data[r >> 4];
      const uint32_t sh   = 31u - ((2u * r) & 31u);
      const uint32_t b0   = ((x_words[q0 >> 5] >> (q0 & 31u)) ^ (word >> sh)) & 1u;
      const uint32_t b1   = ((x_words[q1 >> 5] >> (q1 & 31u)) ^ (word >> (sh - 1u))) & 1u;
      re                  = b0 ? -a : a;
      im                  = b1 ? -a : a;
    }
    const uint32_t e = d.grid_base + s * d.nsc + prb * 12u + k;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (p < static_cast<int>(P)) {
        const float sr = re * wr[p] - im * wi[p];
        const float si = re * wi[p] + im * wr[p];
        grids[e + static_cast<uint32_t>(p) * d.port_stride] = bf16_bits(sr) | (bf16_bits(si) << 16);
      }
    }
  }
}

} // namespace

void launch_pdcch(const pdcch_desc*      d_descs,
                  uint32_t               nof_dcis,
                  const pdcch_code_desc* d_codes,
                  const uint8_t*         d_u_source,
                  const uint32_t*        d_gather,
                  const uint16_t*        d_prbs,
                  const uint32_t*        d_crc_weights,
                  const uint8_t*         d_payloads,
                  uint32_t*              d_grids,
                  const uint32_t*        d_x1,
                  const uint32_t*        d_x2_jump,
                  const uint32_t*        d_x2_lane,
                  hipStream_t            stream)
{
  if (nof_dcis == 0) {
    return;
  }
  hipLaunchKernelGGL(pdcch_kernel, dim3(nof_dcis), dim3(PDCCH_THREADS), 0, stream, d_descs, d_codes, d_u_source, d_gather,
                     d_prbs, d_crc_weights, d_payloads, d_grids, d_x1, d_x2_jump, d_x2_lane);
}

} // namespace srsgpu
