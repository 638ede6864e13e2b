// Host-side construction for the SS/PBCH block plan (capi_ssb.cpp, ssb.hip) that is not the polar code (polar_code.h):
// the refusals, l_start and k_start (TS 38.213 section 4.1, TS 38.211 section 7.4.3.1), the PBCH payload layout and the
// first scrambling (TS 38.212 sections 7.1.1, 7.1.2), the PBCH DM-RS c_init and the PSS / SSS m-sequences (TS 38.211
// sections 7.4.1.4.1, 7.4.2.2.1, 7.4.2.3.1). No HIP call in this translation unit, so that a host-only program can check
// it (tools/ssb_host_check.cpp).
//
// Reference (behaviour, not code): lib/phy/upper/channel_processors/ssb/ssb_processor_impl.cpp:29 (process),
// pbch_encoder_impl.cpp:41 (payload) / :80 (scrambling), include/srsran/ran/ssb/ssb_mapping.h:42 (ssb_get_l_first) /
// :116 (ssb_get_k_first), signal_processors/dmrs_pbch_processor_impl.cpp:29 (c_init),
// include/srsran/phy/upper/sequence_generators/pss_sequence_generator.h, sss_sequence_generator.h.
#pragma once
#include <cstdint>
#include <string>

namespace srsgpu {

constexpr uint32_t SSB_PBCH_BITS   = 864;  ///< E: 432 QPSK symbols.
constexpr uint32_t SSB_PBCH_K      = 56;   ///< 32 payload bits and CRC24C.
constexpr uint32_t SSB_POLAR_N     = 512;
constexpr uint32_t SSB_DYNAMIC_NONE = 0xff;

/// ssb_processor::pdu_t without the payload and the SFN, which the kernel reads from device memory.
struct ssb_block {
  uint32_t phys_cell_id = 0, ssb_idx = 0, L_max = 0;
  uint32_t pattern_case = 0;  ///< 0..4 = cases A..E.
  uint32_t common_scs   = 0;  ///< subCarrierSpacingCommon as a numerology (0..4).
  uint32_t offset_to_pointA = 0, subcarrier_offset = 0;
  uint32_t slot_index = 0;  ///< Within the half frame, in slots of the block's SCS.
  uint32_t hrf        = 0;
  uint32_t nof_ports  = 0;
  uint8_t  ports[4]   = {};
  float    pss_amplitude = 1.f;
};

/// One block as the kernel reads it (ssb.hip). Bit i of a 32-bit PBCH mask is a_i of TS 38.212 section 7.1.1; bit
/// n % 32 of word n / 32 of a sequence mask is set where d(n) = -1.
struct ssb_desc {
  uint32_t payload_offset;  ///< Bytes: three of payload, MSB first, and sfn & 15.
  uint32_t a_const;         ///< The bits of a that the plan fixes: HRF and the block index or the k_SSB bit.
  uint32_t scramble[4];     ///< The first scrambling's mask for v = 0..3, zero on the unscrambled positions.
  uint32_t c_init_data, data_word0;  ///< Second scrambling: N_id, advanced by (ssb_idx & 7) 864 bits = 27 words each.
  uint32_t c_init_dmrs;
  uint32_t pss[4], sss0[4], sss1[4];
  uint32_t grid_base;  ///< Word of (port 0, l_start, k_start) in the block's grid.
  uint32_t nsc, port_stride;
  float    pss_amplitude;
  uint16_t v;          ///< N_id mod 4: the DM-RS subcarriers v, v + 4, v + 8 of an RB.
  uint16_t nof_ports;
  uint8_t  ports[4];
};
static_assert(sizeof(ssb_desc) == 108, "ssb_desc layout");

/// What every block shares. dyn_source[i]: which of the 28 bits read at execution a_i is (0..23 the payload, MSB
/// first; 24..27 the 4th..1st LSB of the SFN), or SSB_DYNAMIC_NONE where the plan fixes a_i. v_hi / v_lo: the positions
/// in a of the 3rd and 2nd LSB of the SFN, which select the first scrambling's offset.
struct ssb_tables {
  uint8_t  u_source[SSB_POLAR_N];       ///< polar_dl_code::u_source of (56, 864).
  uint32_t gather[SSB_PBCH_BITS / 2];   ///< gather[2 r] | gather[2 r + 1] << 16.
  uint32_t crc_weights[32];             ///< x^(24 + j) mod g_CRC24C.
  uint8_t  dyn_source[32];
  uint32_t v_hi, v_lo;
};

/// The one reason the reference's assertions, the grid or the port list refuse the block; empty when it is accepted.
std::string ssb_refusal(const ssb_block& b, uint32_t grid_nof_prb, uint32_t grid_nof_ports);

/// First symbol of candidate block ssb_idx in the half frame (TS 38.213 section 4.1); pattern_case <= 4 and
/// ssb_idx < 64.
uint32_t ssb_l_first(uint32_t pattern_case, uint32_t ssb_idx);

/// First subcarrier of the block from point A, in subcarriers of the block's SCS (TS 38.211 section 7.4.3.1); false
/// when the offsets give no integer subcarrier. For a block whose fields passed the range checks of ssb_refusal.
bool ssb_k_first(const ssb_block& b, uint32_t& k_first);

/// Everything of the descriptor but payload_offset and the grid fields, for an accepted block.
void ssb_fill_desc(const ssb_block& b, ssb_desc& d);

/// dyn_source, v_hi, v_lo and crc_weights (the code tables come from polar_dl_code_build).
void ssb_fill_tables(ssb_tables& t);

} // namespace srsgpu
