// Host-side construction for the PUCCH Format 3 / 4 plan (capi_pucch_f34.cpp, pucch_f34.hip): what the reference's
// estimator and demodulators derive from a PDU before they touch a sample -- the DM-RS symbol mask and the hop
// geometry, the cyclically shifted low-PAPR DM-RS sequences, the scrambling words, the symbol start epochs, the
// Format 4 orthogonal sequences, the roots of the inverse transform -- the refusals and the job descriptors. No HIP
// call in this translation unit, so that a host-only program can check it (tools/pucch_f34_host_check.cpp).
//
// Reference (behaviour, not code): include/srsran/phy/upper/pucch_formats3_4_helpers.h:44 (DM-RS symbol mask),
// lib/phy/upper/signal_processors/pucch/dmrs_pucch_estimator_formats3_4.cpp:29 (m_0, cyclic shift) / :61 (hop split),
// lib/phy/upper/channel_processors/pucch/pucch_demodulator_format4.cpp:110 (block-wise despreading),
// include/srsran/phy/upper/pucch_orthogonal_sequence.h:162 (w_n), pucch_processor_impl.cpp:616 / :703 (validators),
// include/srsran/ran/pucch/pucch_info.h:80 / :104 (code rates),
// lib/phy/generic_functions/transform_precoding/transform_precoder_dft_impl.cpp:32 (1 / sqrt(M)).
#pragma once
#include "srsgpu_phy.h"
#include <cstdint>
#include <string>
#include <vector>

namespace srsgpu {

constexpr uint32_t PUCCH_F34_MAX_PRB     = 16;
constexpr uint32_t PUCCH_F34_MAX_RE      = 12 * PUCCH_F34_MAX_PRB;  ///< Points of the largest inverse transform.
constexpr uint32_t PUCCH_F34_MIN_SYMBOLS = 4;
constexpr uint32_t PUCCH_F34_MAX_SYMBOLS = 14;
constexpr uint32_t PUCCH_F34_MAX_DMRS    = 4;
constexpr uint32_t PUCCH_F34_MAX_DATA    = 12;
constexpr uint32_t PUCCH_F34_MAX_PORTS   = 4;
constexpr uint32_t PUCCH_F34_NO_HOP      = 0xffffu;

/// One workgroup's work: one PDU. Plain data, uploaded as it is.
struct pucch_f34_job {
  uint32_t grid_base;      ///< Word of (grid, port 0, symbol 0, subcarrier 0).
  uint32_t port_stride, nsc;
  uint32_t llr_offset, nof_llrs;
  uint32_t format;         ///< 3 or 4.
  uint32_t nof_prb, nof_ports, nof_hops;
  uint32_t nof_dmrs, nof_data;
  uint32_t pi2_bpsk;
  uint32_t sf;             ///< Format 4: the spreading factor (2 or 4); Format 3: 1.
  uint32_t scramble_word;  ///< First of the PDU's ceil(nof_llrs / 32) words in the scrambling table.
  uint32_t dmrs_row;       ///< Float2 element of the first DM-RS symbol's 12 nof_prb pilots; the others follow.
  uint32_t root_row;       ///< Float2 element of exp(+j 2 pi k / M), k = 0..M-1, M = 12 nof_prb, in the root table.
  uint32_t prb[2];         ///< First grid PRB of each hop.
  float    idft_scale;     ///< 1 / sqrt(M) in float.
  float    scs_hz;
  float    cfo_delta[2];   ///< Per hop: start epoch of its second DM-RS symbol minus the first's (1 when it has one).
  uint8_t  hop_first_dmrs[2], hop_nof_dmrs[2];  ///< Per hop: into dmrs_symbol.
  uint8_t  dmrs_symbol[PUCCH_F34_MAX_DMRS];     ///< Symbol of the slot of each DM-RS symbol.
  uint8_t  data_symbol[PUCCH_F34_MAX_DATA];     ///< Symbol of the slot of each data symbol, in order,
  uint8_t  data_hop[PUCCH_F34_MAX_DATA];        ///< and the hop it lies in.
  uint8_t  w_quarter[12];  ///< Format 4: 1 / w_n(k) = j^w_quarter[k]; Format 3: zeros.
  uint8_t  ports[4];
};
static_assert(sizeof(pucch_f34_job) == 136,"pucch_f34_job is copied by words");

/// TS 38.211 Table 6.4.1.3.3.2-1: bit i set = the i-th allocated symbol carries DM-RS. 0 outside 4..14 symbols.
uint32_t pucch_f34_dmrs_mask(uint32_t nof_symbols, bool hopping, bool additional_dmrs);

/// The modulated symbols of the PDU: 12 nof_prb per data symbol for Format 3, 12 / occ_length for Format 4.
uint32_t pucch_f34_nof_llrs(const srsgpu_pucch_f34_config& c);

/// transform_precoding::is_nof_prbs_valid: 2^a 3^b 5^c.
bool pucch_f34_transform_size_ok(uint32_t nof_prb);

/// pucch_format3_code_rate / pucch_format4_code_rate in float. Format 4 as the reference computes it: E_UCI is divided
/// by the spreading factor, the channel bits in the denominator are not.
float pucch_f34_code_rate(const srsgpu_pucch_f34_config& c);

/// The one reason the PDU is refused; empty when it is accepted.
std::string pucch_f34_refusal(const srsgpu_pucch_f34_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports,
                              uint32_t nof_grids);

/// The reason two PDUs' LLR ranges overlap ("PDU i ... PDU j"); empty when none do.
std::string pucch_f34_llr_overlap(const srsgpu_pucch_f34_config* cfgs, uint32_t nof_pdus);

/// r_{u,0}^{(alpha)}(n) of the PDU's DM-RS symbol at `symbol` of the slot, n = 0..12 nof_prb - 1, as (re, im) floats
/// evaluated in double: u = n_id_hopping mod 30, alpha = 2 pi ((m_0 + n_cs(slot, symbol)) mod 12) / 12.
std::vector<float> pucch_f34_dmrs(const srsgpu_pucch_f34_config& c, uint32_t symbol);

/// Scrambling bits c(32 w + b) of c_init = rnti 2^15 + n_id_scrambling as bit b of word w, ceil(nof_bits / 32) words.
std::vector<uint32_t> pucch_f34_scrambling(const srsgpu_pucch_f34_config& c, uint32_t nof_bits);

/// TS 38.211 Tables 6.3.2.6.3-1 / -2: w_n(k), k = 0..11, as (re, im) floats; empty for another length or index.
std::vector<float> pucch_f4_w(uint32_t occ_length, uint32_t occ_index);

/// The job of an accepted PDU.
pucch_f34_job pucch_f34_make_job(const srsgpu_pucch_f34_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports,
                                 uint32_t dmrs_row, uint32_t root_row, uint32_t scramble_word);

} // namespace srsgpu
