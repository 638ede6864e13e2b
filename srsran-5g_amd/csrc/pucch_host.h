// Host-side construction for the PUCCH Format 0 / 1 detector plan (capi_pucch.cpp, pucch_detector.hip): the refusals,
// the Format 0 candidate tables and thresholds, the Format 1 hop split and thresholds, and the orthogonal sequences;
// the cyclic shift hopping n_cs (pucch_n_cs) is in host_util.h. No HIP call in this translation unit, so that a host-only program can check it
// (tools/pucch_host_check.cpp).
//
// Reference (behaviour, not code): include/srsran/phy/upper/pucch_helper.h:52 (u, v) / :81 (alpha index),
// lib/phy/upper/channel_processors/pucch/pucch_detector_format0.cpp:46 (tables) / :69 (thresholds),
// pucch_detector_format1.cpp:57 (validate_config) / :194 (thresholds) / :519 (hop split),
// pucch_processor_impl.cpp:404 / :482 (validators), include/srsran/phy/upper/pucch_orthogonal_sequence.h:43.
#pragma once
#include "srsgpu_phy.h"
#include <cstdint>
#include <string>
#include <vector>

namespace srsgpu {

constexpr uint32_t PUCCH_NO_HOP         = 0xffff;
constexpr uint32_t PUCCH_MAX_SYMBOLS    = 14;
constexpr uint32_t PUCCH_F1_MAX_ENTRIES = 84;
constexpr uint32_t PUCCH_W_TABLE_FLOATS = 7 * 7 * 7 * 2;  ///< w[N - 1][i][m] as (re, im).

/// One wavefront's work: a Format 0 PDU or a Format 1 resource. Plain data, uploaded as it is.
struct pucch_job {
  uint32_t kind;           ///< 0: Format 0, 1: Format 1.
  uint32_t result_offset;  ///< First result of the job (Format 1: of its first entry).
  uint32_t sym_base[PUCCH_MAX_SYMBOLS];  ///< Per allocated symbol: element of (port 0, symbol, first subcarrier of the PRB).
  uint32_t port_stride;
  uint32_t first_entry;    ///< Format 1: into the entry words (cyclic shift | OCC << 8 | nof_harq_ack << 16).
  uint32_t nof_entries;
  float    threshold;
  uint8_t  alpha[PUCCH_MAX_SYMBOLS];  ///< Per allocated symbol: (m0 + n_cs) mod 12 (Format 1: m0 = 0).
  uint8_t  phi3[12];       ///< (3 phi(n) + 24) mod 24 of the base sequence u, v = 0: its phase in units of 2 pi / 24.
  uint8_t  ports[4];
  uint8_t  nof_symbols, nof_ports, nof_hops, nof_candidates;
  uint8_t  m_cs[8];        ///< Format 0: the candidates in the reference's table order,
  uint8_t  message[8];     ///< and their messages: bit 0 SR, bit 1 and 2 the HARQ-ACK bits.
  uint8_t  hop_first[2], hop_nof_symbols[2], hop_nof_data[2], hop_nof_dmrs[2];  ///< Format 1, in allocated symbols.
  uint16_t dmrs_mask;      ///< Format 1: bit i set = allocated symbol i carries DM-RS.
  uint8_t  occ_mask;       ///< Format 1: bit i set = an entry has OCC i.
  uint8_t  reserved;
};

/// pick_threshold (pucch_detector_format0.cpp:69): std::lower_bound over (ports x symbols, sequences) pairs in
/// lexicographic order, so 3 ports x 1 symbol takes the (4, 1) entry whatever the number of sequences. 0 past the table.
float pucch_f0_threshold(uint32_t nof_ports, uint32_t nof_symbols, uint32_t nof_sequences);

/// pucch_detector_format1.cpp:197: by ports x hops; 0 for a count the reference terminates on.
float pucch_f1_threshold(uint32_t nof_contributions);

/// The Format 0 candidates (m_cs, message) of the payload in the reference's table order; the count (0: no payload).
uint32_t pucch_f0_candidates(uint32_t nof_harq_ack, uint32_t sr_opportunity, uint8_t m_cs[8], uint8_t message[8]);

/// The symbol split of a Format 1 resource, in allocated symbols (0 = start_symbol_index).
struct pucch_f1_split {
  uint32_t nof_hops;
  uint32_t first[2], nof_symbols[2], nof_data[2], nof_dmrs[2];
  uint32_t dmrs_mask;
};
pucch_f1_split pucch_f1_hop_split(uint32_t nof_symbols, bool hopping);

/// The one reason the PDU / the resource is refused; empty when it is accepted.
std::string pucch_f0_refusal(const srsgpu_pucch_f0_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports, uint32_t nof_grids);
std::string pucch_f1_refusal(const srsgpu_pucch_f1_resource& r,
                             const srsgpu_pucch_f1_entry*    entries,
                             uint32_t                        total_entries,
                             uint32_t                        grid_nof_prb,
                             uint32_t                        grid_nof_ports,
                             uint32_t                        nof_grids);

/// The jobs of an accepted PDU / resource.
pucch_job pucch_f0_job(const srsgpu_pucch_f0_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports, uint32_t result_offset);
pucch_job pucch_f1_job(const srsgpu_pucch_f1_resource& r,
                       const srsgpu_pucch_f1_entry*    entries,
                       uint32_t                        grid_nof_prb,
                       uint32_t                        grid_nof_ports,
                       uint32_t                        result_offset);

/// TS 38.211 Table 6.3.2.4.1-2: w_i(m) = exp(j 2 pi phi(m) / N) for N = 1..7 at [(N - 1) * 49 + i * 7 + m], (re, im).
std::vector<float> pucch_w_table();

} // namespace srsgpu
