// Host-side construction for the PDCCH plan (capi_pdcch.cpp, pdcch.hip) that is not the polar code (polar_code.h): the
// reference's refusals and the CCE to PRB mapping. No HIP call in this translation unit, so that a host-only program
// can check it (tools/pdcch_code_check.cpp).
//
// Reference (behaviour, not code): lib/ran/pdcch/cce_to_prb_mapping.cpp (cce_to_prb_mapping_coreset0 /
// _non_interleaved / _interleaved), pdcch_processor_impl.cpp:44 (compute_rb_mask),
// pdcch_processor_validator_impl.cpp:27 (is_valid).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace srsgpu {

enum pdcch_mapping : uint32_t { PDCCH_CORESET0 = 0, PDCCH_NON_INTERLEAVED = 1, PDCCH_INTERLEAVED = 2 };

/// pdcch_processor::coreset_description and the DCI fields the mapping and the refusals read.
struct pdcch_alloc {
  uint32_t bwp_size_rb = 0, bwp_start_rb = 0;
  uint32_t start_symbol = 0, duration = 0;
  uint64_t frequency_resources = 0;  ///< Bit i: the 6-PRB frequency resource i (45 bits).
  uint32_t mapping = PDCCH_NON_INTERLEAVED;
  uint32_t reg_bundle_size = 0, interleaver_size = 0, shift_index = 0;
  uint32_t cce_index = 0, aggregation_level = 0;
  uint32_t nof_payload_bits = 0;
  uint32_t nof_ports = 0;
};

/// The one reason the reference (validator, then the polar code's limits, then the mapper's assertion) or the grid
/// refuses the DCI; empty when it is accepted.
std::string pdcch_refusal(const pdcch_alloc& a, uint32_t grid_nof_prb, uint32_t grid_nof_ports);

/// The PRBs of the DCI's CCEs in ascending order: the set bits of compute_rb_mask. For an allocation that
/// pdcch_refusal accepts up to the PRB check; 6 * aggregation_level / duration entries.
std::vector<uint16_t> pdcch_prbs(const pdcch_alloc& a);

} // namespace srsgpu
