// Host-side construction for the SRS estimator plan (capi_srs.cpp, srs_estimator.hip): what the estimator derives from
// a resource before it touches a sample (TS 38.211 section 6.4.1.4: the sequence length, each antenna port's cyclic
// shift and initial subcarrier, the interleaved case; the IDFT size, sampling rate and search range of the time
// alignment estimator), the refusals, the sequences with their cyclic shift, the phase table and the job descriptors.
// No HIP call in this translation unit, so that a host-only program can check it (tools/srs_host_check.cpp).
//
// Reference (behaviour, not code): lib/ran/srs/srs_information.cpp:38 (per-port information),
// lib/phy/upper/signal_processors/srs/srs_estimator_generic_impl.cpp:109 (max_ta) / :133 (interleaved pilots),
// srs_validator_generic_impl.cpp:30 (validator), include/srsran/ran/srs/srs_resource_configuration.h:142 (is_valid),
// lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.cpp:226 (IDFT size) / :250-263 (search
// range), lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.cpp:243 (sequence and cyclic shift).
#pragma once
#include "srsgpu_phy.h"
#include <cstdint>
#include <string>
#include <vector>

namespace srsgpu {

constexpr uint32_t SRS_MAX_L      = 1632;  ///< 272 PRBs, comb 2.
constexpr uint32_t SRS_MAX_M      = 2048;  ///< IDFT size of SRS_MAX_L.
constexpr uint32_t SRS_CEXP_SIZE  = 1024;  ///< srs_estimator_generic_impl.h:63.
constexpr uint32_t SRS_MAX_PORTS  = 4;

/// What estimate() computes with before it touches a sample.
struct srs_derived {
  uint32_t L;               ///< Sequence length m_SRS,B 12 / K_TC.
  uint32_t n_cs_max;        ///< 8 (comb 2) or 12 (comb 4).
  uint32_t u;               ///< Sequence group n_ID mod 30 (v = 0).
  uint32_t interleaved;     ///< 4 antenna ports and cyclic shift >= n_cs_max / 2: ports 1 and 3 on the other comb.
  uint32_t n_cs[4];         ///< Cyclic shift per antenna port.
  uint32_t k0[4];           ///< Initial grid subcarrier per antenna port.
  uint32_t M, log2M;        ///< IDFT size of the time alignment estimator, 128..2048.
  uint32_t max_ta_samples;  ///< Taps searched on either side.
  double   fs;              ///< M x subcarrier spacing x comb, Hz.
};

/// One workgroup's work: one resource. Plain data, uploaded as it is.
struct srs_job {
  uint32_t grid_base;       ///< Word of (grid, port 0, symbol 0, subcarrier 0).
  uint32_t port_stride, nsc;
  uint32_t result_index;
  uint32_t L, comb, M, log2M, max_ta_samples;
  uint32_t nof_tx, nof_rx, nof_symbols, start_symbol, interleaved;
  uint32_t khz;             ///< Subcarrier spacing in kHz.
  uint32_t reserved;
  uint32_t k0[4];
  uint32_t seq_row[4];      ///< Float2 element of each antenna port's sequence in the sequence table.
  uint32_t rx_ports[4];
  double   fs;
};
static_assert(sizeof(srs_job) == 120, "srs_job is copied by words");

/// The one reason the resource is refused; empty when it is accepted (then d holds its derived quantities).
std::string srs_refusal(const srsgpu_srs_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports, uint32_t nof_grids,
                        uint32_t nof_resources, srs_derived& d);

/// The job of an accepted resource; seq_rows[p] is the table element of antenna port p's sequence.
srs_job srs_make_job(const srsgpu_srs_config& c, const srs_derived& d, const uint32_t seq_rows[4], uint32_t grid_nof_prb,
                     uint32_t grid_nof_ports);

/// r(n) e^{j 2 pi n_cs n / n_cs_max}, n = 0..L-1, as (re, im) floats evaluated in double: the base sequence of group u
/// (v = 0) times the cyclic shift, which the reference takes from a 24-entry table at (n n_cs 24 / n_cs_max) mod 24.
/// Empty for a length the specification does not define.
std::vector<float> srs_sequence(uint32_t u, uint32_t L, uint32_t n_cs, uint32_t n_cs_max);

} // namespace srsgpu
