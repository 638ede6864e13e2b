// Host-side construction for the PUCCH Format 2 plan (capi_pucch_f2.cpp, pucch_f2.hip): what the reference's estimator
// and demodulator derive from a PDU before they touch a sample -- the DM-RS symbols, the scrambling sequence, the
// resampled raised-cosine filter and its number of virtual pilots, the symbol start epochs, the hop geometry -- the
// refusals and the job descriptors. No HIP call in this translation unit, so that a host-only program can check it
// (tools/pucch_f2_host_check.cpp).
//
// Reference (behaviour, not code): lib/phy/upper/signal_processors/pucch/dmrs_pucch_estimator_format2.cpp:34 (c_init) /
// :43 (sequence advanced by 8 bits per PRB) / :58 (hop pattern), lib/phy/upper/signal_processors/
// port_channel_estimator_helpers.cpp:83 (filter) / :224 (virtual pilots), port_channel_estimator_average_impl.cpp:496
// (epochs), lib/phy/upper/channel_processors/pucch/pucch_demodulator_format2.cpp:157 (scrambling c_init),
// pucch_processor_impl.cpp:539 (validator), include/srsran/ran/pucch/pucch_info.h:57 (code rate).
#pragma once
#include "srsgpu_phy.h"
#include <cstdint>
#include <string>
#include <vector>

namespace srsgpu {

constexpr uint32_t PUCCH_F2_MAX_PRB     = 16;
constexpr uint32_t PUCCH_F2_MAX_SYMBOLS = 2;
constexpr uint32_t PUCCH_F2_MAX_PORTS   = 4;
constexpr uint32_t PUCCH_F2_MAX_TAPS    = 11;
constexpr uint32_t PUCCH_F2_MAX_V       = 12;   ///< port_channel_estimator_average_impl::MAX_V_PILOTS
constexpr uint32_t PUCCH_F2_DFT         = 128;  ///< The time alignment estimator's IDFT for up to 64 pilots.
constexpr uint32_t PUCCH_F2_TA_SAMPLES  = 13;   ///< Half a normal CP at 128 x SCS x 3, every numerology.
constexpr uint32_t PUCCH_F2_SCR_WORDS   = 16;   ///< 512 scrambling bits per PDU.
constexpr uint32_t PUCCH_F2_NO_HOP      = 0xffffu;

/// One workgroup's work: one PDU. Plain data, uploaded as it is.
struct pucch_f2_job {
  uint32_t grid_base;      ///< Word of (grid, port 0, symbol 0, subcarrier 0).
  uint32_t port_stride, nsc;
  uint32_t llr_offset;
  uint32_t nof_prb, nof_symbols, start_symbol, nof_ports;
  uint32_t hopping;        ///< 1: two hops of one symbol; 0: one hop of nof_symbols.
  uint32_t nof_taps, n_v;
  uint32_t scramble_word;  ///< First of the PDU's 16 words in the scrambling table.
  uint32_t prb[2];         ///< First grid PRB of each symbol.
  uint32_t dmrs_row[2];    ///< Float2 element of each symbol's 4 nof_prb pilots in the DM-RS table.
  uint32_t ports[4];
  float    taps[PUCCH_F2_MAX_TAPS];
  float    delta_epoch;    ///< Start epoch of the second symbol minus the first's, in symbol durations.
  float    scs_hz;
  uint32_t reserved;
  double   fs;             ///< 128 x subcarrier spacing x 3, Hz.
};
static_assert(sizeof(pucch_f2_job) == 144, "pucch_f2_job is copied by words");

/// pucch_format2_code_rate: payload and CRC bits over the channel bits, in float.
float pucch_f2_code_rate(uint32_t nof_prb, uint32_t nof_symbols, uint32_t nof_uci_bits);

/// The one reason the PDU is refused; empty when it is accepted.
std::string pucch_f2_refusal(const srsgpu_pucch_f2_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports,
                             uint32_t nof_grids);

/// The reason two PDUs' LLR ranges overlap ("PDU i ... PDU j"); empty when none do.
std::string pucch_f2_llr_overlap(const srsgpu_pucch_f2_config* cfgs, uint32_t nof_pdus);

/// filter_type(nof_prb, stride 3): the taps, renormalised in float as the reference does; returns their number
/// (3, 7 or 11) and sets n_v, the virtual pilots on either side.
uint32_t pucch_f2_filter(uint32_t nof_prb, float taps[PUCCH_F2_MAX_TAPS], uint32_t& n_v);

/// The 4 nof_prb DM-RS symbols of the PDU's i-th symbol as (re, im) floats of +-1/sqrt(2).
std::vector<float> pucch_f2_dmrs(const srsgpu_pucch_f2_config& c, uint32_t i);

/// Scrambling bits c(32 w + b) of c_init = rnti 2^15 + n_id as bit b of words[w].
void pucch_f2_scrambling(const srsgpu_pucch_f2_config& c, uint32_t words[PUCCH_F2_SCR_WORDS]);

/// The job of an accepted PDU.
pucch_f2_job pucch_f2_make_job(const srsgpu_pucch_f2_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports,
                               const uint32_t dmrs_rows[2], uint32_t scramble_word);

} // namespace srsgpu
