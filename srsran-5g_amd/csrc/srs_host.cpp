// Derived quantities, refusals, sequences and job descriptors of the SRS estimator plan; see srs_host.h.
#include "srs_host.h"
#include "host_util.h"
#include "low_papr_host.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace srsgpu {

namespace {

constexpr double T_C = 1.0 / (480000.0 * 4096.0);  // phy_time_unit::T_C

} // namespace

std::string srs_refusal(const srsgpu_srs_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports, uint32_t nof_grids,
                        uint32_t nof_resources, srs_derived& d)
{
  std::memset(&d, 0, sizeof(d));
  if (std::string why = numerology_refusal(c.numerology); !why.empty()) {
    return why;
  }
  if (c.nof_antenna_ports != 1 && c.nof_antenna_ports != 2 && c.nof_antenna_ports != 4) {
    return format("The number of antenna ports (i.e., %u) is not 1, 2 or 4.", c.nof_antenna_ports);
  }
  if (c.nof_symbols != 1 && c.nof_symbols != 2 && c.nof_symbols != 4) {
    return format("The number of symbols (i.e., %u) is not 1, 2 or 4.", c.nof_symbols);
  }
  if (c.comb_size != 2 && c.comb_size != 4) {
    return format("The comb size (i.e., %u) is not 2 or 4.", c.comb_size);
  }
  d.n_cs_max = c.comb_size == 4 ? 12 : 8;
  // srs_resource_configuration::is_valid.
  if (c.comb_offset >= c.comb_size) {
    return format("Invalid SRS resource configuration: comb offset %u with comb size %u.", c.comb_offset, c.comb_size);
  }
  if (c.cyclic_shift >= d.n_cs_max) {
    return format("Invalid SRS resource configuration: cyclic shift %u with comb size %u.", c.cyclic_shift, c.comb_size);
  }
  if (c.bandwidth_index > 3 || c.freq_hopping > 3) {
    return format("B_SRS %u or b_hop %u is outside 0..3", c.bandwidth_index, c.freq_hopping);
  }
  if (c.freq_hopping < c.bandwidth_index) {
    return "The SRS estimator does not support frequency hopping.";
  }
  if (c.hopping != 0) {
    return "The SRS estimator does not support group or sequence hopping.";
  }
  if (c.nof_rx_ports == 0) {
    return "Empty list of Rx ports for the SRS estimator.";
  }
  if (c.nof_rx_ports > SRS_MAX_PORTS) {
    return format("The number of receive ports (i.e., %u) exceeds 4", c.nof_rx_ports);
  }
  if (std::string why = rx_port_list_refusal(c.rx_ports, c.nof_rx_ports, grid_nof_ports); !why.empty()) {
    return why;
  }
  if (c.start_symbol + c.nof_symbols > 14u) {
    return format("The start symbol index (i.e., %u) plus the number of symbols (i.e., %u) exceeds the number of symbols "
                  "per slot (i.e., 14)", c.start_symbol, c.nof_symbols);
  }
  if (c.sequence_id > 1023 || c.freq_shift > 268 || c.freq_position > 67) {
    return format("sequence_id %u, freq_shift %u or freq_position %u is outside 0..1023, 0..268, 0..67", c.sequence_id,
                  c.freq_shift, c.freq_position);
  }
  // The row of TS 38.211 Table 6.4.1.4.3-1.
  for (uint32_t b = 0; b < 4; ++b) {
    if (c.m_srs[b] == 0 || c.m_srs[b] % 4 != 0 || c.m_srs[b] > 272 || c.N[b] == 0) {
      return format("Table row: m_srs[%u] = %u is no multiple of 4 in 4..272, or N[%u] = %u is zero", b, c.m_srs[b], b, c.N[b]);
    }
    if (b == 0 ? c.N[0] != 1 : static_cast<uint32_t>(c.m_srs[b]) * c.N[b] != c.m_srs[b - 1]) {
      return format("Table row: m_srs[%u] x N[%u] = %u x %u does not give the bandwidth above it", b, b, c.m_srs[b], c.N[b]);
    }
  }
  if (std::string why = grid_index_refusal(c.grid_index, nof_grids); !why.empty()) {
    return why;
  }
  if (c.result_index >= nof_resources) {
    return format("result_index %u is outside the %u resources", c.result_index, nof_resources);
  }

  const uint32_t comb = c.comb_size, nap = c.nof_antenna_ports;
  d.L           = c.m_srs[c.bandwidth_index] * 12u / comb;
  d.u           = c.sequence_id % 30u;
  d.interleaved = (nap == 4 && c.cyclic_shift >= d.n_cs_max / 2) ? 1 : 0;
  uint32_t sum  = 0;
  for (uint32_t b = 0; b <= c.bandwidth_index; ++b) {
    const uint32_t m_sc = c.m_srs[b] * 12u / comb;
    const uint32_t n_b  = ((4u * c.freq_position) / c.m_srs[b]) % c.N[b];
    sum += comb * m_sc * n_b;
  }
  for (uint32_t p = 0; p < nap; ++p) {
    d.n_cs[p]     = (c.cyclic_shift + (d.n_cs_max * p) / nap) % d.n_cs_max;
    uint32_t k_tc = c.comb_offset;
    if (d.interleaved != 0 && (p == 1 || p == 3)) {
      k_tc = (k_tc + comb / 2) % comb;
    }
    d.k0[p] = c.freq_shift * 12u + k_tc + sum;
    // The validator's bandwidth check, over the antenna ports.
    if (d.k0[p] + (d.L - 1) * comb >= 12u * grid_nof_prb) {
      return format("SRS resource exceeds maximum bandwidth: antenna port %u ends at subcarrier %u of %u.", p,
                    d.k0[p] + (d.L - 1) * comb, 12u * grid_nof_prb);
    }
  }

  // time_alignment_estimator_dft_impl::get_idft: guard-scaled size, next power of two, at least 128.
  const uint32_t scaled = d.L * 4096u / 3300u;
  d.M = 128, d.log2M = 7;
  while (d.M < scaled) {
    d.M <<= 1, ++d.log2M;
  }
  // estimate_ta_correlation, with the reference's double arithmetic in its order: the floors decide integers.
  const uint32_t khz       = 15u << c.numerology;
  const double   half_cp_s = static_cast<double>((144u * 64u) / (1u << (c.numerology + 1))) * T_C;
  d.fs                     = static_cast<double>(static_cast<uint64_t>(d.M) * khz * 1000u * comb);
  const double   max_ta    = 1.0 / static_cast<double>(d.n_cs_max * khz * 1000u * comb);
  d.max_ta_samples         = std::min(static_cast<uint32_t>(std::floor(half_cp_s * d.fs)),
                                      static_cast<uint32_t>(std::floor(max_ta * d.fs)));
  return {};
}

srs_job srs_make_job(const srsgpu_srs_config& c, const srs_derived& d, const uint32_t seq_rows[4], uint32_t grid_nof_prb,
                     uint32_t grid_nof_ports)
{
  srs_job j;
  std::memset(&j, 0, sizeof(j));
  const grid_geometry g(grid_nof_prb, grid_nof_ports, c.grid_index);
  j.nsc            = g.nsc;
  j.port_stride    = g.port_stride;
  j.grid_base      = g.grid_base;
  j.result_index   = c.result_index;
  j.L              = d.L;
  j.comb           = c.comb_size;
  j.M              = d.M;
  j.log2M          = d.log2M;
  j.max_ta_samples = d.max_ta_samples;
  j.nof_tx         = c.nof_antenna_ports;
  j.nof_rx         = c.nof_rx_ports;
  j.nof_symbols    = c.nof_symbols;
  j.start_symbol   = c.start_symbol;
  j.interleaved    = d.interleaved;
  j.khz            = 15u << c.numerology;
  j.fs             = d.fs;
  for (uint32_t p = 0; p < SRS_MAX_PORTS; ++p) {
    j.k0[p]       = d.k0[p < c.nof_antenna_ports ? p : 0];
    j.seq_row[p]  = seq_rows[p < c.nof_antenna_ports ? p : 0];
    j.rx_ports[p] = c.rx_ports[p < c.nof_rx_ports ? p : 0];
  }
  return j;
}

std::vector<float> srs_sequence(uint32_t u, uint32_t L, uint32_t n_cs, uint32_t n_cs_max)
{
  if (u >= 30 || n_cs_max == 0) {
    return {};
  }
  return low_papr_shifted_sequence(u, L, static_cast<uint64_t>(n_cs) * 24u / n_cs_max);  // generate(): alpha_num x 24 / alpha_den
}

} // namespace srsgpu
