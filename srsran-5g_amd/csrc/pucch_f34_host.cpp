// Derived quantities, refusals, sequences and job descriptors of the PUCCH Format 3 / 4 plan; see pucch_f34_host.h.
#include "pucch_f34_host.h"
#include "host_util.h"
#include "low_papr_host.h"
#include <cmath>
#include <cstring>

namespace srsgpu {

namespace {

bool hopping(const srsgpu_pucch_f34_config& c)
{
  return c.second_hop_prb != PUCCH_F34_NO_HOP;
}

uint32_t popcount(uint32_t v)
{
  uint32_t n = 0;
  for (; v != 0; v &= v - 1) {
    ++n;
  }
  return n;
}

uint32_t nof_data_symbols(const srsgpu_pucch_f34_config& c)
{
  return c.nof_symbols - popcount(pucch_f34_dmrs_mask(c.nof_symbols, hopping(c), c.additional_dmrs != 0));
}

} // namespace

uint32_t pucch_f34_dmrs_mask(uint32_t nof_symbols, bool hop, bool additional)
{
  auto bits = [](std::initializer_list<uint32_t> l) {
    uint32_t m = 0;
    for (uint32_t b : l) {
      m |= 1u << b;
    }
    return m;
  };
  switch (nof_symbols) {
    case 4:
      return hop ? bits({0, 2}) : bits({1});
    case 5:
      return bits({0, 3});
    case 6:
    case 7:
      return bits({1, 4});
    case 8:
      return bits({1, 5});
    case 9:
      return bits({1, 6});
    case 10:
      return additional ? bits({1, 3, 6, 8}) : bits({2, 7});
    case 11:
      return additional ? bits({1, 3, 6, 9}) : bits({2, 7});
    case 12:
      return additional ? bits({1, 4, 7, 10}) : bits({2, 8});
    case 13:
      return additional ? bits({1, 4, 7, 11}) : bits({2, 9});
    case 14:
      return additional ? bits({1, 5, 8, 12}) : bits({3, 10});
    default:
      return 0;
  }
}

uint32_t pucch_f34_nof_llrs(const srsgpu_pucch_f34_config& c)
{
  const uint32_t qm = c.pi2_bpsk ? 1u : 2u;
  if (c.format == 4) {
    return 12u * nof_data_symbols(c) * qm / c.occ_length;
  }
  return 12u * c.nof_prb * nof_data_symbols(c) * qm;
}

bool pucch_f34_transform_size_ok(uint32_t nof_prb)
{
  if (nof_prb == 0) {
    return false;
  }
  for (uint32_t p : {2u, 3u, 5u}) {
    while (nof_prb % p == 0) {
      nof_prb /= p;
    }
  }
  return nof_prb == 1;
}

float pucch_f34_code_rate(const srsgpu_pucch_f34_config& c)
{
  const uint32_t n_data = nof_data_symbols(c);
  const uint32_t per_re = c.pi2_bpsk ? 12u : 24u;
  const uint32_t e_uci  = c.format == 4 ? per_re * n_data / c.occ_length : per_re * n_data * c.nof_prb;
  const uint32_t ncb    = uci_nof_codeblocks(c.nof_uci_bits, e_uci);
  // pucch_info.h:116: the Format 4 channel bits are 12 n_data Qm, not divided by the spreading factor.
  const uint32_t channel_bits = (c.format == 4 ? 1u : c.nof_prb) * 12u * n_data * (c.pi2_bpsk ? 1u : 2u);
  return static_cast<float>(c.nof_uci_bits + ncb * uci_crc_size(c.nof_uci_bits)) / static_cast<float>(channel_bits);
}

std::string pucch_f34_refusal(const srsgpu_pucch_f34_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports,
                              uint32_t nof_grids)
{
  if (c.format != 3 && c.format != 4) {
    return format("format %u is neither 3 nor 4", c.format);
  }
  if (std::string why = slot_refusal(c.numerology, c.cp_extended, c.slot_index); !why.empty()) {
    return why;
  }
  if (c.additional_dmrs > 1 || c.pi2_bpsk > 1) {
    return format("additional_dmrs %u and pi2_bpsk %u are flags (0 or 1)", c.additional_dmrs, c.pi2_bpsk);
  }
  if (c.nof_symbols < PUCCH_F34_MIN_SYMBOLS || c.nof_symbols > PUCCH_F34_MAX_SYMBOLS) {
    return format("Invalid Number of OFDM symbols allocated to PUCCH Format %u, i.e., %u. Valid range is 4 to 14.",
                  c.format, c.nof_symbols);
  }
  if (c.format == 3) {
    if (c.nof_prb < 1 || c.nof_prb > PUCCH_F34_MAX_PRB) {
      return format("Number of PRBs (i.e., %u) is outside the allowed range for PUCCH Format 3 (i.e., 1 to 16).", c.nof_prb);
    }
    if (!pucch_f34_transform_size_ok(c.nof_prb)) {
      return format("The number of PRB (i.e., %u) is not valid for the transform precoder: not of the form 2^a 3^b 5^c.",
                    c.nof_prb);
    }
  } else {
    if (c.nof_prb != 1) {
      return format("PUCCH Format 4 occupies one PRB (nof_prb %u)", c.nof_prb);
    }
    if (c.occ_length != 2 && c.occ_length != 4) {
      return format("Invalid OCC length value (i.e., %u). Valid values are 2 and 4.", c.occ_length);
    }
    if (c.occ_index >= c.occ_length) {
      return format("Invalid sequence index i = %u, valid values from 0 to %u.", c.occ_index, c.occ_length - 1u);
    }
  }
  if (c.starting_prb + c.nof_prb > grid_nof_prb) {
    return format("PUCCH Format %u: PRB allocation outside grid (first hop). Requested [%u, %u), grid has %u PRBs.",
                  c.format, c.starting_prb, c.starting_prb + c.nof_prb, grid_nof_prb);
  }
  if (hopping(c) && c.second_hop_prb + c.nof_prb > grid_nof_prb) {
    return format("PUCCH Format %u: PRB allocation outside grid (second hop). Requested [%u, %u), grid has %u PRBs.",
                  c.format, c.second_hop_prb, c.second_hop_prb + c.nof_prb, grid_nof_prb);
  }
  if (std::string why = symbol_allocation_refusal(c.start_symbol_index, c.nof_symbols, c.cp_extended); !why.empty()) {
    return why;
  }
  if (std::string why = rx_ports_refusal(c.ports, c.nof_ports, grid_nof_ports, PUCCH_F34_MAX_PORTS); !why.empty()) {
    return why;
  }
  // The validators check the code rate before the payload size (pucch_processor_impl.cpp:677 / :686, :764 / :773).
  const float rate = pucch_f34_code_rate(c);
  if (rate > 0.80F) {
    return format("The effective code rate (i.e., %f) exceeds the maximum allowed 0.8.", static_cast<double>(rate));
  }
  if (c.nof_uci_bits < 3 || c.nof_uci_bits > 1706) {
    return format("UCI Payload length (i.e., %u) is outside the supported range (i.e., 3 to 1706).", c.nof_uci_bits);
  }
  if (c.n_id_scrambling > 1023 || c.n_id_hopping > 1023) {
    return format("n_id_scrambling %u or n_id_hopping %u is outside 0..1023", c.n_id_scrambling, c.n_id_hopping);
  }
  if (std::string why = grid_index_refusal(c.grid_index, nof_grids); !why.empty()) {
    return why;
  }
  return llr_offset_refusal(c.llr_offset, pucch_f34_nof_llrs(c));
}

std::string pucch_f34_llr_overlap(const srsgpu_pucch_f34_config* cfgs, uint32_t nof_pdus)
{
  std::vector<uint32_t> offsets(nof_pdus), lengths(nof_pdus);
  for (uint32_t i = 0; i < nof_pdus; ++i) {
    offsets[i] = cfgs[i].llr_offset;
    lengths[i] = pucch_f34_nof_llrs(cfgs[i]);
  }
  return llr_overlap(offsets.data(), lengths.data(), nof_pdus);
}

std::vector<float> pucch_f34_dmrs(const srsgpu_pucch_f34_config& c, uint32_t symbol)
{
  static const uint32_t m0_of_occ[4] = {0, 6, 3, 9};  // TS 38.211 Table 6.4.1.3.3.1-1
  const uint32_t        m0    = c.format == 4 ? m0_of_occ[c.occ_index & 3u] : 0u;
  const uint32_t        alpha = (m0 + pucch_n_cs(c.n_id_hopping, pucch_nsymb_per_slot(c.cp_extended), c.slot_index, symbol)) % 12u;
  // alpha 12ths of a turn per element are 2 alpha 24ths.
  return low_papr_shifted_sequence(c.n_id_hopping % 30u, 12u * c.nof_prb, 2u * alpha);
}

std::vector<uint32_t> pucch_f34_scrambling(const srsgpu_pucch_f34_config& c, uint32_t nof_bits)
{
  return gold_words(static_cast<uint32_t>(c.rnti) * (1u << 15) + c.n_id_scrambling, (nof_bits + 31u) / 32u);
}

std::vector<float> pucch_f4_w(uint32_t occ_length, uint32_t occ_index)
{
  // The tables' entries as quarter turns: w_n(k) = j^q. Table 6.3.2.6.3-1 (N_SF = 2) and -2 (N_SF = 4).
  static const uint8_t sf2[2][12] = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 2, 2}};
  static const uint8_t sf4[4][12] = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
                                     {0, 0, 0, 3, 3, 3, 2, 2, 2, 1, 1, 1},
                                     {0, 0, 0, 2, 2, 2, 0, 0, 0, 2, 2, 2},
                                     {0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3}};
  static const float   re[4] = {1.0F, 0.0F, -1.0F, 0.0F}, im[4] = {0.0F, 1.0F, 0.0F, -1.0F};
  std::vector<float>   out;
  if (!((occ_length == 2 || occ_length == 4) && occ_index < occ_length)) {
    return out;
  }
  const uint8_t* q = occ_length == 2 ? sf2[occ_index] : sf4[occ_index];
  for (uint32_t k = 0; k < 12; ++k) {
    out.push_back(re[q[k]]);
    out.push_back(im[q[k]]);
  }
  return out;
}

pucch_f34_job pucch_f34_make_job(const srsgpu_pucch_f34_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports,
                                 uint32_t dmrs_row, uint32_t root_row, uint32_t scramble_word)
{
  pucch_f34_job j;
  std::memset(&j, 0, sizeof(j));
  const grid_geometry g(grid_nof_prb, grid_nof_ports, c.grid_index);
  j.nsc           = g.nsc;
  j.port_stride   = g.port_stride;
  j.grid_base     = g.grid_base;
  j.llr_offset    = c.llr_offset;
  j.nof_llrs      = pucch_f34_nof_llrs(c);
  j.format        = c.format;
  j.nof_prb       = c.nof_prb;
  j.nof_ports     = c.nof_ports;
  j.nof_hops      = hopping(c) ? 2u : 1u;
  j.pi2_bpsk      = c.pi2_bpsk;
  j.sf            = c.format == 4 ? c.occ_length : 1u;
  j.scramble_word = scramble_word;
  j.dmrs_row      = dmrs_row;
  j.root_row      = root_row;
  j.prb[0]        = c.starting_prb;
  j.prb[1]        = hopping(c) ? c.second_hop_prb : c.starting_prb;
  j.idft_scale    = 1.0F / std::sqrt(static_cast<float>(12u * c.nof_prb));
  j.scs_hz        = static_cast<float>((15u << c.numerology) * 1000u);
  // The second hop starts at nof_symbols / 2: with an odd count it is the longer one.
  const uint32_t mask = pucch_f34_dmrs_mask(c.nof_symbols, hopping(c), c.additional_dmrs != 0);
  const uint32_t half = hopping(c) ? c.nof_symbols / 2u : c.nof_symbols;
  j.hop_first_dmrs[0] = j.hop_first_dmrs[1] = 0;
  for (uint32_t i = 0; i < c.nof_symbols; ++i) {
    const uint32_t hop = i >= half ? 1u : 0u;
    if ((mask >> i) & 1u) {
      if (j.hop_nof_dmrs[hop] == 0) {
        j.hop_first_dmrs[hop] = static_cast<uint8_t>(j.nof_dmrs);
      }
      ++j.hop_nof_dmrs[hop];
      j.dmrs_symbol[j.nof_dmrs++] = static_cast<uint8_t>(c.start_symbol_index + i);
    } else {
      j.data_hop[j.nof_data]      = static_cast<uint8_t>(hop);
      j.data_symbol[j.nof_data++] = static_cast<uint8_t>(c.start_symbol_index + i);
    }
  }
  const std::vector<float> ep = symbol_epochs(c.numerology, c.cp_extended != 0);
  for (uint32_t hop = 0; hop < 2; ++hop) {
    j.cfo_delta[hop] = 1.0F;
    if (j.hop_nof_dmrs[hop] >= 2) {
      const uint32_t d0 = j.hop_first_dmrs[hop];
      j.cfo_delta[hop]  = ep[j.dmrs_symbol[d0 + 1]] - ep[j.dmrs_symbol[d0]];
    }
  }
  if (c.format == 4) {
    // 1 / w_n(k) = conj(w_n(k)): the quarter turns negated.
    const std::vector<float> w = pucch_f4_w(c.occ_length, c.occ_index);
    for (uint32_t k = 0; k < 12; ++k) {
      const int q    = w[2 * k] > 0.5F ? 0 : w[2 * k + 1] > 0.5F ? 1 : w[2 * k] < -0.5F ? 2 : 3;
      j.w_quarter[k] = static_cast<uint8_t>((4 - q) & 3);
    }
  }
  for (uint32_t p = 0; p < PUCCH_F34_MAX_PORTS; ++p) {
    j.ports[p] = c.ports[p < c.nof_ports ? p : 0];
  }
  return j;
}

} // namespace srsgpu
