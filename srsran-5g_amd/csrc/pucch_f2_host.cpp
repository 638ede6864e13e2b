// Derived quantities, refusals, sequences and job descriptors of the PUCCH Format 2 plan; see pucch_f2_host.h.
#include "pucch_f2_host.h"
#include "host_util.h"
#include "rc_filter_host.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace srsgpu {

namespace {

uint32_t symbol_prb(const srsgpu_pucch_f2_config& c, uint32_t i)
{
  return (i > 0 && c.second_hop_prb != PUCCH_F2_NO_HOP) ? c.second_hop_prb : c.starting_prb;
}

} // namespace

float pucch_f2_code_rate(uint32_t nof_prb, uint32_t nof_symbols, uint32_t nof_uci_bits)
{
  const uint32_t e_uci = 16u * nof_symbols * nof_prb;
  const uint32_t ncb   = uci_nof_codeblocks(nof_uci_bits, e_uci);
  return static_cast<float>(nof_uci_bits + ncb * uci_crc_size(nof_uci_bits)) / static_cast<float>(nof_prb * 8u * nof_symbols * 2u);
}

std::string pucch_f2_refusal(const srsgpu_pucch_f2_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports,
                             uint32_t nof_grids)
{
  if (std::string why = slot_refusal(c.numerology, c.cp_extended, c.slot_index); !why.empty()) {
    return why;
  }
  if (c.nof_prb < 1 || c.nof_prb > PUCCH_F2_MAX_PRB) {
    return format("Invalid Number of PRB allocated to PUCCH Format 2, i.e., %u. Valid range is 1 to 16.", c.nof_prb);
  }
  if (c.nof_symbols < 1 || c.nof_symbols > PUCCH_F2_MAX_SYMBOLS) {
    return format("Invalid Number of OFDM symbols allocated to PUCCH Format 2, i.e., %u. Valid range is 1 to 2.",
                  c.nof_symbols);
  }
  if (c.second_hop_prb != PUCCH_F2_NO_HOP && c.nof_symbols < 2) {
    return "Frequency hopping requires 2 OFDM symbols.";
  }
  if (c.starting_prb + c.nof_prb > grid_nof_prb) {
    return format("PUCCH Format 2: PRB allocation outside grid (first hop). Requested [%u, %u), grid has %u PRBs.",
                  c.starting_prb, c.starting_prb + c.nof_prb, grid_nof_prb);
  }
  if (c.second_hop_prb != PUCCH_F2_NO_HOP && c.second_hop_prb + c.nof_prb > grid_nof_prb) {
    return format("PUCCH Format 2: PRB allocation outside grid (second hop). Requested [%u, %u), grid has %u PRBs.",
                  c.second_hop_prb, c.second_hop_prb + c.nof_prb, grid_nof_prb);
  }
  if (std::string why = symbol_allocation_refusal(c.start_symbol_index, c.nof_symbols, c.cp_extended); !why.empty()) {
    return why;
  }
  if (std::string why = rx_ports_refusal(c.ports, c.nof_ports, grid_nof_ports, PUCCH_F2_MAX_PORTS); !why.empty()) {
    return why;
  }
  // The validator checks the code rate before the payload size (pucch_processor_impl.cpp:594 / :604).
  const float rate = pucch_f2_code_rate(c.nof_prb, c.nof_symbols, c.nof_uci_bits);
  if (rate > 0.80F) {
    return format("The effective code rate (i.e., %f) exceeds the maximum allowed 0.8.", static_cast<double>(rate));
  }
  if (c.nof_uci_bits < 3 || c.nof_uci_bits > 1706) {
    return format("UCI Payload length, i.e., %u is not supported. Payload length must be 3 to 1706 bits.", c.nof_uci_bits);
  }
  if (c.n_id > 1023) {
    return format("n_id %u is outside 0..1023", c.n_id);
  }
  if (std::string why = grid_index_refusal(c.grid_index, nof_grids); !why.empty()) {
    return why;
  }
  return llr_offset_refusal(c.llr_offset, 16u * c.nof_prb * c.nof_symbols);
}

std::string pucch_f2_llr_overlap(const srsgpu_pucch_f2_config* cfgs, uint32_t nof_pdus)
{
  std::vector<uint32_t> offsets(nof_pdus), lengths(nof_pdus);
  for (uint32_t i = 0; i < nof_pdus; ++i) {
    offsets[i] = cfgs[i].llr_offset;
    lengths[i] = 16u * cfgs[i].nof_prb * cfgs[i].nof_symbols;
  }
  return llr_overlap(offsets.data(), lengths.data(), nof_pdus);
}

uint32_t pucch_f2_filter(uint32_t nof_prb, float taps[PUCCH_F2_MAX_TAPS], uint32_t& n_v)
{
  const uint32_t nof_rbs = std::min(nof_prb, 3u);
  const uint32_t half    = (nof_rbs * 10u + 1u) / 2u / 3u;
  const uint32_t first   = 15u - half * 3u;
  const uint32_t count   = 2u * half + 1u;
  float          total   = 0;
  for (uint32_t i = 0; i < PUCCH_F2_MAX_TAPS; ++i) {
    taps[i] = 0.0F;
  }
  for (uint32_t i = 0; i < count; ++i) {
    taps[i] = static_cast<float>(rc_tap(static_cast<int>(first + 3u * i)));
    total += taps[i];
  }
  const float scale = 1 / total;
  for (uint32_t i = 0; i < count; ++i) {
    taps[i] *= scale;
  }
  n_v = nof_prb == 1 ? 4u : std::min(PUCCH_F2_MAX_V, count / 2u);
  return count;
}

std::vector<float> pucch_f2_dmrs(const srsgpu_pucch_f2_config& c, uint32_t i)
{
  const uint64_t nsymb  = pucch_nsymb_per_slot(c.cp_extended);
  const uint64_t n_id   = c.n_id_0;
  const uint64_t symbol = c.start_symbol_index + i;
  const uint32_t c_init = static_cast<uint32_t>(((nsymb * c.slot_index + symbol + 1) * (2 * n_id + 1) * (1ull << 17) + 2 * n_id) %
                                                (1ull << 31));
  const uint32_t       n = 8u * c.nof_prb;
  std::vector<uint8_t> bits(n);
  gold_bits(c_init, 8u * symbol_prb(c, i), n, bits.data());
  const float        a = static_cast<float>(M_SQRT1_2);
  std::vector<float> out(n);
  for (uint32_t k = 0; k < n; ++k) {
    out[k] = bits[k] ? -a : a;
  }
  return out;
}

void pucch_f2_scrambling(const srsgpu_pucch_f2_config& c, uint32_t words[PUCCH_F2_SCR_WORDS])
{
  const std::vector<uint32_t> w = gold_words(static_cast<uint32_t>(c.rnti) * (1u << 15) + c.n_id, PUCCH_F2_SCR_WORDS);
  std::copy(w.begin(), w.end(), words);
}

pucch_f2_job pucch_f2_make_job(const srsgpu_pucch_f2_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports,
                               const uint32_t dmrs_rows[2], uint32_t scramble_word)
{
  pucch_f2_job j;
  std::memset(&j, 0, sizeof(j));
  const grid_geometry g(grid_nof_prb, grid_nof_ports, c.grid_index);
  j.nsc           = g.nsc;
  j.port_stride   = g.port_stride;
  j.grid_base     = g.grid_base;
  j.llr_offset    = c.llr_offset;
  j.nof_prb       = c.nof_prb;
  j.nof_symbols   = c.nof_symbols;
  j.start_symbol  = c.start_symbol_index;
  j.nof_ports     = c.nof_ports;
  j.hopping       = c.second_hop_prb != PUCCH_F2_NO_HOP ? 1u : 0u;
  j.nof_taps      = pucch_f2_filter(c.nof_prb, j.taps, j.n_v);
  j.scramble_word = scramble_word;
  for (uint32_t i = 0; i < 2; ++i) {
    j.prb[i]      = symbol_prb(c, i);
    j.dmrs_row[i] = dmrs_rows[i < c.nof_symbols ? i : 0];
  }
  for (uint32_t p = 0; p < PUCCH_F2_MAX_PORTS; ++p) {
    j.ports[p] = c.ports[p < c.nof_ports ? p : 0];
  }
  const std::vector<float> ep = symbol_epochs(c.numerology, c.cp_extended != 0);
  j.delta_epoch = c.nof_symbols == 2 ? ep[c.start_symbol_index + 1] - ep[c.start_symbol_index] : 1.0F;
  j.scs_hz      = static_cast<float>((15u << c.numerology) * 1000u);
  j.fs          = static_cast<double>(static_cast<uint64_t>(PUCCH_F2_DFT) * (15u << c.numerology) * 1000u * 3u);
  return j;
}

} // namespace srsgpu
