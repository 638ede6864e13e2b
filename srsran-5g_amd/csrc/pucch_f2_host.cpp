// Derived quantities, refusals, sequences and job descriptors of the PUCCH Format 2 plan; see pucch_f2_host.h.
#include "pucch_f2_host.h"
#include "rc_filter_host.h"
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace srsgpu {

namespace {

std::string format(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
std::string format(const char* fmt, ...)
{
  char    buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return buf;
}

constexpr double PI  = 3.14159265358979323846;
constexpr double T_C = 1.0 / (480000.0 * 4096.0);  // phy_time_unit::T_C

/// Bits c(first) .. c(first + count - 1) of the Gold sequence (TS 38.211 section 5.2.1, N_C = 1600).
void gold_bits(uint32_t c_init, uint32_t first, uint32_t count, uint8_t* out)
{
  uint32_t x1 = 1, x2 = c_init & 0x7fffffffu;  // bit i: x(n + i)
  for (uint32_t n = 0, end = 1600 + first + count; n < end; ++n) {
    if (n >= 1600 + first) {
      out[n - 1600 - first] = static_cast<uint8_t>((x1 ^ x2) & 1u);
    }
    const uint32_t f1 = ((x1 >> 3) ^ x1) & 1u;
    const uint32_t f2 = ((x2 >> 3) ^ (x2 >> 2) ^ (x2 >> 1) ^ x2) & 1u;
    x1                = (x1 >> 1) | (f1 << 30);
    x2                = (x2 >> 1) | (f2 << 30);
  }
}

uint32_t crc_size(uint32_t a)
{
  return a < 12 ? 0 : a < 20 ? 6 : 11;
}

uint32_t symbol_prb(const srsgpu_pucch_f2_config& c, uint32_t i)
{
  return (i > 0 && c.second_hop_prb != PUCCH_F2_NO_HOP) ? c.second_hop_prb : c.starting_prb;
}

} // namespace

float pucch_f2_code_rate(uint32_t nof_prb, uint32_t nof_symbols, uint32_t nof_uci_bits)
{
  const uint32_t e_uci = 16u * nof_symbols * nof_prb;
  const uint32_t ncb   = ((nof_uci_bits >= 360 && e_uci >= 1088) || nof_uci_bits >= 1013) ? 2u : 1u;
  return static_cast<float>(nof_uci_bits + ncb * crc_size(nof_uci_bits)) / static_cast<float>(nof_prb * 8u * nof_symbols * 2u);
}

std::string pucch_f2_refusal(const srsgpu_pucch_f2_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports,
                             uint32_t nof_grids)
{
  if (c.numerology > 4) {
    return format("numerology %u is outside 0..4", c.numerology);
  }
  if (c.cp_extended > 1 || (c.cp_extended == 1 && c.numerology != 2)) {
    return format("the extended cyclic prefix exists at numerology 2 only (numerology %u)", c.numerology);
  }
  if (c.slot_index >= (10u << c.numerology)) {
    return format("slot index %u is outside the frame of %u slots", c.slot_index, 10u << c.numerology);
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
  const uint32_t nsymb = c.cp_extended ? 12u : 14u;
  if (c.start_symbol_index + c.nof_symbols > nsymb) {
    return format("OFDM symbol allocation goes up to symbol %u, exceeding the number of symbols in the given slot with "
                  "%s CP, i.e., %u.", c.start_symbol_index + c.nof_symbols, c.cp_extended ? "extended" : "normal", nsymb);
  }
  if (c.nof_ports == 0) {
    return "The number of receive ports cannot be zero.";
  }
  if (c.nof_ports > grid_nof_ports || c.nof_ports > PUCCH_F2_MAX_PORTS) {
    return format("The number of receive ports, i.e. %u, exceeds the configured maximum number of receive ports, i.e., %u.",
                  c.nof_ports, std::min(grid_nof_ports, PUCCH_F2_MAX_PORTS));
  }
  for (uint32_t r = 0; r < c.nof_ports; ++r) {
    if (c.ports[r] >= grid_nof_ports) {
      return format("Rx port %u lies outside the grid (%u ports)", c.ports[r], grid_nof_ports);
    }
    for (uint32_t q = 0; q < r; ++q) {
      if (c.ports[q] == c.ports[r]) {
        return format("Rx port %u is listed twice", c.ports[r]);
      }
    }
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
  if (c.grid_index >= nof_grids) {
    return format("grid_index %u is outside the %u grids", c.grid_index, nof_grids);
  }
  if (c.llr_offset % 4u != 0) {
    return format("llr_offset %u is no multiple of 4", c.llr_offset);
  }
  if (static_cast<uint64_t>(c.llr_offset) + 16u * c.nof_prb * c.nof_symbols > 0xffffffffull) {
    return format("llr_offset %u leaves no room for the LLRs below 2^32", c.llr_offset);
  }
  return {};
}

std::string pucch_f2_llr_overlap(const srsgpu_pucch_f2_config* cfgs, uint32_t nof_pdus)
{
  std::vector<std::pair<uint64_t, uint32_t>> order;  // (offset, PDU)
  order.reserve(nof_pdus);
  for (uint32_t i = 0; i < nof_pdus; ++i) {
    order.emplace_back(cfgs[i].llr_offset, i);
  }
  std::sort(order.begin(), order.end());
  for (uint32_t k = 1; k < nof_pdus; ++k) {
    const srsgpu_pucch_f2_config& a = cfgs[order[k - 1].second];
    if (order[k - 1].first + 16u * a.nof_prb * a.nof_symbols > order[k].first) {
      return format("the LLRs of PDU %u (%u at offset %u) overlap those of PDU %u (offset %u)", order[k - 1].second,
                    16u * a.nof_prb * a.nof_symbols, a.llr_offset, order[k].second, cfgs[order[k].second].llr_offset);
    }
  }
  return {};
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
  const uint64_t nsymb  = c.cp_extended ? 12u : 14u;
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
  uint8_t bits[32 * PUCCH_F2_SCR_WORDS];
  gold_bits(static_cast<uint32_t>(c.rnti) * (1u << 15) + c.n_id, 0, 32 * PUCCH_F2_SCR_WORDS, bits);
  for (uint32_t w = 0; w < PUCCH_F2_SCR_WORDS; ++w) {
    words[w] = 0;
    for (uint32_t b = 0; b < 32; ++b) {
      words[w] |= static_cast<uint32_t>(bits[32 * w + b]) << b;
    }
  }
}

std::vector<float> pucch_f2_symbol_epochs(uint32_t numerology, bool cp_extended)
{
  const uint32_t     nsymb = cp_extended ? 12u : 14u;
  const uint32_t     khz   = 15u << numerology;
  std::vector<float> ep(nsymb);
  for (uint32_t i = 0; i < nsymb; ++i) {
    uint32_t kappa = cp_extended ? (512u >> numerology) : (144u >> numerology);
    if (!cp_extended && (i == 0 || i == (7u << numerology))) {
      kappa += 16;
    }
    const double cp = static_cast<double>(kappa * 64u) * T_C * khz * 1000;
    ep[i]           = i == 0 ? static_cast<float>(cp) : static_cast<float>(ep[i - 1] + cp + 1.0F);
  }
  return ep;
}

std::vector<float> pucch_f2_twiddles()
{
  std::vector<float> t(2 * PUCCH_F2_DFT);
  for (uint32_t k = 0; k < PUCCH_F2_DFT; ++k) {
    const double a = 2.0 * PI * static_cast<double>(k) / static_cast<double>(PUCCH_F2_DFT);
    t[2 * k]       = static_cast<float>(std::cos(a));
    t[2 * k + 1]   = static_cast<float>(std::sin(a));
  }
  return t;
}

pucch_f2_job pucch_f2_make_job(const srsgpu_pucch_f2_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports,
                               const uint32_t dmrs_rows[2], uint32_t scramble_word)
{
  pucch_f2_job j;
  std::memset(&j, 0, sizeof(j));
  j.nsc           = 12u * grid_nof_prb;
  j.port_stride   = 14u * j.nsc;
  j.grid_base     = c.grid_index * grid_nof_ports * j.port_stride;
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
  const std::vector<float> ep = pucch_f2_symbol_epochs(c.numerology, c.cp_extended != 0);
  j.delta_epoch = c.nof_symbols == 2 ? ep[c.start_symbol_index + 1] - ep[c.start_symbol_index] : 1.0F;
  j.scs_hz      = static_cast<float>((15u << c.numerology) * 1000u);
  j.fs          = static_cast<double>(static_cast<uint64_t>(PUCCH_F2_DFT) * (15u << c.numerology) * 1000u * 3u);
  return j;
}

} // namespace srsgpu
