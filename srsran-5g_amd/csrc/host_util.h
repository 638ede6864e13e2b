// What the control-channel host code (pdcch, csi_rs, ssb, pucch, pucch_f2, pucch_f34, prach and srs *_host.cpp) shares:
// message formatting, the Gold sequence, roots of unity, the refusals whose text is the same for every plan, the LLR
// overlap search, the UCI CRC and codeblock rules, the symbol start epochs and the grid geometry of a job. Header only,
// no HIP call and no HIP type, so that a host-only program can use it (tools/host_util_check.cpp checks it alone).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

namespace srsgpu {

inline std::string format(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
inline std::string format(const char* fmt, ...)
{
  char    buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return buf;
}

/// Bits c(first) .. c(first + count - 1) of the Gold sequence (TS 38.211 section 5.2.1, N_C = 1600) with initial state
/// c_init, one bit per byte.
inline void gold_bits(uint32_t c_init, uint32_t first, uint32_t count, uint8_t* out)
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

/// The same sequence from c(0) on, c(32 w + b) as bit b of word w.
inline std::vector<uint32_t> gold_words(uint32_t c_init, uint32_t nof_words)
{
  std::vector<uint8_t> bits(32 * static_cast<size_t>(nof_words));
  gold_bits(c_init, 0, 32 * nof_words, bits.data());
  std::vector<uint32_t> words(nof_words, 0u);
  for (size_t i = 0; i < bits.size(); ++i) {
    words[i >> 5] |= static_cast<uint32_t>(bits[i]) << (i & 31u);
  }
  return words;
}

/// exp(+j 2 pi k / n), k = 0..n-1, as (re, im) floats evaluated in double.
inline std::vector<float> unit_roots(uint32_t n)
{
  std::vector<float> t(2 * static_cast<size_t>(n));
  for (uint32_t k = 0; k < n; ++k) {
    const double a = 2.0 * 3.14159265358979323846 * static_cast<double>(k) / static_cast<double>(n);
    t[2 * k]       = static_cast<float>(std::cos(a));
    t[2 * k + 1]   = static_cast<float>(std::sin(a));
  }
  return t;
}

/// Symbols of a slot: 14, or 12 with the extended CP.
inline uint32_t pucch_nsymb_per_slot(uint32_t cp_extended) { return cp_extended != 0 ? 12 : 14; }

/// n_cs(n_slot, symbol) of TS 38.211 section 6.3.2.2.2 with c_init = n_id: the byte nsymb n_slot + symbol of the Gold
/// sequence, its first bit the least significant (pucch_helper.h:105: get_byte, then reverse_byte).
inline uint32_t pucch_n_cs(uint32_t n_id, uint32_t nsymb_per_slot, uint32_t n_slot, uint32_t symbol)
{
  uint8_t bits[8];
  gold_bits(n_id, 8 * (nsymb_per_slot * n_slot + symbol), 8, bits);
  uint32_t v = 0;
  for (uint32_t m = 0; m < 8; ++m) {
    v |= static_cast<uint32_t>(bits[m]) << m;
  }
  return v;
}

/// initialize_symbol_start_epochs (port_channel_estimator_average_impl.cpp:496) in float, 14 or 12 entries: each CP
/// duration in seconds (double) times the SCS, accumulated into float.
inline std::vector<float> symbol_epochs(uint32_t numerology, bool cp_extended)
{
  constexpr double   T_C   = 1.0 / (480000.0 * 4096.0);  // phy_time_unit::T_C
  const uint32_t     nsymb = pucch_nsymb_per_slot(cp_extended);
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

/// Where a job finds its grid among the plan's grids of grid_nof_ports x 14 x 12 grid_nof_prb resource elements.
struct grid_geometry {
  uint32_t nsc, port_stride;
  uint32_t grid_base;  ///< Word of (grid, port 0, symbol 0, subcarrier 0).
  grid_geometry(uint32_t grid_nof_prb, uint32_t grid_nof_ports, uint32_t grid_index) :
    nsc(12u * grid_nof_prb), port_stride(14u * nsc), grid_base(grid_index * grid_nof_ports * port_stride)
  {
  }
};

/// CRC bits of an a-bit UCI payload (TS 38.212 section 6.3.1.2.1).
inline uint32_t uci_crc_size(uint32_t a)
{
  return a < 12 ? 0 : a < 20 ? 6 : 11;
}

/// Codeblocks of an a-bit UCI payload rate-matched to e bits (TS 38.212 section 6.3.1.2.1).
inline uint32_t uci_nof_codeblocks(uint32_t a, uint32_t e)
{
  return ((a >= 360 && e >= 1088) || a >= 1013) ? 2u : 1u;
}

// The refusals that more than one plan words alike, one piece each so that every caller keeps its own order of checks.
// Each returns the reason, or an empty string.

inline std::string numerology_refusal(uint32_t numerology)
{
  return numerology > 4 ? format("numerology %u is outside 0..4", numerology) : std::string();
}

/// Numerology, cyclic prefix and slot index, in this order.
inline std::string slot_refusal(uint32_t numerology, uint32_t cp_extended, uint32_t slot_index)
{
  if (numerology > 4) {
    return numerology_refusal(numerology);
  }
  if (cp_extended > 1 || (cp_extended == 1 && numerology != 2)) {
    return format("the extended cyclic prefix exists at numerology 2 only (numerology %u)", numerology);
  }
  if (slot_index >= (10u << numerology)) {
    return format("slot index %u is outside the frame of %u slots", slot_index, 10u << numerology);
  }
  return {};
}

inline std::string symbol_allocation_refusal(uint32_t start_symbol, uint32_t nof_symbols, uint32_t cp_extended)
{
  const uint32_t nsymb = pucch_nsymb_per_slot(cp_extended);
  if (start_symbol + nof_symbols > nsymb) {
    return format("OFDM symbol allocation goes up to symbol %u, exceeding the number of symbols in the given slot with "
                  "%s CP, i.e., %u.", start_symbol + nof_symbols, cp_extended != 0 ? "extended" : "normal", nsymb);
  }
  return {};
}

/// A receive-port list: every port inside the grid, none listed twice.
inline std::string rx_port_list_refusal(const uint8_t* ports, uint32_t nof_ports, uint32_t grid_nof_ports)
{
  for (uint32_t r = 0; r < nof_ports; ++r) {
    if (ports[r] >= grid_nof_ports) {
      return format("Rx port %u lies outside the grid (%u ports)", ports[r], grid_nof_ports);
    }
    for (uint32_t q = 0; q < r; ++q) {
      if (ports[q] == ports[r]) {
        return format("Rx port %u is listed twice", ports[r]);
      }
    }
  }
  return {};
}

/// The number of receive ports (1 .. the smaller of the grid's ports and the plan's max_ports), then the list.
inline std::string rx_ports_refusal(const uint8_t* ports, uint32_t nof_ports, uint32_t grid_nof_ports, uint32_t max_ports)
{
  if (nof_ports == 0) {
    return "The number of receive ports cannot be zero.";
  }
  if (nof_ports > grid_nof_ports || nof_ports > max_ports) {
    return format("The number of receive ports, i.e. %u, exceeds the configured maximum number of receive ports, i.e., %u.",
                  nof_ports, std::min(grid_nof_ports, max_ports));
  }
  return rx_port_list_refusal(ports, nof_ports, grid_nof_ports);
}

inline std::string grid_index_refusal(uint32_t grid_index, uint32_t nof_grids)
{
  return grid_index >= nof_grids ? format("grid_index %u is outside the %u grids", grid_index, nof_grids) : std::string();
}

/// The offset of nof_llrs LLRs in the plan's LLR buffer: its alignment, then its room.
inline std::string llr_offset_refusal(uint32_t llr_offset, uint32_t nof_llrs)
{
  if (llr_offset % 4u != 0) {
    return format("llr_offset %u is no multiple of 4", llr_offset);
  }
  if (static_cast<uint64_t>(llr_offset) + nof_llrs > 0xffffffffull) {
    return format("llr_offset %u leaves no room for the LLRs below 2^32", llr_offset);
  }
  return {};
}

/// The reason two of the n PDUs' LLR ranges [offsets[i], offsets[i] + lengths[i]) overlap ("PDU i ... PDU j"), the
/// first in ascending order of offset; empty when none do.
inline std::string llr_overlap(const uint32_t* offsets, const uint32_t* lengths, uint32_t n)
{
  std::vector<std::pair<uint64_t, uint32_t>> order;  // (offset, PDU)
  order.reserve(n);
  for (uint32_t i = 0; i < n; ++i) {
    order.emplace_back(offsets[i], i);
  }
  std::sort(order.begin(), order.end());
  for (uint32_t k = 1; k < n; ++k) {
    const uint32_t a = order[k - 1].second, b = order[k].second;
    if (order[k - 1].first + lengths[a] > order[k].first) {
      return format("the LLRs of PDU %u (%u at offset %u) overlap those of PDU %u (offset %u)", a, lengths[a], offsets[a], b,
                    offsets[b]);
    }
  }
  return {};
}

} // namespace srsgpu
