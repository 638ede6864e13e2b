// Refusals, cyclic shift hopping, tables and job descriptors of the PUCCH detector plan; see pucch_host.h.
#include "pucch_host.h"
#include "host_util.h"
#include "low_papr_tables.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace srsgpu {

namespace {

/// Slot, CP, symbols, PRBs, n_id and grid shared by both formats' refusals.
std::string common_refusal(uint32_t slot_index, uint32_t numerology, uint32_t cp_extended, uint32_t starting_prb,
                           uint32_t second_hop_prb, uint32_t start_symbol, uint32_t nof_symbols, uint32_t n_id,
                           uint32_t grid_index, uint32_t grid_nof_prb, uint32_t nof_grids)
{
  if (numerology > 4 || cp_extended > 1 || (cp_extended == 1 && numerology != 2)) {
    return format("numerology %u with %s CP is not a numerology 0..4 (the extended CP exists at numerology 2 only)",
                  numerology, cp_extended != 0 ? "extended" : "normal");
  }
  if (slot_index >= (10u << numerology)) {
    return format("slot_index %u is outside the %u slots of a frame", slot_index, 10u << numerology);
  }
  if (std::string why = symbol_allocation_refusal(start_symbol, nof_symbols, cp_extended); !why.empty()) {
    return why;
  }
  if (n_id > 1023) {
    return format("The sequence hopping identifier (i.e., %u) is out of the range [0..1024).", n_id);
  }
  if (starting_prb >= grid_nof_prb) {
    return format("PRB %u lies outside the grid (%u PRBs)", starting_prb, grid_nof_prb);
  }
  if (second_hop_prb != PUCCH_NO_HOP && second_hop_prb >= grid_nof_prb) {
    return format("Second hop PRB %u lies outside the grid (%u PRBs)", second_hop_prb, grid_nof_prb);
  }
  return grid_index_refusal(grid_index, nof_grids);
}

void fill_common(pucch_job& j, uint32_t slot_index, uint32_t cp_extended, uint32_t starting_prb, uint32_t second_hop_prb,
                 uint32_t second_hop_first, uint32_t start_symbol, uint32_t nof_symbols, uint32_t n_id, uint32_t m0,
                 uint32_t grid_index, uint32_t grid_nof_prb, uint32_t grid_nof_ports)
{
  const grid_geometry g(grid_nof_prb, grid_nof_ports, grid_index);
  const uint32_t      nsymb = pucch_nsymb_per_slot(cp_extended);
  j.port_stride  = g.port_stride;
  j.nof_symbols  = static_cast<uint8_t>(nof_symbols);
  for (uint32_t i = 0; i < nof_symbols; ++i) {
    const uint32_t prb = (second_hop_prb != PUCCH_NO_HOP && i >= second_hop_first) ? second_hop_prb : starting_prb;
    j.sym_base[i]      = g.grid_base + (start_symbol + i) * g.nsc + 12 * prb;
    j.alpha[i]         = static_cast<uint8_t>((m0 + pucch_n_cs(n_id, nsymb, slot_index, start_symbol + i)) % 12);
  }
  // compute_group_sequence with neither group nor sequence hopping: u = n_id mod 30, v = 0.
  const int8_t* phi = kLowPaprPhi12[n_id % 30];
  for (uint32_t n = 0; n < 12; ++n) {
    j.phi3[n] = static_cast<uint8_t>((3 * phi[n] + 24) % 24);
  }
}

} // namespace

float pucch_f0_threshold(uint32_t nof_ports, uint32_t nof_symbols, uint32_t nof_sequences)
{
  struct entry {
    uint32_t degrees, sequences;
    double   threshold;
  };
  static const entry table[16] = {{1, 1, 0.5373}, {1, 2, 0.6460}, {1, 4, 0.7556}, {1, 8, 1.6818},
                                  {2, 1, 0.5273}, {2, 2, 0.4038}, {2, 4, 0.7273}, {2, 8, 0.8364},
                                  {4, 1, 0.3455}, {4, 2, 0.2800}, {4, 4, 0.4455}, {4, 8, 0.5000},
                                  {8, 1, 0.2545}, {8, 2, 0.2083}, {8, 4, 0.3000}, {8, 8, 0.3273}};
  const uint32_t degrees = nof_ports * nof_symbols;
  for (const entry& e : table) {
    // The first entry not below (degrees, sequences) in lexicographic order.
    if (e.degrees > degrees || (e.degrees == degrees && e.sequences >= nof_sequences)) {
      return static_cast<float>(e.threshold);
    }
  }
  return 0.0F;
}

float pucch_f1_threshold(uint32_t nof_contributions)
{
  switch (nof_contributions) {
    case 1:
      return 0.9F;
    case 2:
      return 3.0F;
    case 4:
      return 4.45F;
    case 8:
      return 6.95F;
    default:
      return 0.0F;
  }
}

uint32_t pucch_f0_candidates(uint32_t nof_harq_ack, uint32_t sr_opportunity, uint8_t m_cs[8], uint8_t message[8])
{
  // message: bit 0 SR, bit 1 HARQ-ACK 0, bit 2 HARQ-ACK 1. TS 38.213 Tables 9.2.3-3 / -4 (negative or no SR) and
  // 9.2.5-1 / -2 (positive SR), in the order of the reference's tables.
  struct cand {
    uint8_t m_cs, sr, a0, a1;
  };
  static const cand noharq_sr[1]     = {{0, 1, 0, 0}};
  static const cand oneharq_nosr[2]  = {{0, 0, 0, 0}, {6, 0, 1, 0}};
  static const cand twoharq_nosr[4]  = {{0, 0, 0, 0}, {3, 0, 0, 1}, {6, 0, 1, 1}, {9, 0, 1, 0}};
  static const cand oneharq_onesr[4] = {{0, 0, 0, 0}, {6, 0, 1, 0}, {3, 1, 0, 0}, {9, 1, 1, 0}};
  static const cand twoharq_onesr[8] = {{0, 0, 0, 0}, {3, 0, 0, 1}, {6, 0, 1, 1}, {9, 0, 1, 0},
                                        {1, 1, 0, 0}, {4, 1, 0, 1}, {7, 1, 1, 1}, {10, 1, 1, 0}};
  const cand* table = nullptr;
  uint32_t    count = 0;
  if (nof_harq_ack == 0) {
    // The reference takes the SR-only table for no HARQ-ACK whatever sr_opportunity says; its validator refuses the
    // PDU without payload.
    table = noharq_sr, count = 1;
  } else if (nof_harq_ack == 1) {
    table = sr_opportunity != 0 ? oneharq_onesr : oneharq_nosr, count = sr_opportunity != 0 ? 4 : 2;
  } else if (nof_harq_ack == 2) {
    table = sr_opportunity != 0 ? twoharq_onesr : twoharq_nosr, count = sr_opportunity != 0 ? 8 : 4;
  }
  for (uint32_t i = 0; i < count; ++i) {
    m_cs[i]    = table[i].m_cs;
    message[i] = static_cast<uint8_t>(table[i].sr | (table[i].a0 << 1) | (table[i].a1 << 2));
  }
  return count;
}

pucch_f1_split pucch_f1_hop_split(uint32_t nof_symbols, bool hopping)
{
  pucch_f1_split s{};
  // Every other allocated symbol from the first carries DM-RS (pucch_detector_format1.cpp:165), across the hop border:
  // a second hop that starts on an odd allocated symbol starts with a data symbol.
  for (uint32_t i = 0; i < nof_symbols; i += 2) {
    s.dmrs_mask |= 1u << i;
  }
  s.nof_hops       = hopping ? 2 : 1;
  s.first[0]       = 0;
  s.nof_symbols[0] = hopping ? nof_symbols / 2 : nof_symbols;
  s.first[1]       = s.nof_symbols[0];
  s.nof_symbols[1] = nof_symbols - s.nof_symbols[0];
  for (uint32_t h = 0; h < s.nof_hops; ++h) {
    for (uint32_t i = s.first[h]; i < s.first[h] + s.nof_symbols[h]; ++i) {
      ++(((s.dmrs_mask >> i) & 1u) != 0 ? s.nof_dmrs[h] : s.nof_data[h]);
    }
  }
  return s;
}

std::string pucch_f0_refusal(const srsgpu_pucch_f0_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports, uint32_t nof_grids)
{
  if (c.nof_symbols < 1 || c.nof_symbols > 2) {
    return format("Number of symbols (i.e., %u) is out of the range [1..2].", c.nof_symbols);
  }
  const std::string why = common_refusal(c.slot_index, c.numerology, c.cp_extended, c.starting_prb, c.second_hop_prb,
                                         c.start_symbol_index, c.nof_symbols, c.n_id, c.grid_index, grid_nof_prb, nof_grids);
  if (!why.empty()) {
    return why;
  }
  if (c.initial_cyclic_shift > 11) {
    return format("The initial cyclic shift (i.e., %u) is out of the range [0..11].", c.initial_cyclic_shift);
  }
  if (c.nof_harq_ack == 0 && c.sr_opportunity == 0) {
    return "No payload.";
  }
  if (c.nof_harq_ack > 2) {
    return format("The number of HARQ-ACK bits (i.e., %u) is out of the range [0..2].", c.nof_harq_ack);
  }
  if (c.sr_opportunity > 1) {
    return format("sr_opportunity %u is neither 0 nor 1", c.sr_opportunity);
  }
  if (c.nof_ports == 0) {
    return "The number of receive ports cannot be zero.";
  }
  if (c.nof_ports > 4) {
    return format("The number of receive ports (i.e., %u) exceeds 4", c.nof_ports);
  }
  for (uint32_t p = 0; p < c.nof_ports; ++p) {
    if (c.ports[p] >= grid_nof_ports) {
      return format("Port %u lies outside the grid (%u ports)", c.ports[p], grid_nof_ports);
    }
  }
  return {};
}

std::string pucch_f1_refusal(const srsgpu_pucch_f1_resource& r,
                             const srsgpu_pucch_f1_entry*    entries,
                             uint32_t                        total_entries,
                             uint32_t                        grid_nof_prb,
                             uint32_t                        grid_nof_ports,
                             uint32_t                        nof_grids)
{
  if (r.start_symbol_index > 10) {
    return format("Setting %u as the first PUCCH symbol index, but only values between 0 and 10 are valid.",
                  r.start_symbol_index);
  }
  if (r.nof_symbols < 4 || r.nof_symbols > 14) {
    return format("Requiring %u OFDM symbols for PUCCH, but only values between 4 and 14 are valid.", r.nof_symbols);
  }
  const std::string why = common_refusal(r.slot_index, r.numerology, r.cp_extended, r.starting_prb, r.second_hop_prb,
                                         r.start_symbol_index, r.nof_symbols, r.n_id, r.grid_index, grid_nof_prb, nof_grids);
  if (!why.empty()) {
    return why;
  }
  const bool hopping = r.second_hop_prb != PUCCH_NO_HOP;
  if (r.nof_rx_ports == 0) {
    return "The number of receive ports cannot be zero.";
  }
  if (r.nof_rx_ports > grid_nof_ports) {
    return format("The number of receive ports, i.e. %u, exceeds the grid's ports, i.e., %u.", r.nof_rx_ports, grid_nof_ports);
  }
  if (pucch_f1_threshold(r.nof_rx_ports * (hopping ? 2u : 1u)) == 0.0F) {
    return format("%u ports x %u hops is not 1, 2, 4 or 8 contributions: the detector has no threshold for it",
                  r.nof_rx_ports, hopping ? 2u : 1u);
  }
  if (r.nof_entries == 0) {
    return "A Format 1 resource without entries: the noise estimate is undefined";
  }
  if (r.nof_entries > PUCCH_F1_MAX_ENTRIES || static_cast<uint64_t>(r.first_entry) + r.nof_entries > total_entries) {
    return format("Entries %u..%u lie outside the %u entries, or are more than 84", r.first_entry,
                  r.first_entry + r.nof_entries, total_entries);
  }
  const pucch_f1_split split    = pucch_f1_hop_split(r.nof_symbols, hopping);
  const uint32_t       occ_stop = hopping ? std::min(split.nof_data[0], split.nof_data[1]) : split.nof_data[0];
  bool                 seen[7][12] = {};
  for (uint32_t i = 0; i < r.nof_entries; ++i) {
    const srsgpu_pucch_f1_entry& e = entries[r.first_entry + i];
    if (e.initial_cyclic_shift > 11) {
      return format("Setting %u as the initial cyclic shift, but only values between 0 and 11 are valid.",
                    e.initial_cyclic_shift);
    }
    if (e.time_domain_occ >= occ_stop) {
      return format("Cannot have OCCI %u with %u allocated OFDM symbols and frequency hopping %s.", e.time_domain_occ,
                    r.nof_symbols, hopping ? "enabled" : "disabled");
    }
    if (e.nof_harq_ack > 2) {
      return format("At most two ACK bits - requested %u.", e.nof_harq_ack);
    }
    if (seen[e.time_domain_occ][e.initial_cyclic_shift]) {
      return format("Two entries with initial cyclic shift %u and OCCI %u", e.initial_cyclic_shift, e.time_domain_occ);
    }
    seen[e.time_domain_occ][e.initial_cyclic_shift] = true;
  }
  return {};
}

pucch_job pucch_f0_job(const srsgpu_pucch_f0_config& c, uint32_t grid_nof_prb, uint32_t grid_nof_ports, uint32_t result_offset)
{
  pucch_job j;
  std::memset(&j, 0, sizeof(j));
  j.kind          = 0;
  j.result_offset = result_offset;
  // The first symbol lies on starting_prb, any further one on the second hop's PRB (pucch_detector_format0.cpp:150).
  fill_common(j, c.slot_index, c.cp_extended, c.starting_prb, c.second_hop_prb, 1, c.start_symbol_index, c.nof_symbols,
              c.n_id, c.initial_cyclic_shift, c.grid_index, grid_nof_prb, grid_nof_ports);
  j.nof_ports = c.nof_ports;
  std::memcpy(j.ports, c.ports, 4);
  j.nof_hops       = 1;
  j.nof_candidates = static_cast<uint8_t>(pucch_f0_candidates(c.nof_harq_ack, c.sr_opportunity, j.m_cs, j.message));
  j.threshold      = pucch_f0_threshold(c.nof_ports, c.nof_symbols, j.nof_candidates);
  return j;
}

pucch_job pucch_f1_job(const srsgpu_pucch_f1_resource& r,
                       const srsgpu_pucch_f1_entry*    entries,
                       uint32_t                        grid_nof_prb,
                       uint32_t                        grid_nof_ports,
                       uint32_t                        result_offset)
{
  pucch_job j;
  std::memset(&j, 0, sizeof(j));
  const bool           hopping = r.second_hop_prb != PUCCH_NO_HOP;
  const pucch_f1_split split   = pucch_f1_hop_split(r.nof_symbols, hopping);
  j.kind          = 1;
  j.result_offset = result_offset;
  fill_common(j, r.slot_index, r.cp_extended, r.starting_prb, r.second_hop_prb, split.first[1], r.start_symbol_index,
              r.nof_symbols, r.n_id, 0, r.grid_index, grid_nof_prb, grid_nof_ports);
  j.nof_ports = r.nof_rx_ports;
  for (uint8_t p = 0; p < 4; ++p) {
    j.ports[p] = p;
  }
  j.nof_hops    = static_cast<uint8_t>(split.nof_hops);
  j.first_entry = r.first_entry;
  j.nof_entries = r.nof_entries;
  j.threshold   = pucch_f1_threshold(r.nof_rx_ports * split.nof_hops);
  j.dmrs_mask   = static_cast<uint16_t>(split.dmrs_mask);
  for (uint32_t h = 0; h < 2; ++h) {
    j.hop_first[h]       = static_cast<uint8_t>(split.first[h]);
    j.hop_nof_symbols[h] = static_cast<uint8_t>(split.nof_symbols[h]);
    j.hop_nof_data[h]    = static_cast<uint8_t>(split.nof_data[h]);
    j.hop_nof_dmrs[h]    = static_cast<uint8_t>(split.nof_dmrs[h]);
  }
  for (uint32_t i = 0; i < r.nof_entries; ++i) {
    j.occ_mask |= static_cast<uint8_t>(1u << entries[r.first_entry + i].time_domain_occ);
  }
  return j;
}

std::vector<float> pucch_w_table()
{
  static const uint8_t phi4[4][4] = {{0, 0, 0, 0}, {0, 2, 0, 2}, {0, 0, 2, 2}, {0, 2, 2, 0}};
  std::vector<float>   w(PUCCH_W_TABLE_FLOATS, 0.0F);
  for (uint32_t N = 1; N <= 7; ++N) {
    for (uint32_t i = 0; i < N; ++i) {
      for (uint32_t m = 0; m < N; ++m) {
        // For every length but 4 the table's phi(m) is i m mod N.
        const uint32_t phi   = N == 4 ? phi4[i][m] : (i * m) % N;
        const double   angle = 2.0 * M_PI * phi / N;
        const size_t   at    = 2 * ((N - 1) * 49 + i * 7 + m);
        w[at]                = static_cast<float>(std::cos(angle));
        w[at + 1]            = static_cast<float>(std::sin(angle));
      }
    }
  }
  return w;
}

} // namespace srsgpu
