// Refusals, positions, payload layout and sequences of the SS/PBCH block plan; see ssb_host.h.
#include "ssb_host.h"
#include "host_util.h"
#include <cmath>

namespace srsgpu {

namespace {

/// TS 38.212 Table 7.1.1-1: the PBCH payload interleaver pattern G(j).
constexpr uint8_t G[32] = {16, 23, 18, 17, 8, 30, 10, 6, 24, 7, 0, 5, 3, 2, 1, 4,
                           9, 11, 12, 13, 14, 15, 19, 20, 21, 22, 25, 26, 27, 28, 29, 31};
// Where TS 38.212 section 7.1.1 puts the bits that are not the payload's: the 4th..1st LSB of the SFN on G(6..9), the
// half frame bit on G(10), the block index bits 6..4 (L_max = 64) or the MSB of k_SSB and two reserved bits on G(11..13).
constexpr uint32_t J_SFN_LSBS = 6, J_HRF = 10, J_IDX = 11;

/// TS 38.213 section 4.1: the first symbols of the candidate blocks in their period, per case A..E, and the n of the
/// FR2 cases.
constexpr uint8_t  FIRST_SYMBOLS[5][8] = {{2, 8}, {4, 8, 16, 20}, {2, 8}, {4, 8, 16, 20}, {8, 12, 16, 20, 32, 36, 40, 44}};
constexpr uint8_t  NOF_FIRST[5]        = {2, 4, 2, 4, 8};
constexpr uint8_t  PERIOD[5]           = {14, 28, 14, 28, 56};
constexpr uint8_t  N_FR2[16]           = {0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 12, 13, 15, 16, 17, 18};
constexpr uint32_t SSB_SCS_KHZ[5]      = {15, 30, 30, 120, 240};

constexpr uint32_t CRC24C_POLY = 0x1b2b117;

bool is_fr2(uint32_t pattern_case)
{
  return pattern_case >= 3;
}

/// x(i + 7) = x(i + tap) + x(i) from x(0..6), 127 bits.
void m_sequence(const uint8_t (&init)[7], uint32_t tap, uint8_t* x)
{
  uint8_t s[127 + 7];
  for (uint32_t i = 0; i < 7; ++i) {
    s[i] = init[i];
  }
  for (uint32_t i = 0; i < 127; ++i) {
    s[i + 7] = (s[i + tap] + s[i]) & 1;
  }
  for (uint32_t i = 0; i < 127; ++i) {
    x[i] = s[i];
  }
}

/// Mask of d(n) = -1, n = 0..126, for d(n) = 1 - 2 x((n + m) mod 127).
void shifted_mask(const uint8_t* x, uint32_t m, uint32_t* mask)
{
  for (uint32_t w = 0; w < 4; ++w) {
    mask[w] = 0;
  }
  for (uint32_t n = 0; n < 127; ++n) {
    if (x[(n + m) % 127] != 0) {
      mask[n >> 5] |= 1u << (n & 31);
    }
  }
}

} // namespace

uint32_t ssb_l_first(uint32_t pattern_case, uint32_t ssb_idx)
{
  const uint32_t count = NOF_FIRST[pattern_case];
  uint32_t       n     = ssb_idx / count;
  if (is_fr2(pattern_case)) {
    n = N_FR2[n & 15];
  }
  return FIRST_SYMBOLS[pattern_case][ssb_idx % count] + PERIOD[pattern_case] * n;
}

bool ssb_k_first(const ssb_block& b, uint32_t& k_first)
{
  // offsetToPointA counts RBs of 15 kHz (FR1) or 60 kHz (FR2), k_SSB subcarriers of 15 kHz (FR1) or of the common SCS.
  const uint32_t khz = is_fr2(b.pattern_case)
                           ? 60 * 12 * b.offset_to_pointA + (15u << b.common_scs) * b.subcarrier_offset
                           : 15 * (12 * b.offset_to_pointA + b.subcarrier_offset);
  const uint32_t scs = SSB_SCS_KHZ[b.pattern_case];
  k_first            = khz / scs;
  return khz % scs == 0;
}

std::string ssb_refusal(const ssb_block& b, uint32_t grid_nof_prb, uint32_t grid_nof_ports)
{
  if (b.pattern_case > 4) {
    return format("Invalid SSB pattern case (i.e., %u)", b.pattern_case);
  }
  if (b.L_max != 4 && b.L_max != 8 && b.L_max != 64) {
    return format("L_max (i.e., %u) is not 4, 8 or 64", b.L_max);
  }
  if (b.ssb_idx >= b.L_max) {
    return format("ssb_idx (i.e., %u) is not below L_max (i.e., %u)", b.ssb_idx, b.L_max);
  }
  if (b.phys_cell_id > 1007) {
    return format("phys_cell_id (i.e., %u) exceeds 1007", b.phys_cell_id);
  }
  const bool fr2 = is_fr2(b.pattern_case);
  if (b.common_scs > 4 || (fr2 ? b.common_scs < 2 : b.common_scs > 2)) {
    return format("Unsupported combination of FR%u and Common SCS numerology %u", fr2 ? 2u : 1u, b.common_scs);
  }
  if (b.offset_to_pointA > 2199) {
    return format("Invalid offset to Point A %u (max 2199)", b.offset_to_pointA);
  }
  if (b.subcarrier_offset > (fr2 ? 11u : 23u)) {
    return format("Invalid subcarrier offset %u for FR%u (max %u)", b.subcarrier_offset, fr2 ? 2u : 1u, fr2 ? 11u : 23u);
  }
  uint32_t k_first = 0;
  if (!ssb_k_first(b, k_first)) {
    return format("Unsupported combination of SSB SCS %ukHz, Common SCS numerology %u, offsetToPointA %u and "
                  "ssb-SubcarrierOffset %u", SSB_SCS_KHZ[b.pattern_case], b.common_scs, b.offset_to_pointA,
                  b.subcarrier_offset);
  }
  const uint32_t l_first = ssb_l_first(b.pattern_case, b.ssb_idx);
  if (l_first / 14 != b.slot_index) {
    return format("Invalid slot index (%u) for SSB index %u, which lies in slot %u of the half frame", b.slot_index,
                  b.ssb_idx, l_first / 14);
  }
  if (b.hrf > 1) {
    return format("hrf (i.e., %u) is not 0 or 1", b.hrf);
  }
  if (l_first % 14 + 4 > 14) {
    return format("The block's symbols (4 from %u) exceed the slot of the grid", l_first % 14);
  }
  if (static_cast<uint64_t>(k_first) + 240 > 12ull * grid_nof_prb) {
    return format("The block's subcarriers (240 from %u) exceed the grid (%u PRBs)", k_first, grid_nof_prb);
  }
  if (b.nof_ports < 1 || b.nof_ports > 4) {
    return format("The number of ports (i.e., %u) is outside 1..4", b.nof_ports);
  }
  for (uint32_t p = 0; p < b.nof_ports; ++p) {
    if (b.ports[p] >= grid_nof_ports) {
      return format("Port %u is outside the grid's %u ports", static_cast<unsigned>(b.ports[p]), grid_nof_ports);
    }
    for (uint32_t q = 0; q < p; ++q) {
      if (b.ports[q] == b.ports[p]) {
        return format("Port %u is listed twice", static_cast<unsigned>(b.ports[p]));
      }
    }
  }
  if (!std::isfinite(b.pss_amplitude)) {
    return "pss_amplitude is not finite";
  }
  return {};
}

void ssb_fill_tables(ssb_tables& t)
{
  // The payload's bits 1..6 (the SFN's MSBs) go to G(0..5), the others to G(14..31); then the SFN's four LSBs.
  for (uint32_t i = 0; i < 32; ++i) {
    t.dyn_source[i] = SSB_DYNAMIC_NONE;
  }
  uint32_t j_sfn = 0, j_other = 14;
  for (uint32_t i = 0; i < 24; ++i) {
    t.dyn_source[G[i >= 1 && i < 7 ? j_sfn++ : j_other++]] = static_cast<uint8_t>(i);
  }
  for (uint32_t i = 0; i < 4; ++i) {
    t.dyn_source[G[J_SFN_LSBS + i]] = static_cast<uint8_t>(24 + i);
  }
  t.v_hi = G[J_SFN_LSBS + 1];
  t.v_lo = G[J_SFN_LSBS + 2];
  uint32_t power = CRC24C_POLY & 0xffffffu;
  for (uint32_t j = 0; j < 32; ++j) {
    t.crc_weights[j] = power;
    power <<= 1;
    if ((power >> 24) != 0) {
      power ^= CRC24C_POLY;
    }
  }
}

void ssb_fill_desc(const ssb_block& b, ssb_desc& d)
{
  const bool l64 = b.L_max == 64;
  // The fixed bits of a, and the positions the first scrambling leaves alone.
  d.a_const      = (b.hrf & 1u) << G[J_HRF];
  uint32_t plain = (1u << G[J_HRF]) | (1u << G[J_SFN_LSBS + 1]) | (1u << G[J_SFN_LSBS + 2]);
  if (l64) {
    d.a_const |= ((b.ssb_idx >> 5) & 1u) << G[J_IDX] | ((b.ssb_idx >> 4) & 1u) << G[J_IDX + 1] |
                 ((b.ssb_idx >> 3) & 1u) << G[J_IDX + 2];
    plain |= (1u << G[J_IDX]) | (1u << G[J_IDX + 1]) | (1u << G[J_IDX + 2]);
  } else {
    d.a_const |= ((b.subcarrier_offset >> 4) & 1u) << G[J_IDX];
  }
  // The scrambling sequence of N_id from M v on, M the number of scrambled positions, spread over those positions.
  const uint32_t M = l64 ? 26 : 29;
  uint8_t        c[4 * 29];
  gold_bits(b.phys_cell_id, 0, 4 * M, c);
  for (uint32_t v = 0; v < 4; ++v) {
    uint32_t mask = 0, j = 0;
    for (uint32_t i = 0; i < 32; ++i) {
      if (((plain >> i) & 1u) == 0) {
        mask |= static_cast<uint32_t>(c[M * v + j++]) << i;
      }
    }
    d.scramble[v] = mask;
  }
  d.c_init_data = b.phys_cell_id;
  d.data_word0  = (b.ssb_idx & 7u) * (SSB_PBCH_BITS / 32);
  // i_SSB: the block index's three LSBs, or for L_max = 4 its two LSBs and the half frame bit above them.
  const uint32_t i_ssb = b.L_max == 4 ? (b.ssb_idx & 3u) + 4u * b.hrf : (b.ssb_idx & 7u);
  d.c_init_dmrs        = (((i_ssb + 1) * (b.phys_cell_id / 4 + 1)) << 11) + ((i_ssb + 1) << 6) + b.phys_cell_id % 4;
  // PSS: x(i + 7) = x(i + 4) + x(i) from 0110111, shifted by 43 N_id2. SSS: x0 the same recursion and x1(i + 7) =
  // x1(i + 1) + x1(i), both from 1000000, shifted by m0 = 15 floor(N_id1 / 112) + 5 N_id2 and m1 = N_id1 mod 112.
  const uint32_t nid1 = b.phys_cell_id / 3, nid2 = b.phys_cell_id % 3;
  uint8_t        x[127], x0[127], x1[127];
  m_sequence({0, 1, 1, 0, 1, 1, 1}, 4, x);
  m_sequence({1, 0, 0, 0, 0, 0, 0}, 4, x0);
  m_sequence({1, 0, 0, 0, 0, 0, 0}, 1, x1);
  shifted_mask(x, (43 * nid2) % 127, d.pss);
  shifted_mask(x0, 15 * (nid1 / 112) + 5 * nid2, d.sss0);
  shifted_mask(x1, nid1 % 112, d.sss1);
  d.pss_amplitude = b.pss_amplitude;
  d.v             = static_cast<uint16_t>(b.phys_cell_id % 4);
  d.nof_ports     = static_cast<uint16_t>(b.nof_ports);
  for (uint32_t p = 0; p < 4; ++p) {
    d.ports[p] = p < b.nof_ports ? b.ports[p] : 0;
  }
}

} // namespace srsgpu
