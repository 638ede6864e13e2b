// Refusals and RE layout of the NZP-CSI-RS plan; see csi_rs_host.h.
#include "csi_rs_host.h"
#include "host_util.h"
#include <cmath>

namespace srsgpu {

namespace {

/// TS 38.211 Table 7.4.1.5.3-1, rows 1-5: ports, the k_0 values that keep the row's REs inside the RB, whether
/// density 3 / 1 / 0.5 is allowed, and the CDM type.
struct row_rule {
  uint32_t ports, k_end;
  bool     three, one, half;
  uint32_t cdm;
};
constexpr row_rule ROWS[6] = {{},
                              {1, 4, true, false, false, CSI_RS_NO_CDM},
                              {1, 12, false, true, true, CSI_RS_NO_CDM},
                              {2, 11, false, true, true, CSI_RS_FD_CDM2},
                              {4, 9, false, true, false, CSI_RS_FD_CDM2},
                              {4, 11, false, true, false, CSI_RS_FD_CDM2}};
constexpr uint32_t ROW_PORTS_6_12[7] = {8, 8, 8, 12, 12, 16, 16};

bool is_half(uint32_t density)
{
  return density == CSI_RS_DOT5_EVEN || density == CSI_RS_DOT5_ODD;
}

} // namespace

std::string csi_rs_refusal(const csi_rs_signal& s, uint32_t grid_nof_prb, uint32_t grid_nof_ports)
{
  if (s.row < 1 || s.row > 18) {
    return format("Invalid mapping table row (i.e., %u)", s.row);
  }
  if (s.row > 12) {
    return format("Unsupported mapping table row (i.e., %u)", s.row);
  }
  if (s.row > 5) {
    return format("CSI-RS Mapping Row %u needs %u grid ports and the grids of this library have at most 4", s.row,
                  ROW_PORTS_6_12[s.row - 6]);
  }
  if (s.cp > 1 || s.cdm > CSI_RS_CDM8 || s.freq_density > CSI_RS_THREE) {
    return format("cp %u, cdm %u or freq_density %u is not a value of its enumeration", s.cp, s.cdm, s.freq_density);
  }
  const row_rule& r = ROWS[s.row];
  if (s.nof_k_ref != 1) {
    return format("CSI-RS Mapping Row %u: 1 k_ref is needed (i.e., %u given)", s.row, s.nof_k_ref);
  }
  if (s.k_ref[0] >= r.k_end) {
    return format("CSI-RS Mapping Row %u: k_0 (i.e., %u) outside the valid range 0..%u", s.row, s.k_ref[0], r.k_end - 1);
  }
  const bool density_ok = s.freq_density == CSI_RS_THREE ? r.three : s.freq_density == CSI_RS_ONE ? r.one : r.half;
  if (!density_ok) {
    return format("CSI-RS Mapping Row %u: invalid density", s.row);
  }
  if (s.cdm != r.cdm) {
    return format("CSI-RS Mapping Row %u: invalid CDM type", s.row);
  }
  const uint32_t nsymb = s.cp != 0 ? 12 : 14;
  if (s.symbol_l0 >= nsymb) {
    return format("CSI-RS Mapping: l_0, i.e., %u outside the valid range, i.e., [0, %u)", s.symbol_l0, nsymb);
  }
  if (s.row == 5 && s.symbol_l0 + 1 >= nsymb) {
    return format("CSI-RS Mapping Row 5: l_0 + 1, i.e., %u outside the slot of %u symbols", s.symbol_l0 + 1, nsymb);
  }
  if (s.nof_ports != r.ports) {
    return format("CSI-RS number of ports, i.e., %u, does not match the precoding number of ports, i.e., %u", r.ports,
                  s.nof_ports);
  }
  if (r.ports > grid_nof_ports) {
    return format("The precoding number of ports (i.e., %u) exceeds the grid number of ports (i.e., %u)", r.ports,
                  grid_nof_ports);
  }
  if (static_cast<uint64_t>(s.start_rb) + s.nof_rb > grid_nof_prb) {
    return format("The RBs (%u from %u) exceed the grid (%u PRBs)", s.nof_rb, s.start_rb, grid_nof_prb);
  }
  if (!std::isfinite(s.amplitude)) {
    return "The amplitude is not finite";
  }
  if (s.scrambling_id > 1023) {
    return format("scrambling_id %u exceeds 1023", s.scrambling_id);
  }
  return {};
}

csi_rs_layout csi_rs_layout_of(const csi_rs_signal& s)
{
  const row_rule& r = ROWS[s.row];
  csi_rs_layout   y;
  y.nof_ports  = r.ports;
  y.cdm_size   = r.cdm == CSI_RS_FD_CDM2 ? 2 : 1;
  y.nof_groups = r.ports / y.cdm_size;
  y.per_rb     = s.row == 1 ? 3 : y.cdm_size;
  y.k_step     = s.row == 1 ? 4 : 1;
  // The RB comb (build_re_patterns): every RB, or every second one from the first RB of the density's parity.
  const uint32_t end = s.start_rb + s.nof_rb;
  y.rb_begin         = s.start_rb;
  y.rb_stride        = 1;
  if (is_half(s.freq_density)) {
    y.rb_stride = 2;
    if (s.start_rb % 2 != (s.freq_density == CSI_RS_DOT5_ODD ? 1u : 0u)) {
      ++y.rb_begin;
    }
  }
  y.nof_rbs = y.rb_begin < end ? (end - y.rb_begin + y.rb_stride - 1) / y.rb_stride : 0;
  // get_seq_len: density 0.5 halves nof_rb and rounds an odd one up when the first RB is of the density's parity.
  uint32_t len = s.nof_rb;
  if (is_half(s.freq_density)) {
    len /= 2;
    if (s.nof_rb % 2 != 0 && s.start_rb % 2 == (s.freq_density == CSI_RS_DOT5_ODD ? 1u : 0u)) {
      ++len;
    }
  } else if (s.freq_density == CSI_RS_THREE) {
    len *= 3;
  }
  y.seq_len = s.cdm != CSI_RS_NO_CDM ? 2 * len : len;
  // get_nof_skipped_elements: the elements of the RBs below the first occupied one.
  const uint32_t first = y.rb_begin;
  if (s.freq_density == CSI_RS_THREE) {
    y.seq_skip = 3 * first;
  } else if (s.freq_density == CSI_RS_ONE) {
    y.seq_skip = s.row == 2 ? first : 2 * first;
  } else {
    y.seq_skip = s.row == 2 ? first / 2 : first;
  }
  const uint32_t nsymb = s.cp != 0 ? 12 : 14;
  for (uint32_t g = 0; g < y.nof_groups; ++g) {
    y.symbol[g] = s.symbol_l0 + (s.row == 5 ? g : 0);
    y.k_bar[g]  = s.k_ref[0] + (s.row == 4 ? 2 * g : 0);
    y.c_init[g] = static_cast<uint32_t>(
        ((1ull << 10) * (nsymb * s.slot_index + y.symbol[g] + 1) * (2 * s.scrambling_id + 1) + s.scrambling_id) & 0x7fffffffull);
  }
  y.amplitude = static_cast<float>(M_SQRT1_2 * static_cast<double>(s.amplitude));
  return y;
}

} // namespace srsgpu
