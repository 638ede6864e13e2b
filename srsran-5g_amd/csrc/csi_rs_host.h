// Host-side construction for the NZP-CSI-RS plan (capi_csi_rs.cpp, csi_rs.hip): the refusals, the RE positions of
// TS 38.211 Table 7.4.1.5.3-1 rows 1-5, the RB comb of the density, and per used symbol c_init, the skipped sequence
// elements, the sequence length and the amplitude. No HIP call in this translation unit, so that a host-only program
// can check it (tools/csi_rs_host_check.cpp).
//
// Reference (behaviour, not code): lib/phy/upper/signal_processors/nzp_csi_rs_generator_impl.cpp:72
// (get_nof_skipped_elements), :123 (c_init), :129 (amplitude), :142 (get_seq_len), :175 (map);
// lib/ran/csi_rs/csi_rs_pattern.cpp (the rows' assertions and build_re_patterns).
#pragma once
#include <cstdint>
#include <string>

namespace srsgpu {

enum csi_rs_cdm : uint32_t { CSI_RS_NO_CDM = 0, CSI_RS_FD_CDM2 = 1, CSI_RS_CDM4 = 2, CSI_RS_CDM8 = 3 };
enum csi_rs_density : uint32_t { CSI_RS_DOT5_EVEN = 0, CSI_RS_DOT5_ODD = 1, CSI_RS_ONE = 2, CSI_RS_THREE = 3 };

/// nzp_csi_rs_generator::config_t without the precoding weights.
struct csi_rs_signal {
  uint32_t slot_index = 0;  ///< n_slot within the frame.
  uint32_t cp         = 0;  ///< 0 normal (14 symbols), 1 extended (12).
  uint32_t start_rb = 0, nof_rb = 0;
  uint32_t row       = 0;
  uint32_t nof_k_ref = 0;
  uint32_t k_ref[6]  = {};
  uint32_t symbol_l0 = 0, symbol_l1 = 0;
  uint32_t cdm = CSI_RS_NO_CDM, freq_density = CSI_RS_ONE;
  uint32_t scrambling_id = 0;
  uint32_t nof_ports     = 0;  ///< Ports and layers of the precoding matrix.
  float    amplitude     = 1.f;
};

/// What the kernel needs of an accepted signal. A CDM group lies on one symbol in rows 1-5.
struct csi_rs_layout {
  uint32_t nof_ports = 0, cdm_size = 0, nof_groups = 0;
  uint32_t per_rb = 0, k_step = 0;  ///< REs of a group in an RB and their spacing (row 1: 3 at 4; FD-CDM2: 2 at 1).
  uint32_t rb_begin = 0, rb_stride = 1, nof_rbs = 0;
  uint32_t seq_len = 0, seq_skip = 0;  ///< Complex sequence elements per symbol, and skipped ahead of them.
  uint32_t symbol[2] = {}, k_bar[2] = {}, c_init[2] = {};
  float    amplitude = 0.f;  ///< float(M_SQRT1_2 * double(amplitude)): each component of a sequence element.
};

/// One CDM group of one signal, as the kernel reads it (csi_rs.hip): sequence element i of the group's symbol lies on
/// subcarrier 12 (rb_begin + rb_stride (i / per_rb)) + k_bar + k_step (i % per_rb) of every port.
struct csi_rs_job {
  uint32_t c_init;
  uint32_t seq_skip, seq_len;
  uint32_t grid_base;  ///< Word of subcarrier 0 of the group's symbol on port 0 of the signal's grid.
  uint32_t port_stride;
  uint16_t rb_begin, rb_stride;
  uint16_t per_rb, k_step, k_bar;
  uint16_t nof_layers;  ///< Ports of the CDM group: 1, or 2 with the w_f cover (+1, -1) on the second.
  uint16_t nof_ports;
  uint16_t bypass;      ///< One port with the weight 1: the mapper writes the sequence itself.
  float    amplitude;
  float    w[4][2][2];  ///< [port][port of the group] (re, im).
};
static_assert(sizeof(csi_rs_job) == 104, "csi_rs_job layout");

/// The one reason the reference's assertions, this library (rows 6-12) or the grid refuse the signal; empty when it
/// is accepted.
std::string csi_rs_refusal(const csi_rs_signal& s, uint32_t grid_nof_prb, uint32_t grid_nof_ports);

/// For a signal csi_rs_refusal accepts.
csi_rs_layout csi_rs_layout_of(const csi_rs_signal& s);

} // namespace srsgpu
