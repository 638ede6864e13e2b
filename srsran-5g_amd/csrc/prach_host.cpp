// See prach_host.h.
#include "prach_host.h"
#include <algorithm>
#include <cmath>

namespace srsgpu {

namespace {

constexpr double T_C = 1.0 / (480000.0 * 4096.0);  // phy_time_unit::T_C
constexpr double PI  = 3.14159265358979323846;

std::string text(const char* what, uint64_t value)
{
  return std::string(what) + " (" + std::to_string(value) + ")";
}

} // namespace

bool prach_derive(uint32_t format, uint32_t ra_scs, uint32_t n_cs, prach_derived& d)
{
  d = prach_derived();
  // TS 38.211 Table 6.3.3.1-1 (prach_preamble_information.cpp:30): L_RA = 839, the SCS belongs to the format.
  if (format <= SRSGPU_PRACH_FORMAT_3) {
    static const uint32_t symbols[4] = {1, 2, 4, 4}, cp[4] = {3168, 21024, 4688, 3168};
    const uint32_t        scs        = format == SRSGPU_PRACH_FORMAT_3 ? SRSGPU_PRACH_SCS_5 : SRSGPU_PRACH_SCS_1_25;
    if (ra_scs != scs) {
      return false;
    }
    d.L = PRACH_LONG_L, d.N = PRACH_LONG_N, d.nof_symbols = symbols[format], d.cp_kappa = cp[format];
    d.scs_hz = format == SRSGPU_PRACH_FORMAT_3 ? 5000.0 : 1250.0;
  } else if (format <= SRSGPU_PRACH_FORMAT_A3_B3) {
    // Table 6.3.3.1-2 (prach_preamble_information.cpp:46, last_occasion = false as detect() asks): L_RA = 139,
    // N_CP^RA in kappa for 15 kHz, shifted right by the numerology.
    if (ra_scs > SRSGPU_PRACH_SCS_120) {
      return false;
    }
    uint32_t symbols = 0, cp = 0;
    switch (format) {
      case SRSGPU_PRACH_FORMAT_A1: case SRSGPU_PRACH_FORMAT_A1_B1: symbols = 2, cp = 288; break;
      case SRSGPU_PRACH_FORMAT_A2: case SRSGPU_PRACH_FORMAT_A2_B2: symbols = 4, cp = 576; break;
      case SRSGPU_PRACH_FORMAT_A3: case SRSGPU_PRACH_FORMAT_A3_B3: symbols = 6, cp = 864; break;
      case SRSGPU_PRACH_FORMAT_B1: symbols = 2, cp = 216; break;
      case SRSGPU_PRACH_FORMAT_B4: symbols = 12, cp = 936; break;
      case SRSGPU_PRACH_FORMAT_C0: symbols = 1, cp = 1240; break;
      default: symbols = 4, cp = 2048; break;  // C2
    }
    d.L = PRACH_SHORT_L, d.N = PRACH_SHORT_N, d.nof_symbols = symbols, d.cp_kappa = cp >> ra_scs;
    d.scs_hz = 15000.0 * static_cast<double>(1u << ra_scs);
  } else {
    return false;
  }
  // prach_detector_generic_impl.cpp:112-160.
  d.nof_shifts = 1, d.nof_sequences = PRACH_MAX_PREAMBLES;
  if (n_cs != 0 && n_cs <= d.L) {
    d.nof_shifts    = std::min(PRACH_MAX_PREAMBLES, d.L / n_cs);
    d.nof_sequences = (PRACH_MAX_PREAMBLES + d.nof_shifts - 1) / d.nof_shifts;
  }
  const double cp_duration = static_cast<double>(static_cast<uint64_t>(d.cp_kappa) * 64u) * T_C;
  d.cp_prach               = static_cast<uint32_t>(std::floor(cp_duration * d.L * d.scs_hz));
  d.win_width              = ((n_cs == 0 ? d.cp_prach : std::min(n_cs, d.cp_prach)) * d.N) / d.L;
  d.max_delay_samples      = n_cs == 0 ? d.cp_prach : std::min(std::max(n_cs, 1u) - 1u, d.cp_prach);
  d.max_delay_samples      = (d.max_delay_samples * d.N) / d.L;
  // :335 compares the delay with float(max_delay_samples) * 0.8, a double.
  d.delay_end = static_cast<uint32_t>(std::ceil(static_cast<double>(static_cast<float>(d.max_delay_samples)) * 0.8));
  return true;
}

std::string prach_refusal(const srsgpu_prach_occasion& o, const uint16_t* roots, uint32_t total_roots, uint64_t input_words,
                          uint32_t nof_occasions, prach_derived& d)
{
  if (o.nof_preamble_indices == 0) {
    return "no preamble to monitor";
  }
  if (static_cast<uint32_t>(o.start_preamble_index) + o.nof_preamble_indices > PRACH_MAX_PREAMBLES) {
    return text("the monitored preambles end past 64", static_cast<uint32_t>(o.start_preamble_index) + o.nof_preamble_indices);
  }
  if (o.nof_rx_ports < 1 || o.nof_rx_ports > 4) {
    return text("the number of ports is outside 1..4", o.nof_rx_ports);
  }
  if (o.combine_symbols > 1) {
    return text("combine_symbols is neither 0 nor 1", o.combine_symbols);
  }
  if (!prach_derive(o.format, o.ra_scs, o.n_cs, d)) {
    return text("the format has no preamble information at this subcarrier spacing, format", o.format);
  }
  if (o.n_cs > d.L) {
    return text("N_cs exceeds the sequence length", o.n_cs);
  }
  if (o.nof_roots != d.nof_sequences) {
    return text("nof_roots is not the number of root sequences the zone needs, which is", d.nof_sequences);
  }
  if (static_cast<uint64_t>(o.root_offset) + o.nof_roots > total_roots) {
    return text("the roots end past the root array", static_cast<uint64_t>(o.root_offset) + o.nof_roots);
  }
  for (uint32_t i = 0; i < o.nof_roots; ++i) {
    const uint32_t u = roots[o.root_offset + i];
    if (u < 1 || u >= d.L) {
      return text("a root is outside 1..L-1", u);
    }
  }
  if (!(o.threshold > 0.0F) || !std::isfinite(o.threshold)) {
    return "the threshold is not a positive number";
  }
  if (o.win_margin == 0) {
    return "the window margin is zero";
  }
  if (d.win_width == 0) {
    return "the detection window is empty";
  }
  if (2u * o.win_margin + d.win_width > d.N) {
    return text("the window with its margins is longer than the IDFT", 2u * o.win_margin + d.win_width);
  }
  for (uint32_t w = 0; w < d.nof_shifts; ++w) {
    if (prach_window_start(d.N, d.L, o.n_cs, w) + d.win_width > d.N) {
      return text("a window runs past the IDFT, window", w);
    }
  }
  const uint64_t last = static_cast<uint64_t>(o.sample_offset) + static_cast<uint64_t>(o.nof_rx_ports - 1u) * o.port_stride +
                        static_cast<uint64_t>(d.nof_symbols - 1u) * o.symbol_stride + d.L;
  if (last > input_words || last > 0xffffffffull) {
    return text("the samples end outside the input, at word", last);
  }
  if (o.result_index >= nof_occasions) {
    return text("result_index is not below the number of occasions", o.result_index);
  }
  return std::string();
}

void prach_jobs(const srsgpu_prach_occasion& o, const prach_derived& d, const std::vector<uint32_t>& root_rows,
                std::vector<prach_job>& jobs)
{
  for (uint32_t s = 0; s < d.nof_sequences; ++s) {
    prach_job j       = {};
    j.sample_offset   = o.sample_offset, j.port_stride = o.port_stride, j.symbol_stride = o.symbol_stride;
    j.root_row        = root_rows[s];
    j.result_index    = o.result_index;
    j.sequence        = s;
    j.L = d.L, j.N = d.N, j.nof_ports = o.nof_rx_ports, j.nof_symbols = d.nof_symbols, j.combine_symbols = o.combine_symbols;
    j.n_cs = o.n_cs, j.nof_shifts = d.nof_shifts, j.win_width = d.win_width, j.win_margin = o.win_margin;
    j.delay_end       = d.delay_end;
    j.first_preamble  = o.start_preamble_index;
    j.end_preamble    = static_cast<uint32_t>(o.start_preamble_index) + o.nof_preamble_indices;
    // A wavefront walks 64 / group_lanes windows at a time: as many as let the four waves cover the sequence's windows
    // in one round, with at least 8 lanes per window.
    j.group_lanes = 64;
    while (j.group_lanes > 8 && d.nof_shifts > 4 * (64 / j.group_lanes)) {
      j.group_lanes /= 2;
    }
    j.threshold       = o.threshold;
    j.mod_scale       = 1.0F / static_cast<float>(d.N * d.L * d.L);  // :263
    j.win_scale       = static_cast<float>(d.N) / static_cast<float>(d.L);  // :286
    j.rssi_scale      = static_cast<float>(o.nof_rx_ports * d.nof_symbols * d.L);  // :175
    jobs.push_back(j);
  }
}

std::vector<float> prach_root_sequence(uint32_t L, uint32_t u)
{
  // x_u(i) = exp(-j pi u i (i + 1) / L): the phase as an integer modulo 2 L, so nothing grows with i.
  auto x = [L, u](uint64_t i, double& re, double& im) {
    const uint64_t p = (static_cast<uint64_t>(u) * ((i * (i + 1u)) % (2u * L))) % (2u * L);
    const double   a = -PI * static_cast<double>(p) / static_cast<double>(L);
    re = std::cos(a), im = std::sin(a);
  };
  double y0_re = 0.0, y0_im = 0.0;
  for (uint32_t i = 0; i < L; ++i) {
    double re, im;
    x(i, re, im);
    y0_re += re, y0_im += im;
  }
  uint32_t inv = 1;  // u^-1 modulo the prime L
  while ((static_cast<uint64_t>(inv) * u) % L != 1u) {
    ++inv;
  }
  std::vector<float> y(2u * L);
  for (uint32_t n = 0; n < L; ++n) {
    double re, im;
    x((static_cast<uint64_t>(inv) * n) % L, re, im);
    // y_u(n) = conj(x_u(u^-1 n)) y_u(0).
    y[2u * n]      = static_cast<float>(re * y0_re + im * y0_im);
    y[2u * n + 1u] = static_cast<float>(re * y0_im - im * y0_re);
  }
  return y;
}

} // namespace srsgpu
