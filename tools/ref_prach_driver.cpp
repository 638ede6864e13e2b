// Driver of tools/gen_prach_golden.py: runs the reference's prach_detector_generic_impl (with its prach_generator_impl,
// its generic IDFTs of the factory's sizes 1024 / 256 and a prach_buffer_impl, all compiled from the reference tree
// where it lies, never committed) over cases the tool writes, for the fixture tests/golden/prach_detector.npz.
//
//   ref_prach_driver derive IN OUT      IN: u32 n, n x `case_header`. OUT per case: u32 N_cs, f32 threshold, u32 margin,
//                                       u32 nof_sequences, u32 L, then per root sequence the L complex floats that
//                                       prach_generator::generate returns for it, as detect() asks for them.
//   ref_prach_driver detect IN OUT [REPEATS]
//                                       IN: u32 n; per case the `case_header` and nof_ports x nof_symbols x L u32
//                                       (re | im << 16, bf16). OUT per case: `case_result`. REPEATS > 0: also times
//                                       REPEATS passes over every case on this core, "ns_per_pass <value>".
#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include "lib/phy/support/prach_buffer_impl.h"
#include "lib/phy/upper/channel_processors/prach_detector_generic_impl.h"
#include "lib/phy/upper/channel_processors/prach_detector_generic_thresholds.h"
#include "lib/phy/upper/channel_processors/prach_generator_impl.h"
#include "srsran/ran/prach/prach_cyclic_shifts.h"
#include "srsran/ran/prach/prach_preamble_information.h"
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

using namespace srsran;

namespace {

struct case_header {
  uint32_t format, ra_scs, zero_correlation_zone, root_sequence_index, nof_ports, start_preamble_index, nof_preamble_indices,
      combine_symbols;
};
struct case_result {
  float    rssi_dB;
  uint32_t nof_preambles;
  double   time_resolution, time_advance_max;
  uint32_t index[64];
  float    metric[64];
  double   time_advance[64];
};

struct geometry {
  unsigned L, nof_symbols;
};

geometry geometry_of(const case_header& h)
{
  const auto format = static_cast<prach_format_type>(h.format);
  const auto info   = is_long_preamble(format)
                          ? get_prach_preamble_long_info(format)
                          : get_prach_preamble_short_info(format, static_cast<prach_subcarrier_spacing>(h.ra_scs), false);
  return {info.sequence_length, info.nof_symbols};
}

std::unique_ptr<prach_detector> make_detector(bool combine)
{
  dft_processor::configuration long_cfg = {1024, dft_processor::direction::INVERSE};
  dft_processor::configuration short_cfg = {256, dft_processor::direction::INVERSE};
  return std::make_unique<prach_detector_generic_impl>(std::make_unique<dft_processor_generic_impl>(long_cfg),
                                                       std::make_unique<dft_processor_generic_impl>(short_cfg),
                                                       std::make_unique<prach_generator_impl>(), combine);
}

std::vector<char> read_file(const char* path)
{
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    std::fprintf(stderr, "cannot read %s\n", path);
    std::exit(2);
  }
  return std::vector<char>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

template <typename T>
T take(const std::vector<char>& raw, size_t& pos)
{
  T v;
  if (pos + sizeof(T) > raw.size()) {
    std::fprintf(stderr, "input too short\n");
    std::exit(2);
  }
  std::memcpy(&v, raw.data() + pos, sizeof(T));
  pos += sizeof(T);
  return v;
}

template <typename T>
void put(std::ofstream& f, const T& v)
{
  f.write(reinterpret_cast<const char*>(&v), sizeof(T));
}

int derive(const char* in, const char* out)
{
  const std::vector<char> raw = read_file(in);
  size_t                  pos = 0;
  const uint32_t          n   = take<uint32_t>(raw, pos);
  std::ofstream           f(out, std::ios::binary);
  prach_generator_impl    generator;
  for (uint32_t i = 0; i < n; ++i) {
    const case_header h      = take<case_header>(raw, pos);
    const auto        format = static_cast<prach_format_type>(h.format);
    const auto        scs    = static_cast<prach_subcarrier_spacing>(h.ra_scs);
    const geometry    g      = geometry_of(h);
    const unsigned    n_cs   = prach_cyclic_shifts_get(scs, restricted_set_config::UNRESTRICTED, h.zero_correlation_zone);
    detail::threshold_params th;
    th.nof_rx_ports = h.nof_ports, th.scs = scs, th.format = format, th.zero_correlation_zone = h.zero_correlation_zone;
    th.combine_symbols  = h.combine_symbols != 0;
    const auto th_m     = detail::get_threshold_and_margin(th);
    unsigned nof_shifts = 1, nof_sequences = 64;
    if (n_cs != 0) {
      nof_shifts    = std::min(64U, g.L / n_cs);
      nof_sequences = (64 + nof_shifts - 1) / nof_shifts;
    }
    put<uint32_t>(f, n_cs);
    put<float>(f, th_m.first);
    put<uint32_t>(f, th_m.second);
    put<uint32_t>(f, nof_sequences);
    put<uint32_t>(f, g.L);
    for (unsigned s = 0; s < nof_sequences; ++s) {
      prach_generator::configuration c;
      c.format = format, c.root_sequence_index = h.root_sequence_index, c.preamble_index = s * nof_shifts;
      c.restricted_set = restricted_set_config::UNRESTRICTED, c.zero_correlation_zone = h.zero_correlation_zone;
      const span<const cf_t> y = generator.generate(c);
      f.write(reinterpret_cast<const char*>(y.data()), y.size() * sizeof(cf_t));
    }
  }
  return 0;
}

struct loaded_case {
  case_header                       h;
  std::unique_ptr<prach_buffer_impl> buffer;
};

int detect(const char* in, const char* out, int repeats)
{
  const std::vector<char>  raw = read_file(in);
  size_t                   pos = 0;
  const uint32_t           n   = take<uint32_t>(raw, pos);
  std::vector<loaded_case> cases(n);
  for (loaded_case& c : cases) {
    c.h              = take<case_header>(raw, pos);
    const geometry g = geometry_of(c.h);
    c.buffer         = std::make_unique<prach_buffer_impl>(c.h.nof_ports, 1, 1, g.nof_symbols, g.L);
    for (unsigned p = 0; p < c.h.nof_ports; ++p) {
      for (unsigned s = 0; s < g.nof_symbols; ++s) {
        span<cbf16_t> symbol = c.buffer->get_symbol(p, 0, 0, s);
        static_assert(sizeof(cbf16_t) == 4, "one word per RE");
        if (pos + 4 * g.L > raw.size()) {
          std::fprintf(stderr, "input too short\n");
          return 2;
        }
        std::memcpy(static_cast<void*>(symbol.data()), raw.data() + pos, 4 * g.L);
        pos += 4 * g.L;
      }
    }
  }
  std::unique_ptr<prach_detector> detectors[2] = {make_detector(false), make_detector(true)};
  auto run = [&](const loaded_case& c) {
    prach_detector::configuration cfg;
    cfg.root_sequence_index = c.h.root_sequence_index, cfg.format = static_cast<prach_format_type>(c.h.format);
    cfg.restricted_set = restricted_set_config::UNRESTRICTED, cfg.zero_correlation_zone = c.h.zero_correlation_zone;
    cfg.start_preamble_index = c.h.start_preamble_index, cfg.nof_preamble_indices = c.h.nof_preamble_indices;
    cfg.ra_scs = static_cast<prach_subcarrier_spacing>(c.h.ra_scs), cfg.nof_rx_ports = c.h.nof_ports;
    return detectors[c.h.combine_symbols != 0 ? 1 : 0]->detect(*c.buffer, cfg);
  };
  std::ofstream f(out, std::ios::binary);
  for (const loaded_case& c : cases) {
    const prach_detection_result r = run(c);
    case_result                  o = {};
    o.rssi_dB = r.rssi_dB, o.nof_preambles = r.preambles.size();
    o.time_resolution = r.time_resolution.to_seconds(), o.time_advance_max = r.time_advance_max.to_seconds();
    for (unsigned i = 0; i < r.preambles.size(); ++i) {
      o.index[i] = r.preambles[i].preamble_index, o.metric[i] = r.preambles[i].detection_metric;
      o.time_advance[i] = r.preambles[i].time_advance.to_seconds();
    }
    put(f, o);
  }
  if (repeats > 0) {
    unsigned   sink = 0;
    const auto t0   = std::chrono::steady_clock::now();
    for (int rep = 0; rep < repeats; ++rep) {
      for (const loaded_case& c : cases) {
        sink += run(c).preambles.size();
      }
    }
    const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
    std::printf("ns_per_pass %.1f (%u)\n", ns / repeats, sink);
  }
  return 0;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc >= 4 && std::string(argv[1]) == "derive") {
    return derive(argv[2], argv[3]);
  }
  if (argc >= 4 && std::string(argv[1]) == "detect") {
    return detect(argv[2], argv[3], argc > 4 ? std::atoi(argv[4]) : 0);
  }
  std::fprintf(stderr, "usage: %s derive|detect IN OUT [REPEATS]\n", argv[0]);
  return 2;
}
