// Driver of tools/gen_srs_golden.py: runs the reference's srs_estimator_generic_impl (with its
// low_papr_sequence_generator_impl, its time_alignment_estimator_dft_impl over generic IDFTs of every size 128..4096 and
// a resource_grid_impl, all compiled from the reference tree where it lies, never committed) over cases the tool
// writes, for the fixture tests/golden/srs_estimator.npz.
//
//   ref_srs_driver table OUT            OUT: 64 x 4 x (u32 m_srs, u32 N): srs_configuration_get(c_srs, b_srs), as data.
//   ref_srs_driver estimate IN OUT [REPEATS]
//                                       IN: u32 n; per case the `case_header`, then nof_rx_ports x nof_symbols x
//                                       comb sets x L u32 (re | im << 16, bf16): the REs the estimator reads, the comb
//                                       sets in ascending order of their first subcarrier. OUT per case: `case_result`.
//                                       REPEATS > 0: also times REPEATS passes over every case on this core,
//                                       "ns_per_pass <value>".
// The time alignment estimator is wrapped so that each antenna port's own measurement is recorded next to the mean the
// estimator returns.
#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include "lib/phy/support/resource_grid_impl.h"
#include "lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.h"
#include "lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.h"
#include "lib/phy/upper/signal_processors/srs/srs_estimator_generic_impl.h"
#include "srsran/phy/upper/signal_processors/srs/srs_estimator_configuration.h"
#include "srsran/phy/upper/signal_processors/srs/srs_estimator_result.h"
#include "srsran/ran/srs/srs_bandwidth_configuration.h"
#include "srsran/ran/srs/srs_information.h"
#include <algorithm>
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
  uint32_t c_srs, numerology, nof_antenna_ports, nof_symbols, start_symbol, comb_size, comb_offset, cyclic_shift,
      sequence_id, bandwidth_index, freq_position, freq_shift, nof_rx_ports, rx_ports[4], grid_nof_ports, grid_nof_prb;
};
struct case_result {
  float  channel[4][4][2];
  float  epre_dB, noise_var;
  double time_alignment, resolution, ta_min, ta_max;
  double ta_port[4];
};

/// Forwards to the reference's estimator and keeps the measurements of the last estimate() call of the SRS estimator.
class recording_ta_estimator : public time_alignment_estimator
{
public:
  explicit recording_ta_estimator(std::unique_ptr<time_alignment_estimator> base_) : base(std::move(base_)) {}
  time_alignment_measurement
  estimate(span<const cf_t> symbols, bounded_bitset<max_nof_symbols> mask, subcarrier_spacing scs, double max_ta) override
  {
    return base->estimate(symbols, mask, scs, max_ta);
  }
  time_alignment_measurement estimate(const re_buffer_reader<cf_t>&   symbols,
                                      bounded_bitset<max_nof_symbols> mask,
                                      subcarrier_spacing              scs,
                                      double                          max_ta) override
  {
    return base->estimate(symbols, mask, scs, max_ta);
  }
  time_alignment_measurement
  estimate(span<const cf_t> symbols, unsigned stride, subcarrier_spacing scs, double max_ta) override
  {
    return base->estimate(symbols, stride, scs, max_ta);
  }
  time_alignment_measurement
  estimate(const re_buffer_reader<cf_t>& symbols, unsigned stride, subcarrier_spacing scs, double max_ta) override
  {
    const time_alignment_measurement m = base->estimate(symbols, stride, scs, max_ta);
    seen.push_back(m.time_alignment);
    return m;
  }
  std::vector<double> seen;

private:
  std::unique_ptr<time_alignment_estimator> base;
};

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

srs_estimator_configuration config_of(const case_header& h)
{
  srs_estimator_configuration cfg;
  cfg.slot                         = slot_point(h.numerology, 0);
  cfg.resource.nof_antenna_ports   = static_cast<srs_resource_configuration::one_two_four_enum>(h.nof_antenna_ports);
  cfg.resource.nof_symbols         = static_cast<srs_resource_configuration::one_two_four_enum>(h.nof_symbols);
  cfg.resource.start_symbol        = h.start_symbol;
  cfg.resource.configuration_index = h.c_srs;
  cfg.resource.sequence_id         = h.sequence_id;
  cfg.resource.bandwidth_index     = h.bandwidth_index;
  cfg.resource.comb_size           = static_cast<srs_resource_configuration::comb_size_enum>(h.comb_size);
  cfg.resource.comb_offset         = h.comb_offset;
  cfg.resource.cyclic_shift        = h.cyclic_shift;
  cfg.resource.freq_position       = h.freq_position;
  cfg.resource.freq_shift          = h.freq_shift;
  cfg.resource.freq_hopping        = 3;
  cfg.resource.hopping             = srs_resource_configuration::group_or_sequence_hopping_enum::neither;
  for (unsigned r = 0; r < h.nof_rx_ports; ++r) {
    cfg.ports.push_back(static_cast<uint8_t>(h.rx_ports[r]));
  }
  return cfg;
}

struct loaded_case {
  case_header                         h;
  srs_estimator_configuration         cfg;
  std::unique_ptr<resource_grid_impl> grid;
};

int table(const char* out)
{
  std::ofstream f(out, std::ios::binary);
  for (unsigned c_srs = 0; c_srs < 64; ++c_srs) {
    for (unsigned b = 0; b < 4; ++b) {
      const auto     cfg  = srs_configuration_get(c_srs, b);
      const uint32_t v[2] = {cfg ? cfg->m_srs : 0u, cfg ? cfg->N : 0u};
      f.write(reinterpret_cast<const char*>(v), sizeof(v));
    }
  }
  return 0;
}

int estimate(const char* in, const char* out, int repeats)
{
  const std::vector<char>  raw = read_file(in);
  size_t                   pos = 0;
  const uint32_t           n   = take<uint32_t>(raw, pos);
  std::vector<loaded_case> cases(n);
  for (loaded_case& c : cases) {
    c.h    = take<case_header>(raw, pos);
    c.cfg  = config_of(c.h);
    c.grid = std::make_unique<resource_grid_impl>(c.h.grid_nof_ports, 14, NRE * c.h.grid_nof_prb);
    c.grid->set_all_zero();
    std::vector<unsigned> sets;
    unsigned              L = 0;
    for (unsigned p = 0; p < c.h.nof_antenna_ports; ++p) {
      const srs_information info = get_srs_information(c.cfg.resource, p);
      L                          = info.sequence_length;
      if (std::find(sets.begin(), sets.end(), info.mapping_initial_subcarrier) == sets.end()) {
        sets.push_back(info.mapping_initial_subcarrier);
      }
    }
    std::sort(sets.begin(), sets.end());
    for (unsigned r = 0; r < c.h.nof_rx_ports; ++r) {
      for (unsigned s = 0; s < c.h.nof_symbols; ++s) {
        span<cbf16_t> view = c.grid->get_writer().get_view(c.h.rx_ports[r], c.h.start_symbol + s);
        for (unsigned k0 : sets) {
          for (unsigned i = 0; i < L; ++i) {
            const uint32_t w = take<uint32_t>(raw, pos);
            cbf16_t        v;
            v.real                        = bf16_t(static_cast<uint16_t>(w & 0xffffU));
            v.imag                        = bf16_t(static_cast<uint16_t>(w >> 16));
            view[k0 + i * c.h.comb_size] = v;
          }
        }
      }
    }
  }
  time_alignment_estimator_dft_impl::collection_dft_processors dfts;
  for (unsigned size = time_alignment_estimator_dft_impl::min_dft_size; size <= time_alignment_estimator_dft_impl::max_dft_size;
       size *= 2) {
    dft_processor::configuration cfg = {size, dft_processor::direction::INVERSE};
    dfts.emplace(size, std::make_unique<dft_processor_generic_impl>(cfg));
  }
  auto spy_owner = std::make_unique<recording_ta_estimator>(std::make_unique<time_alignment_estimator_dft_impl>(std::move(dfts)));
  recording_ta_estimator*                  spy = spy_owner.get();
  srs_estimator_generic_impl::dependencies deps;
  deps.sequence_generator = std::make_unique<low_papr_sequence_generator_impl>();
  deps.ta_estimator       = std::move(spy_owner);
  srs_estimator_generic_impl estimator(std::move(deps), MAX_RB);

  std::ofstream f(out, std::ios::binary);
  for (const loaded_case& c : cases) {
    spy->seen.clear();
    const srs_estimator_result r = estimator.estimate(c.grid->get_reader(), c.cfg);
    case_result                o = {};
    for (unsigned rx = 0; rx < c.h.nof_rx_ports; ++rx) {
      for (unsigned tx = 0; tx < c.h.nof_antenna_ports; ++tx) {
        const cf_t v        = r.channel_matrix.get_coefficient(rx, tx);
        o.channel[rx][tx][0] = v.real(), o.channel[rx][tx][1] = v.imag();
      }
    }
    o.epre_dB = r.epre_dB.value_or(NAN), o.noise_var = r.noise_variance.value_or(NAN);
    o.time_alignment = r.time_alignment.time_alignment, o.resolution = r.time_alignment.resolution;
    o.ta_min = r.time_alignment.min, o.ta_max = r.time_alignment.max;
    for (unsigned p = 0; p < spy->seen.size() && p < 4; ++p) {
      o.ta_port[p] = spy->seen[p];
    }
    f.write(reinterpret_cast<const char*>(&o), sizeof(o));
  }
  if (repeats > 0) {
    double     sink = 0;
    const auto t0   = std::chrono::steady_clock::now();
    for (int rep = 0; rep < repeats; ++rep) {
      for (const loaded_case& c : cases) {
        sink += estimator.estimate(c.grid->get_reader(), c.cfg).noise_variance.value_or(0.0F);
      }
    }
    const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
    std::printf("ns_per_pass %.1f (%g)\n", ns / repeats, sink);
  }
  return 0;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc >= 3 && std::string(argv[1]) == "table") {
    return table(argv[2]);
  }
  if (argc >= 4 && std::string(argv[1]) == "estimate") {
    return estimate(argv[2], argv[3], argc > 4 ? std::atoi(argv[4]) : 0);
  }
  std::fprintf(stderr, "usage: %s table OUT | estimate IN OUT [REPEATS]\n", argv[0]);
  return 2;
}
