// Driver of tools/gen_csi_rs_golden.py: runs the reference's nzp_csi_rs_generator_impl (with its pseudo-random
// generator, the generic channel precoder, the resource grid mapper and a resource grid; all compiled from the
// reference tree where it lies, never committed) over cases the tool writes, for the fixture tests/golden/csi_rs.npz.
//
//   ref_csi_rs_driver process IN OUT [REPEATS]  IN: u32 nof_cases, then per case the `case_header` below. OUT per case:
//                                               u32 m and m x 4 u32 (port, symbol, subcarrier, word: every grid word
//                                               map() wrote on a sentinel grid; re in the low half, bf16 bit patterns).
//                                               REPEATS > 0: also times REPEATS passes over every case on this core,
//                                               "ns_per_pass <value>".
#include "lib/phy/generic_functions/precoding/channel_precoder_generic.h"
#include "lib/phy/support/resource_grid_impl.h"
#include "lib/phy/support/resource_grid_mapper_impl.h"
#include "lib/phy/upper/sequence_generators/pseudo_random_generator_impl.h"
#include "lib/phy/upper/signal_processors/nzp_csi_rs_generator_impl.h"
#include "srsran/phy/support/precoding_configuration.h"
#include "srsran/phy/support/resource_grid_reader.h"
#include "srsran/phy/support/resource_grid_writer.h"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>

using namespace srsran;

namespace {

struct case_header {
  uint32_t numerology, n_slot, cp;  // cp: 0 normal, 1 extended
  uint32_t start_rb, nof_rb, row, k_ref, symbol_l0, symbol_l1;
  uint32_t cdm, freq_density;  // the values of csi_rs_cdm_type and csi_rs_freq_density_type
  uint32_t scrambling_id;
  float    amplitude;
  uint32_t nof_ports;
  float    weights[32];  // [port][layer] (re, im)
  uint32_t grid_nof_prb, grid_nof_ports;
};
static_assert(sizeof(case_header) == 192, "case_header layout (mirrored by tools/gen_csi_rs_golden.py)");

constexpr uint16_t SENTINEL = 0x7fc1;  // a NaN pattern no product rounds to

template <typename T>
void put(std::ofstream& out, const T* data, size_t count)
{
  out.write(reinterpret_cast<const char*>(data), count * sizeof(T));
}

nzp_csi_rs_generator::config_t make_config(const case_header& h)
{
  nzp_csi_rs_generator::config_t c;
  c.slot                     = slot_point(h.numerology, h.n_slot);
  c.cp                       = h.cp != 0 ? cyclic_prefix::EXTENDED : cyclic_prefix::NORMAL;
  c.start_rb                 = h.start_rb;
  c.nof_rb                   = h.nof_rb;
  c.csi_rs_mapping_table_row = h.row;
  c.freq_allocation_ref_idx  = {h.k_ref};
  c.symbol_l0                = h.symbol_l0;
  c.symbol_l1                = h.symbol_l1;
  c.cdm                      = static_cast<csi_rs_cdm_type>(h.cdm);
  c.freq_density             = static_cast<csi_rs_freq_density_type>(h.freq_density);
  c.scrambling_id            = h.scrambling_id;
  c.amplitude                = h.amplitude;
  c.precoding                = precoding_configuration(h.nof_ports, h.nof_ports, 1, MAX_RB);
  for (unsigned p = 0; p != h.nof_ports; ++p) {
    for (unsigned q = 0; q != h.nof_ports; ++q) {
      c.precoding.set_coefficient(cf_t(h.weights[2 * (4 * p + q)], h.weights[2 * (4 * p + q) + 1]), q, p, 0);
    }
  }
  return c;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc < 4 || std::strcmp(argv[1], "process") != 0) {
    std::fprintf(stderr, "usage: ref_csi_rs_driver process IN OUT [REPEATS]\n");
    return 2;
  }
  std::ifstream        in(argv[2], std::ios::binary);
  std::vector<uint8_t> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  uint32_t             count = 0;
  if (raw.size() < 4) {
    return 2;
  }
  std::memcpy(&count, raw.data(), 4);
  if (raw.size() != 4 + static_cast<size_t>(count) * sizeof(case_header)) {
    std::fprintf(stderr, "ref_csi_rs_driver: input size\n");
    return 2;
  }
  std::vector<case_header>                    headers(count);
  std::vector<nzp_csi_rs_generator::config_t> configs;
  for (uint32_t i = 0; i != count; ++i) {
    std::memcpy(&headers[i], raw.data() + 4 + i * sizeof(case_header), sizeof(case_header));
    configs.push_back(make_config(headers[i]));
  }

  auto generator = std::make_unique<nzp_csi_rs_generator_impl>(
      std::make_unique<pseudo_random_generator_impl>(),
      std::make_unique<resource_grid_mapper_impl>(std::make_unique<channel_precoder_generic>()));
  std::ofstream out(argv[3], std::ios::binary);
  for (uint32_t i = 0; i != count; ++i) {
    const case_header& h = headers[i];
    resource_grid_impl grid(h.grid_nof_ports, 14, 12 * h.grid_nof_prb);
    cbf16_t            mark;
    mark.real = bf16_t(SENTINEL);
    mark.imag = bf16_t(SENTINEL);
    for (unsigned p = 0; p != h.grid_nof_ports; ++p) {
      for (unsigned l = 0; l != 14; ++l) {
        span<cbf16_t> view = grid.get_writer().get_view(p, l);
        std::fill(view.begin(), view.end(), mark);
      }
    }
    generator->map(grid.get_writer(), configs[i]);
    std::vector<uint32_t> written;
    for (unsigned p = 0; p != h.grid_nof_ports; ++p) {
      for (unsigned l = 0; l != 14; ++l) {
        span<const cbf16_t> view = grid.get_reader().get_view(p, l);
        for (unsigned k = 0; k != view.size(); ++k) {
          if (view[k] != mark) {
            written.insert(written.end(),
                           {p, l, k, static_cast<uint32_t>(view[k].real.value()) | (static_cast<uint32_t>(view[k].imag.value()) << 16)});
          }
        }
      }
    }
    const uint32_t m = written.size() / 4;
    put(out, &m, 1);
    put(out, written.data(), written.size());
  }

  const int repeats = argc > 4 ? std::atoi(argv[4]) : 0;
  if (repeats > 0 && count > 0) {
    resource_grid_impl grid(headers[0].grid_nof_ports, 14, 12 * headers[0].grid_nof_prb);
    grid.set_all_zero();
    auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < repeats; ++r) {
      for (uint32_t i = 0; i != count; ++i) {
        generator->map(grid.get_writer(), configs[i]);
      }
    }
    auto     t1   = std::chrono::steady_clock::now();
    unsigned sink = grid.get_reader().get_view(0, headers[0].symbol_l0)[12 * headers[0].start_rb].real.value();
    std::printf("ns_per_pass %.1f (sink %u)\n", std::chrono::duration<double, std::nano>(t1 - t0).count() / repeats, sink);
  }
  return 0;
}
