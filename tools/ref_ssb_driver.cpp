// Driver of tools/gen_ssb_golden.py: runs the reference's ssb_processor_impl (its PBCH encoder and modulator, the PBCH
// DM-RS, PSS and SSS processors with the LUT modulation mapper and a resource grid; all compiled from the reference
// tree where it lies, never committed) over cases the tool writes, for the fixture tests/golden/ssb.npz.
//
//   ref_ssb_driver process IN OUT [REPEATS]  IN: u32 nof_cases, then per case the `case_header` below. OUT per case:
//                                            u32 l_start and k_start (as ssb_processor_impl::process derives them),
//                                            864 bytes (the rate-matched bits of pbch_encoder_impl), a float (the PSS
//                                            amplitude process() computes from beta_pss), u32 m and m x 4 u32 (port,
//                                            symbol, subcarrier, word: every grid word process() wrote on a sentinel
//                                            grid; re in the low half, bf16 bit patterns).
//                                            REPEATS > 0: also times REPEATS passes over every case on this core,
//                                            "ns_per_pass <value>".
#include "crc_calculator_generic_impl.h"
#include "lib/phy/support/resource_grid_impl.h"
#include "lib/phy/upper/channel_modulation/modulation_mapper_lut_impl.h"
#include "lib/phy/upper/channel_processors/ssb/pbch_encoder_impl.h"
#include "lib/phy/upper/channel_processors/ssb/pbch_modulator_impl.h"
#include "lib/phy/upper/channel_processors/ssb/ssb_processor_impl.h"
#include "lib/phy/upper/sequence_generators/pseudo_random_generator_impl.h"
#include "lib/phy/upper/signal_processors/dmrs_pbch_processor_impl.h"
#include "lib/phy/upper/signal_processors/pss_processor_impl.h"
#include "lib/phy/upper/signal_processors/sss_processor_impl.h"
#include "polar/polar_allocator_impl.h"
#include "polar/polar_code_impl.h"
#include "polar/polar_encoder_impl.h"
#include "polar/polar_interleaver_impl.h"
#include "polar/polar_rate_matcher_impl.h"
#include "srsran/phy/support/resource_grid_reader.h"
#include "srsran/phy/support/resource_grid_writer.h"
#include "srsran/ran/ssb/ssb_mapping.h"
#include "srsran/support/math/math_utils.h"
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
  uint32_t phys_cell_id, ssb_idx, L_max, pattern_case, common_scs, offset_to_pointA, subcarrier_offset;
  uint32_t sfn, slot_index, hrf;  // slot_index: within the half frame, in slots of the SS/PBCH block's SCS
  float    beta_pss_dB;
  uint32_t nof_ports;
  uint8_t  ports[4];
  uint8_t  payload[24];  // one bit each
  uint32_t grid_nof_prb, grid_nof_ports;
};
static_assert(sizeof(case_header) == 84, "case_header layout (mirrored by tools/gen_ssb_golden.py)");

constexpr uint16_t SENTINEL = 0x7fc1;  // a NaN pattern no product rounds to

template <typename T>
void put(std::ofstream& out, const T* data, size_t count)
{
  out.write(reinterpret_cast<const char*>(data), count * sizeof(T));
}

std::unique_ptr<pbch_encoder_impl> make_encoder()
{
  return std::make_unique<pbch_encoder_impl>(
      std::make_unique<crc_calculator_generic_impl>(crc_generator_poly::CRC24C), std::make_unique<pseudo_random_generator_impl>(),
      std::make_unique<polar_interleaver_impl>(), std::make_unique<polar_allocator_impl>(), std::make_unique<polar_code_impl>(),
      std::make_unique<polar_encoder_impl>(), std::make_unique<polar_rate_matcher_impl>());
}

std::unique_ptr<ssb_processor_impl> make_processor()
{
  ssb_processor_config config;
  config.encoder   = make_encoder();
  config.modulator = std::make_unique<pbch_modulator_impl>(std::make_unique<modulation_mapper_lut_impl>(),
                                                           std::make_unique<pseudo_random_generator_impl>());
  config.dmrs      = std::make_unique<dmrs_pbch_processor_impl>(std::make_unique<pseudo_random_generator_impl>());
  config.pss       = std::make_unique<pss_processor_impl>();
  config.sss       = std::make_unique<sss_processor_impl>();
  return std::make_unique<ssb_processor_impl>(std::move(config));
}

ssb_processor::pdu_t make_pdu(const case_header& h)
{
  const ssb_pattern_case pattern_case = static_cast<ssb_pattern_case>(h.pattern_case);
  const unsigned         numerology   = to_numerology_value(to_subcarrier_spacing(pattern_case));
  const unsigned         hrf_slots    = 5U << numerology;
  ssb_processor::pdu_t   pdu;
  pdu.slot              = slot_point(numerology, h.sfn, h.hrf * hrf_slots + h.slot_index);
  pdu.phys_cell_id      = h.phys_cell_id;
  pdu.beta_pss          = h.beta_pss_dB;
  pdu.ssb_idx           = h.ssb_idx;
  pdu.L_max             = h.L_max;
  pdu.common_scs        = to_subcarrier_spacing(h.common_scs);
  pdu.subcarrier_offset = h.subcarrier_offset;
  pdu.offset_to_pointA  = h.offset_to_pointA;
  pdu.pattern_case      = pattern_case;
  std::copy(h.payload, h.payload + 24, pdu.bch_payload.begin());
  pdu.ports.assign(h.ports, h.ports + h.nof_ports);
  return pdu;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc < 4 || std::strcmp(argv[1], "process") != 0) {
    std::fprintf(stderr, "usage: ref_ssb_driver process IN OUT [REPEATS]\n");
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
    std::fprintf(stderr, "ref_ssb_driver: input size\n");
    return 2;
  }
  std::vector<case_header>          headers(count);
  std::vector<ssb_processor::pdu_t> pdus;
  for (uint32_t i = 0; i != count; ++i) {
    std::memcpy(&headers[i], raw.data() + 4 + i * sizeof(case_header), sizeof(case_header));
    pdus.push_back(make_pdu(headers[i]));
  }

  std::ofstream                       out(argv[3], std::ios::binary);
  std::unique_ptr<ssb_processor_impl> processor = make_processor();
  std::unique_ptr<pbch_encoder_impl>  encoder   = make_encoder();
  for (uint32_t i = 0; i != count; ++i) {
    const case_header&          h   = headers[i];
    const ssb_processor::pdu_t& pdu = pdus[i];
    const uint32_t              where[2] = {
        ssb_get_l_first(pdu.pattern_case, pdu.ssb_idx) % 14,
        ssb_get_k_first(to_frequency_range(pdu.pattern_case), to_subcarrier_spacing(pdu.pattern_case), pdu.common_scs,
                                     pdu.offset_to_pointA, pdu.subcarrier_offset)};
    put(out, where, 2);

    pbch_encoder::pbch_msg_t msg;
    msg.N_id    = pdu.phys_cell_id;
    msg.ssb_idx = pdu.ssb_idx;
    msg.L_max   = pdu.L_max;
    msg.hrf     = pdu.slot.is_odd_hrf();
    msg.payload = pdu.bch_payload;
    msg.sfn     = pdu.slot.sfn();
    msg.k_ssb   = pdu.subcarrier_offset;
    std::vector<uint8_t> encoded(pbch_encoder::E);
    encoder->encode(encoded, msg);
    put(out, encoded.data(), encoded.size());

    const float pss_amplitude = convert_dB_to_amplitude(pdu.beta_pss);
    put(out, &pss_amplitude, 1);

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
    processor->process(grid.get_writer(), pdu);
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
    uint32_t prb = 0;
    for (const case_header& h : headers) {
      prb = std::max(prb, h.grid_nof_prb);
    }
    resource_grid_impl grid(4, 14, 12 * prb);
    grid.set_all_zero();
    auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < repeats; ++r) {
      for (uint32_t i = 0; i != count; ++i) {
        processor->process(grid.get_writer(), pdus[i]);
      }
    }
    auto     t1   = std::chrono::steady_clock::now();
    unsigned sink = grid.get_reader().get_view(headers[0].ports[0], 5)[60].real.value();
    std::printf("ns_per_pass %.1f (sink %u)\n", std::chrono::duration<double, std::nano>(t1 - t0).count() / repeats, sink);
  }
  return 0;
}
