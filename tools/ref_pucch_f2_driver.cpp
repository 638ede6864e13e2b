// Driver of tools/gen_pucch_f2_golden.py: runs the reference's PUCCH Format 2 receive path -- dmrs_pucch_estimator_format2
// over port_channel_estimator_average_impl (filter smoothing, average in time, no CFO compensation: the settings of
// signal_processor_factories.cpp:140), pucch_demodulator_format2 over the generic ZF equaliser and the demodulation
// mapper, and uci_decoder_impl -- all compiled from the reference tree where it lies, never committed, over cases the
// tool writes, for the fixture tests/golden/pucch_f2.npz.
//
//   ref_pucch_f2_driver process IN OUT [REPEATS]
//       IN: u32 n; per case the `case_header`, then grid_nof_ports x nof_symbols x 12 nof_prb u32 (re | im << 16, bf16):
//       the allocation's REs, each symbol at the PRBs of its hop. OUT per case: 16 nof_prb nof_symbols int8 LLRs; per
//       listed port f32 noise variance, f32 RSRP, f32 EPRE, f64 time alignment (s), f32 CFO (Hz, NaN without); the
//       combined channel_state_information as f32 EPRE dB, f32 RSRP dB, f32 SINR dB, f64 time alignment (s), f32 CFO
//       (Hz), NaN for what is not set; then nof_uci_bits bytes (2 where the decoder wrote nothing) and one status byte
//       (1 valid). REPEATS > 0: also times REPEATS passes over every case on this core, "ns_per_pass <value>".
//   ref_pucch_f2_driver decode IN OUT
//       IN: u32 n; per field u32 A, u32 E and E int8 LLRs. OUT: per field A bytes and one status byte.
#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include "lib/phy/support/interpolator/interpolator_linear_impl.h"
#include "lib/phy/support/resource_grid_impl.h"
#include "lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.h"
#include "lib/phy/upper/channel_modulation/demodulation_mapper_impl.h"
#include "lib/phy/upper/channel_processors/pucch/pucch_demodulator_format2.h"
#include "lib/phy/upper/channel_processors/uci/uci_decoder_impl.h"
#include "lib/phy/upper/equalization/channel_equalizer_generic_impl.h"
#include "lib/phy/upper/sequence_generators/pseudo_random_generator_impl.h"
#include "lib/phy/upper/signal_processors/port_channel_estimator_average_impl.h"
#include "lib/phy/upper/signal_processors/pucch/dmrs_pucch_estimator_format2.h"
#include "crc_calculator_generic_impl.h"
#include "polar/polar_code_impl.h"
#include "polar/polar_deallocator_impl.h"
#include "polar/polar_decoder_impl.h"
#include "polar/polar_encoder_impl.h"
#include "polar/polar_rate_dematcher_impl.h"
#include "short/short_block_detector_impl.h"
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
  uint32_t slot_index, numerology, cp_extended, starting_prb, second_hop_prb, nof_prb, start_symbol, nof_symbols, rnti,
      n_id, n_id_0, nof_ports, ports[4], grid_nof_ports, grid_nof_prb, nof_uci_bits;
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

template <typename T>
void put(std::ofstream& out, const T* data, size_t count)
{
  out.write(reinterpret_cast<const char*>(data), count * sizeof(T));
}

std::unique_ptr<uci_decoder_impl> make_decoder()
{
  return std::make_unique<uci_decoder_impl>(
      std::make_unique<short_block_detector_impl>(), std::make_unique<polar_code_impl>(),
      std::make_unique<polar_rate_dematcher_impl>(),
      std::make_unique<polar_decoder_impl>(std::make_unique<polar_encoder_impl>(), 10),
      std::make_unique<polar_deallocator_impl>(), std::make_unique<crc_calculator_generic_impl>(crc_generator_poly::CRC6),
      std::make_unique<crc_calculator_generic_impl>(crc_generator_poly::CRC11));
}

struct loaded_case {
  case_header                         h;
  std::unique_ptr<resource_grid_impl> grid;
};

struct receiver {
  std::unique_ptr<dmrs_pucch_estimator_format2> estimator;
  std::unique_ptr<pucch_demodulator_format2>    demodulator;
  std::unique_ptr<uci_decoder_impl>             decoder;
  channel_estimate                              estimates;
  std::vector<log_likelihood_ratio>             llr;

  receiver()
  {
    time_alignment_estimator_dft_impl::collection_dft_processors dfts;
    for (unsigned size = time_alignment_estimator_dft_impl::min_dft_size;
         size <= time_alignment_estimator_dft_impl::max_dft_size;
         size *= 2) {
      dft_processor::configuration cfg = {size, dft_processor::direction::INVERSE};
      dfts.emplace(size, std::make_unique<dft_processor_generic_impl>(cfg));
    }
    auto port_estimator = std::make_unique<port_channel_estimator_average_impl>(
        std::make_unique<interpolator_linear_impl>(), std::make_unique<time_alignment_estimator_dft_impl>(std::move(dfts)),
        port_channel_estimator_fd_smoothing_strategy::filter, port_channel_estimator_td_interpolation_strategy::average,
        /* compensate_cfo = */ false);
    estimator   = std::make_unique<dmrs_pucch_estimator_format2>(std::make_unique<pseudo_random_generator_impl>(),
                                                               std::move(port_estimator));
    demodulator = std::make_unique<pucch_demodulator_format2>(
        std::make_unique<channel_equalizer_generic_impl>(channel_equalizer_algorithm_type::zf),
        std::make_unique<demodulation_mapper_impl>(), std::make_unique<pseudo_random_generator_impl>());
    decoder = make_decoder();
  }

  /// pucch_processor_impl::process(grid, format2_configuration) from the estimator on (:163-213).
  uci_status run(const loaded_case& c, span<uint8_t> bits)
  {
    const case_header&                          h = c.h;
    const cyclic_prefix                         cp = h.cp_extended ? cyclic_prefix::EXTENDED : cyclic_prefix::NORMAL;
    dmrs_pucch_estimator::format2_configuration ec;
    ec.slot               = slot_point(h.numerology, h.slot_index);
    ec.cp                 = cp;
    ec.group_hopping      = pucch_group_hopping::NEITHER;
    ec.start_symbol_index = h.start_symbol;
    ec.nof_symbols        = h.nof_symbols;
    ec.starting_prb       = h.starting_prb;
    if (h.second_hop_prb != 0xffffU) {
      ec.second_hop_prb = h.second_hop_prb;
    }
    ec.nof_prb = h.nof_prb;
    ec.n_id_0  = h.n_id_0;
    pucch_demodulator::format2_configuration dc;
    for (unsigned p = 0; p < h.nof_ports; ++p) {
      ec.ports.push_back(static_cast<uint8_t>(h.ports[p]));
      dc.rx_ports.push_back(static_cast<uint8_t>(h.ports[p]));
    }
    channel_estimate::channel_estimate_dimensions dims;
    dims.nof_prb       = h.grid_nof_prb;
    dims.nof_symbols   = get_nsymb_per_slot(cp);
    dims.nof_rx_ports  = h.nof_ports;
    dims.nof_tx_layers = 1;
    estimates.resize(dims);
    estimator->estimate(estimates, c.grid->get_reader(), ec);
    dc.first_prb          = h.starting_prb;
    dc.second_hop_prb     = ec.second_hop_prb;
    dc.nof_prb            = h.nof_prb;
    dc.start_symbol_index = h.start_symbol;
    dc.nof_symbols        = h.nof_symbols;
    dc.rnti               = h.rnti;
    dc.n_id               = h.n_id;
    llr.resize(16 * h.nof_prb * h.nof_symbols);
    demodulator->demodulate(llr, c.grid->get_reader(), estimates, dc);
    return decoder->decode(bits, llr, {modulation_scheme::QPSK});
  }
};

int process(const char* in, const char* out, int repeats)
{
  const std::vector<char>  raw = read_file(in);
  size_t                   pos = 0;
  const uint32_t           n   = take<uint32_t>(raw, pos);
  std::vector<loaded_case> cases(n);
  for (loaded_case& c : cases) {
    c.h    = take<case_header>(raw, pos);
    c.grid = std::make_unique<resource_grid_impl>(c.h.grid_nof_ports, 14, NRE * c.h.grid_nof_prb);
    c.grid->set_all_zero();
    for (unsigned p = 0; p < c.h.grid_nof_ports; ++p) {
      for (unsigned s = 0; s < c.h.nof_symbols; ++s) {
        const unsigned prb  = (s > 0 && c.h.second_hop_prb != 0xffffU) ? c.h.second_hop_prb : c.h.starting_prb;
        span<cbf16_t>  view = c.grid->get_writer().get_view(p, c.h.start_symbol + s);
        for (unsigned k = 0; k < NRE * c.h.nof_prb; ++k) {
          const uint32_t w = take<uint32_t>(raw, pos);
          cbf16_t        v;
          v.real              = bf16_t(static_cast<uint16_t>(w & 0xffffU));
          v.imag              = bf16_t(static_cast<uint16_t>(w >> 16));
          view[NRE * prb + k] = v;
        }
      }
    }
  }
  receiver      rx;
  std::ofstream f(out, std::ios::binary);
  for (const loaded_case& c : cases) {
    std::vector<uint8_t> bits(c.h.nof_uci_bits, 2);
    const uint8_t        valid = rx.run(c, bits) == uci_status::valid ? 1 : 0;
    std::vector<int8_t>  llrs;
    for (log_likelihood_ratio v : rx.llr) {
      llrs.push_back(v.to_value_type());
    }
    put(f, llrs.data(), llrs.size());
    for (unsigned p = 0; p < c.h.nof_ports; ++p) {
      const float  v[3] = {rx.estimates.get_noise_variance(p), rx.estimates.get_rsrp(p, 0), rx.estimates.get_epre(p)};
      const double ta   = rx.estimates.get_time_alignment(p, 0).to_seconds();
      const float  cfo  = rx.estimates.get_cfo_Hz(p, 0).value_or(NAN);
      put(f, v, 3);
      put(f, &ta, 1);
      put(f, &cfo, 1);
    }
    // The ports combined as the processor reports them (pucch_processor_impl.cpp:188); NaN for a value it leaves unset.
    channel_state_information csi;
    rx.estimates.get_channel_state_information(csi);
    const float  db[3]  = {csi.get_epre_dB().value_or(NAN), csi.get_rsrp_dB().value_or(NAN), csi.get_sinr_dB().value_or(NAN)};
    const double csi_ta = csi.get_time_alignment().has_value() ? csi.get_time_alignment()->to_seconds() : NAN;
    const float  csi_cfo = csi.get_cfo_Hz().value_or(NAN);
    put(f, db, 3);
    put(f, &csi_ta, 1);
    put(f, &csi_cfo, 1);
    put(f, bits.data(), bits.size());
    put(f, &valid, 1);
  }
  if (repeats > 0) {
    unsigned             sink = 0;
    std::vector<uint8_t> bits(2048);
    const auto           t0 = std::chrono::steady_clock::now();
    for (int rep = 0; rep < repeats; ++rep) {
      for (const loaded_case& c : cases) {
        sink += static_cast<unsigned>(rx.run(c, span<uint8_t>(bits).first(c.h.nof_uci_bits))) + bits[0];
      }
    }
    const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
    std::printf("ns_per_pass %.1f (%u)\n", ns / repeats, sink);
  }
  return 0;
}

int decode(const char* in, const char* out)
{
  const std::vector<char>           raw = read_file(in);
  size_t                            pos = 0;
  const uint32_t                    n   = take<uint32_t>(raw, pos);
  std::unique_ptr<uci_decoder_impl> decoder = make_decoder();
  std::ofstream                     f(out, std::ios::binary);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t                    a = take<uint32_t>(raw, pos), e = take<uint32_t>(raw, pos);
    std::vector<log_likelihood_ratio> llr;
    for (uint32_t j = 0; j < e; ++j) {
      llr.push_back(log_likelihood_ratio(take<int8_t>(raw, pos)));
    }
    std::vector<uint8_t> bits(a, 2);
    const uint8_t        valid = decoder->decode(bits, llr, {modulation_scheme::QPSK}) == uci_status::valid ? 1 : 0;
    put(f, bits.data(), bits.size());
    put(f, &valid, 1);
  }
  return 0;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc >= 4 && std::string(argv[1]) == "process") {
    return process(argv[2], argv[3], argc > 4 ? std::atoi(argv[4]) : 0);
  }
  if (argc >= 4 && std::string(argv[1]) == "decode") {
    return decode(argv[2], argv[3]);
  }
  std::fprintf(stderr, "usage: %s process IN OUT [REPEATS] | decode IN OUT\n", argv[0]);
  return 2;
}
