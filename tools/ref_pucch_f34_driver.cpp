// Driver of tools/gen_pucch_f34_golden.py: runs the reference's PUCCH Format 3 / 4 receive path --
// dmrs_pucch_estimator_formats3_4 over port_channel_estimator_average_impl (mean smoothing, average in time, no CFO
// compensation: the settings of signal_processor_factories.cpp:146), pucch_demodulator_format3 / format4 over the
// generic ZF equaliser, transform_precoder_dft_impl and the demodulation mapper, and uci_decoder_impl -- all compiled
// from the reference tree where it lies, never committed, over cases the tool writes, for the fixture
// tests/golden/pucch_f34.npz. The transform precoder gets an exact direct DFT (float64 accumulation) behind the
// dft_processor interface: this build's generic DFT has no 12 N sizes (oracle/ref/ref_pusch_demod.cpp notes the same).
//
//   ref_pucch_f34_driver process IN OUT [REPEATS]
//       IN: u32 n; per case the `case_header`, then grid_nof_ports x nof_symbols x 12 nof_prb u32 (re | im << 16, bf16):
//       the allocation's REs, each symbol at the PRBs of its hop (the second from symbol nof_symbols / 2 on). OUT per
//       case: E int8 LLRs; per listed port f32 noise variance, f32 RSRP, f32 EPRE, f64 time alignment (s), f32 CFO (Hz,
//       NaN without); the combined channel_state_information as f32 EPRE dB, f32 RSRP dB, f32 SINR dB, f64 time
//       alignment (s), f32 CFO (Hz), NaN for what is not set; then nof_uci_bits bytes (2 where the decoder wrote
//       nothing) and one status byte (1 valid). REPEATS > 0: also times REPEATS passes, "ns_per_pass <value>".
//   ref_pucch_f34_driver decode IN OUT
//       IN: u32 n; per field u32 A, u32 E, u32 pi2_bpsk and E int8 LLRs. OUT: per field A bytes and one status byte.
//   ref_pucch_f34_driver tables OUT
//       OUT: for nof_symbols 4..14, hopping 0..1, additional_dmrs 0..1 (in that nesting) the u16 DM-RS symbol mask of
//       get_pucch_formats3_4_dmrs_symbol_mask; then w_n(k) of pucch_orthogonal_sequence_format4 for length 2 (n = 0, 1)
//       and length 4 (n = 0..3), 12 x (f32 re, f32 im) each.
#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include "lib/phy/generic_functions/transform_precoding/transform_precoder_dft_impl.h"
#include "lib/phy/support/interpolator/interpolator_linear_impl.h"
#include "lib/phy/support/resource_grid_impl.h"
#include "lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.h"
#include "lib/phy/upper/channel_modulation/demodulation_mapper_impl.h"
#include "lib/phy/upper/channel_processors/pucch/pucch_demodulator_format3.h"
#include "lib/phy/upper/channel_processors/pucch/pucch_demodulator_format4.h"
#include "lib/phy/upper/channel_processors/uci/uci_decoder_impl.h"
#include "lib/phy/upper/equalization/channel_equalizer_generic_impl.h"
#include "lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.h"
#include "lib/phy/upper/sequence_generators/pseudo_random_generator_impl.h"
#include "lib/phy/upper/signal_processors/port_channel_estimator_average_impl.h"
#include "lib/phy/upper/signal_processors/pucch/dmrs_pucch_estimator_formats3_4.h"
#include "srsran/phy/upper/pucch_formats3_4_helpers.h"
#include "srsran/phy/upper/pucch_orthogonal_sequence.h"
#include "crc_calculator_generic_impl.h"
#include "polar/polar_code_impl.h"
#include "polar/polar_deallocator_impl.h"
#include "polar/polar_decoder_impl.h"
#include "polar/polar_encoder_impl.h"
#include "polar/polar_rate_dematcher_impl.h"
#include "short/short_block_detector_impl.h"
#include <chrono>
#include <cmath>
#include <complex>
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
  uint32_t format, slot_index, numerology, cp_extended, starting_prb, second_hop_prb, nof_prb, start_symbol,
      nof_symbols, additional_dmrs, pi2_bpsk, occ_length, occ_index, rnti, n_id_scrambling, n_id_hopping, nof_ports,
      ports[4], grid_nof_ports, grid_nof_prb, nof_uci_bits;
};

/// The inverse (or forward) DFT as its defining sum, accumulated in double.
class direct_dft : public dft_processor
{
public:
  direct_dft(unsigned size, direction dir_) : dir(dir_), in(size), out(size), root(size)
  {
    const double sign = dir == direction::INVERSE ? 1.0 : -1.0;
    for (unsigned k = 0; k != size; ++k) {
      root[k] = std::polar(1.0, sign * 2.0 * M_PI * k / size);
    }
  }
  direction        get_direction() const override { return dir; }
  unsigned         get_size() const override { return in.size(); }
  span<cf_t>       get_input() override { return in; }
  span<const cf_t> run() override
  {
    const unsigned m = in.size();
    for (unsigned n = 0; n != m; ++n) {
      std::complex<double> acc = 0;
      for (unsigned k = 0; k != m; ++k) {
        acc += std::complex<double>(in[k]) * root[(static_cast<uint64_t>(k) * n) % m];
      }
      out[n] = cf_t(static_cast<float>(acc.real()), static_cast<float>(acc.imag()));
    }
    return out;
  }

private:
  direction                         dir;
  std::vector<cf_t>                 in, out;
  std::vector<std::complex<double>> root;
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

std::unique_ptr<transform_precoder> make_precoder()
{
  transform_precoder_dft_impl::collection_dft_processors dfts;
  for (unsigned nof_prb = 1; nof_prb <= 16; ++nof_prb) {
    if (transform_precoding::is_nof_prbs_valid(nof_prb)) {
      dfts.emplace(nof_prb, std::make_unique<direct_dft>(NRE * nof_prb, dft_processor::direction::INVERSE));
    }
  }
  return std::make_unique<transform_precoder_dft_impl>(std::move(dfts));
}

unsigned nof_llrs(const case_header& h)
{
  const unsigned n_data =
      h.nof_symbols -
      get_pucch_formats3_4_dmrs_symbol_mask(h.nof_symbols, h.second_hop_prb != 0xffffU, h.additional_dmrs != 0).count();
  const unsigned qm = h.pi2_bpsk ? 1 : 2;
  return h.format == 4 ? NRE * n_data * qm / h.occ_length : NRE * h.nof_prb * n_data * qm;
}

struct loaded_case {
  case_header                         h;
  std::unique_ptr<resource_grid_impl> grid;
};

struct receiver {
  std::unique_ptr<dmrs_pucch_estimator_formats3_4> estimator;
  std::unique_ptr<pucch_demodulator_format3>       demodulator3;
  std::unique_ptr<pucch_demodulator_format4>       demodulator4;
  std::unique_ptr<uci_decoder_impl>                decoder;
  channel_estimate                                 estimates;
  std::vector<log_likelihood_ratio>                llr;

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
        port_channel_estimator_fd_smoothing_strategy::mean, port_channel_estimator_td_interpolation_strategy::average,
        /* compensate_cfo = */ false);
    estimator    = std::make_unique<dmrs_pucch_estimator_formats3_4>(std::make_unique<pseudo_random_generator_impl>(),
                                                                  std::make_unique<low_papr_sequence_generator_impl>(),
                                                                  std::move(port_estimator));
    demodulator3 = std::make_unique<pucch_demodulator_format3>(
        std::make_unique<channel_equalizer_generic_impl>(channel_equalizer_algorithm_type::zf),
        std::make_unique<demodulation_mapper_impl>(), std::make_unique<pseudo_random_generator_impl>(), make_precoder());
    demodulator4 = std::make_unique<pucch_demodulator_format4>(
        std::make_unique<channel_equalizer_generic_impl>(channel_equalizer_algorithm_type::zf),
        std::make_unique<demodulation_mapper_impl>(), std::make_unique<pseudo_random_generator_impl>(), make_precoder());
    decoder = make_decoder();
  }

  /// pucch_processor_impl::process(grid, format3_configuration / format4_configuration) from the estimator on.
  uci_status run(const loaded_case& c, span<uint8_t> bits)
  {
    const case_header&      h  = c.h;
    const cyclic_prefix     cp = h.cp_extended ? cyclic_prefix::EXTENDED : cyclic_prefix::NORMAL;
    std::optional<unsigned> second_hop;
    if (h.second_hop_prb != 0xffffU) {
      second_hop = h.second_hop_prb;
    }
    channel_estimate::channel_estimate_dimensions dims;
    dims.nof_prb       = h.grid_nof_prb;
    dims.nof_symbols   = get_nsymb_per_slot(cp);
    dims.nof_rx_ports  = h.nof_ports;
    dims.nof_tx_layers = 1;
    estimates.resize(dims);
    llr.resize(nof_llrs(h));
    if (h.format == 3) {
      dmrs_pucch_estimator::format3_configuration ec;
      pucch_demodulator::format3_configuration    dc;
      ec.slot               = slot_point(h.numerology, h.slot_index);
      ec.cp                 = cp;
      ec.group_hopping      = pucch_group_hopping::NEITHER;
      ec.start_symbol_index = h.start_symbol;
      ec.nof_symbols        = h.nof_symbols;
      ec.starting_prb       = h.starting_prb;
      ec.second_hop_prb     = second_hop;
      ec.nof_prb            = h.nof_prb;
      ec.n_id               = h.n_id_hopping;
      ec.additional_dmrs    = h.additional_dmrs != 0;
      for (unsigned p = 0; p < h.nof_ports; ++p) {
        ec.ports.push_back(static_cast<uint8_t>(h.ports[p]));
        dc.rx_ports.push_back(static_cast<uint8_t>(h.ports[p]));
      }
      estimator->estimate(estimates, c.grid->get_reader(), ec);
      dc.first_prb          = h.starting_prb;
      dc.second_hop_prb     = second_hop;
      dc.nof_prb            = h.nof_prb;
      dc.start_symbol_index = h.start_symbol;
      dc.nof_symbols        = h.nof_symbols;
      dc.rnti               = h.rnti;
      dc.n_id               = h.n_id_scrambling;
      dc.additional_dmrs    = h.additional_dmrs != 0;
      dc.pi2_bpsk           = h.pi2_bpsk != 0;
      demodulator3->demodulate(llr, c.grid->get_reader(), estimates, dc);
    } else {
      dmrs_pucch_estimator::format4_configuration ec;
      pucch_demodulator::format4_configuration    dc;
      ec.slot               = slot_point(h.numerology, h.slot_index);
      ec.cp                 = cp;
      ec.group_hopping      = pucch_group_hopping::NEITHER;
      ec.start_symbol_index = h.start_symbol;
      ec.nof_symbols        = h.nof_symbols;
      ec.starting_prb       = h.starting_prb;
      ec.second_hop_prb     = second_hop;
      ec.n_id               = h.n_id_hopping;
      ec.additional_dmrs    = h.additional_dmrs != 0;
      ec.occ_index          = h.occ_index;
      for (unsigned p = 0; p < h.nof_ports; ++p) {
        ec.ports.push_back(static_cast<uint8_t>(h.ports[p]));
        dc.rx_ports.push_back(static_cast<uint8_t>(h.ports[p]));
      }
      estimator->estimate(estimates, c.grid->get_reader(), ec);
      dc.first_prb          = h.starting_prb;
      dc.second_hop_prb     = second_hop;
      dc.start_symbol_index = h.start_symbol;
      dc.nof_symbols        = h.nof_symbols;
      dc.rnti               = h.rnti;
      dc.n_id               = h.n_id_scrambling;
      dc.additional_dmrs    = h.additional_dmrs != 0;
      dc.pi2_bpsk           = h.pi2_bpsk != 0;
      dc.occ_index          = h.occ_index;
      dc.occ_length         = h.occ_length;
      demodulator4->demodulate(llr, c.grid->get_reader(), estimates, dc);
    }
    return decoder->decode(bits, llr, {h.pi2_bpsk ? modulation_scheme::PI_2_BPSK : modulation_scheme::QPSK});
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
        const bool     hop1 = c.h.second_hop_prb != 0xffffU && s >= c.h.nof_symbols / 2;
        const unsigned prb  = hop1 ? c.h.second_hop_prb : c.h.starting_prb;
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
    // The ports combined as the processor reports them (pucch_processor_impl.cpp:271); NaN for a value it leaves unset.
    channel_state_information csi;
    rx.estimates.get_channel_state_information(csi);
    const float  db[3]   = {csi.get_epre_dB().value_or(NAN), csi.get_rsrp_dB().value_or(NAN), csi.get_sinr_dB().value_or(NAN)};
    const double csi_ta  = csi.get_time_alignment().has_value() ? csi.get_time_alignment()->to_seconds() : NAN;
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
    const uint32_t a = take<uint32_t>(raw, pos), e = take<uint32_t>(raw, pos), pi2 = take<uint32_t>(raw, pos);
    std::vector<log_likelihood_ratio> llr;
    for (uint32_t j = 0; j < e; ++j) {
      llr.push_back(log_likelihood_ratio(take<int8_t>(raw, pos)));
    }
    std::vector<uint8_t> bits(a, 2);
    const uci_status     st = decoder->decode(bits, llr, {pi2 ? modulation_scheme::PI_2_BPSK : modulation_scheme::QPSK});
    const uint8_t        valid = st == uci_status::valid ? 1 : 0;
    put(f, bits.data(), bits.size());
    put(f, &valid, 1);
  }
  return 0;
}

int tables(const char* out)
{
  std::ofstream f(out, std::ios::binary);
  for (unsigned n = 4; n <= 14; ++n) {
    for (unsigned hop = 0; hop < 2; ++hop) {
      for (unsigned add = 0; add < 2; ++add) {
        const symbol_slot_mask m    = get_pucch_formats3_4_dmrs_symbol_mask(n, hop != 0, add != 0);
        uint16_t               bits = 0;
        m.for_each(0, n, [&bits](unsigned i) { bits |= static_cast<uint16_t>(1U << i); });
        put(f, &bits, 1);
      }
    }
  }
  for (unsigned len : {2U, 4U}) {
    for (unsigned i = 0; i < len; ++i) {
      for (cf_t w : pucch_orthogonal_sequence_format4::get_sequence(len, i)) {
        const float v[2] = {w.real(), w.imag()};
        put(f, v, 2);
      }
    }
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
  if (argc >= 3 && std::string(argv[1]) == "tables") {
    return tables(argv[2]);
  }
  std::fprintf(stderr, "usage: %s process IN OUT [REPEATS] | decode IN OUT | tables OUT\n", argv[0]);
  return 2;
}
