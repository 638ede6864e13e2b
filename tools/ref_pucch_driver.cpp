// Driver of tools/gen_pucch_golden.py: runs the reference's pucch_detector_format0 and pucch_detector_format1 (with its
// low-PAPR sequence collection, pseudo-random generator and a resource grid, all compiled from the reference tree where
// it lies, never committed; the 12-point transforms are this file's own direct sums in float behind the reference's
// dft_processor interface, since the reference's generic DFT has no size 12 and its other one needs FFTW) over cases the tool writes, for the fixture
// tests/golden/pucch_detector.npz. The detectors are what pucch_processor_impl::process calls for Formats 0 and 1 after
// its validator; the tool only writes cases the validator accepts.
//
//   ref_pucch_driver IN OUT [REPEATS]   IN: u32 nof_f0, u32 nof_f1; per Format 0 case the `f0_header` below and
//                                       nof_symbols x nof_ports x 12 u32 (re | im << 16, bf16: the REs of (symbol,
//                                       listed port)); per Format 1 case the `f1_header`, nof_entries x 3 u32 (cyclic
//                                       shift, OCC, nof_harq_ack) and nof_symbols x nof_ports x 12 u32.
//                                       OUT per Format 0 case: `f0_result`; per Format 1 case one float (the noise
//                                       variance detect() divides by, recomputed here from process_hop as detect() does)
//                                       and one `f1_result` per entry in the case's order.
//                                       REPEATS > 0: also times REPEATS passes over every case on this core,
//                                       "ns_per_pass <value>".
//   ref_pucch_driver ncs IN OUT         IN: u32 n, n x 4 u32 (n_id, symbols per slot, n_slot, symbol). OUT: n x u32, the
//                                       alpha index of pucch_helper::get_alpha_index with m0 = m_cs = 0 (n_cs mod 12) —
//                                       and n x u32 of n_cs itself, recovered as the same byte the helper reads.
#include "srsran/phy/support/resource_grid_reader.h"
#include "srsran/phy/support/resource_grid_writer.h"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>
// process_hop and the hop contributions are private; this test-only driver reads them as they are.
#define private public
#include "lib/phy/upper/channel_processors/pucch/pucch_detector_format1.h"
#undef private
#include "srsran/phy/generic_functions/dft_processor.h"
#include "lib/phy/support/resource_grid_impl.h"
#include "lib/phy/upper/channel_processors/pucch/pucch_detector_format0.h"
#include "lib/phy/upper/sequence_generators/low_papr_sequence_collection_impl.h"
#include "lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.h"
#include "lib/phy/upper/sequence_generators/pseudo_random_generator_impl.h"
#include "srsran/adt/bit_buffer.h"
#include "srsran/support/math/math_utils.h"

using namespace srsran;

namespace {

constexpr uint32_t NO_HOP = 0xffff;

struct f0_header {
  uint32_t slot_index, numerology, cp_extended, starting_prb, second_hop_prb, start_symbol, nof_symbols;
  uint32_t initial_cyclic_shift, n_id, nof_harq_ack, sr_opportunity, nof_ports, ports[4], grid_nof_ports;
};
struct f1_header {
  uint32_t slot_index, numerology, cp_extended, starting_prb, second_hop_prb, start_symbol, nof_symbols;
  uint32_t n_id, nof_ports, nof_entries;
};
struct f0_result {
  uint32_t status, nof_sr, sr, nof_harq_ack, harq_ack[2];
  float    sinr_dB, epre_dB, rsrp_dB;
};
struct f1_result {
  uint32_t status, harq_ack[2];
  float    detection_metric, epre_dB, rsrp_dB, sinr_dB;
};

struct f0_case {
  f0_header             h;
  std::vector<uint32_t> res;
};
struct f1_case {
  f1_header             h;
  std::vector<uint32_t> entries;
  std::vector<uint32_t> res;
};

/// Direct 12-point DFT (unnormalised, exp(-+j 2 pi n k / 12)), twiddles from double.
class dft12 : public dft_processor
{
public:
  explicit dft12(direction dir_) : dir(dir_)
  {
    const double sign = dir == direction::DIRECT ? -1.0 : 1.0;
    for (unsigned q = 0; q != NRE; ++q) {
      twiddle[q] = cf_t(static_cast<float>(std::cos(2.0 * M_PI * q / NRE)), static_cast<float>(sign * std::sin(2.0 * M_PI * q / NRE)));
    }
  }
  direction        get_direction() const override { return dir; }
  unsigned         get_size() const override { return NRE; }
  span<cf_t>       get_input() override { return input; }
  span<const cf_t> run() override
  {
    for (unsigned k = 0; k != NRE; ++k) {
      cf_t acc = 0;
      for (unsigned n = 0; n != NRE; ++n) {
        acc += input[n] * twiddle[(n * k) % NRE];
      }
      output[k] = acc;
    }
    return output;
  }

private:
  direction             dir;
  std::array<cf_t, NRE> twiddle, input, output;
};

template <typename T>
void put(std::ofstream& out, const T* data, size_t count)
{
  out.write(reinterpret_cast<const char*>(data), count * sizeof(T));
}

std::unique_ptr<low_papr_sequence_collection> make_low_papr()
{
  std::array<float, NRE> alphas;
  for (unsigned n = 0; n != NRE; ++n) {
    alphas[n] = TWOPI * static_cast<float>(n) / static_cast<float>(NRE);
  }
  low_papr_sequence_generator_impl generator;
  return std::make_unique<low_papr_sequence_collection_impl>(generator, 1, 0, alphas);
}

void fill_grid(resource_grid_impl& grid, unsigned port, unsigned symbol, unsigned prb, const uint32_t* words)
{
  span<cbf16_t> view = grid.get_writer().get_view(port, symbol);
  for (unsigned k = 0; k != NRE; ++k) {
    cbf16_t v;
    v.real                = bf16_t(static_cast<uint16_t>(words[k] & 0xffffU));
    v.imag                = bf16_t(static_cast<uint16_t>(words[k] >> 16));
    view[NRE * prb + k] = v;
  }
}

cyclic_prefix cp_of(uint32_t extended)
{
  return extended != 0 ? cyclic_prefix::EXTENDED : cyclic_prefix::NORMAL;
}

std::unique_ptr<resource_grid_impl> make_grid_f0(const f0_case& c)
{
  const f0_header& h        = c.h;
  const unsigned   nof_prb  = std::max(h.starting_prb, h.second_hop_prb == NO_HOP ? 0U : h.second_hop_prb) + 1;
  auto             grid     = std::make_unique<resource_grid_impl>(h.grid_nof_ports, 14, NRE * nof_prb);
  grid->set_all_zero();
  for (unsigned s = 0; s != h.nof_symbols; ++s) {
    const unsigned prb = (s != 0 && h.second_hop_prb != NO_HOP) ? h.second_hop_prb : h.starting_prb;
    for (unsigned p = 0; p != h.nof_ports; ++p) {
      fill_grid(*grid, h.ports[p], h.start_symbol + s, prb, c.res.data() + NRE * (s * h.nof_ports + p));
    }
  }
  return grid;
}

pucch_detector::format0_configuration make_config_f0(const f0_header& h)
{
  pucch_detector::format0_configuration cfg;
  cfg.slot           = slot_point(h.numerology, h.slot_index);
  cfg.cp             = cp_of(h.cp_extended);
  cfg.starting_prb   = h.starting_prb;
  if (h.second_hop_prb != NO_HOP) {
    cfg.second_hop_prb.emplace(h.second_hop_prb);
  }
  cfg.start_symbol_index   = h.start_symbol;
  cfg.nof_symbols          = h.nof_symbols;
  cfg.initial_cyclic_shift = h.initial_cyclic_shift;
  cfg.n_id                 = h.n_id;
  cfg.nof_harq_ack         = h.nof_harq_ack;
  cfg.sr_opportunity       = h.sr_opportunity != 0;
  for (unsigned p = 0; p != h.nof_ports; ++p) {
    cfg.ports.push_back(static_cast<uint8_t>(h.ports[p]));
  }
  return cfg;
}

std::unique_ptr<resource_grid_impl> make_grid_f1(const f1_case& c)
{
  const f1_header& h       = c.h;
  const unsigned   nof_prb = std::max(h.starting_prb, h.second_hop_prb == NO_HOP ? 0U : h.second_hop_prb) + 1;
  auto             grid    = std::make_unique<resource_grid_impl>(h.nof_ports, 14, NRE * nof_prb);
  grid->set_all_zero();
  for (unsigned s = 0; s != h.nof_symbols; ++s) {
    const unsigned prb = (h.second_hop_prb != NO_HOP && s >= h.nof_symbols / 2) ? h.second_hop_prb : h.starting_prb;
    for (unsigned p = 0; p != h.nof_ports; ++p) {
      fill_grid(*grid, p, h.start_symbol + s, prb, c.res.data() + NRE * (s * h.nof_ports + p));
    }
  }
  return grid;
}

pucch_detector::format1_configuration make_config_f1(const f1_header& h)
{
  pucch_detector::format1_configuration cfg;
  cfg.slot         = slot_point(h.numerology, h.slot_index);
  cfg.cp           = cp_of(h.cp_extended);
  cfg.starting_prb = h.starting_prb;
  if (h.second_hop_prb != NO_HOP) {
    cfg.second_hop_prb.emplace(h.second_hop_prb);
  }
  cfg.start_symbol_index = h.start_symbol;
  cfg.nof_symbols        = h.nof_symbols;
  cfg.group_hopping      = pucch_group_hopping::NEITHER;
  // The detector reads grid ports 0..get_nof_ports()-1 whatever this list says.
  for (unsigned p = 0; p != h.nof_ports; ++p) {
    cfg.ports.push_back(static_cast<uint8_t>(p));
  }
  cfg.beta_pucch           = 1.0F;
  cfg.time_domain_occ      = 0;
  cfg.initial_cyclic_shift = 0;
  cfg.n_id                 = h.n_id;
  cfg.nof_harq_ack         = 0;
  return cfg;
}

pucch_format1_map<unsigned> make_mux(const f1_case& c)
{
  pucch_format1_map<unsigned> mux;
  for (unsigned e = 0; e != c.h.nof_entries; ++e) {
    mux.insert(c.entries[3 * e], c.entries[3 * e + 1], c.entries[3 * e + 2]);
  }
  return mux;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc < 3) {
    std::fprintf(stderr, "usage: ref_pucch_driver IN OUT [REPEATS] | ncs IN OUT\n");
    return 2;
  }
  const bool           ncs_mode = std::string(argv[1]) == "ncs";
  const char*          in_path  = ncs_mode ? argv[2] : argv[1];
  const char*          out_path = ncs_mode ? argv[3] : argv[2];
  std::ifstream        in(in_path, std::ios::binary);
  std::vector<uint8_t> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  size_t               pos  = 0;
  auto                 take = [&](void* dst, size_t n) {
    if (pos + n > raw.size()) {
      std::fprintf(stderr, "ref_pucch_driver: truncated input\n");
      std::exit(2);
    }
    std::memcpy(dst, raw.data() + pos, n);
    pos += n;
  };
  std::ofstream out(out_path, std::ios::binary);

  if (ncs_mode) {
    uint32_t n = 0;
    take(&n, 4);
    pucch_helper          helper(std::make_unique<pseudo_random_generator_impl>());
    std::vector<uint32_t> alpha(n), ncs(n);
    for (uint32_t i = 0; i != n; ++i) {
      uint32_t q[4];
      take(q, sizeof(q));
      // Numerology 4 gives a frame of 160 slots: every n_slot below that is a valid slot_point of it. The helper's n_cs
      // depends on the slot through nsymb * n_slot + symbol only.
      const cyclic_prefix cp = q[1] == 12 ? cyclic_prefix::EXTENDED : cyclic_prefix::NORMAL;
      alpha[i]               = helper.get_alpha_index(slot_point(4, q[2]), cp, q[0], q[3], 0, 0);
      pseudo_random_generator_impl prg;
      static_bit_buffer<8 * 14 * 160> cs(8 * q[1] * 160);
      prg.init(q[0]);
      prg.generate(cs);
      ncs[i] = reverse_byte(cs.get_byte(q[1] * q[2] + q[3]));
    }
    put(out, alpha.data(), n);
    put(out, ncs.data(), n);
    return 0;
  }

  uint32_t nof_f0 = 0, nof_f1 = 0;
  take(&nof_f0, 4);
  take(&nof_f1, 4);
  std::vector<f0_case> f0(nof_f0);
  std::vector<f1_case> f1(nof_f1);
  for (f0_case& c : f0) {
    take(&c.h, sizeof(f0_header));
    c.res.resize(static_cast<size_t>(NRE) * c.h.nof_symbols * c.h.nof_ports);
    take(c.res.data(), 4 * c.res.size());
  }
  for (f1_case& c : f1) {
    take(&c.h, sizeof(f1_header));
    c.entries.resize(3 * static_cast<size_t>(c.h.nof_entries));
    take(c.entries.data(), 4 * c.entries.size());
    c.res.resize(static_cast<size_t>(NRE) * c.h.nof_symbols * c.h.nof_ports);
    take(c.res.data(), 4 * c.res.size());
  }

  pucch_detector_format0 det0(std::make_unique<pseudo_random_generator_impl>(), make_low_papr());
  pucch_detector_format1 det1(
      make_low_papr(), std::make_unique<pseudo_random_generator_impl>(),
      std::make_unique<dft12>(dft_processor::direction::DIRECT), std::make_unique<dft12>(dft_processor::direction::INVERSE));

  std::vector<std::unique_ptr<resource_grid_impl>>   grids0, grids1;
  std::vector<pucch_detector::format0_configuration> cfgs0;
  std::vector<pucch_detector::format1_configuration> cfgs1;
  std::vector<pucch_format1_map<unsigned>>           muxes;
  for (const f0_case& c : f0) {
    grids0.push_back(make_grid_f0(c));
    cfgs0.push_back(make_config_f0(c.h));
  }
  for (const f1_case& c : f1) {
    grids1.push_back(make_grid_f1(c));
    cfgs1.push_back(make_config_f1(c.h));
    muxes.push_back(make_mux(c));
  }

  for (uint32_t i = 0; i != nof_f0; ++i) {
    auto      res = det0.detect(grids0[i]->get_reader(), cfgs0[i]);
    f0_result r   = {};
    r.status       = res.first.get_status() == uci_status::valid ? 1 : 0;
    r.nof_sr       = res.first.get_sr_bits().size();
    r.sr           = r.nof_sr != 0 ? res.first.get_sr_bits()[0] : 0;
    r.nof_harq_ack = res.first.get_harq_ack_bits().size();
    for (unsigned b = 0; b != r.nof_harq_ack; ++b) {
      r.harq_ack[b] = res.first.get_harq_ack_bits()[b];
    }
    r.sinr_dB = res.second.get_sinr_dB().value_or(std::numeric_limits<float>::quiet_NaN());
    r.epre_dB = res.second.get_epre_dB().value_or(std::numeric_limits<float>::quiet_NaN());
    r.rsrp_dB = res.second.get_rsrp_dB().value_or(std::numeric_limits<float>::quiet_NaN());
    put(out, &r, 1);
  }
  for (uint32_t i = 0; i != nof_f1; ++i) {
    const f1_case& c = f1[i];
    // The noise variance as detect() forms it (pucch_detector_format1.cpp:174-190), from the same process_hop calls.
    {
      det1.dmrs_mask.reset();
      for (unsigned s = c.h.start_symbol, end = c.h.start_symbol + c.h.nof_symbols; s < end; s += 2) {
        det1.dmrs_mask.set(s);
      }
      static_vector<pucch_detector_format1::hop_contribution_mux, 84> m0(0), m1(0);
      auto     hop0    = det1.process_hop(m0, grids1[i]->get_reader(), cfgs1[i], muxes[i], 0);
      float    noise   = hop0.noise_var_contribution;
      unsigned samples = hop0.nof_noise_samples;
      if (cfgs1[i].second_hop_prb.has_value()) {
        auto hop1 = det1.process_hop(m1, grids1[i]->get_reader(), cfgs1[i], muxes[i], 1);
        noise += hop1.noise_var_contribution;
        samples += hop1.nof_noise_samples;
      }
      noise /= samples;
      put(out, &noise, 1);
    }
    const auto& results = det1.detect(grids1[i]->get_reader(), cfgs1[i], muxes[i]);
    for (unsigned e = 0; e != c.h.nof_entries; ++e) {
      const auto& res = results.get(c.entries[3 * e], c.entries[3 * e + 1]);
      f1_result   r   = {};
      r.status         = res.detection_result.uci_message.get_status() == uci_status::valid ? 1 : 0;
      for (unsigned b = 0; b != c.entries[3 * e + 2]; ++b) {
        r.harq_ack[b] = res.detection_result.uci_message.get_harq_ack_bits()[b];
      }
      r.detection_metric = res.detection_result.detection_metric;
      r.epre_dB          = res.csi.get_epre_dB().value_or(std::numeric_limits<float>::quiet_NaN());
      r.rsrp_dB          = res.csi.get_rsrp_dB().value_or(std::numeric_limits<float>::quiet_NaN());
      r.sinr_dB          = res.csi.get_sinr_dB().value_or(std::numeric_limits<float>::quiet_NaN());
      put(out, &r, 1);
    }
  }

  const int repeats = argc > 3 ? std::atoi(argv[3]) : 0;
  if (repeats > 0) {
    auto     t0   = std::chrono::steady_clock::now();
    unsigned sink = 0;
    for (int r = 0; r < repeats; ++r) {
      for (uint32_t i = 0; i != nof_f0; ++i) {
        sink += det0.detect(grids0[i]->get_reader(), cfgs0[i]).first.get_status() == uci_status::valid;
      }
      for (uint32_t i = 0; i != nof_f1; ++i) {
        sink += det1.detect(grids1[i]->get_reader(), cfgs1[i], muxes[i]).size();
      }
    }
    auto t1 = std::chrono::steady_clock::now();
    std::printf("ns_per_pass %.1f (sink %u)\n", std::chrono::duration<double, std::nano>(t1 - t0).count() / repeats, sink);
  }
  return 0;
}
