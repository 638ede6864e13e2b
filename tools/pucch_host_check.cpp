// Stand-alone check of srsran-5g_amd/csrc/pucch_host.cpp (tests/test_pucch_oracle.py builds it with the address and
// undefined-behaviour sanitizers): n_cs against the reference's values recorded in the fixture, the Format 1 hop split
// for every length with and without hopping against the reference's closed forms, the threshold picks, the job
// descriptors' bounds and every refusal.
//
//   pucch_host_check DUMP    DUMP: u32 n, then n x 5 u32 (n_id, symbols per slot, n_slot, symbol, n_cs).
#include "host_util.h"
#include "pucch_host.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <vector>

using namespace srsgpu;

namespace {

int failures = 0;

#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                                                    \
      std::printf(__VA_ARGS__);                                                                                        \
      std::printf("\n");                                                                                               \
      ++failures;                                                                                                      \
    }                                                                                                                  \
  } while (0)

srsgpu_pucch_f0_config good_f0()
{
  srsgpu_pucch_f0_config c = {};
  c.slot_index = 3, c.numerology = 1, c.starting_prb = 5, c.second_hop_prb = PUCCH_NO_HOP, c.start_symbol_index = 12;
  c.nof_symbols = 2, c.initial_cyclic_shift = 4, c.nof_harq_ack = 1, c.n_id = 77, c.sr_opportunity = 1, c.nof_ports = 2;
  c.ports[0] = 3, c.ports[1] = 0;
  return c;
}

srsgpu_pucch_f1_resource good_f1()
{
  srsgpu_pucch_f1_resource r = {};
  r.slot_index = 7, r.numerology = 1, r.starting_prb = 2, r.second_hop_prb = 9, r.start_symbol_index = 0, r.nof_symbols = 14;
  r.n_id = 500, r.nof_rx_ports = 2, r.first_entry = 0, r.nof_entries = 3;
  return r;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc < 2) {
    return 2;
  }
  std::ifstream        in(argv[1], std::ios::binary);
  std::vector<uint8_t> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  const uint32_t*      words = reinterpret_cast<const uint32_t*>(raw.data());
  CHECK(raw.size() >= 4 && raw.size() == 4 + 20ull * words[0], "dump of %zu bytes", raw.size());
  const uint32_t n = failures == 0 ? words[0] : 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t* q = words + 1 + 5 * i;
    CHECK(pucch_n_cs(q[0], q[1], q[2], q[3]) == q[4], "n_cs(%u, %u, %u, %u)", q[0], q[1], q[2], q[3]);
  }

  // Hop split (pucch_detector_format1.cpp:519-541).
  for (uint32_t nsym = 4; nsym <= 14; ++nsym) {
    const pucch_f1_split a = pucch_f1_hop_split(nsym, false);
    CHECK(a.nof_hops == 1 && a.first[0] == 0 && a.nof_symbols[0] == nsym && a.nof_data[0] == nsym / 2 &&
              a.nof_dmrs[0] == (nsym + 1) / 2, "no hopping, %u symbols", nsym);
    const pucch_f1_split b = pucch_f1_hop_split(nsym, true);
    CHECK(b.nof_hops == 2 && b.first[0] == 0 && b.nof_symbols[0] == nsym / 2 && b.nof_data[0] == nsym / 4 &&
              b.nof_dmrs[0] == nsym / 2 - nsym / 4, "hopping, %u symbols, first hop", nsym);
    CHECK(b.first[1] == nsym / 2 && b.nof_symbols[1] == (nsym + 1) / 2 && b.nof_data[1] == (nsym - 1 + 3) / 4 &&
              b.nof_dmrs[1] == (nsym + 1) / 2 - (nsym - 1 + 3) / 4, "hopping, %u symbols, second hop", nsym);
    // A second hop that starts on an odd allocated symbol starts with a data symbol.
    CHECK((((b.dmrs_mask >> b.first[1]) & 1u) != 0) == ((nsym / 2) % 2 == 0), "second hop's first symbol, %u symbols", nsym);
  }

  // Thresholds: lower_bound over (ports x symbols, sequences).
  CHECK(pucch_f0_threshold(1, 1, 1) == 0.5373F && pucch_f0_threshold(1, 2, 2) == 0.4038F, "exact entries");
  CHECK(pucch_f0_threshold(3, 1, 1) == 0.3455F && pucch_f0_threshold(3, 1, 8) == 0.3455F, "3 ports x 1 symbol takes (4, 1)");
  CHECK(pucch_f0_threshold(3, 2, 4) == 0.2545F && pucch_f0_threshold(4, 2, 8) == 0.3273F, "6 and 8 degrees");
  CHECK(pucch_f1_threshold(1) == 0.9F && pucch_f1_threshold(2) == 3.0F && pucch_f1_threshold(4) == 4.45F &&
            pucch_f1_threshold(8) == 6.95F && pucch_f1_threshold(3) == 0.0F && pucch_f1_threshold(6) == 0.0F, "Format 1");
  uint8_t m_cs[8], msg[8];
  CHECK(pucch_f0_candidates(0, 1, m_cs, msg) == 1 && pucch_f0_candidates(1, 0, m_cs, msg) == 2 &&
            pucch_f0_candidates(2, 0, m_cs, msg) == 4 && pucch_f0_candidates(1, 1, m_cs, msg) == 4 &&
            pucch_f0_candidates(2, 1, m_cs, msg) == 8, "candidate counts");
  CHECK(m_cs[5] == 4 && msg[5] == (1 | (0 << 1) | (1 << 2)), "positive SR, ACK bits (0, 1): m_cs 4");

  // The orthogonal sequences: unit modulus, rows of one length orthogonal.
  const std::vector<float> w = pucch_w_table();
  CHECK(w.size() == PUCCH_W_TABLE_FLOATS, "table size");
  for (uint32_t N = 1; N <= 7; ++N) {
    for (uint32_t i = 0; i < N; ++i) {
      for (uint32_t k = 0; k < N; ++k) {
        double re = 0, im = 0;
        for (uint32_t m = 0; m < N; ++m) {
          const float* a = &w[2 * ((N - 1) * 49 + i * 7 + m)];
          const float* b = &w[2 * ((N - 1) * 49 + k * 7 + m)];
          re += a[0] * b[0] + a[1] * b[1];
          im += a[1] * b[0] - a[0] * b[1];
        }
        CHECK(std::fabs(re - (i == k ? N : 0)) < 1e-5 && std::fabs(im) < 1e-5, "w of length %u, rows %u and %u", N, i, k);
      }
    }
  }

  // Accepted configurations and their jobs.
  const srsgpu_pucch_f1_entry entries[4] = {{0, 0, 1, 0}, {5, 0, 0, 0}, {5, 2, 2, 0}, {5, 2, 1, 0}};
  CHECK(pucch_f0_refusal(good_f0(), 20, 4, 2).empty(), "%s", pucch_f0_refusal(good_f0(), 20, 4, 2).c_str());
  CHECK(pucch_f1_refusal(good_f1(), entries, 3, 20, 2, 1).empty(), "%s", pucch_f1_refusal(good_f1(), entries, 3, 20, 2, 1).c_str());
  const pucch_job j0 = pucch_f0_job(good_f0(), 20, 4, 11);
  CHECK(j0.kind == 0 && j0.result_offset == 11 && j0.nof_candidates == 4 && j0.nof_symbols == 2 && j0.nof_ports == 2 &&
            j0.threshold == pucch_f0_threshold(2, 2, 4), "Format 0 job");
  CHECK(j0.sym_base[0] == 12u * 240 + 60 && j0.sym_base[1] == 13u * 240 + 60 && j0.port_stride == 14u * 240, "Format 0 bases");
  const pucch_job j1 = pucch_f1_job(good_f1(), entries, 20, 2, 5);
  CHECK(j1.kind == 1 && j1.nof_hops == 2 && j1.occ_mask == 0b101 && j1.nof_entries == 3 && j1.threshold == 4.45F &&
            j1.hop_nof_data[0] == 3 && j1.hop_nof_dmrs[0] == 4 && j1.hop_nof_data[1] == 4 && j1.hop_nof_dmrs[1] == 3,
        "Format 1 job");
  CHECK(j1.sym_base[6] == 6u * 240 + 24 && j1.sym_base[7] == 7u * 240 + 108, "Format 1 hop border");
  for (uint32_t s = 0; s < 14; ++s) {
    CHECK(j1.alpha[s] == pucch_n_cs(500, 14, 7, s) % 12, "alpha of symbol %u", s);
  }

  // Refusals.
  uint32_t refused = 0;
  auto     f0_refused = [&](void (*change)(srsgpu_pucch_f0_config&), uint32_t prb = 20, uint32_t ports = 4, uint32_t grids = 2) {
    srsgpu_pucch_f0_config c = good_f0();
    change(c);
    ++refused;
    return !pucch_f0_refusal(c, prb, ports, grids).empty();
  };
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.nof_symbols = 0; }), "no symbols");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.nof_symbols = 3; }), "three symbols");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.start_symbol_index = 13; }), "past the slot");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.cp_extended = 1; }), "extended CP at numerology 1");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.numerology = 2, c.cp_extended = 1; }), "symbol 13 of 12");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.numerology = 5; }), "numerology");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.slot_index = 20; }), "slot");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.initial_cyclic_shift = 12; }), "cyclic shift");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.n_id = 1024; }), "n_id");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.nof_harq_ack = 0, c.sr_opportunity = 0; }), "no payload");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.nof_harq_ack = 3; }), "three bits");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.nof_ports = 0; }), "no ports");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.nof_ports = 5; }), "five ports");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.ports[1] = 4; }), "port outside the grid");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.starting_prb = 20; }), "PRB outside the grid");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.second_hop_prb = 20; }), "second hop outside the grid");
  CHECK(f0_refused([](srsgpu_pucch_f0_config& c) { c.grid_index = 2; }), "grid index");

  auto f1_refused = [&](void (*change)(srsgpu_pucch_f1_resource&), const srsgpu_pucch_f1_entry* e, uint32_t total = 3) {
    srsgpu_pucch_f1_resource r = good_f1();
    change(r);
    ++refused;
    return !pucch_f1_refusal(r, e, total, 20, 2, 1).empty();
  };
  auto same = [](srsgpu_pucch_f1_resource&) {};
  CHECK(f1_refused([](srsgpu_pucch_f1_resource& r) { r.nof_entries = 0; }, entries), "no entries");
  CHECK(f1_refused([](srsgpu_pucch_f1_resource& r) { r.nof_entries = 4; }, entries), "entries past the list");
  CHECK(f1_refused([](srsgpu_pucch_f1_resource& r) { r.nof_symbols = 3; }, entries), "three symbols");
  CHECK(f1_refused([](srsgpu_pucch_f1_resource& r) { r.nof_symbols = 13, r.start_symbol_index = 2; }, entries), "past the slot");
  CHECK(f1_refused([](srsgpu_pucch_f1_resource& r) { r.start_symbol_index = 11, r.nof_symbols = 3; }, entries), "start 11");
  CHECK(f1_refused([](srsgpu_pucch_f1_resource& r) { r.nof_rx_ports = 3; }, entries), "3 ports x 2 hops");
  CHECK(f1_refused([](srsgpu_pucch_f1_resource& r) { r.nof_rx_ports = 3, r.second_hop_prb = PUCCH_NO_HOP; }, entries), "3 ports");
  CHECK(f1_refused([](srsgpu_pucch_f1_resource& r) { r.nof_rx_ports = 0; }, entries), "no ports");
  CHECK(f1_refused([](srsgpu_pucch_f1_resource& r) { r.nof_rx_ports = 4; }, entries), "more ports than the grid");
  CHECK(f1_refused([](srsgpu_pucch_f1_resource& r) { r.starting_prb = 20; }, entries), "PRB outside the grid");
  CHECK(f1_refused([](srsgpu_pucch_f1_resource& r) { r.second_hop_prb = 300; }, entries), "second hop outside the grid");
  CHECK(f1_refused([](srsgpu_pucch_f1_resource& r) { r.grid_index = 1; }, entries), "grid index");
  CHECK(f1_refused([](srsgpu_pucch_f1_resource& r) { r.n_id = 2000; }, entries), "n_id");
  // OCC 2 needs three data symbols in the shorter hop: 14 symbols with hopping have them, 10 symbols do not (2 and 3).
  CHECK(f1_refused([](srsgpu_pucch_f1_resource& r) { r.nof_symbols = 10; }, entries), "OCC 2 with 10 symbols and hopping");
  CHECK(!f1_refused([](srsgpu_pucch_f1_resource& r) { r.nof_symbols = 12; }, entries), "OCC 2 with 12 symbols and hopping");
  --refused;
  const srsgpu_pucch_f1_entry twice[3] = {{0, 0, 1, 0}, {5, 1, 0, 0}, {5, 1, 2, 0}};
  CHECK(f1_refused(same, twice), "the same (shift, OCC) twice");
  const srsgpu_pucch_f1_entry shift[3] = {{12, 0, 1, 0}, {5, 0, 0, 0}, {5, 2, 2, 0}};
  CHECK(f1_refused(same, shift), "cyclic shift 12");
  const srsgpu_pucch_f1_entry bits[3] = {{1, 0, 3, 0}, {5, 0, 0, 0}, {5, 2, 2, 0}};
  CHECK(f1_refused(same, bits), "three bits");
  const srsgpu_pucch_f1_entry occ[3] = {{1, 0, 1, 0}, {5, 0, 0, 0}, {5, 3, 2, 0}};
  CHECK(f1_refused(same, occ), "OCC 3 with 14 symbols and hopping");

  std::printf("%u n_cs values, %u refusals, %d failures\n", n, refused, failures);
  return failures == 0 ? 0 : 1;
}
