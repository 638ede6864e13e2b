// Stand-alone check of srsran-5g_amd/csrc/srs_host.cpp (no HIP, no GPU), built by tests/test_srs_oracle.py with the
// address and undefined-behaviour sanitizers and run as a child process.
//
//   srs_host_check DUMP    DUMP (written by the test from the float64 restatement tests/srs_cases.py):
//                          u32 n; n x (the srsgpu_srs_config bytes, u32 grid_nof_prb, then 15 u32: L, n_cs_max, u,
//                          interleaved, n_cs[4], k0[4], M, log2 M, max_ta_samples, and f64 fs);
//                          u32 m; m x (u32 u, u32 L, u32 n_cs, u32 n_cs_max, 2 L f64: the sequence as (re, im)).
// Checks srs_refusal's derived quantities and srs_sequence against the dump, the phase table, the job descriptors and
// every refusal.
#include "host_util.h"
#include "srs_host.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

using namespace srsgpu;

namespace {

int failures = 0;

#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      ++failures;                                                                                                      \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond);                                                       \
      std::printf(__VA_ARGS__);                                                                                        \
      std::printf("\n");                                                                                               \
    }                                                                                                                  \
  } while (0)

template <typename T>
T take(const std::vector<char>& raw, size_t& pos)
{
  T v;
  if (pos + sizeof(T) > raw.size()) {
    std::printf("dump too short\n");
    std::exit(2);
  }
  std::memcpy(&v, raw.data() + pos, sizeof(T));
  pos += sizeof(T);
  return v;
}

/// C_SRS 13 of TS 38.211 Table 6.4.1.4.3-1 (48 | 24 | 12 | 4 PRBs), B_SRS 1, comb 4, 4 ports interleaved, rx ports 2 and 0.
srsgpu_srs_config good_resource()
{
  srsgpu_srs_config c = {};
  c.m_srs[0] = 48, c.m_srs[1] = 24, c.m_srs[2] = 12, c.m_srs[3] = 4;
  c.N[0] = 1, c.N[1] = 2, c.N[2] = 2, c.N[3] = 3;
  c.numerology = 1, c.nof_antenna_ports = 4, c.nof_symbols = 2, c.start_symbol = 12, c.comb_size = 4, c.comb_offset = 3;
  c.cyclic_shift = 7, c.bandwidth_index = 1, c.freq_hopping = 3, c.hopping = 0, c.nof_rx_ports = 2;
  c.rx_ports[0] = 2, c.rx_ports[1] = 0;
  c.sequence_id = 77, c.freq_shift = 3, c.freq_position = 7, c.grid_index = 1, c.result_index = 1;
  return c;
}

void check_refusals()
{
  srs_derived       d;
  const std::string ok = srs_refusal(good_resource(), 52, 4, 2, 2, d);
  CHECK(ok.empty(), "%s", ok.c_str());
  // n_b = (4 x 7 / 48) mod 1 = 0, then (28 / 24) mod 2 = 1: k0 = 36 + k_TC + 4 x 72 x 1.
  CHECK(d.L == 72 && d.interleaved == 1 && d.k0[0] == 36 + 3 + 288 && d.k0[1] == 36 + 1 + 288 && d.k0[2] == d.k0[0] &&
            d.k0[3] == d.k0[1] && d.n_cs[0] == 7 && d.n_cs[1] == 10 && d.n_cs[2] == 1 && d.n_cs[3] == 4 && d.u == 17 &&
            d.M == 128 && d.log2M == 7,
        "derived: L %u k0 %u %u n_cs %u %u %u %u M %u", d.L, d.k0[0], d.k0[1], d.n_cs[0], d.n_cs[1], d.n_cs[2], d.n_cs[3], d.M);
  auto refused = [&](const char* what, const srsgpu_srs_config& c, uint32_t prb = 52, uint32_t ports = 4, uint32_t grids = 2,
                     uint32_t nof = 2) { CHECK(!srs_refusal(c, prb, ports, grids, nof, d).empty(), "%s is accepted", what); };
  srsgpu_srs_config c;
  c = good_resource(), c.numerology = 5, refused("numerology 5", c);
  c = good_resource(), c.nof_antenna_ports = 3, refused("three antenna ports", c);
  c = good_resource(), c.nof_antenna_ports = 0, refused("no antenna port", c);
  c = good_resource(), c.nof_symbols = 3, refused("three symbols", c);
  c = good_resource(), c.comb_size = 8, refused("comb 8", c);
  c = good_resource(), c.comb_offset = 4, refused("comb offset 4 of comb 4", c);
  c = good_resource(), c.comb_size = 2, c.comb_offset = 2, refused("comb offset 2 of comb 2", c);
  c = good_resource(), c.cyclic_shift = 12, refused("cyclic shift 12 of comb 4", c);
  c = good_resource(), c.comb_size = 2, c.comb_offset = 1, c.cyclic_shift = 8, refused("cyclic shift 8 of comb 2", c);
  c = good_resource(), c.bandwidth_index = 4, refused("B_SRS 4", c);
  c = good_resource(), c.freq_hopping = 0, refused("frequency hopping", c);
  c = good_resource(), c.hopping = 1, refused("group hopping", c);
  c = good_resource(), c.hopping = 2, refused("sequence hopping", c);
  c = good_resource(), c.nof_rx_ports = 0, refused("no rx port", c);
  c = good_resource(), c.nof_rx_ports = 5, refused("five rx ports", c);
  c = good_resource(), c.rx_ports[1] = 4, refused("rx port outside the grid", c);
  refused("rx port outside a 2-port grid", good_resource(), 52, 2);
  c = good_resource(), c.rx_ports[1] = 2, refused("rx port listed twice", c);
  c = good_resource(), c.start_symbol = 13, refused("symbols past the slot", c);
  c = good_resource(), c.sequence_id = 1024, refused("sequence_id 1024", c);
  c = good_resource(), c.freq_shift = 269, refused("freq_shift 269", c);
  c = good_resource(), c.freq_position = 68, refused("freq_position 68", c);
  c = good_resource(), c.m_srs[1] = 22, refused("m_srs no multiple of 4", c);
  c = good_resource(), c.N[0] = 2, refused("N[0] not 1", c);
  c = good_resource(), c.N[2] = 3, refused("m_srs[2] N[2] not m_srs[1]", c);
  c = good_resource(), c.N[3] = 0, refused("N[3] zero", c);
  c = good_resource(), c.m_srs[0] = 276, c.N[0] = 1, refused("m_srs above 272", c);
  refused("resource past the grid", good_resource(), 50);
  c = good_resource(), c.freq_shift = 200, refused("resource past the grid by its shift", c, 52);
  c = good_resource(), c.grid_index = 2, refused("grid outside the grids", c);
  c = good_resource(), c.result_index = 2, refused("result outside the resources", c);
  CHECK(srs_refusal(good_resource(), 51, 4, 2, 2, d).empty(), "the resource ends in PRB 50");

  srs_refusal(good_resource(), 52, 4, 2, 2, d);
  const uint32_t rows[4] = {10, 20, 30, 40};
  const srs_job  j       = srs_make_job(good_resource(), d, rows, 52, 4);
  CHECK(j.nsc == 624 && j.port_stride == 14 * 624 && j.grid_base == 4 * 14 * 624 && j.result_index == 1 && j.L == 72 &&
            j.comb == 4 && j.nof_tx == 4 && j.nof_rx == 2 && j.nof_symbols == 2 && j.start_symbol == 12 && j.interleaved == 1 &&
            j.khz == 30 && j.k0[1] == d.k0[1] && j.seq_row[3] == 40 && j.rx_ports[0] == 2 && j.rx_ports[1] == 0 &&
            j.rx_ports[3] == 2 && j.fs == d.fs && j.M == d.M && j.max_ta_samples == d.max_ta_samples,
        "job");
  CHECK(srs_sequence(30, 72, 0, 12).empty() && srs_sequence(3, 30 + 1, 0, 12).empty(), "undefined sequences");
}

} // namespace

int main(int argc, char** argv)
{
  if (argc < 2) {
    std::printf("usage: %s DUMP\n", argv[0]);
    return 2;
  }
  std::ifstream           f(argv[1], std::ios::binary);
  const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  size_t                  pos = 0;
  const uint32_t          n   = take<uint32_t>(raw, pos);
  for (uint32_t i = 0; i < n; ++i) {
    const srsgpu_srs_config c   = take<srsgpu_srs_config>(raw, pos);
    const uint32_t          prb = take<uint32_t>(raw, pos);
    uint32_t                v[15];
    for (uint32_t& x : v) {
      x = take<uint32_t>(raw, pos);
    }
    const double      fs = take<double>(raw, pos);
    srs_derived       d;
    const std::string why = srs_refusal(c, prb, 4, c.grid_index + 1, c.result_index + 1, d);
    CHECK(why.empty(), "resource %u: %s", i, why.c_str());
    bool same = d.L == v[0] && d.n_cs_max == v[1] && d.u == v[2] && d.interleaved == v[3] && d.M == v[12] && d.log2M == v[13] &&
                d.max_ta_samples == v[14] && d.fs == fs;
    for (uint32_t p = 0; p < c.nof_antenna_ports; ++p) {
      same = same && d.n_cs[p] == v[4 + p] && d.k0[p] == v[8 + p];
    }
    CHECK(same, "resource %u: L %u n_cs %u %u %u %u k0 %u %u %u %u M %u max_ta_samples %u (wanted %u) fs %g", i, d.L, d.n_cs[0],
          d.n_cs[1], d.n_cs[2], d.n_cs[3], d.k0[0], d.k0[1], d.k0[2], d.k0[3], d.M, d.max_ta_samples, v[14], d.fs);
    // One PRB less and the resource no longer fits.
    CHECK(!srs_refusal(c, prb - 1, 4, c.grid_index + 1, c.result_index + 1, d).empty(), "resource %u fits %u PRBs", i, prb - 1);
  }
  const uint32_t m = take<uint32_t>(raw, pos);
  for (uint32_t i = 0; i < m; ++i) {
    const uint32_t u = take<uint32_t>(raw, pos), L = take<uint32_t>(raw, pos), n_cs = take<uint32_t>(raw, pos),
                   n_cs_max = take<uint32_t>(raw, pos);
    const std::vector<float> s = srs_sequence(u, L, n_cs, n_cs_max);
    CHECK(s.size() == 2u * L, "size");
    double worst = 0.0;
    for (uint32_t k = 0; k < L && s.size() == 2u * L; ++k) {
      const double re = take<double>(raw, pos), im = take<double>(raw, pos);
      worst           = std::max(worst, std::hypot(s[2 * k] - re, s[2 * k + 1] - im));
    }
    CHECK(worst < 2e-7, "sequence u %u L %u n_cs %u / %u deviates by %g", u, L, n_cs, n_cs_max, worst);
  }
  CHECK(pos == raw.size(), "dump has %zu bytes left", raw.size() - pos);
  const std::vector<float> t = unit_roots(SRS_CEXP_SIZE);
  CHECK(t.size() == 2048 && t[0] == 1.0F && t[1] == 0.0F && std::fabs(t[2 * 256 + 1] - 1.0F) < 1e-7F && std::fabs(t[2 * 512] + 1.0F) < 1e-7F &&
            std::fabs(t[2 * 128] - std::sqrt(0.5F)) < 1e-7F,
        "phase table");
  check_refusals();
  std::printf("%u resources, %u sequences, %d failures\n", n, m, failures);
  return failures == 0 ? 0 : 1;
}
