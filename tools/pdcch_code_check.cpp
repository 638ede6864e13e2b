// Host-only check of the PDCCH plan's table construction (srsran-5g_amd/csrc/polar_code.cpp: polar_dl_code_build;
// pdcch_host.cpp: pdcch_refusal, pdcch_prbs) against tables dumped from the fixture tests/golden/pdcch.npz, built with
// the address and undefined-behaviour sanitizers by tests/test_pdcch_oracle.py. No HIP, nothing loaded into Python.
//
//   pdcch_code_check DUMP   DUMP: u32 nof_codes, then per code u32 K, E, n, N bytes (1 frozen), K bytes (input
//                           interleaver), E u16 (rate-matching gather table); u32 nof_dcis, then per DCI 16 u32
//                           (bwp_size_rb, bwp_start_rb, start_symbol, duration, frequency_resources low / high, mapping,
//                           reg_bundle_size, interleaver_size, shift_index, cce_index, aggregation_level,
//                           nof_payload_bits, nof_ports, grid_nof_prb, grid_nof_ports), u32 nof_prbs and the PRBs as u16.
//                           Prints "<codes> codes, <dcis> DCIs" and exits 0 when everything agrees.
#include "pdcch_host.h"
#include "polar_code.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

using namespace srsgpu;

namespace {

struct reader {
  std::vector<uint8_t> raw;
  size_t               pos = 0;
  explicit reader(const char* path)
  {
    std::ifstream in(path, std::ios::binary);
    raw.assign((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  }
  template <typename T>
  std::vector<T> take(size_t count)
  {
    if (pos + count * sizeof(T) > raw.size()) {
      std::fprintf(stderr, "pdcch_code_check: truncated dump\n");
      std::exit(2);
    }
    std::vector<T> out(count);
    if (count > 0) {
      std::memcpy(out.data(), raw.data() + pos, count * sizeof(T));
    }
    pos += count * sizeof(T);
    return out;
  }
  uint32_t u32() { return take<uint32_t>(1)[0]; }
};

int failures = 0;

void expect(bool ok, const char* what, uint32_t a, uint32_t b)
{
  if (!ok) {
    std::printf("MISMATCH %s (%u, %u)\n", what, a, b);
    ++failures;
  }
}

/// u_source against the input interleaver and the allocation done one after the other; the tables' ranges.
void check_composition(const polar_dl_code& code)
{
  const uint32_t N = 1u << code.n;
  uint32_t       k = 0;
  for (uint32_t q = 0; q < N; ++q) {
    if (code.frozen[q] != 0) {
      expect(code.u_source[q] == POLAR_DL_FROZEN, "u_source of a frozen position", code.K, q);
    } else {
      expect(k < code.K && code.u_source[q] == code.input_interleaver[k], "u_source of a message position", code.K, q);
      ++k;
    }
  }
  expect(k == code.K, "number of message positions", code.K, k);
  std::vector<uint8_t> seen(code.K, 0);
  for (uint8_t v : code.input_interleaver) {
    expect(v < code.K && seen[v]++ == 0, "input interleaver is a permutation", code.K, v);
  }
  for (uint16_t g : code.gather) {
    expect(g < N, "gather entry inside the mother code", code.K, g);
  }
}

} // namespace

int main(int argc, char** argv)
{
  if (argc < 2) {
    std::fprintf(stderr, "usage: pdcch_code_check DUMP\n");
    return 2;
  }
  reader         r(argv[1]);
  const uint32_t nof_codes = r.u32();
  for (uint32_t i = 0; i < nof_codes; ++i) {
    const uint32_t K = r.u32(), E = r.u32(), n = r.u32();
    const auto     frozen = r.take<uint8_t>(1u << n);
    const auto     pi     = r.take<uint8_t>(K);
    const auto     gather = r.take<uint16_t>(E);
    expect(polar_dl_code_refusal(K, E) == nullptr, "refused", K, E);
    polar_dl_code code;
    polar_dl_code_build(K, E, code);
    expect(code.n == n, "n", K, E);
    expect(code.frozen == frozen, "frozen set", K, E);
    expect(code.input_interleaver == pi, "input interleaver", K, E);
    expect(code.gather == gather, "gather table", K, E);
    check_composition(code);
  }
  // The limits of the downlink code (polar_code_impl.cpp:339, :363).
  expect(polar_dl_code_refusal(35, 108) != nullptr && polar_dl_code_refusal(165, 216) != nullptr, "K limits", 35, 165);
  expect(polar_dl_code_refusal(108, 108) != nullptr && polar_dl_code_refusal(107, 108) == nullptr, "K < E", 108, 108);

  const uint32_t nof_dcis = r.u32();
  for (uint32_t i = 0; i < nof_dcis; ++i) {
    const auto  f = r.take<uint32_t>(16);
    pdcch_alloc a;
    a.bwp_size_rb         = f[0];
    a.bwp_start_rb        = f[1];
    a.start_symbol        = f[2];
    a.duration            = f[3];
    a.frequency_resources = f[4] | (static_cast<uint64_t>(f[5]) << 32);
    a.mapping             = f[6];
    a.reg_bundle_size     = f[7];
    a.interleaver_size    = f[8];
    a.shift_index         = f[9];
    a.cce_index           = f[10];
    a.aggregation_level   = f[11];
    a.nof_payload_bits    = f[12];
    a.nof_ports           = f[13];
    const auto        want = r.take<uint16_t>(r.u32());
    const std::string why  = pdcch_refusal(a, f[14], f[15]);
    if (!why.empty()) {
      std::printf("DCI %u refused: %s\n", i, why.c_str());
      ++failures;
      continue;
    }
    expect(pdcch_prbs(a) == want, "PRBs of DCI", i, a.aggregation_level);
    // One PRB less in the grid refuses the DCI whose top PRB is the grid's last.
    if (!want.empty() && want.back() + 1u == f[14]) {
      expect(!pdcch_refusal(a, f[14] - 1, f[15]).empty(), "PRB outside the grid accepted", i, want.back());
    }
    // Field values that wrap 32-bit sums are refused like any other out-of-range value.
    pdcch_alloc wrap = a;
    wrap.start_symbol = 0xffffffffu;
    expect(!pdcch_refusal(wrap, f[14], f[15]).empty(), "wrapping start symbol accepted", i, 0);
    wrap                  = a;
    wrap.cce_index        = 0xffffffffu;
    expect(!pdcch_refusal(wrap, f[14], f[15]).empty(), "wrapping CCE index accepted", i, 0);
    wrap                  = a;
    wrap.nof_payload_bits = 0xfffffff0u;
    expect(!pdcch_refusal(wrap, f[14], f[15]).empty(), "wrapping payload size accepted", i, 0);
  }
  expect(r.pos == r.raw.size(), "dump fully read", static_cast<uint32_t>(r.pos), static_cast<uint32_t>(r.raw.size()));

  // Arbitrary field values: every allocation is either refused with a message or mapped inside the BWP.
  uint32_t state = 12345u, accepted = 0;
  auto     next  = [&state](uint32_t mod) {
    state = state * 1664525u + 1013904223u;
    return (state >> 8) % mod;
  };
  for (uint32_t i = 0; i < 20000; ++i) {
    pdcch_alloc a;
    a.bwp_size_rb         = next(300);
    a.bwp_start_rb        = next(300);
    a.start_symbol        = next(16);
    a.duration            = next(5);
    a.frequency_resources = (static_cast<uint64_t>(next(1u << 23)) << 23) | next(1u << 23);
    a.mapping             = next(4);
    a.reg_bundle_size     = next(8);
    a.interleaver_size    = next(8);
    a.shift_index         = i % 7 == 0 ? 0xffffffffu - next(100) : next(1024);
    a.cce_index           = i % 11 == 0 ? 0xffffffffu - next(20) : next(140);
    a.aggregation_level   = 1u << next(6);
    a.nof_payload_bits    = next(150);
    a.nof_ports           = next(6);
    if (pdcch_refusal(a, 275, 4).empty()) {
      ++accepted;
      const auto prbs = pdcch_prbs(a);
      expect(prbs.size() == 6 * a.aggregation_level / a.duration, "PRB count", i, static_cast<uint32_t>(prbs.size()));
      for (size_t j = 0; j < prbs.size(); ++j) {
        expect(prbs[j] < a.bwp_start_rb + a.bwp_size_rb && prbs[j] >= a.bwp_start_rb && (j == 0 || prbs[j] > prbs[j - 1]),
               "PRBs ascending inside the BWP", i, prbs[j]);
      }
    }
  }
  expect(accepted > 20, "some arbitrary allocations are accepted", accepted, 0);

  std::printf("%u codes, %u DCIs, %u arbitrary allocations accepted, %d failures\n", nof_codes, nof_dcis, accepted, failures);
  return failures == 0 ? 0 : 1;
}
