// Stand-alone check of the NZP-CSI-RS host construction (srsran-5g_amd/csrc/csi_rs_host.cpp), built with the address
// and undefined-behaviour sanitizers by tests/test_csi_rs_oracle.py::test_host_construction. No GPU, no Python.
//
//   csi_rs_host_check DUMP   DUMP: u32 nof_signals, then per signal 16 u32 (slot_index, cp, start_rb, nof_rb, row, k_ref,
//                            symbol_l0, symbol_l1, cdm, freq_density, scrambling_id, nof_ports, grid_nof_prb,
//                            grid_nof_ports, seq_len, seq_skip), a float (amplitude), u32 n and n x 3 u32 (symbol,
//                            subcarrier, c_init of the symbol): the REs the reference wrote on port 0, ascending, with
//                            the restatement's sequence length, skipped elements and c_init. Then u32 nof_refusals and
//                            per refusal the same record with nof_k_ref in place of seq_len (seq_skip unused), u32
//                            len and len characters the reason must contain.
#include "csi_rs_host.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <limits>
#include <string>
#include <vector>

using namespace srsgpu;

namespace {

int failures = 0;

void expect(bool ok, const char* what, uint32_t a, uint32_t b)
{
  if (!ok) {
    std::printf("FAIL %s (%u, %u)\n", what, a, b);
    ++failures;
  }
}

struct reader {
  std::vector<uint8_t> raw;
  size_t               pos = 0;
  template <typename T>
  std::vector<T> take(size_t n)
  {
    std::vector<T> v(n);
    if (pos + n * sizeof(T) > raw.size()) {
      std::printf("FAIL truncated dump\n");
      std::exit(1);
    }
    if (n > 0) {
      std::memcpy(v.data(), raw.data() + pos, n * sizeof(T));
    }
    pos += n * sizeof(T);
    return v;
  }
  uint32_t u32() { return take<uint32_t>(1)[0]; }
};

csi_rs_signal signal_of(const std::vector<uint32_t>& f, float amplitude)
{
  csi_rs_signal s;
  s.slot_index    = f[0];
  s.cp            = f[1];
  s.start_rb      = f[2];
  s.nof_rb        = f[3];
  s.row           = f[4];
  s.nof_k_ref     = 1;
  s.k_ref[0]      = f[5];
  s.symbol_l0     = f[6];
  s.symbol_l1     = f[7];
  s.cdm           = f[8];
  s.freq_density  = f[9];
  s.scrambling_id = f[10];
  s.nof_ports     = f[11];
  s.amplitude     = amplitude;
  return s;
}

/// (symbol, subcarrier, c_init) of every RE of the layout, ascending.
std::vector<uint32_t> res_of(const csi_rs_layout& y)
{
  std::vector<uint32_t> out;
  for (uint32_t g = 0; g < y.nof_groups; ++g) {
    for (uint32_t i = 0; i < y.seq_len; ++i) {
      const uint32_t rb = y.rb_begin + y.rb_stride * (i / y.per_rb);
      out.insert(out.end(), {y.symbol[g], 12 * rb + y.k_bar[g] + y.k_step * (i % y.per_rb), y.c_init[g]});
    }
  }
  // Row 4 interleaves its two groups on one symbol: order by (symbol, subcarrier).
  std::vector<uint32_t> sorted;
  std::vector<size_t>   idx(out.size() / 3);
  for (size_t i = 0; i < idx.size(); ++i) {
    idx[i] = i;
  }
  for (size_t i = 1; i < idx.size(); ++i) {
    for (size_t j = i; j > 0; --j) {
      const size_t a = idx[j - 1], b = idx[j];
      if (out[3 * a] < out[3 * b] || (out[3 * a] == out[3 * b] && out[3 * a + 1] <= out[3 * b + 1])) {
        break;
      }
      std::swap(idx[j - 1], idx[j]);
    }
  }
  for (size_t i : idx) {
    sorted.insert(sorted.end(), {out[3 * i], out[3 * i + 1], out[3 * i + 2]});
  }
  return sorted;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc != 2) {
    std::fprintf(stderr, "usage: csi_rs_host_check DUMP\n");
    return 2;
  }
  reader        r;
  std::ifstream in(argv[1], std::ios::binary);
  r.raw.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());

  const uint32_t nof_signals = r.u32();
  for (uint32_t i = 0; i < nof_signals; ++i) {
    const auto          f    = r.take<uint32_t>(16);
    const float         amp  = r.take<float>(1)[0];
    const auto          want = r.take<uint32_t>(3 * static_cast<size_t>(r.u32()));
    const csi_rs_signal s    = signal_of(f, amp);
    const std::string   why  = csi_rs_refusal(s, f[12], f[13]);
    if (!why.empty()) {
      std::printf("signal %u refused: %s\n", i, why.c_str());
      ++failures;
      continue;
    }
    const csi_rs_layout y = csi_rs_layout_of(s);
    expect(y.seq_len == f[14], "sequence length", i, y.seq_len);
    expect(y.seq_skip == f[15], "skipped elements", i, y.seq_skip);
    expect(y.seq_len == y.nof_rbs * y.per_rb, "sequence length against the RB comb", i, y.nof_rbs);
    expect(res_of(y) == want, "REs and c_init", i, y.seq_len);
    const float a = static_cast<float>(M_SQRT1_2 * static_cast<double>(amp));
    expect(std::memcmp(&a, &y.amplitude, 4) == 0, "amplitude", i, 0);
    // One PRB less in the grid refuses the signal that ends on the grid's last PRB; a port less, the row's ports.
    if (s.start_rb + s.nof_rb == f[12]) {
      expect(!csi_rs_refusal(s, f[12] - 1, f[13]).empty(), "RBs outside the grid accepted", i, 0);
    }
    if (y.nof_ports > 1) {
      expect(!csi_rs_refusal(s, f[12], y.nof_ports - 1).empty(), "ports outside the grid accepted", i, 0);
    }
    // Field values that wrap 32-bit sums are refused like any other out-of-range value.
    csi_rs_signal wrap = s;
    wrap.start_rb      = 0xffffffffu;
    expect(!csi_rs_refusal(wrap, f[12], f[13]).empty(), "wrapping start_rb accepted", i, 0);
    wrap           = s;
    wrap.nof_rb    = 0xfffffff0u;
    wrap.start_rb  = 32;
    expect(!csi_rs_refusal(wrap, f[12], f[13]).empty(), "wrapping nof_rb accepted", i, 0);
    wrap           = s;
    wrap.symbol_l0 = 0xffffffffu;
    expect(!csi_rs_refusal(wrap, f[12], f[13]).empty(), "wrapping l_0 accepted", i, 0);
  }

  const uint32_t nof_refusals = r.u32();
  for (uint32_t i = 0; i < nof_refusals; ++i) {
    const auto        f    = r.take<uint32_t>(16);
    const float       amp  = r.take<float>(1)[0];
    const auto        text = r.take<char>(r.u32());
    const std::string want(text.begin(), text.end());
    csi_rs_signal     s = signal_of(f, amp);
    s.nof_k_ref         = f[14];
    const std::string why = csi_rs_refusal(s, f[12], f[13]);
    if (why.find(want) == std::string::npos) {
      std::printf("FAIL refusal %u: wanted '%s', got '%s'\n", i, want.c_str(), why.c_str());
      ++failures;
    }
  }
  expect(r.pos == r.raw.size(), "dump fully read", static_cast<uint32_t>(r.pos), static_cast<uint32_t>(r.raw.size()));

  // Arbitrary field values: every signal is either refused with a message or laid out inside the grid.
  uint32_t state = 54321u, accepted = 0;
  auto     next  = [&state](uint32_t mod) {
    state = state * 1664525u + 1013904223u;
    return (state >> 8) % mod;
  };
  for (uint32_t i = 0; i < 40000; ++i) {
    csi_rs_signal s;
    s.slot_index    = next(170);
    s.cp            = next(20) == 0 ? 2 : next(2);
    s.start_rb      = i % 13 == 0 ? 0xffffffffu - next(50) : next(150);
    s.nof_rb        = i % 17 == 0 ? 0xffffffffu - next(50) : next(150);
    s.row           = next(10) == 0 ? next(20) : 1 + next(5);
    s.nof_k_ref     = next(5) == 0 ? next(8) : 1;
    s.k_ref[0]      = next(14);
    s.symbol_l0     = next(16);
    s.symbol_l1     = next(16);
    s.cdm           = next(10) == 0 ? next(5) : next(2);
    s.freq_density  = next(4 + next(2));
    s.scrambling_id = next(1030);
    s.nof_ports     = next(4) == 0 ? next(6) : (s.row <= 2 ? 1u : s.row == 3 ? 2u : 4u);
    s.amplitude     = i % 19 == 0 ? std::numeric_limits<float>::infinity() : 0.25f * static_cast<float>(next(16));
    const uint32_t grid_nof_prb = 275 - next(3) * next(100), grid_nof_ports = 4 - next(2) * next(4);
    if (csi_rs_refusal(s, grid_nof_prb, grid_nof_ports).empty()) {
      ++accepted;
      const csi_rs_layout y = csi_rs_layout_of(s);
      expect(y.seq_len == y.nof_rbs * y.per_rb, "sequence length against the RB comb", i, y.seq_len);
      expect(y.nof_ports <= grid_nof_ports && y.nof_groups * y.cdm_size == y.nof_ports, "ports", i, y.nof_ports);
      expect(2 * (y.seq_skip + y.seq_len) <= 2048, "the sequence lies in chunk 0", i, y.seq_skip + y.seq_len);
      for (uint32_t g = 0; g < y.nof_groups; ++g) {
        expect(y.symbol[g] < (s.cp != 0 ? 12u : 14u), "symbol", i, y.symbol[g]);
        expect(y.k_bar[g] + y.k_step * (y.per_rb - 1) < 12, "subcarrier of the RB", i, y.k_bar[g]);
        expect(y.c_init[g] < (1u << 31), "c_init", i, y.c_init[g]);
      }
      if (y.nof_rbs > 0) {
        const uint32_t last = y.rb_begin + y.rb_stride * (y.nof_rbs - 1);
        expect(y.rb_begin >= s.start_rb && last < s.start_rb + s.nof_rb && last < grid_nof_prb, "RBs", i, last);
      }
    }
  }
  expect(accepted > 1000, "some arbitrary signals are accepted", accepted, 0);

  std::printf("%u signals, %u refusals, %u arbitrary signals accepted, %d failures\n", nof_signals, nof_refusals, accepted,
              failures);
  return failures == 0 ? 0 : 1;
}
