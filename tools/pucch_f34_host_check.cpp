// Stand-alone check of srsran-5g_amd/csrc/pucch_f34_host.cpp, built with -fsanitize=address,undefined by
// tests/test_pucch_f34_oracle.py (no HIP, nothing loaded into Python).
//
//   pucch_f34_host_check DUMP
//       DUMP: u32 n; per PDU the 40 bytes of srsgpu_pucch_f34_config, u32 grid_nof_prb, u32 grid_nof_ports, and what the
//       Python restatement derives from it: u32 DM-RS symbol mask, u32 number of LLRs, u32 number of DM-RS symbols and
//       per DM-RS symbol its u32 symbol of the slot and 12 nof_prb x (f32 re, f32 im); u32 number of scrambling words
//       and the words; 12 x (f32 re, f32 im) of w_n (Format 4 only); 2 x f32 epoch distances of the hops' first two
//       DM-RS symbols (1 where a hop has one); u32 number of data symbols and per data symbol u8 symbol, u8 hop.
// Then the hand-made part: the DM-RS table's shape, every refusal with its message, the code rates, the overlap search.
#include "host_util.h"
#include "pucch_f34_host.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

using namespace srsgpu;

namespace {

int failures = 0;

void expect(bool ok, const char* what, unsigned index = 0)
{
  if (!ok) {
    ++failures;
    std::printf("FAIL %s (%u)\n", what, index);
  }
}

template <typename T>
T take(const std::vector<char>& raw, size_t& pos)
{
  T v{};
  if (pos + sizeof(T) > raw.size()) {
    std::printf("FAIL dump too short\n");
    std::exit(1);
  }
  std::memcpy(&v, raw.data() + pos, sizeof(T));
  pos += sizeof(T);
  return v;
}

bool close_to(const std::vector<float>& got, const std::vector<char>& raw, size_t& pos, size_t count)
{
  bool ok = got.size() == count;
  for (size_t i = 0; i < count; ++i) {
    const float want = take<float>(raw, pos);
    ok               = ok && i < got.size() && std::fabs(got[i] - want) < 2e-6F;
  }
  return ok;
}

srsgpu_pucch_f34_config base_config()
{
  srsgpu_pucch_f34_config c;
  std::memset(&c, 0, sizeof(c));
  c.format             = 3;
  c.numerology         = 1;
  c.nof_prb            = 2;
  c.start_symbol_index = 2;
  c.nof_symbols        = 8;
  c.starting_prb       = 3;
  c.second_hop_prb     = PUCCH_F34_NO_HOP;
  c.occ_length         = 2;
  c.rnti               = 0x4601;
  c.n_id_scrambling    = 77;
  c.n_id_hopping       = 500;
  c.nof_uci_bits       = 20;
  c.nof_ports          = 2;
  c.ports[1]           = 1;
  return c;
}

void refused(srsgpu_pucch_f34_config c, const char* needle, unsigned index, uint32_t prb = 24, uint32_t ports = 2, uint32_t grids = 1)
{
  const std::string why = pucch_f34_refusal(c, prb, ports, grids);
  expect(why.find(needle) != std::string::npos, needle, index);
}

void dumped(const char* path)
{
  std::ifstream           f(path, std::ios::binary);
  const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  size_t                  pos = 0;
  const uint32_t          n   = take<uint32_t>(raw, pos);
  for (uint32_t i = 0; i < n; ++i) {
    const auto     c        = take<srsgpu_pucch_f34_config>(raw, pos);
    const uint32_t grid_prb = take<uint32_t>(raw, pos), grid_ports = take<uint32_t>(raw, pos);
    expect(pucch_f34_refusal(c, grid_prb, grid_ports, 3).empty(), "a dumped PDU is accepted", i);
    const bool hop = c.second_hop_prb != PUCCH_F34_NO_HOP;
    expect(pucch_f34_dmrs_mask(c.nof_symbols, hop, c.additional_dmrs != 0) == take<uint32_t>(raw, pos), "DM-RS mask", i);
    expect(pucch_f34_nof_llrs(c) == take<uint32_t>(raw, pos), "number of LLRs", i);
    const pucch_f34_job j = pucch_f34_make_job(c, grid_prb, grid_ports, 5, 7, 9);
    expect(j.nof_dmrs == take<uint32_t>(raw, pos), "number of DM-RS symbols", i);
    for (uint32_t s = 0; s < j.nof_dmrs; ++s) {
      expect(j.dmrs_symbol[s] == take<uint32_t>(raw, pos), "DM-RS symbol", i);
      expect(close_to(pucch_f34_dmrs(c, j.dmrs_symbol[s]), raw, pos, 24u * c.nof_prb), "DM-RS sequence", i);
    }
    const uint32_t              nwords = take<uint32_t>(raw, pos);
    const std::vector<uint32_t> words  = pucch_f34_scrambling(c, j.nof_llrs);
    expect(words.size() == nwords, "number of scrambling words", i);
    for (uint32_t w = 0; w < nwords; ++w) {
      const uint32_t want = take<uint32_t>(raw, pos);
      expect(w < words.size() && words[w] == want, "scrambling word", i);
    }
    if (c.format == 4) {
      const std::vector<float> w = pucch_f4_w(c.occ_length, c.occ_index);
      size_t                   at = pos;
      expect(close_to(w, raw, pos, 24), "w_n", i);
      for (uint32_t k = 0; k < 12; ++k) {  // 1 / w = j^w_quarter
        const float re = take<float>(raw, at), im = take<float>(raw, at);
        const float qr[4] = {1, 0, -1, 0}, qi[4] = {0, 1, 0, -1};
        expect(std::fabs(qr[j.w_quarter[k]] - re) < 1e-6F && std::fabs(qi[j.w_quarter[k]] + im) < 1e-6F, "1 / w_n", i);
      }
    }
    for (uint32_t h = 0; h < 2; ++h) {
      expect(std::fabs(j.cfo_delta[h] - take<float>(raw, pos)) < 1e-6F, "epoch distance", i);
    }
    expect(j.nof_data == take<uint32_t>(raw, pos), "number of data symbols", i);
    for (uint32_t d = 0; d < j.nof_data; ++d) {
      const uint8_t sym = take<uint8_t>(raw, pos), dh = take<uint8_t>(raw, pos);
      expect(j.data_symbol[d] == sym && j.data_hop[d] == dh, "data symbol and hop", i);
    }
    expect(j.nof_hops == (hop ? 2u : 1u) && j.root_row == 7 && j.dmrs_row == 5 && j.scramble_word == 9, "job rows", i);
    expect(j.hop_nof_dmrs[0] + j.hop_nof_dmrs[1] == j.nof_dmrs && j.nof_dmrs + j.nof_data == c.nof_symbols, "symbol split", i);
    expect(std::fabs(j.idft_scale - 1.0F / std::sqrt(12.0F * c.nof_prb)) < 1e-9F, "IDFT scale", i);
  }
  expect(pos == raw.size(), "the dump is consumed");
  std::printf("%u dumped PDUs\n", n);
}

void hand_made()
{
  // The DM-RS table: 1, 2 or 4 symbols, inside the allocation, both hops served when hopping.
  for (uint32_t n = 4; n <= 14; ++n) {
    for (uint32_t hop = 0; hop < 2; ++hop) {
      for (uint32_t add = 0; add < 2; ++add) {
        const uint32_t m     = pucch_f34_dmrs_mask(n, hop != 0, add != 0);
        const uint32_t count = static_cast<uint32_t>(__builtin_popcount(m));
        const uint32_t want  = n == 4 ? (hop ? 2u : 1u) : (add && n >= 10 ? 4u : 2u);
        expect(count == want && (m >> n) == 0, "DM-RS table shape", n);
        if (hop) {
          expect((m & ((1u << (n / 2)) - 1u)) != 0 && (m >> (n / 2)) != 0, "a DM-RS symbol in each hop", n);
        }
      }
    }
  }
  expect(pucch_f34_dmrs_mask(3, false, false) == 0 && pucch_f34_dmrs_mask(15, true, true) == 0, "no table outside 4..14");
  for (uint32_t p = 1; p <= 16; ++p) {
    const bool bad = p == 7 || p == 11 || p == 13 || p == 14;
    expect(pucch_f34_transform_size_ok(p) == !bad, "transform sizes", p);
  }
  expect(!pucch_f34_transform_size_ok(0), "transform size 0");

  srsgpu_pucch_f34_config c = base_config();
  expect(pucch_f34_refusal(c, 24, 2, 1).empty(), "the base PDU is accepted");
  unsigned k = 0;
  { auto d = c; d.format = 2; refused(d, "neither 3 nor 4", k++); }
  { auto d = c; d.numerology = 5; refused(d, "numerology", k++); }
  { auto d = c; d.cp_extended = 1; refused(d, "extended cyclic prefix", k++); }
  { auto d = c; d.slot_index = 20; refused(d, "slot index", k++); }
  { auto d = c; d.pi2_bpsk = 2; refused(d, "flags", k++); }
  { auto d = c; d.nof_symbols = 3; refused(d, "Invalid Number of OFDM symbols", k++); }
  { auto d = c; d.nof_symbols = 15; d.start_symbol_index = 0; refused(d, "Invalid Number of OFDM symbols", k++); }
  { auto d = c; d.nof_prb = 0; refused(d, "outside the allowed range", k++); }
  { auto d = c; d.nof_prb = 17; refused(d, "outside the allowed range", k++); }
  for (uint8_t p : {7, 11, 13, 14}) {
    auto d = c; d.nof_prb = p; refused(d, "not valid for the transform precoder", k++);
  }
  { auto d = c; d.format = 4; refused(d, "one PRB", k++); }
  { auto d = c; d.format = 4; d.nof_prb = 1; d.occ_length = 3; refused(d, "Invalid OCC length", k++); }
  { auto d = c; d.format = 4; d.nof_prb = 1; d.occ_length = 4; d.occ_index = 4; refused(d, "Invalid sequence index", k++); }
  { auto d = c; d.starting_prb = 23; refused(d, "outside grid (first hop)", k++); }
  { auto d = c; d.second_hop_prb = 23; refused(d, "outside grid (second hop)", k++); }
  { auto d = c; d.start_symbol_index = 7; refused(d, "exceeding the number of symbols", k++); }
  { auto d = c; d.numerology = 2; d.cp_extended = 1; d.start_symbol_index = 5; refused(d, "extended CP", k++); }
  { auto d = c; d.nof_ports = 0; refused(d, "cannot be zero", k++); }
  { auto d = c; d.nof_ports = 3; refused(d, "exceeds the configured maximum", k++); }
  { auto d = c; d.ports[1] = 2; refused(d, "outside the grid", k++); }
  { auto d = c; d.ports[1] = 0; refused(d, "listed twice", k++); }
  { auto d = c; d.nof_uci_bits = 240; refused(d, "exceeds the maximum allowed 0.8", k++); }  // (240 + 11) / 288
  { auto d = c; d.nof_uci_bits = 2; refused(d, "outside the supported range", k++); }
  { auto d = c; d.nof_prb = 16; d.nof_symbols = 14; d.start_symbol_index = 0; d.nof_uci_bits = 1707; refused(d, "outside the supported range", k++); }
  { auto d = c; d.n_id_scrambling = 1024; refused(d, "outside 0..1023", k++); }
  { auto d = c; d.n_id_hopping = 1024; refused(d, "outside 0..1023", k++); }
  { auto d = c; d.grid_index = 1; refused(d, "grid_index", k++); }
  { auto d = c; d.llr_offset = 6; refused(d, "multiple of 4", k++); }
  { auto d = c; d.llr_offset = 0xfffffffcu; refused(d, "below 2^32", k++); }
  // The code rate is checked before the payload range: a payload of 2000 bits reports the rate.
  { auto d = c; d.nof_uci_bits = 2000; refused(d, "exceeds the maximum allowed 0.8", k++); }

  // Code rates: Format 3, 2 PRB x 6 data symbols, QPSK: (20 + 11) / 288; pi/2-BPSK halves the channel bits.
  expect(std::fabs(pucch_f34_code_rate(c) - 31.0F / 288.0F) < 1e-7F, "Format 3 code rate");
  { auto d = c; d.pi2_bpsk = 1; expect(std::fabs(pucch_f34_code_rate(d) - 31.0F / 144.0F) < 1e-7F, "pi/2-BPSK code rate"); }
  // Format 4, SF 4: E = 24 x 6 / 4 = 36 LLRs, but the denominator keeps all 144 channel bits.
  { auto d = c; d.format = 4; d.nof_prb = 1; d.occ_length = 4; expect(pucch_f34_nof_llrs(d) == 36, "Format 4 LLRs");
    expect(std::fabs(pucch_f34_code_rate(d) - 31.0F / 144.0F) < 1e-7F, "Format 4 code rate"); }
  // Two codeblocks from 360 bits on at E >= 1088: 4 PRB x 14 symbols, QPSK: E = 1152, CRC 22.
  { auto d = c; d.nof_prb = 4; d.nof_symbols = 14; d.start_symbol_index = 0; d.nof_uci_bits = 360;
    expect(pucch_f34_nof_llrs(d) == 1152 && std::fabs(pucch_f34_code_rate(d) - 382.0F / 1152.0F) < 1e-7F, "two codeblocks"); }
  // 9 LLRs: SF 4, pi/2-BPSK, 3 data symbols.
  { auto d = c; d.format = 4; d.nof_prb = 1; d.occ_length = 4; d.pi2_bpsk = 1; d.nof_symbols = 4; d.nof_uci_bits = 3;
    expect(pucch_f34_nof_llrs(d) == 9 && pucch_f34_refusal(d, 24, 2, 1).empty(), "9 LLRs"); }

  // Overlap: ranges of 9 LLRs at 0 and 12 do not overlap, at 0 and 8 they do; order does not matter.
  srsgpu_pucch_f34_config two[2] = {c, c};
  for (auto& d : two) {
    d.format = 4; d.nof_prb = 1; d.occ_length = 4; d.pi2_bpsk = 1; d.nof_symbols = 4; d.nof_uci_bits = 3;
  }
  two[0].llr_offset = 12;
  expect(pucch_f34_llr_overlap(two, 2).empty(), "adjacent ranges");
  two[0].llr_offset = 8;
  expect(pucch_f34_llr_overlap(two, 2).find("overlap") != std::string::npos, "overlapping ranges");
  expect(pucch_f34_llr_overlap(two, 0).empty(), "no PDUs");

  // Tables: the roots and the orthogonal sequences.
  const std::vector<float> r = unit_roots(12);
  expect(r.size() == 24 && std::fabs(r[0] - 1) < 1e-7F && std::fabs(r[6]) < 1e-7F && std::fabs(r[7] - 1) < 1e-7F, "roots");
  expect(pucch_f4_w(3, 0).empty() && pucch_f4_w(2, 2).empty() && pucch_f4_w(4, 3).size() == 24, "w_n lengths");
  const std::vector<uint32_t> words = pucch_f34_scrambling(c, 4608);
  expect(words.size() == 144 && pucch_f34_scrambling(c, 9).size() == 1, "scrambling words");
}

} // namespace

int main(int argc, char** argv)
{
  if (argc > 1) {
    dumped(argv[1]);
  }
  hand_made();
  std::printf("%d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
