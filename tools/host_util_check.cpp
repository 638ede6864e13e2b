// Stand-alone check of srsran-5g_amd/csrc/host_util.h (no HIP, no GPU), built by tests/test_host_util.py with the
// address and undefined-behaviour sanitizers and run as a child process.
//
//   host_util_check DUMP   DUMP (written by the test from the numpy restatement the fixtures trust):
//                          u32 n; n x (u32 c_init, u32 first, u32 count, count x u8 Gold bits);
//                          u32 m; m x (u32 size, 2 size x f64 cos / sin of 2 pi k / size).
// Checks gold_bits and unit_roots against the dump, gold_words against the packed gold_bits, pucch_n_cs against the
// sequence's bytes, the overlap search, every shared refusal with its message, the UCI rules and the grid geometry.
#include "host_util.h"
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

void check_gold_words(uint32_t c_init)
{
  for (uint32_t nof_words : {0u, 1u, 2u, 5u}) {
    const std::vector<uint32_t> words = gold_words(c_init, nof_words);
    std::vector<uint8_t>        bits(32 * nof_words);
    gold_bits(c_init, 0, 32 * nof_words, bits.data());
    CHECK(words.size() == nof_words, "c_init %u: %zu words", c_init, words.size());
    for (uint32_t i = 0; i < 32 * nof_words && i < 32 * words.size(); ++i) {
      CHECK(((words[i >> 5] >> (i & 31u)) & 1u) == bits[i], "c_init %u: bit %u of %u words", c_init, i, nof_words);
    }
  }
  // The byte b of the sequence, first bit the least significant, is n_cs of symbol b of slot 0 and of its other splits.
  const std::vector<uint32_t> words = gold_words(c_init, 70);
  for (uint32_t b : {0u, 3u, 13u, 14u, 279u}) {
    const uint32_t byte = (words[b >> 2] >> (8 * (b & 3u))) & 0xffu;
    CHECK(pucch_n_cs(c_init, 14, b / 14, b % 14) == byte && pucch_n_cs(c_init, 12, b / 12, b % 12) == byte,
          "n_cs of c_init %u, byte %u", c_init, b);
  }
}

void check_dump(const char* path)
{
  std::ifstream     f(path, std::ios::binary);
  std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  size_t            pos = 0;
  const uint32_t    n   = take<uint32_t>(raw, pos);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c_init = take<uint32_t>(raw, pos), first = take<uint32_t>(raw, pos), count = take<uint32_t>(raw, pos);
    std::vector<uint8_t> got(count);  // exactly count bytes: a bit written past them is the sanitizer's to find
    gold_bits(c_init, first, count, got.data());
    for (uint32_t k = 0; k < count; ++k) {
      const uint8_t want = take<uint8_t>(raw, pos);
      CHECK(got[k] == want, "c_init %u: c(%u) = %u, not %u", c_init, first + k, got[k], want);
    }
    if (first == 0) {
      check_gold_words(c_init);
    }
  }
  const uint32_t m = take<uint32_t>(raw, pos);
  for (uint32_t i = 0; i < m; ++i) {
    const uint32_t           size = take<uint32_t>(raw, pos);
    const std::vector<float> r    = unit_roots(size);
    CHECK(r.size() == 2 * size, "%u roots: %zu floats", size, r.size());
    for (uint32_t k = 0; k < 2 * size; ++k) {
      // A float nearest to a value in [-1, 1] lies within 2^-25 of it; the two libraries' doubles differ by far less.
      const double want = take<double>(raw, pos);
      CHECK(k >= r.size() || std::fabs(r[k] - want) <= 0x1p-24, "%u roots: float %u is %.9g, not %.17g", size, k, r[k], want);
    }
    CHECK(r.size() < 2 || (r[0] == 1.0F && r[1] == 0.0F), "%u roots: the first is not 1", size);
  }
  CHECK(pos == raw.size(), "dump has %zu bytes left", raw.size() - pos);
  std::printf("%u Gold ranges, %u root tables\n", n, m);
}

bool has(const std::string& s, const char* part)
{
  return s.find(part) != std::string::npos;
}

void check_overlap()
{
  const uint32_t adjacent[3] = {64, 160, 0}, lengths[3] = {96, 96, 64};  // unsorted: [0, 64) [64, 160) [160, 256)
  CHECK(llr_overlap(adjacent, lengths, 3).empty(), "adjacent ranges overlap: %s", llr_overlap(adjacent, lengths, 3).c_str());
  const uint32_t  crossing[3] = {64, 156, 0};
  const std::string why       = llr_overlap(crossing, lengths, 3);
  CHECK(why == "the LLRs of PDU 0 (96 at offset 64) overlap those of PDU 1 (offset 156)", "\"%s\"", why.c_str());
  const uint32_t equal[3] = {64, 64, 0};
  CHECK(has(llr_overlap(equal, lengths, 3), "PDU 0 (96 at offset 64) overlap those of PDU 1"), "equal offsets pass");
  const uint32_t top[2] = {0xfffffffcu, 0}, top_lengths[2] = {4, 4};
  CHECK(llr_overlap(top, top_lengths, 2).empty(), "a range that ends at 2^32 overlaps the one at 0");
  CHECK(llr_overlap(adjacent, lengths, 0).empty() && llr_overlap(adjacent, lengths, 1).empty() &&
            llr_overlap(nullptr, nullptr, 0).empty(),
        "no or one PDU overlaps");
}

void check_refusals()
{
  CHECK(numerology_refusal(4).empty() && numerology_refusal(5) == "numerology 5 is outside 0..4", "numerology");
  CHECK(slot_refusal(0, 0, 9).empty() && slot_refusal(2, 1, 39).empty() && slot_refusal(4, 0, 159).empty(), "good slots");
  CHECK(slot_refusal(5, 0, 0) == "numerology 5 is outside 0..4", "numerology comes first");
  CHECK(slot_refusal(1, 1, 99) == "the extended cyclic prefix exists at numerology 2 only (numerology 1)", "CP before slot");
  CHECK(has(slot_refusal(2, 2, 0), "extended cyclic prefix"), "cp_extended 2");
  CHECK(slot_refusal(1, 0, 20) == "slot index 20 is outside the frame of 20 slots", "slot index");

  CHECK(symbol_allocation_refusal(12, 2, 0).empty() && symbol_allocation_refusal(10, 2, 1).empty(), "good allocations");
  CHECK(symbol_allocation_refusal(13, 2, 0) == "OFDM symbol allocation goes up to symbol 15, exceeding the number of symbols "
                                               "in the given slot with normal CP, i.e., 14.", "normal CP");
  CHECK(symbol_allocation_refusal(11, 2, 1) == "OFDM symbol allocation goes up to symbol 13, exceeding the number of symbols "
                                               "in the given slot with extended CP, i.e., 12.", "extended CP");

  const uint8_t ports[4] = {2, 0, 3, 2};
  CHECK(rx_ports_refusal(ports, 3, 4, 4).empty() && rx_port_list_refusal(ports, 0, 4).empty(), "good port lists");
  CHECK(rx_ports_refusal(ports, 0, 4, 4) == "The number of receive ports cannot be zero.", "no ports");
  CHECK(rx_ports_refusal(ports, 3, 2, 4) == "The number of receive ports, i.e. 3, exceeds the configured maximum number of "
                                            "receive ports, i.e., 2.", "more ports than the grid");
  CHECK(rx_ports_refusal(ports, 3, 4, 2) == "The number of receive ports, i.e. 3, exceeds the configured maximum number of "
                                            "receive ports, i.e., 2.", "more ports than the plan");
  CHECK(rx_ports_refusal(ports, 3, 3, 4) == "Rx port 3 lies outside the grid (3 ports)", "a port outside the grid");
  CHECK(rx_port_list_refusal(ports, 4, 4) == "Rx port 2 is listed twice", "a port twice");
  CHECK(rx_port_list_refusal(ports, 4, 3) == "Rx port 3 lies outside the grid (3 ports)", "outside comes before twice");

  CHECK(grid_index_refusal(1, 2).empty() && grid_index_refusal(2, 2) == "grid_index 2 is outside the 2 grids", "grid_index");
  CHECK(llr_offset_refusal(64, 96).empty() && llr_offset_refusal(0xfffffffcu, 3).empty(), "good LLR offsets");
  CHECK(llr_offset_refusal(6, 96) == "llr_offset 6 is no multiple of 4", "alignment");
  CHECK(llr_offset_refusal(0xfffffffcu, 4) == "llr_offset 4294967292 leaves no room for the LLRs below 2^32", "room");
  CHECK(has(llr_offset_refusal(0xfffffffeu, 4), "multiple of 4"), "alignment comes before room");
  // A message longer than the buffer is cut, not overrun.
  CHECK(format("%0300d", 1).size() == 255, "format cuts at 255 characters");
}

void check_rules()
{
  CHECK(uci_crc_size(11) == 0 && uci_crc_size(12) == 6 && uci_crc_size(19) == 6 && uci_crc_size(20) == 11, "CRC sizes");
  CHECK(uci_nof_codeblocks(359, 1088) == 1 && uci_nof_codeblocks(360, 1087) == 1 && uci_nof_codeblocks(360, 1088) == 2 &&
            uci_nof_codeblocks(1012, 1087) == 1 && uci_nof_codeblocks(1013, 0) == 2,
        "codeblock rule");
  const grid_geometry g(52, 4, 3);
  CHECK(g.nsc == 624 && g.port_stride == 8736 && g.grid_base == 3 * 4 * 8736, "grid geometry");
  CHECK(pucch_nsymb_per_slot(0) == 14 && pucch_nsymb_per_slot(1) == 12, "symbols per slot");
  CHECK(symbol_epochs(0, false).size() == 14 && symbol_epochs(2, true).size() == 12, "epoch counts");
}

} // namespace

int main(int argc, char** argv)
{
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s DUMP\n", argv[0]);
    return 2;
  }
  check_dump(argv[1]);
  check_overlap();
  check_refusals();
  check_rules();
  std::printf("%d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
