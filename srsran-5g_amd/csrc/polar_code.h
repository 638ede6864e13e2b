// Host-side construction of the uplink polar code (nMax = 10) of TS 38.212 sections 5.3.1.2 and 5.4.1.1 for the UCI
// polar decoder plan (capi_uci_polar_decoder.cpp, uci_polar_decoder.hip): everything the kernel reads as tables is
// fixed here at plan creation, per distinct (K, E). No HIP call in this translation unit, so that a host-only program
// can check it (tools/polar_code_check.cpp). The downlink code (nMax = 9) of the PDCCH plan is built here too, from the
// same frozen-set rules (polar_dl_code below; tools/pdcch_code_check.cpp).
//
// Reference (behaviour, not code): lib/phy/upper/channel_coding/polar/polar_code_impl.cpp:325 (set_code_params), :421
// (set); the three dematching steps of polar_rate_dematcher_impl.cpp:100 composed into one table; the node types and
// the tree walk of polar_decoder_impl.cpp:85 / :310 flattened into an op list; polar_deallocator_impl.cpp:27.
#pragma once
#include <cstdint>
#include <vector>

namespace srsgpu {

/// Dematching table entries that are no LLR offset: a punctured position or a repetition that does not exist (0), and
/// a shortened position (+127, polar_rate_dematcher_impl.cpp:66).
constexpr uint16_t POLAR_DEMAP_NONE      = 0xffff;
constexpr uint16_t POLAR_DEMAP_SHORTENED = 0xfffe;

/// Ops of the flattened successive-cancellation walk: type | stage << 2 | position << 6. F and G compute the LLRs of
/// stage - 1 from those of `stage` (G with the estimated bits [position, position + 2^(stage-1))); LEAF is a rate-1
/// node of 2^stage bits at `position`; COMBINE xors the upper half of the estimated bits of the node of 2^stage bits at
/// `position` into its lower half. Rate-0 nodes emit nothing.
enum polar_op_type : uint32_t { POLAR_OP_F = 0, POLAR_OP_G = 1, POLAR_OP_LEAF = 2, POLAR_OP_COMBINE = 3 };

constexpr uint32_t polar_op(polar_op_type type, uint32_t stage, uint32_t position)
{
  return static_cast<uint32_t>(type) | (stage << 2) | (position << 6);
}

struct polar_code {
  uint32_t K = 0, E = 0;
  uint32_t n = 0;       ///< log2 of the mother code size N.
  uint32_t nPC = 0;     ///< Parity-check bits (3 for K <= 25).
  uint32_t nWmPC = 0;   ///< Of which placed by row weight (the reference fixes position 252 or 248).
  std::vector<uint8_t>  frozen;       ///< N entries, 1 = frozen (the complement of the K + nPC most reliable).
  std::vector<uint16_t> pc;           ///< nPC positions, increasing.
  std::vector<uint16_t> info;         ///< The K message positions, increasing, PC positions skipped.
  std::vector<uint16_t> interleaver;  ///< Sub-block interleaver J(0..N-1).
  /// Composed dematching map, R = max(1, ceil(E / N)) rows of N: entry [r N + p] is the offset in the codeblock's LLRs
  /// of the r-th LLR of mother-code position p (accumulated in increasing r), or one of the marks above.
  std::vector<uint16_t> demap;
  std::vector<uint32_t> ops;          ///< The decoder's schedule.
  std::vector<uint16_t> crc_weight;   ///< x^(K-1-k) mod g for de-allocated bit k (CRC6 for K <= 25, else CRC11).
};

/// Why the reference's assertions refuse (K, E) (polar_code_impl.cpp:334, :345, :363, :407), or nullptr.
const char* polar_code_refusal(uint32_t K, uint32_t E);

/// log2 of the mother code size (polar_code_impl.cpp:365-404).
uint32_t polar_code_size_log(uint32_t K, uint32_t E);

/// Fills `code` for an accepted (K, E).
void polar_code_build(uint32_t K, uint32_t E, polar_code& code);

/// Downlink polar code (nMax = 9, no parity-check bits, input interleaver, no channel interleaver) of the PDCCH plan
/// (capi_pdcch.cpp, pdcch.hip). Reference (behaviour, not code): pdcch_encoder_impl.cpp:63 (channel_coding),
/// polar_code_impl.cpp:325 / :421 with nMax = 9, polar_interleaver_impl.cpp:45, polar_allocator_impl.cpp:27,
/// polar_rate_matcher_impl.cpp:100 without its channel interleaver.
constexpr uint32_t POLAR_DL_K_MAX  = 164;   ///< polar_interleaver_impl::K_MAX_IL
constexpr uint8_t  POLAR_DL_FROZEN = 0xff;  ///< u_source mark of a frozen position.

struct polar_dl_code {
  uint32_t K = 0, E = 0;
  uint32_t n = 0;                          ///< log2 of the mother code size N (5..9).
  std::vector<uint8_t>  frozen;            ///< N entries, 1 = frozen.
  std::vector<uint8_t>  input_interleaver; ///< K entries: c'[k] = c[input_interleaver[k]] (TS 38.212 Table 5.3.1.1-1).
  /// Input interleaver and allocation composed: N entries, the index in c of the bit at encoder input position q, or
  /// POLAR_DL_FROZEN.
  std::vector<uint8_t>  u_source;
  /// Sub-block interleaver and bit selection composed: E entries, rate-matched bit j is encoded bit gather[j].
  std::vector<uint16_t> gather;
};

/// Why the reference's assertions refuse a downlink (K, E) (polar_code_impl.cpp:334, :339, :363), or nullptr.
const char* polar_dl_code_refusal(uint32_t K, uint32_t E);

/// Fills `code` for an accepted downlink (K, E).
void polar_dl_code_build(uint32_t K, uint32_t E, polar_dl_code& code);

/// Codeblocks of a UCI field of A bits in E LLRs (uci_info.h:40, uci_decoder_impl.cpp:49-69).
struct uci_polar_segmentation {
  uint32_t nof_codeblocks;  ///< 1 or 2.
  uint32_t crc_size;        ///< 6 or 11.
  uint32_t K;               ///< Message, filler and CRC bits; the same for both codeblocks.
  uint32_t E_cb;            ///< LLRs per codeblock; codeblock 1 starts at E_cb.
  uint32_t filler;          ///< Filler bits ahead of codeblock 0's message bits.
  uint32_t bits0;           ///< Message bits of codeblock 0 (the rest are codeblock 1's).
};

constexpr uci_polar_segmentation uci_polar_segment(uint32_t A, uint32_t E)
{
  const uint32_t C = ((A >= 360 && E >= 1088) || A >= 1013) ? 2 : 1;
  const uint32_t L = A < 20 ? 6 : 11;
  return {C, L, A / C + A % C + L, E / C, A % C, A / C};
}

} // namespace srsgpu
