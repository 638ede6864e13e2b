// Uplink polar code construction for the UCI polar decoder plan and downlink construction for the PDCCH plan; see
// polar_code.h. Written from TS 38.212 sections 5.3.1.1 (input interleaver), 5.3.1.2 (n, the frozen and parity-check
// sets) and 5.4.1.1 (sub-block interleaver, bit selection, channel interleaver) and the reference's behaviour where it
// departs from the text (noted at each place).
#include "polar_code.h"
#include "polar_dl_tables.h"
#include "polar_tables.h"
#include <algorithm>

namespace srsgpu {

namespace {

constexpr uint32_t N_MAX_LOG = 10;
constexpr uint32_t E_MAX     = 8192;  // polar_code::EMAX

/// The walk of polar_decoder_impl::simplified_node (:310) over the node types of :85, flattened.
struct schedule_builder {
  const std::vector<uint32_t>& frozen_before;  // prefix counts of frozen positions
  uint32_t                     N;
  std::vector<uint32_t>&       ops;
  bool                         finished = false;

  void node(uint32_t stage, uint32_t pos)
  {
    const uint32_t size   = 1u << stage;
    const uint32_t frozen = frozen_before[pos + size] - frozen_before[pos];
    if (frozen == size) {
      // rate_0_node (:209): only a last, single frozen bit ends the walk.
      finished = pos == N - 1;
      return;
    }
    if (frozen == 0) {
      ops.push_back(polar_op(POLAR_OP_LEAF, stage, pos));
      finished = pos + size == N;  // rate_1_node (:254)
      return;
    }
    // rate_r_node (:259), with its early returns once the last bit is decided.
    ops.push_back(polar_op(POLAR_OP_F, stage, pos));
    node(stage - 1, pos);
    if (finished) {
      return;
    }
    ops.push_back(polar_op(POLAR_OP_G, stage, pos));
    node(stage - 1, pos + size / 2);
    if (finished) {
      return;
    }
    ops.push_back(polar_op(POLAR_OP_COMBINE, stage, pos));
  }
};

} // namespace

/// log2 of the mother code size for an uplink (n_max_log = 10) or downlink (9) code (polar_code_impl.cpp:365-404).
static uint32_t size_log(uint32_t K, uint32_t E, uint32_t n_max_log)
{
  uint32_t e = 1;
  while ((1u << e) < E) {
    ++e;
  }
  const uint32_t n1 = (8 * E <= 9 * (1u << (e - 1)) && 16 * K < 9 * E) ? e - 1 : e;
  uint32_t       k  = 0;
  while (k < 10 && (1u << k) < K) {
    ++k;
  }
  return std::max(5u, std::min({n1, k + 3, n_max_log}));
}

uint32_t polar_code_size_log(uint32_t K, uint32_t E)
{
  return size_log(K, E, N_MAX_LOG);
}

/// Sub-block interleaver and the `count` most reliable positions the rate matching leaves usable, increasing
/// reliability (polar_code_impl.cpp:426-456), shared by the uplink and downlink constructions.
static void reliable_set(uint32_t K, uint32_t E, uint32_t n, uint32_t count, std::vector<uint16_t>& interleaver,
                         std::vector<uint16_t>& k_set)
{
  const uint32_t N = 1u << n;
  // Sub-block interleaver, section 5.4.1.1: J(i) = P(floor(32 i / N)) N / 32 + i mod (N / 32).
  interleaver.resize(N);
  for (uint32_t i = 0; i < N; ++i) {
    interleaver[i] = static_cast<uint16_t>(kPolarSubblockPattern[32 * i / N] * (N / 32) + i % (N / 32));
  }

  // Frozen set, section 5.3.1.2: positions that the rate matching drops (the first N - E after interleaving when
  // puncturing, 16 K <= 7 E, with a further low range; the last N - E when shortening) cannot carry information.
  std::vector<uint8_t> excluded(N, 0);
  const bool           puncture = E < N && 16 * K <= 7 * E;
  const bool           shorten  = E < N && !puncture;
  if (puncture) {
    // The reference excludes positions 0..T (polar_code_impl.cpp:440-445, :306): for E < 3 N / 4 that is one more than
    // the ceil(9 N / 16 - E / 4) of the specification. Restated as the reference behaves.
    const uint32_t T = E >= 3 * N / 4 ? 3 * N / 4 - E / 2 - 1 : 9 * N / 16 - E / 4;
    for (uint32_t i = 0; i < N - E; ++i) {
      excluded[interleaver[i]] = 1;
    }
    for (uint32_t q = 0; q <= T && q < N; ++q) {
      excluded[q] = 1;
    }
  } else if (shorten) {
    for (uint32_t i = E; i < N; ++i) {
      excluded[interleaver[i]] = 1;
    }
    excluded[0] = 1;  // T = 0 in the reference's set difference (:306).
  }
  // The `count` most reliable of the remaining positions, least reliable first.
  k_set.clear();
  for (int i = 1023; i >= 0 && k_set.size() < count; --i) {
    const uint16_t q = kPolarReliabilitySequence[i];
    if (q < N && excluded[q] == 0) {
      k_set.push_back(q);
    }
  }
  std::reverse(k_set.begin(), k_set.end());
}

const char* polar_code_refusal(uint32_t K, uint32_t E)
{
  if (E > E_MAX) {
    return "more than 8192 encoded bits per codeblock";
  }
  if (K < 18 || (K > 25 && K < 31)) {
    return "K (message, filler and CRC bits per codeblock) outside 18..25 and 31..1023";
  }
  if (K > 1023) {
    return "K (message, filler and CRC bits per codeblock) above 1023";
  }
  if (K + (K <= 25 ? 3u : 0u) >= E) {
    return "K + nPC does not fit the encoded bits of the codeblock";
  }
  if (K >= (1u << polar_code_size_log(K, E))) {
    return "K does not fit the mother code size N";
  }
  return nullptr;
}

void polar_code_build(uint32_t K, uint32_t E, polar_code& code)
{
  code       = polar_code{};
  code.K     = K;
  code.E     = E;
  code.n     = polar_code_size_log(K, E);
  code.nPC   = K <= 25 ? 3 : 0;
  code.nWmPC = (code.nPC > 0 && E > K + 189) ? 1 : 0;
  const uint32_t N = 1u << code.n;

  std::vector<uint16_t> k_set;
  reliable_set(K, E, code.n, K + code.nPC, code.interleaver, k_set);
  const bool puncture = E < N && 16 * K <= 7 * E;
  const bool shorten  = E < N && !puncture;
  code.frozen.assign(N, 1);
  for (uint16_t q : k_set) {
    code.frozen[q] = 0;
  }
  // Parity-check positions: the nPC - nWmPC least reliable of the set, and for nWmPC = 1 the reference's fixed choice
  // (:465: 252 for K <= 21, else 248; N = 256 whenever nWmPC = 1).
  for (uint32_t i = 0; i + code.nWmPC < code.nPC && i < k_set.size(); ++i) {
    code.pc.push_back(k_set[i]);
  }
  if (code.nWmPC == 1) {
    code.pc.push_back(K <= 21 ? 252 : 248);
  }
  std::sort(code.pc.begin(), code.pc.end());
  // De-allocation order (polar_deallocator_impl.cpp:34): increasing position, the parity-check positions skipped.
  for (uint32_t q = 0; q < N; ++q) {
    if (code.frozen[q] == 0 && std::find(code.pc.begin(), code.pc.end(), q) == code.pc.end()) {
      code.info.push_back(static_cast<uint16_t>(q));
    }
  }

  // Channel de-interleaver (polar_rate_dematcher_impl.cpp:74): source[i] = offset in the codeblock's LLRs of e_i. The
  // triangle of side T, T (T + 1) / 2 >= E, is written by rows and read by columns.
  std::vector<uint16_t> source(E);
  {
    uint32_t T = 1;
    while (T * (T + 1) / 2 < E) {
      ++T;
    }
    uint32_t out = 0;
    for (uint32_t r = 0; r < T; ++r) {
      uint32_t in = r;
      for (uint32_t c = 0; c < T - r && in < E; ++c) {
        source[in] = static_cast<uint16_t>(out++);
        in += T - c;
      }
    }
  }
  // Composed with the bit de-selection (:45) and the sub-block de-interleaver (:29).
  const uint32_t R = std::max(1u, (E + N - 1) / N);
  code.demap.assign(static_cast<size_t>(R) * N, POLAR_DEMAP_NONE);
  for (uint32_t j = 0; j < N; ++j) {
    const uint32_t p = code.interleaver[j];
    if (puncture) {
      code.demap[p] = j < N - E ? POLAR_DEMAP_NONE : source[j - (N - E)];
    } else if (shorten) {
      code.demap[p] = j < E ? source[j] : POLAR_DEMAP_SHORTENED;
    } else {
      for (uint32_t r = 0; r * N + j < E; ++r) {
        code.demap[static_cast<size_t>(r) * N + p] = source[r * N + j];
      }
    }
  }

  // Decoder schedule.
  std::vector<uint32_t> frozen_before(N + 1, 0);
  for (uint32_t q = 0; q < N; ++q) {
    frozen_before[q + 1] = frozen_before[q] + code.frozen[q];
  }
  schedule_builder builder{frozen_before, N, code.ops};
  builder.node(code.n, 0);

  // CRC weights: the remainder of the K de-allocated bits is the xor of x^(K-1-k) mod g over the set bits k
  // (crc_calculator_generic_impl.cpp:50 / :54: CRC11 0xe21, CRC6 0x61; uci_info.h:54).
  const uint32_t order = K <= 25 ? 6 : 11, poly = K <= 25 ? 0x61 : 0xe21;
  code.crc_weight.resize(K);
  uint32_t power = 1;
  for (uint32_t i = 0; i < K; ++i) {
    code.crc_weight[K - 1 - i] = static_cast<uint16_t>(power);
    power <<= 1;
    if ((power >> order) != 0) {
      power ^= poly;
    }
  }
}

const char* polar_dl_code_refusal(uint32_t K, uint32_t E)
{
  if (K < 36 || K > POLAR_DL_K_MAX) {
    return "K (payload and CRC bits) outside 36..164";
  }
  if (K >= E) {
    return "K does not fit the encoded bits";
  }
  if (E > E_MAX) {
    return "more than 8192 encoded bits";
  }
  return nullptr;
}

void polar_dl_code_build(uint32_t K, uint32_t E, polar_dl_code& code)
{
  code   = polar_dl_code{};
  code.K = K;
  code.E = E;
  code.n = size_log(K, E, 9);
  const uint32_t N = 1u << code.n;

  std::vector<uint16_t> interleaver, k_set;
  reliable_set(K, E, code.n, K, interleaver, k_set);
  code.frozen.assign(N, 1);
  for (uint16_t q : k_set) {
    code.frozen[q] = 0;
  }

  // Input interleaver (polar_interleaver_impl.cpp:45): the pattern entries of at least 164 - K, in table order, less
  // 164 - K: c'[k] = c[pi[k]].
  for (uint32_t m = 0; m < POLAR_DL_K_MAX; ++m) {
    if (kPolarInputInterleaverPattern[m] >= POLAR_DL_K_MAX - K) {
      code.input_interleaver.push_back(static_cast<uint8_t>(kPolarInputInterleaverPattern[m] - (POLAR_DL_K_MAX - K)));
    }
  }

  // Allocation (polar_allocator_impl.cpp: no parity-check bits, increasing position) composed with it.
  code.u_source.assign(N, POLAR_DL_FROZEN);
  uint32_t k = 0;
  for (uint32_t q = 0; q < N; ++q) {
    if (code.frozen[q] == 0) {
      code.u_source[q] = code.input_interleaver[k++];
    }
  }

  // Sub-block interleaver and bit selection (polar_rate_matcher_impl.cpp:41), no channel interleaver.
  const bool puncture = E < N && 16 * K <= 7 * E;
  code.gather.resize(E);
  for (uint32_t j = 0; j < E; ++j) {
    code.gather[j] = interleaver[E >= N ? j % N : puncture ? j + (N - E) : j];
  }
}

} // namespace srsgpu
