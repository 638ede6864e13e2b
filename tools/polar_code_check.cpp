// Stand-alone check of srsran-5g_amd/csrc/polar_code.cpp (no GPU, no Python): built by
// tests/test_uci_polar_oracle.py with the address and undefined-behaviour sanitizers.
//
//   polar_code_check DUMP    DUMP: u32 nof_codes, then per code u32 K, E, n, nPC, N bytes (1 frozen), 3 u16 (PC set),
//                            N u16 (sub-block interleaver), as the reference's polar_code_impl::set leaves them
//                            (tests/golden/uci_polar.npz).
//
// Per code it compares n, nPC, the frozen mask, the PC set and the interleaver with the dump; checks the message
// positions; rebuilds the composed dematching map from its three steps done one after the other; and runs the op list
// through a scalar interpreter against a recursive successive-cancellation decoder on pseudo-random LLRs. Exits
// non-zero on the first difference.
#include "polar_code.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

using namespace srsgpu;

namespace {

[[noreturn]] void die(uint32_t K, uint32_t E, const char* what)
{
  std::printf("polar_code_check: K=%u E=%u: %s differs\n", K, E, what);
  std::exit(1);
}

int sat_sum(int a, int b)
{
  if (a == -b) {
    return 0;
  }
  if (std::abs(a) > 120) {
    return a;
  }
  if (std::abs(b) > 120) {
    return b;
  }
  const int s = a + b;
  return s > 120 ? 120 : s < -120 ? -120 : s;
}

int soft_xor(int a, int b)
{
  const int m = std::min(std::abs(a), std::abs(b));
  return a * b < 0 ? -m : m;
}

void transform(uint8_t* x, uint32_t size)
{
  for (uint32_t t = 1; t < size; t <<= 1) {
    for (uint32_t i = 0; i < size; ++i) {
      if ((i & t) == 0) {
        x[i] ^= x[i + t];
      }
    }
  }
}

/// Recursive decoder: returns the node's estimated bits in est[pos..pos+size), the decoded bits in u.
void decode_node(const std::vector<int>& llr, uint32_t pos, const polar_code& c, std::vector<uint8_t>& est,
                 std::vector<uint8_t>& u)
{
  const uint32_t size   = static_cast<uint32_t>(llr.size());
  uint32_t       frozen = 0;
  for (uint32_t i = 0; i < size; ++i) {
    frozen += c.frozen[pos + i];
  }
  if (frozen == size) {
    return;
  }
  if (frozen == 0) {
    for (uint32_t i = 0; i < size; ++i) {
      est[pos + i] = u[pos + i] = llr[i] <= 0;
    }
    transform(&u[pos], size);
    return;
  }
  const uint32_t   half = size / 2;
  std::vector<int> child(half);
  for (uint32_t i = 0; i < half; ++i) {
    child[i] = soft_xor(llr[i], llr[i + half]);
  }
  decode_node(child, pos, c, est, u);
  for (uint32_t i = 0; i < half; ++i) {
    child[i] = sat_sum(llr[i + half], est[pos + i] ? -llr[i] : llr[i]);
  }
  decode_node(child, pos + half, c, est, u);
  for (uint32_t i = 0; i < half; ++i) {
    est[pos + i] ^= est[pos + half + i];
  }
}

/// The op list as the kernel reads it: stage s lives at llr[2^s .. 2^(s+1)).
std::vector<uint8_t> run_ops(const std::vector<int>& top, const polar_code& c)
{
  const uint32_t       N = 1u << c.n;
  std::vector<int>     llr(2 * N, 0);
  std::vector<uint8_t> est(N, 0), u(N, 0);
  std::copy(top.begin(), top.end(), llr.begin() + N);
  for (uint32_t op : c.ops) {
    const uint32_t type = op & 3u, s = (op >> 2) & 15u, pos = op >> 6, size = 1u << s, half = size / 2;
    if (s > c.n || pos + size > N || pos % size != 0 || (type != POLAR_OP_LEAF && s == 0)) {
      die(c.K, c.E, "op bounds");
    }
    int* in  = &llr[size];
    int* out = &llr[half];
    switch (type) {
      case POLAR_OP_F:
        for (uint32_t i = 0; i < half; ++i) {
          out[i] = soft_xor(in[i], in[i + half]);
        }
        break;
      case POLAR_OP_G:
        for (uint32_t i = 0; i < half; ++i) {
          out[i] = sat_sum(in[i + half], est[pos + i] ? -in[i] : in[i]);
        }
        break;
      case POLAR_OP_LEAF:
        for (uint32_t i = 0; i < size; ++i) {
          est[pos + i] = u[pos + i] = in[i] <= 0;
        }
        transform(&u[pos], size);
        break;
      default:
        for (uint32_t i = 0; i < half; ++i) {
          est[pos + i] ^= est[pos + half + i];
        }
    }
  }
  return u;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc < 2) {
    std::fprintf(stderr, "usage: polar_code_check DUMP\n");
    return 2;
  }
  std::ifstream        in(argv[1], std::ios::binary);
  std::vector<uint8_t> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  size_t               pos  = 0;
  auto                 take = [&](void* dst, size_t bytes) {
    if (pos + bytes > raw.size()) {
      std::printf("polar_code_check: truncated dump\n");
      std::exit(2);
    }
    std::memcpy(dst, raw.data() + pos, bytes);
    pos += bytes;
  };
  // The reference's assertions (polar_code_impl.cpp:334, :345, :363), the K ranges included that no UCI field reaches.
  const struct {
    uint32_t K, E;
    bool     accepted;
  } probes[] = {{17, 100, false},  {18, 100, true},    {25, 100, true},   {26, 100, false}, {30, 100, false},
                {31, 100, true},   {1023, 2000, true}, {1024, 2000, false}, {18, 21, false}, {18, 22, true},
                {31, 31, false},   {31, 32, true},     {100, 8193, false}, {100, 8192, true}, {18, 0, false}};
  for (const auto& p : probes) {
    if ((polar_code_refusal(p.K, p.E) == nullptr) != p.accepted) {
      die(p.K, p.E, "acceptance");
    }
  }
  uint32_t count = 0;
  take(&count, 4);
  uint32_t seed = 12345;
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t head[4];
    take(head, 16);
    const uint32_t K = head[0], E = head[1];
    if (polar_code_refusal(K, E) != nullptr) {
      die(K, E, "acceptance");
    }
    polar_code c;
    polar_code_build(K, E, c);
    const uint32_t        N = 1u << head[2];
    std::vector<uint8_t>  frozen(N);
    std::vector<uint16_t> jj(N);
    uint16_t              pc[3];
    take(frozen.data(), N);
    take(pc, 6);
    take(jj.data(), 2 * N);
    if (c.n != head[2]) {
      die(K, E, "n");
    }
    if (c.nPC != head[3] || c.pc.size() != c.nPC || !std::equal(c.pc.begin(), c.pc.end(), pc)) {
      die(K, E, "PC set");
    }
    if (c.frozen != frozen) {
      die(K, E, "F-set");
    }
    if (c.interleaver != jj) {
      die(K, E, "interleaver");
    }
    if (c.info.size() != K || c.crc_weight.size() != K) {
      die(K, E, "message positions");
    }
    for (uint32_t k = 0; k < K; ++k) {
      if (c.frozen[c.info[k]] != 0 || (k > 0 && c.info[k] <= c.info[k - 1])) {
        die(K, E, "message positions");
      }
    }
    // Dematching in three steps on LLR "names": f_i is called i + 1; 0 stands for a punctured position, -1 for a
    // shortened one. Repetitions are listed in the order the reference adds them.
    std::vector<int> e(E);
    {
      uint32_t T = 1, S = 1;
      while (S < E) {
        S += ++T;
      }
      uint32_t out = 0;
      for (uint32_t r = 0; r != T; ++r) {
        uint32_t at = r;
        for (uint32_t col = 0; col != T - r && at < E; ++col) {
          e[at] = static_cast<int>(++out);
          at += T - col;
        }
      }
    }
    const uint32_t                R = c.demap.size() / N;
    std::vector<std::vector<int>> y(N);
    for (uint32_t j = 0; j < N; ++j) {
      if (E >= N) {
        for (uint32_t k = j; k < E; k += N) {
          y[j].push_back(e[k]);
        }
      } else if (16 * K <= 7 * E) {
        y[j].push_back(j < N - E ? 0 : e[j - (N - E)]);
      } else {
        y[j].push_back(j < E ? e[j] : -1);
      }
    }
    if (c.demap.size() != static_cast<size_t>(R) * N || R != std::max(1u, (E + N - 1) / N)) {
      die(K, E, "dematching map size");
    }
    for (uint32_t j = 0; j < N; ++j) {
      const uint32_t p = jj[j];
      for (uint32_t r = 0; r < R; ++r) {
        const uint16_t t    = c.demap[static_cast<size_t>(r) * N + p];
        const int      want = r < y[j].size() ? y[j][r] : 0;
        const int      got  = t == POLAR_DEMAP_NONE ? 0 : t == POLAR_DEMAP_SHORTENED ? -1 : static_cast<int>(t) + 1;
        if (got != want || (t < POLAR_DEMAP_SHORTENED && t >= E)) {
          die(K, E, "dematching map");
        }
      }
    }
    // The op list against the recursive decoder, LLRs over the whole range including +-127 and 0.
    for (int round = 0; round < 3; ++round) {
      std::vector<int> top(N);
      for (int& v : top) {
        seed         = seed * 1664525u + 1013904223u;
        const int x  = static_cast<int>((seed >> 16) % 255u) - 127;
        v            = (std::abs(x) > 120 && std::abs(x) != 127) ? 0 : (round == 2 ? x / 40 : x);
      }
      std::vector<uint8_t> est(N, 0), u(N, 0);
      decode_node(top, 0, c, est, u);
      if (run_ops(top, c) != u) {
        die(K, E, "op list");
      }
    }
  }
  if (pos != raw.size()) {
    std::printf("polar_code_check: trailing bytes in the dump\n");
    return 2;
  }
  std::printf("polar_code_check: %u codes agree\n", count);
  return 0;
}
