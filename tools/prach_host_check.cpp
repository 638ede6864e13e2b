// Stand-alone check of srsran-5g_amd/csrc/prach_host.cpp (no HIP, no GPU), built by tests/test_prach_oracle.py with the
// address and undefined-behaviour sanitizers and run as a child process.
//
//   prach_host_check DUMP    DUMP (written by the test from the float64 restatement tests/prach_cases.py):
//                            u32 n; n x 15 u32 (format, ra_scs, n_cs, defined, L, N, nof_symbols, cp_prach, nof_shifts,
//                            nof_sequences, win_width, max_delay, delay_end, start of window 1, start of the last window);
//                            u32 m; m x (u32 L, u32 u, 2 L f64: y_u as (re, im)).
// Checks prach_derive and prach_window_start against the dump, prach_root_sequence against the dump and against a
// direct sum, the radix-4 Stockham passes (prach_stockham4, the code the kernel runs) against a direct sum for 1024 and
// 256 points, the job descriptors and every refusal.
#include "host_util.h"
#include "prach_host.h"
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

void check_stockham(uint32_t N)
{
  const std::vector<float> twf = unit_roots(PRACH_LONG_N);
  std::vector<cpx>         tw(PRACH_LONG_N), a(N), b(N);
  std::memcpy(static_cast<void*>(tw.data()), twf.data(), twf.size() * sizeof(float));
  uint32_t state = 12345u + N;
  for (cpx& v : a) {
    state = state * 1664525u + 1013904223u;
    v.x   = static_cast<float>(static_cast<int32_t>(state >> 8) % 2001 - 1000) / 1000.0F;
    state = state * 1664525u + 1013904223u;
    v.y   = static_cast<float>(static_cast<int32_t>(state >> 8) % 2001 - 1000) / 1000.0F;
  }
  const std::vector<cpx> x = a;
  cpx *src = a.data(), *dst = b.data();
  for (uint32_t ns = 1; ns < N; ns <<= 2) {
    for (uint32_t j = 0; j < N / 4; ++j) {
      prach_stockham4(src, dst, tw.data(), PRACH_LONG_N, N, ns, j);
    }
    std::swap(src, dst);
  }
  double worst = 0.0, largest = 0.0;
  for (uint32_t m = 0; m < N; ++m) {
    double re = 0.0, im = 0.0;
    for (uint32_t f = 0; f < N; ++f) {
      const double ang = 2.0 * 3.14159265358979323846 * static_cast<double>((static_cast<uint64_t>(f) * m) % N) / N;
      re += x[f].x * std::cos(ang) - x[f].y * std::sin(ang);
      im += x[f].x * std::sin(ang) + x[f].y * std::cos(ang);
    }
    worst   = std::max(worst, std::hypot(src[m].x - re, src[m].y - im));
    largest = std::max(largest, std::hypot(re, im));
  }
  CHECK(worst < 1e-5 * largest, "%u-point inverse transform deviates by %g of %g", N, worst, largest);
}

srsgpu_prach_occasion good_occasion()
{
  srsgpu_prach_occasion o = {};
  o.format = SRSGPU_PRACH_FORMAT_0, o.ra_scs = SRSGPU_PRACH_SCS_1_25, o.nof_rx_ports = 2, o.combine_symbols = 1;
  o.n_cs = 46, o.nof_roots = 4, o.root_offset = 1, o.start_preamble_index = 5, o.nof_preamble_indices = 20;
  o.win_margin = 5, o.threshold = 0.25F, o.sample_offset = 3, o.port_stride = 900, o.symbol_stride = 839, o.result_index = 1;
  return o;
}

void check_refusals()
{
  const uint16_t roots[5] = {1, 129, 710, 140, 838};
  prach_derived  d;
  const uint64_t words = 3 + 900 + 839;
  CHECK(prach_refusal(good_occasion(), roots, 5, words, 2, d).empty(), "%s", prach_refusal(good_occasion(), roots, 5, words, 2, d).c_str());
  CHECK(d.L == 839 && d.N == 1024 && d.nof_shifts == 18 && d.nof_sequences == 4, "derived");
  auto refused = [&](const char* what, srsgpu_prach_occasion o, const uint16_t* r = nullptr, uint32_t nr = 5, uint64_t w = 0,
                     uint32_t nof = 2) {
    const std::string why = prach_refusal(o, r ? r : roots, nr, w ? w : words, nof, d);
    CHECK(!why.empty(), "%s is accepted", what);
  };
  srsgpu_prach_occasion o;
  o = good_occasion(), o.nof_preamble_indices = 0, refused("no preamble", o);
  o = good_occasion(), o.start_preamble_index = 50, refused("preambles past 64", o);
  o = good_occasion(), o.nof_rx_ports = 0, refused("no port", o);
  o = good_occasion(), o.nof_rx_ports = 5, refused("five ports", o);
  o = good_occasion(), o.combine_symbols = 2, refused("combine_symbols 2", o);
  o = good_occasion(), o.format = 14, refused("format 14", o);
  o = good_occasion(), o.ra_scs = SRSGPU_PRACH_SCS_15, refused("Format 0 at 15 kHz", o);
  o = good_occasion(), o.format = SRSGPU_PRACH_FORMAT_3, refused("Format 3 at 1.25 kHz", o);
  o = good_occasion(), o.format = SRSGPU_PRACH_FORMAT_B4, refused("B4 at 1.25 kHz", o);
  o = good_occasion(), o.ra_scs = 6, refused("SCS 6", o);
  o = good_occasion(), o.n_cs = 840, o.nof_roots = 64, refused("N_cs above L", o);
  o = good_occasion(), o.nof_roots = 3, refused("too few roots", o);
  o = good_occasion(), o.nof_roots = 5, refused("too many roots", o);
  o = good_occasion(), o.root_offset = 2, refused("roots past the array", o);
  const uint16_t zero_root[5] = {1, 129, 0, 140, 838}, big_root[5] = {1, 129, 839, 140, 838};
  refused("root 0", good_occasion(), zero_root);
  refused("root L", good_occasion(), big_root);
  o = good_occasion(), o.threshold = 0.0F, refused("threshold 0", o);
  o = good_occasion(), o.threshold = -1.0F, refused("negative threshold", o);
  o = good_occasion(), o.threshold = std::nanf(""), refused("NaN threshold", o);
  o = good_occasion(), o.win_margin = 0, refused("margin 0", o);
  o = good_occasion(), o.win_margin = 490, refused("window longer than the IDFT", o);
  refused("samples past the input", good_occasion(), nullptr, 5, words - 1);
  o = good_occasion(), o.symbol_stride = 0xffffffffu, o.format = SRSGPU_PRACH_FORMAT_2, refused("samples past 2^32", o, nullptr, 5, ~0ull);
  o = good_occasion(), o.result_index = 2, refused("result past the occasions", o);

  std::vector<prach_job> jobs;
  prach_refusal(good_occasion(), roots, 5, words, 2, d);
  prach_jobs(good_occasion(), d, {10, 20, 30, 40}, jobs);
  CHECK(jobs.size() == 4 && jobs[3].sequence == 3 && jobs[3].root_row == 40 && jobs[0].first_preamble == 5 && jobs[0].end_preamble == 25,
        "jobs");
  CHECK(jobs[0].group_lanes == 8, "18 windows: %u lanes per window", jobs[0].group_lanes);
  srsgpu_prach_occasion wide = good_occasion();
  wide.n_cs = 0, wide.nof_roots = 64;
  const std::vector<uint16_t> many(65, 7);
  CHECK(prach_refusal(wide, many.data(), 65, words, 2, d).empty(), "N_cs 0");
  jobs.clear();
  prach_jobs(wide, d, std::vector<uint32_t>(64, 0), jobs);
  CHECK(jobs.size() == 64 && jobs[63].group_lanes == 64 && jobs[63].nof_shifts == 1, "one window: a whole wave");
  CHECK(jobs[1].mod_scale == 1.0F / static_cast<float>(1024u * 839u * 839u) && jobs[1].rssi_scale == 2.0F * 839.0F, "scales");
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
    uint32_t v[15];
    for (uint32_t& x : v) {
      x = take<uint32_t>(raw, pos);
    }
    prach_derived d;
    const bool    defined = prach_derive(v[0], v[1], v[2], d);
    CHECK(defined == (v[3] != 0), "format %u scs %u", v[0], v[1]);
    if (!defined || v[3] == 0) {
      continue;
    }
    CHECK(d.L == v[4] && d.N == v[5] && d.nof_symbols == v[6] && d.cp_prach == v[7] && d.nof_shifts == v[8] &&
              d.nof_sequences == v[9] && d.win_width == v[10] && d.max_delay_samples == v[11] && d.delay_end == v[12],
          "format %u scs %u N_cs %u: %u %u %u %u %u %u %u %u %u", v[0], v[1], v[2], d.L, d.N, d.nof_symbols, d.cp_prach, d.nof_shifts,
          d.nof_sequences, d.win_width, d.max_delay_samples, d.delay_end);
    CHECK(prach_window_start(d.N, d.L, v[2], 0) == 0 && prach_window_start(d.N, d.L, v[2], d.nof_shifts > 1 ? 1 : 0) == v[13] &&
              prach_window_start(d.N, d.L, v[2], d.nof_shifts - 1) == v[14],
          "window starts of format %u N_cs %u", v[0], v[2]);
  }
  const uint32_t m = take<uint32_t>(raw, pos);
  for (uint32_t i = 0; i < m; ++i) {
    const uint32_t           L = take<uint32_t>(raw, pos), u = take<uint32_t>(raw, pos);
    const std::vector<float> y = prach_root_sequence(L, u);
    CHECK(y.size() == 2u * L, "size");
    double worst = 0.0, worst_direct = 0.0;
    for (uint32_t k = 0; k < L; ++k) {
      const double re = take<double>(raw, pos), im = take<double>(raw, pos);
      worst           = std::max(worst, std::hypot(y[2 * k] - re, y[2 * k + 1] - im));
      if (k % 97 == 0) {  // the definition itself, as a direct sum
        double sr = 0.0, si = 0.0;
        for (uint32_t t = 0; t < L; ++t) {
          const uint64_t p   = (static_cast<uint64_t>(u) * t * (t + 1) + 2ull * k * t) % (2ull * L);
          const double   ang = -3.14159265358979323846 * static_cast<double>(p) / L;
          sr += std::cos(ang), si += std::sin(ang);
        }
        worst_direct = std::max(worst_direct, std::hypot(y[2 * k] - sr, y[2 * k + 1] - si));
      }
    }
    CHECK(worst < 1e-5 && worst_direct < 1e-5, "y_%u of length %u deviates by %g / %g", u, L, worst, worst_direct);
  }
  CHECK(pos == raw.size(), "dump has %zu bytes left", raw.size() - pos);
  check_stockham(PRACH_LONG_N);
  check_stockham(PRACH_SHORT_N);
  const std::vector<float> tw = unit_roots(8);
  CHECK(tw.size() == 16 && tw[0] == 1.0F && std::fabs(tw[5] - 1.0F) < 1e-7F && std::fabs(tw[8] + 1.0F) < 1e-7F, "twiddles");
  check_refusals();
  std::printf("%u derived rows, %u root sequences, %d failures\n", n, m, failures);
  return failures == 0 ? 0 : 1;
}
