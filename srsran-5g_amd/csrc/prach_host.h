// Host-side construction for the PRACH detector plan (capi_prach.cpp, prach_detector.hip): the format rows of TS 38.211
// Tables 6.3.3.1-1 / -2, everything detect() derives from them (cp_prach, the window width, the maximum delay, each
// window's start), the refusals, the Zadoff-Chu root sequences in the frequency domain and the IDFT twiddles. No HIP
// call in this translation unit, so that a host-only program can check it (tools/prach_host_check.cpp). The radix-4
// Stockham butterfly the kernel runs is defined here for both sides, so the same program checks it against a direct sum.
//
// Reference (behaviour, not code): lib/ran/prach/prach_preamble_information.cpp:30 / :46 (format rows),
// lib/phy/upper/channel_processors/prach_detector_generic_impl.cpp:104-160 (derived quantities) / :268 (window start) /
// :273-278 (reference interval), prach_generator_impl.cpp:97 / :212 (y_u, restated here as the DFT of x_u).
#pragma once
#include "cpx.h"
#include "srsgpu_phy.h"
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIP__)
#define SRSGPU_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SRSGPU_HD inline
#endif

namespace srsgpu {

constexpr uint32_t PRACH_LONG_L = 839, PRACH_SHORT_L = 139;
constexpr uint32_t PRACH_LONG_N = 1024, PRACH_SHORT_N = 256;  ///< The reference factory's IDFT sizes.
constexpr uint32_t PRACH_MAX_PREAMBLES = SRSGPU_PRACH_MAX_PREAMBLES;

/// What detect() computes with before it touches a sample.
struct prach_derived {
  uint32_t L;                  ///< L_RA.
  uint32_t N;                  ///< IDFT size.
  uint32_t nof_symbols;
  double   scs_hz;             ///< The preamble's subcarrier spacing.
  uint32_t cp_kappa;           ///< N_CP^RA in units of kappa (64 T_c), shifted by the numerology for the short formats.
  uint32_t cp_prach;           ///< floor(CP duration x L x scs).
  uint32_t nof_shifts;         ///< Preambles per root sequence.
  uint32_t nof_sequences;
  uint32_t win_width;
  uint32_t max_delay_samples;
  uint32_t delay_end;          ///< A delay is accepted while delay < 0.8 max_delay_samples, i.e. delay < delay_end.
};

/// The format row and what follows from N_cs; false for a format / SCS pair the reference's info functions do not define.
bool prach_derive(uint32_t format, uint32_t ra_scs, uint32_t n_cs, prach_derived& d);

/// (N - (N_cs w N) / L) mod N (prach_detector_generic_impl.cpp:268).
SRSGPU_HD uint32_t prach_window_start(uint32_t N, uint32_t L, uint32_t n_cs, uint32_t window)
{
  return (N - (n_cs * window * N) / L) % N;
}

/// One workgroup's work: one root sequence of one occasion. Plain data, uploaded as it is.
struct prach_job {
  uint32_t sample_offset, port_stride, symbol_stride;
  uint32_t root_row;            ///< Float2 element of the root sequence's first value in the root table.
  uint32_t result_index;
  uint32_t sequence;            ///< i_sequence.
  uint32_t L, N, nof_ports, nof_symbols, combine_symbols;
  uint32_t n_cs, nof_shifts, win_width, win_margin, delay_end;
  uint32_t first_preamble, end_preamble;  ///< Monitored preambles, all sequences.
  uint32_t group_lanes;         ///< Lanes of a wavefront that share one window: a power of two, 8..64.
  float    threshold;
  float    mod_scale;           ///< 1.0F / float(N L L).
  float    win_scale;           ///< float(N) / float(L).
  float    rssi_scale;          ///< float(ports x symbols x L).
};

/// The one reason the occasion is refused; empty when it is accepted (then d holds its derived quantities).
std::string prach_refusal(const srsgpu_prach_occasion& o, const uint16_t* roots, uint32_t total_roots, uint64_t input_words,
                          uint32_t nof_occasions, prach_derived& d);

/// The jobs of an accepted occasion, one per root sequence; root_rows[i] is the table row of its i-th root.
void prach_jobs(const srsgpu_prach_occasion& o, const prach_derived& d, const std::vector<uint32_t>& root_rows,
                std::vector<prach_job>& jobs);

/// y_u(n), n = 0..L-1, as (re, im) floats: the L-point DFT of x_u(i) = exp(-j pi u i (i + 1) / L), amplitude sqrt(L),
/// evaluated in double in closed form: y_u(n) = x_u*(u^-1 n) y_u(0), y_u(0) the direct sum.
std::vector<float> prach_root_sequence(uint32_t L, uint32_t u);

/// Butterfly j (0..N/4-1) of the radix-4 Stockham pass with sub-transform length ns (1, 4, 16, ...) of an inverse
/// (exp(+j)) N-point transform: in -> out. tw is unit_roots(tw_n) of host_util.h, tw_n a multiple of N. The arithmetic is
/// written out: it compiles for the host too, where signal_device.h's helpers do not exist.
SRSGPU_HD void prach_stockham4(const cpx* in, cpx* out, const cpx* tw, uint32_t tw_n, uint32_t N, uint32_t ns,
                               uint32_t j)
{
  const uint32_t q = N >> 2, k = j & (ns - 1u), step = tw_n / (ns << 2);
  cpx            v[4];
#pragma unroll
  for (uint32_t r = 0; r < 4u; ++r) {
    const cpx x = in[j + r * q], w = tw[r * k * step];
    v[r]        = {x.x * w.x - x.y * w.y, x.x * w.y + x.y * w.x};
  }
  const cpx      s02 = {v[0].x + v[2].x, v[0].y + v[2].y}, d02 = {v[0].x - v[2].x, v[0].y - v[2].y};
  const cpx      s13 = {v[1].x + v[3].x, v[1].y + v[3].y}, d13 = {v[1].x - v[3].x, v[1].y - v[3].y};
  const uint32_t at = ((j - k) << 2) + k;
  out[at]           = {s02.x + s13.x, s02.y + s13.y};
  out[at + ns]      = {d02.x - d13.y, d02.y + d13.x};  // + j d13
  out[at + 2u * ns] = {s02.x - s13.x, s02.y - s13.y};
  out[at + 3u * ns] = {d02.x + d13.y, d02.y - d13.x};  // - j d13
}

} // namespace srsgpu
