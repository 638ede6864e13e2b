// The low-PAPR base sequence of TS 38.211 section 5.2.2 for host code: the PUSCH estimator's transform-precoded DM-RS
// (capi_pusch_chest.cpp), the SRS estimator's sequences (srs_host.cpp) and the PUCCH Format 3 / 4 DM-RS
// (pucch_f34_host.cpp). No HIP call and no HIP type, so that a host-only program can use it.
//
// Reference (behaviour, not code): lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.cpp:176 / :194.
#pragma once
#include "low_papr_tables.h"
#include <cmath>
#include <cstdint>
#include <vector>

namespace srsgpu {

/// The phase of the base sequence of group u (v = 0, alpha = 0) and length m as integers arg[n] in units of pi / nzc, as
/// low_papr_sequence_generator_impl.cpp builds it: the phase tables for m = 6..24 (nzc = 4), the length-30 formula, and
/// Zadoff-Chu of the largest prime N_ZC < m for m >= 36 with q = (int)(q_hat + 0.5), q_hat = (float) N_ZC (u + 1) / 31.
/// Returns false for a length the specification does not define.
inline bool low_papr_argument(unsigned u, unsigned m, std::vector<int>& arg, unsigned& nzc)
{
  arg.assign(m, 0);
  nzc               = 4;
  const int8_t* phi = m == 6 ? kLowPaprPhi6[u] : m == 12 ? kLowPaprPhi12[u] : m == 18 ? kLowPaprPhi18[u]
                                                                  : m == 24 ? kLowPaprPhi24[u] : nullptr;
  if (phi != nullptr) {
    for (unsigned n = 0; n < m; ++n) {
      arg[n] = phi[n];  // units of pi / 4 = pi / N_ZC with N_ZC = 4
    }
  } else if (m == 30) {
    nzc = 31;
    for (unsigned n = 0; n < m; ++n) {
      arg[n] = -static_cast<int>(((u + 1ull) * (n + 1ull) * (n + 2ull)) % 62u);
    }
  } else if (m >= 36) {
    nzc = m - 1;
    auto prime = [](unsigned x) {
      for (unsigned d = 2; d * d <= x; ++d) {
        if (x % d == 0) {
          return false;
        }
      }
      return x > 1;
    };
    while (!prime(nzc)) {
      --nzc;
    }
    const float   q_hat = static_cast<float>(nzc) * static_cast<float>(u + 1) / 31.f;
    const int64_t q     = static_cast<int64_t>(static_cast<float>(static_cast<double>(q_hat) + 0.5));
    for (unsigned n = 0; n < m; ++n) {
      const int64_t mm = n % nzc;
      arg[n]           = -static_cast<int>((q * mm * (mm + 1)) % (2 * nzc));
    }
  } else {
    return false;
  }
  return true;
}

/// The sequence itself, appended to out as pairs of floats (C: float2 or cpx), each value evaluated in double.
template <typename C>
inline bool low_papr_sequence(unsigned u, unsigned m, std::vector<C>& out)
{
  std::vector<int> arg;
  unsigned         nzc = 4;
  if (!low_papr_argument(u, m, arg, nzc)) {
    return false;
  }
  for (unsigned n = 0; n < m; ++n) {
    const double a = 3.14159265358979323846 * static_cast<double>(arg[n]) / static_cast<double>(nzc);
    C            v;
    v.x = static_cast<float>(std::cos(a));
    v.y = static_cast<float>(std::sin(a));
    out.push_back(v);
  }
  return true;
}

/// The sequence with a cyclic shift, r(n) e^{j 2 pi step n / 24}, n = 0..m-1, as (re, im) floats evaluated in double: the
/// shift in 24ths of a turn, the resolution of the reference's table (low_papr_sequence_generator_impl.cpp:243). Empty
/// for a length the specification does not define.
inline std::vector<float> low_papr_shifted_sequence(unsigned u, unsigned m, uint64_t step)
{
  std::vector<int>   arg;
  unsigned           nzc = 4;
  std::vector<float> out;
  if (!low_papr_argument(u, m, arg, nzc)) {
    return out;
  }
  out.reserve(2 * static_cast<size_t>(m));
  for (unsigned n = 0; n < m; ++n) {
    const double a = 3.14159265358979323846 * static_cast<double>(arg[n]) / static_cast<double>(nzc) +
                     2.0 * 3.14159265358979323846 * static_cast<double>((n * step) % 24u) / 24.0;
    out.push_back(static_cast<float>(std::cos(a)));
    out.push_back(static_cast<float>(std::sin(a)));
  }
  return out;
}

} // namespace srsgpu
