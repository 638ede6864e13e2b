// The prototype of the estimators' frequency-domain smoothing filter, shared by the PUSCH DM-RS estimator plan
// (capi_pusch_chest.cpp) and the PUCCH Format 2 plan (pucch_f2_host.cpp). Host only, no HIP call.
#pragma once
#include <cmath>

namespace srsgpu {

/// Raised cosine, roll-off 0.2, 10 samples per symbol, n = 0..30 (t = (n - 15) / 10), as the reference tabulates it
/// (port_channel_estimator_helpers.cpp:51 RC_FILTER): normalised to unit energy and quantised to 7 decimals, so that
/// the float taps the estimator derives from it are the reference's bit for bit. The reference's table holds
/// 0.3235207 at n = 14 and 16, one unit of the last decimal below the rounded prototype value (0.32352076).
inline double rc_tap(int n)
{
  const double pi   = 3.14159265358979323846;
  const double beta = 0.2;
  auto         raw  = [&](int i) {
    const double t    = (i - 15) / 10.0;
    const double sinc = (t == 0) ? 1.0 : std::sin(pi * t) / (pi * t);
    return sinc * std::cos(pi * beta * t) / (1 - (2 * beta * t) * (2 * beta * t));  // |2 beta t| < 1 for i = 0..30
  };
  double energy = 0;
  for (int i = 0; i != 31; ++i) {
    energy += raw(i) * raw(i);
  }
  double q = std::nearbyint(raw(n) / std::sqrt(energy) * 1e7);
  if (n == 14 || n == 16) {
    q -= 1;
  }
  return q / 1e7;
}

} // namespace srsgpu
