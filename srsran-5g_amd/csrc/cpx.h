// The complex value of the signal kernels, for host and device code alike (prach_host.h's butterfly compiles for both).
#pragma once

namespace srsgpu {

/// A plain pair of floats with 4-byte alignment. Not float2: its 8-byte alignment turns the kernels' LDS accesses into
/// 8-byte ones (ofdm.hip, which wants exactly that, keeps float2).
struct cpx {
  float x, y;
};

} // namespace srsgpu
