// PRACH detection on gfx950: every occasion of a batch in one launch, one 256-thread workgroup per (occasion, root
// sequence), from the bf16 frequency-domain preamble symbols to the per-preamble decisions. float32 throughout.
//
// Reference (behaviour, not code): lib/phy/upper/channel_processors/prach_detector_generic_impl.cpp:80 (detect),
// :168-175 (RSSI), :186 (early stop), :223-302 (per port: combine, conjugate root, IDFT, modulus square, windows),
// :305-343 (per preamble: |den|, divide, peak, decision), prach_detector_generic_impl.h:76 (vector_noise_estimation).
//
// A workgroup first sums the occasion's power (every workgroup of the occasion does, so none waits for another), then,
// port by port: loads the symbols and sums them in symbol order, multiplies by the conjugate root sequence (a float2 row
// of the plan's root table), places the two halves at the ends of the zeroed IDFT input in LDS, runs a radix-4
// Stockham inverse transform of its own in LDS (5 passes for 1024 points, 4 for 256; prach_host.h:prach_stockham4,
// twiddles from an LDS copy of the plan's table), takes the scaled modulus square, and lets each wavefront walk its
// windows, 64 / group_lanes of them at a time (group_lanes = 64: wave w takes windows w, w + 4, ...; 8: eight windows
// per wave at once): the reference energy is a sum over the window and its margins with wrap, lane-strided within the
// group and reduced by __shfl_xor; numerator and denominator of a (window, sample) accumulate in LDS words only that
// group of lanes touches. After the last port the same lanes find the first largest sample of num / |den| and the
// group's first lane stores the preamble's slot. No atomics:
// sequence s owns the slots of its preambles, sequence 0 also the header.
#include "prach_host.h"
#include "signal_device.h"
#include "srsgpu_internal.h"

namespace srsgpu {
namespace {

constexpr uint32_t PRACH_THREADS = 256;
constexpr uint32_t PRACH_WAVES   = PRACH_THREADS / 64;

__device__ __forceinline__ void store_preamble(srsgpu_prach_result* __restrict__ out, uint32_t preamble, uint32_t detected,
                                               uint32_t delay, float metric, float peak)
{
  srsgpu_prach_preamble p;
  p.detected = detected, p.delay_samples = delay, p.metric = metric, p.peak = peak;
  out->preambles[preamble] = p;
}

/// One port's (or symbol's) share of every window of the sequence: groups of G lanes take one window each, a wavefront
/// 64 / G windows at a time. A (window, sample) word of num / den is only ever touched by one group of one wavefront.
template <uint32_t G>
__device__ __forceinline__ void accumulate_windows(const prach_job& job, const float* mod, float* num, float* den)
{
  constexpr uint32_t groups = 64u / G;
  const uint32_t     lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, group = lane / G, gl = lane & (G - 1u);
  const uint32_t     L = job.L, N = job.N, nof_shifts = job.nof_shifts, ww = job.win_width;
  for (uint32_t w0 = wave * groups; w0 < nof_shifts; w0 += PRACH_WAVES * groups) {
    const uint32_t w      = w0 + group;
    const bool     active = w < nof_shifts;
    const uint32_t start  = prach_window_start(N, L, job.n_cs, active ? w : 0u);
    const uint32_t from   = (start + N - job.win_margin) % N;
    const uint32_t len    = 2u * job.win_margin + ww;
    float          reference = 0.0F;
    if (active) {
      for (uint32_t i = gl; i < len; i += G) {
        const uint32_t at = from + i;
        reference += mod[at >= N ? at - N : at];
      }
    }
#pragma unroll
    for (uint32_t m = G >> 1; m >= 1u; m >>= 1) {
      reference += __shfl_xor(reference, static_cast<int>(m));
    }
    if (active) {
      for (uint32_t s = gl; s < ww; s += G) {
        const float v    = mod[start + s] * job.win_scale;
        float       diff = reference - v;
        if (!is_normal(diff)) {
          diff = 1e-9F;
        }
        num[w * ww + s] += v;
        den[w * ww + s] += diff;
      }
    }
  }
}

/// After the last port: num / |den|, the first strictly largest sample and the decision, by the lanes that accumulated.
template <uint32_t G>
__device__ __forceinline__ void decide_preambles(const prach_job& job, const float* num, const float* den,
                                                 srsgpu_prach_result* __restrict__ out)
{
  constexpr uint32_t groups = 64u / G;
  const uint32_t     lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, group = lane / G, gl = lane & (G - 1u);
  const uint32_t     nof_shifts = job.nof_shifts, ww = job.win_width, first_slot = job.sequence * nof_shifts;
  for (uint32_t w0 = wave * groups; w0 < nof_shifts; w0 += PRACH_WAVES * groups) {
    const uint32_t w = w0 + group, preamble = first_slot + w;
    const bool     active    = w < nof_shifts && preamble < PRACH_MAX_PREAMBLES;
    const bool     monitored = active && preamble >= job.first_preamble && preamble < job.end_preamble;
    float          peak  = -INFINITY;
    uint32_t       delay = 0;
    if (monitored) {
      for (uint32_t s = gl; s < ww; s += G) {
        const float m = num[w * ww + s] / fabsf(den[w * ww + s]);
        if (m > peak) {
          peak  = m;
          delay = s;
        }
      }
    }
#pragma unroll
    for (uint32_t m = G >> 1; m >= 1u; m >>= 1) {
      const float    other_peak  = __shfl_xor(peak, static_cast<int>(m));
      const uint32_t other_delay = __shfl_xor(delay, static_cast<int>(m));
      if (other_peak > peak || (other_peak == peak && other_delay < delay)) {
        peak  = other_peak;
        delay = other_delay;
      }
    }
    if (active && gl == 0u) {
      if (!(peak > -INFINITY)) {  // no sample compared greater: what max_element leaves
        peak  = 0.0F;
        delay = 0;
      }
      const bool detected = peak > job.threshold && delay < job.delay_end;
      if (monitored) {
        store_preamble(out, preamble, detected ? 1u : 0u, delay, peak / job.threshold, peak);
      } else {
        store_preamble(out, preamble, 0u, 0u, 0.0F, 0.0F);
      }
    }
  }
}

__global__ __launch_bounds__(PRACH_THREADS) void prach_detector_kernel(const prach_job* __restrict__ jobs,
                                                                        const cpx* __restrict__ roots,
                                                                        const cpx* __restrict__ twiddles,
                                                                        const uint32_t* __restrict__ input,
                                                                        srsgpu_prach_result* __restrict__ results)
{
  __shared__ cpx       buf[2][PRACH_LONG_N];
  __shared__ cpx       tw[PRACH_LONG_N];
  __shared__ float     mod[PRACH_LONG_N];
  __shared__ float     num[PRACH_LONG_N];
  __shared__ float     den[PRACH_LONG_N];
  __shared__ float     partial[PRACH_WAVES];
  __shared__ prach_job job;

  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  copy_words(&job, jobs + blockIdx.x, tid, PRACH_THREADS);
  for (uint32_t i = tid; i < PRACH_LONG_N; i += PRACH_THREADS) {
    tw[i] = twiddles[i];
  }
  __syncthreads();
  const uint32_t L = job.L, N = job.N, P = job.nof_ports, S = job.nof_symbols;
  const uint32_t nof_shifts = job.nof_shifts, ww = job.win_width;
  const uint32_t first_slot = job.sequence * nof_shifts;
  srsgpu_prach_result* __restrict__ out = results + job.result_index;

  // RSSI over every port and symbol of the occasion.
  float          power = 0.0F;
  const uint32_t per_port = S * L;
#pragma unroll 4
  for (uint32_t i = tid; i < P * per_port; i += PRACH_THREADS) {  // (several loads in flight per thread)
    const uint32_t p = i / per_port, r = i - p * per_port, s = r / L, n = r - s * L;
    power += norm2(bf16c(input[job.sample_offset + p * job.port_stride + s * job.symbol_stride + n]));
  }
  power = wave_sum(power);
  if (lane == 0u) {
    partial[wave] = power;
  }
  __syncthreads();
  const float rssi = ((partial[0] + partial[1]) + (partial[2] + partial[3])) / static_cast<float>(L) / job.rssi_scale;
  const bool  early = !is_normal(rssi);
  if (job.sequence == 0u && tid == 0u) {
    out->rssi        = rssi;
    out->early_stop  = early ? 1u : 0u;
    out->reserved[0] = out->reserved[1] = 0u;
  }
  // Nothing to detect: after the early stop, or when none of this sequence's preambles is monitored.
  const uint32_t end_slot = min(first_slot + nof_shifts, PRACH_MAX_PREAMBLES);
  if (early || first_slot >= job.end_preamble || end_slot <= job.first_preamble) {
    for (uint32_t slot = first_slot + tid; slot < end_slot; slot += PRACH_THREADS) {
      store_preamble(out, slot, 0u, 0u, 0.0F, 0.0F);
    }
    return;
  }

  for (uint32_t i = tid; i < nof_shifts * ww; i += PRACH_THREADS) {
    num[i] = 0.0F;
    den[i] = 0.0F;
  }
  const cpx* __restrict__ root = roots + job.root_row;
  const uint32_t half = L / 2u;  // the IDFT input: its first L / 2 + 1 bins are the last ones of the product, :251-252
  const uint32_t nof_rounds = job.combine_symbols != 0u ? 1u : S;
  for (uint32_t p = 0; p < P; ++p) {
    for (uint32_t round = 0; round < nof_rounds; ++round) {
      const uint32_t base = job.sample_offset + p * job.port_stride + round * job.symbol_stride;
      for (uint32_t t = tid; t < N; t += PRACH_THREADS) {
        cpx v = {0.0F, 0.0F};
        if (t <= half || t >= N - half) {
          const uint32_t n = t <= half ? half + t : t - (N - half);
          cpx            x = bf16c(input[base + n]);
          if (job.combine_symbols != 0u) {
#pragma unroll 4
            for (uint32_t s = 1; s < S; ++s) {
              const cpx y = bf16c(input[base + s * job.symbol_stride + n]);
              x.x += y.x;
              x.y += y.y;
            }
          }
          const cpx r = root[n];  // x conj(r) written out: through cmulc this product contracts into other FMAs
          v           = {x.x * r.x + x.y * r.y, x.y * r.x - x.x * r.y};
        }
        buf[0][t] = v;
      }
      __syncthreads();
      uint32_t src = 0;
      for (uint32_t ns = 1; ns < N; ns <<= 2) {
        for (uint32_t j = tid; j < (N >> 2); j += PRACH_THREADS) {
          prach_stockham4(buf[src], buf[src ^ 1u], tw, PRACH_LONG_N, N, ns, j);
        }
        __syncthreads();
        src ^= 1u;
      }
      for (uint32_t t = tid; t < N; t += PRACH_THREADS) {
        mod[t] = norm2(buf[src][t]) * job.mod_scale;
      }
      __syncthreads();
      switch (job.group_lanes) {
        case 8: accumulate_windows<8>(job, mod, num, den); break;
        case 16: accumulate_windows<16>(job, mod, num, den); break;
        case 32: accumulate_windows<32>(job, mod, num, den); break;
        default: accumulate_windows<64>(job, mod, num, den); break;
      }
      __syncthreads();
    }
  }

  // The lanes that accumulated a window also decide its preamble.
  switch (job.group_lanes) {
    case 8: decide_preambles<8>(job, num, den, out); break;
    case 16: decide_preambles<16>(job, num, den, out); break;
    case 32: decide_preambles<32>(job, num, den, out); break;
    default: decide_preambles<64>(job, num, den, out); break;
  }
}

} // namespace

void launch_prach_detector(const prach_job*     d_jobs,
                           uint32_t             nof_jobs,
                           const float*         d_roots,
                           const float*         d_twiddles,
                           const uint32_t*      d_input,
                           srsgpu_prach_result* d_results,
                           hipStream_t          stream)
{
  if (nof_jobs == 0) {
    return;
  }
  hipLaunchKernelGGL(prach_detector_kernel, dim3(nof_jobs), dim3(PRACH_THREADS), 0, stream, d_jobs,
                     reinterpret_cast<const cpx*>(d_roots), reinterpret_cast<const cpx*>(d_twiddles), d_input,
                     d_results);
}

} // namespace srsgpu
