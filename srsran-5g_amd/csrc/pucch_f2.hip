// PUCCH Format 2 front end on gfx950: every PDU of a batch in one launch, one 256-thread workgroup per PDU, from the
// bf16 grid words to the descrambled int8 LLRs and the per-port channel state. float32 from the grid words; double only
// for the time alignment scalars. No atomics, no scratch, nothing kept in HBM between the stages.
//
// Reference (behaviour, not code): lib/phy/upper/signal_processors/pucch/dmrs_pucch_estimator_format2.cpp:87,
// lib/phy/upper/signal_processors/port_channel_estimator_average_impl.cpp:77 (hop loop, normalisation, noise floor) /
// :154 (one hop) / :322 (LSE and CFO) / :422 (noise), port_channel_estimator_helpers.cpp:203 (filter smoothing) / :307
// (virtual pilots), lib/srsvec/unwrap.cpp:40, lib/phy/support/interpolator/interpolator_linear_impl.cpp:29,
// lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.cpp:174 / :245 / :51,
// lib/phy/upper/channel_processors/pucch/pucch_demodulator_format2.cpp:92 / :162, equalization/equalize_zf_1xn.h:128,
// channel_modulation/demodulation_mapper_qpsk.cpp:45.
//
// Mapping. Estimation: wave w is receive port w, lane is pilot (16 PRB x 4 pilots = 64 = one wave), so every sum over a
// port's pilots is a wave reduction; the virtual pilots, the FIR, the interpolation and the time alignment exchange
// pilots through the wave's own LDS rows. The loops are uniform over the workgroup (the hop and symbol counts belong to
// the PDU), so the rows are ordered with plain workgroup barriers, a handful per hop. The time alignment needs 30 bins
// of the 128-point inverse transform (13 searched on either side plus two for the 5-point fit): lane b sums its bin
// directly with twiddles from a table, and no transform runs. Equalisation: after the last barrier thread t takes data
// RE t (at most 16 x 8 x 2 = 256), symbol-major as get_data_re_ests orders them.
//
// As in the reference, the data REs of receive port i come from grid port i, the pilots from grid port ports[i]
// (pucch_demodulator_format2.cpp:185 against port_channel_estimator_helpers.cpp:182), and the estimates the equaliser
// reads are bf16 (channel_estimate holds cbf16_t).
#include "pucch_f2_host.h"
#include "signal_device.h"
#include "srsgpu_internal.h"

// Every product and sum rounds on its own, as the float32 restatement of this sequence does (tests/pucch_f2_cases.py).
#pragma clang fp contract(off)

namespace srsgpu {
namespace {

constexpr uint32_t F2_THREADS = 256;
constexpr uint32_t F2_PILOTS  = 4 * PUCCH_F2_MAX_PRB;              // 64
constexpr uint32_t F2_ROW     = F2_PILOTS + 2 * PUCCH_F2_MAX_V;    // pilots with the virtual ones on either side
constexpr uint32_t F2_RES     = 12 * PUCCH_F2_MAX_PRB;             // 192
constexpr int      F2_M       = static_cast<int>(PUCCH_F2_TA_SAMPLES);
constexpr int      F2_SIDE    = F2_M + 2;                          // bins kept on either side
constexpr float    F2_PI      = 3.14159265358979323846F;
constexpr float    F2_TWOPI   = 6.28318530717958647692F;           // the reference's float TWOPI
constexpr double   F2_T_C     = 1.0 / (480000.0 * 4096.0);

/// Bin n of the correlation (n taken modulo 128) in the wave's row of 2 F2_SIDE kept bins.
__device__ __forceinline__ float corr_at(const float* row, int n)
{
  n &= static_cast<int>(PUCCH_F2_DFT) - 1;
  return row[n < F2_SIDE ? n : n - (static_cast<int>(PUCCH_F2_DFT) - 2 * F2_SIDE)];
}

/// ZF 1 x N as the chunked PUSCH kernel's one-layer path (pusch_demodulator.hip equalize_zf1): ports with an abnormal
/// channel or noise variance are skipped, nvar = sum |h|^2 nv / (sum |h|^2)^2.
__device__ __forceinline__ void equalize_zf1(const cpx* y, const cpx* h, uint32_t P, const float* nv, cpx& eq, float& var)
{
  float ch_mod_sq = 0.f, nvar_acc = 0.f;
  cpx   acc       = {0.f, 0.f};
#pragma unroll
  for (uint32_t p = 0; p < PUCCH_F2_MAX_PORTS; ++p) {
    if (p < P) {
      const float norm = norm2(h[p]);
      if (is_normal(norm) && is_normal(nv[p]) && nv[p] > 0.f) {
        ch_mod_sq += norm;
        nvar_acc += norm * nv[p];
        const cpx z = cmulc(y[p], h[p]);
        acc         = {acc.x + z.x, acc.y + z.y};
      }
    }
  }
  if (is_normal(ch_mod_sq) && is_normal(nvar_acc)) {
    const float rcp = 1.f / ch_mod_sq;
    eq              = {acc.x * rcp, acc.y * rcp};
    var             = nvar_acc * rcp * rcp;
  } else {
    eq  = {0.f, 0.f};
    var = __builtin_inff();
  }
}

/// QPSK soft bit: 2 sqrt(2) x / nvar scaled by 120 / 24, clipped to +-120, rounded half to even.
__device__ __forceinline__ int demap_qpsk(float x, float rcp)
{
  const float g = 2.0f * 1.41421356f;
  float       v = ((g * x) * rcp) * (120.f / 24.f);
  v             = fminf(fmaxf(v, -120.f), 120.f);
  return static_cast<int>(__builtin_rintf(v));
}

__global__ __launch_bounds__(F2_THREADS) void pucch_f2_kernel(const pucch_f2_job* __restrict__ jobs,
                                                              const cpx* __restrict__ dmrs,
                                                              const uint32_t* __restrict__ scrambling,
                                                              const cpx* __restrict__ twiddles,
                                                              const uint32_t* __restrict__ grids,
                                                              int8_t* __restrict__ llrs,
                                                              srsgpu_pucch_f2_result* __restrict__ results)
{
  __shared__ pucch_f2_job           job;
  __shared__ cpx                    enl[PUCCH_F2_MAX_PORTS][F2_ROW];
  __shared__ cpx                    smooth[PUCCH_F2_MAX_PORTS][F2_PILOTS];
  __shared__ uint32_t               est[PUCCH_F2_MAX_PORTS][PUCCH_F2_MAX_SYMBOLS][F2_RES];
  __shared__ cpx                    tw[PUCCH_F2_DFT];
  __shared__ float                  corr[PUCCH_F2_MAX_PORTS][2 * F2_SIDE];
  __shared__ float                  port_nv[PUCCH_F2_MAX_PORTS];
  __shared__ srsgpu_pucch_f2_result res;

  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  copy_words(&job, jobs + blockIdx.x, tid, F2_THREADS);
  if (tid < PUCCH_F2_DFT) {
    tw[tid] = twiddles[tid];
  }
  for (uint32_t i = tid; i < sizeof(res) / 4u; i += F2_THREADS) {
    reinterpret_cast<uint32_t*>(&res)[i] = 0u;
  }
  __syncthreads();

  const uint32_t N = 4u * job.nof_prb, P = job.nof_ports, nsym = job.nof_symbols, nsc = job.nsc;
  const uint32_t nof_hops = job.hopping != 0u ? 2u : 1u, per_hop = job.hopping != 0u ? 1u : nsym;
  const uint32_t nv = job.n_v, ntaps = job.nof_taps, half = ntaps / 2u;
  const bool     port_on = w < P, on = port_on && lane < N;
  const uint32_t base    = job.grid_base + job.ports[port_on ? w : 0u] * job.port_stride + job.start_symbol * nsc;

  float rsrp = 0.f, epre = 0.f, noise = 0.f, ta = 0.f, cfo_hz = __builtin_nanf("");
  for (uint32_t hop = 0; hop < nof_hops; ++hop) {
    const uint32_t prb = job.prb[hop];  // (one hop: symbol 0's PRB serves both symbols)
    cpx            rx[2] = {{0.f, 0.f}, {0.f, 0.f}}, pil[2] = {{0.f, 0.f}, {0.f, 0.f}}, lse[2];
#pragma unroll
    for (uint32_t s = 0; s < 2u; ++s) {
      if (s < per_hop && on) {
        const uint32_t sym = hop + s;
        rx[s]              = bf16c(grids[base + sym * nsc + 12u * prb + 1u + 3u * lane]);
        pil[s]             = dmrs[job.dmrs_row[sym] + lane];
      }
      lse[s] = cmulc(rx[s], pil[s]);
    }
    cpx f = lse[0];
    if (per_hop == 2u) {
      // CFO: the phase of sum lse_1 conj(lse_0) over the epochs' distance; reported, never compensated.
      const cpx   z  = cmulc(lse[1], lse[0]);
      const float ph = atan2f(wave_sum(z.y), wave_sum(z.x));
      cfo_hz         = ph / F2_TWOPI / job.delta_epoch * job.scs_hz;
      f              = {(lse[0].x + lse[1].x) * 0.5f, (lse[0].y + lse[1].y) * 0.5f};
    }
    if (on) {
      enl[w][PUCCH_F2_MAX_V + lane] = f;
    }
    __syncthreads();
    // Virtual pilots: lanes 0..nv-1 those before the band, lanes nv..2 nv-1 those after it, each from the regression of
    // the modulus and of the unwrapped argument over the nv pilots next to it.
    if (port_on && lane < 2u * nv) {
      const bool     is_end = lane >= nv;
      const uint32_t i      = is_end ? lane - nv : lane;
      const cpx*     bp     = &enl[w][PUCCH_F2_MAX_V + (is_end ? N - nv : 0u)];
      float          sum_ab = 0.f, dot_ab = 0.f, sum_ar = 0.f, dot_ar = 0.f, k = 0.f, prev = 0.f;
      for (uint32_t j = 0; j < nv; ++j) {
        const cpx   p  = bp[j];
        const float ab = sqrtf(norm2(p)), ar = atan2f(p.y, p.x);
        if (j > 0u && fabsf(ar - prev) > F2_PI) {
          k -= copysignf(1.0f, ar - prev);
        }
        prev            = ar;
        const float aru = ar + 2.0f * k * F2_PI;
        sum_ab += ab;
        dot_ab += ab * static_cast<float>(j);
        sum_ar += aru;
        dot_ar += aru * static_cast<float>(j);
      }
      const float fn = static_cast<float>(nv), mean_x = static_cast<float>(nv * (nv - 1u)) / 2.0f / fn;
      const float den      = static_cast<float>((nv - 1u) * nv * (2u * nv - 1u)) / 6.0f - fn * mean_x * mean_x;
      const float mean_ab  = sum_ab / fn, mean_ar = sum_ar / fn;
      const float slope_ab = (dot_ab - mean_x * mean_ab * fn) / den, slope_ar = (dot_ar - mean_x * mean_ar * fn) / den;
      const float xv       = static_cast<float>(static_cast<int>(i) + (is_end ? static_cast<int>(nv) : -static_cast<int>(nv)));
      const float rho      = slope_ab * xv + (mean_ab - slope_ab * mean_x);
      const float arg      = slope_ar * xv + (mean_ar - slope_ar * mean_x) + (rho > 0.f ? 0.f : F2_PI);
      float       sn, cs;
      sincosf(arg, &sn, &cs);
      enl[w][is_end ? PUCCH_F2_MAX_V + N + i : PUCCH_F2_MAX_V - nv + i] = {fabsf(rho) * cs, fabsf(rho) * sn};
    }
    __syncthreads();
    // The resampled raised cosine over the enlarged row ("same" convolution; half <= nv, so no tap leaves the row).
    cpx g = {0.f, 0.f};
    if (on) {
      for (uint32_t t = 0; t < ntaps; ++t) {
        const cpx p = enl[w][PUCCH_F2_MAX_V + lane + t - half];
        g.x += job.taps[t] * p.x;
        g.y += job.taps[t] * p.y;
      }
      smooth[w][lane] = g;
    }
    float e = 0.f, nz = 0.f;
#pragma unroll
    for (uint32_t s = 0; s < 2u; ++s) {
      if (s < per_hop) {
        const cpx pred = cmul(g, pil[s]);
        e += norm2(rx[s]);
        nz += norm2(cpx{rx[s].x - pred.x, rx[s].y - pred.y});
      }
    }
    rsrp += wave_sum(norm2(g)) * static_cast<float>(per_hop);
    epre += wave_sum(e);
    noise += wave_sum(nz);
    __syncthreads();
    // The 30 bins of the 128-point inverse transform that the search and the 5-point fit read, one lane each.
    if (port_on && lane < 2u * F2_SIDE) {
      const uint32_t n = lane < static_cast<uint32_t>(F2_SIDE) ? lane : PUCCH_F2_DFT - 2u * F2_SIDE + lane;
      cpx            v = {0.f, 0.f};
      for (uint32_t k = 0; k < N; ++k) {
        const cpx z = cmul(smooth[w][k], tw[(k * n) & (PUCCH_F2_DFT - 1u)]);
        v           = {v.x + z.x, v.y + z.y};
      }
      corr[w][lane] = norm2(v);
    }
    // Linear interpolation (offset 1, stride 3, ends held), rounded to bf16 as the estimates the demodulator reads.
    if (port_on) {
      for (uint32_t k = lane; k < 12u * job.nof_prb; k += 64u) {
        cpx v;
        if (k < 1u) {
          v = smooth[w][0];
        } else {
          const uint32_t j = (k - 1u) / 3u, r = (k - 1u) % 3u;
          if (j >= N - 1u) {
            v = smooth[w][N - 1u];
          } else {
            const cpx   a = smooth[w][j], b = smooth[w][j + 1u];
            const float q = static_cast<float>(r) / 3.0f;
            v             = {a.x + (b.x - a.x) * q, a.y + (b.y - a.y) * q};
          }
        }
        const uint32_t word = to_bf16c(v);
        for (uint32_t s = 0; s < per_hop; ++s) {
          est[w][hop + s][k] = word;
        }
      }
    }
    __syncthreads();
    // Peak within +-13 taps (the delayed half wins a tie) and its 5-point refinement; every lane of the wave alike.
    if (port_on) {
      const float* row = corr[w];
      float        dv = -INFINITY, av = -INFINITY;
      int          di = 0, ai = 0;
      for (int n = 0; n < F2_M; ++n) {
        if (row[n] > dv) {
          dv = row[n];
          di = n;
        }
        const float c = corr_at(row, static_cast<int>(PUCCH_F2_DFT) - F2_M + n);
        if (c > av) {
          av = c;
          ai = n;
        }
      }
      const int   idx = (dv >= av) ? di : -(F2_M - ai);
      auto        cv  = [&](int i) { return corr_at(row, idx + i - 2); };
      const float num = -0.4F * cv(0) + -0.2F * cv(1) + 0.0F * cv(2) + 0.2F * cv(3) + 0.4F * cv(4);
      const float den = 0.571429F * cv(0) + -0.285714F * cv(1) + -0.571429F * cv(2) + -0.285714F * cv(3) + 0.571429F * cv(4);
      const float q    = -num / den;
      const float frac = (isnan(q) || isinf(q) || fabsf(q) > 1.0F) ? 0.0F : q;
      ta += static_cast<float>((static_cast<double>(idx) + static_cast<double>(frac)) / job.fs);
    }
  }

  // Normalisation over both hops (do_compute :110-121) and the report.
  if (port_on && lane == 0u) {
    const float n_all = static_cast<float>(N * nsym);
    if (nof_hops == 2u) {
      ta = ta / 2.0F;
    }
    rsrp = rsrp / n_all;
    epre = epre / n_all;
    noise = fmaxf(rsrp / 1e10F, noise / static_cast<float>(N * nsym - 1u));
    const double    tc_units = static_cast<double>(ta) / F2_T_C;
    const long long tc10     = static_cast<long long>(tc_units * 10.0);  // from_seconds: truncate x10, round half away
    const long long tc       = tc10 / 10 + (tc10 % 10) / 5;
    res.noise_var[w]      = noise;
    res.rsrp[w]           = rsrp;
    res.epre[w]           = epre;
    res.cfo_hz[w]         = cfo_hz;
    res.time_alignment[w] = static_cast<double>(tc) * F2_T_C;
    port_nv[w]            = noise;
  }
  __syncthreads();
  copy_words(results + blockIdx.x, &res, tid, F2_THREADS);

  // Equalisation, demapping and descrambling: thread t takes data RE t.
  const uint32_t per_symbol = 8u * job.nof_prb;
  if (tid < per_symbol * nsym) {
    const uint32_t s = tid / per_symbol, i = tid % per_symbol;
    const uint32_t k = 12u * (i / 8u) + 3u * ((i % 8u) / 2u) + 2u * (i & 1u);  // REs 0, 2, 3, 5, 6, 8, 9, 11 of a PRB
    const uint32_t at = job.grid_base + (job.start_symbol + s) * nsc + 12u * job.prb[s] + k;
    cpx            y[PUCCH_F2_MAX_PORTS], h[PUCCH_F2_MAX_PORTS];
    float          nvs[PUCCH_F2_MAX_PORTS];
#pragma unroll
    for (uint32_t p = 0; p < PUCCH_F2_MAX_PORTS; ++p) {
      if (p < P) {
        y[p]   = bf16c(grids[at + p * job.port_stride]);  // grid port p, as the reference reads it
        h[p]   = bf16c(est[p][s][k]);
        nvs[p] = port_nv[p];
      }
    }
    cpx   eq;
    float var;
    equalize_zf1(y, h, P, nvs, eq, var);
    const float    rcp = var > 0.f ? 1.f / var : 0.f;
    int            l0 = demap_qpsk(eq.x, rcp), l1 = demap_qpsk(eq.y, rcp);
    const uint32_t bit = 2u * tid;
    const uint32_t c   = scrambling[job.scramble_word + (bit >> 5)] >> (bit & 31u);
    l0                 = (c & 1u) ? -l0 : l0;
    l1                 = (c & 2u) ? -l1 : l1;
    int8_t* out = llrs + job.llr_offset + bit;
    out[0]      = static_cast<int8_t>(l0);
    out[1]      = static_cast<int8_t>(l1);
  }
}

} // namespace

void launch_pucch_f2(const pucch_f2_job*     d_jobs,
                     uint32_t                nof_jobs,
                     const float*            d_dmrs,
                     const uint32_t*         d_scrambling,
                     const float*            d_twiddles,
                     const uint32_t*         d_grids,
                     int8_t*                 d_llrs,
                     srsgpu_pucch_f2_result* d_results,
                     hipStream_t             stream)
{
  if (nof_jobs == 0) {
    return;
  }
  hipLaunchKernelGGL(pucch_f2_kernel, dim3(nof_jobs), dim3(F2_THREADS), 0, stream, d_jobs,
                     reinterpret_cast<const cpx*>(d_dmrs), d_scrambling, reinterpret_cast<const cpx*>(d_twiddles), d_grids,
                     d_llrs, d_results);
}

} // namespace srsgpu
