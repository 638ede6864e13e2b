// PUCCH Formats 0 and 1 on gfx950: every Format 0 PDU and every Format 1 resource of a batch of slots detected in one
// launch, one wavefront (one 64-thread workgroup) per PDU or resource, from the bf16 resource grids of the uplink
// plans' layout to the UCI bits and the linear channel state. float32 throughout.
//
// Reference (behaviour, not code): lib/phy/upper/channel_processors/pucch/pucch_detector_format0.cpp:114 (detect),
// pucch_detector_format1.cpp:156 (detect) / :512 (process_hop) / :288 (combine_symbols) / :334 (estimate_channels) /
// :406 (combine_reconstructed_contributions) / :464 (compute_contributions) / :108 (detect_symbol).
//
// Every r_{u,v}^{alpha}(n) = exp(j (phi(n) pi / 4 + 2 pi alpha_idx n / 12)) is a 24th root of unity, and so is every
// twiddle of the 12-point transforms: one 24-entry cosine table serves all of them and no sincosf runs here. The
// orthogonal sequences w (lengths 5 and 7 are no 24th roots) come as a table from the host (pucch_host.cpp).
//
// Format 1. All allocated symbols of both hops are loaded once into LDS (symbol-major rows of 12 REs per port),
// multiplied by conj(r) of the symbol's base sequence, and transformed: row k of the 12-point DFT is the despread
// signal of initial cyclic shift k. Per hop and per OCC that an entry has, lane 4 k + p combines the data and the
// DM-RS symbols of (shift k, port p) with w* / sqrt(n); the sums over ports are two butterfly exchanges; the strongest
// shift is a wave-wide maximum; the pruned channel goes back through the 12-point inverse transform times w into the
// rebuilt DM-RS, accumulated over the OCCs in LDS. The hop's noise is the wave-wide sum of |lse - rebuilt|^2 over the
// DM-RS rows. Then one lane per entry combines the hops as detect() does and stores its 32-byte result.
//
// Format 0. Lane 8 c + row correlates row (symbol, port) with candidate c's sequence; three butterfly exchanges sum
// the rows; every lane then walks the candidates in table order for the first strictly largest metric.
#include "pucch_host.h"
#include "signal_device.h"
#include "srsgpu_internal.h"

namespace srsgpu {
namespace {

constexpr int PUCCH_THREADS  = 64;
constexpr int PUCCH_MAX_ROWS = 14 * 4;  // symbols x ports

// cos(2 pi k / 24); sin(2 pi k / 24) = cos(2 pi (k + 18) / 24).
__constant__ float kCos24[24] = {1.0F,           0.96592582629F,  0.86602540378F,  0.70710678119F,  0.5F,  0.25881904510F,
                                 0.0F,           -0.25881904510F, -0.5F,           -0.70710678119F, -0.86602540378F,
                                 -0.96592582629F, -1.0F,          -0.96592582629F, -0.86602540378F, -0.70710678119F,
                                 -0.5F,          -0.25881904510F, 0.0F,            0.25881904510F,  0.5F,
                                 0.70710678119F, 0.86602540378F,  0.96592582629F};

/// exp(j 2 pi k / 24), k in [0, 24).
__device__ __forceinline__ cpx root24(uint32_t k)
{
  const uint32_t ks = k + 18u;
  return {kCos24[k], kCos24[ks >= 24u ? ks - 24u : ks]};
}

__device__ __forceinline__ cpx w_at(const float* __restrict__ w, uint32_t n, uint32_t i, uint32_t m)
{
  const uint32_t at = 2u * ((n - 1u) * 49u + i * 7u + m);
  return {w[at], w[at + 1u]};
}

__device__ __forceinline__ void store_result(srsgpu_pucch_result* __restrict__ out, uint32_t sr, uint32_t a0, uint32_t a1,
                                             bool valid, float metric, float epre, float rsrp, float noise_var)
{
  srsgpu_pucch_result r;
  r.sr               = static_cast<uint8_t>(sr);
  r.harq_ack[0]      = static_cast<uint8_t>(a0);
  r.harq_ack[1]      = static_cast<uint8_t>(a1);
  r.status           = valid ? 1 : 0;
  r.detection_metric = metric;
  r.epre             = epre;
  r.rsrp             = rsrp;
  r.noise_var        = noise_var;
  r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
  *out = r;
}

__device__ void detect_format0(const pucch_job& job, const uint32_t* __restrict__ grids,
                               srsgpu_pucch_result* __restrict__ results, cpx* lse)
{
  const uint32_t lane = threadIdx.x, P = job.nof_ports, rows = job.nof_symbols * P;
  for (uint32_t t = lane; t < rows * 12u; t += PUCCH_THREADS) {
    const uint32_t row = t / 12u, n = t - 12u * row, s = row / P, p = row - s * P;
    lse[t] = bf16c(grids[job.sym_base[s] + job.ports[p] * job.port_stride + n]);
  }
  __syncthreads();
  const uint32_t c = lane >> 3, row = lane & 7u;
  const bool     active = c < job.nof_candidates && row < rows;
  float          power = 0.0F, corr2 = 0.0F, noise = 0.0F;
  if (active) {
    const uint32_t s = row / P;
    uint32_t       alpha = job.alpha[s] + job.m_cs[c];
    alpha                = alpha >= 12u ? alpha - 12u : alpha;
    cpx   corr = {0.0F, 0.0F};
    float pw   = 0.0F;
    uint32_t k = 0;  // 2 alpha n mod 24
#pragma unroll
    for (uint32_t n = 0; n < 12u; ++n) {
      const cpx      x  = lse[row * 12u + n];
      const uint32_t kk = job.phi3[n] + k;
      const cpx      r  = root24(kk >= 24u ? kk - 24u : kk);
      const cpx      y  = cmulc(x, r);
      corr.x += y.x;
      corr.y += y.y;
      pw += norm2(x);
      k += 2u * alpha;
      k = k >= 24u ? k - 24u : k;
    }
    power = pw / 12.0F;               // srsvec::average_power
    corr2 = norm2(corr) / 12.0F;      // corr_contribution
    noise = power * 12.0F - corr2;
  }
#pragma unroll
  for (int m = 1; m <= 4; m <<= 1) {
    power += __shfl_xor(power, m);
    corr2 += __shfl_xor(corr2, m);
    noise += __shfl_xor(noise, m);
  }
  const float metric = is_normal(noise) ? corr2 / noise : 0.0F;
  float    best = 0.0F, best_rsrp = 0.0F, best_noise = 0.0F;
  uint32_t message = 0;
  for (uint32_t i = 0; i < job.nof_candidates; ++i) {
    const float m = __shfl(metric, static_cast<int>(8u * i));
    const float r = __shfl(corr2, static_cast<int>(8u * i));
    const float v = __shfl(noise, static_cast<int>(8u * i));
    if (m > best) {
      best       = m;
      best_rsrp  = r;
      best_noise = v;
      message    = job.message[i];
    }
  }
  const float epre = __shfl(power, 0) / static_cast<float>(rows);
  if (lane == 0) {
    store_result(results + job.result_offset, message & 1u, (message >> 1) & 1u, (message >> 2) & 1u,
                 best > job.threshold, best, epre, best_rsrp, best_noise);
  }
}

__device__ void detect_format1(const pucch_job& job, const uint32_t* __restrict__ entries, const float* __restrict__ w,
                               const uint32_t* __restrict__ grids, srsgpu_pucch_result* __restrict__ results, cpx* lse,
                               cpx* dft, cpx* rebuilt, cpx* ch, float (*met)[7][12][4])
{
  const uint32_t lane = threadIdx.x, P = job.nof_ports, S = job.nof_symbols, items = S * P * 12u;
  const uint32_t dmrs_mask = job.dmrs_mask;

  // Load, EPRE, match to the base sequence of each symbol (m0 = m_cs = 0).
  float epre = 0.0F;
  for (uint32_t t = lane; t < items; t += PUCCH_THREADS) {
    const uint32_t row = t / 12u, n = t - 12u * row, s = row / P, p = row - s * P;
    const cpx      x = bf16c(grids[job.sym_base[s] + job.ports[p] * job.port_stride + n]);
    epre += norm2(x);
    const uint32_t k = (job.phi3[n] + 2u * job.alpha[s] * n) % 24u;
    lse[t]           = cmulc(x, root24(k));
    rebuilt[t]       = {0.0F, 0.0F};
  }
  __syncthreads();
  // 12-point DFT of every row: bin k is the despread signal of initial cyclic shift k.
  for (uint32_t t = lane; t < items; t += PUCCH_THREADS) {
    const uint32_t row = t / 12u, k = t - 12u * row;
    cpx            acc = {0.0F, 0.0F};
    uint32_t       q = 0;  // n k mod 12
#pragma unroll
    for (uint32_t n = 0; n < 12u; ++n) {
      const cpx y = cmul(lse[row * 12u + n], root24(q == 0u ? 0u : 24u - 2u * q));
      acc.x += y.x;
      acc.y += y.y;
      q += k;
      q = q >= 12u ? q - 12u : q;
    }
    dft[t] = acc;
  }
  __syncthreads();
  epre = wave_sum(epre) / static_cast<float>(items);

  const uint32_t k = lane >> 2, p = lane & 3u;
  const bool     active = lane < 48u && p < P;
  float          noise = 0.0F;
  uint32_t       noise_samples[2] = {0u, 0u};
  for (uint32_t hop = 0; hop < job.nof_hops; ++hop) {
    const uint32_t first = job.hop_first[hop], end = first + job.hop_nof_symbols[hop];
    const uint32_t nd = job.hop_nof_data[hop], nm = job.hop_nof_dmrs[hop];
    const float    inv_sqrt_nd = 1.0F / sqrtf(static_cast<float>(nd)), inv_sqrt_nm = 1.0F / sqrtf(static_cast<float>(nm));
    noise_samples[hop]         = nm * P * 12u;
    for (uint32_t occ = 0; occ < nd; ++occ) {
      if (((job.occ_mask >> occ) & 1u) == 0u) {
        continue;
      }
      // Despread in time: data and DM-RS symbols separately, with w* / sqrt(n).
      cpx data = {0.0F, 0.0F}, dmrs = {0.0F, 0.0F};
      if (active) {
        uint32_t id = 0, im = 0;
        for (uint32_t s = first; s < end; ++s) {
          const cpx  v       = dft[(s * P + p) * 12u + k];
          const bool is_dmrs = ((dmrs_mask >> s) & 1u) != 0u;
          const cpx  ws      = is_dmrs ? w_at(w, nm, occ, im) : w_at(w, nd, occ, id);
          const cpx  y       = cmulc(v, ws);
          if (is_dmrs) {
            dmrs.x += y.x, dmrs.y += y.y, ++im;
          } else {
            data.x += y.x, data.y += y.y, ++id;
          }
        }
        data = {data.x * inv_sqrt_nd, data.y * inv_sqrt_nd};
        dmrs = {dmrs.x * inv_sqrt_nm, dmrs.y * inv_sqrt_nm};
      }
      // Main and cross contributions and the channel energy, summed over the ports of a shift.
      const float est_norm = 1.0F / (sqrtf(static_cast<float>(nm)) * 12.0F);
      cpx         chv   = {dmrs.x * est_norm, dmrs.y * est_norm};
      cpx         cross = cmulc(dmrs, data);
      float       main_c = norm2(data) + norm2(dmrs), energy = norm2(chv);
#pragma unroll
      for (int m = 1; m <= 2; m <<= 1) {
        main_c += __shfl_xor(main_c, m);
        cross.x += __shfl_xor(cross.x, m);
        cross.y += __shfl_xor(cross.y, m);
        energy += __shfl_xor(energy, m);
      }
      const float scale = 1.0F / static_cast<float>(12u * (nm + nd));
      // Shifts 10 dB or more below the strongest one carry no channel.
      const float threshold = wave_max(lane < 48u ? energy : 0.0F) / 10.0F;
      if (!(energy > threshold)) {
        chv = {0.0F, 0.0F};
      }
      if (lane < 48u) {
        ch[p * 12u + k] = active ? chv : cpx{0.0F, 0.0F};
        if (p == 0u) {
          met[hop][occ][k][0] = main_c * scale;
          met[hop][occ][k][1] = cross.x * scale;
          met[hop][occ][k][2] = cross.y * scale;
          met[hop][occ][k][3] = energy * (1.0F / static_cast<float>(P));
        }
      }
      __syncthreads();
      // Rebuild the DM-RS: the inverse DFT of the channel coefficients, times conj(w*) = w of the symbol.
      for (uint32_t t = lane + first * P * 12u; t < end * P * 12u; t += PUCCH_THREADS) {
        const uint32_t row = t / 12u, n = t - 12u * row, s = row / P, pp = row - s * P;
        if (((dmrs_mask >> s) & 1u) == 0u) {
          continue;
        }
        cpx      acc = {0.0F, 0.0F};
        uint32_t q = 0;  // n k mod 12
#pragma unroll
        for (uint32_t kk = 0; kk < 12u; ++kk) {
          const cpx y = cmul(ch[pp * 12u + kk], root24(2u * q));
          acc.x += y.x;
          acc.y += y.y;
          q += n;
          q = q >= 12u ? q - 12u : q;
        }
        const uint32_t im = __popc(dmrs_mask & ((1u << s) - 1u) & ~((1u << first) - 1u));
        const cpx      y  = cmul(acc, w_at(w, nm, occ, im));
        rebuilt[t].x += y.x;
        rebuilt[t].y += y.y;
      }
      __syncthreads();
    }
    // The hop's noise: received minus rebuilt DM-RS.
    float acc = 0.0F;
    for (uint32_t t = lane + first * P * 12u; t < end * P * 12u; t += PUCCH_THREADS) {
      const uint32_t s = t / (12u * P);
      if (((dmrs_mask >> s) & 1u) != 0u) {
        const cpx d = {lse[t].x - rebuilt[t].x, lse[t].y - rebuilt[t].y};
        acc += norm2(d);
      }
    }
    noise += wave_sum(acc);
  }
  const float n0 = static_cast<float>(noise_samples[0]), n1 = static_cast<float>(noise_samples[1]);
  const float noise_var = noise / static_cast<float>(noise_samples[0] + noise_samples[1]);

  for (uint32_t e = lane; e < job.nof_entries; e += PUCCH_THREADS) {
    const uint32_t word = entries[job.first_entry + e];
    const uint32_t ics = word & 0xffu, occ = (word >> 8) & 0xffu, nof_bits = (word >> 16) & 0xffu;
    float          main_c = met[0][occ][ics][0], rsrp = met[0][occ][ics][3];
    cpx            cross = {met[0][occ][ics][1], met[0][occ][ics][2]};
    if (job.nof_hops == 2) {
      main_c += met[1][occ][ics][0];
      cross.x += met[1][occ][ics][1];
      cross.y += met[1][occ][ics][2];
      rsrp = (rsrp * n0 + met[1][occ][ics][3] * n1) / static_cast<float>(noise_samples[0] + noise_samples[1]);
    }
    // detect_symbol: the BPSK or QPSK symbol with the largest real part of symbol x cross term.
    const float a  = 0.70710678118654752440F;
    const float m1 = a * cross.x - a * cross.y, m2 = a * cross.x + a * cross.y;
    uint32_t    b0 = 0, b1 = 0;
    float       detected = m1;
    if (nof_bits == 2u && fabsf(m2) > fabsf(m1)) {
      detected = m2;
      b1       = 1;
    }
    if (nof_bits == 2u ? detected < 0.0F : !(detected > 0.0F)) {
      detected = -detected;
      b0       = 1u - b0;
      b1       = nof_bits == 2u ? 1u - b1 : 0u;
    }
    const float metric = (main_c + 2.0F * detected) / noise_var;
    bool        valid  = metric > job.threshold;
    // SR only: the detected bit must be 0.
    valid = valid && (nof_bits != 0u || b0 == 0u);
    store_result(results + job.result_offset + e, 0u, b0, b1, valid, metric / job.threshold, epre, rsrp, noise_var);
  }
}

__global__ __launch_bounds__(PUCCH_THREADS) void pucch_detector_kernel(const pucch_job* __restrict__ jobs,
                                                                        const uint32_t* __restrict__ entries,
                                                                        const float* __restrict__ w,
                                                                        const uint32_t* __restrict__ grids,
                                                                        srsgpu_pucch_result* __restrict__ results)
{
  __shared__ cpx   lse[PUCCH_MAX_ROWS * 12];
  __shared__ cpx   dft[PUCCH_MAX_ROWS * 12];
  __shared__ cpx   rebuilt[PUCCH_MAX_ROWS * 12];
  __shared__ cpx   ch[48];
  __shared__ float met[2][7][12][4];
  __shared__ pucch_job job;

  // The descriptor goes to LDS once: every lane indexes its byte tables.
  copy_words(&job, jobs + blockIdx.x, threadIdx.x, PUCCH_THREADS);
  __syncthreads();
  if (job.kind == 0u) {
    detect_format0(job, grids, results, lse);
  } else {
    detect_format1(job, entries, w, grids, results, lse, dft, rebuilt, ch, met);
  }
}

} // namespace

void launch_pucch_detector(const pucch_job*     d_jobs,
                           uint32_t             nof_jobs,
                           const uint32_t*      d_entries,
                           const float*         d_w,
                           const uint32_t*      d_grids,
                           srsgpu_pucch_result* d_results,
                           hipStream_t          stream)
{
  if (nof_jobs == 0) {
    return;
  }
  hipLaunchKernelGGL(pucch_detector_kernel, dim3(nof_jobs), dim3(PUCCH_THREADS), 0, stream, d_jobs, d_entries, d_w, d_grids,
                     d_results);
}

} // namespace srsgpu
