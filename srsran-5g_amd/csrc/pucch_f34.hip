// PUCCH Format 3 / 4 front end on gfx950: every PDU of a batch in one launch, one 256-thread workgroup per PDU, from
// the bf16 grid words to the descrambled int8 LLRs and the per-port channel state. float32 throughout. No atomics, no
// scratch, nothing kept in HBM between the stages.
//
// Reference (behaviour, not code): lib/phy/upper/signal_processors/pucch/dmrs_pucch_estimator_formats3_4.cpp:94,
// lib/phy/upper/signal_processors/port_channel_estimator_average_impl.cpp:77 (hop loop, normalisation, noise floor) /
// :154 (one hop) / :322 (LSE and CFO) / :422 (noise), port_channel_estimator_helpers.cpp:212 (mean smoothing),
// include/srsran/phy/upper/pucch_formats3_4_helpers.h:158 (equalisation and deprecoding symbol by symbol),
// equalization/equalize_zf_1xn.h:128, lib/phy/generic_functions/transform_precoding/transform_precoder_dft_impl.cpp:32 /
// :60, lib/phy/upper/channel_processors/pucch/pucch_demodulator_format4.cpp:110 (despreading),
// channel_modulation/demodulation_mapper_impl.cpp:33 (pi/2-BPSK), demodulation_mapper_qpsk.cpp:40 / :122.
//
// Stage 1, estimation: wave w is receive port w, its lanes stride over the 12 nof_prb pilots of a DM-RS symbol. Per hop
// the LSEs of the hop's DM-RS symbols are added in symbol order and scaled by 1 / count (the reference's average over
// time), then averaged over the pilots (mean smoothing); that one value, rounded to bf16, is the estimate of every RE of
// the hop. EPRE, RSRP and the noise residual add up over both hops and are normalised once.
// Stage 2, equalisation and inverse DFT: thread = (data symbol, RE) for ZF 1 x N into LDS, then every data symbol's
// M-point inverse DFT side by side, LDS to LDS, thread = (four data symbols, output): a direct M-term sum against the
// M-th roots, indexed (k n) mod M by an incremental walk. M <= 192 and a PDU has at most 2 304 outputs; the typical PDU has 1..4 PRB, where a
// mixed-radix transform would save microseconds nobody waits for (profiles/pucch_formats_3_4.md has the worst case).
// The post-equalisation noise variance does not depend on the RE (one estimate per hop), so its mean over a symbol's
// valid values is computed once per hop, by the reference's own sequential sum of M equal terms.
// Stage 3, output: thread = 4 LLRs = one store. Format 4 despreads over the PDU's stream; QPSK or pi/2-BPSK with the
// parity of the stream index; descrambling; a 32-bit store inside the range, bytes at its tail.
//
// The time alignment is reported as 0: under mean smoothing the reference's estimator correlates one constant per hop,
// whose peak is bin 0 with a symmetric neighbourhood (findings of srsgpu_pucch_f34_plan_*).

// Every product and sum rounds on its own, as the float32 restatement of this sequence does
// (tests/pucch_f34_cases.py); the pragma precedes the device helpers so that it reaches them too. The one exception is
// written out: the inverse DFT's terms are four fmaf each, which halves the arithmetic of the stage that bounds the
// largest PDU (72.5 -> 50.1 us for 16 PRB x 14 symbols on an MI355X), and the restatement fuses the same four.
#pragma clang fp contract(off)

#include "pucch_f34_host.h"
#include "signal_device.h"
#include "srsgpu_internal.h"

namespace srsgpu {
namespace {

constexpr uint32_t F34_THREADS = 256;
constexpr uint32_t F34_GROUP   = 4;  // data symbols one thread transforms side by side
constexpr float    F34_TWOPI   = 6.28318530717958647692F;  // the reference's float TWOPI
constexpr float    F34_GAIN    = 2.0F * 1.41421356F;        // 2 sqrt(2)

/// ZF 1 x N: ports with an abnormal channel or noise variance are skipped, nvar = sum |h|^2 nv / (sum |h|^2)^2.
__device__ __forceinline__ void zf_weights(const cpx* h, uint32_t P, const float* nv, bool* use, float& rcp, float& var)
{
  float ch_mod_sq = 0.f, nvar_acc = 0.f;
#pragma unroll
  for (uint32_t p = 0; p < PUCCH_F34_MAX_PORTS; ++p) {
    use[p] = false;
    if (p < P) {
      const float norm = norm2(h[p]);
      if (is_normal(norm) && is_normal(nv[p]) && nv[p] > 0.f) {
        use[p] = true;
        ch_mod_sq += norm;
        nvar_acc += norm * nv[p];
      }
    }
  }
  if (is_normal(ch_mod_sq) && is_normal(nvar_acc)) {
    rcp = 1.f / ch_mod_sq;
    var = nvar_acc * rcp * rcp;
  } else {
    rcp = 0.f;
    var = __builtin_inff();
    for (uint32_t p = 0; p < PUCCH_F34_MAX_PORTS; ++p) {
      use[p] = false;
    }
  }
}

/// The vectorised quantiser of the reference's QPSK demapper: l = (g x) / nvar by the reciprocal, scaled by 120 / 24,
/// clipped to +-120, rounded half to even.
__device__ __forceinline__ int quantize_vector(float gx, float nvar)
{
  const float rcp = nvar > 0.f ? 1.f / nvar : 0.f;
  float       v   = (gx * rcp) * (120.f / 24.f);
  v               = fminf(fmaxf(v, -120.f), 120.f);
  return static_cast<int>(__builtin_rintf(v));
}

/// log_likelihood_ratio::quantize of the scalar demappers: l = g x / nvar, clipped to +-24, times 120 / 24, rounded half
/// away from zero; 0 unless nvar > 0.
__device__ __forceinline__ int quantize_scalar(float gx, float nvar)
{
  if (!(nvar > 0.f)) {
    return 0;
  }
  float l = gx / nvar;
  if (fabsf(l) > 24.f) {
    l = copysignf(24.f, l);
  }
  return static_cast<int>(roundf(l / 24.f * 120.f));
}

__global__ __launch_bounds__(F34_THREADS) void pucch_f34_kernel(const pucch_f34_job* __restrict__ jobs,
                                                                const cpx* __restrict__ dmrs,
                                                                const uint32_t* __restrict__ scrambling,
                                                                const cpx* __restrict__ roots,
                                                                const uint32_t* __restrict__ grids,
                                                                int8_t* __restrict__ llrs,
                                                                srsgpu_pucch_f2_result* __restrict__ results)
{
  __shared__ pucch_f34_job          job;
  __shared__ cpx                    eq[PUCCH_F34_MAX_DATA][PUCCH_F34_MAX_RE];
  __shared__ cpx                    td[PUCCH_F34_MAX_DATA][PUCCH_F34_MAX_RE];
  __shared__ cpx                    tw[PUCCH_F34_MAX_RE];
  __shared__ uint32_t               est[2][PUCCH_F34_MAX_PORTS];
  __shared__ float                  port_nv[PUCCH_F34_MAX_PORTS];
  __shared__ float                  hop_nv[2];
  __shared__ srsgpu_pucch_f2_result res;

  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  copy_words(&job, jobs + blockIdx.x, tid, F34_THREADS);
  for (uint32_t i = tid; i < sizeof(res) / 4u; i += F34_THREADS) {
    reinterpret_cast<uint32_t*>(&res)[i] = 0u;
  }
  __syncthreads();

  const uint32_t M = 12u * job.nof_prb, P = job.nof_ports, nsc = job.nsc, nof_hops = job.nof_hops;
  if (tid < M) {
    tw[tid] = roots[job.root_row + tid];
  }
  const bool     port_on = w < P;
  const uint32_t pbase   = job.grid_base + job.ports[port_on ? w : 0u] * job.port_stride;
  const float    fm      = static_cast<float>(M);

  // ---- Stage 1: estimation, wave = receive port ----
  float rsrp = 0.f, epre = 0.f, noise = 0.f, cfo = 0.f;
  bool  have_cfo = false;
  for (uint32_t hop = 0; hop < nof_hops; ++hop) {
    const uint32_t first = job.hop_first_dmrs[hop], nd = job.hop_nof_dmrs[hop];
    const uint32_t col   = 12u * job.prb[hop];
    const float    inv   = 1.0F / static_cast<float>(nd);
    cpx            msum = {0.f, 0.f}, zc = {0.f, 0.f};
    float          e = 0.f;
    if (port_on) {
      for (uint32_t k = lane; k < M; k += 64u) {
        cpx acc = {0.f, 0.f}, l0 = {0.f, 0.f};
        for (uint32_t s = 0; s < nd; ++s) {
          const cpx rx  = bf16c(grids[pbase + job.dmrs_symbol[first + s] * nsc + col + k]);
          const cpx pil = dmrs[job.dmrs_row + (first + s) * M + k];
          const cpx l   = cmulc(rx, pil);
          e += norm2(rx);
          if (s == 0u) {
            acc = l;
            l0  = l;
          } else {
            if (s == 1u) {
              const cpx z = cmulc(l, l0);
              zc          = {zc.x + z.x, zc.y + z.y};
            }
            acc = {acc.x + l.x, acc.y + l.y};
          }
        }
        msum = {msum.x + acc.x * inv, msum.y + acc.y * inv};
      }
    }
    const cpx mean = {wave_sum(msum.x) / fm, wave_sum(msum.y) / fm};
    float     nz   = 0.f;
    if (port_on) {
      for (uint32_t k = lane; k < M; k += 64u) {
        for (uint32_t s = 0; s < nd; ++s) {
          const cpx rx   = bf16c(grids[pbase + job.dmrs_symbol[first + s] * nsc + col + k]);
          const cpx pred = cmul(mean, dmrs[job.dmrs_row + (first + s) * M + k]);
          nz += norm2(cpx{rx.x - pred.x, rx.y - pred.y});
        }
      }
    }
    rsrp += (norm2(mean) * fm) * static_cast<float>(nd);
    epre += wave_sum(e);
    noise += wave_sum(nz);
    const float zx = wave_sum(zc.x), zy = wave_sum(zc.y);
    if (nd >= 2u) {
      // CFO: the phase of sum lse_1 conj(lse_0) over the epochs' distance; the hops' values averaged; never applied.
      const float c = atan2f(zy, zx) / F34_TWOPI / job.cfo_delta[hop];
      cfo           = have_cfo ? (cfo + c) / 2.0F : c;
      have_cfo      = true;
    }
    if (port_on && lane == 0u) {
      est[hop][w] = to_bf16c(mean);
    }
  }
  if (port_on && lane == 0u) {
    const float n_all = static_cast<float>(M * job.nof_dmrs);
    rsrp              = rsrp / n_all;
    epre              = epre / n_all;
    noise             = fmaxf(rsrp / 1e10F, noise / static_cast<float>(M * job.nof_dmrs - 1u));
    res.noise_var[w]      = noise;
    res.rsrp[w]           = rsrp;
    res.epre[w]           = epre;
    res.cfo_hz[w]         = have_cfo ? cfo * job.scs_hz : __builtin_nanf("");
    res.time_alignment[w] = 0.0;
    port_nv[w]            = noise;
  }
  __syncthreads();
  copy_words(results + blockIdx.x, &res, tid, F34_THREADS);

  // The mean over a symbol's valid noise variances: M equal terms added one after the other, as the reference adds them.
  if (tid < nof_hops) {
    cpx   h[PUCCH_F34_MAX_PORTS];
    float nvs[PUCCH_F34_MAX_PORTS];
    bool  use[PUCCH_F34_MAX_PORTS];
    for (uint32_t p = 0; p < PUCCH_F34_MAX_PORTS; ++p) {
      h[p]   = bf16c(est[tid][p < P ? p : 0u]);
      nvs[p] = port_nv[p < P ? p : 0u];
    }
    float rcp, var;
    zf_weights(h, P, nvs, use, rcp, var);
    if (var > 0.f && var < __builtin_inff()) {
      float acc = 0.f;
      for (uint32_t i = 0; i < M; ++i) {
        acc += var;
      }
      var = acc / fm;
    }
    hop_nv[tid] = var;
  }

  // ---- Stage 2: equalisation, thread = (data symbol, RE) ----
  const uint32_t nof_re = job.nof_data * M;
  for (uint32_t i = tid; i < nof_re; i += F34_THREADS) {
    const uint32_t d = i / M, k = i - d * M, hop = job.data_hop[d];
    const uint32_t at = job.grid_base + job.data_symbol[d] * nsc + 12u * job.prb[hop] + k;
    cpx            h[PUCCH_F34_MAX_PORTS];
    float          nvs[PUCCH_F34_MAX_PORTS];
    bool           use[PUCCH_F34_MAX_PORTS];
#pragma unroll
    for (uint32_t p = 0; p < PUCCH_F34_MAX_PORTS; ++p) {
      h[p]   = bf16c(est[hop][p < P ? p : 0u]);
      nvs[p] = port_nv[p < P ? p : 0u];
    }
    float rcp, var;
    zf_weights(h, P, nvs, use, rcp, var);
    cpx acc = {0.f, 0.f};
#pragma unroll
    for (uint32_t p = 0; p < PUCCH_F34_MAX_PORTS; ++p) {
      if (use[p]) {
        const cpx z = cmulc(bf16c(grids[at + job.ports[p] * job.port_stride]), h[p]);
        acc         = {acc.x + z.x, acc.y + z.y};
      }
    }
    eq[d][k] = {acc.x * rcp, acc.y * rcp};
  }
  __syncthreads();

  // ---- The inverse DFT of every data symbol: thread = (group of four data symbols, output). One root per term serves
  // the four symbols, whose reads of eq are the same address across the wave, and the four sums are independent, so the
  // LDS latency of one term hides behind the arithmetic of the others. Each output adds its M terms in the order of k.
  const float    scale  = job.idft_scale;
  const uint32_t last   = job.nof_data - 1u;
  const uint32_t groups = (job.nof_data + F34_GROUP - 1u) / F34_GROUP;
  for (uint32_t i = tid; i < groups * M; i += F34_THREADS) {
    const uint32_t g = i / M, n = i - g * M, d0 = F34_GROUP * g;
    uint32_t       row[F34_GROUP];
    cpx            acc[F34_GROUP];
#pragma unroll
    for (uint32_t j = 0; j < F34_GROUP; ++j) {
      row[j] = d0 + j < last ? d0 + j : last;  // past the last symbol: computed again, not stored
      acc[j] = {0.f, 0.f};
    }
    uint32_t r = 0;
    for (uint32_t k = 0; k < M; ++k) {
      const cpx t = tw[r];
#pragma unroll
      for (uint32_t j = 0; j < F34_GROUP; ++j) {
        const cpx x = eq[row[j]][k];
        acc[j]      = {fmaf(x.x, t.x, fmaf(-x.y, t.y, acc[j].x)), fmaf(x.x, t.y, fmaf(x.y, t.x, acc[j].y))};
      }
      r += n;
      r = r >= M ? r - M : r;
    }
#pragma unroll
    for (uint32_t j = 0; j < F34_GROUP; ++j) {
      if (d0 + j <= last) {
        td[d0 + j][n] = {acc[j].x * scale, acc[j].y * scale};
      }
    }
  }
  __syncthreads();

  // ---- Stage 3: despreading, demapping, descrambling; thread = 4 LLRs ----
  const uint32_t E = job.nof_llrs, qm = job.pi2_bpsk != 0u ? 1u : 2u, sf = job.sf;
  const uint32_t nof_symbols = E / qm, per_word = 4u / qm, mod = 12u / sf;
  const uint32_t vector_end  = (nof_symbols / 16u) * 16u;  // the reference's QPSK demapper takes 16 symbols per vector
  for (uint32_t wd = tid; 4u * wd < E; wd += F34_THREADS) {
    int v[4] = {0, 0, 0, 0};
    for (uint32_t j = 0; j < per_word; ++j) {
      const uint32_t s = wd * per_word + j;
      if (s >= nof_symbols) {
        break;
      }
      cpx   z;
      float nvar;
      if (job.format == 4u) {
        const uint32_t l = s / mod, r = s - l * mod;
        const float    hv = hop_nv[job.data_hop[l]];
        z    = {0.f, 0.f};
        nvar = 0.f;
        for (uint32_t b = 0; b < sf; ++b) {
          const uint32_t k = r + b * mod, q = job.w_quarter[k];
          const cpx      y = td[l][k];
          const cpx      t = q == 0u ? y : q == 1u ? cpx{-y.y, y.x} : q == 2u ? cpx{-y.x, -y.y} : cpx{y.y, -y.x};
          z                = {z.x + t.x, z.y + t.y};
          nvar += hv;
        }
        const float inv_sf = 1.0F / static_cast<float>(sf);
        z                  = {z.x * inv_sf, z.y * inv_sf};
      } else {
        const uint32_t d = s / M;
        z                = td[d][s - d * M];
        nvar             = hop_nv[job.data_hop[d]];
      }
      if (qm == 2u) {
        const bool vec = s < vector_end;
        v[2u * j]      = vec ? quantize_vector(F34_GAIN * z.x, nvar) : quantize_scalar(F34_GAIN * z.x, nvar);
        v[2u * j + 1u] = vec ? quantize_vector(F34_GAIN * z.y, nvar) : quantize_scalar(F34_GAIN * z.y, nvar);
      } else {
        // Odd symbols of the stream are rotated by -j: (im, -re).
        const float sum = (s & 1u) ? z.y + (-z.x) : z.x + z.y;
        v[j]            = quantize_scalar(F34_GAIN * sum, nvar);
      }
    }
    const uint32_t bit = 4u * wd;
    const uint32_t c   = scrambling[job.scramble_word + (bit >> 5)] >> (bit & 31u);
    uint32_t       packed = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) {
      const int x = ((c >> b) & 1u) ? -v[b] : v[b];
      packed |= (static_cast<uint32_t>(x) & 0xffu) << (8u * b);
    }
    int8_t* out = llrs + job.llr_offset + bit;
    if (bit + 4u <= E) {
      *reinterpret_cast<uint32_t*>(out) = packed;
    } else {
      for (uint32_t b = 0; bit + b < E; ++b) {
        out[b] = static_cast<int8_t>((packed >> (8u * b)) & 0xffu);
      }
    }
  }
}

} // namespace

void launch_pucch_f34(const pucch_f34_job*    d_jobs,
                      uint32_t                nof_jobs,
                      const float*            d_dmrs,
                      const uint32_t*         d_scrambling,
                      const float*            d_roots,
                      const uint32_t*         d_grids,
                      int8_t*                 d_llrs,
                      srsgpu_pucch_f2_result* d_results,
                      hipStream_t             stream)
{
  if (nof_jobs == 0) {
    return;
  }
  hipLaunchKernelGGL(pucch_f34_kernel, dim3(nof_jobs), dim3(F34_THREADS), 0, stream, d_jobs,
                     reinterpret_cast<const cpx*>(d_dmrs), d_scrambling, reinterpret_cast<const cpx*>(d_roots), d_grids,
                     d_llrs, d_results);
}

} // namespace srsgpu
