// SRS estimation on gfx950: every resource of a batch in one launch, one 512-thread workgroup per resource, from the
// bf16 grid words to the channel matrix, the EPRE, the noise variance and the time alignment. float32 from the grid
// words; double only for the time alignment scalars. No atomics, no scratch.
//
// Reference (behaviour, not code): lib/phy/upper/signal_processors/srs/srs_estimator_generic_impl.cpp:137-206 (LSE,
// EPRE and time alignment per antenna port), :56-77 (phase compensation through the 1024-entry table), :213-258
// (coefficients and noise residual), :264-267 (normalisation);
// lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.cpp:174 (correlation summed over the rx
// ports) / :245 (peak search) / :51 (quadratic refinement).
//
// The reference keeps the mean LSE of every (subcarrier, rx port, antenna port); at 1632 x 4 x 4 values that does not
// fit the LDS, so nothing of it is kept. LDS holds the IDFT buffer, the correlation, the antenna ports' sequences and
// the phase table; the sum over symbols of a received RE is read from the grid words again wherever it is needed (once
// per antenna port for the time alignment, once for the coefficients and once for the residual: at most 104 KB per
// comb set, which stays in L2). The sum over symbols is taken before the product with the conjugate sequence, where the
// reference multiplies each symbol and sums: the same value up to float32 rounding.
//
// The inverse transform (radix 2, decimation in frequency, two stages per barrier, bit-reversed read-back at the
// searched bins only) and the peak search with its 5- / 3-tap refinement are the lines of pusch_chest.hip:701-811,
// copied: that kernel runs them on a template-sized team with its own LDS layout and reductions, and sharing them as
// device functions would change its compiled code.
#include "srs_host.h"
#include "signal_device.h"
#include "srsgpu_internal.h"

namespace srsgpu {
namespace {

constexpr uint32_t SRS_THREADS = 512;
constexpr uint32_t SRS_WAVES   = SRS_THREADS / 64;
constexpr float    SRS_TWOPI   = 6.28318530717958647692F;  // the reference's float TWOPI (math_utils.h:36)

/// int(round(1024 (n ps + po) / 2 pi)) in float32, every operation rounded on its own as the reference's source reads
/// (:66-68); a negative index wraps through unsigned, modulo the table size.
__device__ __forceinline__ uint32_t phase_index(uint32_t n, float ps, float po)
{
#pragma clang fp contract(off)
  const float a = static_cast<float>(n) * ps + po;
  const float t = (static_cast<float>(SRS_CEXP_SIZE) * a) / SRS_TWOPI;
  return static_cast<uint32_t>(static_cast<int>(roundf(t))) & (SRS_CEXP_SIZE - 1u);
}

/// Sums of N floats over the workgroup; every thread ends with them. red: SRS_WAVES x N floats.
template <int N>
__device__ __forceinline__ void block_sum(float (&v)[N], float* red)
{
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    v[i] = wave_sum(v[i]);
  }
  __syncthreads();  // the previous reduction's readers are done
  if (lane == 0u) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      red[wave * N + i] = v[i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float s = 0.0F;
#pragma unroll
    for (uint32_t w = 0; w < SRS_WAVES; ++w) {
      s += red[w * N + i];
    }
    v[i] = s;
  }
}

__device__ __forceinline__ void take_larger(float& v, int& i, float ov, int oi)
{
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

/// The first largest value over the workgroup and its index; every thread ends with them.
__device__ __forceinline__ void block_argmax(float& v, int& i, float* redf, int* redi)
{
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    take_larger(v, i, __shfl_xor(v, m), __shfl_xor(i, m));
  }
  __syncthreads();
  if (lane == 0u) {
    redf[wave] = v;
    redi[wave] = i;
  }
  __syncthreads();
  v = redf[0];
  i = redi[0];
#pragma unroll
  for (uint32_t w = 1; w < SRS_WAVES; ++w) {
    take_larger(v, i, redf[w], redi[w]);
  }
}

/// The sum over the resource's symbols of one received RE; with POWER also the sum of their powers.
template <bool POWER>
__device__ __forceinline__ cpx symbol_sum(const uint32_t* __restrict__ grids, uint32_t at, uint32_t nsc, uint32_t S,
                                          float& power)
{
  cpx y = {0.0F, 0.0F};
  for (uint32_t s = 0; s < S; ++s) {
    const cpx v = bf16c(grids[at + s * nsc]);
    y.x += v.x;
    y.y += v.y;
    if (POWER) {
      power += norm2(v);
    }
  }
  return y;
}

__global__ __launch_bounds__(SRS_THREADS) void srs_estimator_kernel(const srs_job* __restrict__ jobs,
                                                                     const cpx* __restrict__ seqs,
                                                                     const cpx* __restrict__ cexp_table,
                                                                     const uint32_t* __restrict__ grids,
                                                                     srsgpu_srs_result* __restrict__ results)
{
  __shared__ cpx               X[SRS_MAX_M];
  __shared__ float             corr[SRS_MAX_M];
  __shared__ cpx               seq[SRS_MAX_PORTS][SRS_MAX_L];
  __shared__ cpx               cexp[SRS_CEXP_SIZE];
  __shared__ float             redf[SRS_WAVES * 8];
  __shared__ int               redi[SRS_WAVES];
  __shared__ srs_job           job;
  __shared__ srsgpu_srs_result res;

  const uint32_t tid = threadIdx.x;
  copy_words(&job, jobs + blockIdx.x, tid, SRS_THREADS);
  for (uint32_t i = tid; i < SRS_CEXP_SIZE; i += SRS_THREADS) {
    cexp[i] = cexp_table[i];
  }
  for (uint32_t i = tid; i < sizeof(res) / 4u; i += SRS_THREADS) {
    reinterpret_cast<uint32_t*>(&res)[i] = 0u;
  }
  __syncthreads();
  const uint32_t L = job.L, comb = job.comb, P = job.nof_tx, R = job.nof_rx, S = job.nof_symbols, nsc = job.nsc;
  const int      M = static_cast<int>(job.M), lgM = static_cast<int>(job.log2M), m = static_cast<int>(job.max_ta_samples);
  const bool     interleaved = job.interleaved != 0u;
  for (uint32_t p = 0; p < P; ++p) {
    const cpx* __restrict__ row = seqs + job.seq_row[p];
    for (uint32_t n = tid; n < L; n += SRS_THREADS) {
      seq[p][n] = row[n];
    }
  }
  __syncthreads();
  auto rx_base = [&](uint32_t r) { return job.grid_base + job.rx_ports[r] * job.port_stride + job.start_symbol * nsc; };
  const float inv_s = 1.0F / static_cast<float>(S);

  // Per antenna port: the mean LSE of every rx port through the inverse transform, |.|^2 summed over the rx ports, the
  // peak within +-max_ta_samples taps (the delayed half wins a tie) and its quadratic refinement.
  float  epre_acc = 0.0F;
  double ta_sum   = 0.0;
  // Only the bins the search and the refinement read: n in [0, m + 2) and [M - m - 2, M).
  const int nb  = min(M, 2 * (m + 2));
  auto      bin = [&](int t) { return t < m + 2 ? t : M - nb + t; };
  for (uint32_t p = 0; p < P; ++p) {
    const bool owner = p == 0u || (interleaved && p == 1u);  // its REs count for the EPRE (:169)
    for (uint32_t r = 0; r < R; ++r) {
      const uint32_t base = rx_base(r) + job.k0[p];
      for (int n = static_cast<int>(tid); n < M; n += static_cast<int>(SRS_THREADS)) {
        cpx v = {0.0F, 0.0F};
        if (n < static_cast<int>(L)) {
          float     unused = 0.0F;
          const cpx y = owner ? symbol_sum<true>(grids, base + static_cast<uint32_t>(n) * comb, nsc, S, epre_acc)
                              : symbol_sum<false>(grids, base + static_cast<uint32_t>(n) * comb, nsc, S, unused);
          const cpx z = cmulc(y, seq[p][n]);
          v           = {z.x * inv_s, z.y * inv_s};
        }
        X[n] = v;
      }
      __syncthreads();
      // Radix-2 decimation in frequency, inverse sign, two stages per barrier: a thread takes the four elements
      // i0 + {0, h, 2h, 3h} through the stage of span 2h (twiddles e^{+j 2 pi j' / 4h}, j' = j, j + h) and the stage of
      // span h (e^{+j 2 pi j / 2h}) in registers. Natural-order input, bit-reversed output.
      auto twiddle = [](int j, int span2) {  // e^{+j 2 pi j / span2} (revolutions)
        const float rev = static_cast<float>(j) / static_cast<float>(span2);
        return cpx{__builtin_amdgcn_cosf(rev), __builtin_amdgcn_sinf(rev)};
      };
      int lh = lgM - 1;
      for (; lh >= 1; lh -= 2) {
        const int h = 1 << (lh - 1);
        for (int b = static_cast<int>(tid); b < M / 4; b += static_cast<int>(SRS_THREADS)) {
          const int j  = b & (h - 1);
          const int i0 = ((b >> (lh - 1)) << (lh + 1)) + j;
          const cpx x0 = X[i0], x1 = X[i0 + h], x2 = X[i0 + 2 * h], x3 = X[i0 + 3 * h];
          const cpx y0 = {x0.x + x2.x, x0.y + x2.y};
          const cpx y2 = cmul({x0.x - x2.x, x0.y - x2.y}, twiddle(j, 4 * h));
          const cpx y1 = {x1.x + x3.x, x1.y + x3.y};
          const cpx y3 = cmul({x1.x - x3.x, x1.y - x3.y}, twiddle(j + h, 4 * h));
          const cpx w1 = twiddle(j, 2 * h);
          X[i0]         = {y0.x + y1.x, y0.y + y1.y};
          X[i0 + h]     = cmul({y0.x - y1.x, y0.y - y1.y}, w1);
          X[i0 + 2 * h] = {y2.x + y3.x, y2.y + y3.y};
          X[i0 + 3 * h] = cmul({y2.x - y3.x, y2.y - y3.y}, w1);
        }
        __syncthreads();
      }
      if (lh == 0) {  // odd number of stages: the last one (span 1, unit twiddle) alone
        for (int b = static_cast<int>(tid); b < M / 2; b += static_cast<int>(SRS_THREADS)) {
          const cpx a = X[2 * b], c = X[2 * b + 1];
          X[2 * b]     = {a.x + c.x, a.y + c.y};
          X[2 * b + 1] = {a.x - c.x, a.y - c.y};
        }
        __syncthreads();
      }
      for (int t = static_cast<int>(tid); t < nb; t += static_cast<int>(SRS_THREADS)) {
        const int   n  = bin(t);
        const float pw = norm2(X[__brev(static_cast<uint32_t>(n)) >> (32 - lgM)]);
        corr[n]        = r != 0u ? corr[n] + pw : pw;
      }
      __syncthreads();
    }
    float dv = -INFINITY, av = -INFINITY;
    int   di = 0x7fffffff, ai = 0x7fffffff;
    for (int n = static_cast<int>(tid); n < m; n += static_cast<int>(SRS_THREADS)) {
      if (corr[n] > dv) {
        dv = corr[n];
        di = n;
      }
      if (corr[M - m + n] > av) {
        av = corr[M - m + n];
        ai = n;
      }
    }
    block_argmax(dv, di, redf, redi);
    block_argmax(av, ai, redf, redi);
    const int   idx = (dv >= av) ? di : -(m - ai);
    const int   nt  = (m > 2) ? 5 : 3;  // (M is never the largest DFT size, 4096: the refinement always runs)
    auto        cv  = [&](int i) { return corr[(idx + i - nt / 2) & (M - 1)]; };
    float       num, den, corr_k;
    if (nt == 5) {
      num    = -0.4F * cv(0) + -0.2F * cv(1) + 0.0F * cv(2) + 0.2F * cv(3) + 0.4F * cv(4);
      den    = 0.571429F * cv(0) + -0.285714F * cv(1) + -0.571429F * cv(2) + -0.285714F * cv(3) + 0.571429F * cv(4);
      corr_k = 1.0F;
    } else {
      num    = -0.5F * cv(0) + 0.0F * cv(1) + 0.5F * cv(2);
      den    = 0.5F * cv(0) + -1.0F * cv(1) + 0.5F * cv(2);
      corr_k = 0.5F;
    }
    const float q    = -corr_k * num / den;
    const float frac = (isnan(q) || isinf(q) || fabsf(q) > 1.0F) ? 0.0F : q;
    ta_sum += (static_cast<double>(idx) + static_cast<double>(frac)) / job.fs;
    if (tid == 0u) {
      res.ta_idx[p] = idx;
    }
    __syncthreads();  // the refinement has read corr before the next antenna port writes it
  }
  const double ta = ta_sum / static_cast<double>(P);

  // Phase compensation (:222-229): the slope and, per comb set, the offset of its first subcarrier, cast as the
  // reference casts them.
  const float    ps    = static_cast<float>(static_cast<double>(SRS_TWOPI) * ta * static_cast<double>(job.khz) * 1000.0 *
                                      static_cast<double>(comb));
  const uint32_t nsets = interleaved ? 2u : 1u;  // set q: the REs of antenna port q (ports of the same parity share it)
  float          po[2];
#pragma unroll
  for (uint32_t q = 0; q < 2u; ++q) {
#pragma clang fp contract(off)
    po[q] = ps * static_cast<float>(job.k0[q] % comb) / static_cast<float>(comb);
  }

  // Per rx port: the coefficients (the mean of the compensated LSE of every antenna port), then the residual of the
  // compensated sum over symbols against nof_symbols x coefficient x sequence of every antenna port on its comb set.
  // The reference calls srsvec::subtract(noise_help, recovered, noise_help), whose first argument is the output: the
  // helper becomes recovered - helper and changes sign with every antenna port, so with two or four ports on a comb
  // set every other port's signal is added where it was meant to be removed. Restated as it is.
  float noise_acc = 0.0F;
  for (uint32_t r = 0; r < R; ++r) {
    const uint32_t base = rx_base(r);
    float          acc[8] = {0.0F, 0.0F, 0.0F, 0.0F, 0.0F, 0.0F, 0.0F, 0.0F};
    for (uint32_t n = tid; n < L; n += SRS_THREADS) {
#pragma unroll
      for (uint32_t q = 0; q < 2u; ++q) {
        if (q < nsets) {
          float     unused = 0.0F;
          const cpx y = symbol_sum<false>(grids, base + job.k0[q] + n * comb, nsc, S, unused);
          const cpx c = cexp[phase_index(n, ps, po[q])];
#pragma unroll
          for (uint32_t p = 0; p < SRS_MAX_PORTS; ++p) {
            if (p < P && (interleaved ? (p & 1u) == q : q == 0u)) {
              const cpx lse = cmulc(y, seq[p][n]);
              const cpx z   = cmul({lse.x * inv_s, lse.y * inv_s}, c);
              acc[2 * p] += z.x;
              acc[2 * p + 1] += z.y;
            }
          }
        }
      }
    }
    block_sum<8>(acc, redf);
    const float inv_l = 1.0F / static_cast<float>(L);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      acc[i] = acc[i] * inv_l;
    }
    const float fs_ = static_cast<float>(S);
    for (uint32_t n = tid; n < L; n += SRS_THREADS) {
#pragma unroll
      for (uint32_t q = 0; q < 2u; ++q) {
        if (q < nsets) {
          float     unused = 0.0F;
          const cpx y = symbol_sum<false>(grids, base + job.k0[q] + n * comb, nsc, S, unused);
          cpx       e = cmul(y, cexp[phase_index(n, ps, po[q])]);
#pragma unroll
          for (uint32_t p = 0; p < SRS_MAX_PORTS; ++p) {
            if (p < P && (interleaved ? (p & 1u) == q : q == 0u)) {
              const cpx rec = cmul(seq[p][n], {fs_ * acc[2 * p], fs_ * acc[2 * p + 1]});
              e = {rec.x - e.x, rec.y - e.y};  // recovered - helper, as the reference's subtract call leaves it (:249)
            }
          }
          noise_acc += norm2(e);
        }
      }
    }
    if (tid == 0u) {
#pragma unroll
      for (uint32_t p = 0; p < SRS_MAX_PORTS; ++p) {
        if (p < P) {
          res.channel[r][p][0] = acc[2 * p];
          res.channel[r][p][1] = acc[2 * p + 1];
        }
      }
    }
  }

  // Normalisation (:264-267): degrees of freedom and the doubled RE count of the interleaved case.
  float fin[2] = {epre_acc, noise_acc};
  block_sum<2>(fin, redf);
  if (tid == 0u) {
    const uint32_t nof_estimates = interleaved ? 2u : P, correction = interleaved ? 2u : 1u;
    res.noise_var      = fin[1] / static_cast<float>((S * L - nof_estimates) * correction * R);
    res.epre           = fin[0] / static_cast<float>(L) / static_cast<float>(S * correction * R);
    res.time_alignment = ta;
    res.resolution     = 1.0 / job.fs;
    res.ta_max         = static_cast<double>(job.max_ta_samples) / job.fs;
  }
  __syncthreads();
  copy_words(results + job.result_index, &res, tid, SRS_THREADS);
}

} // namespace

void launch_srs_estimator(const srs_job*     d_jobs,
                          uint32_t           nof_jobs,
                          const float*       d_seqs,
                          const float*       d_cexp,
                          const uint32_t*    d_grids,
                          srsgpu_srs_result* d_results,
                          hipStream_t        stream)
{
  if (nof_jobs == 0) {
    return;
  }
  hipLaunchKernelGGL(srs_estimator_kernel, dim3(nof_jobs), dim3(SRS_THREADS), 0, stream, d_jobs,
                     reinterpret_cast<const cpx*>(d_seqs), reinterpret_cast<const cpx*>(d_cexp), d_grids, d_results);
}

} // namespace srsgpu
