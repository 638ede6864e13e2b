// NZP-CSI-RS on gfx950: every signal of a batch of slots in one launch, into the bf16 resource grids of the PDSCH
// modulator's layout. Rows 1-5 of TS 38.211 Table 7.4.1.5.3-1: one to four ports, no CDM or FD-CDM2.
//
// Reference (behaviour, not code): lib/phy/upper/signal_processors/nzp_csi_rs_generator_impl.cpp:111 (sequence), :291
// (w_f cover) / :175 (one mapper call per CDM group, over all ports), support/resource_grid_mapper_impl.cpp:140 (RE
// order, the bypass of a lone weight 1), channel_precoder_generic.cpp:27 (precoding), adt/bf16.h:39.
//
// Work decomposition. A job is one CDM group of one signal on its symbol (csi_rs_host.h); blockIdx.y cuts its sequence
// into runs of 256 elements. The first lanes of a workgroup evaluate the at most 17 Gold words of the run by jump-ahead
// (gold_device.h; every CSI-RS sequence lies in chunk 0), and after one barrier lane t takes element t of the run:
// consecutive lanes on consecutive REs of the symbol. An element is the group's one or two ports (the second under
// the w_f cover) precoded onto every port of the signal, so a group stores zeros on the ports of the other group when
// the matrix is the identity, as the reference's mapper does.
//
// Floating point follows the reference exactly: every product term is rounded separately (no contraction), and the
// terms are summed in the reference's order.
#include "csi_rs_host.h"
#include "gold_device.h"
#include "signal_device.h"
#include "srsgpu_internal.h"

#pragma clang fp contract(off)

namespace srsgpu {
namespace {

constexpr uint32_t CSI_RS_THREADS = 256;

__global__ __launch_bounds__(CSI_RS_THREADS) void csi_rs_kernel(const csi_rs_job* __restrict__ jobs,
                                                                 uint32_t* __restrict__ grids,
                                                                 const uint32_t* __restrict__ x1,
                                                                 const uint32_t* __restrict__ x2_jump,
                                                                 const uint32_t* __restrict__ x2_lane)
{
  __shared__ uint32_t gold[CSI_RS_THREADS / 16 + 1];

  const csi_rs_job& jb  = jobs[blockIdx.x];
  const uint32_t    tid = threadIdx.x;
  const uint32_t    i0  = blockIdx.y * CSI_RS_THREADS;
  if (i0 >= jb.seq_len) {
    return;  // the whole workgroup: a shorter job of a plan with longer ones
  }
  // Element i reads sequence bits 2 (seq_skip + i) and the next one.
  const uint32_t count = min(CSI_RS_THREADS, jb.seq_len - i0);
  const uint32_t n0    = 2u * (jb.seq_skip + i0);
  const uint32_t w0    = n0 >> 5;
  const uint32_t nw    = ((n0 + 2u * count - 1u) >> 5) - w0 + 1u;
  if (tid < nw) {
    gold[tid] = gold_word(jb.c_init, w0 + tid, 0, x1, x2_jump, x2_lane);
  }
  __syncthreads();
  if (tid >= count) {
    return;
  }
  const uint32_t i    = i0 + tid;
  const uint32_t n    = n0 + 2u * tid;
  const uint32_t word = gold[(n >> 5) - w0];
  const uint32_t sh   = 31u - (n & 31u);
  const float    amp  = jb.amplitude;
  const float    re   = ((word >> sh) & 1u) ? -amp : amp;
  const float    im   = ((word >> (sh - 1u)) & 1u) ? -amp : amp;
  const uint32_t rb   = i / jb.per_rb, j = i - rb * jb.per_rb;
  const uint32_t e    = jb.grid_base + 12u * (jb.rb_begin + jb.rb_stride * rb) + jb.k_bar + jb.k_step * j;
  if (jb.bypass != 0) {
    grids[e] = bf16_bits(re) | (bf16_bits(im) << 16);
    return;
  }
  // The second port of the group: w_f = (+1, -1) along the sequence.
  const float s1 = (i & 1u) ? -1.f : 1.f;
  const float a = s1 * re, b = s1 * im;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if (p < static_cast<int>(jb.nof_ports)) {
      const float wr0 = jb.w[p][0][0], wi0 = jb.w[p][0][1];
      float       sr  = re * wr0 - im * wi0;
      float       si  = re * wi0 + im * wr0;
      if (jb.nof_layers == 2) {
        const float wr1 = jb.w[p][1][0], wi1 = jb.w[p][1][1];
        sr = sr + (a * wr1 - b * wi1);
        si = si + (a * wi1 + b * wr1);
      }
      grids[e + static_cast<uint32_t>(p) * jb.port_stride] = bf16_bits(sr) | (bf16_bits(si) << 16);
    }
  }
}

} // namespace

void launch_csi_rs(const csi_rs_job* d_jobs,
                   uint32_t          nof_jobs,
                   uint32_t          max_seq_len,
                   uint32_t*         d_grids,
                   const uint32_t*   d_x1,
                   const uint32_t*   d_x2_jump,
                   const uint32_t*   d_x2_lane,
                   hipStream_t       stream)
{
  if (nof_jobs == 0 || max_seq_len == 0) {
    return;
  }
  hipLaunchKernelGGL(csi_rs_kernel, dim3(nof_jobs, (max_seq_len + CSI_RS_THREADS - 1) / CSI_RS_THREADS),
                     dim3(CSI_RS_THREADS), 0, stream, d_jobs, d_grids, d_x1, d_x2_jump, d_x2_lane);
}

} // namespace srsgpu
