// Host side of the NZP-CSI-RS C ABI (include/srsgpu_phy.h): refuses what the reference's assertions, this library and
// the grid refuse (csi_rs_host.cpp), lays every signal's CDM groups out as jobs and uploads them. Everything on the
// device is csi_rs.hip.
#include "capi_internal.h"
#include "csi_rs_host.h"
#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

using namespace srsgpu;

static_assert(sizeof(srsgpu_csi_rs_config) == 212, "srsgpu_csi_rs_config layout (mirrored by srsgpu)");

struct srsgpu_csi_rs_plan {
  srsgpu_context*           ctx = nullptr;
  device_buffer<csi_rs_job> d_jobs;
  uint32_t                  nof_jobs    = 0;
  uint32_t                  max_seq_len = 0;
};

extern "C" {

int srsgpu_csi_rs_plan_create(srsgpu_context*             ctx,
                              const srsgpu_csi_rs_config* cfgs,
                              uint32_t                    nof_signals,
                              uint32_t                    grid_nof_prb,
                              uint32_t                    grid_nof_ports,
                              uint32_t                    nof_grids,
                              srsgpu_csi_rs_plan**        plan_out)
{
  if (const int err = check_grid_args(ctx, plan_out, cfgs, nof_signals, grid_nof_prb, grid_nof_ports, nof_grids)) {
    return err;
  }
  const uint32_t nsc = 12 * grid_nof_prb, port_stride = 14 * nsc;
  std::vector<csi_rs_job> jobs;
  // (grid, symbol, RB) -> the subcarriers of the RB that are written and the signal that wrote last, for the overlap check.
  std::unordered_map<uint64_t, std::pair<uint32_t, uint32_t>> owner;
  uint32_t                                                    max_seq_len = 0;
  for (uint32_t i = 0; i < nof_signals; ++i) {
    const srsgpu_csi_rs_config& c = cfgs[i];
    csi_rs_signal               s;
    s.slot_index = c.slot_index;
    s.cp         = c.cp;
    s.start_rb   = c.start_rb;
    s.nof_rb     = c.nof_rb;
    s.row        = c.row;
    s.nof_k_ref  = c.nof_k_ref;
    std::copy(c.k_ref, c.k_ref + 6, s.k_ref);
    s.symbol_l0     = c.symbol_l0;
    s.symbol_l1     = c.symbol_l1;
    s.cdm           = c.cdm;
    s.freq_density  = c.freq_density;
    s.scrambling_id = c.scrambling_id;
    s.nof_ports     = c.nof_ports;
    s.amplitude     = c.amplitude;
    const std::string why = csi_rs_refusal(s, grid_nof_prb, grid_nof_ports);
    if (!why.empty()) {
      return fail(SRSGPU_ERR_INVALID_ARG, "signal %u: %s", i, why.c_str());
    }
    if (c.slot_index >= 160) {
      return fail(SRSGPU_ERR_INVALID_ARG, "signal %u: slot_index %u exceeds 159", i, c.slot_index);
    }
    if (c.grid_index >= nof_grids) {
      return fail(SRSGPU_ERR_INVALID_ARG, "signal %u: grid_index %u is outside the %u grids", i, c.grid_index, nof_grids);
    }
    const csi_rs_layout y = csi_rs_layout_of(s);
    if (y.seq_len != y.nof_rbs * y.per_rb ||
        (y.nof_rbs > 0 && y.rb_begin + y.rb_stride * (y.nof_rbs - 1) >= grid_nof_prb)) {
      return fail(SRSGPU_ERR_INVALID_ARG, "signal %u: internal layout bound exceeded", i);
    }
    if (y.seq_len == 0) {
      continue;  // density 0.5 over no RB of its parity: nothing to write
    }
    const bool bypass = y.nof_ports == 1 && c.precoding[0][0][0] == 1.f && c.precoding[0][0][1] == 0.f;
    for (uint32_t g = 0; g < y.nof_groups; ++g) {
      uint32_t re_mask = 0;
      for (uint32_t j = 0; j < y.per_rb; ++j) {
        re_mask |= 1u << (y.k_bar[g] + y.k_step * j);
      }
      if (y.symbol[g] >= 14 || (re_mask >> 12) != 0) {
        return fail(SRSGPU_ERR_INVALID_ARG, "signal %u: internal layout bound exceeded", i);
      }
      for (uint32_t r = 0; r < y.nof_rbs; ++r) {
        const uint32_t rb  = y.rb_begin + y.rb_stride * r;
        const uint64_t key = (static_cast<uint64_t>(c.grid_index) * 14 + y.symbol[g]) * 275 + rb;
        auto           ins = owner.emplace(key, std::make_pair(re_mask, i));
        if (!ins.second) {
          if ((ins.first->second.first & re_mask) != 0) {
            return fail(SRSGPU_ERR_INVALID_ARG, "signals %u and %u both write REs of PRB %u of symbol %u of grid %u: one "
                        "launch gives them no order", ins.first->second.second, i, rb, y.symbol[g], c.grid_index);
          }
          ins.first->second.first |= re_mask;
          ins.first->second.second = i;
        }
      }
      csi_rs_job jb{};
      jb.c_init      = y.c_init[g];
      jb.seq_skip    = y.seq_skip;
      jb.seq_len     = y.seq_len;
      jb.grid_base   = c.grid_index * grid_nof_ports * port_stride + y.symbol[g] * nsc;
      jb.port_stride = port_stride;
      jb.rb_begin    = static_cast<uint16_t>(y.rb_begin);
      jb.rb_stride   = static_cast<uint16_t>(y.rb_stride);
      jb.per_rb      = static_cast<uint16_t>(y.per_rb);
      jb.k_step      = static_cast<uint16_t>(y.k_step);
      jb.k_bar       = static_cast<uint16_t>(y.k_bar[g]);
      jb.nof_layers  = static_cast<uint16_t>(y.cdm_size);
      jb.nof_ports   = static_cast<uint16_t>(y.nof_ports);
      jb.bypass      = bypass ? 1 : 0;
      jb.amplitude   = y.amplitude;
      for (uint32_t p = 0; p < y.nof_ports; ++p) {
        for (uint32_t q = 0; q < y.cdm_size; ++q) {
          jb.w[p][q][0] = c.precoding[p][g * y.cdm_size + q][0];
          jb.w[p][q][1] = c.precoding[p][g * y.cdm_size + q][1];
        }
      }
      jobs.push_back(jb);
      max_seq_len = std::max(max_seq_len, y.seq_len);
    }
  }
  std::lock_guard<std::mutex> lock(ctx->mtx);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int r = ensure_gold_tables(ctx)) {
    return r;
  }
  plan_ptr<srsgpu_csi_rs_plan> plan(new srsgpu_csi_rs_plan());
  plan->ctx         = ctx;
  plan->nof_jobs    = static_cast<uint32_t>(jobs.size());
  plan->max_seq_len = max_seq_len;
  if (!plan->d_jobs.upload(jobs)) {
    return fail(SRSGPU_ERR_HIP, "failed to upload the CSI-RS jobs");
  }
  *plan_out = plan.release();
  return SRSGPU_OK;
}

int srsgpu_csi_rs_plan_execute(const srsgpu_csi_rs_plan* plan, uint32_t* d_grids, void* stream)
{
  if (plan == nullptr || (plan->nof_jobs > 0 && d_grids == nullptr)) {
    return fail(SRSGPU_ERR_INVALID_ARG, "null argument");
  }
  launch_csi_rs(plan->d_jobs.get(), plan->nof_jobs, plan->max_seq_len, d_grids, plan->ctx->d_gold_x1.get(),
                plan->ctx->d_gold_x2_jump.get(), plan->ctx->d_gold_x2_lane.get(), static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return SRSGPU_OK;
}

void srsgpu_csi_rs_plan_destroy(srsgpu_csi_rs_plan* plan)
{
  if (plan == nullptr) {
    return;
  }
  delete plan;
}

} // extern "C"
