// Host side of the SS/PBCH block C ABI (include/srsgpu_phy.h): refuses what ssb_processor_impl::process asserts and
// what the grid or the port list cannot hold (ssb_host.cpp), derives l_start and k_start, builds the PBCH's downlink
// polar code tables for (56, 864) once (polar_code.cpp) and uploads them with the block descriptors. Everything on the
// device is ssb.hip.
#include "capi_internal.h"
#include "polar_code.h"
#include "ssb_host.h"
#include <algorithm>
#include <vector>

using namespace srsgpu;

static_assert(sizeof(srsgpu_ssb_config) == 64, "srsgpu_ssb_config layout (mirrored by srsgpu)");

struct srsgpu_ssb_plan {
  srsgpu_context*           ctx = nullptr;
  device_buffer<ssb_desc>   d_descs;
  device_buffer<ssb_tables> d_tables;
  uint32_t                  nof_blocks    = 0;
  uint64_t                  payload_bytes = 0;  ///< The payload buffer must hold at least this many bytes.
};

namespace {

/// The subcarrier runs [begin, end) of the block that the reference writes on symbol s of the block.
struct run {
  uint32_t begin, end;
};
const std::vector<run>& written_runs(uint32_t s)
{
  static const std::vector<run> pss_only = {{56, 183}}, whole = {{0, 240}}, edges_and_sss = {{0, 48}, {56, 183}, {192, 240}};
  return s == 0 ? pss_only : s == 2 ? edges_and_sss : whole;
}

/// A run of one block on (grid, port, symbol), for the overlap check.
struct placed_run {
  uint64_t where;  ///< (grid, port, symbol)
  uint32_t begin, end, block;
};

} // namespace

extern "C" {

int srsgpu_ssb_plan_create(srsgpu_context*          ctx,
                           const srsgpu_ssb_config* cfgs,
                           uint32_t                 nof_blocks,
                           uint32_t                 grid_nof_prb,
                           uint32_t                 grid_nof_ports,
                           uint32_t                 nof_grids,
                           srsgpu_ssb_plan**        plan_out)
{
  if (const int err = check_grid_args(ctx, plan_out, cfgs, nof_blocks, grid_nof_prb, grid_nof_ports, nof_grids)) {
    return err;
  }
  const uint32_t nsc = 12 * grid_nof_prb, port_stride = 14 * nsc;
  std::vector<ssb_desc>   descs(nof_blocks);
  std::vector<placed_run> placed;
  uint64_t                payload_bytes = 0;
  for (uint32_t i = 0; i < nof_blocks; ++i) {
    const srsgpu_ssb_config& c = cfgs[i];
    ssb_block                b;
    b.phys_cell_id      = c.phys_cell_id;
    b.ssb_idx           = c.ssb_idx;
    b.L_max             = c.L_max;
    b.pattern_case      = c.pattern_case;
    b.common_scs        = c.common_scs;
    b.offset_to_pointA  = c.offset_to_pointA;
    b.subcarrier_offset = c.subcarrier_offset;
    b.slot_index        = c.slot_index;
    b.hrf               = c.hrf;
    b.nof_ports         = c.nof_ports;
    std::copy(c.ports, c.ports + 4, b.ports);
    b.pss_amplitude       = c.pss_amplitude;
    const std::string why = ssb_refusal(b, grid_nof_prb, grid_nof_ports);
    if (!why.empty()) {
      return fail(SRSGPU_ERR_INVALID_ARG, "block %u: %s", i, why.c_str());
    }
    if (c.grid_index >= nof_grids) {
      return fail(SRSGPU_ERR_INVALID_ARG, "block %u: grid_index %u is outside the %u grids", i, c.grid_index, nof_grids);
    }
    const uint32_t l_start = ssb_l_first(b.pattern_case, b.ssb_idx) % 14;
    uint32_t       k_start = 0;
    (void)ssb_k_first(b, k_start);
    for (uint32_t p = 0; p < b.nof_ports; ++p) {
      for (uint32_t s = 0; s < 4; ++s) {
        const uint64_t where = (static_cast<uint64_t>(c.grid_index) * 4 + b.ports[p]) * 14 + l_start + s;
        for (const run& r : written_runs(s)) {
          for (const placed_run& o : placed) {
            if (o.where == where && o.begin < k_start + r.end && k_start + r.begin < o.end) {
              return fail(SRSGPU_ERR_INVALID_ARG, "blocks %u and %u both write REs of symbol %u of port %u of grid %u: one "
                          "launch gives them no order", o.block, i, l_start + s, static_cast<unsigned>(b.ports[p]),
                          c.grid_index);
            }
          }
        }
      }
    }
    for (uint32_t p = 0; p < b.nof_ports; ++p) {
      for (uint32_t s = 0; s < 4; ++s) {
        for (const run& r : written_runs(s)) {
          placed.push_back({(static_cast<uint64_t>(c.grid_index) * 4 + b.ports[p]) * 14 + l_start + s, k_start + r.begin,
                            k_start + r.end, i});
        }
      }
    }
    ssb_desc& d = descs[i];
    d           = ssb_desc{};
    ssb_fill_desc(b, d);
    d.payload_offset = c.payload_offset;
    payload_bytes    = std::max<uint64_t>(payload_bytes, static_cast<uint64_t>(c.payload_offset) + 4);
    d.grid_base      = c.grid_index * grid_nof_ports * port_stride + l_start * nsc + k_start;
    d.nsc            = nsc;
    d.port_stride    = port_stride;
  }
  // The PBCH's code: K = 56, E = 864, n = 9, the (K, E) family of the PDCCH plan.
  std::vector<ssb_tables> tables(1);
  ssb_tables&             t = tables[0];
  ssb_fill_tables(t);
  polar_dl_code code;
  if (polar_dl_code_refusal(SSB_PBCH_K, SSB_PBCH_BITS) != nullptr) {
    return fail(SRSGPU_ERR_INVALID_ARG, "the PBCH polar code is refused");
  }
  polar_dl_code_build(SSB_PBCH_K, SSB_PBCH_BITS, code);
  if (code.n != 9 || code.u_source.size() != SSB_POLAR_N || code.gather.size() != SSB_PBCH_BITS) {
    return fail(SRSGPU_ERR_INVALID_ARG, "the PBCH polar code has unexpected sizes");
  }
  std::copy(code.u_source.begin(), code.u_source.end(), t.u_source);
  for (uint32_t r = 0; r < SSB_PBCH_BITS / 2; ++r) {
    t.gather[r] = code.gather[2 * r] | (static_cast<uint32_t>(code.gather[2 * r + 1]) << 16);
  }
  std::lock_guard<std::mutex> lock(ctx->mtx);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int r = ensure_gold_tables(ctx)) {
    return r;
  }
  plan_ptr<srsgpu_ssb_plan> plan(new srsgpu_ssb_plan());
  plan->ctx           = ctx;
  plan->nof_blocks    = nof_blocks;
  plan->payload_bytes = payload_bytes;
  if (nof_blocks > 0 && (!plan->d_descs.upload(descs) || !plan->d_tables.upload(tables))) {
    return fail(SRSGPU_ERR_HIP, "failed to upload the SSB tables");
  }
  *plan_out = plan.release();
  return SRSGPU_OK;
}

int srsgpu_ssb_plan_execute(const srsgpu_ssb_plan* plan,
                            const uint8_t*         d_payloads,
                            uint64_t               payload_bytes,
                            uint32_t*              d_grids,
                            void*                  stream)
{
  if (plan == nullptr || (plan->nof_blocks > 0 && (d_payloads == nullptr || d_grids == nullptr))) {
    return fail(SRSGPU_ERR_INVALID_ARG, "null argument");
  }
  if (payload_bytes < plan->payload_bytes) {
    return fail(SRSGPU_ERR_INVALID_ARG, "the payload buffer holds %llu bytes, the plan's blocks read %llu",
                static_cast<unsigned long long>(payload_bytes), static_cast<unsigned long long>(plan->payload_bytes));
  }
  launch_ssb(plan->d_descs.get(), plan->nof_blocks, plan->d_tables.get(), d_payloads, d_grids, plan->ctx->d_gold_x1.get(),
             plan->ctx->d_gold_x2_jump.get(), plan->ctx->d_gold_x2_lane.get(), static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return SRSGPU_OK;
}

void srsgpu_ssb_plan_destroy(srsgpu_ssb_plan* plan)
{
  if (plan == nullptr) {
    return;
  }
  delete plan;
}

} // extern "C"
