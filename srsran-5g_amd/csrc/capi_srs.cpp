// Host side of the SRS estimator C ABI (include/srsgpu_phy.h): refuses what the reference's validator and assertions
// refuse and what it leaves undefined, builds one job per resource (srs_host.cpp), computes one sequence row per distinct
// (u, L, cyclic shift / n_cs_max) in double and uploads jobs, rows and the phase table. Everything on the device is
// srs_estimator.hip.
#include "capi_internal.h"
#include "host_util.h"
#include "srs_host.h"
#include <map>
#include <tuple>
#include <vector>

using namespace srsgpu;

static_assert(sizeof(srsgpu_srs_config) == 44, "srsgpu_srs_config layout (mirrored by srsgpu)");
static_assert(sizeof(srsgpu_srs_result) == 192, "srsgpu_srs_result layout (mirrored by srsgpu)");

struct srsgpu_srs_estimator_plan {
  srsgpu_context*        ctx = nullptr;
  device_buffer<srs_job> d_jobs;
  device_buffer<float>   d_seqs;
  device_buffer<float>   d_cexp;
  uint32_t               nof_jobs = 0;
};

extern "C" {

int srsgpu_srs_estimator_plan_create(srsgpu_context*             ctx,
                                     const srsgpu_srs_config*    resources,
                                     uint32_t                    nof_resources,
                                     uint32_t                    grid_nof_prb,
                                     uint32_t                    grid_nof_ports,
                                     uint32_t                    nof_grids,
                                     srsgpu_srs_estimator_plan** plan_out)
{
  if (const int err = check_grid_args(ctx, plan_out, resources, nof_resources, grid_nof_prb, grid_nof_ports, nof_grids)) {
    return err;
  }
  std::vector<srs_job>                                         jobs;
  std::vector<float>                                           rows;
  std::map<std::tuple<uint32_t, uint32_t, uint32_t>, uint32_t> row_of;  // (u, L, n_cs 24 / n_cs_max) -> float2 element
  std::vector<uint8_t>                                         taken(nof_resources, 0);
  jobs.reserve(nof_resources);
  for (uint32_t i = 0; i < nof_resources; ++i) {
    const srsgpu_srs_config& c = resources[i];
    srs_derived              d;
    const std::string        why = srs_refusal(c, grid_nof_prb, grid_nof_ports, nof_grids, nof_resources, d);
    if (!why.empty()) {
      return fail(SRSGPU_ERR_INVALID_ARG, "SRS resource %u: %s", i, why.c_str());
    }
    if (taken[c.result_index] != 0) {
      return fail(SRSGPU_ERR_INVALID_ARG, "SRS resource %u: result %u belongs to another resource too", i, c.result_index);
    }
    taken[c.result_index] = 1;
    uint32_t seq_rows[4] = {0, 0, 0, 0};
    for (uint32_t p = 0; p < c.nof_antenna_ports; ++p) {
      const auto key = std::make_tuple(d.u, d.L, d.n_cs[p] * 24u / d.n_cs_max);
      auto       it  = row_of.find(key);
      if (it == row_of.end()) {
        const std::vector<float> s = srs_sequence(d.u, d.L, d.n_cs[p], d.n_cs_max);
        if (s.size() != 2 * static_cast<size_t>(d.L)) {
          return fail(SRSGPU_ERR_INVALID_ARG, "SRS resource %u: no low-PAPR sequence of length %u", i, d.L);
        }
        it = row_of.emplace(key, static_cast<uint32_t>(rows.size() / 2)).first;
        rows.insert(rows.end(), s.begin(), s.end());
      }
      seq_rows[p] = it->second;
    }
    jobs.push_back(srs_make_job(c, d, seq_rows, grid_nof_prb, grid_nof_ports));
  }
  std::lock_guard<std::mutex> lock(ctx->mtx);
  HIP_TRY(hipSetDevice(ctx->device));
  plan_ptr<srsgpu_srs_estimator_plan> plan(new srsgpu_srs_estimator_plan());
  plan->ctx      = ctx;
  plan->nof_jobs = static_cast<uint32_t>(jobs.size());
  if (!plan->d_jobs.upload(jobs) || !plan->d_seqs.upload(rows) || !plan->d_cexp.upload(unit_roots(SRS_CEXP_SIZE))) {
    return fail(SRSGPU_ERR_HIP, "failed to upload the SRS estimator tables");
  }
  *plan_out = plan.release();
  return SRSGPU_OK;
}

int srsgpu_srs_estimator_plan_execute(const srsgpu_srs_estimator_plan* plan,
                                      const uint32_t*                  d_grids,
                                      srsgpu_srs_result*               d_results,
                                      void*                            stream)
{
  if (plan == nullptr || (plan->nof_jobs > 0 && (d_grids == nullptr || d_results == nullptr))) {
    return fail(SRSGPU_ERR_INVALID_ARG, "null argument");
  }
  launch_srs_estimator(plan->d_jobs.get(), plan->nof_jobs, plan->d_seqs.get(), plan->d_cexp.get(), d_grids, d_results,
                       static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return SRSGPU_OK;
}

void srsgpu_srs_estimator_plan_destroy(srsgpu_srs_estimator_plan* plan)
{
  if (plan == nullptr) {
    return;
  }
  delete plan;
}

} // extern "C"
