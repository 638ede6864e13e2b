// Host side of the PUCCH detector C ABI (include/srsgpu_phy.h): refuses what the reference's validators and asserts
// refuse and what it leaves undefined, builds one job per Format 0 PDU and Format 1 resource (pucch_host.cpp) and
// uploads them with the entry words and the orthogonal sequences. Everything on the device is pucch_detector.hip.
#include "capi_internal.h"
#include "pucch_host.h"
#include <vector>

using namespace srsgpu;

static_assert(sizeof(srsgpu_pucch_f0_config) == 24, "srsgpu_pucch_f0_config layout (mirrored by srsgpu)");
static_assert(sizeof(srsgpu_pucch_f1_resource) == 28, "srsgpu_pucch_f1_resource layout (mirrored by srsgpu)");
static_assert(sizeof(srsgpu_pucch_f1_entry) == 4, "srsgpu_pucch_f1_entry layout (mirrored by srsgpu)");
static_assert(sizeof(srsgpu_pucch_result) == 32, "srsgpu_pucch_result layout (mirrored by srsgpu)");

struct srsgpu_pucch_detector_plan {
  srsgpu_context*          ctx = nullptr;
  device_buffer<pucch_job> d_jobs;
  device_buffer<uint32_t>  d_entries;
  device_buffer<float>     d_w;
  uint32_t                 nof_jobs = 0;
};

extern "C" {

int srsgpu_pucch_detector_plan_create(srsgpu_context*                 ctx,
                                      const srsgpu_pucch_f0_config*   f0,
                                      uint32_t                        nof_f0,
                                      const srsgpu_pucch_f1_resource* f1_resources,
                                      uint32_t                        nof_f1,
                                      const srsgpu_pucch_f1_entry*    f1_entries,
                                      uint32_t                        nof_entries,
                                      uint32_t                        grid_nof_prb,
                                      uint32_t                        grid_nof_ports,
                                      uint32_t                        nof_grids,
                                      srsgpu_pucch_detector_plan**    plan_out)
{
  if ((f1_resources == nullptr && nof_f1 > 0) || (f1_entries == nullptr && nof_entries > 0)) {
    return fail(SRSGPU_ERR_INVALID_ARG, "null argument");
  }
  if (const int err = check_grid_args(ctx, plan_out, f0, nof_f0, grid_nof_prb, grid_nof_ports, nof_grids)) {
    return err;
  }
  std::vector<pucch_job> jobs;
  std::vector<uint32_t>  entry_words(nof_entries, 0);
  std::vector<uint8_t>   owned(nof_entries, 0);
  jobs.reserve(static_cast<size_t>(nof_f0) + nof_f1);
  for (uint32_t i = 0; i < nof_f0; ++i) {
    const std::string why = pucch_f0_refusal(f0[i], grid_nof_prb, grid_nof_ports, nof_grids);
    if (!why.empty()) {
      return fail(SRSGPU_ERR_INVALID_ARG, "Format 0 PDU %u: %s", i, why.c_str());
    }
    jobs.push_back(pucch_f0_job(f0[i], grid_nof_prb, grid_nof_ports, i));
  }
  for (uint32_t i = 0; i < nof_f1; ++i) {
    const srsgpu_pucch_f1_resource& r = f1_resources[i];
    const std::string why = pucch_f1_refusal(r, f1_entries, nof_entries, grid_nof_prb, grid_nof_ports, nof_grids);
    if (!why.empty()) {
      return fail(SRSGPU_ERR_INVALID_ARG, "Format 1 resource %u: %s", i, why.c_str());
    }
    for (uint32_t e = r.first_entry; e < r.first_entry + r.nof_entries; ++e) {
      if (owned[e] != 0) {
        return fail(SRSGPU_ERR_INVALID_ARG, "Format 1 resource %u: entry %u belongs to another resource too", i, e);
      }
      owned[e]       = 1;
      entry_words[e] = f1_entries[e].initial_cyclic_shift | (static_cast<uint32_t>(f1_entries[e].time_domain_occ) << 8) |
                       (static_cast<uint32_t>(f1_entries[e].nof_harq_ack) << 16);
    }
    jobs.push_back(pucch_f1_job(r, f1_entries, grid_nof_prb, grid_nof_ports, nof_f0 + r.first_entry));
  }
  for (uint32_t e = 0; e < nof_entries; ++e) {
    if (owned[e] == 0) {
      return fail(SRSGPU_ERR_INVALID_ARG, "Format 1 entry %u belongs to no resource: its result would stay unwritten", e);
    }
  }
  std::lock_guard<std::mutex> lock(ctx->mtx);
  HIP_TRY(hipSetDevice(ctx->device));
  plan_ptr<srsgpu_pucch_detector_plan> plan(new srsgpu_pucch_detector_plan());
  plan->ctx      = ctx;
  plan->nof_jobs = static_cast<uint32_t>(jobs.size());
  if (!plan->d_jobs.upload(jobs) || !plan->d_entries.upload(entry_words) || !plan->d_w.upload(pucch_w_table())) {
    return fail(SRSGPU_ERR_HIP, "failed to upload the PUCCH detector tables");
  }
  *plan_out = plan.release();
  return SRSGPU_OK;
}

int srsgpu_pucch_detector_plan_execute(const srsgpu_pucch_detector_plan* plan,
                                       const uint32_t*                   d_grids,
                                       srsgpu_pucch_result*              d_results,
                                       void*                             stream)
{
  if (plan == nullptr || (plan->nof_jobs > 0 && (d_grids == nullptr || d_results == nullptr))) {
    return fail(SRSGPU_ERR_INVALID_ARG, "null argument");
  }
  launch_pucch_detector(plan->d_jobs.get(), plan->nof_jobs, plan->d_entries.get(), plan->d_w.get(), d_grids, d_results,
                        static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return SRSGPU_OK;
}

void srsgpu_pucch_detector_plan_destroy(srsgpu_pucch_detector_plan* plan)
{
  if (plan == nullptr) {
    return;
  }
  delete plan;
}

} // extern "C"
