// Host side of the PUCCH Format 3 / 4 C ABI (include/srsgpu_phy.h): refuses what the reference's validators and
// assertions refuse and what they leave undefined, builds one job per PDU (pucch_f34_host.cpp) with its DM-RS
// sequences and scrambling words, one table of roots per transform size in use, and uploads jobs and tables.
// Everything on the device is pucch_f34.hip.
#include "capi_internal.h"
#include "host_util.h"
#include "pucch_f34_host.h"
#include <vector>

using namespace srsgpu;

static_assert(sizeof(srsgpu_pucch_f34_config) == 40, "srsgpu_pucch_f34_config layout (mirrored by srsgpu)");

struct srsgpu_pucch_f34_plan {
  srsgpu_context*              ctx = nullptr;
  device_buffer<pucch_f34_job> d_jobs;
  device_buffer<float>         d_dmrs;
  device_buffer<uint32_t>      d_scrambling;
  device_buffer<float>         d_roots;
  uint32_t                     nof_jobs = 0;
};

extern "C" {

int srsgpu_pucch_f34_plan_create(srsgpu_context*                ctx,
                                 const srsgpu_pucch_f34_config* pdus,
                                 uint32_t                       nof_pdus,
                                 uint32_t                       grid_nof_prb,
                                 uint32_t                       grid_nof_ports,
                                 uint32_t                       nof_grids,
                                 srsgpu_pucch_f34_plan**        plan_out)
{
  if (const int err = check_grid_args(ctx, plan_out, pdus, nof_pdus, grid_nof_prb, grid_nof_ports, nof_grids)) {
    return err;
  }
  std::vector<pucch_f34_job> jobs;
  std::vector<float>         dmrs, roots;
  std::vector<uint32_t>      scrambling;
  uint32_t                   root_row[PUCCH_F34_MAX_PRB + 1];
  for (uint32_t& r : root_row) {
    r = 0xffffffffu;
  }
  jobs.reserve(nof_pdus);
  for (uint32_t i = 0; i < nof_pdus; ++i) {
    const srsgpu_pucch_f34_config& c   = pdus[i];
    const std::string              why = pucch_f34_refusal(c, grid_nof_prb, grid_nof_ports, nof_grids);
    if (!why.empty()) {
      return fail(SRSGPU_ERR_INVALID_ARG, "PUCCH Format 3/4 PDU %u: %s", i, why.c_str());
    }
    if (root_row[c.nof_prb] == 0xffffffffu) {
      const std::vector<float> t = unit_roots(12u * c.nof_prb);
      root_row[c.nof_prb]        = static_cast<uint32_t>(roots.size() / 2);
      roots.insert(roots.end(), t.begin(), t.end());
    }
    const uint32_t dmrs_row = static_cast<uint32_t>(dmrs.size() / 2);
    pucch_f34_job  job = pucch_f34_make_job(c, grid_nof_prb, grid_nof_ports, dmrs_row, root_row[c.nof_prb],
                                            static_cast<uint32_t>(scrambling.size()));
    for (uint32_t s = 0; s < job.nof_dmrs; ++s) {
      const std::vector<float> seq = pucch_f34_dmrs(c, job.dmrs_symbol[s]);
      if (seq.size() != 24u * c.nof_prb) {
        return fail(SRSGPU_ERR_INVALID_ARG, "PUCCH Format 3/4 PDU %u: no low-PAPR sequence of length %u", i, 12u * c.nof_prb);
      }
      dmrs.insert(dmrs.end(), seq.begin(), seq.end());
    }
    const std::vector<uint32_t> words = pucch_f34_scrambling(c, job.nof_llrs);
    scrambling.insert(scrambling.end(), words.begin(), words.end());
    jobs.push_back(job);
  }
  const std::string overlap = pucch_f34_llr_overlap(pdus, nof_pdus);
  if (!overlap.empty()) {
    return fail(SRSGPU_ERR_INVALID_ARG, "PUCCH Format 3/4: %s", overlap.c_str());
  }
  std::lock_guard<std::mutex> lock(ctx->mtx);
  HIP_TRY(hipSetDevice(ctx->device));
  plan_ptr<srsgpu_pucch_f34_plan> plan(new srsgpu_pucch_f34_plan());
  plan->ctx      = ctx;
  plan->nof_jobs = static_cast<uint32_t>(jobs.size());
  if (!plan->d_jobs.upload(jobs) || !plan->d_dmrs.upload(dmrs) || !plan->d_scrambling.upload(scrambling) ||
      !plan->d_roots.upload(roots)) {
    return fail(SRSGPU_ERR_HIP, "failed to upload the PUCCH Format 3/4 tables");
  }
  *plan_out = plan.release();
  return SRSGPU_OK;
}

int srsgpu_pucch_f34_plan_execute(const srsgpu_pucch_f34_plan* plan,
                                  const uint32_t*              d_grids,
                                  int8_t*                      d_llrs,
                                  srsgpu_pucch_f2_result*      d_results,
                                  void*                        stream)
{
  if (plan == nullptr || (plan->nof_jobs > 0 && (d_grids == nullptr || d_llrs == nullptr || d_results == nullptr))) {
    return fail(SRSGPU_ERR_INVALID_ARG, "null argument");
  }
  if ((reinterpret_cast<uintptr_t>(d_llrs) & 3u) != 0) {
    return fail(SRSGPU_ERR_INVALID_ARG, "d_llrs is not 4-byte aligned");
  }
  launch_pucch_f34(plan->d_jobs.get(), plan->nof_jobs, plan->d_dmrs.get(), plan->d_scrambling.get(),
                   plan->d_roots.get(), d_grids, d_llrs, d_results, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return SRSGPU_OK;
}

void srsgpu_pucch_f34_plan_destroy(srsgpu_pucch_f34_plan* plan)
{
  if (plan == nullptr) {
    return;
  }
  delete plan;
}

} // extern "C"
