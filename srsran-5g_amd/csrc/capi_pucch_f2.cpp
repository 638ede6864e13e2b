// Host side of the PUCCH Format 2 C ABI (include/srsgpu_phy.h): refuses what the reference's validator and assertions
// refuse and what they leave undefined, builds one job per PDU (pucch_f2_host.cpp) with its DM-RS symbols and scrambling
// words and uploads jobs and tables. Everything on the device is pucch_f2.hip.
#include "capi_internal.h"
#include "host_util.h"
#include "pucch_f2_host.h"
#include <vector>

using namespace srsgpu;

static_assert(sizeof(srsgpu_pucch_f2_config) == 32, "srsgpu_pucch_f2_config layout (mirrored by srsgpu)");
static_assert(sizeof(srsgpu_pucch_f2_result) == 96, "srsgpu_pucch_f2_result layout (mirrored by srsgpu)");

struct srsgpu_pucch_f2_plan {
  srsgpu_context*             ctx = nullptr;
  device_buffer<pucch_f2_job> d_jobs;
  device_buffer<float>        d_dmrs;
  device_buffer<uint32_t>     d_scrambling;
  device_buffer<float>        d_twiddles;
  uint32_t                    nof_jobs = 0;
};

extern "C" {

int srsgpu_pucch_f2_plan_create(srsgpu_context*               ctx,
                                const srsgpu_pucch_f2_config* pdus,
                                uint32_t                      nof_pdus,
                                uint32_t                      grid_nof_prb,
                                uint32_t                      grid_nof_ports,
                                uint32_t                      nof_grids,
                                srsgpu_pucch_f2_plan**        plan_out)
{
  if (const int err = check_grid_args(ctx, plan_out, pdus, nof_pdus, grid_nof_prb, grid_nof_ports, nof_grids)) {
    return err;
  }
  std::vector<pucch_f2_job> jobs;
  std::vector<float>        dmrs;
  std::vector<uint32_t>     scrambling;
  jobs.reserve(nof_pdus);
  for (uint32_t i = 0; i < nof_pdus; ++i) {
    const srsgpu_pucch_f2_config& c   = pdus[i];
    const std::string             why = pucch_f2_refusal(c, grid_nof_prb, grid_nof_ports, nof_grids);
    if (!why.empty()) {
      return fail(SRSGPU_ERR_INVALID_ARG, "PUCCH Format 2 PDU %u: %s", i, why.c_str());
    }
    uint32_t rows[2] = {0, 0};
    for (uint32_t s = 0; s < c.nof_symbols; ++s) {
      const std::vector<float> seq = pucch_f2_dmrs(c, s);
      rows[s]                      = static_cast<uint32_t>(dmrs.size() / 2);
      dmrs.insert(dmrs.end(), seq.begin(), seq.end());
    }
    uint32_t words[PUCCH_F2_SCR_WORDS];
    pucch_f2_scrambling(c, words);
    jobs.push_back(pucch_f2_make_job(c, grid_nof_prb, grid_nof_ports, rows, static_cast<uint32_t>(scrambling.size())));
    scrambling.insert(scrambling.end(), words, words + PUCCH_F2_SCR_WORDS);
  }
  const std::string overlap = pucch_f2_llr_overlap(pdus, nof_pdus);
  if (!overlap.empty()) {
    return fail(SRSGPU_ERR_INVALID_ARG, "PUCCH Format 2: %s", overlap.c_str());
  }
  std::lock_guard<std::mutex> lock(ctx->mtx);
  HIP_TRY(hipSetDevice(ctx->device));
  plan_ptr<srsgpu_pucch_f2_plan> plan(new srsgpu_pucch_f2_plan());
  plan->ctx      = ctx;
  plan->nof_jobs = static_cast<uint32_t>(jobs.size());
  if (!plan->d_jobs.upload(jobs) || !plan->d_dmrs.upload(dmrs) || !plan->d_scrambling.upload(scrambling) ||
      !plan->d_twiddles.upload(unit_roots(PUCCH_F2_DFT))) {
    return fail(SRSGPU_ERR_HIP, "failed to upload the PUCCH Format 2 tables");
  }
  *plan_out = plan.release();
  return SRSGPU_OK;
}

int srsgpu_pucch_f2_plan_execute(const srsgpu_pucch_f2_plan* plan,
                                 const uint32_t*             d_grids,
                                 int8_t*                     d_llrs,
                                 srsgpu_pucch_f2_result*     d_results,
                                 void*                       stream)
{
  if (plan == nullptr || (plan->nof_jobs > 0 && (d_grids == nullptr || d_llrs == nullptr || d_results == nullptr))) {
    return fail(SRSGPU_ERR_INVALID_ARG, "null argument");
  }
  launch_pucch_f2(plan->d_jobs.get(), plan->nof_jobs, plan->d_dmrs.get(), plan->d_scrambling.get(),
                  plan->d_twiddles.get(), d_grids, d_llrs, d_results, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return SRSGPU_OK;
}

void srsgpu_pucch_f2_plan_destroy(srsgpu_pucch_f2_plan* plan)
{
  if (plan == nullptr) {
    return;
  }
  delete plan;
}

} // extern "C"
