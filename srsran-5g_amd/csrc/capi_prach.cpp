// Host side of the PRACH detector C ABI (include/srsgpu_phy.h): refuses what the reference's asserts refuse and what it
// leaves undefined, builds one job per (occasion, root sequence) (prach_host.cpp), computes one root-sequence row per
// distinct (L, u) in double and uploads jobs, rows and twiddles. Everything on the device is prach_detector.hip.
#include "capi_internal.h"
#include "host_util.h"
#include "prach_host.h"
#include <map>
#include <vector>

using namespace srsgpu;

static_assert(sizeof(srsgpu_prach_occasion) == 36, "srsgpu_prach_occasion layout (mirrored by srsgpu)");
static_assert(sizeof(srsgpu_prach_preamble) == 16, "srsgpu_prach_preamble layout (mirrored by srsgpu)");
static_assert(sizeof(srsgpu_prach_result) == 16 + 16 * SRSGPU_PRACH_MAX_PREAMBLES, "srsgpu_prach_result layout (mirrored by srsgpu)");

struct srsgpu_prach_detector_plan {
  srsgpu_context*          ctx = nullptr;
  device_buffer<prach_job> d_jobs;
  device_buffer<float>     d_roots;
  device_buffer<float>     d_twiddles;
  uint32_t                 nof_jobs = 0;
};

extern "C" {

int srsgpu_prach_detector_plan_create(srsgpu_context*              ctx,
                                      const srsgpu_prach_occasion* occasions,
                                      uint32_t                     nof_occasions,
                                      const uint16_t*              roots,
                                      uint32_t                     nof_roots,
                                      uint64_t                     input_words,
                                      srsgpu_prach_detector_plan** plan_out)
{
  if (ctx == nullptr || plan_out == nullptr || (occasions == nullptr && nof_occasions > 0) || (roots == nullptr && nof_roots > 0)) {
    return fail(SRSGPU_ERR_INVALID_ARG, "null argument");
  }
  std::vector<prach_job>                       jobs;
  std::vector<float>                           rows;
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> row_of;  // (L, u) -> float2 element of the row
  std::vector<uint8_t>                         taken(nof_occasions, 0);
  for (uint32_t i = 0; i < nof_occasions; ++i) {
    const srsgpu_prach_occasion& o = occasions[i];
    prach_derived                d;
    const std::string why = prach_refusal(o, roots, nof_roots, input_words, nof_occasions, d);
    if (!why.empty()) {
      return fail(SRSGPU_ERR_INVALID_ARG, "PRACH occasion %u: %s", i, why.c_str());
    }
    if (taken[o.result_index] != 0) {
      return fail(SRSGPU_ERR_INVALID_ARG, "PRACH occasion %u: result %u belongs to another occasion too", i, o.result_index);
    }
    taken[o.result_index] = 1;
    std::vector<uint32_t> root_rows(o.nof_roots);
    for (uint32_t s = 0; s < o.nof_roots; ++s) {
      const uint32_t u  = roots[o.root_offset + s];
      auto           it = row_of.find({d.L, u});
      if (it == row_of.end()) {
        it = row_of.emplace(std::make_pair(d.L, u), static_cast<uint32_t>(rows.size() / 2)).first;
        const std::vector<float> y = prach_root_sequence(d.L, u);
        rows.insert(rows.end(), y.begin(), y.end());
      }
      root_rows[s] = it->second;
    }
    prach_jobs(o, d, root_rows, jobs);
  }
  std::lock_guard<std::mutex> lock(ctx->mtx);
  HIP_TRY(hipSetDevice(ctx->device));
  plan_ptr<srsgpu_prach_detector_plan> plan(new srsgpu_prach_detector_plan());
  plan->ctx      = ctx;
  plan->nof_jobs = static_cast<uint32_t>(jobs.size());
  if (!plan->d_jobs.upload(jobs) || !plan->d_roots.upload(rows) || !plan->d_twiddles.upload(unit_roots(PRACH_LONG_N))) {
    return fail(SRSGPU_ERR_HIP, "failed to upload the PRACH detector tables");
  }
  *plan_out = plan.release();
  return SRSGPU_OK;
}

int srsgpu_prach_detector_plan_execute(const srsgpu_prach_detector_plan* plan,
                                       const uint32_t*                   d_input,
                                       srsgpu_prach_result*              d_results,
                                       void*                             stream)
{
  if (plan == nullptr || (plan->nof_jobs > 0 && (d_input == nullptr || d_results == nullptr))) {
    return fail(SRSGPU_ERR_INVALID_ARG, "null argument");
  }
  launch_prach_detector(plan->d_jobs.get(), plan->nof_jobs, plan->d_roots.get(), plan->d_twiddles.get(), d_input, d_results,
                        static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return SRSGPU_OK;
}

void srsgpu_prach_detector_plan_destroy(srsgpu_prach_detector_plan* plan)
{
  if (plan == nullptr) {
    return;
  }
  delete plan;
}

int srsgpu_prach_max_delay_samples(uint32_t format, uint32_t ra_scs, uint32_t n_cs, uint32_t* max_delay_samples)
{
  prach_derived d;
  if (max_delay_samples == nullptr) {
    return fail(SRSGPU_ERR_INVALID_ARG, "null argument");
  }
  if (!prach_derive(format, ra_scs, n_cs, d) || n_cs > d.L) {
    return fail(SRSGPU_ERR_INVALID_ARG, "PRACH format %u has no preamble information at SCS %u with N_cs %u", format, ra_scs, n_cs);
  }
  *max_delay_samples = d.max_delay_samples;
  return SRSGPU_OK;
}

} // extern "C"
