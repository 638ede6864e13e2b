// Host side of the UCI decoder C ABI (include/srsgpu_phy.h): validates the fields, fixes each one's detection constants
// (the minimum count of non-zero LLRs of calculate_uci_min_encoded_bits, include/srsran/ran/uci/uci_info.h:85, and the
// GLRT threshold of short_block_detector_impl.cpp:221) and uploads the descriptors. The decoding itself is
// uci_decoder.hip.
#include "capi_internal.h"
#include <algorithm>
#include <vector>

using namespace srsgpu;

static_assert(sizeof(srsgpu_uci_field_config) == 12, "srsgpu_uci_field_config layout (mirrored by srsgpu)");

struct srsgpu_uci_decoder_plan {
  srsgpu_context* ctx        = nullptr;
  device_buffer<uci_field_desc> d_desc;
  uint32_t        nof_fields = 0;
  bool            uses[3]    = {false, false, false};  ///< Sources some field reads.
};

namespace {

constexpr uint8_t MIN_NONZERO[11] = {2, 3, 9, 10, 11, 12, 13, 14, 14, 15, 17};
constexpr uint8_t THRESHOLD[11]   = {0, 0, 12, 14, 16, 18, 20, 22, 24, 26, 29};
/// Far above any PUSCH's capacity (275 PRB x 14 symbols x 4 layers x 8 bits); keeps the kernel's block arithmetic in
/// 32 bits.
constexpr uint32_t MAX_ENC_BITS = 1u << 24;

} // namespace

extern "C" {

int srsgpu_uci_decoder_plan_create(srsgpu_context*                ctx,
                                   const srsgpu_uci_field_config* cfgs,
                                   uint32_t                       nof_fields,
                                   srsgpu_uci_decoder_plan**      plan_out)
{
  if (ctx == nullptr || plan_out == nullptr || (cfgs == nullptr && nof_fields > 0)) {
    return fail(SRSGPU_ERR_INVALID_ARG, "null argument");
  }
  std::vector<uci_field_desc> descs(nof_fields);
  bool                        uses[3] = {false, false, false};
  for (uint32_t f = 0; f < nof_fields; ++f) {
    const srsgpu_uci_field_config& c  = cfgs[f];
    const uint32_t                 qm = c.modulation_order;
    if (c.nof_bits == 0) {
      return fail(SRSGPU_ERR_INVALID_ARG, "field %u: nof_bits is 0 (a UCI field has 1..11 bits here)", f);
    }
    if (c.nof_bits > 11) {
      return fail(SRSGPU_ERR_INVALID_ARG, "field %u: %u bits: polar-coded UCI (12 bits and more) is not implemented, "
                  "only the short block codes of 1..11 bits", f, static_cast<unsigned>(c.nof_bits));
    }
    if (qm != 1 && qm != 2 && qm != 4 && qm != 6 && qm != 8) {
      return fail(SRSGPU_ERR_INVALID_ARG, "field %u: modulation_order %u is not 1, 2, 4, 6 or 8", f, qm);
    }
    if (c.source > 2) {
      return fail(SRSGPU_ERR_INVALID_ARG, "field %u: source %u is not 0, 1 or 2", f, static_cast<unsigned>(c.source));
    }
    if (c.nof_enc_bits > MAX_ENC_BITS) {
      return fail(SRSGPU_ERR_INVALID_ARG, "field %u: nof_enc_bits %u exceeds %u", f, c.nof_enc_bits, MAX_ENC_BITS);
    }
    uci_field_desc& d = descs[f];
    d                 = uci_field_desc{};
    d.llr_offset      = c.llr_offset;
    d.nof_enc         = c.nof_enc_bits;
    d.nof_bits        = c.nof_bits;
    d.qm              = c.modulation_order;
    d.source          = c.source;
    d.min_nonzero     = MIN_NONZERO[c.nof_bits - 1];
    d.threshold       = THRESHOLD[c.nof_bits - 1];
    uses[c.source]    = true;
  }
  std::lock_guard<std::mutex> lock(ctx->mtx);
  HIP_TRY(hipSetDevice(ctx->device));
  plan_ptr<srsgpu_uci_decoder_plan> plan(new srsgpu_uci_decoder_plan());
  plan->ctx        = ctx;
  plan->nof_fields = nof_fields;
  std::copy(uses, uses + 3, plan->uses);
  if (!plan->d_desc.upload(descs)) {
    return fail(SRSGPU_ERR_HIP, "failed to upload the UCI field descriptors");
  }
  *plan_out = plan.release();
  return SRSGPU_OK;
}

int srsgpu_uci_decoder_plan_execute(const srsgpu_uci_decoder_plan* plan,
                                    const int8_t*                  d_src0,
                                    const int8_t*                  d_src1,
                                    const int8_t*                  d_src2,
                                    uint16_t*                      d_msgs,
                                    uint8_t*                       d_status,
                                    void*                          stream)
{
  if (plan == nullptr || (plan->nof_fields > 0 && (d_msgs == nullptr || d_status == nullptr))) {
    return fail(SRSGPU_ERR_INVALID_ARG, "null argument");
  }
  if ((plan->uses[0] && d_src0 == nullptr) || (plan->uses[1] && d_src1 == nullptr) ||
      (plan->uses[2] && d_src2 == nullptr)) {
    return fail(SRSGPU_ERR_INVALID_ARG, "an input stream the plan reads is NULL");
  }
  launch_uci_decode(plan->d_desc.get(), plan->nof_fields, d_src0, d_src1, d_src2, d_msgs, d_status,
                    static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return SRSGPU_OK;
}

void srsgpu_uci_decoder_plan_destroy(srsgpu_uci_decoder_plan* plan)
{
  if (plan == nullptr) {
    return;
  }
  delete plan;
}

} // extern "C"
