// Host side of the UCI polar decoder C ABI (include/srsgpu_phy.h): segments every field as
// uci_decoder_impl::decode_codeword_polar does (lib/phy/upper/channel_processors/uci/uci_decoder_impl.cpp:43), refuses
// what the reference's assertions refuse (polar_code_impl.cpp:334-407), builds the tables of every distinct (K, E) once
// (polar_code.cpp) and uploads them with the field descriptors. The decoding itself is uci_polar_decoder.hip.
#include "capi_internal.h"
#include "polar_code.h"
#include <algorithm>
#include <map>
#include <utility>
#include <vector>

using namespace srsgpu;

static_assert(sizeof(srsgpu_uci_polar_field_config) == 16, "srsgpu_uci_polar_field_config layout (mirrored by srsgpu)");

struct srsgpu_uci_polar_decoder_plan {
  srsgpu_context*       ctx        = nullptr;
  device_buffer<uci_polar_field_desc> d_fields;
  device_buffer<uci_polar_code_desc>  d_codes;
  device_buffer<uint32_t>             d_ops;
  device_buffer<uint16_t>             d_tables;
  uint32_t              nof_fields = 0;
  bool                  uses[3]    = {false, false, false};  ///< Sources some field reads.
};

namespace {

constexpr uint32_t MIN_BITS = 12, MAX_BITS = 1706;  // uci_decoder_impl.cpp:30 and uci_decoder_impl.h:74

} // namespace

extern "C" {

int srsgpu_uci_polar_decoder_plan_create(srsgpu_context*                      ctx,
                                         const srsgpu_uci_polar_field_config* cfgs,
                                         uint32_t                             nof_fields,
                                         srsgpu_uci_polar_decoder_plan**      plan_out)
{
  if (ctx == nullptr || plan_out == nullptr || (cfgs == nullptr && nof_fields > 0)) {
    return fail(SRSGPU_ERR_INVALID_ARG, "null argument");
  }
  std::vector<uci_polar_field_desc>                fields(nof_fields);
  std::vector<uci_polar_code_desc>                 codes;
  std::vector<uint32_t>                            ops;
  std::vector<uint16_t>                            tables;
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> code_index;
  std::vector<std::pair<uint64_t, uint32_t>>       words;  // (first output word, field), for the overlap check
  bool                                             uses[3] = {false, false, false};
  for (uint32_t f = 0; f < nof_fields; ++f) {
    const srsgpu_uci_polar_field_config& c = cfgs[f];
    const uint32_t                       A = c.nof_bits;
    if (A < MIN_BITS || A > MAX_BITS) {
      return fail(SRSGPU_ERR_INVALID_ARG, "field %u: nof_bits %u is outside 12..1706 (the polar-coded UCI sizes; 1..11 "
                  "bits are short block codes, srsgpu_uci_decoder_plan)", f, A);
    }
    if (c.source > 2) {
      return fail(SRSGPU_ERR_INVALID_ARG, "field %u: source %u is not 0, 1 or 2", f, static_cast<unsigned>(c.source));
    }
    const uci_polar_segmentation seg = uci_polar_segment(A, c.nof_enc_bits);
    if (const char* why = polar_code_refusal(seg.K, seg.E_cb)) {
      return fail(SRSGPU_ERR_INVALID_ARG, "field %u: %u bits in %u encoded bits (%u codeblock(s), K = %u, E = %u each): %s",
                  f, A, c.nof_enc_bits, seg.nof_codeblocks, seg.K, seg.E_cb, why);
    }
    const auto key = std::make_pair(seg.K, seg.E_cb);
    auto       it  = code_index.find(key);
    if (it == code_index.end()) {
      polar_code code;
      polar_code_build(seg.K, seg.E_cb, code);
      uci_polar_code_desc d{};
      d.ops_offset   = static_cast<uint32_t>(ops.size());
      d.nof_ops      = static_cast<uint32_t>(code.ops.size());
      d.demap_offset = static_cast<uint32_t>(tables.size());
      d.info_offset  = static_cast<uint32_t>(tables.size() + code.demap.size());
      d.K            = static_cast<uint16_t>(seg.K);
      d.n            = static_cast<uint8_t>(code.n);
      d.R            = static_cast<uint8_t>(code.demap.size() >> code.n);
      ops.insert(ops.end(), code.ops.begin(), code.ops.end());
      tables.insert(tables.end(), code.demap.begin(), code.demap.end());
      tables.insert(tables.end(), code.info.begin(), code.info.end());
      tables.insert(tables.end(), code.crc_weight.begin(), code.crc_weight.end());
      it = code_index.emplace(key, static_cast<uint32_t>(codes.size())).first;
      codes.push_back(d);
    }
    uci_polar_field_desc& d = fields[f];
    d                       = uci_polar_field_desc{};
    d.llr_offset            = c.llr_offset;
    d.E_cb                  = seg.E_cb;
    d.msg_word_offset       = c.msg_word_offset;
    d.code                  = it->second;
    d.nof_bits              = static_cast<uint16_t>(A);
    d.source                = c.source;
    d.nof_cb                = static_cast<uint8_t>(seg.nof_codeblocks);
    uses[c.source]          = true;
    words.emplace_back(c.msg_word_offset, f);
  }
  // Every field owns whole output words: two fields may not share one.
  std::sort(words.begin(), words.end());
  for (size_t i = 1; i < words.size(); ++i) {
    const uint32_t prev = words[i - 1].second;
    if (words[i - 1].first + (cfgs[prev].nof_bits + 31u) / 32u > words[i].first) {
      return fail(SRSGPU_ERR_INVALID_ARG, "fields %u and %u: their message words overlap (msg_word_offset %u with %u "
                  "bits, msg_word_offset %u)", prev, words[i].second, cfgs[prev].msg_word_offset,
                  static_cast<unsigned>(cfgs[prev].nof_bits), cfgs[words[i].second].msg_word_offset);
    }
  }
  std::lock_guard<std::mutex> lock(ctx->mtx);
  HIP_TRY(hipSetDevice(ctx->device));
  plan_ptr<srsgpu_uci_polar_decoder_plan> plan(new srsgpu_uci_polar_decoder_plan());
  plan->ctx        = ctx;
  plan->nof_fields = nof_fields;
  std::copy(uses, uses + 3, plan->uses);
  // With a field there is a code, and every code has operations and tables: none of the four is empty then.
  if (!plan->d_fields.upload(fields) || !plan->d_codes.upload(codes) || !plan->d_ops.upload(ops) ||
      !plan->d_tables.upload(tables)) {
    return fail(SRSGPU_ERR_HIP, "failed to upload the UCI polar decoder tables");
  }
  *plan_out = plan.release();
  return SRSGPU_OK;
}

int srsgpu_uci_polar_decoder_plan_execute(const srsgpu_uci_polar_decoder_plan* plan,
                                          const int8_t*                        d_src0,
                                          const int8_t*                        d_src1,
                                          const int8_t*                        d_src2,
                                          uint32_t*                            d_msgs,
                                          uint8_t*                             d_status,
                                          void*                                stream)
{
  if (plan == nullptr || (plan->nof_fields > 0 && (d_msgs == nullptr || d_status == nullptr))) {
    return fail(SRSGPU_ERR_INVALID_ARG, "null argument");
  }
  if ((plan->uses[0] && d_src0 == nullptr) || (plan->uses[1] && d_src1 == nullptr) ||
      (plan->uses[2] && d_src2 == nullptr)) {
    return fail(SRSGPU_ERR_INVALID_ARG, "an input stream the plan reads is NULL");
  }
  launch_uci_polar_decode(plan->d_fields.get(), plan->nof_fields, plan->d_codes.get(), plan->d_ops.get(),
                          plan->d_tables.get(), d_src0, d_src1, d_src2, d_msgs, d_status, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return SRSGPU_OK;
}

void srsgpu_uci_polar_decoder_plan_destroy(srsgpu_uci_polar_decoder_plan* plan)
{
  if (plan == nullptr) {
    return;
  }
  delete plan;
}

} // extern "C"
