// Host side of the PDCCH C ABI (include/srsgpu_phy.h): refuses what pdcch_processor_impl::process refuses
// (pdcch_host.cpp), maps every DCI's CCEs to PRBs, builds the downlink polar code tables of every distinct (K, E) once
// (polar_code.cpp) and uploads them with the DCI descriptors. Everything on the device is pdcch.hip.
#include "capi_internal.h"
#include "pdcch_host.h"
#include "polar_code.h"
#include <algorithm>
#include <cmath>
#include <map>
#include <unordered_map>
#include <utility>
#include <vector>

using namespace srsgpu;

static_assert(sizeof(srsgpu_pdcch_config) == 128, "srsgpu_pdcch_config layout (mirrored by srsgpu)");

struct srsgpu_pdcch_plan {
  srsgpu_context*  ctx           = nullptr;
  device_buffer<pdcch_desc>      d_descs;
  device_buffer<pdcch_code_desc> d_codes;
  device_buffer<uint8_t>         d_u_source;
  device_buffer<uint32_t>        d_gather;
  device_buffer<uint16_t>        d_prbs;
  device_buffer<uint32_t>        d_crc_weights;
  uint32_t         nof_dcis      = 0;
  uint64_t         payload_bytes = 0;  ///< The payload buffer must hold at least this many bytes.
};

namespace {

constexpr uint32_t CRC24C_POLY = 0x1b2b117;

/// x^(24 + j) mod g_CRC24C (crc_calculator_generic_impl.cpp:40: 0x1b2b117), j = 0..PDCCH_CRC_WEIGHTS-1.
std::vector<uint32_t> crc24c_weights()
{
  std::vector<uint32_t> w(PDCCH_CRC_WEIGHTS);
  uint32_t              power = CRC24C_POLY & 0xffffffu;
  for (uint32_t j = 0; j < PDCCH_CRC_WEIGHTS; ++j) {
    w[j] = power;
    power <<= 1;
    if ((power >> 24) != 0) {
      power ^= CRC24C_POLY;
    }
  }
  return w;
}

} // namespace

extern "C" {

int srsgpu_pdcch_plan_create(srsgpu_context*            ctx,
                             const srsgpu_pdcch_config* cfgs,
                             uint32_t                   nof_dcis,
                             uint32_t                   grid_nof_prb,
                             uint32_t                   grid_nof_ports,
                             uint32_t                   nof_grids,
                             srsgpu_pdcch_plan**        plan_out)
{
  if (const int err = check_grid_args(ctx, plan_out, cfgs, nof_dcis, grid_nof_prb, grid_nof_ports, nof_grids)) {
    return err;
  }
  const uint32_t nsc = 12 * grid_nof_prb, port_stride = 14 * nsc;
  const std::vector<uint32_t>                       crc_w = crc24c_weights();
  std::vector<pdcch_desc>                           descs(nof_dcis);
  std::vector<pdcch_code_desc>                      codes;
  std::vector<uint8_t>                              u_source;
  std::vector<uint32_t>                             gather;
  std::vector<uint16_t>                             prb_table;
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> code_index;
  std::unordered_map<uint64_t, uint32_t>            owner;  // (grid, symbol, PRB) -> DCI, for the overlap check
  uint64_t                                          payload_bytes = 0;
  for (uint32_t i = 0; i < nof_dcis; ++i) {
    const srsgpu_pdcch_config& c = cfgs[i];
    pdcch_alloc                a;
    a.bwp_size_rb         = c.bwp_size_rb;
    a.bwp_start_rb        = c.bwp_start_rb;
    a.start_symbol        = c.start_symbol_index;
    a.duration            = c.duration;
    a.frequency_resources = c.frequency_resources;
    a.mapping             = c.cce_to_reg_mapping;
    a.reg_bundle_size     = c.reg_bundle_size;
    a.interleaver_size    = c.interleaver_size;
    a.shift_index         = c.shift_index;
    a.cce_index           = c.cce_index;
    a.aggregation_level   = c.aggregation_level;
    a.nof_payload_bits    = c.nof_payload_bits;
    a.nof_ports           = c.nof_ports;
    const std::string why = pdcch_refusal(a, grid_nof_prb, grid_nof_ports);
    if (!why.empty()) {
      return fail(SRSGPU_ERR_INVALID_ARG, "DCI %u: %s", i, why.c_str());
    }
    if (c.rnti > 0xffff || c.n_rnti > 0xffff || c.n_id_pdcch_data > 0xffff || c.n_id_pdcch_dmrs > 0xffff ||
        c.slot_index >= 160) {
      return fail(SRSGPU_ERR_INVALID_ARG, "DCI %u: rnti %u, n_rnti %u, n_id_pdcch_data %u or n_id_pdcch_dmrs %u exceeds 16 "
                  "bits, or slot_index %u exceeds 159", i, c.rnti, c.n_rnti, c.n_id_pdcch_data, c.n_id_pdcch_dmrs, c.slot_index);
    }
    if (c.grid_index >= nof_grids) {
      return fail(SRSGPU_ERR_INVALID_ARG, "DCI %u: grid_index %u is outside the %u grids", i, c.grid_index, nof_grids);
    }
    const std::vector<uint16_t> prbs = pdcch_prbs(a);
    for (uint32_t s = 0; s < a.duration; ++s) {
      for (uint16_t prb : prbs) {
        const uint64_t key = (static_cast<uint64_t>(c.grid_index) * 14 + a.start_symbol + s) * 275 + prb;
        const auto     ins = owner.emplace(key, i);
        if (!ins.second) {
          return fail(SRSGPU_ERR_INVALID_ARG, "DCIs %u and %u both write PRB %u of symbol %u of grid %u: one launch gives "
                      "them no order", ins.first->second, i, static_cast<unsigned>(prb), a.start_symbol + s, c.grid_index);
        }
      }
    }

    const uint32_t K = a.nof_payload_bits + 24, E = 108 * a.aggregation_level;
    const auto     key = std::make_pair(K, E);
    auto           it  = code_index.find(key);
    if (it == code_index.end()) {
      polar_dl_code code;
      polar_dl_code_build(K, E, code);
      pdcch_code_desc cd{};
      cd.u_source_offset = static_cast<uint32_t>(u_source.size());
      cd.gather_offset   = static_cast<uint32_t>(gather.size());
      cd.K               = static_cast<uint16_t>(K);
      cd.n               = static_cast<uint16_t>(code.n);
      u_source.insert(u_source.end(), code.u_source.begin(), code.u_source.end());
      for (uint32_t r = 0; r < E / 2; ++r) {
        gather.push_back(code.gather[2 * r] | (static_cast<uint32_t>(code.gather[2 * r + 1]) << 16));
      }
      it = code_index.emplace(key, static_cast<uint32_t>(codes.size())).first;
      codes.push_back(cd);
    }

    pdcch_desc& d    = descs[i];
    d                = pdcch_desc{};
    d.payload_offset = c.payload_offset;
    payload_bytes    = std::max<uint64_t>(payload_bytes, static_cast<uint64_t>(c.payload_offset) + (a.nof_payload_bits + 7) / 8);
    d.code           = it->second;
    // The 24 ones ahead of the payload (pdcch_encoder_impl.cpp:41), and the RNTI on the last 16 parity bits (:54).
    uint32_t crc_init = c.rnti;
    for (uint32_t j = a.nof_payload_bits; j < a.nof_payload_bits + 24; ++j) {
      crc_init ^= crc_w[j];
    }
    d.crc_init    = crc_init;
    d.c_init_data = ((c.n_rnti << 16) + c.n_id_pdcch_data) & 0x7fffffffu;
    for (uint32_t s = 0; s < a.duration; ++s) {
      d.c_init_dmrs[s] = ((14u * c.slot_index + a.start_symbol + s + 1u) * (2u * c.n_id_pdcch_dmrs + 1u) * (1u << 17) +
                          2u * c.n_id_pdcch_dmrs) & 0x7fffffffu;
    }
    d.grid_base   = c.grid_index * grid_nof_ports * port_stride + a.start_symbol * nsc;
    d.nsc         = nsc;
    d.port_stride = port_stride;
    d.prb_offset  = static_cast<uint32_t>(prb_table.size());
    prb_table.insert(prb_table.end(), prbs.begin(), prbs.end());
    // reference_point_k_rb (pdcch_processor_impl.cpp:113) and the span of DM-RS sequence words the PRBs read.
    const uint32_t ref   = a.mapping == PDCCH_CORESET0 ? a.bwp_start_rb : 0;
    const uint32_t first = 6 * (prbs.front() - ref), last = 6 * (prbs.back() - ref) + 5;
    d.dmrs_word0       = first >> 5;
    d.dmrs_nof_words   = static_cast<uint16_t>((last >> 5) - (first >> 5) + 1);
    d.nof_payload_bits = static_cast<uint16_t>(a.nof_payload_bits);
    d.nof_prb          = static_cast<uint16_t>(prbs.size());
    d.reference_rb     = static_cast<uint16_t>(ref);
    d.duration         = static_cast<uint16_t>(a.duration);
    d.nof_ports        = static_cast<uint16_t>(a.nof_ports);
    // modulation_mapper_lut_impl.cpp:154 (+-sqrt(1/2) as floats), pdcch_modulator_impl.cpp:54 (the scaling when it is a
    // normal float); dmrs_pdcch_processor_impl.cpp:49 (M_SQRT1_2 x amplitude in double, then a float).
    const float qpsk   = static_cast<float>(M_SQRT1_2);
    d.data_amplitude   = std::isnormal(c.data_scaling) ? qpsk * c.data_scaling : qpsk;
    d.dmrs_amplitude   = static_cast<float>(M_SQRT1_2 * static_cast<double>(c.dmrs_amplitude));
    for (uint32_t p = 0; p < a.nof_ports; ++p) {
      d.w[p][0] = c.precoding[p][0];
      d.w[p][1] = c.precoding[p][1];
    }
    if (prbs.size() > PDCCH_MAX_PRBS || d.dmrs_nof_words > PDCCH_MAX_DMRS_WORDS || E / 32 > PDCCH_MAX_DATA_WORDS) {
      return fail(SRSGPU_ERR_INVALID_ARG, "DCI %u: internal table bound exceeded", i);
    }
  }
  std::lock_guard<std::mutex> lock(ctx->mtx);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int r = ensure_gold_tables(ctx)) {
    return r;
  }
  plan_ptr<srsgpu_pdcch_plan> plan(new srsgpu_pdcch_plan());
  plan->ctx           = ctx;
  plan->nof_dcis      = nof_dcis;
  plan->payload_bytes = payload_bytes;
  // With a DCI there is a code with its tables and at least one PRB: none of the six tables is empty then.
  if (nof_dcis > 0 && (!plan->d_descs.upload(descs) || !plan->d_codes.upload(codes) ||
                       !plan->d_u_source.upload(u_source) || !plan->d_gather.upload(gather) ||
                       !plan->d_prbs.upload(prb_table) || !plan->d_crc_weights.upload(crc_w))) {
    return fail(SRSGPU_ERR_HIP, "failed to upload the PDCCH tables");
  }
  *plan_out = plan.release();
  return SRSGPU_OK;
}

int srsgpu_pdcch_plan_execute(const srsgpu_pdcch_plan* plan,
                              const uint8_t*           d_payloads,
                              uint64_t                 payload_bytes,
                              uint32_t*                d_grids,
                              void*                    stream)
{
  if (plan == nullptr || (plan->nof_dcis > 0 && (d_payloads == nullptr || d_grids == nullptr))) {
    return fail(SRSGPU_ERR_INVALID_ARG, "null argument");
  }
  if (payload_bytes < plan->payload_bytes) {
    return fail(SRSGPU_ERR_INVALID_ARG, "the payload buffer holds %llu bytes, the plan's DCIs read %llu",
                static_cast<unsigned long long>(payload_bytes), static_cast<unsigned long long>(plan->payload_bytes));
  }
  launch_pdcch(plan->d_descs.get(), plan->nof_dcis, plan->d_codes.get(), plan->d_u_source.get(), plan->d_gather.get(),
               plan->d_prbs.get(), plan->d_crc_weights.get(), d_payloads, d_grids, plan->ctx->d_gold_x1.get(),
               plan->ctx->d_gold_x2_jump.get(), plan->ctx->d_gold_x2_lane.get(), static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return SRSGPU_OK;
}

void srsgpu_pdcch_plan_destroy(srsgpu_pdcch_plan* plan)
{
  if (plan == nullptr) {
    return;
  }
  delete plan;
}

} // extern "C"
