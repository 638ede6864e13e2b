// CCE to PRB mapping and refusals of the PDCCH plan; see pdcch_host.h.
#include "pdcch_host.h"
#include "host_util.h"
#include "polar_code.h"
#include <algorithm>

namespace srsgpu {

namespace {

constexpr uint32_t REG_PER_CCE = 6, RB_PER_RESOURCE = 6, MAX_RESOURCES = 45;

uint32_t nof_resources(const pdcch_alloc& a)
{
  return static_cast<uint32_t>(__builtin_popcountll(a.frequency_resources & ((1ull << MAX_RESOURCES) - 1)));
}

/// Bundle size L, interleaver rows R, shift and CORESET PRBs of an interleaved mapping; CORESET0 fixes L = 6, R = 2
/// and spans the BWP (cce_to_prb_mapping.cpp:152).
struct interleaving {
  uint32_t L, R, shift, nof_rb;
};

interleaving interleaving_of(const pdcch_alloc& a)
{
  if (a.mapping == PDCCH_CORESET0) {
    return {6, 2, a.shift_index, a.bwp_size_rb};
  }
  return {a.reg_bundle_size, a.interleaver_size, a.shift_index, RB_PER_RESOURCE * nof_resources(a)};
}

} // namespace

std::string pdcch_refusal(const pdcch_alloc& a, uint32_t grid_nof_prb, uint32_t grid_nof_ports)
{
  const bool interleaved = a.mapping == PDCCH_INTERLEAVED;
  if (a.mapping > PDCCH_INTERLEAVED) {
    return format("cce_to_reg_mapping %u is not 0 (CORESET0), 1 (non-interleaved) or 2 (interleaved)", a.mapping);
  }
  if ((a.frequency_resources >> MAX_RESOURCES) != 0) {
    return "frequency_resources has bits above the 45 frequency resources";
  }
  if (static_cast<uint64_t>(a.bwp_start_rb) + a.bwp_size_rb > 275) {
    return format("The BWP (%u PRBs from %u) exceeds 275 PRBs", a.bwp_size_rb, a.bwp_start_rb);
  }
  if (a.duration < 1 || a.duration > 3) {
    return format("The CORESET duration (i.e., %u) is out of the range 1..3", a.duration);
  }
  if (static_cast<uint64_t>(a.start_symbol) + a.duration > 14) {
    return format("The CORESET start symbol index (i.e., %u) plus the duration (i.e., %u) exceeds the slot duration "
                  "(i.e., 14)", a.start_symbol, a.duration);
  }
  if (interleaved && a.reg_bundle_size != 6 && a.reg_bundle_size != (a.duration == 3 ? 3u : 2u)) {
    return format("Invalid REG bundle size (i.e., %u) for CORESET duration of %u", a.reg_bundle_size, a.duration);
  }
  if (interleaved && a.interleaver_size != 2 && a.interleaver_size != 3 && a.interleaver_size != 6) {
    return format("Invalid interleaver size (i.e., %u)", a.interleaver_size);
  }
  const uint32_t al = a.aggregation_level;
  if (al != 1 && al != 2 && al != 4 && al != 8 && al != 16) {
    return format("Invalid aggregation level (i.e., %u)", al);
  }
  const uint32_t nof_cce = nof_resources(a) * a.duration;
  if (a.cce_index + static_cast<uint64_t>(al) > nof_cce) {
    return format("The CCE index (i.e., %u) plus the aggregation level (i.e., %u) exceeds CORESET capacity (i.e., %u)",
                  a.cce_index, al, nof_cce);
  }
  if (a.nof_payload_bits == 0) {
    return "Empty payload";
  }
  const uint32_t K = a.nof_payload_bits + 24, E = 108 * al;
  if (const char* why = polar_dl_code_refusal(K, E)) {
    return format("%u payload bits at aggregation level %u (K = %u, E = %u): %s", a.nof_payload_bits, al, K, E, why);
  }
  if (a.mapping != PDCCH_NON_INTERLEAVED) {
    const interleaving il    = interleaving_of(a);
    const uint32_t     n_reg = il.nof_rb * a.duration;
    if (n_reg == 0 || n_reg % (il.L * il.R) != 0 || il.L % a.duration != 0) {
      return format("Invalid CORESET configuration: N_REG = %u is not a positive multiple of L R = %u x %u, or L is no "
                    "multiple of the duration %u", n_reg, il.L, il.R, a.duration);
    }
    // CORESET0 spans the BWP, not the frequency resources the validator counts: CCEs past its REGs would wrap around
    // the interleaver onto REG bundles the DCI already has.
    if (static_cast<uint64_t>(a.cce_index + al) * REG_PER_CCE > n_reg) {
      return format("The CCE index (i.e., %u) plus the aggregation level (i.e., %u) exceeds the %u REGs of CORESET0",
                    a.cce_index, al, n_reg);
    }
  }
  if (a.nof_ports < 1 || a.nof_ports > grid_nof_ports) {
    return format("The precoding number of ports (i.e., %u) is outside 1..%u, the grid's ports", a.nof_ports,
                  grid_nof_ports);
  }
  const std::vector<uint16_t> prbs  = pdcch_prbs(a);
  const uint64_t              limit = std::min<uint64_t>(grid_nof_prb, static_cast<uint64_t>(a.bwp_start_rb) + a.bwp_size_rb);
  if (prbs.size() != REG_PER_CCE * al / a.duration || prbs.back() >= limit) {
    return format("PRB %u of the DCI lies outside the BWP (%u PRBs from %u) or the grid (%u PRBs)",
                  prbs.empty() ? 0u : static_cast<unsigned>(prbs.back()), a.bwp_size_rb, a.bwp_start_rb, grid_nof_prb);
  }
  return {};
}

std::vector<uint16_t> pdcch_prbs(const pdcch_alloc& a)
{
  const uint32_t dur = a.duration, al = a.aggregation_level;
  // REG indices of the CCEs, ascending.
  std::vector<uint32_t> regs;
  if (a.mapping == PDCCH_NON_INTERLEAVED) {
    for (uint32_t g = REG_PER_CCE * a.cce_index; g != REG_PER_CCE * (a.cce_index + al); ++g) {
      regs.push_back(g);
    }
  } else {
    // REG bundle x = c R + r goes to bundle f(x) = (r C + c + n_shift) mod (N_REG / L), C = N_REG / (L R).
    const interleaving il    = interleaving_of(a);
    const uint32_t     n_reg = il.nof_rb * dur;
    const uint32_t     C     = n_reg / (il.L * il.R);
    const uint32_t     per_cce = REG_PER_CCE / il.L;
    for (uint32_t x = a.cce_index * per_cce; x != (a.cce_index + al) * per_cce; ++x) {
      const uint32_t f = ((x % il.R) * C + x / il.R + il.shift) % (n_reg / il.L);
      for (uint32_t g = f * il.L; g != (f + 1) * il.L; ++g) {
        regs.push_back(g);
      }
    }
    std::sort(regs.begin(), regs.end());
  }
  // A PRB holds `dur` consecutive REGs (one per symbol): every dur-th REG of the list names a PRB.
  std::vector<uint16_t> prbs;
  if (a.mapping == PDCCH_CORESET0) {
    for (size_t i = 0; i < regs.size(); i += dur) {
      prbs.push_back(static_cast<uint16_t>(regs[i] / dur + a.bwp_start_rb));
    }
    return prbs;
  }
  // The walk over the frequency resources from bwp_start_rb: the CORESET's PRBs are numbered through the set
  // resources only, and a PRB is taken when its first REG is the next of the list.
  size_t   next = 0;
  uint32_t reg  = 0;
  for (uint32_t res = 0; res != MAX_RESOURCES && next < regs.size(); ++res) {
    if (((a.frequency_resources >> res) & 1u) == 0) {
      continue;
    }
    for (uint32_t prb = res * RB_PER_RESOURCE + a.bwp_start_rb, end = prb + RB_PER_RESOURCE; prb != end && next < regs.size();
         ++prb, reg += dur) {
      if (reg == regs[next]) {
        prbs.push_back(static_cast<uint16_t>(prb));
        next += dur;
      }
    }
  }
  return prbs;
}

} // namespace srsgpu
