// UCI decoder for polar-coded fields (12..1706 message bits) on gfx950: one wavefront per codeblock, one workgroup of
// two wavefronts per field, every field of a plan in one launch. Restates uci_decoder_impl::decode_codeword_polar
// exactly (integers only): rate dematching with the promotion sum, the simplified successive-cancellation decoder,
// de-allocation and the CRC check per codeblock.
//
// Reference (behaviour, not code): lib/phy/upper/channel_processors/uci/uci_decoder_impl.cpp:43 (decode_codeword_polar),
// :80 (decode_codeblock_polar); lib/phy/upper/channel_coding/polar/polar_rate_dematcher_impl.cpp:100 with
// log_likelihood_ratio::promotion_sum (lib/phy/upper/log_likelihood_ratio.cpp:75); polar_decoder_impl.cpp:335 (decode),
// :227 (rate-1 node), :259 (rate-R node) with soft_xor (include/srsran/phy/upper/log_likelihood_ratio.h:207) and the
// saturated sum (log_likelihood_ratio.cpp:58); polar_deallocator_impl.cpp:27.
//
// One rule differs from the reference on purpose: both codeblocks of a two-codeblock field are always decoded and
// written. The reference decodes codeblock 1 only when codeblock 0 passes its CRC and otherwise leaves the caller's
// bits untouched, so for that case no value of those bits is "the reference's"; the status is 0 either way.
//
// Everything that depends only on (K, E) is a table built at plan creation (polar_code.cpp) and shared by all
// codeblocks with that code: the composed dematching map, the op list of the tree walk, the message positions and
// the CRC weights. Control flow is wave-uniform: the wave fetches 64 ops with one vector load and broadcasts them one
// by one with v_readlane, so no op waits for a memory round trip of its own.
//
// LLR stages 6..10 live in LDS, int8, stage s (2^s values) at byte offset 2^s of the wave's 2 KiB, dword aligned, and
// f / g run there on four packed values per lane and step. Stages 0..5, 63 values, live in ONE register with the same
// layout, stage s in lanes [2^s, 2^(s+1)): f and g fetch their two operands with two cross-lane moves that are in
// flight together and write nothing to LDS, so an op on a small node, and most ops of a tree are on small nodes, costs
// one ds_bpermute round trip where the LDS path costs a read, a write and the wait for the write before the next op
// may read (measured: profiles/uci_polar_decoder.md).
// Estimated bits x and decoded bits u are bit-packed in registers, lane l (< 32) holding bits 32 l .. 32 l + 31: a
// rate-1 leaf is a ballot per 64 values, its polar transform log2(size) butterfly steps (masks inside a word,
// __shfl_xor between words), the combine a shifted xor. The CRC is linear: the xor of x^(K-1-k) mod g over the set
// de-allocated bits k, reduced across the wave.
//
// Output: each wave packs its codeblock's message bits with ballots into its own LDS words; after the workgroup
// barrier (two-codeblock fields only) wave 0 assembles every output word of the field, funnel-shifting codeblock 1's
// bits behind codeblock 0's, so the word the two codeblocks share is written once, whole, without atomics.
// Byte traffic per codeblock: E LLR bytes and 2 R N table bytes read, the op list, 4 K table bytes.
#include "polar_code.h"
#include "srsgpu_internal.h"

namespace srsgpu {
namespace {

constexpr int POLAR_THREADS = 128;  // two wavefronts: codeblocks 0 and 1 of one field
constexpr int LLR_MAX       = 120;  // log_likelihood_ratio::LLR_MAX
constexpr int LLR_INFTY     = 127;  // log_likelihood_ratio::LLR_INFTY

/// Makes this wave's LDS writes visible to its own other lanes.
__device__ inline void wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ inline int iabs(int x)
{
  return x < 0 ? -x : x;
}

/// tackle_special_sums (log_likelihood_ratio.cpp:40) over a finite result r of a + b.
__device__ inline int special_sums(int a, int b, int r)
{
  r = iabs(b) > LLR_MAX ? b : r;
  r = iabs(a) > LLR_MAX ? a : r;
  return a == -b ? 0 : r;
}

/// log_likelihood_ratio::promotion_sum (log_likelihood_ratio.cpp:75).
__device__ inline int promotion_sum(int a, int b)
{
  const int s = a + b;
  return special_sums(a, b, s > LLR_MAX ? LLR_INFTY : s < -LLR_MAX ? -LLR_INFTY : s);
}

/// soft_xor (log_likelihood_ratio.h:207).
__device__ inline int f_value(int x, int y)
{
  const int m = min(iabs(x), iabs(y));
  return (x ^ y) < 0 ? -m : m;
}

/// switch_combine (polar_decoder_impl.cpp:42): y + x for bit 0, y - x for bit 1, saturated (log_likelihood_ratio.cpp:58).
__device__ inline int g_value(int x, int y, uint32_t bit)
{
  const int c = bit != 0 ? -x : x;
  return special_sums(y, c, min(max(y + c, -LLR_MAX), LLR_MAX));
}

__device__ inline int byte_of(uint32_t w, int k)
{
  return static_cast<int>(static_cast<int8_t>(w >> (8 * k)));
}

__device__ inline uint32_t pack4(int a, int b, int c, int d)
{
  return (static_cast<uint32_t>(a) & 0xffu) | ((static_cast<uint32_t>(b) & 0xffu) << 8) |
         ((static_cast<uint32_t>(c) & 0xffu) << 16) | (static_cast<uint32_t>(d) << 24);
}

// The shuffle form, not common.h's DPP wave_xor: the same integers but other code, whose speed here is not measured.
__device__ inline uint32_t wave_xor_shfl(uint32_t v)
{
  for (int o = 32; o > 0; o >>= 1) {
    v ^= static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), o));
  }
  return v;
}

__global__ __launch_bounds__(POLAR_THREADS) void uci_polar_decoder_kernel(
    const uci_polar_field_desc* __restrict__ fields,
    const uci_polar_code_desc* __restrict__  codes,
    const uint32_t* __restrict__             ops,
    const uint16_t* __restrict__             tables,
    const int8_t* __restrict__               src0,
    const int8_t* __restrict__               src1,
    const int8_t* __restrict__               src2,
    uint32_t* __restrict__                   msgs,
    uint8_t* __restrict__                    status)
{
  __shared__ uint32_t s_llr[2][512];  // per wave: stage s at bytes [2^s, 2^(s+1))
  __shared__ uint32_t s_u[2][32];     // per wave: the decoded bits u, 32 per word
  __shared__ uint32_t s_msg[2][34];   // per wave: the codeblock's message bits, 32 per word, zeros above the last
  __shared__ uint32_t s_ok[2];

  // One codeblock per wavefront: everything derived from the descriptors is wave-uniform, and so is every branch.
  const uint32_t             lane = threadIdx.x & 63u;
  const uint32_t             wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t             f    = blockIdx.x;
  const uci_polar_field_desc fd   = fields[f];
  if (wave >= fd.nof_cb) {
    return;  // one-codeblock field: no barrier below
  }
  const uci_polar_code_desc cd = codes[fd.code];
  const uint32_t            n = cd.n, N = 1u << n, K = cd.K, R = cd.R;
  const int8_t*   llrs  = (fd.source == 0 ? src0 : fd.source == 1 ? src1 : src2) + fd.llr_offset + wave * fd.E_cb;
  int8_t*         llr8  = reinterpret_cast<int8_t*>(s_llr[wave]);
  const uint16_t* demap = tables + cd.demap_offset;
  const uint16_t* info  = tables + cd.info_offset;

  // Rate dematching (polar_rate_dematcher_impl.cpp:100) through the composed map, straight into the top stage: row r
  // of the map names the r-th LLR of each position, added in increasing r as the reference does (:51).
  // Stages 0..5 (63 values) live in one register, stage s in lanes [2^s, 2^(s+1)) as in LDS; a 32-bit mother code
  // starts there, so lanes 32..63 dematch positions 0..31 (the lower lanes repeat them, unused).
  int reg = 0;
  for (uint32_t p = n == 5 ? (lane & 31u) : lane; p < N; p += 64) {
    const uint32_t t0  = demap[p];
    int            acc = t0 == POLAR_DEMAP_SHORTENED ? LLR_INFTY : t0 == POLAR_DEMAP_NONE ? 0 : llrs[t0];
    for (uint32_t r = 1; r < R; ++r) {
      const uint32_t t = demap[r * N + p];
      if (t != POLAR_DEMAP_NONE) {
        acc = promotion_sum(acc, llrs[t]);
      }
    }
    if (n == 5) {
      reg = acc;
    } else {
      llr8[N + p] = static_cast<int8_t>(acc);
    }
  }
  if (lane < 34) {
    s_msg[wave][lane] = 0;
  }
  wave_sync();

  uint32_t est = 0, u = 0;  // lanes 0..31: bits 32 lane .. 32 lane + 31; lanes 32..63 stay 0
  for (uint32_t base = 0; base < cd.nof_ops; base += 64) {
    const uint32_t mine  = base + lane < cd.nof_ops ? ops[cd.ops_offset + base + lane] : 0u;
    const uint32_t count = min(64u, cd.nof_ops - base);
    for (uint32_t i = 0; i < count; ++i) {
      const uint32_t op   = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(mine), static_cast<int>(i)));
      const uint32_t type = op & 3u, s = (op >> 2) & 15u, pos = op >> 6;
      if (type == POLAR_OP_F || type == POLAR_OP_G) {
        // Stage s -> stage s - 1 (polar_decoder_impl.cpp:270 / :284): x = first half, y = second half.
        const uint32_t half = 1u << (s - 1);
        const bool     is_g = type == POLAR_OP_G;
        if (s <= 6) {
          // Into the register stages: lane half + i takes x_i and y_i, from LDS for stage 6 (position a multiple of
          // 64, so the estimated bits are one whole word) and from the register itself below. No LDS write, no wait.
          const uint32_t word = static_cast<uint32_t>(
              __builtin_amdgcn_readlane(static_cast<int>(est), static_cast<int>(pos >> 5)));
          int      x, y;
          uint32_t bitp;
          if (s == 6) {
            x    = llr8[64 + (lane & 31u)];
            y    = llr8[96 + (lane & 31u)];
            bitp = lane & 31u;
          } else {
            x    = __shfl_down(reg, half);
            y    = __shfl_down(reg, 2 * half);
            bitp = (pos + lane - half) & 31u;
          }
          const int r = is_g ? g_value(x, y, (word >> bitp) & 1u) : f_value(x, y);
          reg         = (lane >= half && lane < 2 * half) ? r : reg;
        } else {
          // Stages 7..10 in LDS, four packed values per lane and step.
          const uint32_t  quads = half >> 2;
          const uint32_t* in    = s_llr[wave] + (half >> 1);  // byte offset 2^s
          uint32_t*       out   = s_llr[wave] + (half >> 2);  // byte offset 2^(s-1)
          for (uint32_t d0 = 0; d0 < quads; d0 += 64) {
            const uint32_t d    = min(d0 + lane, quads - 1);
            const uint32_t bitp = pos + 4 * d;
            // The shuffle runs in every lane; bits of a rate-R node's left child are final when g runs (:280).
            const uint32_t word = static_cast<uint32_t>(__shfl(static_cast<int>(est), static_cast<int>(bitp >> 5)));
            const uint32_t nib  = is_g ? (word >> (bitp & 31u)) & 15u : 0u;
            const uint32_t x = in[d], y = in[quads + d];
            uint32_t       r;
            if (is_g) {
              r = pack4(g_value(byte_of(x, 0), byte_of(y, 0), nib & 1u), g_value(byte_of(x, 1), byte_of(y, 1), nib & 2u),
                        g_value(byte_of(x, 2), byte_of(y, 2), nib & 4u), g_value(byte_of(x, 3), byte_of(y, 3), nib & 8u));
            } else {
              r = pack4(f_value(byte_of(x, 0), byte_of(y, 0)), f_value(byte_of(x, 1), byte_of(y, 1)),
                        f_value(byte_of(x, 2), byte_of(y, 2)), f_value(byte_of(x, 3), byte_of(y, 3)));
            }
            if (d0 + lane < quads) {
              out[d] = r;
            }
          }
          wave_sync();
        }
      } else if (type == POLAR_OP_LEAF) {
        // Rate-1 node (:227): hard decisions `value <= 0` of the 2^s LLRs of stage s, then their polar transform.
        const uint32_t size = 1u << s;
        uint32_t       bits = 0;
        if (s <= 5) {
          // The register stage: the ballot's bits [size, 2 size) are the node's, at most 32 of them, one word.
          const unsigned long long m = __ballot(reg <= 0) >> size;
          const uint32_t           v = size == 32 ? static_cast<uint32_t>(m) : static_cast<uint32_t>(m) & ((1u << size) - 1u);
          bits                       = lane == (pos >> 5) ? v << (pos & 31u) : 0u;
        } else {
          for (uint32_t c0 = 0; c0 < size; c0 += 64) {
            const int                v    = llr8[size + c0 + lane];
            const unsigned long long m    = __ballot(v <= 0);
            const uint32_t           word = (pos + c0) >> 5;
            bits |= lane == word ? static_cast<uint32_t>(m) : 0u;
            bits |= lane == word + 1 ? static_cast<uint32_t>(m >> 32) : 0u;
          }
        }
        est |= bits;
        // x = u G and G is its own inverse: butterflies of span t < size stay inside the node's aligned range.
        if (size > 1) {
          bits ^= (bits >> 1) & 0x55555555u;
        }
        if (size > 2) {
          bits ^= (bits >> 2) & 0x33333333u;
        }
        if (size > 4) {
          bits ^= (bits >> 4) & 0x0f0f0f0fu;
        }
        if (size > 8) {
          bits ^= (bits >> 8) & 0x00ff00ffu;
        }
        if (size > 16) {
          bits ^= (bits >> 16) & 0x0000ffffu;
        }
        for (uint32_t t = 1; 32 * t < size; t <<= 1) {
          const uint32_t other = static_cast<uint32_t>(__shfl_xor(static_cast<int>(bits), static_cast<int>(t)));
          bits ^= (lane & t) == 0 ? other : 0u;
        }
        u |= bits;
      } else {
        // Combine (:302): the node's upper half of estimated bits xored into its lower half.
        const uint32_t half = 1u << (s - 1);
        if (half >= 32) {
          const uint32_t other = static_cast<uint32_t>(__shfl_down(static_cast<int>(est), half >> 5));
          est ^= (lane >= (pos >> 5) && lane < ((pos + half) >> 5)) ? other : 0u;
        } else {
          const uint32_t mask = ((1u << half) - 1u) << (pos & 31u);
          est ^= lane == (pos >> 5) ? (est >> half) & mask : 0u;
        }
      }
    }
  }

  // De-allocation (polar_deallocator_impl.cpp:27) and CRC over all K bits, filler and CRC included
  // (uci_decoder_impl.cpp:107).
  if (lane < 32) {
    s_u[wave][lane] = u;
  }
  wave_sync();
  const uint16_t* weights = info + K;
  uint32_t        crc     = 0;
  for (uint32_t k = lane; k < K; k += 64) {
    const uint32_t q = info[k];
    crc ^= ((s_u[wave][q >> 5] >> (q & 31u)) & 1u) != 0 ? weights[k] : 0u;
  }
  const bool ok = wave_xor_shfl(crc) == 0;

  // Message bits of this codeblock (uci_decoder_impl.cpp:113): K-set bits [filler, K - L).
  const uint32_t A      = fd.nof_bits;
  const uint32_t bits0  = A / fd.nof_cb;
  const uint32_t nbits  = wave == 0 ? bits0 : A - bits0;
  const uint32_t filler = wave == 0 ? A % fd.nof_cb : 0u;
  for (uint32_t j0 = 0; j0 < nbits; j0 += 64) {
    const uint32_t j   = j0 + lane;
    uint32_t       bit = 0;
    if (j < nbits) {
      const uint32_t q = info[j + filler];
      bit              = (s_u[wave][q >> 5] >> (q & 31u)) & 1u;
    }
    const unsigned long long m = __ballot(bit != 0);
    if (lane == 0) {
      s_msg[wave][j0 >> 5]       = static_cast<uint32_t>(m);
      s_msg[wave][(j0 >> 5) + 1] = static_cast<uint32_t>(m >> 32);
    }
  }
  if (lane == 0) {
    s_ok[wave] = ok ? 1u : 0u;
  }
  if (fd.nof_cb == 2) {
    __syncthreads();  // both waves of a two-codeblock field get here
  } else {
    wave_sync();
  }
  if (wave != 0) {
    return;
  }
  // Wave 0 writes every word of the field, the last one whole with zeros above bit A - 1.
  const uint32_t words = (A + 31u) >> 5;
  if (lane < words) {
    uint32_t v = 32u * lane < bits0 ? s_msg[0][min(lane, 33u)] : 0u;
    if (fd.nof_cb == 2) {
      const int start = static_cast<int>(32u * lane) - static_cast<int>(bits0);  // first bit wanted of codeblock 1
      if (start >= 0) {
        const uint32_t           q    = min(static_cast<uint32_t>(start) >> 5, 32u);
        const unsigned long long pair = s_msg[1][q] | (static_cast<unsigned long long>(s_msg[1][q + 1]) << 32);
        v |= static_cast<uint32_t>(pair >> (static_cast<uint32_t>(start) & 31u));
      } else if (start > -32) {
        v |= s_msg[1][0] << static_cast<uint32_t>(-start);
      }
    }
    msgs[fd.msg_word_offset + lane] = v;
  }
  if (lane == 0) {
    status[f] = (ok && (fd.nof_cb == 1 || s_ok[1] != 0)) ? 1 : 0;
  }
}

} // namespace

void launch_uci_polar_decode(const uci_polar_field_desc* d_fields,
                             uint32_t                    nof_fields,
                             const uci_polar_code_desc*  d_codes,
                             const uint32_t*             d_ops,
                             const uint16_t*             d_tables,
                             const int8_t*               d_src0,
                             const int8_t*               d_src1,
                             const int8_t*               d_src2,
                             uint32_t*                   d_msgs,
                             uint8_t*                    d_status,
                             hipStream_t                 stream)
{
  if (nof_fields == 0) {
    return;
  }
  hipLaunchKernelGGL(uci_polar_decoder_kernel, dim3(nof_fields), dim3(POLAR_THREADS), 0, stream, d_fields, d_codes,
                     d_ops, d_tables, d_src0, d_src1, d_src2, d_msgs, d_status);
}

} // namespace srsgpu
