/*
 * srsgpu_phy.h — C ABI of the MI355X (gfx950) 5G NR PHY acceleration library (libsrsgpu_phy.so).
 *
 * Drop-in boundary for the srsRAN upper-PHY channel-coding hot path. Every entry point names the reference interface
 * it replaces (paths relative to the srsRAN tree, include/ or lib/). Plain C: pointers, sizes, POD structs; no C++ or
 * torch types. Device pointers are HIP device (HBM) addresses; `stream` is a hipStream_t (NULL = default stream).
 *
 * Error convention: functions return SRSGPU_OK (0) or a negative SRSGPU_ERR_* code; srsgpu_last_error() returns a
 * thread-local description of the last failure. Invalid configurations are rejected with the same conditions the
 * reference asserts on (e.g. ldpc_decoder_impl.cpp:48-:56, :73-:88).
 */
#ifndef SRSGPU_PHY_H
#define SRSGPU_PHY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRSGPU_OK 0
#define SRSGPU_ERR_INVALID_ARG (-1)
#define SRSGPU_ERR_HIP (-2)
#define SRSGPU_ERR_NO_MEMORY (-3)

/* CRC generator polynomials, same numbering as srsran::crc_generator_poly
 * (include/srsran/phy/upper/channel_coding/crc_calculator.h:33). */
#define SRSGPU_CRC24A 0
#define SRSGPU_CRC24B 1
#define SRSGPU_CRC24C 2
#define SRSGPU_CRC16 3
#define SRSGPU_CRC11 4
#define SRSGPU_CRC6 5
#define SRSGPU_CRC_NONE 255 /* no CRC early stop: the decoder runs max_iterations (crc == nullptr) */

/* LDPC decoder arithmetic variants of the reference (lib/phy/upper/channel_coding/channel_coding_factories.cpp,
 * create_ldpc_decoder_factory_sw): "generic" rounds the normalised min-sum magnitudes (ldpc_decoder_generic.cpp:70);
 * "avx2"/"avx512"/"neon" truncate a 16-bit fixed-point product (avx2_support.h:71). Results are bit-exact with the
 * selected variant. */
#define SRSGPU_LDPC_IMPL_GENERIC 0
#define SRSGPU_LDPC_IMPL_SIMD 1

typedef struct srsgpu_context srsgpu_context;

/** Library version (major * 10000 + minor * 100 + patch). */
int srsgpu_version(void);

/** Thread-local description of the last error. */
const char* srsgpu_last_error(void);

/** Creates a context on HIP device `device` (one process per GPU). Uploads the lifted base-graph tables. */
int srsgpu_context_create(int device, srsgpu_context** ctx);

/** Destroys a context and frees its device memory. */
void srsgpu_context_destroy(srsgpu_context* ctx);

/** HIP device index of a context (-1 for NULL): the device a binding allocates its own buffers and streams on. */
int srsgpu_context_device(const srsgpu_context* ctx);

/** Kernel-selection options of a context, read when a plan is created (not from the process environment: what a plan
 *  runs depends only on its context and configuration). Every default is the measured-fastest choice; the others are
 *  alternative kernels with identical results, kept for the parity tests that pin them. */
typedef enum {
  /** Packed LDPC decoder, even Z: -1 (default) the edge-split kernel when a launch gives under ~3 waves per SIMD,
   *  else the one-row-pair kernel; 0 always the one-row-pair kernel; 1 always the edge-split kernel. */
  SRSGPU_OPTION_DECODER_SPLIT = 1,
  /** 0 (default) / 1: codeblocks of Z = 144..192 two per workgroup (three waves for two codeblocks). */
  SRSGPU_OPTION_DECODER_PAIRS = 2,
  /** 1 (default) / 0: the PUSCH decoder dematches plain first transmissions itself (0: every codeblock through the
   *  separate rate dematcher kernel). */
  SRSGPU_OPTION_DECODER_FUSED_DEMATCH = 3,
  /** 0 (default) / 1: the PDSCH encoder's one-bit-per-byte kernel for every codeblock (0: the packed-word kernel where
   *  Z % 32 == 0 and the message is byte aligned). */
  SRSGPU_OPTION_ENCODER_BYTE_KERNEL = 4,
  /** 0 (default) / 1: the PDSCH encoder clears its codeword output before every execution (0: only when its
   *  codeblocks do not each store whole words that tile the output). */
  SRSGPU_OPTION_ENCODER_ZERO_OUTPUT = 5,
  /** 1 (default) / 0: a PUSCH decoder plan whose transport blocks all have one codeblock, every one dematched by the
   *  decoder itself, has the decoder kernel write the transport blocks and their CRC flags and skips the TB-stage
   *  launch (0: always the separate TB stage). */
  SRSGPU_OPTION_DECODER_TB_FOLD = 6,
  /** 0 (default) / 1: the PUSCH demodulator's general paths for every transmission: the search for an RE's OFDM
   *  symbol (0: a closed form where every data symbol carries the same number of REs) and LLR-by-LLR descrambling and
   *  packing (0: four LLRs at a time where layers x modulation order is a multiple of 4). */
  SRSGPU_OPTION_DEMOD_GENERAL_PATHS = 7
} srsgpu_option;

/** Sets option `option` (srsgpu_option) of a context for the plans created afterwards. */
int srsgpu_context_set_option(srsgpu_context* ctx, int option, int value);

/** Reads option `option` of a context. */
int srsgpu_context_get_option(const srsgpu_context* ctx, int option, int* value);

/* ------------------------------------------------------------------------------------------------------------------
 * LDPC decoder — replaces srsran::ldpc_decoder::decode(bit_buffer& output, span<const log_likelihood_ratio> input,
 * crc_calculator* crc, const configuration& cfg)   (include/srsran/phy/upper/channel_coding/ldpc/ldpc_decoder.h:72,
 * lib/phy/upper/channel_coding/ldpc/ldpc_decoder_impl.cpp:60), batched over codeblocks.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint8_t  base_graph;      /* 1 or 2 (codeblock_metadata::tb_common.base_graph) */
  uint8_t  crc_poly;        /* SRSGPU_CRC* used for early stopping, or SRSGPU_CRC_NONE (crc == nullptr) */
  uint16_t lifting_size;    /* Z (tb_common.lifting_size) */
  uint16_t nof_filler_bits; /* cb_specific.nof_filler_bits */
  uint8_t  nof_crc_bits;    /* cb_specific.nof_crc_bits: 16 or 24 */
  uint8_t  max_iterations;  /* algorithm_conf.max_iterations (> 0) */
  float    scaling_factor;  /* algorithm_conf.scaling_factor, in (0, 1) */
  uint32_t llr_offset;      /* index of the codeblock's first LLR in the batch LLR buffer */
  uint32_t nof_llrs;        /* input.size(): (K + 2) * Z <= nof_llrs <= N_short * Z */
  uint32_t out_offset;      /* byte offset of the codeblock's K*Z output bits, packed MSB first (bit_buffer) */
} srsgpu_ldpc_decoder_config;

/** Pre-validated, device-resident batch of decoder work (reusable across calls and capturable in a hipGraph). */
typedef struct srsgpu_ldpc_decoder_plan srsgpu_ldpc_decoder_plan;

/** Validates `nof_cbs` configurations, builds the CRC early-stop tables they need and uploads the work descriptors.
 *  Blocking (host <-> device copies); call it outside the timed / captured region. */
int srsgpu_ldpc_decoder_plan_create(srsgpu_context*                   ctx,
                                    int                               impl,
                                    const srsgpu_ldpc_decoder_config* cfgs,
                                    uint32_t                          nof_cbs,
                                    srsgpu_ldpc_decoder_plan**        plan);

/** Decodes the planned codeblocks: reads int8 LLRs from d_llrs, writes packed bits to d_out and, per codeblock, the
 *  number of iterations on CRC success or -1 (std::nullopt) to d_nof_iterations[i]. Asynchronous on `stream`; no host
 *  synchronisation, no allocation (hipGraph-capturable). */
int srsgpu_ldpc_decoder_plan_execute(const srsgpu_ldpc_decoder_plan* plan,
                                     const int8_t*                   d_llrs,
                                     uint8_t*                        d_out,
                                     int32_t*                        d_nof_iterations,
                                     void*                           stream);

void srsgpu_ldpc_decoder_plan_destroy(srsgpu_ldpc_decoder_plan* plan);

/** One-shot convenience: plan_create + plan_execute + stream synchronisation + plan_destroy. */
int srsgpu_ldpc_decode(srsgpu_context*                   ctx,
                       int                               impl,
                       const srsgpu_ldpc_decoder_config* cfgs,
                       uint32_t                          nof_cbs,
                       const int8_t*                     d_llrs,
                       uint8_t*                          d_out,
                       int32_t*                          d_nof_iterations,
                       void*                             stream);

/* ------------------------------------------------------------------------------------------------------------------
 * PUSCH codeblock decoding — the operation behind hal::hw_accelerator_pusch_dec
 * (include/srsran/hal/phy/upper/channel_processors/pusch/hw_accelerator_pusch_dec.h:88-:112: configure_operation,
 * enqueue_operation, dequeue_operation, read_operation_outputs) and pusch_codeblock_decoder::decode
 * (lib/phy/upper/channel_processors/pusch/pusch_codeblock_decoder.cpp:33): rate dematching with HARQ soft combining
 * into a device-resident soft buffer (ldpc_rate_dematcher_impl.cpp:46), LDPC decoding and the codeblock CRC check,
 * batched over every codeblock of a slot.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint8_t  base_graph;       /* 1 or 2 */
  uint8_t  rv;               /* redundancy version 0..3 */
  uint8_t  modulation_order; /* Qm: 1, 2, 4, 6, 8 */
  uint8_t  crc_poly;         /* codeblock CRC: CRC24B (segmented TB), CRC24A or CRC16 (single codeblock) */
  uint16_t lifting_size;     /* Z */
  uint16_t nof_filler_bits;  /* F */
  uint8_t  nof_crc_bits;     /* 16 or 24 */
  uint8_t  max_iterations;   /* > 0 */
  uint8_t  new_data;         /* 1: first transmission (copy), 0: combine with the HARQ buffer */
  uint8_t  use_early_stop;   /* 1: CRC after every iteration; 0: max_iterations then one CRC check */
  float    scaling_factor;   /* normalised min-sum factor in (0, 1) */
  uint32_t Nref;             /* limited-buffer rate matching N_ref, 0 = none */
  uint32_t rm_length;        /* E: rate-matched length (multiple of Qm) */
  uint32_t llr_offset;       /* first of the E LLRs in the codeword LLR buffer */
  uint32_t harq_offset;      /* first of the N_short * Z LLRs of the codeblock's HARQ soft buffer */
  uint32_t out_offset;       /* byte offset of the packed K*Z decoded message bits */
} srsgpu_pusch_cb_config;

typedef struct srsgpu_pusch_cb_plan srsgpu_pusch_cb_plan;

/** Validates the codeblock configurations (reference assertions of ldpc_rate_dematcher_impl.cpp:54-:99 and the
 *  decoder's) and uploads the work descriptors. Blocking; outside the timed / captured region. */
int srsgpu_pusch_cb_plan_create(srsgpu_context*               ctx,
                                int                           impl,
                                const srsgpu_pusch_cb_config* cfgs,
                                uint32_t                      nof_cbs,
                                srsgpu_pusch_cb_plan**        plan);

/** Rate-dematches d_llrs into the HARQ buffers d_harq (in place), then decodes every codeblock whose entry in
 *  d_cb_crc_ok (persistent per-codeblock HARQ flags, may be NULL) is 0: writes the packed message to d_out, the number
 *  of iterations (or -1; 0 for codeblocks skipped because their CRC had already passed) to d_nof_iterations, and sets
 *  d_cb_crc_ok on success. Asynchronous on `stream`, hipGraph-capturable. */
int srsgpu_pusch_cb_plan_execute(const srsgpu_pusch_cb_plan* plan,
                                 const int8_t*               d_llrs,
                                 int8_t*                     d_harq,
                                 uint8_t*                    d_out,
                                 int32_t*                    d_nof_iterations,
                                 uint8_t*                    d_cb_crc_ok,
                                 void*                       stream);

void srsgpu_pusch_cb_plan_destroy(srsgpu_pusch_cb_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * PDSCH encoder — replaces srsran::pdsch_encoder::encode(span<uint8_t> codeword, span<const uint8_t> transport_block,
 * const configuration& cfg) (include/srsran/phy/upper/channel_processors/pdsch/pdsch_encoder.h,
 * lib/phy/upper/channel_processors/pdsch/pdsch_encoder_impl.cpp:28) and hal::hw_accelerator_pdsch_enc in TB mode
 * (hw_accelerator_pdsch_enc.h): TB CRC, segmentation, CB CRC24B, LDPC encoding and rate matching of every transport
 * block of a slot. The codeword is written packed MSB first (G = nof_ch_symbols * Qm bits per TB).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint8_t  base_graph;       /* 1 or 2 */
  uint8_t  rv;               /* 0..3 */
  uint8_t  modulation_order; /* Qm: 1, 2, 4, 6, 8 */
  uint8_t  nof_layers;       /* 1..4 */
  uint32_t tbs_bytes;        /* transport block size in bytes */
  uint32_t nof_ch_symbols;   /* number of channel symbols (multiple of nof_layers) */
  uint32_t Nref;             /* limited-buffer rate matching N_ref, 0 = none */
  uint32_t tb_offset;        /* byte offset of the transport block in the TB buffer */
  uint32_t cw_offset;        /* byte offset of the codeword in the output buffer (multiple of 4) */
} srsgpu_pdsch_tb_config;

typedef struct srsgpu_pdsch_encoder_plan srsgpu_pdsch_encoder_plan;

/** Segments every transport block (ldpc_segmenter_tx_impl.cpp:58), validates and uploads the work. Blocking. */
int srsgpu_pdsch_encoder_plan_create(srsgpu_context*               ctx,
                                     const srsgpu_pdsch_tb_config* cfgs,
                                     uint32_t                      nof_tbs,
                                     srsgpu_pdsch_encoder_plan**   plan);

/** Number of codeblocks the plan encodes (all transport blocks). */
uint32_t srsgpu_pdsch_encoder_plan_nof_codeblocks(const srsgpu_pdsch_encoder_plan* plan);

/** Encodes the planned transport blocks from d_tbs into d_codewords. The plan owns (zeroes, then fills) the output
 *  byte range [min cw_offset, max(cw_offset + ceil(G/32)*4)). Asynchronous on `stream`, hipGraph-capturable. */
int srsgpu_pdsch_encoder_plan_execute(const srsgpu_pdsch_encoder_plan* plan,
                                      const uint8_t*                   d_tbs,
                                      uint8_t*                         d_codewords,
                                      void*                            stream);

void srsgpu_pdsch_encoder_plan_destroy(srsgpu_pdsch_encoder_plan* plan);

/** Stage timing (see srsgpu_pusch_decoder_plan_enable_timing): stages 0: output clear + TB CRC, 1: codeblock
 *  encoding and rate matching (ms[2]). */
int srsgpu_pdsch_encoder_plan_enable_timing(srsgpu_pdsch_encoder_plan* plan, int enable);
int srsgpu_pdsch_encoder_plan_stage_times(srsgpu_pdsch_encoder_plan* plan, float* ms, uint32_t* nof_executes);

/* ------------------------------------------------------------------------------------------------------------------
 * PDSCH modulator — replaces srsran::pdsch_modulator::modulate(resource_grid_writer& grid, span<const bit_buffer>
 * codewords, const config_t& config) (include/srsran/phy/upper/channel_processors/pdsch/pdsch_modulator.h:93,
 * lib/phy/upper/channel_processors/pdsch/pdsch_modulator_impl.cpp:107): scrambling with the TS 38.211 §5.2.1 Gold
 * sequence (c_init = rnti * 2^15 + n_id, codeword q = 0, :30), modulation mapping (modulation_mapper_lut_impl.cpp:39,
 * amplitude sqrt(1 / average power) times `scaling`), layer mapping, wideband precoding (channel_precoder_generic.cpp:51)
 * and resource-element mapping (resource_grid_mapper_impl.cpp:269) into bf16 resource grids, for every PDSCH
 * transmission of a batch of slots. Codewords come packed MSB first (the PDSCH encoder's output format).
 * A resource grid holds `grid_nof_ports` x 14 symbols x 12 * `grid_nof_prb` subcarriers of complex bf16 (re, im)
 * pairs (srsran::cbf16_t), port-major then symbol-major; grid g starts g * grid_nof_ports * 14 * 12 * grid_nof_prb
 * elements into d_grids. Only the PDSCH REs are written (the DM-RS REs belong to the DM-RS processor).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint16_t rnti;                        /* n_RNTI */
  uint16_t n_id;                        /* n_ID, 0..1023 */
  uint8_t  modulation_order;            /* Qm of modulation1: 2 (QPSK), 4, 6, 8 (256QAM) */
  uint8_t  nof_layers;                  /* 1..4 */
  uint8_t  nof_ports;                   /* precoding ports, nof_layers..4 (<= grid_nof_ports) */
  uint8_t  start_symbol;                /* start_symbol_index */
  uint8_t  nof_symbols;                 /* start_symbol + nof_symbols <= 14 */
  uint8_t  dmrs_type;                   /* dmrs_config_type: 1 or 2 */
  uint8_t  nof_cdm_groups_without_data; /* 1..2 (type 1), 1..3 (type 2) */
  uint8_t  reserved;
  uint16_t dmrs_symbol_mask;            /* dmrs_symb_pos: bit l = OFDM symbol l carries DM-RS */
  uint16_t bwp_start_rb;                /* BWP start (CRB) */
  uint16_t bwp_size_rb;                 /* BWP size */
  uint16_t rb_start;                    /* contiguous non-interleaved VRB allocation [rb_start, rb_start + nof_rb) */
  uint16_t nof_rb;
  uint16_t pad;
  float    scaling;                     /* config.scaling (applied when std::isnormal) */
  float    precoding[4][4][2];          /* wideband precoding weight [port][layer] = (re, im) */
  uint32_t cw_offset;                   /* byte offset of the packed codeword (multiple of 4) */
  uint32_t nof_bits;                    /* codeword length: data REs x nof_layers x Qm */
  uint32_t grid_index;                  /* resource grid (slot) the transmission is mapped into */
} srsgpu_pdsch_mod_config;

/* Generalised frequency allocation, reserved resource elements and per-PRG precoding of one transmission (the
 * *_plan_create_ex entry points; a NULL extension array, or NULL members, keep the contiguous / no reserved REs /
 * wideband defaults of the plain configuration).
 *
 * srsgpu_re_pattern mirrors srsran::re_pattern (include/srsran/phy/support/re_pattern.h): the REs of re_mask (bit k =
 * subcarrier k of a PRB) in every CRB of crb_mask and every OFDM symbol of symbol_mask. */
typedef struct {
  const uint8_t* crb_mask;    /* one byte per grid CRB (nonzero = included); NULL = every CRB */
  uint16_t       re_mask;     /* 12 bits */
  uint16_t       symbol_mask; /* 14 bits */
} srsgpu_re_pattern;

typedef struct {
  const uint8_t*           crb_mask;     /* allocated CRBs, one byte per grid CRB: rb_allocation::get_crb_mask of any
                                            type-0 bitmap or interleaved VRB-to-PRB mapping (pdsch_modulator_impl.cpp:58,
                                            pusch_demodulator.h:55 rb_mask); NULL = the contiguous allocation of the
                                            plain configuration */
  const srsgpu_re_pattern* reserved;     /* reserved REs besides the DM-RS (pdsch_modulator::config_t::reserved: SSB,
                                            CSI-RS, ZP-CSI-RS, PT-RS ...); PDSCH modulator only */
  uint32_t                 nof_reserved;
  uint16_t                 prg_size;     /* precoding resource block group size in PRBs (precoding_configuration);
                                            0 = the wideband weights of the plain configuration */
  uint16_t                 nof_prg;      /* PRGs in prg_weights: PRG i covers CRBs [i prg_size, (i + 1) prg_size) */
  const float*             prg_weights;  /* [nof_prg][port][layer] (re, im), ports x layers of the configuration */
} srsgpu_alloc_ext;

typedef struct srsgpu_pdsch_modulator_plan srsgpu_pdsch_modulator_plan;

/** Validates the transmissions (the reference's assertions: time allocation inside the slot, allocation inside the
 *  BWP and the grid, codeword length equal to the allocation's data REs x layers x Qm) and uploads the work. */
int srsgpu_pdsch_modulator_plan_create(srsgpu_context*                ctx,
                                       const srsgpu_pdsch_mod_config* cfgs,
                                       uint32_t                       nof_tx,
                                       uint32_t                       grid_nof_prb,
                                       uint32_t                       grid_nof_ports,
                                       srsgpu_pdsch_modulator_plan**  plan);

/** As srsgpu_pdsch_modulator_plan_create with an optional allocation extension per transmission (exts may be NULL):
 *  CRB-mask allocations, reserved RE patterns and per-PRG precoding. The data REs are the allocated CRBs' REs of the
 *  allocated symbols minus the BWP's DM-RS pattern on DM-RS symbols and the reserved patterns, in symbol-major,
 *  ascending-subcarrier order (resource_grid_mapper_impl.cpp:269). */
int srsgpu_pdsch_modulator_plan_create_ex(srsgpu_context*                ctx,
                                          const srsgpu_pdsch_mod_config* cfgs,
                                          const srsgpu_alloc_ext*        exts,
                                          uint32_t                       nof_tx,
                                          uint32_t                       grid_nof_prb,
                                          uint32_t                       grid_nof_ports,
                                          srsgpu_pdsch_modulator_plan**  plan);

/** Modulates and maps every planned transmission from d_codewords into d_grids (uint32 per RE: re | im << 16).
 *  Asynchronous on `stream`, hipGraph-capturable. */
int srsgpu_pdsch_modulator_plan_execute(const srsgpu_pdsch_modulator_plan* plan,
                                        const uint8_t*                     d_codewords,
                                        uint32_t*                          d_grids,
                                        void*                              stream);

void srsgpu_pdsch_modulator_plan_destroy(srsgpu_pdsch_modulator_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * PDSCH DM-RS — replaces srsran::dmrs_pdsch_processor::map(resource_grid_writer& grid, const config_t& config)
 * (include/srsran/phy/upper/signal_processors/dmrs_pdsch_processor.h:65, lib/phy/upper/signal_processors/
 * dmrs_pdsch_processor_impl.cpp:117) for every PDSCH transmission of a batch of slots: DM-RS sequence per symbol
 * (c_init = ((14 n_slot + l + 1)(2 N_ID + 1) 2^17 + 2 N_ID + n_SCID) mod 2^31), CDM cover codes of DM-RS ports
 * 0..nof_layers-1, per-CDM-group wideband precoding and mapping (bf16, same grid layout as the PDSCH modulator).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint16_t slot_index;           /* n_slot within the frame */
  uint16_t scrambling_id;        /* N_ID^{n_SCID} */
  uint8_t  n_scid;               /* 0 or 1 */
  uint8_t  dmrs_type;            /* 1 or 2 */
  uint8_t  nof_layers;           /* DM-RS ports 0..nof_layers-1 (1..4) */
  uint8_t  nof_ports;            /* antenna ports (precoding), nof_layers..grid_nof_ports */
  uint16_t dmrs_symbol_mask;     /* symbols_mask */
  uint16_t reference_point_k_rb; /* sequence reference RB (0: point A) */
  uint16_t rb_start;             /* contiguous CRB allocation (rb_mask), rb_start >= reference_point_k_rb */
  uint16_t nof_rb;
  float    amplitude;            /* DM-RS amplitude (beta) */
  float    precoding[4][4][2];   /* [port][layer] (re, im) */
  uint32_t grid_index;
} srsgpu_pdsch_dmrs_config;

typedef struct srsgpu_pdsch_dmrs_plan srsgpu_pdsch_dmrs_plan;

int srsgpu_pdsch_dmrs_plan_create(srsgpu_context*                 ctx,
                                  const srsgpu_pdsch_dmrs_config* cfgs,
                                  uint32_t                        nof_tx,
                                  uint32_t                        grid_nof_prb,
                                  uint32_t                        grid_nof_ports,
                                  srsgpu_pdsch_dmrs_plan**        plan);

/** As srsgpu_pdsch_dmrs_plan_create, with an optional extension per transmission (NULL array or NULL crb_mask: the
 *  contiguous rb_start / nof_rb allocation): crb_mask is dmrs_pdsch_processor::config_t::rb_mask (one byte per grid
 *  CRB, any pattern; the sequence skips the unallocated CRBs, dmrs_helper.cpp dmrs_sequence_generate). Reserved
 *  patterns and PRGs are rejected: the reference's DM-RS precoding has one PRG (dmrs_pdsch_processor_impl.cpp:149). */
int srsgpu_pdsch_dmrs_plan_create_ex(srsgpu_context*                 ctx,
                                     const srsgpu_pdsch_dmrs_config* cfgs,
                                     const srsgpu_alloc_ext*         exts,
                                     uint32_t                        nof_tx,
                                     uint32_t                        grid_nof_prb,
                                     uint32_t                        grid_nof_ports,
                                     srsgpu_pdsch_dmrs_plan**        plan);

/** Writes the DM-RS REs of every planned transmission into d_grids. Asynchronous on `stream`. */
int srsgpu_pdsch_dmrs_plan_execute(const srsgpu_pdsch_dmrs_plan* plan, uint32_t* d_grids, void* stream);

void srsgpu_pdsch_dmrs_plan_destroy(srsgpu_pdsch_dmrs_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * PDCCH — replaces srsran::pdcch_processor::process(resource_grid_writer& grid, const pdu_t& pdu)
 * (include/srsran/phy/upper/channel_processors/pdcch/pdcch_processor.h, lib/phy/upper/channel_processors/pdcch/
 * pdcch_processor_impl.cpp:79) for every DCI of a batch of slots, in one launch: the CCE to PRB mapping
 * (lib/ran/pdcch/cce_to_prb_mapping.cpp, at plan creation), DCI encoding (pdcch_encoder_impl.cpp: CRC24C with the RNTI,
 * the downlink polar code, rate matching), scrambling, QPSK and mapping (pdcch_modulator_impl.cpp) and the DM-RS
 * (signal_processors/dmrs_pdcch_processor_impl.cpp), into bf16 grids of the PDSCH modulator's layout. Bit-exact with
 * the reference. Only the REs of the DCIs' PRBs on the CORESET symbols are written.
 *
 * Precoding is one layer and one PRG: a weight per port. The reference's generic mapper does not define per-PRG
 * precoding for an allocation below its top PRG (resource_grid_mapper_impl.cpp:225). Powers are linear amplitudes, as
 * in the PDSCH configurations: data_scaling is pdcch_modulator::config_t::scaling (applied when it is a normal float),
 * dmrs_amplitude is dmrs_pdcch_processor::config_t::amplitude; the dB fields of the PDU are converted by the caller.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint64_t frequency_resources; /* coreset_description: bit i set = the 6-PRB frequency resource i (45 bits) */
  uint32_t bwp_size_rb;
  uint32_t bwp_start_rb;
  uint32_t start_symbol_index;
  uint32_t duration;            /* 1..3 symbols */
  uint32_t cce_to_reg_mapping;  /* 0 CORESET0, 1 non-interleaved, 2 interleaved */
  uint32_t reg_bundle_size;     /* interleaved only: 2 or 6 (duration 1, 2), 3 or 6 (duration 3) */
  uint32_t interleaver_size;    /* interleaved only: 2, 3 or 6 */
  uint32_t shift_index;         /* interleaved: n_shift; CORESET0: the cell identity */
  uint32_t slot_index;          /* n_slot within the frame (pdu_t::slot) */
  uint32_t rnti;                /* dci_description: scrambles the CRC */
  uint32_t n_id_pdcch_dmrs;
  uint32_t n_id_pdcch_data;
  uint32_t n_rnti;
  uint32_t cce_index;
  uint32_t aggregation_level;   /* 1, 2, 4, 8 or 16 */
  uint32_t nof_ports;           /* 1..grid_nof_ports */
  float    data_scaling;        /* linear amplitude of the data REs */
  float    dmrs_amplitude;      /* linear amplitude of the DM-RS REs */
  float    precoding[4][2];     /* [port] (re, im) */
  uint32_t payload_offset;      /* byte offset of the payload in d_payloads; bits packed MSB first */
  uint32_t nof_payload_bits;    /* 12..128, and fewer than 108 * aggregation_level - 24 */
  uint32_t grid_index;          /* resource grid (slot) the DCI is mapped into, < nof_grids */
  uint32_t reserved;
} srsgpu_pdcch_config;

typedef struct srsgpu_pdcch_plan srsgpu_pdcch_plan;

/** Refuses, with the reference's reason as the message, what pdcch_processor_validator_impl::is_valid, the polar
 *  code (36 <= K <= 164, K < E) and the CCE mapper's assertion refuse; a PRB outside the BWP or the grid; ports outside
 *  1..grid_nof_ports; and two DCIs that write the same REs (one launch gives them no order). */
int srsgpu_pdcch_plan_create(srsgpu_context*            ctx,
                             const srsgpu_pdcch_config* cfgs,
                             uint32_t                   nof_dcis,
                             uint32_t                   grid_nof_prb,
                             uint32_t                   grid_nof_ports,
                             uint32_t                   nof_grids,
                             srsgpu_pdcch_plan**        plan);

/** Encodes and maps every planned DCI: reads the payloads from d_payloads (payload_bytes bytes, device memory, so a
 *  captured graph carries new DCIs on every replay) and writes d_grids (uint32 per RE: re | im << 16). One launch,
 *  asynchronous on `stream`, allocation-free, hipGraph-capturable. */
int srsgpu_pdcch_plan_execute(const srsgpu_pdcch_plan* plan,
                              const uint8_t*           d_payloads,
                              uint64_t                 payload_bytes,
                              uint32_t*                d_grids,
                              void*                    stream);

void srsgpu_pdcch_plan_destroy(srsgpu_pdcch_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * SS/PBCH block — replaces srsran::ssb_processor::process(resource_grid_writer& grid, const pdu_t& pdu)
 * (include/srsran/phy/upper/channel_processors/ssb/ssb_processor.h, lib/phy/upper/channel_processors/ssb/
 * ssb_processor_impl.cpp:29) for every block of a batch of slots, in one launch: PBCH payload generation, first
 * scrambling, CRC24C, polar encoding and rate matching (pbch_encoder_impl.cpp:41-:163), second scrambling, QPSK and RE
 * mapping (pbch_modulator_impl.cpp:30-:91), the PBCH DM-RS (signal_processors/dmrs_pbch_processor_impl.cpp:29-:85), the
 * PSS and the SSS (pss_processor_impl.cpp, sss_processor_impl.cpp), on every port of a port list without precoding,
 * into bf16 grids of the PDSCH modulator's layout. Bit-exact with the reference. Only the REs the reference writes are
 * written: symbol l_start outside the PSS and the gaps beside the SSS stay as they are.
 *
 * l_start and k_start are derived at plan creation (include/srsran/ran/ssb/ssb_mapping.h:42 / :116). pss_amplitude is
 * linear, as in the PDCCH plan: the caller converts beta_pss. The 24 BCH payload bits and the SFN's four LSBs are read
 * from device memory at execution, four bytes per block: bytes 0-2 the payload, MSB first, byte 3 sfn & 15.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint32_t phys_cell_id;      /* 0..1007 */
  uint32_t ssb_idx;           /* < L_max */
  uint32_t L_max;             /* 4, 8 or 64 */
  uint32_t pattern_case;      /* ssb_pattern_case: 0..4 = A..E */
  uint32_t common_scs;        /* subCarrierSpacingCommon as a numerology: 0..2 for cases A-C, 2..4 for D and E */
  uint32_t offset_to_pointA;  /* 0..2199, in RBs of 15 kHz (A-C) or 60 kHz (D, E) */
  uint32_t subcarrier_offset; /* k_SSB: 0..23 (A-C) or 0..11 (D, E) */
  uint32_t slot_index;        /* pdu_t::slot.hrf_slot_index(): the slot within the half frame, block SCS */
  uint32_t hrf;               /* pdu_t::slot.is_odd_hrf() */
  float    pss_amplitude;     /* linear; finite */
  uint32_t nof_ports;         /* 1..4 */
  uint8_t  ports[4];          /* grid ports the block is written to, each once */
  uint32_t grid_index;        /* resource grid (slot) the block is mapped into, < nof_grids */
  uint32_t payload_offset;    /* byte offset of the block's four bytes in d_payloads */
  uint32_t reserved[2];
} srsgpu_ssb_config;

typedef struct srsgpu_ssb_plan srsgpu_ssb_plan;

/** Refuses, with the reference's reason as the message where it has one, a slot that is not the block's, the offsets
 *  and SCS combinations ssb_get_k_first asserts on, ssb_idx >= L_max, L_max outside {4, 8, 64}, a block outside the grid
 *  in subcarriers or symbols, a port outside the grid or listed twice, two blocks that write the same REs (one launch
 *  gives them no order), and grids past 2^32 words. */
int srsgpu_ssb_plan_create(srsgpu_context*          ctx,
                           const srsgpu_ssb_config* cfgs,
                           uint32_t                 nof_blocks,
                           uint32_t                 grid_nof_prb,
                           uint32_t                 grid_nof_ports,
                           uint32_t                 nof_grids,
                           srsgpu_ssb_plan**        plan);

/** Encodes and maps every planned block: reads the payloads and SFN bits from d_payloads (payload_bytes bytes, device
 *  memory, so a captured graph carries a new MIB or SFN on every replay) and writes d_grids (uint32 per RE:
 *  re | im << 16). One launch, asynchronous on `stream`, allocation-free, hipGraph-capturable. */
int srsgpu_ssb_plan_execute(const srsgpu_ssb_plan* plan,
                            const uint8_t*         d_payloads,
                            uint64_t               payload_bytes,
                            uint32_t*              d_grids,
                            void*                  stream);

void srsgpu_ssb_plan_destroy(srsgpu_ssb_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * NZP-CSI-RS — replaces srsran::nzp_csi_rs_generator::map(resource_grid_writer& grid, const config_t& config)
 * (include/srsran/phy/upper/signal_processors/nzp_csi_rs_generator.h, lib/phy/upper/signal_processors/
 * nzp_csi_rs_generator_impl.cpp:175) for every signal of a batch of slots, in one launch: the RE positions of TS 38.211
 * Table 7.4.1.5.3-1 (lib/ran/csi_rs/csi_rs_pattern.cpp, at plan creation), the sequence (:111, c_init :123, the skipped
 * elements :72, the length :142), the w_f cover (:291) and the precoding of each CDM group onto all ports, into bf16
 * grids of the PDSCH modulator's layout. Bit-exact with the reference. Only the words the reference writes are written:
 * with the identity matrix these include zeros on the ports of the other CDM group (rows 4 and 5).
 *
 * Rows 1-5 (1, 2 or 4 ports; no CDM or FD-CDM2). Rows 6-12 need 8-16 grid ports and are refused, rows 13-18 the
 * reference refuses itself. Precoding is one PRG: a ports x ports matrix (the same mapper reason as the PDCCH plan).
 * amplitude is config_t::amplitude, linear. Extended CP changes c_init and the l_0 range; the grid keeps 14 symbols.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint32_t slot_index;        /* n_slot within the frame (config_t::slot) */
  uint32_t cp;                /* 0 normal, 1 extended */
  uint32_t start_rb;          /* first RB of the resource, from CRB 0 = grid PRB 0 */
  uint32_t nof_rb;
  uint32_t row;               /* csi_rs_mapping_table_row: 1..5 */
  uint32_t nof_k_ref;         /* entries of freq_allocation_ref_idx: 1 for rows 1..5 */
  uint32_t k_ref[6];          /* freq_allocation_ref_idx (k_0, ...) */
  uint32_t symbol_l0;
  uint32_t symbol_l1;         /* unused by rows 1..5 */
  uint32_t cdm;               /* csi_rs_cdm_type: 0 no_CDM, 1 fd_CDM2, 2 cdm4_FD2_TD2, 3 cdm8_FD2_TD4 */
  uint32_t freq_density;      /* csi_rs_freq_density_type: 0 dot5_even_RB, 1 dot5_odd_RB, 2 one, 3 three */
  uint32_t scrambling_id;     /* 0..1023 */
  float    amplitude;         /* linear; finite */
  uint32_t nof_ports;         /* ports and layers of the precoding matrix: the row's ports */
  float    precoding[4][4][2]; /* [port][layer] (re, im) */
  uint32_t grid_index;        /* resource grid (slot) the signal is mapped into, < nof_grids */
  uint32_t reserved;
} srsgpu_csi_rs_config;

typedef struct srsgpu_csi_rs_plan srsgpu_csi_rs_plan;

/** Refuses, with the reference's reason as the message where it has one, what the pattern's assertions refuse (k_ref
 *  count and range, density and CDM per row, l_0 outside the slot, the precoding's dimensions), rows above 5, row 5
 *  with l_0 on the last symbol, RBs or ports outside the grid, an amplitude that is not finite, and two signals that
 *  write the same REs (one launch gives them no order). */
int srsgpu_csi_rs_plan_create(srsgpu_context*             ctx,
                              const srsgpu_csi_rs_config* cfgs,
                              uint32_t                    nof_signals,
                              uint32_t                    grid_nof_prb,
                              uint32_t                    grid_nof_ports,
                              uint32_t                    nof_grids,
                              srsgpu_csi_rs_plan**        plan);

/** Writes every planned signal into d_grids (uint32 per RE: re | im << 16). One launch, asynchronous on `stream`,
 *  allocation-free, hipGraph-capturable. */
int srsgpu_csi_rs_plan_execute(const srsgpu_csi_rs_plan* plan, uint32_t* d_grids, void* stream);

void srsgpu_csi_rs_plan_destroy(srsgpu_csi_rs_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * PUCCH Formats 0 and 1 — replaces srsran::pucch_processor::process(grid, format0_configuration) and
 * process(grid, format1_batch_configuration) (lib/phy/upper/channel_processors/pucch/pucch_processor_impl.cpp:42 / :74)
 * with the detectors behind them (pucch_detector_format0.cpp:114, pucch_detector_format1.cpp:156) for every Format 0
 * PDU and every Format 1 resource (one PRB, or two with hopping, and all PUCCHs multiplexed on it) of a batch of
 * slots, in one launch, from bf16 grids of the uplink plans' layout to the UCI bits and the channel state.
 *
 * PRBs are grid PRBs (the BWP start already added). Format 0 reads the listed grid ports; Format 1 reads grid ports
 * 0..nof_rx_ports-1, as the reference's Format 1 detector does whatever its configuration lists. All powers are
 * linear; the caller takes 10 log10. Group and sequence hopping are not supported (the reference terminates).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint16_t slot_index;           /* n_slot within the frame */
  uint8_t  numerology;           /* 0..4 */
  uint8_t  cp_extended;          /* 1: extended CP (numerology 2 only), 12 symbols per slot */
  uint16_t starting_prb;
  uint16_t second_hop_prb;       /* 0xffff: no hopping */
  uint8_t  start_symbol_index;
  uint8_t  nof_symbols;          /* 1 or 2 */
  uint8_t  initial_cyclic_shift; /* 0..11 */
  uint8_t  nof_harq_ack;         /* 0..2 */
  uint16_t n_id;                 /* 0..1023 */
  uint8_t  sr_opportunity;       /* 0 or 1 */
  uint8_t  nof_ports;            /* 1..4 */
  uint8_t  ports[4];             /* grid ports, in the order of format0_configuration::ports */
  uint32_t grid_index;
} srsgpu_pucch_f0_config;

typedef struct {
  uint16_t slot_index;
  uint8_t  numerology;
  uint8_t  cp_extended;
  uint16_t starting_prb;
  uint16_t second_hop_prb;       /* 0xffff: no hopping */
  uint8_t  start_symbol_index;   /* 0..10 */
  uint8_t  nof_symbols;          /* 4..14 */
  uint16_t n_id;
  uint8_t  nof_rx_ports;         /* grid ports 0..nof_rx_ports-1; times the hops one of 1, 2, 4, 8 */
  uint8_t  reserved[3];
  uint32_t grid_index;
  uint32_t first_entry;          /* the resource's entries are f1_entries[first_entry .. first_entry + nof_entries) */
  uint32_t nof_entries;          /* 1..84 */
} srsgpu_pucch_f1_resource;

typedef struct {
  uint8_t initial_cyclic_shift;  /* 0..11 */
  uint8_t time_domain_occ;       /* below the data symbols of the shorter hop */
  uint8_t nof_harq_ack;          /* 0 (SR only), 1 or 2 */
  uint8_t reserved;
} srsgpu_pucch_f1_entry;

/** One per Format 0 PDU, then one per Format 1 entry, in the caller's order. */
typedef struct {
  uint8_t  sr;                /* Format 0 with an SR opportunity: the SR bit; otherwise 0 */
  uint8_t  harq_ack[2];       /* the detected HARQ-ACK bits (Format 1 SR only: harq_ack[0] is the detected bit) */
  uint8_t  status;            /* 0 invalid, 1 valid */
  float    detection_metric;  /* Format 0: best_metric; Format 1: the metric over its threshold */
  float    epre;
  float    rsrp;              /* Format 0: the chosen sequence's sum_corr, as the reference reports it */
  float    noise_var;         /* Format 0: the chosen sequence's sum_noise_var; Format 1: the resource's variance */
  uint32_t reserved[3];       /* written as zero */
} srsgpu_pucch_result;

typedef struct srsgpu_pucch_detector_plan srsgpu_pucch_detector_plan;

/** Refuses what pucch_pdu_validator_impl::is_valid and the detectors' assertions refuse, and where the reference is
 *  undefined: a Format 1 resource without entries, a time_domain_occ not below the data symbols of the shorter hop,
 *  two entries of a resource with the same (cyclic shift, OCC), nof_rx_ports x hops outside {1, 2, 4, 8}, and a PRB,
 *  port or grid outside the grids. */
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
                                      srsgpu_pucch_detector_plan**    plan);

/** Detects every planned PDU and resource: reads d_grids (uint32 per RE: re | im << 16, bf16; nof_grids x ports x 14 x
 *  12 PRBs) and writes the nof_f0 + nof_entries results. One launch, asynchronous on `stream`, allocation-free,
 *  hipGraph-capturable. */
int srsgpu_pucch_detector_plan_execute(const srsgpu_pucch_detector_plan* plan,
                                       const uint32_t*                   d_grids,
                                       srsgpu_pucch_result*              d_results,
                                       void*                             stream);

void srsgpu_pucch_detector_plan_destroy(srsgpu_pucch_detector_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * PRACH detector — replaces srsran::prach_detector::detect(const prach_buffer&, const configuration&)
 * (include/srsran/phy/upper/channel_processors/prach_detector.h:78, the generic detector of
 * lib/phy/upper/channel_processors/prach_detector_generic_impl.cpp:80 with the factory's IDFT sizes 1024 / 256) for
 * every occasion of a batch in one launch: correlation with every root sequence on every port, the cyclic-shift
 * windows with their noise estimates, and the decision per preamble.
 *
 * An occasion carries the physical values the detector computes with, not the PDU's indices: N_cs (what
 * prach_cyclic_shifts_get returns for the zone), the Zadoff-Chu roots u of its root sequences (TS 38.211 Tables
 * 6.3.3.1-3 / -4 applied to root_sequence_index + i), and the threshold and window margin of
 * detail::get_threshold_and_margin. Unrestricted sets only. All powers are linear; delays are in samples of the IDFT:
 * time_advance = delay_samples / (N x ra_scs), N = 1024 (long) or 256 (short).
 * ------------------------------------------------------------------------------------------------------------------ */
enum {
  SRSGPU_PRACH_FORMAT_0 = 0, SRSGPU_PRACH_FORMAT_1, SRSGPU_PRACH_FORMAT_2, SRSGPU_PRACH_FORMAT_3, SRSGPU_PRACH_FORMAT_A1,
  SRSGPU_PRACH_FORMAT_A2, SRSGPU_PRACH_FORMAT_A3, SRSGPU_PRACH_FORMAT_B1, SRSGPU_PRACH_FORMAT_B4, SRSGPU_PRACH_FORMAT_C0,
  SRSGPU_PRACH_FORMAT_C2, SRSGPU_PRACH_FORMAT_A1_B1, SRSGPU_PRACH_FORMAT_A2_B2, SRSGPU_PRACH_FORMAT_A3_B3
};                                /* the order of prach_format_type */
enum {
  SRSGPU_PRACH_SCS_15 = 0, SRSGPU_PRACH_SCS_30, SRSGPU_PRACH_SCS_60, SRSGPU_PRACH_SCS_120, SRSGPU_PRACH_SCS_1_25,
  SRSGPU_PRACH_SCS_5
};                                /* the order of prach_subcarrier_spacing */
#define SRSGPU_PRACH_MAX_PREAMBLES 64

typedef struct {
  uint8_t  format;               /* SRSGPU_PRACH_FORMAT_* */
  uint8_t  ra_scs;               /* SRSGPU_PRACH_SCS_*: 1.25 kHz for Formats 0-2, 5 kHz for Format 3, 15-120 kHz for the short ones */
  uint8_t  nof_rx_ports;         /* 1..4 */
  uint8_t  combine_symbols;      /* 1: the symbols of a port are summed before the correlation (the factory's default) */
  uint16_t n_cs;                 /* N_cs, 0..L_RA */
  uint16_t nof_roots;            /* 64 when n_cs == 0, else ceil(64 / min(64, L_RA / n_cs)) */
  uint32_t root_offset;          /* the roots u of the root sequences are roots[root_offset .. root_offset + nof_roots) */
  uint8_t  start_preamble_index; /* monitored preambles [start, start + nof), within 0..64 */
  uint8_t  nof_preamble_indices; /* 1..64 */
  uint16_t win_margin;           /* > 0, samples of the IDFT */
  float    threshold;            /* > 0 */
  uint32_t sample_offset;        /* word of (port 0, symbol 0, RE 0) in the input */
  uint32_t port_stride;          /* words between ports */
  uint32_t symbol_stride;        /* words between symbols; the L_RA REs of a symbol are consecutive */
  uint32_t result_index;         /* the occasion's srsgpu_prach_result; a permutation of 0..nof_occasions-1 over the plan */
} srsgpu_prach_occasion;

typedef struct {
  uint32_t detected;             /* 1: peak > threshold and delay_samples < 0.8 x the maximum delay */
  uint32_t delay_samples;        /* position of the first largest sample of the preamble's window */
  float    metric;               /* peak / threshold (prach_detection_result::preamble_indication::detection_metric) */
  float    peak;
} srsgpu_prach_preamble;

/** One per occasion. A preamble outside the monitored range is all zero; so is every preamble after an early stop. */
typedef struct {
  float                 rssi;        /* linear, with the reference's arithmetic (divided by L_RA twice) */
  uint32_t              early_stop;  /* 1: the RSSI is no normal number and nothing was detected (detect()'s early return) */
  uint32_t              reserved[2]; /* written as zero */
  srsgpu_prach_preamble preambles[SRSGPU_PRACH_MAX_PREAMBLES];  /* by preamble index: the order of the indications */
} srsgpu_prach_result;

typedef struct srsgpu_prach_detector_plan srsgpu_prach_detector_plan;

/** Refuses what detect() asserts on and what it leaves undefined: monitored preambles outside 0..64 or none, ports
 *  outside 1..4, a format / SCS pair without preamble information, n_cs > L_RA, a root outside 1..L_RA-1, a wrong
 *  nof_roots, threshold <= 0 or win_margin == 0, a window with its margins longer than the IDFT, samples outside the
 *  input_words words of the input, and two occasions with one result. */
int srsgpu_prach_detector_plan_create(srsgpu_context*              ctx,
                                      const srsgpu_prach_occasion* occasions,
                                      uint32_t                     nof_occasions,
                                      const uint16_t*              roots,
                                      uint32_t                     nof_roots,
                                      uint64_t                     input_words,
                                      srsgpu_prach_detector_plan** plan);

/** Detects every occasion: reads d_input (uint32 per RE: re | im << 16, bf16, as prach_buffer holds them) and writes
 *  every byte of the nof_occasions results. One launch for long and short occasions together, asynchronous on
 *  `stream`, allocation-free, hipGraph-capturable. */
int srsgpu_prach_detector_plan_execute(const srsgpu_prach_detector_plan* plan,
                                       const uint32_t*                   d_input,
                                       srsgpu_prach_result*              d_results,
                                       void*                             stream);

void srsgpu_prach_detector_plan_destroy(srsgpu_prach_detector_plan* plan);

/** max_delay_samples of detect() (prach_detector_generic_impl.cpp:159) for a format, SCS and N_cs, in samples of the
 *  IDFT: time_advance_max = 0.8 x it / (N x ra_scs). No device call. Fails for a format / SCS pair without preamble
 *  information or N_cs > L_RA. */
int srsgpu_prach_max_delay_samples(uint32_t format, uint32_t ra_scs, uint32_t n_cs, uint32_t* max_delay_samples);

/* ------------------------------------------------------------------------------------------------------------------
 * SRS estimator — replaces srsran::srs_estimator::estimate(const resource_grid_reader&, const
 * srs_estimator_configuration&) (include/srsran/phy/upper/signal_processors/srs/srs_estimator.h, the generic estimator
 * of lib/phy/upper/signal_processors/srs/srs_estimator_generic_impl.cpp:79 with get_srs_information of
 * lib/ran/srs/srs_information.cpp:38, the DFT time alignment estimator of
 * lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.cpp:174 / :245 and the low-PAPR sequences
 * of lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.cpp:243) for every SRS resource of a batch of
 * slots in one launch, from bf16 grids of the uplink plans' layout to the wideband channel matrix, the EPRE, the noise
 * variance and the time alignment.
 *
 * A resource carries physical values. The row of TS 38.211 Table 6.4.1.4.3-1 that C_SRS selects arrives as data: the
 * four (m_srs[b], N[b]) pairs, which a binding fills from srs_configuration_get(c_srs, b), b = 0..3. Subcarriers are
 * grid subcarriers. All powers are linear; the caller takes 10 log10. The reference reports time_alignment.min as the
 * smallest positive double (srs_estimator_generic_impl.cpp:115 / :203); the plan reports ta_max only and the lower
 * bound is -ta_max. Frequency, group and sequence hopping are not supported (the reference refuses them).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint16_t m_srs[4];          /* m_SRS,b of the C_SRS row, b = 0..3: multiples of 4, m_srs[b] N[b] = m_srs[b - 1] */
  uint8_t  N[4];              /* N_b of the row; N[0] = 1 */
  uint8_t  numerology;        /* 0..4: the subcarrier spacing, 15 kHz << numerology */
  uint8_t  nof_antenna_ports; /* 1, 2 or 4 */
  uint8_t  nof_symbols;       /* 1, 2 or 4 */
  uint8_t  start_symbol;      /* start_symbol + nof_symbols <= 14 */
  uint8_t  comb_size;         /* K_TC: 2 or 4 */
  uint8_t  comb_offset;       /* < comb_size */
  uint8_t  cyclic_shift;      /* < 8 (comb 2) or < 12 (comb 4) */
  uint8_t  bandwidth_index;   /* B_SRS, 0..3 */
  uint8_t  freq_hopping;      /* b_hop, 0..3; below bandwidth_index is frequency hopping, which is refused */
  uint8_t  hopping;           /* group_or_sequence_hopping_enum: 0 neither; anything else is refused */
  uint8_t  nof_rx_ports;      /* 1..4 */
  uint8_t  reserved;
  uint8_t  rx_ports[4];       /* grid ports, in the order of srs_estimator_configuration::ports */
  uint16_t sequence_id;       /* n_ID^SRS, 0..1023 */
  uint16_t freq_shift;        /* n_shift, 0..268 */
  uint16_t freq_position;     /* n_RRC, 0..67 */
  uint16_t reserved2;
  uint32_t grid_index;        /* < nof_grids */
  uint32_t result_index;      /* the resource's srsgpu_srs_result; a permutation of 0..nof_resources-1 over the plan */
} srsgpu_srs_config;

/** One per resource, 192 bytes, every byte written by every execute. */
typedef struct {
  float    channel[4][4][2];  /* [rx port index][tx port] (re, im): srs_channel_matrix; unused entries zero */
  double   time_alignment;    /* seconds: the mean over the tx ports */
  double   resolution;        /* 1 / fs, fs = IDFT size x subcarrier spacing x comb_size */
  double   ta_max;            /* max_ta_samples / fs; the measurement lies in [-ta_max, ta_max] */
  float    epre;              /* linear */
  float    noise_var;         /* linear */
  int32_t  ta_idx[4];         /* per tx port: the peak's tap before the fractional refinement (negative: advanced) */
  uint32_t reserved[4];       /* written as zero */
} srsgpu_srs_result;

typedef struct srsgpu_srs_estimator_plan srsgpu_srs_estimator_plan;

/** Refuses what srs_validator_generic_impl::is_valid and the estimator's assertions refuse (an invalid resource,
 *  frequency hopping, group or sequence hopping, no rx port, a resource past the grid, start_symbol + nof_symbols > 14)
 *  and in addition: port, symbol or comb counts outside their sets, an rx port outside the grid or listed twice, a
 *  table row that is not self-consistent, a grid outside the grids, and a result_index outside the resources or used
 *  twice. The bandwidth check walks the antenna ports (the reference's validator walks the rx port count,
 *  srs_validator_generic_impl.cpp:52-53). Blocking. */
int srsgpu_srs_estimator_plan_create(srsgpu_context*             ctx,
                                     const srsgpu_srs_config*    resources,
                                     uint32_t                    nof_resources,
                                     uint32_t                    grid_nof_prb,
                                     uint32_t                    grid_nof_ports,
                                     uint32_t                    nof_grids,
                                     srsgpu_srs_estimator_plan** plan);

/** Estimates every planned resource: reads d_grids (uint32 per RE: re | im << 16, bf16; nof_grids x ports x 14 x
 *  12 PRBs) and writes every byte of the nof_resources results. One launch, one workgroup per resource, asynchronous
 *  on `stream`, allocation-free, hipGraph-capturable. */
int srsgpu_srs_estimator_plan_execute(const srsgpu_srs_estimator_plan* plan,
                                      const uint32_t*                  d_grids,
                                      srsgpu_srs_result*               d_results,
                                      void*                            stream);

void srsgpu_srs_estimator_plan_destroy(srsgpu_srs_estimator_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * PUCCH Format 2 front end — the part of srsran::pucch_processor::process(const resource_grid_reader&, const
 * format2_configuration&) (lib/phy/upper/channel_processors/pucch/pucch_processor_impl.cpp:145) in front of the UCI
 * decoder: dmrs_pucch_estimator_format2::estimate (lib/phy/upper/signal_processors/pucch/
 * dmrs_pucch_estimator_format2.cpp:87, over port_channel_estimator_average_impl with filter smoothing, the average
 * time strategy and no CFO compensation) and pucch_demodulator_format2::demodulate
 * (lib/phy/upper/channel_processors/pucch/pucch_demodulator_format2.cpp:92: ZF 1 x N, QPSK, descrambling), for every
 * Format 2 PDU of a batch of slots in one launch, from bf16 grids of the uplink plans' layout to descrambled int8 LLRs
 * and the per-port channel state. The LLRs lie where srsgpu_uci_decoder_plan (3..11 bits, Qm 2) and
 * srsgpu_uci_polar_decoder_plan (12 bits and more) read them in place: E = 16 nof_prb nof_symbols at llr_offset.
 *
 * PRBs are grid PRBs (the BWP start already added). Group hopping is NEITHER in the reference's processor and no
 * parameter here. As in the reference, the data REs of receive port i are read from grid port i and its pilots from
 * grid port ports[i] (pucch_demodulator_format2.cpp:185): the two agree for the port list 0..P-1. All powers are
 * linear; the caller takes 10 log10 and combines the ports as channel_estimate::get_channel_state_information does.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint16_t slot_index;         /* slot within the frame, < 10 << numerology */
  uint8_t  numerology;         /* 0..4 */
  uint8_t  cp_extended;        /* 0 normal, 1 extended (numerology 2 only) */
  uint16_t starting_prb;       /* first grid PRB of the first (or only) hop */
  uint16_t second_hop_prb;     /* first grid PRB of the second symbol; 0xffff: no intra-slot hopping */
  uint8_t  nof_prb;            /* 1..16 */
  uint8_t  start_symbol_index; /* start_symbol_index + nof_symbols <= 14 (12 with the extended CP) */
  uint8_t  nof_symbols;        /* 1..2; hopping needs 2 */
  uint8_t  nof_ports;          /* 1..4 */
  uint16_t rnti;               /* scrambling: c_init = rnti 2^15 + n_id */
  uint16_t n_id;               /* 0..1023 */
  uint16_t n_id_0;             /* DM-RS scrambling identity, 0..65535 */
  uint16_t nof_uci_bits;       /* HARQ-ACK + SR + CSI Part 1 bits, 3..1706; validation only */
  uint8_t  ports[4];           /* grid ports, in the order of format2_configuration::ports */
  uint32_t grid_index;         /* < nof_grids */
  uint32_t llr_offset;         /* first of the PDU's 16 nof_prb nof_symbols LLRs in d_llrs; a multiple of 4 */
} srsgpu_pucch_f2_config;

/** One per PDU, in PDU order, 96 bytes, every byte written by every execute; entries of ports past nof_ports are 0. */
typedef struct {
  float  noise_var[4];      /* linear, already floored at rsrp / 10^10 */
  float  rsrp[4];           /* linear */
  float  epre[4];           /* linear */
  float  cfo_hz[4];         /* NaN when no hop has two symbols; reported, never compensated */
  double time_alignment[4]; /* seconds, a multiple of T_c: the mean of the hops */
} srsgpu_pucch_f2_result;

typedef struct srsgpu_pucch_f2_plan srsgpu_pucch_f2_plan;

/** Refuses what pucch_pdu_validator_impl::is_valid and the estimator's and demodulator's assertions refuse (nof_prb
 *  outside 1..16, symbols outside 1..2, hopping with one symbol, PRBs or symbols outside the grid or the slot, no
 *  ports or more than the grid has, an effective code rate above 0.8 -- checked before the payload size, as there --
 *  and a payload outside 3..1706 bits) and in addition: a port outside the grid or listed twice, a numerology, slot
 *  index, cyclic prefix or n_id outside its range, a grid_index outside the grids, an llr_offset that is no multiple
 *  of 4 and LLR ranges of two PDUs that overlap. A refused create leaves no live device buffer. Blocking. */
int srsgpu_pucch_f2_plan_create(srsgpu_context*               ctx,
                                const srsgpu_pucch_f2_config* pdus,
                                uint32_t                      nof_pdus,
                                uint32_t                      grid_nof_prb,
                                uint32_t                      grid_nof_ports,
                                uint32_t                      nof_grids,
                                srsgpu_pucch_f2_plan**        plan);

/** Processes every planned PDU: reads d_grids (uint32 per RE: re | im << 16, bf16; nof_grids x ports x 14 x 12 PRBs),
 *  writes the PDUs' LLRs into d_llrs (nothing outside their ranges) and every byte of the nof_pdus results. One
 *  launch, one workgroup per PDU, asynchronous on `stream`, allocation-free, hipGraph-capturable. */
int srsgpu_pucch_f2_plan_execute(const srsgpu_pucch_f2_plan* plan,
                                 const uint32_t*             d_grids,
                                 int8_t*                     d_llrs,
                                 srsgpu_pucch_f2_result*     d_results,
                                 void*                       stream);

void srsgpu_pucch_f2_plan_destroy(srsgpu_pucch_f2_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * PUCCH Format 3 / 4 front end — the part of srsran::pucch_processor::process(const resource_grid_reader&, const
 * format3_configuration&) and (..., const format4_configuration&) (lib/phy/upper/channel_processors/pucch/
 * pucch_processor_impl.cpp:227 / :315) in front of the UCI decoder: dmrs_pucch_estimator_formats3_4::estimate
 * (lib/phy/upper/signal_processors/pucch/dmrs_pucch_estimator_formats3_4.cpp:94, over
 * port_channel_estimator_average_impl with mean smoothing, the average time strategy and no CFO compensation:
 * signal_processor_factories.cpp:146) and pucch_demodulator_format3 / format4::demodulate (ZF 1 x N per data symbol,
 * the 12 nof_prb-point inverse DFT scaled by 1 / sqrt(12 nof_prb), the mean of the valid noise variances, Format 4's
 * inverse block-wise spreading, QPSK or pi/2-BPSK soft demapping, descrambling), for every Format 3 and Format 4 PDU of
 * a batch of slots in one launch, from bf16 grids of the uplink plans' layout to descrambled int8 LLRs and the per-port
 * channel state. The LLRs lie where srsgpu_uci_decoder_plan (3..11 bits, Qm 1 or 2) and
 * srsgpu_uci_polar_decoder_plan (12 bits and more) read them in place: E = 12 nof_prb n_data Qm for Format 3 and
 * 12 n_data Qm / occ_length for Format 4 at llr_offset, n_data the symbols without DM-RS (TS 38.211 Table
 * 6.4.1.3.3.2-1), Qm 1 with pi2_bpsk and 2 without.
 *
 * PRBs are grid PRBs (the BWP start already added). Group hopping is NEITHER in the reference's processor and no
 * parameter here. Data REs and pilots of receive port i both come from grid port ports[i]
 * (pucch_formats3_4_helpers.h:208), unlike Format 2. All powers are linear; the caller takes 10 log10 and combines the
 * ports as channel_estimate::get_channel_state_information does. The result record is srsgpu_pucch_f2_result with its
 * meaning unchanged; the time alignment is 0 for every port, which is what the reference reports under mean smoothing
 * (its estimator sees one constant per hop).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint16_t slot_index;         /* slot within the frame, < 10 << numerology */
  uint8_t  format;             /* 3 or 4 */
  uint8_t  numerology;         /* 0..4 */
  uint8_t  cp_extended;        /* 0 normal, 1 extended (numerology 2 only) */
  uint8_t  nof_prb;            /* Format 3: 1..16 of the form 2^a 3^b 5^c; Format 4: 1 */
  uint8_t  start_symbol_index; /* start_symbol_index + nof_symbols <= 14 (12 with the extended CP) */
  uint8_t  nof_symbols;        /* 4..14 */
  uint16_t starting_prb;       /* first grid PRB of the first (or only) hop */
  uint16_t second_hop_prb;     /* first grid PRB from symbol nof_symbols / 2 on; 0xffff: no intra-slot hopping */
  uint8_t  additional_dmrs;    /* 0 or 1: four DM-RS symbols for 10..14 symbols */
  uint8_t  pi2_bpsk;           /* 0: QPSK, 1: pi/2-BPSK */
  uint8_t  occ_length;         /* Format 4: 2 or 4; Format 3: ignored */
  uint8_t  occ_index;          /* Format 4: < occ_length; Format 3: ignored */
  uint16_t rnti;               /* scrambling: c_init = rnti 2^15 + n_id_scrambling */
  uint16_t n_id_scrambling;    /* 0..1023 */
  uint16_t n_id_hopping;       /* 0..1023: u = n_id_hopping mod 30 and the cyclic shift hopping n_cs */
  uint16_t nof_uci_bits;       /* HARQ-ACK + SR + CSI Part 1 bits, 3..1706; validation only */
  uint8_t  nof_ports;          /* 1..4 */
  uint8_t  ports[4];           /* grid ports, in the order of formatN_configuration::ports */
  uint8_t  reserved[3];        /* 0 */
  uint32_t grid_index;         /* < nof_grids */
  uint32_t llr_offset;         /* first of the PDU's E LLRs in d_llrs; a multiple of 4 (E itself need not be one) */
} srsgpu_pucch_f34_config;

typedef struct srsgpu_pucch_f34_plan srsgpu_pucch_f34_plan;

/** Refuses what pucch_pdu_validator_impl::is_valid (pucch_processor_impl.cpp:616 / :703) refuses (PRBs or symbols
 *  outside the grid or the slot, no ports or more than the grid has, an effective code rate above 0.8 -- checked
 *  before the payload size, as there --, a payload outside 3..1706 bits, nof_prb outside 1..16, occ_length other than
 *  2 or 4), what the demodulators and the transform precoder assert on (nof_symbols outside 4..14, a nof_prb that is no
 *  2^a 3^b 5^c -- the validator admits 7, 11, 13 and 14 --, occ_index >= occ_length) and in addition: a format other
 *  than 3 or 4, a Format 4 nof_prb other than 1, a port outside the grid or listed twice, a numerology, slot index,
 *  cyclic prefix, flag or identity outside its range, a grid_index outside the grids, an llr_offset that is no
 *  multiple of 4 and LLR ranges of two PDUs that overlap. A refused create leaves no live device buffer. Blocking. */
int srsgpu_pucch_f34_plan_create(srsgpu_context*                ctx,
                                 const srsgpu_pucch_f34_config* pdus,
                                 uint32_t                       nof_pdus,
                                 uint32_t                       grid_nof_prb,
                                 uint32_t                       grid_nof_ports,
                                 uint32_t                       nof_grids,
                                 srsgpu_pucch_f34_plan**        plan);

/** Processes every planned PDU: reads d_grids (uint32 per RE: re | im << 16, bf16; nof_grids x ports x 14 x 12 PRBs),
 *  writes each PDU's E LLRs into d_llrs (4-byte aligned; nothing outside the ranges, whose tails are stored by bytes)
 *  and every byte of the nof_pdus results (entries of ports past nof_ports are 0). One launch, one workgroup per PDU,
 *  asynchronous on `stream`, allocation-free, hipGraph-capturable. */
int srsgpu_pucch_f34_plan_execute(const srsgpu_pucch_f34_plan* plan,
                                  const uint32_t*              d_grids,
                                  int8_t*                      d_llrs,
                                  srsgpu_pucch_f2_result*      d_results,
                                  void*                        stream);

void srsgpu_pucch_f34_plan_destroy(srsgpu_pucch_f34_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * OFDM slot modulator / demodulator — replace srsran::ofdm_slot_modulator::modulate(span<cf_t> output,
 * const resource_grid_reader& grid, unsigned port_index, unsigned slot_index)
 * (include/srsran/phy/lower/modulation/ofdm_modulator.h:100, lib/phy/lower/modulation/ofdm_modulator_impl.cpp:115,
 * per symbol :56) and ofdm_slot_demodulator::demodulate(resource_grid_writer& grid, span<const cf_t> input,
 * unsigned port_index, unsigned slot_index) (ofdm_demodulator.h:102, ofdm_demodulator_impl.cpp:154, per symbol :94),
 * batched over every (grid, port, symbol) of a set of slots.
 * Modulator, per symbol: grid subcarriers [0, rg/2) -> DFT bins [N - rg/2, N), [rg/2, rg) -> bins [0, rg/2), inverse
 * DFT (unnormalised), times the TS 38.211 section 5.4 phase compensation (phase_compensation_lut.h) and `scale`, CP =
 * copy of the last cp_len samples. Demodulator: N samples from cp_len - window_offset, direct DFT, the same
 * compensation (receive sign) and the DFT-window phase ramp, bins back to the grid as bf16.
 * Grids: nof_ports x nsymb (14, or 12 with extended CP) x 12 * bw_rb uint32 (re | im << 16, bf16), grid g at
 * g * nof_ports * nsymb * 12 * bw_rb. Time samples: complex float (re, im) interleaved, one slot of (grid g, port p)
 * at srsgpu_ofdm_plan_sample_offset(plan, g, p) (grids, then ports, consecutively).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint32_t numerology;                /* subcarrier spacing 15 kHz x 2^numerology, 0..4 */
  uint32_t bw_rb;                     /* resource grid bandwidth in RB: 12 * bw_rb < dft_size */
  uint32_t dft_size;                  /* 2^n 128..8192, 3 x 2^m 384..6144, 4608 (generic DFT sizes) */
  uint32_t cp_extended;               /* 0: normal cyclic prefix (14 symbols), 1: extended (12 symbols) */
  uint32_t nof_samples_window_offset; /* demodulator DFT window advance, < 144 * dft_size / 2048 (0: none) */
  float    scale;                     /* scaling factor at the DFT output (std::isnormal) */
  double   center_freq_hz;            /* carrier centre frequency for the phase compensation */
} srsgpu_ofdm_config;

typedef struct srsgpu_ofdm_plan srsgpu_ofdm_plan;

/** Plans the modulation of nof_grids slots (grid g is slot slot_index[g] within its subframe) of nof_ports ports. */
int srsgpu_ofdm_modulator_plan_create(srsgpu_context*           ctx,
                                      const srsgpu_ofdm_config* cfg,
                                      uint32_t                  nof_grids,
                                      uint32_t                  nof_ports,
                                      const uint32_t*           slot_index,
                                      srsgpu_ofdm_plan**        plan);

/** Plans the demodulation of nof_grids slots of nof_ports ports (same layouts). */
int srsgpu_ofdm_demodulator_plan_create(srsgpu_context*           ctx,
                                        const srsgpu_ofdm_config* cfg,
                                        uint32_t                  nof_grids,
                                        uint32_t                  nof_ports,
                                        const uint32_t*           slot_index,
                                        srsgpu_ofdm_plan**        plan);

/** Symbol-granularity plans — replace srsran::ofdm_symbol_modulator::modulate(output, grid, port, symbol_index) and
 *  ofdm_symbol_demodulator::demodulate(grid, input, port, symbol_index) (include/srsran/phy/lower/modulation/
 *  ofdm_modulator.h:58, ofdm_demodulator.h:59), batched over ports and a run of consecutive symbols: symbols
 *  [first_symbol, first_symbol + nof_symbols) of slot `slot_index` of the subframe (the symbol index within the
 *  subframe the reference passes is slot_index * symbols_per_slot + first_symbol). Layouts: grid rows
 *  [port][symbol - first_symbol][subcarrier]; samples [port][CP + N of each symbol, consecutive]
 *  (srsgpu_ofdm_plan_sample_offset(plan, 0, port)). Executed with srsgpu_ofdm_(de)modulator_plan_execute. */
int srsgpu_ofdm_modulator_symbols_plan_create(srsgpu_context*           ctx,
                                              const srsgpu_ofdm_config* cfg,
                                              uint32_t                  nof_ports,
                                              uint32_t                  slot_index,
                                              uint32_t                  first_symbol,
                                              uint32_t                  nof_symbols,
                                              srsgpu_ofdm_plan**        plan);

int srsgpu_ofdm_demodulator_symbols_plan_create(srsgpu_context*           ctx,
                                                const srsgpu_ofdm_config* cfg,
                                                uint32_t                  nof_ports,
                                                uint32_t                  slot_index,
                                                uint32_t                  first_symbol,
                                                uint32_t                  nof_symbols,
                                                srsgpu_ofdm_plan**        plan);

/** Sector groups — one launch for the same symbol (or slot) of several sectors sharing a GPU, where the reference runs
 *  one lower-PHY sector per cell, each with its own OFDM objects (lib/ru/generic/ru_factory_generic_impl.cpp:75-90,
 *  lib/phy/lower/lower_phy_factory.cpp:70/:84). Concatenates the jobs of `members` (the sectors' plans, each keeping
 *  its own carrier frequency, scaling and slot/symbol positions) into one plan: member i's grids follow member i-1's
 *  (srsgpu_ofdm_plan_nof_grid_words words each) and its time samples follow member i-1's; the plan's grid g runs over
 *  the members' grids in order (srsgpu_ofdm_plan_sample_offset). The members must share direction, DFT size, bandwidth,
 *  DFT window offset and number of ports (one kernel runs every job). The members stay owned by the caller. */
int srsgpu_ofdm_plan_concat(srsgpu_context*                ctx,
                            const srsgpu_ofdm_plan* const* members,
                            uint32_t                       nof_members,
                            srsgpu_ofdm_plan**             plan);

/** One (grid, port, symbol) transform of an OFDM launch: the grid row at grid_offset (uint32 words), the symbol's
 *  cyclic prefix at sample_offset (complex samples), its length, and the phase compensation times the scaling. */
typedef struct {
  uint32_t grid_offset;
  uint32_t sample_offset;
  uint32_t cp_len;
  uint32_t reserved;
  float    coef_re;
  float    coef_im;
} srsgpu_ofdm_job;

/** The plan's jobs (one per grid, port and symbol, offsets relative to the plan's own buffers), as its launch runs
 *  them: capacity entries at most, *nof_jobs = how many the plan has. */
int srsgpu_ofdm_plan_get_jobs(const srsgpu_ofdm_plan* plan, srsgpu_ofdm_job* jobs, uint32_t capacity,
                              uint32_t* nof_jobs);

/** Runs a caller-assembled job list — the jobs of several plans (sectors, slots, symbols) at offsets of the caller's
 *  choosing within d_in / d_out — with the launch parameters of `plan` (direction, DFT size, bandwidth, DFT window
 *  offset); the jobs' plans must share them. d_jobs, d_in and d_out are device-accessible (HBM, or mapped host memory
 *  the kernel reads / writes in place). Not for the split DFT sizes (9216 .. 98304 points: their scratch is per plan).
 *  Asynchronous on `stream`. */
int srsgpu_ofdm_jobs_execute(const srsgpu_ofdm_plan* plan,
                             const srsgpu_ofdm_job*  d_jobs,
                             uint32_t                nof_jobs,
                             const void*             d_in,
                             void*                   d_out,
                             void*                   stream);

/** An OFDM job with absolute device addresses: the grid row (12 * bw_rb uint32 bf16 pairs) and the first sample of
 *  the symbol's cyclic prefix, each anywhere device-accessible — HBM, or host memory mapped for the device — so the
 *  caller's own buffers (a resource grid's rows, a radio buffer) are read or written in place. grid_copy (demodulation
 *  only, 0: none): a second row the same subcarriers are written to — the HBM copy of a mapped uplink grid that the
 *  PUSCH slot batch on the same GPU reads instead of fetching the host grid back over PCIe. */
typedef struct {
  uint64_t grid;
  uint64_t samples;
  uint32_t cp_len;
  float    coef_re;
  float    coef_im;
  uint32_t reserved;
  uint64_t grid_copy;
} srsgpu_ofdm_direct_job;

/** srsgpu_ofdm_jobs_execute over direct-address jobs (same launch parameters, same restrictions): the lower PHY's
 *  sector group demodulates straight into the rows of an uplink grid that its owner has mapped, instead of into a
 *  staging entry copied into the grid afterwards (puxch_processor_impl.cpp:78, the grid write per symbol). */
int srsgpu_ofdm_jobs_execute_direct(const srsgpu_ofdm_plan*       plan,
                                    const srsgpu_ofdm_direct_job* d_jobs,
                                    uint32_t                      nof_jobs,
                                    void*                         stream);

/** uint32 words of the plan's grids (grids x ports x symbols x 12 * bw_rb). */
uint64_t srsgpu_ofdm_plan_nof_grid_words(const srsgpu_ofdm_plan* plan);

/** Total number of complex samples of the plan's time buffer (all grids and ports). */
uint64_t srsgpu_ofdm_plan_nof_samples(const srsgpu_ofdm_plan* plan);

/** First complex sample of (grid, port) in the time buffer. */
uint64_t srsgpu_ofdm_plan_sample_offset(const srsgpu_ofdm_plan* plan, uint32_t grid, uint32_t port);

/** Modulates d_grids into d_samples. Asynchronous on `stream`, hipGraph-capturable.
 *  Concurrency: plans of the split DFT sizes (9216..98304 points) own a mutable HBM scratch row per (grid, port,
 *  symbol) job, so one such plan must not execute on two streams at the same time (order the executes, or create one
 *  plan per stream). Plans of the other sizes hold read-only state only and may run concurrently. Same for the
 *  demodulator below. */
int srsgpu_ofdm_modulator_plan_execute(const srsgpu_ofdm_plan* plan,
                                       const uint32_t*         d_grids,
                                       float*                  d_samples,
                                       void*                   stream);

/** As srsgpu_ofdm_modulator_plan_execute, every RE taken from d_twin (same layout as d_grids, e.g. the PDSCH slot
 *  batch's HBM grid) unless it holds 0xffffffff, then from d_grids (the REs the host channels wrote): the modulation
 *  of a grid whose PDSCH REs never left the GPU (lower_phy_gpu's PDxCH, downlink_processor_single_executor_impl.cpp:268
 *  send_resource_grid -> pdxch_processor_impl handle_request). Not for the split DFT sizes. */
int srsgpu_ofdm_modulator_plan_execute_twin(const srsgpu_ofdm_plan* plan,
                                            const uint32_t*         d_grids,
                                            const uint32_t*         d_twin,
                                            float*                  d_samples,
                                            void*                   stream);

/** Demodulates d_samples into d_grids (every subcarrier of every symbol is written). Asynchronous. */
int srsgpu_ofdm_demodulator_plan_execute(const srsgpu_ofdm_plan* plan,
                                         const float*            d_samples,
                                         uint32_t*               d_grids,
                                         void*                   stream);

void srsgpu_ofdm_plan_destroy(srsgpu_ofdm_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * PUSCH demodulator — replaces srsran::pusch_demodulator::demodulate(pusch_codeword_buffer& codeword_buffer,
 * pusch_demodulator_notifier& notifier, const resource_grid_reader& grid, const channel_estimate& estimates,
 * const configuration& config) (include/srsran/phy/upper/channel_processors/pusch/pusch_demodulator.h:95,
 * lib/phy/upper/channel_processors/pusch/pusch_demodulator_impl.cpp:272) for every PUSCH transmission of a batch of
 * slots: per data RE, channel equalization (channel_equalizer_generic_impl.cpp: ZF 1 x N, ZF 2 x N; MMSE with one
 * layer == ZF), soft demapping (demodulation_mapper_impl.cpp, the SIMD arithmetic) and descrambling
 * (c_init = rnti * 2^15 + n_id), LLRs written to the codeword buffer in the reference's order (RE, layer, bit).
 * SRSGPU_EQ_MMSE with 2..4 layers and ZF with 3..4 layers are extensions the open-source reference does not implement
 * (its equalize_mmse_* / equalize_zf_3x4 / _4x4 assert): unbiased linear MMSE.
 * Inputs: rx grids as in the OFDM demodulator (grid_nof_ports x 14 x 12 * grid_nof_prb uint32 bf16 pairs per slot);
 * channel estimates per slot [layer 0..3][port][symbol][subcarrier] bf16 pairs (srsran::channel_estimate's path-major
 * layout, channel_estimation.h:310); noise variances d_noise_var[4 * tx + port] (channel_estimate::get_noise_variance).
 * ------------------------------------------------------------------------------------------------------------------ */
/* ------------------------------------------------------------------------------------------------------------------
 * PUSCH DM-RS channel estimator — replaces srsran::dmrs_pusch_estimator::estimate(channel_estimate& estimate,
 * const resource_grid_reader& grid, const configuration& config)
 * (include/srsran/phy/upper/signal_processors/dmrs_pusch_estimator.h, lib/phy/upper/signal_processors/
 * dmrs_pusch_estimator_impl.cpp:28, port_channel_estimator_average_impl.cpp:77) for every PUSCH transmission of a
 * batch of slots, pseudo-random DM-RS sequence, the "average" (default) and "interpolate" time-domain strategies
 * (port_channel_estimator_td_interpolation_strategy), the none / mean / filter (default) frequency-domain smoothing,
 * and the estimator's CFO estimation with optional compensation (compensate_cfo, du_low's default:
 * du_low_config.h:69; port_channel_estimator_average_impl.cpp:128, :322, :475). Outputs per transmission and rx port:
 * the channel estimate of every RE of the allocation in the layout the demodulator reads, the noise variance
 * (d_noise_var[4 * tx + port]) and, when d_metrics is not NULL, SRSGPU_CHEST_METRICS floats at
 * d_metrics[SRSGPU_CHEST_METRICS * (4 * tx + port)]: RSRP, EPRE, noise variance, SNR, time alignment (seconds,
 * channel_estimate::get_time_alignment, DFT estimator time_alignment_estimator_dft_impl.cpp:178), CFO (Hz, NaN with one
 * DM-RS symbol: channel_estimate::get_cfo_Hz), 0, 0. One layer is the reference's scope
 * (port_channel_estimator_average_impl.cpp:83 asserts it); 2..4 layers (ports 1000..1003) are an extension: the w_f
 * cover code is removed over adjacent pilot pairs. Frequency hopping: the reference's PUSCH estimator never sets
 * hopping_symbol_index / rb_mask2 (dmrs_pusch_estimator_impl.cpp:107-172; only the PUCCH estimators do), so the PUSCH
 * path has no hopping to replace.
 * ------------------------------------------------------------------------------------------------------------------ */
#define SRSGPU_CHEST_FD_NONE 0
#define SRSGPU_CHEST_FD_MEAN 1
#define SRSGPU_CHEST_FD_FILTER 2
#define SRSGPU_CHEST_TD_AVERAGE 0
#define SRSGPU_CHEST_TD_INTERPOLATE 1
#define SRSGPU_CHEST_METRICS 8

/* Channel-estimate layouts (estimate_layout of the estimator and demodulator configurations). PER_SYMBOL is the
 * reference's channel_estimate: every allocated symbol holds its estimate. COMPACT stores, with the "average" time
 * strategy (one estimate for all the symbols of the allocation), only the row of start_symbol, and the demodulator
 * reads that row for every symbol: identical LLRs with 1/nof_symbols of the estimate traffic. With CFO compensation
 * (compensate_cfo and >= 2 DM-RS symbols) the row holds the unrotated estimate and the first allocated element of the
 * next row the normalised CFO (float32 bits); the demodulator (cfo_compensated = 1) applies each symbol's rotation
 * in bf16 exactly as the estimator would have written it. The "interpolate" strategy needs PER_SYMBOL. */
#define SRSGPU_CE_PER_SYMBOL 0
#define SRSGPU_CE_COMPACT 1

typedef struct {
  uint16_t scrambling_id;    /* N_ID^{n_SCID}, 0..65535 */
  uint8_t  n_scid;           /* 0 or 1 */
  uint8_t  dmrs_type;        /* 1 or 2 */
  uint8_t  nof_tx_layers;    /* 1..4 */
  uint8_t  nof_rx_ports;     /* ports 0..n-1 of the grid */
  uint8_t  start_symbol;     /* first_symbol */
  uint8_t  nof_symbols;      /* start_symbol + nof_symbols <= 14 */
  uint16_t dmrs_symbol_mask; /* symbols_mask: DM-RS symbols, inside [start_symbol, start_symbol + nof_symbols) */
  uint16_t rb_start;         /* contiguous CRB allocation (rb_mask) */
  uint16_t nof_rb;
  uint16_t slot_index;       /* n_slot within the frame (DM-RS c_init) */
  uint8_t  fd_smoothing;     /* SRSGPU_CHEST_FD_* */
  uint8_t  estimate_layout;  /* SRSGPU_CE_PER_SYMBOL or SRSGPU_CE_COMPACT */
  uint8_t  td_strategy;      /* SRSGPU_CHEST_TD_AVERAGE or SRSGPU_CHEST_TD_INTERPOLATE */
  uint8_t  compensate_cfo;   /* 1: compensate the estimated CFO (needs >= 2 DM-RS symbols to act) */
  float    scaling;          /* beta_PUSCH^DMRS (DM-RS amplitude relative to data), > 0 */
  uint32_t grid_index;       /* slot of the rx grid and of the estimate buffer */
  uint8_t  numerology;       /* subcarrier spacing 15 kHz x 2^numerology (0..4), normal cyclic prefix */
  uint8_t  dmrs_sequence;    /* SRSGPU_DMRS_PSEUDO_RANDOM (scrambling_id, n_scid) or SRSGPU_DMRS_LOW_PAPR (transform
                                precoding: scrambling_id = n_RS_ID 0..1007, the group n_RS_ID mod 30 sequence on every
                                DM-RS symbol, dmrs_pusch_estimator_impl.cpp:77; one layer, type 1) */
  uint8_t  pad[2];
} srsgpu_pusch_chest_config;
#define SRSGPU_DMRS_PSEUDO_RANDOM 0
#define SRSGPU_DMRS_LOW_PAPR 1

typedef struct srsgpu_pusch_chest_plan srsgpu_pusch_chest_plan;

int srsgpu_pusch_chest_plan_create(srsgpu_context*                  ctx,
                                   const srsgpu_pusch_chest_config* cfgs,
                                   uint32_t                         nof_tx,
                                   uint32_t                         grid_nof_prb,
                                   uint32_t                         grid_nof_ports,
                                   srsgpu_pusch_chest_plan**        plan);

/** As srsgpu_pusch_chest_plan_create with an optional allocation extension per transmission (exts may be NULL):
 *  srsgpu_alloc_ext::crb_mask is configuration::rb_mask. The pilots of the allocated CRBs (the sequence skipping the
 *  unallocated ones, dmrs_helper.cpp:64) are smoothed and interpolated as one band, the time alignment takes the RE-mask
 *  path (port_channel_estimator_helpers.cpp:285), and PRB i of the band is written at the i-th allocated CRB. (The
 *  reference writes every PRB of a non-contiguous mask at the lowest CRB instead, port_channel_estimator_average_impl.cpp:
 *  297: DESIGN.md.) Reserved patterns and PRGs are rejected. */
int srsgpu_pusch_chest_plan_create_ex(srsgpu_context*                  ctx,
                                      const srsgpu_pusch_chest_config* cfgs,
                                      const srsgpu_alloc_ext*          exts,
                                      uint32_t                         nof_tx,
                                      uint32_t                         grid_nof_prb,
                                      uint32_t                         grid_nof_ports,
                                      srsgpu_pusch_chest_plan**        plan);

/** Estimates every planned transmission: reads d_grids, writes d_ch_estimates (slot layout [layer 0..3][port]
 *  [symbol][subcarrier], only the allocated REs), d_noise_var and optionally d_metrics (SRSGPU_CHEST_METRICS floats
 *  per transmission and port). Asynchronous on `stream`. */
int srsgpu_pusch_chest_plan_execute(const srsgpu_pusch_chest_plan* plan,
                                    const uint32_t*                d_grids,
                                    uint32_t*                      d_ch_estimates,
                                    float*                         d_noise_var,
                                    float*                         d_metrics,
                                    void*                          stream);

void srsgpu_pusch_chest_plan_destroy(srsgpu_pusch_chest_plan* plan);

#define SRSGPU_EQ_ZF 0
#define SRSGPU_EQ_MMSE 1

typedef struct {
  uint16_t rnti;                        /* n_RNTI */
  uint16_t n_id;                        /* n_ID, 0..1023 */
  uint8_t  modulation_order;            /* Qm: 2, 4, 6, 8 */
  uint8_t  nof_tx_layers;               /* 1..4 */
  uint8_t  nof_rx_ports;                /* 1..grid_nof_ports (ports 0..n-1) */
  uint8_t  start_symbol;
  uint8_t  nof_symbols;                 /* start_symbol + nof_symbols <= 14 */
  uint8_t  dmrs_type;                   /* 1 or 2 */
  uint8_t  nof_cdm_groups_without_data; /* 1..2 (type 1), 1..3 (type 2) */
  uint8_t  equalizer;                   /* SRSGPU_EQ_ZF or SRSGPU_EQ_MMSE */
  uint16_t dmrs_symbol_mask;            /* bit l = OFDM symbol l carries DM-RS */
  uint16_t rb_start;                    /* contiguous CRB allocation [rb_start, rb_start + nof_rb) (rb_mask) */
  uint16_t nof_rb;
  uint8_t  estimate_layout;             /* SRSGPU_CE_PER_SYMBOL or SRSGPU_CE_COMPACT (as the estimator wrote it) */
  uint8_t  cfo_compensated;             /* COMPACT only: the estimator compensated the CFO (its compensate_cfo) */
  uint32_t grid_index;                  /* slot (rx grid and channel estimate) of the transmission */
  uint32_t llr_offset;                  /* first codeword LLR in the output buffer */
  uint8_t  numerology;                  /* COMPACT + cfo_compensated: subcarrier spacing of the symbol epochs */
  uint8_t  transform_precoding;         /* 1: transform precoding (DFT-s-OFDM; one layer, every data symbol's REs a
                                           multiple of 12 with 2^a 3^b 5^c PRBs, TS 38.211 section 6.3.1.4):
                                           configuration::enable_transform_precoding, pusch_demodulator_impl.cpp:346 */
  uint8_t  pad2[2];
} srsgpu_pusch_demod_config;

typedef struct srsgpu_pusch_demodulator_plan srsgpu_pusch_demodulator_plan;

/** Validates the transmissions (supported layer / port / modulation combinations, allocation inside the grid) and
 *  uploads the work. */
int srsgpu_pusch_demodulator_plan_create(srsgpu_context*                  ctx,
                                         const srsgpu_pusch_demod_config* cfgs,
                                         uint32_t                         nof_tx,
                                         uint32_t                         grid_nof_prb,
                                         uint32_t                         grid_nof_ports,
                                         srsgpu_pusch_demodulator_plan**  plan);

/** Number of codeword LLRs of transmission `tx` (data REs x layers x Qm). */
uint32_t srsgpu_pusch_demodulator_plan_nof_llrs(const srsgpu_pusch_demodulator_plan* plan, uint32_t tx);

/** 1 when the plan finds the OFDM symbol of transmission `tx`'s REs by the closed form (every symbol with data carries
 *  the same number of REs, no DM-RS symbol carries data, at most two interior runs of symbols without data), 0 when it
 *  searches the symbols' cumulative RE counts (every other layout, SRSGPU_OPTION_DEMOD_GENERAL_PATHS, or no such tx). */
int srsgpu_pusch_demodulator_plan_symbol_closed_form(const srsgpu_pusch_demodulator_plan* plan, uint32_t tx);

/** Demodulates every planned transmission into d_llrs. Asynchronous on `stream`, hipGraph-capturable. */
int srsgpu_pusch_demodulator_plan_execute(const srsgpu_pusch_demodulator_plan* plan,
                                          const uint32_t*                      d_grids,
                                          const uint32_t*                      d_ch_estimates,
                                          const float*                         d_noise_var,
                                          int8_t*                              d_llrs,
                                          void*                                stream);

void srsgpu_pusch_demodulator_plan_destroy(srsgpu_pusch_demodulator_plan* plan);

/** As srsgpu_pusch_demodulator_plan_create with an optional allocation extension per transmission (exts may be NULL):
 *  srsgpu_alloc_ext::crb_mask is configuration::rb_mask (any CRB pattern; data REs in symbol-major, ascending-subcarrier
 *  order, pusch_demodulator_impl.cpp:290); reserved patterns and PRGs are rejected (the demodulator has neither). */
int srsgpu_pusch_demodulator_plan_create_ex(srsgpu_context*                  ctx,
                                            const srsgpu_pusch_demod_config* cfgs,
                                            const srsgpu_alloc_ext*          exts,
                                            uint32_t                         nof_tx,
                                            uint32_t                         grid_nof_prb,
                                            uint32_t                         grid_nof_ports,
                                            srsgpu_pusch_demodulator_plan**  plan);

/** Copies the descrambling sequence of transmission tx (TS 38.211 section 5.2.1, c_init = rnti 2^15 + n_id: the
 *  sequence pusch_demodulator_impl.cpp:277 generates and passes to pusch_codeword_buffer::on_new_block) into d_words:
 *  ceil(nof_llrs / 32) 32-bit words, bit 31 of word w = c(32 w) (the plan keeps it resident). Asynchronous. */
int srsgpu_pusch_demodulator_plan_scrambling(const srsgpu_pusch_demodulator_plan* plan,
                                             uint32_t                             tx,
                                             uint32_t*                            d_words,
                                             void*                                stream);

/* Post-equalization statistics (pusch_demodulator_notifier::demodulation_stats, pusch_demodulator_impl.cpp:355-443):
 * SRSGPU_DEMOD_STATS floats per transmission, rows 0..13 = OFDM symbol l (on_provisional_stats) and row 14 = the whole
 * transmission (on_end_stats), each (SINR dB, EVM): SINR = -10 log10(mean of the finite equalizer noise variances,
 * after transform deprecoding) or +inf, EVM = sqrt(mean |modulate(hard decisions) - equalized symbol|^2) per symbol
 * (evm_calculator_generic_impl.cpp), the total EVM weighting each symbol's by its size. NaN rows: no data REs. */
#define SRSGPU_DEMOD_STATS 30

/** As srsgpu_pusch_demodulator_plan_execute, and when d_stats is not NULL also writes the statistics of every
 *  transmission (d_stats[SRSGPU_DEMOD_STATS * tx + 2 * row + {0: SINR dB, 1: EVM}]). Asynchronous, hipGraph-capturable
 *  (the plan's accumulators are reset by the same execute). */
int srsgpu_pusch_demodulator_plan_execute_ex(const srsgpu_pusch_demodulator_plan* plan,
                                             const uint32_t*                      d_grids,
                                             const uint32_t*                      d_ch_estimates,
                                             const float*                         d_noise_var,
                                             int8_t*                              d_llrs,
                                             float*                               d_stats,
                                             void*                                stream);

/* ------------------------------------------------------------------------------------------------------------------
 * UL-SCH demultiplexer (UCI on PUSCH, TS 38.212 section 6.2.7) — replaces srsran::ulsch_demultiplex::demultiplex /
 * set_csi_part2 (include/srsran/phy/upper/channel_processors/pusch/ulsch_demultiplex.h:64,
 * lib/phy/upper/channel_processors/pusch/ulsch_demultiplex_impl.cpp:199) for every transmission of a batch: routes the
 * demodulated, descrambled codeword LLRs (the PUSCH demodulator's output, RE by RE) to the UL-SCH data stream (the PUSCH
 * decoder's input; REs carrying HARQ-ACK of <= 2 bits stay in it as zeros), HARQ-ACK, CSI Part 1 and CSI Part 2 LLR
 * streams, with the reference's 1- / 2-bit UCI placeholder handling (the scrambling sequence c_init = rnti 2^15 + n_id
 * re-applied to the "y" and "x" placeholder bits, :91 / :131). The RE sets per OFDM symbol (reserved HARQ-ACK REs,
 * HARQ-ACK, CSI Part 1, CSI Part 2, :316) are fixed at plan creation; CSI Part 2 is placed from csi2_first_symbol on
 * (0: as if set_csi_part2 were called before the first symbol). Input and output offsets are in LLRs.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint8_t  modulation_order;            /* Qm: 2, 4, 6, 8 */
  uint8_t  nof_layers;                  /* 1..4 */
  uint16_t nof_prb;                     /* allocated PRBs (count) */
  uint8_t  start_symbol;                /* start_symbol_index */
  uint8_t  nof_symbols;
  uint16_t dmrs_symbol_mask;            /* DM-RS symbols */
  uint8_t  dmrs_type;                   /* 1 or 2 */
  uint8_t  nof_cdm_groups_without_data; /* 1..2 (type 1), 1..3 (type 2) */
  uint16_t rnti;                        /* scrambling c_init = rnti 2^15 + n_id (placeholders) */
  uint16_t n_id;
  uint16_t csi2_first_symbol;           /* CSI Part 2 REs only in OFDM symbols >= this one: the symbol whose
                                           demultiplexing completes CSI Part 1, where the reference's processor calls
                                           set_csi_part2 (pusch_processor_impl.cpp:72-100, ulsch_demultiplex_impl.cpp:241)
                                           0: from the first symbol, as if set before it */
  uint32_t nof_harq_ack_rvd;            /* G^HARQ-ACK_rvd */
  uint32_t nof_harq_ack_bits;           /* O^HARQ-ACK */
  uint32_t nof_enc_harq_ack_bits;       /* G^HARQ-ACK */
  uint32_t nof_csi_part1_bits;          /* O^CSI-1 */
  uint32_t nof_enc_csi_part1_bits;      /* G^CSI-1 */
  uint32_t nof_csi_part2_bits;          /* O^CSI-2 */
  uint32_t nof_enc_csi_part2_bits;      /* G^CSI-2 (0: none) */
  uint32_t llr_offset;                  /* first codeword LLR in the input */
  uint32_t sch_offset;                  /* first UL-SCH LLR in d_sch */
  uint32_t harq_offset;                 /* first HARQ-ACK LLR in d_harq */
  uint32_t csi1_offset;                 /* first CSI Part 1 LLR in d_csi1 */
  uint32_t csi2_offset;                 /* first CSI Part 2 LLR in d_csi2 */
} srsgpu_ulsch_demux_config;

typedef struct srsgpu_ulsch_demux_plan srsgpu_ulsch_demux_plan;

/** Validates the transmissions (every UCI field must fit the allocation, as the reference asserts at the end of the
 *  codeword) and uploads the RE routing. */
int srsgpu_ulsch_demux_plan_create(srsgpu_context*                  ctx,
                                   const srsgpu_ulsch_demux_config* cfgs,
                                   uint32_t                         nof_tx,
                                   srsgpu_ulsch_demux_plan**        plan);

/** LLRs of transmission tx: stream 0 = codeword (input), 1 = UL-SCH, 2 = HARQ-ACK, 3 = CSI Part 1, 4 = CSI Part 2. */
uint32_t srsgpu_ulsch_demux_plan_nof_llrs(const srsgpu_ulsch_demux_plan* plan, uint32_t tx, uint32_t stream);

/** LLRs of `stream` (as above) that transmission tx's OFDM symbol l (0..13, slot numbering) carries: counts[l]. The
 *  reference's demultiplexer hands a UCI field's LLRs to its decoder buffer while it demultiplexes the symbol that holds
 *  them and ends the field in the symbol that completes it (ulsch_demultiplex_impl.cpp:474-576); a host that replays
 *  the GPU's streams into the reference's UCI decoders feeds them symbol by symbol with these counts. */
int srsgpu_ulsch_demux_plan_symbol_llrs(const srsgpu_ulsch_demux_plan* plan, uint32_t tx, uint32_t stream,
                                        uint32_t counts[14]);

/** Demultiplexes every planned transmission. Asynchronous on `stream`, hipGraph-capturable. Output pointers of streams
 *  no transmission uses may be NULL. */
int srsgpu_ulsch_demux_plan_execute(const srsgpu_ulsch_demux_plan* plan,
                                    const int8_t*                  d_llrs,
                                    int8_t*                        d_sch,
                                    int8_t*                        d_harq,
                                    int8_t*                        d_csi1,
                                    int8_t*                        d_csi2,
                                    void*                          stream);

void srsgpu_ulsch_demux_plan_destroy(srsgpu_ulsch_demux_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * UCI decoder, short blocks — replaces srsran::uci_decoder::decode(span<const log_likelihood_ratio> llr,
 * const configuration& config) (include/srsran/phy/upper/channel_processors/uci/uci_decoder.h) for messages of 1..11
 * bits, which uci_decoder_impl::decode hands to the short-block detector
 * (lib/phy/upper/channel_processors/uci/uci_decoder_impl.cpp:119), for every field of a batch in one launch. Restates
 * short_block_detector_impl::detect (lib/phy/upper/channel_coding/short/short_block_detector_impl.cpp:186) bit for
 * bit: the validation on the count of non-zero LLRs (:60), the rate dematching with a saturating sum per block (:160,
 * as the AVX2 build sums LLRs, log_likelihood_ratio.cpp:432), the 1-bit sign decision, the 2-bit search (:89) and the
 * 3..11-bit maximum-likelihood search with the GLRT validity threshold (:129, :221). Input LLRs lie in [-120, 120], as
 * the PUSCH demodulator writes them. Fields of 12 bits and more (polar code) are rejected: they stay with the host.
 * A field reads its LLRs from one of three input streams, so that a plan decodes the UL-SCH demultiplexer's HARQ-ACK,
 * CSI Part 1 and CSI Part 2 streams where they lie (source 0, 1, 2 with llr_offset = that plan's harq_offset,
 * csi1_offset, csi2_offset).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint8_t  nof_bits;         /* A: message bits, 1..11 */
  uint8_t  modulation_order; /* Qm: 1, 2, 4, 6, 8 (the block before rate matching: Qm, 3 Qm or 32 bits) */
  uint8_t  source;           /* input stream of the field: 0, 1 or 2 (d_src0 / d_src1 / d_src2) */
  uint8_t  reserved;
  uint32_t nof_enc_bits;     /* E: encoded LLRs of the field (0: the field comes out invalid) */
  uint32_t llr_offset;       /* first LLR of the field in its input stream */
} srsgpu_uci_field_config;

typedef struct srsgpu_uci_decoder_plan srsgpu_uci_decoder_plan;

/** Validates the fields and uploads their descriptors. SRSGPU_ERR_INVALID_ARG for nof_bits = 0, nof_bits > 11 (polar
 *  coded UCI is not implemented), a modulation_order outside {1, 2, 4, 6, 8}, source > 2 or nof_enc_bits > 2^24 (far
 *  above any PUSCH's capacity). Blocking. */
int srsgpu_uci_decoder_plan_create(srsgpu_context*                ctx,
                                   const srsgpu_uci_field_config* cfgs,
                                   uint32_t                       nof_fields,
                                   srsgpu_uci_decoder_plan**      plan);

/** Decodes every planned field: d_msgs[f] bit j = message bit j of field f (bits nof_bits and above 0; every message
 *  bit 1 for a field that fails the validation, as the reference fills it), d_status[f] = 1 valid / 0 invalid (the
 *  detector's return value). Input streams no field reads may be NULL. Asynchronous on `stream`, no allocation,
 *  hipGraph-capturable. */
int srsgpu_uci_decoder_plan_execute(const srsgpu_uci_decoder_plan* plan,
                                    const int8_t*                  d_src0,
                                    const int8_t*                  d_src1,
                                    const int8_t*                  d_src2,
                                    uint16_t*                      d_msgs,
                                    uint8_t*                       d_status,
                                    void*                          stream);

void srsgpu_uci_decoder_plan_destroy(srsgpu_uci_decoder_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * UCI decoder, polar-coded fields — replaces srsran::uci_decoder::decode for messages of 12..1706 bits, which
 * uci_decoder_impl::decode hands to decode_codeword_polar
 * (lib/phy/upper/channel_processors/uci/uci_decoder_impl.cpp:119, :43), for every field of a batch in one launch, one
 * wavefront per codeblock. Restates the chain bit for bit: segmentation into one or two codeblocks and the 6- / 11-bit
 * CRC (include/srsran/ran/uci/uci_info.h:40, :54; uci_decoder_impl.cpp:58-69), the uplink polar code of (K, E) with
 * nMax = 10 (lib/phy/upper/channel_coding/polar/polar_code_impl.cpp:325, :421), the rate dematching with the promotion
 * sum in the reference's order (polar_rate_dematcher_impl.cpp:100, lib/phy/upper/log_likelihood_ratio.cpp:75), the
 * simplified successive-cancellation decoder (polar_decoder_impl.cpp:335), the de-allocation
 * (polar_deallocator_impl.cpp:27) and the CRC over all K bits of a codeblock (uci_decoder_impl.cpp:107). Input LLRs lie
 * in [-120, 120] or are +-127, as log_likelihood_ratio holds them. Together with srsgpu_uci_decoder_plan (1..11 bits)
 * this covers uci_decoder::decode.
 *
 * One rule differs: both codeblocks of a two-codeblock field are always decoded and their bits written. The reference
 * decodes codeblock 1 only when codeblock 0 passes its CRC (uci_decoder_impl.cpp:65) and otherwise leaves the caller's
 * bits untouched, so no value of those bits is the reference's; the status is invalid either way.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint16_t nof_bits;         /* A: message bits, 12..1706 */
  uint8_t  source;           /* input stream of the field: 0, 1 or 2 (d_src0 / d_src1 / d_src2) */
  uint8_t  reserved;
  uint32_t nof_enc_bits;     /* E: encoded LLRs of the field; two codeblocks read floor(E / 2) each */
  uint32_t llr_offset;       /* first LLR of the field in its input stream */
  uint32_t msg_word_offset;  /* first of the field's ceil(A / 32) words in d_msgs */
} srsgpu_uci_polar_field_config;

typedef struct srsgpu_uci_polar_decoder_plan srsgpu_uci_polar_decoder_plan;

/** Validates the fields, builds the tables of every distinct code once and uploads them. SRSGPU_ERR_INVALID_ARG, with a
 *  message naming the field and the reason, for what the reference's assertions refuse: nof_bits outside 12..1706
 *  (uci_decoder_impl.cpp:124, uci_decoder_impl.h:74), source > 2, more than 8192 encoded bits per codeblock
 *  (polar_code_impl.cpp:334), K + nPC >= E per codeblock (:363), K >= N or K outside 18..25 / 31..1023 (:407, :345;
 *  neither can follow from a nof_bits in range), and fields whose message words overlap. Blocking. */
int srsgpu_uci_polar_decoder_plan_create(srsgpu_context*                      ctx,
                                         const srsgpu_uci_polar_field_config* cfgs,
                                         uint32_t                             nof_fields,
                                         srsgpu_uci_polar_decoder_plan**      plan);

/** Decodes every planned field: message bit j of field f is bit j mod 32 of d_msgs[msg_word_offset + j / 32] (the
 *  field's last word is written whole, zeros above bit A - 1; words of no field are not written), d_status[f] = 1 when
 *  the CRC of every codeblock passes (uci_status::valid), else 0. Input streams no field reads may be NULL.
 *  Asynchronous on `stream`, no allocation, hipGraph-capturable. */
int srsgpu_uci_polar_decoder_plan_execute(const srsgpu_uci_polar_decoder_plan* plan,
                                          const int8_t*                        d_src0,
                                          const int8_t*                        d_src1,
                                          const int8_t*                        d_src2,
                                          uint32_t*                            d_msgs,
                                          uint8_t*                             d_status,
                                          void*                                stream);

void srsgpu_uci_polar_decoder_plan_destroy(srsgpu_uci_polar_decoder_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * PUSCH decoder (transport-block level) — replaces srsran::pusch_decoder (include/srsran/phy/upper/channel_processors/
 * pusch/pusch_decoder.h; lib/phy/upper/channel_processors/pusch/pusch_decoder_impl.cpp: new_data :98, segmentation
 * :190, codeblock tasks :283, join_and_notify :386): segmentation, per-codeblock rate dematching + HARQ combining +
 * LDPC decoding + CB CRC, codeblock concatenation and TB CRC24A check, for every transport block of a slot.
 * The HARQ context lives in device memory owned by the caller: d_harq (C * N_short * Z LLRs per TB), d_cb_crc_ok (one
 * flag per codeblock) and d_cb_msgs (SRSGPU_CB_MSG_STRIDE bytes of decoded message per codeblock).
 * ------------------------------------------------------------------------------------------------------------------ */
#define SRSGPU_CB_MSG_STRIDE 1056u /* bytes per codeblock message slot (22 * 384 bits) */

typedef struct {
  uint8_t  base_graph;       /* 1 or 2 */
  uint8_t  rv;               /* 0..3 */
  uint8_t  modulation_order; /* Qm */
  uint8_t  nof_layers;       /* 1..4 */
  uint8_t  new_data;         /* 1: new transmission (resets the TB's CB CRC flags) */
  uint8_t  use_early_stop;   /* LDPC early stop with the codeblock CRC */
  uint8_t  max_iterations;   /* nof_ldpc_iterations (> 0) */
  uint8_t  reserved;
  float    scaling_factor;   /* normalised min-sum factor in (0, 1) */
  uint32_t tbs_bytes;        /* transport block size in bytes */
  uint32_t nof_ch_symbols;   /* G / Qm */
  uint32_t Nref;             /* limited-buffer rate matching N_ref, 0 = none */
  uint32_t llr_offset;       /* first of the G codeword LLRs */
  uint32_t harq_offset;      /* first LLR of the TB's HARQ soft buffer */
  uint32_t cb_offset;        /* index of the TB's first codeblock (CRC flags, messages, iteration counts) */
  uint32_t tb_offset;        /* byte offset of the decoded transport block */
} srsgpu_pusch_tb_config;

typedef struct srsgpu_pusch_decoder_plan srsgpu_pusch_decoder_plan;

int srsgpu_pusch_decoder_plan_create(srsgpu_context*               ctx,
                                     int                           impl,
                                     const srsgpu_pusch_tb_config* cfgs,
                                     uint32_t                      nof_tbs,
                                     srsgpu_pusch_decoder_plan**   plan);

uint32_t srsgpu_pusch_decoder_plan_nof_codeblocks(const srsgpu_pusch_decoder_plan* plan);

/** Number of LLR bytes the LDPC decoder stage moves per execute: every codeblock's span of the HARQ buffer, trimmed to
 *  the rate dematcher's zero tail for new transmissions (what decode() would trim to, ldpc_decoder_impl.cpp:94); for
 *  a codeblock whose rate dematching the decoder performs itself (first transmissions that are a plain copy), the E
 *  codeword LLRs it reads plus the N HARQ bytes it writes. For traffic accounting. */
uint64_t srsgpu_pusch_decoder_plan_decoder_input_llrs(const srsgpu_pusch_decoder_plan* plan);

/** Decodes the planned transport blocks. d_tb_crc_ok[t] = 1 when the TB CRC passed (pusch_decoder_result
 *  tb_crc_ok); d_cb_nof_iterations[c] as in srsgpu_pusch_cb_plan_execute. Asynchronous, hipGraph-capturable.
 *  A plan of at most 8 large segmented TBs runs its TB stage over slices whose CRC sums live in the plan (reset by
 *  every execute): executes (and assembles) of one plan must be ordered, e.g. on one stream, never concurrent. */
int srsgpu_pusch_decoder_plan_execute(const srsgpu_pusch_decoder_plan* plan,
                                      const int8_t*                    d_llrs,
                                      int8_t*                          d_harq,
                                      uint8_t*                         d_cb_crc_ok,
                                      uint8_t*                         d_cb_msgs,
                                      int32_t*                         d_cb_nof_iterations,
                                      uint8_t*                         d_tbs,
                                      uint8_t*                         d_tb_crc_ok,
                                      void*                            stream);

/** As srsgpu_pusch_decoder_plan_execute, with codeblock c's HARQ soft buffer (N bytes, the rate dematcher's output and
 *  the decoder's input) at d_harq_cbs[c], c = srsgpu_pusch_tb_config::cb_offset + the codeblock's index in its TB (the
 *  index of its CRC flag and message) - a device array covering every such index of the plan, e.g. the slots of
 *  a persistent rx-buffer arena (the reference's rx_buffer.h:72 get_codeblock_soft_bits for the codeblock's absolute
 *  identifier, :65) - instead of at d_harq + srsgpu_pusch_tb_config::harq_offset. The soft bits stay in the arena: no
 *  copy into a batch buffer before the decode and back after it (srsgpu_harq_copy_arenas). Asynchronous,
 *  hipGraph-capturable (the pointer array may change between replays). */
int srsgpu_pusch_decoder_plan_execute_arena(const srsgpu_pusch_decoder_plan* plan,
                                            const int8_t*                    d_llrs,
                                            int8_t* const*                   d_harq_cbs,
                                            uint8_t*                         d_cb_crc_ok,
                                            uint8_t*                         d_cb_msgs,
                                            int32_t*                         d_cb_nof_iterations,
                                            uint8_t*                         d_tbs,
                                            uint8_t*                         d_tb_crc_ok,
                                            void*                            stream);

/** The transport-block stage alone (pusch_decoder_impl.cpp:386 join_and_notify, :438 concatenate_codeblocks): TB
 *  assembly from the codeblock messages and flags already in d_cb_msgs / d_cb_crc_ok (the plan's codeblock layout,
 *  SRSGPU_CB_MSG_STRIDE bytes per codeblock) and the TB CRC24A check; a TB CRC mismatch clears the TB's codeblock
 *  flags, as execute does. For codeblocks decoded elsewhere: codeblock-sharded decoding, where every rank runs the
 *  srsgpu_pusch_cb_plan of its codeblock range and the FAPI rank gathers the messages and flags (srsgpu/dist.py
 *  CodeblockShard). Asynchronous, hipGraph-capturable. */
int srsgpu_pusch_decoder_plan_assemble(const srsgpu_pusch_decoder_plan* plan,
                                       uint8_t*                         d_cb_crc_ok,
                                       const uint8_t*                   d_cb_msgs,
                                       uint8_t*                         d_tbs,
                                       uint8_t*                         d_tb_crc_ok,
                                       void*                            stream);

void srsgpu_pusch_decoder_plan_destroy(srsgpu_pusch_decoder_plan* plan);

/** HARQ soft buffers kept across slots in a persistent arena, one slot of arena_stride bytes per absolute codeblock
 *  identifier (the reference's rx buffer pool: rx_buffer.h:65 get_absolute_codeblock_id, :72 get_codeblock_soft_bits),
 *  moved to / from a slot batch's contiguous HARQ buffer (srsgpu_pusch_tb_config::harq_offset layout) around a
 *  srsgpu_pusch_decoder_plan_execute. d_jobs: device array of nof_jobs entries. Asynchronous on `stream`. */
#define SRSGPU_HARQ_TO_BATCH 0
#define SRSGPU_HARQ_TO_ARENA 1
typedef struct {
  uint32_t slot;         /* arena slot (absolute codeblock identifier) */
  uint32_t batch_offset; /* first byte of the codeblock's soft bits in the batch HARQ buffer */
  uint32_t bytes;        /* soft bits to move (N of the codeblock) */
  uint32_t arena;        /* srsgpu_harq_copy_arenas: index into the arena table (0 for srsgpu_harq_copy) */
} srsgpu_harq_copy_job;

int srsgpu_harq_copy(srsgpu_context*             ctx,
                     int                         direction,
                     int8_t*                     d_arena,
                     uint32_t                    arena_stride,
                     int8_t*                     d_batch,
                     const srsgpu_harq_copy_job* d_jobs,
                     uint32_t                    nof_jobs,
                     void*                       stream);

/** As srsgpu_harq_copy over several arenas in one launch (the rx buffer pools of several sectors, whose slots one
 *  GPU service batch gathers): job j moves between arena d_arenas[j.arena] (a device array of arena base pointers)
 *  and the batch buffer. */
int srsgpu_harq_copy_arenas(srsgpu_context*             ctx,
                            int                         direction,
                            int8_t* const*              d_arenas,
                            uint32_t                    arena_stride,
                            int8_t*                     d_batch,
                            const srsgpu_harq_copy_job* d_jobs,
                            uint32_t                    nof_jobs,
                            void*                       stream);

/** A list of copies as one launch: span i copies bytes bytes (a multiple of 16, 16-byte aligned addresses) from src to
 *  dst; src / dst device-accessible (HBM, or mapped host memory the kernel reads or writes in place). d_spans itself is
 *  device-accessible; max_bytes = the largest span. Replaces the per-slot rx-grid upload of a slot batch (one
 *  hipMemcpyAsync per slot: the DMA engines manage ~29 GB/s for 0.5–1 MB copies where a kernel reading mapped memory
 *  reaches 37–50 GB/s, profiles/r5_pcie_probe.txt). Asynchronous on `stream`. */
typedef struct {
  const void* src;
  void*       dst;
  uint64_t    bytes;
} srsgpu_copy_span;

int srsgpu_copy_spans(const srsgpu_copy_span* d_spans, uint32_t nof_spans, uint64_t max_bytes, void* stream);

/** As srsgpu_copy_spans, but each 32-bit word of a source replaces the destination's only when it is not `sentinel`:
 *  the gather of a multi-device PDSCH slot batch, whose shards map their UEs' REs into sentinel-filled grids and merge
 *  their bands into the root device's grid (peer reads over xGMI) before its one download
 *  (downlink_processor_single_executor_impl.cpp:268-274 sends one grid per slot). */
int srsgpu_merge_spans(const srsgpu_copy_span* d_spans,
                       uint32_t                nof_spans,
                       uint64_t                max_bytes,
                       uint32_t                sentinel,
                       void*                   stream);

/** As srsgpu_pusch_chest_plan_execute, with the span copies d_spans[0, nof_spans) (each as in srsgpu_copy_spans,
 *  max_bytes the largest) done in the same launch by extra workgroups while the estimator's run: for a slot batch whose rx
 *  grids are read from mapped host memory, the data-symbol rows, which the estimator does not read, arrive while it
 *  works on the DM-RS rows copied before (pusch_processor_impl.cpp:165-213 estimates from the DM-RS symbols only). */
int srsgpu_pusch_chest_plan_execute_copy(const srsgpu_pusch_chest_plan* plan,
                                         const uint32_t*                d_grids,
                                         uint32_t*                      d_ch_estimates,
                                         float*                         d_noise_var,
                                         float*                         d_metrics,
                                         const srsgpu_copy_span*        d_spans,
                                         uint32_t                       nof_spans,
                                         uint64_t                       max_bytes,
                                         void*                          stream);

/** Stage timing: with enable = 1 every execute records HIP events on its stream around the three kernel stages
 *  (0: rate dematching, 1: LDPC decoding, 2: TB assembly + CRC); with enable = 2 only around the decoding stage (two
 *  events: the least perturbation of a timed run); 0 disables. stage_times synchronises on them and returns the
 *  accumulated milliseconds per stage (ms[3], stages not timed read 0) and the number of executes since the previous
 *  call. */
int srsgpu_pusch_decoder_plan_enable_timing(srsgpu_pusch_decoder_plan* plan, int enable);
int srsgpu_pusch_decoder_plan_stage_times(srsgpu_pusch_decoder_plan* plan, float* ms, uint32_t* nof_executes);

/** Number of device allocations that the contexts and plans of this process hold at the moment of the call. A plan's
 *  create followed by its destroy leaves it unchanged, and so does a create that fails (lifetime tests). */
int64_t srsgpu_debug_live_device_buffers(void);

#ifdef __cplusplus
}
#endif

#endif /* SRSGPU_PHY_H */
