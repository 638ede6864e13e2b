"""PUSCH: the DM-RS channel estimator (srsgpu_pusch_chest_plan), the demodulator (srsgpu_pusch_demodulator_plan), the
UL-SCH demultiplexer (srsgpu_ulsch_demux_plan) and the transport-block decoder (srsgpu_pusch_decoder_plan)."""
import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from ._abi import (Context, make_crb_mask_exts, span_list, SrsGpuError, torch, _check, _cptr, _dptr, _Handle, _lib,
                   _stage_times, _stream_handle)
from .ldpc import IMPL_BY_NAME


class PuschChestConfig(ctypes.Structure):
    """srsgpu_pusch_chest_config (include/srsgpu_phy.h): dmrs_pusch_estimator::configuration of one transmission."""
    _fields_ = [
        ("scrambling_id", ctypes.c_uint16),
        ("n_scid", ctypes.c_uint8),
        ("dmrs_type", ctypes.c_uint8),
        ("nof_tx_layers", ctypes.c_uint8),
        ("nof_rx_ports", ctypes.c_uint8),
        ("start_symbol", ctypes.c_uint8),
        ("nof_symbols", ctypes.c_uint8),
        ("dmrs_symbol_mask", ctypes.c_uint16),
        ("rb_start", ctypes.c_uint16),
        ("nof_rb", ctypes.c_uint16),
        ("slot_index", ctypes.c_uint16),
        ("fd_smoothing", ctypes.c_uint8),
        ("estimate_layout", ctypes.c_uint8),
        ("td_strategy", ctypes.c_uint8),
        ("compensate_cfo", ctypes.c_uint8),
        ("scaling", ctypes.c_float),
        ("grid_index", ctypes.c_uint32),
        ("numerology", ctypes.c_uint8),
        ("dmrs_sequence", ctypes.c_uint8),
        ("pad", ctypes.c_uint8 * 2),
    ]


assert ctypes.sizeof(PuschChestConfig) == 32
CHEST_FD_NONE, CHEST_FD_MEAN, CHEST_FD_FILTER = 0, 1, 2
CHEST_TD_AVERAGE, CHEST_TD_INTERPOLATE = 0, 1
CHEST_METRICS = 8  # per (tx, port): RSRP, EPRE, noise variance, SNR, TA (s), CFO (Hz, NaN without), 0, 0
CE_PER_SYMBOL, CE_COMPACT = 0, 1  # channel-estimate layouts (SRSGPU_CE_*)
EQ_ZF, EQ_MMSE = 0, 1


@dataclass
class PuschChannelEstimation:
    """dmrs_pusch_estimator::configuration (dmrs_pusch_estimator.h:63): pseudo-random DM-RS, contiguous CRB
    allocation (or `crb_mask`: rb_mask, one byte per grid CRB), rx ports 0..nof_rx_ports-1."""
    scrambling_id: int
    n_scid: int
    dmrs_type: int
    nof_tx_layers: int
    nof_rx_ports: int
    start_symbol: int
    nof_symbols: int
    dmrs_symbol_mask: int
    rb_start: int
    nof_rb: int
    slot_index: int
    scaling: float = 1.0
    fd_smoothing: int = CHEST_FD_FILTER
    estimate_layout: int = CE_PER_SYMBOL
    td_strategy: int = CHEST_TD_AVERAGE
    compensate_cfo: int = 0
    numerology: int = 1
    crb_mask: Optional[np.ndarray] = None
    dmrs_sequence: int = 0  # DMRS_PSEUDO_RANDOM, or DMRS_LOW_PAPR (transform precoding: scrambling_id = n_RS_ID)


DMRS_PSEUDO_RANDOM, DMRS_LOW_PAPR = 0, 1


def make_pusch_chest_configs(ests: Sequence[PuschChannelEstimation], grid_index: Sequence[int]):
    arr = (PuschChestConfig * len(ests))()
    for i, (e, g) in enumerate(zip(ests, grid_index)):
        a = arr[i]
        a.scrambling_id, a.n_scid, a.dmrs_type, a.nof_tx_layers = e.scrambling_id, e.n_scid, e.dmrs_type, e.nof_tx_layers
        a.nof_rx_ports, a.start_symbol, a.nof_symbols = e.nof_rx_ports, e.start_symbol, e.nof_symbols
        a.dmrs_symbol_mask, a.rb_start, a.nof_rb, a.slot_index = e.dmrs_symbol_mask, e.rb_start, e.nof_rb, e.slot_index
        a.estimate_layout, a.td_strategy, a.compensate_cfo = e.estimate_layout, e.td_strategy, e.compensate_cfo
        a.numerology = e.numerology
        a.fd_smoothing, a.scaling, a.grid_index = e.fd_smoothing, e.scaling, g
        a.dmrs_sequence = e.dmrs_sequence
    return arr


class PuschChannelEstimatorPlan(_Handle):
    """srsgpu_pusch_chest_plan: DM-RS channel estimation of a batch of PUSCH transmissions from rx grids
    (S, Pg, 14, nsc) into estimates (S, 4, Pg, 14, nsc) (uint32 bf16 pairs), noise variances (ntx, 4) and optional
    metrics (ntx, 4, CHEST_METRICS: RSRP, EPRE, noise variance, SNR, TA seconds, CFO Hz or NaN, 0, 0)."""
    _destroy = "srsgpu_pusch_chest_plan_destroy"

    def __init__(self, ctx: Context, cfg_array, grid_nof_prb: int, grid_nof_ports: int = 4, exts=None):
        self.ctx = ctx
        if exts is None:
            self._create("srsgpu_pusch_chest_plan_create", ctx.handle, _cptr(cfg_array), len(cfg_array), grid_nof_prb,
                         grid_nof_ports)
        else:
            self._create("srsgpu_pusch_chest_plan_create_ex", ctx.handle, _cptr(cfg_array), _cptr(exts),
                         len(cfg_array), grid_nof_prb, grid_nof_ports)

    def execute(self, d_grids, d_ch_est, d_noise_var, d_metrics=None, stream=None):
        _check(_lib().srsgpu_pusch_chest_plan_execute(self.handle, _dptr(d_grids), _dptr(d_ch_est), _dptr(d_noise_var),
                                                      _dptr(d_metrics), _stream_handle(stream)))

    def execute_copy(self, d_grids, d_ch_est, d_noise_var, spans, d_metrics=None, stream=None):
        """execute, with the copies spans = [(src, dst)] done by extra workgroups of the same launch. Returns the
        device span list (keep it alive until the stream has run the launch)."""
        d, nbytes = span_list(spans)
        _check(_lib().srsgpu_pusch_chest_plan_execute_copy(self.handle, _dptr(d_grids), _dptr(d_ch_est),
                                                           _dptr(d_noise_var), _dptr(d_metrics), _dptr(d), len(spans),
                                                           int(nbytes.max()), _stream_handle(stream)))
        return d


class PuschChannelEstimator:
    """GPU counterpart of srsran::dmrs_pusch_estimator::estimate (dmrs_pusch_estimator_impl.cpp:28)."""

    def __init__(self, ctx: Context, grid_nof_prb: int, grid_nof_ports: int = 4):
        self.ctx, self.grid_nof_prb, self.grid_nof_ports = ctx, grid_nof_prb, grid_nof_ports

    def estimate_batch(self, grids_u16, ests: Sequence[PuschChannelEstimation], grid_index: Sequence[int]):
        """grids_u16 (S, Pg, 14, nsc, 2) -> (estimates (S, 4, Pg, 14, nsc, 2) uint16, noise_var (ntx, 4),
        metrics (ntx, 4, CHEST_METRICS))."""
        dev = torch.device("cuda", self.ctx.device)
        exts, _keep = make_crb_mask_exts(ests, self.grid_nof_prb)
        plan = PuschChannelEstimatorPlan(self.ctx, make_pusch_chest_configs(ests, grid_index), self.grid_nof_prb,
                                         self.grid_nof_ports, exts)
        g = np.ascontiguousarray(grids_u16, np.uint16)
        S = g.shape[0]
        d_g = torch.from_numpy(g.view(np.int32).reshape(-1).copy()).to(dev)
        d_ce = torch.zeros(S * 4 * g.shape[1] * g.shape[2] * g.shape[3], dtype=torch.int32, device=dev)
        d_nv = torch.zeros(4 * len(ests), dtype=torch.float32, device=dev)
        d_m = torch.zeros(4 * CHEST_METRICS * len(ests), dtype=torch.float32, device=dev)
        plan.execute(d_g, d_ce, d_nv, d_m)
        torch.cuda.synchronize(dev)
        plan.close()
        ce = d_ce.cpu().numpy().view(np.uint16).reshape((S, 4) + g.shape[1:])
        return ce, d_nv.cpu().numpy().reshape(-1, 4), d_m.cpu().numpy().reshape(-1, 4, CHEST_METRICS)


class PuschDemodConfig(ctypes.Structure):
    """srsgpu_pusch_demod_config (include/srsgpu_phy.h): one transmission of pusch_demodulator::configuration."""
    _fields_ = [
        ("rnti", ctypes.c_uint16),
        ("n_id", ctypes.c_uint16),
        ("modulation_order", ctypes.c_uint8),
        ("nof_tx_layers", ctypes.c_uint8),
        ("nof_rx_ports", ctypes.c_uint8),
        ("start_symbol", ctypes.c_uint8),
        ("nof_symbols", ctypes.c_uint8),
        ("dmrs_type", ctypes.c_uint8),
        ("nof_cdm_groups_without_data", ctypes.c_uint8),
        ("equalizer", ctypes.c_uint8),
        ("dmrs_symbol_mask", ctypes.c_uint16),
        ("rb_start", ctypes.c_uint16),
        ("nof_rb", ctypes.c_uint16),
        ("estimate_layout", ctypes.c_uint8),
        ("cfo_compensated", ctypes.c_uint8),
        ("grid_index", ctypes.c_uint32),
        ("llr_offset", ctypes.c_uint32),
        ("numerology", ctypes.c_uint8),
        ("transform_precoding", ctypes.c_uint8),
        ("pad2", ctypes.c_uint8 * 2),
    ]


assert ctypes.sizeof(PuschDemodConfig) == 32
DEMOD_STATS = 30  # SRSGPU_DEMOD_STATS: 15 rows (symbols 0..13, then the transmission) x (SINR dB, EVM)


@dataclass
class PuschDemodulation:
    """pusch_demodulator::configuration (pusch_demodulator.h:51) of one transmission, rx ports 0..nof_rx_ports-1: a
    contiguous CRB allocation [rb_start, rb_start + nof_rb) or `crb_mask` (rb_mask, one byte per grid CRB), and
    optionally transform precoding (enable_transform_precoding, one layer)."""
    rnti: int
    n_id: int
    modulation_order: int
    nof_tx_layers: int
    nof_rx_ports: int
    start_symbol: int
    nof_symbols: int
    dmrs_symbol_mask: int
    dmrs_type: int
    nof_cdm_groups_without_data: int
    rb_start: int
    nof_rb: int
    equalizer: int = EQ_ZF
    estimate_layout: int = CE_PER_SYMBOL
    cfo_compensated: int = 0  # compact layout written with CFO compensation (the estimator's compensate_cfo)
    numerology: int = 1
    crb_mask: Optional[np.ndarray] = None
    transform_precoding: int = 0

    def nof_llrs(self) -> int:
        dm = (4 if self.dmrs_type == 2 else 6) * self.nof_cdm_groups_without_data
        nrb = int(np.count_nonzero(self.crb_mask)) if self.crb_mask is not None else self.nof_rb
        nre = sum((12 - dm if (self.dmrs_symbol_mask >> l) & 1 else 12) * nrb
                  for l in range(self.start_symbol, self.start_symbol + self.nof_symbols))
        return nre * self.nof_tx_layers * self.modulation_order


def make_pusch_demod_configs(demods: Sequence[PuschDemodulation], grid_index: Sequence[int], llr_offsets=None):
    arr = (PuschDemodConfig * len(demods))()
    off = 0
    offs = []
    for i, (m, g) in enumerate(zip(demods, grid_index)):
        a = arr[i]
        a.rnti, a.n_id, a.modulation_order, a.nof_tx_layers = m.rnti, m.n_id, m.modulation_order, m.nof_tx_layers
        a.nof_rx_ports, a.start_symbol, a.nof_symbols = m.nof_rx_ports, m.start_symbol, m.nof_symbols
        a.dmrs_type, a.nof_cdm_groups_without_data, a.equalizer = (m.dmrs_type, m.nof_cdm_groups_without_data,
                                                                   m.equalizer)
        a.dmrs_symbol_mask, a.rb_start, a.nof_rb, a.grid_index = m.dmrs_symbol_mask, m.rb_start, m.nof_rb, g
        a.estimate_layout = m.estimate_layout
        a.cfo_compensated, a.numerology = m.cfo_compensated, m.numerology
        a.transform_precoding = m.transform_precoding
        a.llr_offset = off if llr_offsets is None else llr_offsets[i]
        offs.append(a.llr_offset)
        off += m.nof_llrs()
    return arr, offs, off


class PuschDemodulatorPlan(_Handle):
    """srsgpu_pusch_demodulator_plan: equalization + soft demapping + descrambling of a batch of PUSCH transmissions
    from rx grids (nslots, ports, 14, nsc) and channel estimates (nslots, 4 layers, ports, 14, nsc) (uint32 bf16 pairs)
    and noise variances (ntx, 4) float32 into int8 codeword LLRs."""
    _destroy = "srsgpu_pusch_demodulator_plan_destroy"

    def __init__(self, ctx: Context, cfg_array, grid_nof_prb: int, grid_nof_ports: int = 4, exts=None):
        self.ctx = ctx
        if exts is None:
            self._create("srsgpu_pusch_demodulator_plan_create", ctx.handle, _cptr(cfg_array), len(cfg_array),
                         grid_nof_prb, grid_nof_ports)
        else:
            self._create("srsgpu_pusch_demodulator_plan_create_ex", ctx.handle, _cptr(cfg_array), _cptr(exts),
                         len(cfg_array), grid_nof_prb, grid_nof_ports)
        self.nof_tx = len(cfg_array)

    def nof_llrs(self, tx: int) -> int:
        return int(_lib().srsgpu_pusch_demodulator_plan_nof_llrs(self.handle, tx))

    def symbol_closed_form(self, tx: int) -> bool:
        """The plan finds the OFDM symbol of transmission `tx`'s REs by the closed form, not by the search."""
        return bool(_lib().srsgpu_pusch_demodulator_plan_symbol_closed_form(self.handle, tx))

    def execute(self, d_grids, d_ch_est, d_noise_var, d_llrs, stream=None, d_stats=None):
        """d_stats: optional float32 device buffer of DEMOD_STATS floats per transmission (SINR dB / EVM rows)."""
        if d_stats is None:
            _check(_lib().srsgpu_pusch_demodulator_plan_execute(self.handle, _dptr(d_grids), _dptr(d_ch_est),
                                                                _dptr(d_noise_var), _dptr(d_llrs),
                                                                _stream_handle(stream)))
        else:
            _check(_lib().srsgpu_pusch_demodulator_plan_execute_ex(self.handle, _dptr(d_grids), _dptr(d_ch_est),
                                                                   _dptr(d_noise_var), _dptr(d_llrs), _dptr(d_stats),
                                                                   _stream_handle(stream)))


class PuschDemodulator:
    """GPU counterpart of srsran::pusch_demodulator::demodulate (pusch_demodulator_impl.cpp:272): demodulate() takes
    bf16 grids / channel estimates as uint16 (..., 2) arrays and returns the codeword LLRs (int8) of each
    transmission."""

    def __init__(self, ctx: Context, grid_nof_prb: int, grid_nof_ports: int = 4):
        self.ctx, self.grid_nof_prb, self.grid_nof_ports = ctx, grid_nof_prb, grid_nof_ports

    def demodulate_batch(self, grids_u16, ch_est_u16, noise_vars, demods: Sequence[PuschDemodulation],
                         grid_index: Sequence[int], with_stats: bool = False):
        """grids_u16 (S, Pg, 14, nsc, 2); ch_est_u16 (S, 4, Pg, 14, nsc, 2); noise_vars (ntx, 4). Returns the LLRs of
        each transmission and, with_stats, also the (ntx, 15, 2) statistics (SINR dB, EVM per symbol / total)."""
        dev = torch.device("cuda", self.ctx.device)
        arr, offs, total = make_pusch_demod_configs(demods, grid_index)
        exts, _keep = make_crb_mask_exts(demods, self.grid_nof_prb)
        plan = PuschDemodulatorPlan(self.ctx, arr, self.grid_nof_prb, self.grid_nof_ports, exts)
        g = torch.from_numpy(np.ascontiguousarray(grids_u16, np.uint16).view(np.int32).reshape(-1).copy()).to(dev)
        h = torch.from_numpy(np.ascontiguousarray(ch_est_u16, np.uint16).view(np.int32).reshape(-1).copy()).to(dev)
        nv = torch.from_numpy(np.ascontiguousarray(noise_vars, np.float32).reshape(-1).copy()).to(dev)
        out = torch.full((max(total, 4),), 77, dtype=torch.int8, device=dev)
        st = torch.full((max(len(demods), 1) * DEMOD_STATS,), 55.0, dtype=torch.float32, device=dev) \
            if with_stats else None
        plan.execute(g, h, nv, out, d_stats=st)
        torch.cuda.synchronize(dev)
        n = [plan.nof_llrs(i) for i in range(len(demods))]
        plan.close()
        o = out.cpu().numpy()
        llrs = [o[a:a + k] for a, k in zip(offs, n)]
        if not with_stats:
            return llrs
        return llrs, st.cpu().numpy()[:len(demods) * DEMOD_STATS].reshape(len(demods), 15, 2)


class UlschDemuxConfig(ctypes.Structure):
    """srsgpu_ulsch_demux_config (include/srsgpu_phy.h): ulsch_demultiplex::configuration of one transmission plus
    the CSI Part 2 size, the scrambling identity (placeholders) and the stream offsets."""
    _fields_ = [
        ("modulation_order", ctypes.c_uint8),
        ("nof_layers", ctypes.c_uint8),
        ("nof_prb", ctypes.c_uint16),
        ("start_symbol", ctypes.c_uint8),
        ("nof_symbols", ctypes.c_uint8),
        ("dmrs_symbol_mask", ctypes.c_uint16),
        ("dmrs_type", ctypes.c_uint8),
        ("nof_cdm_groups_without_data", ctypes.c_uint8),
        ("rnti", ctypes.c_uint16),
        ("n_id", ctypes.c_uint16),
        ("csi2_first_symbol", ctypes.c_uint16),
        ("nof_harq_ack_rvd", ctypes.c_uint32),
        ("nof_harq_ack_bits", ctypes.c_uint32),
        ("nof_enc_harq_ack_bits", ctypes.c_uint32),
        ("nof_csi_part1_bits", ctypes.c_uint32),
        ("nof_enc_csi_part1_bits", ctypes.c_uint32),
        ("nof_csi_part2_bits", ctypes.c_uint32),
        ("nof_enc_csi_part2_bits", ctypes.c_uint32),
        ("llr_offset", ctypes.c_uint32),
        ("sch_offset", ctypes.c_uint32),
        ("harq_offset", ctypes.c_uint32),
        ("csi1_offset", ctypes.c_uint32),
        ("csi2_offset", ctypes.c_uint32),
    ]


assert ctypes.sizeof(UlschDemuxConfig) == 64


@dataclass
class UlschDemultiplexing:
    """ulsch_demultiplex::configuration (ulsch_demultiplex.h:48) + set_csi_part2 sizes + the transmission's rnti /
    n_id (scrambling of the UCI placeholders)."""
    modulation_order: int
    nof_layers: int
    nof_prb: int
    start_symbol: int
    nof_symbols: int
    dmrs_symbol_mask: int
    dmrs_type: int
    nof_cdm_groups_without_data: int
    rnti: int
    n_id: int
    nof_harq_ack_rvd: int = 0
    nof_harq_ack_bits: int = 0
    nof_enc_harq_ack_bits: int = 0
    nof_csi_part1_bits: int = 0
    nof_enc_csi_part1_bits: int = 0
    nof_csi_part2_bits: int = 0
    nof_enc_csi_part2_bits: int = 0
    csi2_first_symbol: int = 0  # CSI Part 2 from this symbol on (the processor's set_csi_part2 point; 0: from the start)


class UlschDemuxPlan(_Handle):
    """srsgpu_ulsch_demux_plan: UCI-on-PUSCH demultiplexing of a batch of codewords (int8 LLRs) into the UL-SCH,
    HARQ-ACK, CSI Part 1 and CSI Part 2 streams."""
    _destroy = "srsgpu_ulsch_demux_plan_destroy"

    STREAMS = ("codeword", "sch", "harq", "csi1", "csi2")

    def __init__(self, ctx: Context, demuxes: Sequence[UlschDemultiplexing], llr_offsets: Sequence[int]):
        self.ctx = ctx
        arr = (UlschDemuxConfig * len(demuxes))()
        for i, (m, off) in enumerate(zip(demuxes, llr_offsets)):
            a = arr[i]
            for f, _ in UlschDemuxConfig._fields_:
                if hasattr(m, f):
                    setattr(a, f, getattr(m, f))
            a.llr_offset = off
        # First pass sizes the output streams, the second fixes their offsets.
        self._create("srsgpu_ulsch_demux_plan_create", ctx.handle, _cptr(arr), len(arr))
        n = [[int(_lib().srsgpu_ulsch_demux_plan_nof_llrs(self.handle, t, k)) for k in range(5)]
             for t in range(len(arr))]
        self.close()
        self.offsets = {k: [] for k in self.STREAMS[1:]}
        self.totals = {}
        for j, k in enumerate(self.STREAMS[1:]):
            o = 0
            for t in range(len(arr)):
                self.offsets[k].append(o)
                o += n[t][j + 1]
            self.totals[k] = o
        for t in range(len(arr)):
            arr[t].sch_offset, arr[t].harq_offset = self.offsets["sch"][t], self.offsets["harq"][t]
            arr[t].csi1_offset, arr[t].csi2_offset = self.offsets["csi1"][t], self.offsets["csi2"][t]
        self._create("srsgpu_ulsch_demux_plan_create", ctx.handle, _cptr(arr), len(arr))
        self.counts = n

    def symbol_llrs(self, tx: int, stream: str) -> np.ndarray:
        """LLRs of `stream` (codeword, sch, harq, csi1, csi2) per OFDM symbol 0..13 of transmission tx."""
        out = np.zeros(14, np.uint32)
        _check(_lib().srsgpu_ulsch_demux_plan_symbol_llrs(self.handle, tx, self.STREAMS.index(stream),
                                                          out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def execute(self, d_llrs, d_sch, d_harq=None, d_csi1=None, d_csi2=None, stream=None):
        _check(_lib().srsgpu_ulsch_demux_plan_execute(self.handle, _dptr(d_llrs), _dptr(d_sch), _dptr(d_harq),
                                                      _dptr(d_csi1), _dptr(d_csi2), _stream_handle(stream)))


class UlschDemultiplexer:
    """GPU counterpart of srsran::ulsch_demultiplex (ulsch_demultiplex_impl.cpp:199): demultiplex_batch() takes each
    transmission's codeword LLRs and returns dicts of the sch / harq / csi1 / csi2 LLR streams."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def demultiplex_batch(self, codewords: Sequence[np.ndarray], demuxes: Sequence[UlschDemultiplexing]):
        dev = torch.device("cuda", self.ctx.device)
        offs, o = [], 0
        for cw in codewords:
            offs.append(o)
            o += cw.size
        plan = UlschDemuxPlan(self.ctx, demuxes, offs)
        d_in = torch.from_numpy(np.concatenate([np.asarray(c, np.int8) for c in codewords])).to(dev)
        outs = {k: torch.full((max(plan.totals[k], 4),), 99, dtype=torch.int8, device=dev) for k in plan.totals}
        plan.execute(d_in, outs["sch"], outs["harq"], outs["csi1"], outs["csi2"])
        torch.cuda.synchronize(dev)
        host = {k: v.cpu().numpy() for k, v in outs.items()}
        res = []
        for t in range(len(demuxes)):
            res.append({k: host[k][plan.offsets[k][t]: plan.offsets[k][t] + plan.counts[t][j + 1]]
                        for j, k in enumerate(("sch", "harq", "csi1", "csi2"))})
        plan.close()
        return res


class PuschTbConfig(ctypes.Structure):
    """srsgpu_pusch_tb_config (include/srsgpu_phy.h)."""
    _fields_ = [
        ("base_graph", ctypes.c_uint8),
        ("rv", ctypes.c_uint8),
        ("modulation_order", ctypes.c_uint8),
        ("nof_layers", ctypes.c_uint8),
        ("new_data", ctypes.c_uint8),
        ("use_early_stop", ctypes.c_uint8),
        ("max_iterations", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8),
        ("scaling_factor", ctypes.c_float),
        ("tbs_bytes", ctypes.c_uint32),
        ("nof_ch_symbols", ctypes.c_uint32),
        ("Nref", ctypes.c_uint32),
        ("llr_offset", ctypes.c_uint32),
        ("harq_offset", ctypes.c_uint32),
        ("cb_offset", ctypes.c_uint32),
        ("tb_offset", ctypes.c_uint32),
    ]


assert ctypes.sizeof(PuschTbConfig) == 40
CB_MSG_STRIDE = 1056


@dataclass
class PuschTransportBlock:
    """pusch_decoder::configuration (pusch_decoder.h:55) + the TB geometry of one transport block."""
    tbs_bytes: int
    base_graph: int
    rv: int
    modulation_order: int
    nof_layers: int
    nof_ch_symbols: int
    Nref: int = 0
    new_data: bool = True
    use_early_stop: bool = True
    nof_ldpc_iterations: int = 6
    scaling_factor: float = 0.8


def make_pusch_tb_configs(tbs: Sequence[PuschTransportBlock], nof_cbs: Sequence[int], cb_lengths: Sequence[int]):
    """Contiguous layout: codeword LLRs, HARQ buffers (C * N per TB), codeblock slots, TB bytes.
    nof_cbs[i] / cb_lengths[i] (N_short * Z) come from the segmentation (srsgpu.sch)."""
    arr = (PuschTbConfig * len(tbs))()
    lo = ho = co = to = 0
    for i, t in enumerate(tbs):
        a = arr[i]
        a.base_graph, a.rv, a.modulation_order, a.nof_layers = t.base_graph, t.rv, t.modulation_order, t.nof_layers
        a.new_data, a.use_early_stop, a.max_iterations = int(t.new_data), int(t.use_early_stop), t.nof_ldpc_iterations
        a.scaling_factor, a.tbs_bytes, a.nof_ch_symbols, a.Nref = t.scaling_factor, t.tbs_bytes, t.nof_ch_symbols, t.Nref
        a.llr_offset, a.harq_offset, a.cb_offset, a.tb_offset = lo, ho, co, to
        lo += t.nof_ch_symbols * t.modulation_order
        ho += nof_cbs[i] * cb_lengths[i]
        co += nof_cbs[i]
        to += t.tbs_bytes
    return arr, lo, ho, co, to


class PuschDecoderPlan(_Handle):
    """srsgpu_pusch_decoder_plan (TB level)."""
    _destroy = "srsgpu_pusch_decoder_plan_destroy"

    def __init__(self, ctx: Context, impl: int, cfg_array):
        self.ctx = ctx
        self._create("srsgpu_pusch_decoder_plan_create", ctx.handle, impl, _cptr(cfg_array), len(cfg_array))
        self.nof_tbs = len(cfg_array)
        self.nof_codeblocks = int(_lib().srsgpu_pusch_decoder_plan_nof_codeblocks(self.handle))
        self.decoder_input_llrs = int(_lib().srsgpu_pusch_decoder_plan_decoder_input_llrs(self.handle))

    def execute(self, d_llrs, d_harq, d_cb_crc_ok, d_cb_msgs, d_cb_iters, d_tbs, d_tb_crc_ok, stream=None):
        _check(_lib().srsgpu_pusch_decoder_plan_execute(self.handle, _dptr(d_llrs), _dptr(d_harq), _dptr(d_cb_crc_ok),
                                                        _dptr(d_cb_msgs), _dptr(d_cb_iters), _dptr(d_tbs),
                                                        _dptr(d_tb_crc_ok), _stream_handle(stream)))

    def execute_arena(self, d_llrs, d_harq_cbs, d_cb_crc_ok, d_cb_msgs, d_cb_iters, d_tbs, d_tb_crc_ok, stream=None):
        """As execute, with codeblock c's HARQ soft buffer at the device address d_harq_cbs[c] (an int64 tensor of one
        pointer per codeblock, e.g. slots of a persistent arena) instead of in a contiguous batch buffer."""
        _check(_lib().srsgpu_pusch_decoder_plan_execute_arena(self.handle, _dptr(d_llrs), _dptr(d_harq_cbs),
                                                              _dptr(d_cb_crc_ok), _dptr(d_cb_msgs), _dptr(d_cb_iters),
                                                              _dptr(d_tbs), _dptr(d_tb_crc_ok), _stream_handle(stream)))

    def assemble(self, d_cb_crc_ok, d_cb_msgs, d_tbs, d_tb_crc_ok, stream=None):
        """TB stage only, from codeblock messages / flags decoded elsewhere (codeblock-sharded decoding)."""
        _check(_lib().srsgpu_pusch_decoder_plan_assemble(self.handle, _dptr(d_cb_crc_ok), _dptr(d_cb_msgs), _dptr(d_tbs),
                                                         _dptr(d_tb_crc_ok), _stream_handle(stream)))

    def enable_timing(self, enable=True, decode_only=False):
        """Stage events on every execute: all three stages, or (decode_only) just around the LDPC decoding."""
        _check(_lib().srsgpu_pusch_decoder_plan_enable_timing(self.handle, (2 if decode_only else 1) if enable else 0))

    def stage_times(self):
        """([ms dematch, ms decode, ms TB stage], number of executes) accumulated since the previous call."""
        return _stage_times("srsgpu_pusch_decoder_plan", self.handle, 3)


class PuschDecoder:
    """GPU counterpart of srsran::pusch_decoder with a device-resident HARQ context (one per set of TBs)."""

    def __init__(self, ctx: Context, dec_type: str = "auto"):
        if dec_type not in IMPL_BY_NAME:
            raise SrsGpuError(f"invalid decoder type '{dec_type}'")
        self.ctx = ctx
        self.impl = IMPL_BY_NAME[dec_type]
        self.harq = None

    def decode_batch(self, llrs_list, tbs: Sequence[PuschTransportBlock]):
        """Returns (tb_crc_ok list, TB byte arrays, per-TB lists of CB iteration counts). The HARQ context is kept
        between calls (retransmissions: same TBs, new_data False)."""
        from . import sch
        nof_cbs, cb_len = [], []
        for t in tbs:
            seg = sch.segment(t.tbs_bytes * 8, t.base_graph, t.modulation_order, t.nof_layers, t.nof_ch_symbols)
            nof_cbs.append(seg.nof_segments)
            cb_len.append((66 if t.base_graph == 1 else 50) * seg.lifting_size)
        arr, nllr, nharq, ncb, ntb = make_pusch_tb_configs(tbs, nof_cbs, cb_len)
        dev = torch.device("cuda", self.ctx.device)
        if self.harq is None or self.harq[0].numel() != nharq:
            self.harq = (torch.zeros(nharq, dtype=torch.int8, device=dev),
                         torch.zeros(ncb, dtype=torch.uint8, device=dev),
                         torch.zeros(ncb * CB_MSG_STRIDE, dtype=torch.uint8, device=dev))
        d_harq, d_crc, d_msgs = self.harq
        d_llrs = torch.from_numpy(np.concatenate([np.asarray(x, np.int8) for x in llrs_list])).to(dev)
        assert d_llrs.numel() == nllr
        d_iters = torch.zeros(ncb, dtype=torch.int32, device=dev)
        d_tbs = torch.zeros(max(ntb, 1), dtype=torch.uint8, device=dev)
        d_tb_ok = torch.zeros(len(tbs), dtype=torch.uint8, device=dev)
        plan = PuschDecoderPlan(self.ctx, self.impl, arr)
        plan.execute(d_llrs, d_harq, d_crc, d_msgs, d_iters, d_tbs, d_tb_ok)
        torch.cuda.synchronize(dev)
        plan.close()
        ok = d_tb_ok.cpu().numpy()
        tb_bytes = d_tbs.cpu().numpy()
        iters = d_iters.cpu().numpy()
        out_tbs, out_iters = [], []
        off = co = 0
        for i, t in enumerate(tbs):
            out_tbs.append(tb_bytes[off: off + t.tbs_bytes].copy())
            out_iters.append(iters[co: co + nof_cbs[i]].tolist())
            off += t.tbs_bytes
            co += nof_cbs[i]
        return [bool(x) for x in ok], out_tbs, out_iters
