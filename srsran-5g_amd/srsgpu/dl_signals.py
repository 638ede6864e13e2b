"""The rest of the downlink grid: PDCCH (srsgpu_pdcch_plan), SS/PBCH blocks (srsgpu_ssb_plan) and NZP-CSI-RS
(srsgpu_csi_rs_plan)."""
import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from ._abi import Context, SrsGpuError, torch, _check, _cptr, _dptr, _Handle, _lib, _stream_handle


class PdcchConfig(ctypes.Structure):
    """srsgpu_pdcch_config (include/srsgpu_phy.h): the CORESET, the DCI, linear amplitudes, one weight per port, where
    the payload bits lie in the payload buffer and the grid the DCI is mapped into."""
    _fields_ = [
        ("frequency_resources", ctypes.c_uint64),
        ("bwp_size_rb", ctypes.c_uint32),
        ("bwp_start_rb", ctypes.c_uint32),
        ("start_symbol_index", ctypes.c_uint32),
        ("duration", ctypes.c_uint32),
        ("cce_to_reg_mapping", ctypes.c_uint32),
        ("reg_bundle_size", ctypes.c_uint32),
        ("interleaver_size", ctypes.c_uint32),
        ("shift_index", ctypes.c_uint32),
        ("slot_index", ctypes.c_uint32),
        ("rnti", ctypes.c_uint32),
        ("n_id_pdcch_dmrs", ctypes.c_uint32),
        ("n_id_pdcch_data", ctypes.c_uint32),
        ("n_rnti", ctypes.c_uint32),
        ("cce_index", ctypes.c_uint32),
        ("aggregation_level", ctypes.c_uint32),
        ("nof_ports", ctypes.c_uint32),
        ("data_scaling", ctypes.c_float),
        ("dmrs_amplitude", ctypes.c_float),
        ("precoding", ctypes.c_float * 8),
        ("payload_offset", ctypes.c_uint32),
        ("nof_payload_bits", ctypes.c_uint32),
        ("grid_index", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


assert ctypes.sizeof(PdcchConfig) == 128


@dataclass
class Pdcch:
    """pdcch_processor::pdu_t (pdcch_processor.h:134) of one DCI: the CORESET (frequency_resources: bit i set = the 6-PRB
    resource i; mapping 0 CORESET0, 1 non-interleaved, 2 interleaved), the DCI with its payload bits, linear
    amplitudes in place of the dB offsets, and one complex precoding weight per port."""
    bwp_size_rb: int
    bwp_start_rb: int
    start_symbol: int
    duration: int
    frequency_resources: int
    mapping: int
    slot_index: int
    rnti: int
    n_id_pdcch_dmrs: int
    n_id_pdcch_data: int
    n_rnti: int
    cce_index: int
    aggregation_level: int
    payload: np.ndarray
    weights: np.ndarray
    reg_bundle_size: int = 0
    interleaver_size: int = 0
    shift_index: int = 0
    data_scaling: float = 1.0
    dmrs_amplitude: float = 1.0
    grid_index: int = 0


def pdcch_pack_payloads(dcis: Sequence[Pdcch]):
    """The DCIs' payload bits packed MSB first, each from a byte boundary: (uint8 buffer, byte offsets)."""
    chunks, offsets, pos = [], [], 0
    for d in dcis:
        packed = np.packbits(np.asarray(d.payload, np.uint8))
        offsets.append(pos)
        chunks.append(packed)
        pos += packed.size
    return (np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)), offsets


def make_pdcch_configs(dcis: Sequence[Pdcch], payload_offsets: Sequence[int]):
    arr = (PdcchConfig * max(len(dcis), 1))()
    for a, d, o in zip(arr, dcis, payload_offsets):
        a.frequency_resources, a.bwp_size_rb, a.bwp_start_rb = d.frequency_resources, d.bwp_size_rb, d.bwp_start_rb
        a.start_symbol_index, a.duration, a.cce_to_reg_mapping = d.start_symbol, d.duration, d.mapping
        a.reg_bundle_size, a.interleaver_size, a.shift_index = d.reg_bundle_size, d.interleaver_size, d.shift_index
        a.slot_index, a.rnti, a.n_id_pdcch_dmrs, a.n_id_pdcch_data = d.slot_index, d.rnti, d.n_id_pdcch_dmrs, d.n_id_pdcch_data
        a.n_rnti, a.cce_index, a.aggregation_level = d.n_rnti, d.cce_index, d.aggregation_level
        wc = np.asarray(d.weights, np.complex64).ravel()
        a.nof_ports = wc.size
        w = np.zeros((4, 2), np.float32)
        w[: min(wc.size, 4), 0], w[: min(wc.size, 4), 1] = wc.real[:4], wc.imag[:4]
        a.precoding[:] = w.reshape(-1).tolist()
        a.data_scaling, a.dmrs_amplitude = float(d.data_scaling), float(d.dmrs_amplitude)
        a.payload_offset, a.nof_payload_bits, a.grid_index = o, int(np.asarray(d.payload).size), d.grid_index
    return arr


class PdcchPlan(_Handle):
    """srsgpu_pdcch_plan: every DCI of a batch of slots encoded, modulated and mapped with its DM-RS in one launch.
    dcis: Pdcch entries; payload_offsets: byte offset of each DCI's packed payload in the buffer given to execute()
    (default: pdcch_pack_payloads order). self.payload_bytes: the least size of that buffer."""
    _destroy = "srsgpu_pdcch_plan_destroy"

    def __init__(self, ctx: Context, dcis: Sequence[Pdcch], grid_nof_prb: int, grid_nof_ports: int = 4,
                 nof_grids: Optional[int] = None, payload_offsets: Optional[Sequence[int]] = None):
        self.ctx = ctx
        self.nof_dcis = len(dcis)
        if payload_offsets is None:
            _, payload_offsets = pdcch_pack_payloads(dcis)
        if nof_grids is None:
            nof_grids = max([d.grid_index for d in dcis], default=0) + 1
        self.nof_grids, self.grid_nof_prb, self.grid_nof_ports = nof_grids, grid_nof_prb, grid_nof_ports
        self.payload_bytes = max([o + (np.asarray(d.payload).size + 7) // 8 for o, d in zip(payload_offsets, dcis)],
                                 default=0)
        arr = make_pdcch_configs(dcis, payload_offsets)
        self._create("srsgpu_pdcch_plan_create", ctx.handle, _cptr(arr), len(dcis), grid_nof_prb, grid_nof_ports,
                     nof_grids)

    def execute(self, d_payloads, d_grids, stream=None):
        """d_payloads: uint8 device tensor of the packed payloads; d_grids: (nof_grids, ports, 14, 12 PRBs) int32 /
        uint32 words (re | im << 16, bf16). Asynchronous on `stream`."""
        _check(_lib().srsgpu_pdcch_plan_execute(self.handle, _dptr(d_payloads), int(d_payloads.numel() * d_payloads.element_size()),
                                                _dptr(d_grids),
                                                _stream_handle(stream)))


class PdcchProcessor:
    """GPU counterpart of pdcch_processor_impl::process for a list of DCIs: process_batch() returns the grids as a
    (nof_grids, ports, 14, 12 PRBs) uint32 array (re | im << 16), every RE no DCI writes holding `fill`."""

    def __init__(self, ctx: Context, grid_nof_prb: int, grid_nof_ports: int = 4):
        self.ctx, self.grid_nof_prb, self.grid_nof_ports = ctx, grid_nof_prb, grid_nof_ports

    def process_batch(self, dcis: Sequence[Pdcch], nof_grids: Optional[int] = None, fill: int = 0) -> np.ndarray:
        dev = torch.device("cuda", self.ctx.device)
        payloads, offsets = pdcch_pack_payloads(dcis)
        plan = PdcchPlan(self.ctx, dcis, self.grid_nof_prb, self.grid_nof_ports, nof_grids, offsets)
        d_payloads = torch.from_numpy(np.concatenate([payloads, np.zeros(1, np.uint8)])).to(dev)
        host = np.full((plan.nof_grids, self.grid_nof_ports, 14, 12 * self.grid_nof_prb), fill, np.uint32)
        d_grids = torch.from_numpy(host.view(np.int32)).to(dev)
        plan.execute(d_payloads, d_grids)
        torch.cuda.synchronize(dev)
        plan.close()
        return d_grids.cpu().numpy().view(np.uint32)


class SsbConfig(ctypes.Structure):
    """srsgpu_ssb_config (include/srsgpu_phy.h): ssb_processor::pdu_t of one block without the payload and the SFN, a
    linear PSS amplitude, the port list, the grid the block is mapped into and where its four bytes lie in the payload
    buffer."""
    _fields_ = [
        ("phys_cell_id", ctypes.c_uint32),
        ("ssb_idx", ctypes.c_uint32),
        ("L_max", ctypes.c_uint32),
        ("pattern_case", ctypes.c_uint32),
        ("common_scs", ctypes.c_uint32),
        ("offset_to_pointA", ctypes.c_uint32),
        ("subcarrier_offset", ctypes.c_uint32),
        ("slot_index", ctypes.c_uint32),
        ("hrf", ctypes.c_uint32),
        ("pss_amplitude", ctypes.c_float),
        ("nof_ports", ctypes.c_uint32),
        ("ports", ctypes.c_uint8 * 4),
        ("grid_index", ctypes.c_uint32),
        ("payload_offset", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32 * 2),
    ]


assert ctypes.sizeof(SsbConfig) == 64


@dataclass
class Ssb:
    """ssb_processor::pdu_t (ssb_processor.h:42) of one block: pattern_case 0..4 = A..E, common_scs a numerology,
    slot_index the slot within the half frame, a linear PSS amplitude in place of beta_pss, the 24 BCH payload bits and
    the SFN (its four LSBs are used)."""
    phys_cell_id: int
    ssb_idx: int
    L_max: int
    pattern_case: int
    common_scs: int
    offset_to_pointA: int
    subcarrier_offset: int
    slot_index: int
    hrf: int
    payload: np.ndarray
    sfn: int = 0
    ports: Sequence[int] = (0,)
    pss_amplitude: float = 1.0
    grid_index: int = 0


def ssb_pack_payloads(blocks: Sequence[Ssb]):
    """Four bytes per block, in order: the 24 payload bits MSB first, then sfn & 15: (uint8 buffer, byte offsets)."""
    chunks = [np.concatenate([np.packbits(np.asarray(b.payload, np.uint8)[:24]), [b.sfn & 15]]).astype(np.uint8)
              for b in blocks]
    return (np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)), [4 * i for i in range(len(blocks))]


def make_ssb_configs(blocks: Sequence[Ssb], payload_offsets: Sequence[int]):
    arr = (SsbConfig * max(len(blocks), 1))()
    for a, b, o in zip(arr, blocks, payload_offsets):
        a.phys_cell_id, a.ssb_idx, a.L_max, a.pattern_case = b.phys_cell_id, b.ssb_idx, b.L_max, b.pattern_case
        a.common_scs, a.offset_to_pointA, a.subcarrier_offset = b.common_scs, b.offset_to_pointA, b.subcarrier_offset
        a.slot_index, a.hrf, a.pss_amplitude = b.slot_index, b.hrf, float(b.pss_amplitude)
        ports = [int(p) for p in b.ports]
        a.nof_ports = len(ports)
        a.ports[:] = [min(p, 255) for p in (ports + [0] * 4)[:4]]
        a.grid_index, a.payload_offset = b.grid_index, o
    return arr


class SsbPlan(_Handle):
    """srsgpu_ssb_plan: every SS/PBCH block of a batch of slots encoded, modulated and mapped with its DM-RS, PSS and SSS
    in one launch. payload_offsets: byte offset of each block's four bytes in the buffer given to execute() (default:
    ssb_pack_payloads order). self.payload_bytes: the least size of that buffer."""
    _destroy = "srsgpu_ssb_plan_destroy"

    def __init__(self, ctx: Context, blocks: Sequence[Ssb], grid_nof_prb: int, grid_nof_ports: int = 4,
                 nof_grids: Optional[int] = None, payload_offsets: Optional[Sequence[int]] = None):
        self.ctx = ctx
        self.nof_blocks = len(blocks)
        if payload_offsets is None:
            payload_offsets = [4 * i for i in range(len(blocks))]
        if nof_grids is None:
            nof_grids = max([b.grid_index for b in blocks], default=0) + 1
        self.nof_grids, self.grid_nof_prb, self.grid_nof_ports = nof_grids, grid_nof_prb, grid_nof_ports
        self.payload_bytes = max([o + 4 for o, _ in zip(payload_offsets, blocks)], default=0)
        arr = make_ssb_configs(blocks, payload_offsets)
        self._create("srsgpu_ssb_plan_create", ctx.handle, _cptr(arr), len(blocks), grid_nof_prb, grid_nof_ports,
                     nof_grids)

    def execute(self, d_payloads, d_grids, stream=None):
        """d_payloads: uint8 device tensor, four bytes per block; d_grids: (nof_grids, ports, 14, 12 PRBs) int32 / uint32
        words (re | im << 16, bf16). Asynchronous on `stream`."""
        _check(_lib().srsgpu_ssb_plan_execute(self.handle, _dptr(d_payloads), int(d_payloads.numel() * d_payloads.element_size()),
                                              _dptr(d_grids), _stream_handle(stream)))


class SsbProcessor:
    """GPU counterpart of ssb_processor_impl::process for a list of blocks: process_batch() returns the grids as a
    (nof_grids, ports, 14, 12 PRBs) uint32 array (re | im << 16), every RE no block writes holding `fill`."""

    def __init__(self, ctx: Context, grid_nof_prb: int, grid_nof_ports: int = 4):
        self.ctx, self.grid_nof_prb, self.grid_nof_ports = ctx, grid_nof_prb, grid_nof_ports

    def process_batch(self, blocks: Sequence[Ssb], nof_grids: Optional[int] = None, fill: int = 0) -> np.ndarray:
        dev = torch.device("cuda", self.ctx.device)
        payloads, offsets = ssb_pack_payloads(blocks)
        plan = SsbPlan(self.ctx, blocks, self.grid_nof_prb, self.grid_nof_ports, nof_grids, offsets)
        d_payloads = torch.from_numpy(np.concatenate([payloads, np.zeros(1, np.uint8)])).to(dev)
        host = np.full((plan.nof_grids, self.grid_nof_ports, 14, 12 * self.grid_nof_prb), fill, np.uint32)
        d_grids = torch.from_numpy(host.view(np.int32)).to(dev)
        plan.execute(d_payloads, d_grids)
        torch.cuda.synchronize(dev)
        plan.close()
        return d_grids.cpu().numpy().view(np.uint32)


class CsiRsConfig(ctypes.Structure):
    """srsgpu_csi_rs_config (include/srsgpu_phy.h): nzp_csi_rs_generator::config_t of one signal with a ports x ports
    precoding matrix ([port][layer] (re, im)) and the grid the signal is mapped into."""
    _fields_ = [
        ("slot_index", ctypes.c_uint32),
        ("cp", ctypes.c_uint32),
        ("start_rb", ctypes.c_uint32),
        ("nof_rb", ctypes.c_uint32),
        ("row", ctypes.c_uint32),
        ("nof_k_ref", ctypes.c_uint32),
        ("k_ref", ctypes.c_uint32 * 6),
        ("symbol_l0", ctypes.c_uint32),
        ("symbol_l1", ctypes.c_uint32),
        ("cdm", ctypes.c_uint32),
        ("freq_density", ctypes.c_uint32),
        ("scrambling_id", ctypes.c_uint32),
        ("amplitude", ctypes.c_float),
        ("nof_ports", ctypes.c_uint32),
        ("precoding", ctypes.c_float * 32),
        ("grid_index", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


assert ctypes.sizeof(CsiRsConfig) == 212


@dataclass
class CsiRs:
    """nzp_csi_rs_generator::config_t (nzp_csi_rs_generator.h:46) of one signal: cdm 0 none / 1 FD-CDM2 / 2 CDM4 / 3 CDM8,
    freq_density 0 0.5 on even RBs / 1 0.5 on odd RBs / 2 one / 3 three, a linear amplitude, and the one-PRG precoding
    as a (ports, ports) complex matrix [port, layer] (None: the identity)."""
    slot_index: int
    start_rb: int
    nof_rb: int
    row: int
    k_ref: Sequence[int]
    symbol_l0: int
    cdm: int
    freq_density: int
    scrambling_id: int
    amplitude: float = 1.0
    weights: Optional[np.ndarray] = None
    symbol_l1: int = 0
    cp: int = 0
    grid_index: int = 0


CSI_RS_ROW_PORTS = {1: 1, 2: 1, 3: 2, 4: 4, 5: 4}


def make_csi_rs_configs(signals: Sequence[CsiRs]):
    arr = (CsiRsConfig * max(len(signals), 1))()
    for a, s in zip(arr, signals):
        a.slot_index, a.cp, a.start_rb, a.nof_rb, a.row = s.slot_index, s.cp, s.start_rb, s.nof_rb, s.row
        k_ref = list(s.k_ref)
        a.nof_k_ref = len(k_ref)
        a.k_ref[:] = (k_ref + [0] * 6)[:6]
        a.symbol_l0, a.symbol_l1, a.cdm, a.freq_density = s.symbol_l0, s.symbol_l1, s.cdm, s.freq_density
        a.scrambling_id, a.amplitude, a.grid_index = s.scrambling_id, float(s.amplitude), s.grid_index
        if s.weights is None:
            wc = np.eye(CSI_RS_ROW_PORTS.get(s.row, 1), dtype=np.complex64)
        else:
            wc = np.asarray(s.weights, np.complex64)
        if wc.ndim != 2 or wc.shape[0] != wc.shape[1]:
            raise SrsGpuError("CSI-RS precoding must be a square (ports, layers) matrix")
        a.nof_ports = wc.shape[0]
        n = min(wc.shape[0], 4)
        w = np.zeros((4, 4, 2), np.float32)
        w[:n, :n, 0], w[:n, :n, 1] = wc.real[:n, :n], wc.imag[:n, :n]
        a.precoding[:] = w.reshape(-1).tolist()
    return arr


class CsiRsPlan(_Handle):
    """srsgpu_csi_rs_plan: every NZP-CSI-RS of a batch of slots generated, precoded and mapped in one launch."""
    _destroy = "srsgpu_csi_rs_plan_destroy"

    def __init__(self, ctx: Context, signals: Sequence[CsiRs], grid_nof_prb: int, grid_nof_ports: int = 4,
                 nof_grids: Optional[int] = None):
        self.ctx = ctx
        self.nof_signals = len(signals)
        if nof_grids is None:
            nof_grids = max([s.grid_index for s in signals], default=0) + 1
        self.nof_grids, self.grid_nof_prb, self.grid_nof_ports = nof_grids, grid_nof_prb, grid_nof_ports
        arr = make_csi_rs_configs(signals)
        self._create("srsgpu_csi_rs_plan_create", ctx.handle, _cptr(arr), len(signals), grid_nof_prb, grid_nof_ports,
                     nof_grids)

    def execute(self, d_grids, stream=None):
        """d_grids: (nof_grids, ports, 14, 12 PRBs) int32 / uint32 words (re | im << 16, bf16). Asynchronous on
        `stream`."""
        _check(_lib().srsgpu_csi_rs_plan_execute(self.handle, _dptr(d_grids), _stream_handle(stream)))


class NzpCsiRsGenerator:
    """GPU counterpart of nzp_csi_rs_generator_impl::map for a list of signals: map_batch() returns the grids as a
    (nof_grids, ports, 14, 12 PRBs) uint32 array (re | im << 16), every RE no signal writes holding `fill`."""

    def __init__(self, ctx: Context, grid_nof_prb: int, grid_nof_ports: int = 4):
        self.ctx, self.grid_nof_prb, self.grid_nof_ports = ctx, grid_nof_prb, grid_nof_ports

    def map_batch(self, signals: Sequence[CsiRs], nof_grids: Optional[int] = None, fill: int = 0) -> np.ndarray:
        dev = torch.device("cuda", self.ctx.device)
        plan = CsiRsPlan(self.ctx, signals, self.grid_nof_prb, self.grid_nof_ports, nof_grids)
        host = np.full((plan.nof_grids, self.grid_nof_ports, 14, 12 * self.grid_nof_prb), fill, np.uint32)
        d_grids = torch.from_numpy(host.view(np.int32)).to(dev)
        plan.execute(d_grids)
        torch.cuda.synchronize(dev)
        plan.close()
        return d_grids.cpu().numpy().view(np.uint32)
