"""PDSCH: the transport-block encoder (srsgpu_pdsch_encoder_plan), the modulator (srsgpu_pdsch_modulator_plan) and the
DM-RS generator (srsgpu_pdsch_dmrs_plan)."""
import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from ._abi import (AllocExtC, Context, RePatternC, torch, _check, _cptr, _dptr, _Handle, _lib, _stage_times,
                   _stream_handle)


class PdschTbConfig(ctypes.Structure):
    """srsgpu_pdsch_tb_config (include/srsgpu_phy.h)."""
    _fields_ = [
        ("base_graph", ctypes.c_uint8),
        ("rv", ctypes.c_uint8),
        ("modulation_order", ctypes.c_uint8),
        ("nof_layers", ctypes.c_uint8),
        ("tbs_bytes", ctypes.c_uint32),
        ("nof_ch_symbols", ctypes.c_uint32),
        ("Nref", ctypes.c_uint32),
        ("tb_offset", ctypes.c_uint32),
        ("cw_offset", ctypes.c_uint32),
    ]


assert ctypes.sizeof(PdschTbConfig) == 24


@dataclass
class PdschTransportBlock:
    """pdsch_encoder::configuration (pdsch_encoder.h) of one transport block."""
    base_graph: int
    rv: int
    modulation_order: int
    nof_layers: int
    nof_ch_symbols: int
    Nref: int = 0


def make_pdsch_configs(tbs_bytes: Sequence[int], tbs: Sequence[PdschTransportBlock]):
    """Packs transport blocks with contiguous TB / codeword (word-aligned) offsets."""
    arr = (PdschTbConfig * len(tbs))()
    to = co = 0
    cw_offsets = []
    for i, (nb, t) in enumerate(zip(tbs_bytes, tbs)):
        a = arr[i]
        a.base_graph, a.rv, a.modulation_order, a.nof_layers = t.base_graph, t.rv, t.modulation_order, t.nof_layers
        a.tbs_bytes, a.nof_ch_symbols, a.Nref, a.tb_offset, a.cw_offset = nb, t.nof_ch_symbols, t.Nref, to, co
        cw_offsets.append(co)
        to += nb
        co += (t.nof_ch_symbols * t.modulation_order + 31) // 32 * 4
    return arr, to, co, cw_offsets


class PdschEncoderPlan(_Handle):
    """srsgpu_pdsch_encoder_plan: TB CRC + segmentation + CB CRC + LDPC + rate matching of a slot's TBs."""
    _destroy = "srsgpu_pdsch_encoder_plan_destroy"

    def __init__(self, ctx: Context, cfg_array):
        self.ctx = ctx
        self._create("srsgpu_pdsch_encoder_plan_create", ctx.handle, _cptr(cfg_array), len(cfg_array))
        self.nof_tbs = len(cfg_array)
        self.nof_codeblocks = int(_lib().srsgpu_pdsch_encoder_plan_nof_codeblocks(self.handle))

    def execute(self, d_tbs, d_codewords, stream=None):
        _check(_lib().srsgpu_pdsch_encoder_plan_execute(self.handle, _dptr(d_tbs), _dptr(d_codewords),
                                                        _stream_handle(stream)))

    def enable_timing(self, enable=True):
        _check(_lib().srsgpu_pdsch_encoder_plan_enable_timing(self.handle, int(enable)))

    def stage_times(self):
        """([ms TB CRC, ms encode], number of executes) accumulated since the previous call."""
        return _stage_times("srsgpu_pdsch_encoder_plan", self.handle, 2)


class PdschEncoder:
    """GPU counterpart of srsran::pdsch_encoder (pdsch_encoder_impl.cpp:28); encode() returns the codeword unpacked
    one bit per byte like the reference."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def encode_batch(self, tbs: Sequence[np.ndarray], cfgs: Sequence[PdschTransportBlock]):
        arr, ntb, ncw, cw_offsets = make_pdsch_configs([t.size for t in tbs], cfgs)
        dev = torch.device("cuda", self.ctx.device)
        d_tbs = torch.from_numpy(np.concatenate([np.asarray(t, np.uint8) for t in tbs])).to(dev)
        d_cw = torch.full((max(ncw, 4),), 0xAB, dtype=torch.uint8, device=dev)
        plan = PdschEncoderPlan(self.ctx, arr)
        plan.execute(d_tbs, d_cw)
        torch.cuda.synchronize(dev)
        plan.close()
        cw = d_cw.cpu().numpy()
        out = []
        for off, c in zip(cw_offsets, cfgs):
            G = c.nof_ch_symbols * c.modulation_order
            out.append(np.unpackbits(cw[off: off + (G + 7) // 8])[:G])
        return out

    def encode(self, tb: np.ndarray, cfg: PdschTransportBlock) -> np.ndarray:
        return self.encode_batch([tb], [cfg])[0]


class PdschModConfig(ctypes.Structure):
    """srsgpu_pdsch_mod_config (include/srsgpu_phy.h): one PDSCH transmission of pdsch_modulator::config_t."""
    _fields_ = [
        ("rnti", ctypes.c_uint16),
        ("n_id", ctypes.c_uint16),
        ("modulation_order", ctypes.c_uint8),
        ("nof_layers", ctypes.c_uint8),
        ("nof_ports", ctypes.c_uint8),
        ("start_symbol", ctypes.c_uint8),
        ("nof_symbols", ctypes.c_uint8),
        ("dmrs_type", ctypes.c_uint8),
        ("nof_cdm_groups_without_data", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8),
        ("dmrs_symbol_mask", ctypes.c_uint16),
        ("bwp_start_rb", ctypes.c_uint16),
        ("bwp_size_rb", ctypes.c_uint16),
        ("rb_start", ctypes.c_uint16),
        ("nof_rb", ctypes.c_uint16),
        ("pad", ctypes.c_uint16),
        ("scaling", ctypes.c_float),
        ("precoding", ctypes.c_float * 32),
        ("cw_offset", ctypes.c_uint32),
        ("nof_bits", ctypes.c_uint32),
        ("grid_index", ctypes.c_uint32),
    ]


assert ctypes.sizeof(PdschModConfig) == 168


@dataclass
class PdschModulation:
    """pdsch_modulator::config_t (pdsch_modulator.h:38) of one transmission: contiguous non-interleaved VRB allocation
    [rb_start, rb_start + nof_rb) of the BWP and wideband precoding `weights` (nof_ports x nof_layers complex), or the
    general form: `crb_mask` (one byte per grid CRB, alloc.vrb_to_crb_mask of any type-0 / type-1 / interleaved
    allocation), `reserved` RE patterns (alloc.ReservedPattern: SSB, CSI-RS, ...) and per-PRG precoding
    (`prg_size` PRBs per PRG, `prg_weights` nof_prg x nof_ports x nof_layers complex)."""
    rnti: int
    n_id: int
    modulation_order: int
    nof_layers: int
    nof_ports: int
    bwp_start_rb: int
    bwp_size_rb: int
    rb_start: int
    nof_rb: int
    start_symbol: int
    nof_symbols: int
    dmrs_symbol_mask: int
    dmrs_type: int
    nof_cdm_groups_without_data: int
    scaling: float
    weights: np.ndarray
    crb_mask: Optional[np.ndarray] = None
    reserved: Sequence = ()
    prg_size: int = 0
    prg_weights: Optional[np.ndarray] = None

    def is_general(self) -> bool:
        return self.crb_mask is not None or len(self.reserved) > 0 or self.prg_size > 0

    def nof_re(self, grid_nof_prb: Optional[int] = None) -> int:
        if self.is_general():
            from . import alloc
            n = grid_nof_prb if grid_nof_prb is not None else self.bwp_start_rb + self.bwp_size_rb
            crbs = self.crb_mask
            if crbs is None:
                crbs = np.zeros(n, np.uint8)
                crbs[self.bwp_start_rb + self.rb_start:self.bwp_start_rb + self.rb_start + self.nof_rb] = 1
            return alloc.count_data_res(n, np.asarray(crbs)[:n], self.start_symbol, self.nof_symbols,
                                        self.dmrs_symbol_mask, self.dmrs_type, self.nof_cdm_groups_without_data,
                                        self.bwp_start_rb, self.bwp_size_rb, self.reserved)
        dm = (4 if self.dmrs_type == 2 else 6) * self.nof_cdm_groups_without_data
        return sum((12 - dm if (self.dmrs_symbol_mask >> l) & 1 else 12) * self.nof_rb
                   for l in range(self.start_symbol, self.start_symbol + self.nof_symbols))


def make_alloc_exts(mods, grid_nof_prb: int):
    """srsgpu_alloc_ext array of the general transmissions (None when every one is contiguous and wideband); the
    returned keep-alive list holds the buffers the structures point to until the plan is created."""
    if not any(m.is_general() for m in mods):
        return None, []
    exts = (AllocExtC * len(mods))()
    keep = []
    for i, m in enumerate(mods):
        if not m.is_general():
            continue
        e = exts[i]
        if m.crb_mask is not None:
            c = np.zeros(grid_nof_prb, np.uint8)
            src = np.asarray(m.crb_mask, np.uint8)[:grid_nof_prb]
            c[:src.size] = src
            keep.append(c)
            e.crb_mask = c.ctypes.data
        if len(m.reserved):
            pats = (RePatternC * len(m.reserved))()
            for j, r in enumerate(m.reserved):
                pats[j].re_mask, pats[j].symbol_mask = r.re_mask, r.symbol_mask
                if r.crb_mask is not None:
                    c = np.zeros(grid_nof_prb, np.uint8)
                    src = np.asarray(r.crb_mask, np.uint8)[:grid_nof_prb]
                    c[:src.size] = src
                    keep.append(c)
                    pats[j].crb_mask = c.ctypes.data
            keep.append(pats)
            e.reserved, e.nof_reserved = _cptr(pats), len(m.reserved)
        if m.prg_size > 0:
            w = np.ascontiguousarray(np.asarray(m.prg_weights, np.complex64).reshape(-1, m.nof_ports, m.nof_layers))
            keep.append(w)
            e.prg_size, e.nof_prg, e.prg_weights = m.prg_size, w.shape[0], w.ctypes.data
    return exts, keep


def make_pdsch_mod_configs(mods: Sequence[PdschModulation], cw_offsets: Sequence[int], grid_index: Sequence[int],
                           grid_nof_prb: Optional[int] = None):
    arr = (PdschModConfig * len(mods))()
    for i, (m, off, g) in enumerate(zip(mods, cw_offsets, grid_index)):
        a = arr[i]
        a.rnti, a.n_id, a.modulation_order, a.nof_layers, a.nof_ports = (m.rnti, m.n_id, m.modulation_order,
                                                                         m.nof_layers, m.nof_ports)
        a.start_symbol, a.nof_symbols, a.dmrs_type = m.start_symbol, m.nof_symbols, m.dmrs_type
        a.nof_cdm_groups_without_data, a.dmrs_symbol_mask = m.nof_cdm_groups_without_data, m.dmrs_symbol_mask
        a.bwp_start_rb, a.bwp_size_rb, a.rb_start, a.nof_rb = m.bwp_start_rb, m.bwp_size_rb, m.rb_start, m.nof_rb
        a.scaling = m.scaling
        w = np.zeros((4, 4, 2), np.float32)
        wc = np.asarray(m.weights, np.complex64).reshape(m.nof_ports, m.nof_layers)
        w[:m.nof_ports, :m.nof_layers, 0] = wc.real
        w[:m.nof_ports, :m.nof_layers, 1] = wc.imag
        a.precoding[:] = w.reshape(-1).tolist()
        a.cw_offset, a.nof_bits, a.grid_index = off, m.nof_re(grid_nof_prb) * m.nof_layers * m.modulation_order, g
    return arr


class PdschModulatorPlan(_Handle):
    """srsgpu_pdsch_modulator_plan: scrambling, modulation, layer mapping, precoding and RE mapping of a batch of
    PDSCH transmissions into bf16 resource grids (grid_nof_ports x 14 x 12 * grid_nof_prb, uint32 re | im << 16)."""
    _destroy = "srsgpu_pdsch_modulator_plan_destroy"

    def __init__(self, ctx: Context, cfg_array, grid_nof_prb: int, grid_nof_ports: int = 4, exts=None):
        self.ctx = ctx
        if exts is None:
            self._create("srsgpu_pdsch_modulator_plan_create", ctx.handle, _cptr(cfg_array), len(cfg_array),
                         grid_nof_prb, grid_nof_ports)
        else:
            self._create("srsgpu_pdsch_modulator_plan_create_ex", ctx.handle, _cptr(cfg_array), _cptr(exts),
                         len(cfg_array), grid_nof_prb, grid_nof_ports)
        self.grid_nof_prb, self.grid_nof_ports = grid_nof_prb, grid_nof_ports

    def grid_elements(self) -> int:
        return self.grid_nof_ports * 14 * 12 * self.grid_nof_prb

    def execute(self, d_codewords, d_grids, stream=None):
        _check(_lib().srsgpu_pdsch_modulator_plan_execute(self.handle, _dptr(d_codewords), _dptr(d_grids),
                                                          _stream_handle(stream)))


class PdschModulator:
    """GPU counterpart of srsran::pdsch_modulator::modulate(grid, codewords, config) (pdsch_modulator_impl.cpp:107):
    modulate() takes the packed codeword and returns the grid as uint16 bf16 bit patterns (ports, 14, nsc, 2), written
    over `grid` (or zeros) at the PDSCH REs only."""

    def __init__(self, ctx: Context, grid_nof_prb: int, grid_nof_ports: int = 4):
        self.ctx, self.grid_nof_prb, self.grid_nof_ports = ctx, grid_nof_prb, grid_nof_ports

    def modulate_batch(self, codewords: Sequence[np.ndarray], mods: Sequence[PdschModulation], grid_index=None,
                       grids: np.ndarray = None):
        dev = torch.device("cuda", self.ctx.device)
        offs, buf, o = [], [], 0
        for cw in codewords:
            b = np.asarray(cw, np.uint8)
            pad = (-b.size) % 4
            buf.append(np.concatenate([b, np.zeros(pad, np.uint8)]))
            offs.append(o)
            o += b.size + pad
        grid_index = list(range(len(mods))) if grid_index is None else list(grid_index)
        ngrids = max(grid_index) + 1 if grid_index else 1
        arr = make_pdsch_mod_configs(mods, offs, grid_index, self.grid_nof_prb)
        exts, _keep = make_alloc_exts(mods, self.grid_nof_prb)
        plan = PdschModulatorPlan(self.ctx, arr, self.grid_nof_prb, self.grid_nof_ports, exts)
        shape = (ngrids, self.grid_nof_ports, 14, 12 * self.grid_nof_prb, 2)
        g0 = np.zeros(shape, np.uint16) if grids is None else np.ascontiguousarray(grids, np.uint16).reshape(shape)
        d_grid = torch.from_numpy(g0.view(np.uint32).reshape(-1).view(np.int32)).to(dev)
        d_cw = torch.from_numpy(np.concatenate(buf) if buf else np.zeros(4, np.uint8)).to(dev)
        plan.execute(d_cw, d_grid)
        torch.cuda.synchronize(dev)
        plan.close()
        return d_grid.cpu().numpy().view(np.uint16).reshape(shape)

    def modulate(self, codeword: np.ndarray, mod: PdschModulation, grid: np.ndarray = None) -> np.ndarray:
        return self.modulate_batch([codeword], [mod], grids=None if grid is None else grid[None])[0]


class PdschDmrsConfig(ctypes.Structure):
    """srsgpu_pdsch_dmrs_config (include/srsgpu_phy.h): dmrs_pdsch_processor::config_t of one transmission."""
    _fields_ = [
        ("slot_index", ctypes.c_uint16),
        ("scrambling_id", ctypes.c_uint16),
        ("n_scid", ctypes.c_uint8),
        ("dmrs_type", ctypes.c_uint8),
        ("nof_layers", ctypes.c_uint8),
        ("nof_ports", ctypes.c_uint8),
        ("dmrs_symbol_mask", ctypes.c_uint16),
        ("reference_point_k_rb", ctypes.c_uint16),
        ("rb_start", ctypes.c_uint16),
        ("nof_rb", ctypes.c_uint16),
        ("amplitude", ctypes.c_float),
        ("precoding", ctypes.c_float * 32),
        ("grid_index", ctypes.c_uint32),
    ]


assert ctypes.sizeof(PdschDmrsConfig) == 152


@dataclass
class PdschDmrs:
    """dmrs_pdsch_processor::config_t (dmrs_pdsch_processor.h:38): contiguous CRB allocation (or `crb_mask`, one byte
    per grid CRB: rb_mask of any type-0 / interleaved allocation), DM-RS ports 0..nof_layers-1, wideband precoding
    weights (nof_ports x nof_layers complex)."""
    slot_index: int
    scrambling_id: int
    n_scid: int
    dmrs_type: int
    nof_layers: int
    nof_ports: int
    dmrs_symbol_mask: int
    reference_point_k_rb: int
    rb_start: int
    nof_rb: int
    amplitude: float
    weights: np.ndarray
    crb_mask: Optional[np.ndarray] = None

    def is_general(self) -> bool:
        return self.crb_mask is not None


def make_pdsch_dmrs_configs(dmrs: Sequence[PdschDmrs], grid_index: Sequence[int]):
    arr = (PdschDmrsConfig * len(dmrs))()
    for i, (m, g) in enumerate(zip(dmrs, grid_index)):
        a = arr[i]
        a.slot_index, a.scrambling_id, a.n_scid, a.dmrs_type = m.slot_index, m.scrambling_id, m.n_scid, m.dmrs_type
        a.nof_layers, a.nof_ports, a.dmrs_symbol_mask = m.nof_layers, m.nof_ports, m.dmrs_symbol_mask
        a.reference_point_k_rb, a.rb_start, a.nof_rb, a.amplitude = (m.reference_point_k_rb, m.rb_start, m.nof_rb,
                                                                      m.amplitude)
        w = np.zeros((4, 4, 2), np.float32)
        wc = np.asarray(m.weights, np.complex64).reshape(m.nof_ports, m.nof_layers)
        w[:m.nof_ports, :m.nof_layers, 0] = wc.real
        w[:m.nof_ports, :m.nof_layers, 1] = wc.imag
        a.precoding[:] = w.reshape(-1).tolist()
        a.grid_index = g
    return arr


class PdschDmrsPlan(_Handle):
    """srsgpu_pdsch_dmrs_plan: PDSCH DM-RS generation, cover codes, precoding and mapping into bf16 grids."""
    _destroy = "srsgpu_pdsch_dmrs_plan_destroy"

    def __init__(self, ctx: Context, cfg_array, grid_nof_prb: int, grid_nof_ports: int = 4, exts=None):
        self.ctx = ctx
        if exts is None:
            self._create("srsgpu_pdsch_dmrs_plan_create", ctx.handle, _cptr(cfg_array), len(cfg_array), grid_nof_prb,
                         grid_nof_ports)
        else:
            self._create("srsgpu_pdsch_dmrs_plan_create_ex", ctx.handle, _cptr(cfg_array), _cptr(exts),
                         len(cfg_array), grid_nof_prb, grid_nof_ports)

    def execute(self, d_grids, stream=None):
        _check(_lib().srsgpu_pdsch_dmrs_plan_execute(self.handle, _dptr(d_grids), _stream_handle(stream)))
