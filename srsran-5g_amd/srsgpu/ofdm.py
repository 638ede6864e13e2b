"""OFDM modulation and demodulation (srsgpu_ofdm_plan)."""
import ctypes
from typing import Sequence

import numpy as np

from ._abi import Context, torch, _check, _cptr, _dptr, _Handle, _lib, _stream_handle


class OfdmConfig(ctypes.Structure):
    """srsgpu_ofdm_config (include/srsgpu_phy.h): ofdm_modulator_configuration / ofdm_demodulator_configuration."""
    _fields_ = [
        ("numerology", ctypes.c_uint32),
        ("bw_rb", ctypes.c_uint32),
        ("dft_size", ctypes.c_uint32),
        ("cp_extended", ctypes.c_uint32),
        ("nof_samples_window_offset", ctypes.c_uint32),
        ("scale", ctypes.c_float),
        ("center_freq_hz", ctypes.c_double),
    ]


assert ctypes.sizeof(OfdmConfig) == 32


class OfdmPlan(_Handle):
    """srsgpu_ofdm_plan: OFDM slot modulation (inverse=True) or demodulation of nof_grids slots x nof_ports ports.
    Grids: (nof_grids, nof_ports, nsymb, 12 bw_rb) uint32 bf16 pairs; time buffer: nof_samples complex floats (as
    2 * nof_samples float32), slot of (grid, port) at sample_offset(grid, port).
    symbols=(first, count): a symbol-granularity plan of one slot (slot_indices holds one slot index) covering only
    those symbols (srsgpu_ofdm_*_symbols_plan_create; grid rows [port][symbol - first])."""
    _destroy = "srsgpu_ofdm_plan_destroy"

    def __init__(self, ctx: Context, inverse: bool, numerology: int, bw_rb: int, dft_size: int, scale: float,
                 center_freq_hz: float, slot_indices: Sequence[int], nof_ports: int, cp_extended: bool = False,
                 window_offset: int = 0, symbols=None):
        self.ctx, self.inverse = ctx, inverse
        cfg = OfdmConfig(numerology, bw_rb, dft_size, int(cp_extended), window_offset, scale, center_freq_hz)
        kind = "modulator" if inverse else "demodulator"
        if symbols is not None:
            if len(slot_indices) != 1:
                raise ValueError("a symbol-granularity plan covers one slot")
            self._create(f"srsgpu_ofdm_{kind}_symbols_plan_create", ctx.handle, ctypes.byref(cfg), nof_ports,
                         slot_indices[0], symbols[0], symbols[1])
        else:
            slots = (ctypes.c_uint32 * max(len(slot_indices), 1))(*slot_indices)
            self._create(f"srsgpu_ofdm_{kind}_plan_create", ctx.handle, ctypes.byref(cfg), len(slot_indices), nof_ports,
                         _cptr(slots))
        self.nof_grids, self.nof_ports = len(slot_indices), nof_ports
        self.nsymb, self.nsc = (12 if cp_extended else 14), 12 * bw_rb
        if symbols is not None:
            self.nsymb = symbols[1]
        self.nof_samples = int(_lib().srsgpu_ofdm_plan_nof_samples(self.handle))
        self.grid_words = int(_lib().srsgpu_ofdm_plan_nof_grid_words(self.handle))

    @classmethod
    def concat(cls, members: Sequence["OfdmPlan"]) -> "OfdmPlan":
        """srsgpu_ofdm_plan_concat: one plan running the members' jobs (a sector group): member i's grid words and time
        samples follow member i-1's."""
        arr = (ctypes.c_void_p * len(members))(*[m.handle for m in members])
        self = cls.__new__(cls)
        self._create("srsgpu_ofdm_plan_concat", members[0].ctx.handle, _cptr(arr), len(members))
        self.ctx, self.inverse = members[0].ctx, members[0].inverse
        self.nof_grids = sum(m.nof_grids for m in members)
        self.nof_ports, self.nsymb, self.nsc = members[0].nof_ports, members[0].nsymb, members[0].nsc
        self.nof_samples = int(_lib().srsgpu_ofdm_plan_nof_samples(self.handle))
        self.grid_words = int(_lib().srsgpu_ofdm_plan_nof_grid_words(self.handle))
        return self

    def sample_offset(self, grid: int, port: int) -> int:
        return int(_lib().srsgpu_ofdm_plan_sample_offset(self.handle, grid, port))

    OFDM_JOB = np.dtype([("grid_offset", "<u4"), ("sample_offset", "<u4"), ("cp_len", "<u4"), ("reserved", "<u4"),
                         ("coef_re", "<f4"), ("coef_im", "<f4")])

    def jobs(self) -> np.ndarray:
        """srsgpu_ofdm_plan_get_jobs: the plan's (grid, port, symbol) jobs as a structured array (OFDM_JOB)."""
        n = ctypes.c_uint32()
        _check(_lib().srsgpu_ofdm_plan_get_jobs(self.handle, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, self.OFDM_JOB)
        _check(_lib().srsgpu_ofdm_plan_get_jobs(self.handle, out.ctypes.data, n.value, ctypes.byref(n)))
        return out

    def execute_jobs(self, d_jobs, nof_jobs: int, d_in, d_out, stream=None):
        """srsgpu_ofdm_jobs_execute: a caller-assembled job list with this plan's launch parameters."""
        _check(_lib().srsgpu_ofdm_jobs_execute(self.handle, _dptr(d_jobs), nof_jobs, _dptr(d_in), _dptr(d_out),
                                               _stream_handle(stream)))

    OFDM_DIRECT_JOB = np.dtype([("grid", "<u8"), ("samples", "<u8"), ("cp_len", "<u4"), ("coef_re", "<f4"),
                                ("coef_im", "<f4"), ("reserved", "<u4"), ("grid_copy", "<u8")])

    def direct_jobs(self, d_grid, d_samples) -> np.ndarray:
        """The plan's jobs as srsgpu_ofdm_direct_job (OFDM_DIRECT_JOB) over the given grid and sample buffers."""
        j = self.jobs()
        out = np.zeros(len(j), self.OFDM_DIRECT_JOB)
        out["grid"] = _dptr(d_grid) + 4 * j["grid_offset"].astype(np.uint64)
        out["samples"] = _dptr(d_samples) + 8 * j["sample_offset"].astype(np.uint64)
        out["cp_len"], out["coef_re"], out["coef_im"] = j["cp_len"], j["coef_re"], j["coef_im"]
        return out

    def execute_jobs_direct(self, d_jobs, nof_jobs: int, stream=None):
        """srsgpu_ofdm_jobs_execute_direct: direct-address jobs with this plan's launch parameters."""
        _check(_lib().srsgpu_ofdm_jobs_execute_direct(self.handle, _dptr(d_jobs), nof_jobs, _stream_handle(stream)))

    def execute(self, d_in, d_out, stream=None):
        f = _lib().srsgpu_ofdm_modulator_plan_execute if self.inverse else _lib().srsgpu_ofdm_demodulator_plan_execute
        _check(f(self.handle, _dptr(d_in), _dptr(d_out), _stream_handle(stream)))

    def execute_twin(self, d_grid, d_twin, d_samples, stream=None):
        """srsgpu_ofdm_modulator_plan_execute_twin: every RE from d_twin unless it holds 0xffffffff, else from d_grid."""
        _check(_lib().srsgpu_ofdm_modulator_plan_execute_twin(self.handle, _dptr(d_grid), _dptr(d_twin), _dptr(d_samples),
                                                              _stream_handle(stream)))


class OfdmSlotModulator:
    """GPU counterpart of srsran::ofdm_slot_modulator (ofdm_modulator_impl.cpp:115): modulate(grid, slot) takes a
    (nof_ports, nsymb, 12 bw_rb, 2) bf16 grid and returns (nof_ports, slot_size) complex64 samples."""

    def __init__(self, ctx: Context, numerology, bw_rb, dft_size, scale, center_freq_hz, cp_extended=False):
        self.ctx = ctx
        self.args = (numerology, bw_rb, dft_size, scale, center_freq_hz)
        self.cp_extended = cp_extended

    def modulate(self, grid_u16: np.ndarray, slot_index: int) -> np.ndarray:
        P = grid_u16.shape[0]
        plan = OfdmPlan(self.ctx, True, *self.args, [slot_index], P, self.cp_extended)
        dev = torch.device("cuda", self.ctx.device)
        g = np.ascontiguousarray(grid_u16, np.uint16).view(np.int32).reshape(-1)
        d_grid = torch.from_numpy(g.copy()).to(dev)
        d_out = torch.zeros(2 * plan.nof_samples, dtype=torch.float32, device=dev)
        plan.execute(d_grid, d_out)
        torch.cuda.synchronize(dev)
        plan.close()
        return d_out.cpu().numpy().view(np.complex64).reshape(P, -1)


class OfdmSlotDemodulator:
    """GPU counterpart of srsran::ofdm_slot_demodulator (ofdm_demodulator_impl.cpp:154): demodulate(samples, slot)
    takes (nof_ports, slot_size) complex samples and returns the (nof_ports, nsymb, 12 bw_rb, 2) bf16 grid."""

    def __init__(self, ctx: Context, numerology, bw_rb, dft_size, scale, center_freq_hz, cp_extended=False,
                 window_offset=0):
        self.ctx = ctx
        self.args = (numerology, bw_rb, dft_size, scale, center_freq_hz)
        self.cp_extended, self.window_offset = cp_extended, window_offset

    def demodulate(self, samples: np.ndarray, slot_index: int) -> np.ndarray:
        P = samples.shape[0]
        plan = OfdmPlan(self.ctx, False, *self.args, [slot_index], P, self.cp_extended, self.window_offset)
        dev = torch.device("cuda", self.ctx.device)
        x = np.ascontiguousarray(samples, np.complex64).view(np.float32).reshape(-1)
        d_in = torch.from_numpy(x.copy()).to(dev)
        d_grid = torch.zeros(P * plan.nsymb * plan.nsc, dtype=torch.int32, device=dev)
        plan.execute(d_in, d_grid)
        torch.cuda.synchronize(dev)
        plan.close()
        return d_grid.cpu().numpy().view(np.uint16).reshape(P, plan.nsymb, plan.nsc, 2)
