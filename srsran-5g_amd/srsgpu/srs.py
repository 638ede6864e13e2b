"""SRS channel estimation (srsgpu_srs_estimator_plan)."""
import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from ._abi import Context, torch, _check, _cptr, _dptr, _Handle, _lib, _stream_handle


class SrsConfig(ctypes.Structure):
    """srsgpu_srs_config (include/srsgpu_phy.h): one SRS resource with the row of TS 38.211 Table 6.4.1.4.3-1 that its
    C_SRS selects as data, the rx ports to read and where its grid and its result lie."""
    _fields_ = [
        ("m_srs", ctypes.c_uint16 * 4),
        ("N", ctypes.c_uint8 * 4),
        ("numerology", ctypes.c_uint8),
        ("nof_antenna_ports", ctypes.c_uint8),
        ("nof_symbols", ctypes.c_uint8),
        ("start_symbol", ctypes.c_uint8),
        ("comb_size", ctypes.c_uint8),
        ("comb_offset", ctypes.c_uint8),
        ("cyclic_shift", ctypes.c_uint8),
        ("bandwidth_index", ctypes.c_uint8),
        ("freq_hopping", ctypes.c_uint8),
        ("hopping", ctypes.c_uint8),
        ("nof_rx_ports", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8),
        ("rx_ports", ctypes.c_uint8 * 4),
        ("sequence_id", ctypes.c_uint16),
        ("freq_shift", ctypes.c_uint16),
        ("freq_position", ctypes.c_uint16),
        ("reserved2", ctypes.c_uint16),
        ("grid_index", ctypes.c_uint32),
        ("result_index", ctypes.c_uint32),
    ]


assert ctypes.sizeof(SrsConfig) == 44
# srsgpu_srs_result, 192 bytes per resource: channel[rx port index][tx port] as (re, im), times in seconds, powers linear.
SRS_RESULT_DTYPE = np.dtype([("channel", "<f4", (4, 4, 2)), ("time_alignment", "<f8"), ("resolution", "<f8"),
                             ("ta_max", "<f8"), ("epre", "<f4"), ("noise_var", "<f4"), ("ta_idx", "<i4", (4,)),
                             ("reserved", "<u4", (4,))])
assert SRS_RESULT_DTYPE.itemsize == 192


@dataclass
class SrsResource:
    """One SRS resource of srsgpu_srs_estimator_plan: srs_estimator_configuration with C_SRS already turned into its
    row of TS 38.211 Table 6.4.1.4.3-1, table_row = ((m_srs[0], N[0]), ..., (m_srs[3], N[3])), which a binding takes from
    srs_configuration_get(c_srs, b). rx_ports: the grid ports in the order of srs_estimator_configuration::ports.
    freq_hopping is b_hop (default: no hopping); hopping is group_or_sequence_hopping_enum (0: neither)."""
    table_row: Sequence[tuple]
    numerology: int
    nof_antenna_ports: int
    nof_symbols: int
    start_symbol: int
    comb_size: int
    comb_offset: int
    cyclic_shift: int
    sequence_id: int
    bandwidth_index: int
    freq_position: int
    freq_shift: int
    rx_ports: Sequence[int]
    grid_index: int = 0
    freq_hopping: int = 3
    hopping: int = 0
    result_index: Optional[int] = None


class SrsEstimatorPlan(_Handle):
    """srsgpu_srs_estimator_plan: every SRS resource of a batch of slots estimated in one launch. Results: one
    SRS_RESULT_DTYPE record per resource, at the resource's result_index (default: its position). Raises SrsGpuError on
    a refusal."""
    _destroy = "srsgpu_srs_estimator_plan_destroy"

    def __init__(self, ctx: Context, resources: Sequence[SrsResource], grid_nof_prb: int, grid_nof_ports: int = 4,
                 nof_grids: Optional[int] = None):
        self.ctx = ctx
        if nof_grids is None:
            nof_grids = max([r.grid_index for r in resources], default=0) + 1
        self.nof_grids, self.grid_nof_prb, self.grid_nof_ports = nof_grids, grid_nof_prb, grid_nof_ports
        self.nof_resources = len(resources)
        cfg = (SrsConfig * max(len(resources), 1))()
        for i, (a, r) in enumerate(zip(cfg, resources)):
            for b, (m_srs, n_b) in enumerate(list(r.table_row)[:4]):
                a.m_srs[b], a.N[b] = m_srs, n_b
            a.numerology, a.nof_antenna_ports, a.nof_symbols, a.start_symbol = r.numerology, r.nof_antenna_ports, r.nof_symbols, r.start_symbol
            a.comb_size, a.comb_offset, a.cyclic_shift, a.bandwidth_index = r.comb_size, r.comb_offset, r.cyclic_shift, r.bandwidth_index
            a.freq_hopping, a.hopping, a.nof_rx_ports = r.freq_hopping, r.hopping, len(r.rx_ports)
            for k, p in enumerate(list(r.rx_ports)[:4]):
                a.rx_ports[k] = p
            a.sequence_id, a.freq_shift, a.freq_position = r.sequence_id, r.freq_shift, r.freq_position
            a.grid_index = r.grid_index
            a.result_index = i if r.result_index is None else r.result_index
        self._create("srsgpu_srs_estimator_plan_create", ctx.handle, _cptr(cfg), len(resources), grid_nof_prb,
                     grid_nof_ports, nof_grids)

    def execute(self, d_grids, d_results, stream=None):
        """d_grids: (nof_grids, ports, 14, 12 PRBs) int32 / uint32 words (re | im << 16, bf16); d_results: device tensor
        of at least 192 * nof_resources bytes, every byte of which is written. Asynchronous on `stream`."""
        _check(_lib().srsgpu_srs_estimator_plan_execute(self.handle, _dptr(d_grids), _dptr(d_results),
                                                        _stream_handle(stream)))

    def run(self, grids: np.ndarray) -> np.ndarray:
        """Uploads grids, executes once and returns the results as an SRS_RESULT_DTYPE array. The binding that fills
        srs_estimator_result takes epre_dB = 10 log10(epre) and time_alignment.min = -ta_max."""
        dev = torch.device("cuda", self.ctx.device)
        d_grids = torch.from_numpy(np.ascontiguousarray(grids).view(np.int32)).to(dev)
        d_results = torch.zeros(SRS_RESULT_DTYPE.itemsize * max(self.nof_resources, 1), dtype=torch.uint8, device=dev)
        self.execute(d_grids, d_results)
        torch.cuda.synchronize(dev)
        return d_results.cpu().numpy().view(SRS_RESULT_DTYPE)[: self.nof_resources]
