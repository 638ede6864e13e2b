"""PRACH detection (srsgpu_prach_detector_plan)."""
import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from ._abi import Context, torch, _check, _cptr, _dptr, _Handle, _lib, _stream_handle
from .pucch import PucchResult


class PrachOccasionConfig(ctypes.Structure):
    """srsgpu_prach_occasion (include/srsgpu_phy.h): one PRACH occasion with the physical values the detector computes
    with (N_cs, the roots u, threshold and window margin) and where its samples lie in the input."""
    _fields_ = [
        ("format", ctypes.c_uint8),
        ("ra_scs", ctypes.c_uint8),
        ("nof_rx_ports", ctypes.c_uint8),
        ("combine_symbols", ctypes.c_uint8),
        ("n_cs", ctypes.c_uint16),
        ("nof_roots", ctypes.c_uint16),
        ("root_offset", ctypes.c_uint32),
        ("start_preamble_index", ctypes.c_uint8),
        ("nof_preamble_indices", ctypes.c_uint8),
        ("win_margin", ctypes.c_uint16),
        ("threshold", ctypes.c_float),
        ("sample_offset", ctypes.c_uint32),
        ("port_stride", ctypes.c_uint32),
        ("symbol_stride", ctypes.c_uint32),
        ("result_index", ctypes.c_uint32),
    ]


assert ctypes.sizeof(PrachOccasionConfig) == 36
# prach_format_type and prach_subcarrier_spacing, in the reference's order (SRSGPU_PRACH_FORMAT_* / SRSGPU_PRACH_SCS_*).
PRACH_FORMATS = ("0", "1", "2", "3", "A1", "A2", "A3", "B1", "B4", "C0", "C2", "A1/B1", "A2/B2", "A3/B3")
PRACH_SCS_HZ = (15000.0, 30000.0, 60000.0, 120000.0, 1250.0, 5000.0)
# srsgpu_prach_result, 1040 bytes per occasion: the header and 64 preamble slots by preamble index.
PRACH_PREAMBLE_DTYPE = np.dtype([("detected", "<u4"), ("delay_samples", "<u4"), ("metric", "<f4"), ("peak", "<f4")])
PRACH_RESULT_DTYPE = np.dtype([("rssi", "<f4"), ("early_stop", "<u4"), ("reserved", "<u4", (2,)),
                               ("preambles", PRACH_PREAMBLE_DTYPE, (64,))])
assert PRACH_RESULT_DTYPE.itemsize == 1040


@dataclass
class PrachOccasion:
    """One PRACH occasion of srsgpu_prach_detector_plan: prach_detector::configuration with its indices already turned
    into physical values. format: an index into PRACH_FORMATS or its name; ra_scs: an index into PRACH_SCS_HZ; roots: the
    Zadoff-Chu roots u of the occasion's root sequences (64 when n_cs == 0, else ceil(64 / min(64, L // n_cs)));
    sample_offset, port_stride, symbol_stride: words of the input."""
    format: object
    ra_scs: int
    nof_rx_ports: int
    n_cs: int
    roots: Sequence[int]
    threshold: float
    win_margin: int
    sample_offset: int
    port_stride: int
    symbol_stride: int
    start_preamble_index: int = 0
    nof_preamble_indices: int = 64
    combine_symbols: int = 1
    result_index: Optional[int] = None

    @property
    def format_index(self) -> int:
        return PRACH_FORMATS.index(self.format) if isinstance(self.format, str) else int(self.format)

    @property
    def is_long(self) -> bool:
        return self.format_index < 4

    @property
    def sample_rate_hz(self) -> float:
        """N x delta f_RA of the detector's IDFT (1024 points for the long formats, 256 for the short ones)."""
        return (1024 if self.is_long else 256) * PRACH_SCS_HZ[self.ra_scs]


class PrachDetectorPlan(_Handle):
    """srsgpu_prach_detector_plan: every occasion of a batch detected in one launch. Results: one PRACH_RESULT_DTYPE
    record per occasion, at the occasion's result_index (default: its position). Raises SrsGpuError on a refusal."""
    _destroy = "srsgpu_prach_detector_plan_destroy"

    def __init__(self, ctx: Context, occasions: Sequence[PrachOccasion], input_words: int):
        self.ctx = ctx
        self.nof_occasions = len(occasions)
        occ = (PrachOccasionConfig * max(len(occasions), 1))()
        roots = [u for o in occasions for u in o.roots]
        c_roots = (ctypes.c_uint16 * max(len(roots), 1))(*roots)
        at = 0
        for i, (a, o) in enumerate(zip(occ, occasions)):
            a.format, a.ra_scs, a.nof_rx_ports, a.combine_symbols = o.format_index, o.ra_scs, o.nof_rx_ports, o.combine_symbols
            a.n_cs, a.nof_roots, a.root_offset = o.n_cs, len(o.roots), at
            a.start_preamble_index, a.nof_preamble_indices = o.start_preamble_index, o.nof_preamble_indices
            a.win_margin, a.threshold = o.win_margin, o.threshold
            a.sample_offset, a.port_stride, a.symbol_stride = o.sample_offset, o.port_stride, o.symbol_stride
            a.result_index = i if o.result_index is None else o.result_index
            at += len(o.roots)
        self._create("srsgpu_prach_detector_plan_create", ctx.handle, _cptr(occ), len(occasions), _cptr(c_roots),
                     len(roots), input_words)

    def execute(self, d_input, d_results, stream=None):
        """d_input: int32 / uint32 words (re | im << 16, bf16); d_results: device tensor of at least 1040 *
        nof_occasions bytes, every byte of which is written. Asynchronous on `stream`."""
        _check(_lib().srsgpu_prach_detector_plan_execute(self.handle, _dptr(d_input), _dptr(d_results),
                                                         _stream_handle(stream)))


@dataclass
class PrachPreamble:
    """prach_detection_result::preamble_indication, in seconds."""
    preamble_index: int
    time_advance: float
    detection_metric: float


@dataclass
class PrachResult:
    """prach_detection_result of one occasion: times in seconds, the RSSI linear (rssi_dB takes the logarithm)."""
    rssi: float
    time_resolution: float
    time_advance_max: float
    preambles: list

    @property
    def rssi_dB(self):
        return PucchResult._db(self.rssi)


def prach_max_delay_samples(occasion: PrachOccasion) -> int:
    """srsgpu_prach_max_delay_samples: max_delay_samples of prach_detector_generic_impl.cpp:159 for the occasion."""
    out = ctypes.c_uint32()
    _check(_lib().srsgpu_prach_max_delay_samples(occasion.format_index, occasion.ra_scs, occasion.n_cs,
                                                 ctypes.byref(out)))
    return out.value


class PrachDetector:
    """GPU counterpart of prach_detector::detect for a batch of occasions: detect_batch(words, occasions) returns one
    PrachResult per occasion. words: the input as uint32 (re | im << 16, bf16)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def raw_batch(self, words: np.ndarray, occasions: Sequence[PrachOccasion]) -> np.ndarray:
        """The results as a PRACH_RESULT_DTYPE array."""
        dev = torch.device("cuda", self.ctx.device)
        words = np.ascontiguousarray(words).reshape(-1)
        plan = PrachDetectorPlan(self.ctx, occasions, words.size)
        d_input = torch.from_numpy(words.view(np.int32)).to(dev)
        d_results = torch.zeros(PRACH_RESULT_DTYPE.itemsize * max(len(occasions), 1), dtype=torch.uint8, device=dev)
        plan.execute(d_input, d_results)
        torch.cuda.synchronize(dev)
        plan.close()
        return d_results.cpu().numpy().view(PRACH_RESULT_DTYPE)[: len(occasions)]

    def detect_batch(self, words: np.ndarray, occasions: Sequence[PrachOccasion]):
        raw = self.raw_batch(words, occasions)
        out = []
        for i, o in enumerate(occasions):
            r = raw[i if o.result_index is None else o.result_index]
            rate = o.sample_rate_hz
            found = [PrachPreamble(k, float(p["delay_samples"]) / rate, float(p["metric"]))
                     for k, p in enumerate(r["preambles"]) if p["detected"]]
            out.append(PrachResult(float(r["rssi"]), 1.0 / rate, 0.8 * prach_max_delay_samples(o) / rate, found))
        return out
