"""PUCCH: Formats 0 and 1 (srsgpu_pucch_detector_plan), Format 2 (srsgpu_pucch_f2_plan) and Formats 3 and 4
(srsgpu_pucch_f34_plan), the latter two with the UCI decoders behind them."""
import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from ._abi import Context, torch, _check, _cptr, _dptr, _Handle, _lib, _stream_handle
from .uci import uci_polar_unpack, UciDecoderPlan, UciPolarDecoderPlan


class PucchF0Config(ctypes.Structure):
    """srsgpu_pucch_f0_config (include/srsgpu_phy.h): pucch_detector::format0_configuration of one PDU (PRBs already
    offset by the BWP start; second_hop_prb 0xffff = no hopping) and the grid it is read from."""
    _fields_ = [
        ("slot_index", ctypes.c_uint16),
        ("numerology", ctypes.c_uint8),
        ("cp_extended", ctypes.c_uint8),
        ("starting_prb", ctypes.c_uint16),
        ("second_hop_prb", ctypes.c_uint16),
        ("start_symbol_index", ctypes.c_uint8),
        ("nof_symbols", ctypes.c_uint8),
        ("initial_cyclic_shift", ctypes.c_uint8),
        ("nof_harq_ack", ctypes.c_uint8),
        ("n_id", ctypes.c_uint16),
        ("sr_opportunity", ctypes.c_uint8),
        ("nof_ports", ctypes.c_uint8),
        ("ports", ctypes.c_uint8 * 4),
        ("grid_index", ctypes.c_uint32),
    ]


class PucchF1Resource(ctypes.Structure):
    """srsgpu_pucch_f1_resource: the common configuration of the PUCCHs multiplexed on one PRB (two with hopping)."""
    _fields_ = [
        ("slot_index", ctypes.c_uint16),
        ("numerology", ctypes.c_uint8),
        ("cp_extended", ctypes.c_uint8),
        ("starting_prb", ctypes.c_uint16),
        ("second_hop_prb", ctypes.c_uint16),
        ("start_symbol_index", ctypes.c_uint8),
        ("nof_symbols", ctypes.c_uint8),
        ("n_id", ctypes.c_uint16),
        ("nof_rx_ports", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 3),
        ("grid_index", ctypes.c_uint32),
        ("first_entry", ctypes.c_uint32),
        ("nof_entries", ctypes.c_uint32),
    ]


class PucchF1Entry(ctypes.Structure):
    """srsgpu_pucch_f1_entry: one multiplexed PUCCH of a resource (an element of pucch_format1_map<unsigned>)."""
    _fields_ = [
        ("initial_cyclic_shift", ctypes.c_uint8),
        ("time_domain_occ", ctypes.c_uint8),
        ("nof_harq_ack", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8),
    ]


assert ctypes.sizeof(PucchF0Config) == 24 and ctypes.sizeof(PucchF1Resource) == 28 and ctypes.sizeof(PucchF1Entry) == 4
PUCCH_NO_HOP = 0xffff
# srsgpu_pucch_result, 32 bytes: one per Format 0 PDU, then one per Format 1 entry.
PUCCH_RESULT_DTYPE = np.dtype([("sr", "u1"), ("harq_ack", "u1", (2,)), ("status", "u1"), ("detection_metric", "<f4"),
                               ("epre", "<f4"), ("rsrp", "<f4"), ("noise_var", "<f4"), ("reserved", "<u4", (3,))])
assert PUCCH_RESULT_DTYPE.itemsize == 32


@dataclass
class PucchF0:
    """pucch_detector::format0_configuration (pucch_detector.h) of one PDU: grid PRBs (the BWP start added), second_hop_prb
    None without hopping, and `ports` the grid ports to read, in order."""
    slot_index: int
    starting_prb: int
    start_symbol_index: int
    nof_symbols: int
    initial_cyclic_shift: int
    n_id: int
    nof_harq_ack: int
    sr_opportunity: int
    ports: Sequence[int] = (0,)
    second_hop_prb: Optional[int] = None
    numerology: int = 1
    cp_extended: int = 0
    grid_index: int = 0


@dataclass
class PucchF1:
    """pucch_detector::format1_configuration of one resource with its multiplexed PUCCHs: entries = [(initial cyclic
    shift, time-domain OCC, nof_harq_ack)], nof_harq_ack 0 meaning SR only. Grid ports 0..nof_rx_ports-1 are read."""
    slot_index: int
    starting_prb: int
    start_symbol_index: int
    nof_symbols: int
    n_id: int
    nof_rx_ports: int
    entries: Sequence[tuple] = ()
    second_hop_prb: Optional[int] = None
    numerology: int = 1
    cp_extended: int = 0
    grid_index: int = 0


def make_pucch_configs(f0_pdus: Sequence[PucchF0], f1_resources: Sequence[PucchF1]):
    """The three C arrays of srsgpu_pucch_detector_plan_create; the entries of the resources follow one another."""
    f0 = (PucchF0Config * max(len(f0_pdus), 1))()
    for a, d in zip(f0, f0_pdus):
        a.slot_index, a.numerology, a.cp_extended = d.slot_index, d.numerology, d.cp_extended
        a.starting_prb = d.starting_prb
        a.second_hop_prb = PUCCH_NO_HOP if d.second_hop_prb is None else d.second_hop_prb
        a.start_symbol_index, a.nof_symbols, a.initial_cyclic_shift = d.start_symbol_index, d.nof_symbols, d.initial_cyclic_shift
        a.nof_harq_ack, a.n_id, a.sr_opportunity = d.nof_harq_ack, d.n_id, d.sr_opportunity
        a.nof_ports = len(d.ports)
        for i, p in enumerate(list(d.ports)[:4]):
            a.ports[i] = p
        a.grid_index = d.grid_index
    nof_entries = sum(len(r.entries) for r in f1_resources)
    f1 = (PucchF1Resource * max(len(f1_resources), 1))()
    ent = (PucchF1Entry * max(nof_entries, 1))()
    first = 0
    for a, r in zip(f1, f1_resources):
        a.slot_index, a.numerology, a.cp_extended = r.slot_index, r.numerology, r.cp_extended
        a.starting_prb = r.starting_prb
        a.second_hop_prb = PUCCH_NO_HOP if r.second_hop_prb is None else r.second_hop_prb
        a.start_symbol_index, a.nof_symbols, a.n_id, a.nof_rx_ports = r.start_symbol_index, r.nof_symbols, r.n_id, r.nof_rx_ports
        a.grid_index, a.first_entry, a.nof_entries = r.grid_index, first, len(r.entries)
        for i, (ics, occ, nof_harq_ack) in enumerate(r.entries):
            e = ent[first + i]
            e.initial_cyclic_shift, e.time_domain_occ, e.nof_harq_ack = ics, occ, nof_harq_ack
        first += len(r.entries)
    return f0, f1, ent, nof_entries


class PucchDetectorPlan(_Handle):
    """srsgpu_pucch_detector_plan: every Format 0 PDU and every Format 1 resource of a batch of slots detected in one
    launch. Results: nof_f0 + (all entries) records of PUCCH_RESULT_DTYPE, the Format 0 PDUs first, then the entries of
    the resources in order. Raises SrsGpuError on a refusal."""
    _destroy = "srsgpu_pucch_detector_plan_destroy"

    def __init__(self, ctx: Context, f0_pdus: Sequence[PucchF0], f1_resources: Sequence[PucchF1], grid_nof_prb: int,
                 grid_nof_ports: int = 4, nof_grids: Optional[int] = None):
        self.ctx = ctx
        if nof_grids is None:
            nof_grids = max([d.grid_index for d in list(f0_pdus) + list(f1_resources)], default=0) + 1
        self.nof_grids, self.grid_nof_prb, self.grid_nof_ports = nof_grids, grid_nof_prb, grid_nof_ports
        f0, f1, ent, nof_entries = make_pucch_configs(f0_pdus, f1_resources)
        self.nof_f0, self.nof_entries = len(f0_pdus), nof_entries
        self.nof_results = self.nof_f0 + nof_entries
        self._create("srsgpu_pucch_detector_plan_create", ctx.handle, _cptr(f0), len(f0_pdus), _cptr(f1),
                     len(f1_resources), _cptr(ent), nof_entries, grid_nof_prb, grid_nof_ports, nof_grids)

    def execute(self, d_grids, d_results, stream=None):
        """d_grids: (nof_grids, ports, 14, 12 PRBs) int32 / uint32 words (re | im << 16, bf16); d_results: device tensor
        of at least 32 * nof_results bytes. Asynchronous on `stream`."""
        _check(_lib().srsgpu_pucch_detector_plan_execute(self.handle, _dptr(d_grids), _dptr(d_results),
                                                         _stream_handle(stream)))


@dataclass
class PucchResult:
    """pucch_processor_result of one PUCCH: the message (sr and harq_ack bits, status True = uci_status::valid), the
    detection metric (Format 1: over its threshold, as the reference reports it) and the linear channel state."""
    sr: int
    harq_ack: tuple
    valid: bool
    detection_metric: float
    epre: float
    rsrp: float
    noise_var: float

    @staticmethod
    def _db(v):
        return float(10.0 * np.log10(v)) if v > 0 else float("-inf") if v == 0 else float("nan")

    @property
    def epre_dB(self):
        return self._db(self.epre)

    @property
    def rsrp_dB(self):
        return self._db(self.rsrp)


class PucchDetector:
    """GPU counterpart of pucch_processor::process for Format 0 PDUs and Format 1 batches: process_batch(grids, f0_pdus,
    f1_resources) returns ([PucchResult per PDU], [[PucchResult per entry] per resource]). grids: (nof_grids, ports,
    14, 12 PRBs) uint32 (re | im << 16, bf16)."""

    def __init__(self, ctx: Context, grid_nof_prb: int, grid_nof_ports: int = 4):
        self.ctx, self.grid_nof_prb, self.grid_nof_ports = ctx, grid_nof_prb, grid_nof_ports

    def raw_batch(self, grids: np.ndarray, f0_pdus: Sequence[PucchF0], f1_resources: Sequence[PucchF1]) -> np.ndarray:
        """The results as a PUCCH_RESULT_DTYPE array."""
        dev = torch.device("cuda", self.ctx.device)
        plan = PucchDetectorPlan(self.ctx, f0_pdus, f1_resources, self.grid_nof_prb, self.grid_nof_ports, grids.shape[0])
        d_grids = torch.from_numpy(np.ascontiguousarray(grids).view(np.int32)).to(dev)
        d_results = torch.zeros(32 * max(plan.nof_results, 1), dtype=torch.uint8, device=dev)
        plan.execute(d_grids, d_results)
        torch.cuda.synchronize(dev)
        plan.close()
        return d_results.cpu().numpy().view(PUCCH_RESULT_DTYPE)[: plan.nof_results]

    def process_batch(self, grids, f0_pdus: Sequence[PucchF0], f1_resources: Sequence[PucchF1]):
        raw = self.raw_batch(grids, f0_pdus, f1_resources)

        def one(r, nof_harq_ack):
            return PucchResult(int(r["sr"]), tuple(int(b) for b in r["harq_ack"][:nof_harq_ack]), bool(r["status"]),
                               float(r["detection_metric"]), float(r["epre"]), float(r["rsrp"]), float(r["noise_var"]))
        f0_out = [one(raw[i], d.nof_harq_ack) for i, d in enumerate(f0_pdus)]
        f1_out, at = [], len(f0_pdus)
        for r in f1_resources:
            f1_out.append([one(raw[at + i], e[2]) for i, e in enumerate(r.entries)])
            at += len(r.entries)
        return f0_out, f1_out


class PucchF2Config(ctypes.Structure):
    """srsgpu_pucch_f2_config (include/srsgpu_phy.h): one PUCCH Format 2 PDU, PRBs as grid PRBs, second_hop_prb
    PUCCH_NO_HOP without hopping, where its grid lies and where its 16 nof_prb nof_symbols LLRs go."""
    _fields_ = [
        ("slot_index", ctypes.c_uint16),
        ("numerology", ctypes.c_uint8),
        ("cp_extended", ctypes.c_uint8),
        ("starting_prb", ctypes.c_uint16),
        ("second_hop_prb", ctypes.c_uint16),
        ("nof_prb", ctypes.c_uint8),
        ("start_symbol_index", ctypes.c_uint8),
        ("nof_symbols", ctypes.c_uint8),
        ("nof_ports", ctypes.c_uint8),
        ("rnti", ctypes.c_uint16),
        ("n_id", ctypes.c_uint16),
        ("n_id_0", ctypes.c_uint16),
        ("nof_uci_bits", ctypes.c_uint16),
        ("ports", ctypes.c_uint8 * 4),
        ("grid_index", ctypes.c_uint32),
        ("llr_offset", ctypes.c_uint32),
    ]


assert ctypes.sizeof(PucchF2Config) == 32
# srsgpu_pucch_f2_result, 96 bytes per PDU: per listed port, powers linear, time alignment in seconds, CFO in Hz (NaN
# when no hop has two symbols).
PUCCH_F2_RESULT_DTYPE = np.dtype([("noise_var", "<f4", (4,)), ("rsrp", "<f4", (4,)), ("epre", "<f4", (4,)),
                                  ("cfo_hz", "<f4", (4,)), ("time_alignment", "<f8", (4,))])
assert PUCCH_F2_RESULT_DTYPE.itemsize == 96


@dataclass
class PucchF2:
    """pucch_processor::format2_configuration of one PDU: grid PRBs (the BWP start added), second_hop_prb None without
    hopping, `ports` the grid ports in order, and the payload as its three fields (CSI Part 2 is refused by the
    reference). llr_offset None: the PDUs' LLRs follow one another."""
    slot_index: int
    starting_prb: int
    nof_prb: int
    start_symbol_index: int
    nof_symbols: int
    rnti: int
    n_id: int
    n_id_0: int
    nof_harq_ack: int = 0
    nof_sr: int = 0
    nof_csi_part1: int = 0
    ports: Sequence[int] = (0,)
    second_hop_prb: Optional[int] = None
    numerology: int = 1
    cp_extended: int = 0
    grid_index: int = 0
    llr_offset: Optional[int] = None

    @property
    def nof_uci_bits(self) -> int:
        return self.nof_harq_ack + self.nof_sr + self.nof_csi_part1

    @property
    def nof_llrs(self) -> int:
        return 16 * self.nof_prb * self.nof_symbols


def make_pucch_f2_configs(pdus: Sequence[PucchF2]):
    """The C array of srsgpu_pucch_f2_plan_create and the LLR offsets used (a PDU without one follows the PDU before
    it; 16 nof_prb nof_symbols is a multiple of 4)."""
    cfg = (PucchF2Config * max(len(pdus), 1))()
    offsets, o = [], 0
    for a, d in zip(cfg, pdus):
        a.slot_index, a.numerology, a.cp_extended = d.slot_index, d.numerology, d.cp_extended
        a.starting_prb = d.starting_prb
        a.second_hop_prb = PUCCH_NO_HOP if d.second_hop_prb is None else d.second_hop_prb
        a.nof_prb, a.start_symbol_index, a.nof_symbols, a.nof_ports = d.nof_prb, d.start_symbol_index, d.nof_symbols, len(d.ports)
        a.rnti, a.n_id, a.n_id_0, a.nof_uci_bits = d.rnti, d.n_id, d.n_id_0, d.nof_uci_bits
        for i, p in enumerate(list(d.ports)[:4]):
            a.ports[i] = p
        a.grid_index = d.grid_index
        a.llr_offset = o if d.llr_offset is None else d.llr_offset
        offsets.append(int(a.llr_offset))
        o = int(a.llr_offset) + max(d.nof_llrs, 0)
    return cfg, offsets


class PucchF2Plan(_Handle):
    """srsgpu_pucch_f2_plan: estimation, equalisation, demapping and descrambling of every Format 2 PDU of a batch of
    slots in one launch. Results: one PUCCH_F2_RESULT_DTYPE record per PDU. Raises SrsGpuError on a refusal."""
    _destroy = "srsgpu_pucch_f2_plan_destroy"

    def __init__(self, ctx: Context, pdus: Sequence[PucchF2], grid_nof_prb: int, grid_nof_ports: int = 4,
                 nof_grids: Optional[int] = None):
        self.ctx = ctx
        if nof_grids is None:
            nof_grids = max([d.grid_index for d in pdus], default=0) + 1
        self.nof_grids, self.grid_nof_prb, self.grid_nof_ports = nof_grids, grid_nof_prb, grid_nof_ports
        cfg, self.llr_offsets = make_pucch_f2_configs(pdus)
        self.nof_pdus = len(pdus)
        self.nof_llrs = max([o + d.nof_llrs for o, d in zip(self.llr_offsets, pdus)], default=0)
        self._create("srsgpu_pucch_f2_plan_create", ctx.handle, _cptr(cfg), len(pdus), grid_nof_prb, grid_nof_ports,
                     nof_grids)

    def execute(self, d_grids, d_llrs, d_results, stream=None):
        """d_grids: (nof_grids, ports, 14, 12 PRBs) int32 / uint32 words (re | im << 16, bf16); d_llrs: int8, at least
        nof_llrs entries, written only inside the PDUs' ranges; d_results: at least 96 * nof_pdus bytes, every byte of
        which is written. Asynchronous on `stream`."""
        _check(_lib().srsgpu_pucch_f2_plan_execute(self.handle, _dptr(d_grids), _dptr(d_llrs), _dptr(d_results),
                                                   _stream_handle(stream)))


@dataclass
class PucchF2Result:
    """pucch_processor_result of one Format 2 PDU: the payload split in the reference's order (HARQ-ACK, SR, CSI
    Part 1), the status (True = uci_status::valid) and the channel state, per port (linear, seconds, Hz) and combined as
    channel_estimate::get_channel_state_information combines it (dB; cfo_hz NaN when no hop has two symbols)."""
    harq_ack: np.ndarray
    sr: np.ndarray
    csi_part1: np.ndarray
    valid: bool
    noise_var: np.ndarray
    rsrp: np.ndarray
    epre: np.ndarray
    time_alignment_ports: np.ndarray
    cfo_hz_ports: np.ndarray
    epre_dB: float
    rsrp_dB: float
    sinr_dB: float
    time_alignment: float
    cfo_hz: float

    @property
    def payload(self) -> np.ndarray:
        return np.concatenate([self.harq_ack, self.sr, self.csi_part1]).astype(np.uint8)


class PucchF2Batch:
    """The three plans of a batch of Format 2 PDUs with their device buffers: launch(d_grids) enqueues the front end,
    the short-block decoder (payloads of 3..11 bits, Qm 2) and the polar decoder (12 bits and more; E <= 512 never
    reaches two codeblocks) on one stream, both decoders reading source 0 at the PDUs' LLR offsets; results() reads
    them back. Allocation-free between the two, so launch() can be captured in a graph."""

    def __init__(self, ctx: Context, pdus: Sequence[PucchF2], grid_nof_prb: int, grid_nof_ports: int = 4,
                 nof_grids: Optional[int] = None):
        self.ctx, self.pdus = ctx, list(pdus)
        dev = torch.device("cuda", ctx.device)
        self.front = PucchF2Plan(ctx, self.pdus, grid_nof_prb, grid_nof_ports, nof_grids)
        offs = self.front.llr_offsets
        self.short_ids = [i for i, d in enumerate(self.pdus) if d.nof_uci_bits <= 11]
        self.polar_ids = [i for i, d in enumerate(self.pdus) if d.nof_uci_bits >= 12]
        self.short = UciDecoderPlan(ctx, [(self.pdus[i].nof_uci_bits, 2, 0, self.pdus[i].nof_llrs, offs[i])
                                          for i in self.short_ids]) if self.short_ids else None
        self.polar = UciPolarDecoderPlan(ctx, [(self.pdus[i].nof_uci_bits, 0, self.pdus[i].nof_llrs, offs[i], None)
                                               for i in self.polar_ids]) if self.polar_ids else None
        self.d_llrs = torch.zeros(self.front.nof_llrs + 4, dtype=torch.int8, device=dev)
        self.d_results = torch.zeros(PUCCH_F2_RESULT_DTYPE.itemsize * max(len(self.pdus), 1), dtype=torch.uint8, device=dev)
        self.d_short_msgs = torch.zeros(max(len(self.short_ids), 1), dtype=torch.int16, device=dev)
        self.d_short_status = torch.zeros(max(len(self.short_ids), 1), dtype=torch.uint8, device=dev)
        self.d_polar_msgs = torch.zeros(max(self.polar.nof_msg_words if self.polar else 0, 1), dtype=torch.int32, device=dev)
        self.d_polar_status = torch.zeros(max(len(self.polar_ids), 1), dtype=torch.uint8, device=dev)

    def launch(self, d_grids, stream=None):
        self.front.execute(d_grids, self.d_llrs, self.d_results, stream)
        if self.short is not None:
            self.short.execute(self.d_llrs, None, None, self.d_short_msgs, self.d_short_status, stream)
        if self.polar is not None:
            self.polar.execute(self.d_llrs, None, None, self.d_polar_msgs, self.d_polar_status, stream)

    def raw(self):
        """(LLRs int8, PUCCH_F2_RESULT_DTYPE records) as the front end left them."""
        return (self.d_llrs.cpu().numpy()[: self.front.nof_llrs],
                self.d_results.cpu().numpy().view(PUCCH_F2_RESULT_DTYPE)[: len(self.pdus)])

    def results(self):
        _, raw = self.raw()
        bits, valid = [None] * len(self.pdus), [False] * len(self.pdus)
        if self.short is not None:
            msgs, status = self.d_short_msgs.cpu().numpy().view(np.uint16), self.d_short_status.cpu().numpy()
            for k, i in enumerate(self.short_ids):
                a = self.pdus[i].nof_uci_bits
                bits[i], valid[i] = ((int(msgs[k]) >> np.arange(a)) & 1).astype(np.uint8), bool(status[k])
        if self.polar is not None:
            words, status = self.d_polar_msgs.cpu().numpy().view(np.uint32), self.d_polar_status.cpu().numpy()
            for k, i in enumerate(self.polar_ids):
                bits[i] = uci_polar_unpack(words, self.polar.msg_word_offsets[k], self.pdus[i].nof_uci_bits)
                valid[i] = bool(status[k])
        return [pucch_f2_result(d, b, v, r) for d, b, v, r in zip(self.pdus, bits, valid, raw)]

    def close(self):
        for plan in (self.front, self.short, self.polar):
            if plan is not None:
                plan.close()


def _power_db(v):
    v = float(v)
    return float(10.0 * np.log10(v)) if v > 0 else float("-inf") if v == 0 else float("nan")


def pucch_f2_result(pdu: PucchF2, bits, valid, record) -> PucchF2Result:
    """One PUCCH_F2_RESULT_DTYPE record and the decoded payload as a PucchF2Result: the payload split into HARQ-ACK,
    SR and CSI Part 1, and the ports combined as channel_estimate::get_channel_state_information does (mean EPRE and
    RSRP; time alignment and CFO of the port with the best RSRP / noise variance, the first unless another is strictly
    better, 1000 standing for a zero noise variance; SINR from the summed RSRP over the summed noise variance, 60 dB
    when that sum is no normal number). The dB conversion happens here, on the host."""
    P = len(pdu.ports)
    nv, rsrp, epre = (np.asarray(record[k][:P], np.float32) for k in ("noise_var", "rsrp", "epre"))
    ta, cfo = np.asarray(record["time_alignment"][:P]), np.asarray(record["cfo_hz"][:P])
    best, best_snr = 0, np.float32(0)
    for i in range(P):
        snr = rsrp[i] / nv[i] if nv[i] != 0 else np.float32(1000)
        if snr > best_snr:
            best, best_snr = i, snr
    nsum = np.float32(nv.sum(dtype=np.float32))
    normal = np.isfinite(nsum) and abs(nsum) >= np.finfo(np.float32).tiny
    sinr = float(rsrp.sum(dtype=np.float32) / nsum) if normal else 1e6
    b = np.asarray(bits, np.uint8)
    h, s = pdu.nof_harq_ack, pdu.nof_harq_ack + pdu.nof_sr
    return PucchF2Result(b[:h], b[h:s], b[s:], bool(valid), nv, rsrp, epre, ta, cfo,
                         _power_db(epre.mean(dtype=np.float32)), _power_db(rsrp.mean(dtype=np.float32)), _power_db(sinr),
                         float(ta[best]), float(cfo[best]))


class PucchF2Processor:
    """GPU counterpart of pucch_processor::process(grid, format2_configuration) (pucch_processor_impl.cpp:145) for a
    batch: process_batch(grids, pdus) returns one PucchF2Result per PDU. grids: (nof_grids, ports, 14, 12 PRBs) uint32
    (re | im << 16, bf16)."""

    def __init__(self, ctx: Context, grid_nof_prb: int, grid_nof_ports: int = 4):
        self.ctx, self.grid_nof_prb, self.grid_nof_ports = ctx, grid_nof_prb, grid_nof_ports

    def process_batch(self, grids: np.ndarray, pdus: Sequence[PucchF2]):
        dev = torch.device("cuda", self.ctx.device)
        batch = PucchF2Batch(self.ctx, pdus, self.grid_nof_prb, self.grid_nof_ports, grids.shape[0])
        d_grids = torch.from_numpy(np.ascontiguousarray(grids).view(np.int32)).to(dev)
        batch.launch(d_grids)
        torch.cuda.synchronize(dev)
        out = batch.results()
        batch.close()
        return out


class PucchF34Config(ctypes.Structure):
    """srsgpu_pucch_f34_config (include/srsgpu_phy.h): one PUCCH Format 3 or 4 PDU, PRBs as grid PRBs, second_hop_prb
    PUCCH_NO_HOP without hopping, where its grid lies and where its E LLRs go."""
    _fields_ = [
        ("slot_index", ctypes.c_uint16),
        ("format", ctypes.c_uint8),
        ("numerology", ctypes.c_uint8),
        ("cp_extended", ctypes.c_uint8),
        ("nof_prb", ctypes.c_uint8),
        ("start_symbol_index", ctypes.c_uint8),
        ("nof_symbols", ctypes.c_uint8),
        ("starting_prb", ctypes.c_uint16),
        ("second_hop_prb", ctypes.c_uint16),
        ("additional_dmrs", ctypes.c_uint8),
        ("pi2_bpsk", ctypes.c_uint8),
        ("occ_length", ctypes.c_uint8),
        ("occ_index", ctypes.c_uint8),
        ("rnti", ctypes.c_uint16),
        ("n_id_scrambling", ctypes.c_uint16),
        ("n_id_hopping", ctypes.c_uint16),
        ("nof_uci_bits", ctypes.c_uint16),
        ("nof_ports", ctypes.c_uint8),
        ("ports", ctypes.c_uint8 * 4),
        ("reserved", ctypes.c_uint8 * 3),
        ("grid_index", ctypes.c_uint32),
        ("llr_offset", ctypes.c_uint32),
    ]


assert ctypes.sizeof(PucchF34Config) == 40


def pucch_f34_dmrs_symbols(nof_symbols: int, hopping: bool, additional_dmrs: bool):
    """TS 38.211 Table 6.4.1.3.3.2-1: the allocated symbols (0 = the first) of a Format 3 / 4 PDU that carry DM-RS."""
    if nof_symbols == 4:
        return (0, 2) if hopping else (1,)
    two = {5: (0, 3), 6: (1, 4), 7: (1, 4), 8: (1, 5), 9: (1, 6), 10: (2, 7), 11: (2, 7), 12: (2, 8), 13: (2, 9),
           14: (3, 10)}
    four = {10: (1, 3, 6, 8), 11: (1, 3, 6, 9), 12: (1, 4, 7, 10), 13: (1, 4, 7, 11), 14: (1, 5, 8, 12)}
    if additional_dmrs and nof_symbols in four:
        return four[nof_symbols]
    return two.get(nof_symbols, ())


@dataclass
class PucchF3:
    """pucch_processor::format3_configuration of one PDU: grid PRBs (the BWP start added), second_hop_prb None without
    hopping, `ports` the grid ports in order, and the payload as its three fields (CSI Part 2 is refused by the
    reference). llr_offset None: the PDU's LLRs follow the PDU before it at the next multiple of 4."""
    slot_index: int
    starting_prb: int
    nof_prb: int
    start_symbol_index: int
    nof_symbols: int
    rnti: int
    n_id_scrambling: int
    n_id_hopping: int
    nof_harq_ack: int = 0
    nof_sr: int = 0
    nof_csi_part1: int = 0
    ports: Sequence[int] = (0,)
    second_hop_prb: Optional[int] = None
    additional_dmrs: bool = False
    pi2_bpsk: bool = False
    numerology: int = 1
    cp_extended: int = 0
    grid_index: int = 0
    llr_offset: Optional[int] = None
    format = 3
    occ_length = 0
    occ_index = 0

    @property
    def nof_uci_bits(self) -> int:
        return self.nof_harq_ack + self.nof_sr + self.nof_csi_part1

    @property
    def modulation_order(self) -> int:
        return 1 if self.pi2_bpsk else 2

    @property
    def nof_data_symbols(self) -> int:
        return self.nof_symbols - len(pucch_f34_dmrs_symbols(self.nof_symbols, self.second_hop_prb is not None,
                                                             self.additional_dmrs))

    @property
    def nof_llrs(self) -> int:
        return 12 * self.nof_prb * self.nof_data_symbols * self.modulation_order


@dataclass
class PucchF4:
    """pucch_processor::format4_configuration of one PDU (one PRB); see PucchF3. occ_length is the spreading factor."""
    slot_index: int
    starting_prb: int
    start_symbol_index: int
    nof_symbols: int
    rnti: int
    n_id_scrambling: int
    n_id_hopping: int
    occ_length: int
    occ_index: int
    nof_harq_ack: int = 0
    nof_sr: int = 0
    nof_csi_part1: int = 0
    ports: Sequence[int] = (0,)
    second_hop_prb: Optional[int] = None
    additional_dmrs: bool = False
    pi2_bpsk: bool = False
    numerology: int = 1
    cp_extended: int = 0
    grid_index: int = 0
    llr_offset: Optional[int] = None
    format = 4
    nof_prb = 1

    nof_uci_bits = PucchF3.nof_uci_bits
    modulation_order = PucchF3.modulation_order
    nof_data_symbols = PucchF3.nof_data_symbols

    @property
    def nof_llrs(self) -> int:
        return 12 * self.nof_data_symbols * self.modulation_order // max(self.occ_length, 1)


def make_pucch_f34_configs(pdus):
    """The C array of srsgpu_pucch_f34_plan_create and the LLR offsets used (a PDU without one follows the PDU before
    it, at the next multiple of 4: E need not be one)."""
    cfg = (PucchF34Config * max(len(pdus), 1))()
    offsets, o = [], 0
    for a, d in zip(cfg, pdus):
        a.slot_index, a.format, a.numerology, a.cp_extended = d.slot_index, d.format, d.numerology, d.cp_extended
        a.nof_prb, a.start_symbol_index, a.nof_symbols = d.nof_prb, d.start_symbol_index, d.nof_symbols
        a.starting_prb = d.starting_prb
        a.second_hop_prb = PUCCH_NO_HOP if d.second_hop_prb is None else d.second_hop_prb
        a.additional_dmrs, a.pi2_bpsk = int(d.additional_dmrs), int(d.pi2_bpsk)
        a.occ_length, a.occ_index = d.occ_length, d.occ_index
        a.rnti, a.n_id_scrambling, a.n_id_hopping = d.rnti, d.n_id_scrambling, d.n_id_hopping
        a.nof_uci_bits, a.nof_ports = d.nof_uci_bits, len(d.ports)
        for i, p in enumerate(list(d.ports)[:4]):
            a.ports[i] = p
        a.grid_index = d.grid_index
        a.llr_offset = o if d.llr_offset is None else d.llr_offset
        offsets.append(int(a.llr_offset))
        o = (int(a.llr_offset) + max(d.nof_llrs, 0) + 3) // 4 * 4
    return cfg, offsets


class PucchF34Plan(_Handle):
    """srsgpu_pucch_f34_plan: estimation, equalisation, the inverse DFT, despreading, demapping and descrambling of
    every Format 3 and Format 4 PDU of a batch of slots in one launch. Results: one PUCCH_F2_RESULT_DTYPE record per
    PDU. Raises SrsGpuError on a refusal."""
    _destroy = "srsgpu_pucch_f34_plan_destroy"

    def __init__(self, ctx: Context, pdus, grid_nof_prb: int, grid_nof_ports: int = 4, nof_grids: Optional[int] = None):
        self.ctx = ctx
        if nof_grids is None:
            nof_grids = max([d.grid_index for d in pdus], default=0) + 1
        self.nof_grids, self.grid_nof_prb, self.grid_nof_ports = nof_grids, grid_nof_prb, grid_nof_ports
        cfg, self.llr_offsets = make_pucch_f34_configs(pdus)
        self.nof_pdus = len(pdus)
        self.nof_llrs = max([o + max(d.nof_llrs, 0) for o, d in zip(self.llr_offsets, pdus)], default=0)
        self._create("srsgpu_pucch_f34_plan_create", ctx.handle, _cptr(cfg), len(pdus), grid_nof_prb, grid_nof_ports,
                     nof_grids)

    def execute(self, d_grids, d_llrs, d_results, stream=None):
        """d_grids: (nof_grids, ports, 14, 12 PRBs) int32 / uint32 words (re | im << 16, bf16); d_llrs: int8, 4-byte
        aligned, at least nof_llrs entries, written only inside the PDUs' ranges; d_results: at least 96 * nof_pdus
        bytes, every byte of which is written. Asynchronous on `stream`."""
        _check(_lib().srsgpu_pucch_f34_plan_execute(self.handle, _dptr(d_grids), _dptr(d_llrs), _dptr(d_results),
                                                    _stream_handle(stream)))


class PucchF34Batch(PucchF2Batch):
    """The three plans of a batch of Format 3 / 4 PDUs with their device buffers, as PucchF2Batch: launch(d_grids)
    enqueues the front end, the short-block decoder (3..11 bits, modulation order 1 with pi/2-BPSK and 2 without) and
    the polar decoder (12 bits and more; a field of E >= 1088 with >= 360 bits takes two codeblocks there) on one
    stream, both decoders reading source 0 at the PDUs' LLR offsets; results() reads them back."""

    def __init__(self, ctx: Context, pdus, grid_nof_prb: int, grid_nof_ports: int = 4, nof_grids: Optional[int] = None):
        self.ctx, self.pdus = ctx, list(pdus)
        dev = torch.device("cuda", ctx.device)
        self.front = PucchF34Plan(ctx, self.pdus, grid_nof_prb, grid_nof_ports, nof_grids)
        offs = self.front.llr_offsets
        self.short_ids = [i for i, d in enumerate(self.pdus) if d.nof_uci_bits <= 11]
        self.polar_ids = [i for i, d in enumerate(self.pdus) if d.nof_uci_bits >= 12]
        self.short = UciDecoderPlan(ctx, [(self.pdus[i].nof_uci_bits, self.pdus[i].modulation_order, 0,
                                           self.pdus[i].nof_llrs, offs[i]) for i in self.short_ids]) if self.short_ids else None
        self.polar = UciPolarDecoderPlan(ctx, [(self.pdus[i].nof_uci_bits, 0, self.pdus[i].nof_llrs, offs[i], None)
                                               for i in self.polar_ids]) if self.polar_ids else None
        self.d_llrs = torch.zeros(self.front.nof_llrs + 4, dtype=torch.int8, device=dev)
        self.d_results = torch.zeros(PUCCH_F2_RESULT_DTYPE.itemsize * max(len(self.pdus), 1), dtype=torch.uint8, device=dev)
        self.d_short_msgs = torch.zeros(max(len(self.short_ids), 1), dtype=torch.int16, device=dev)
        self.d_short_status = torch.zeros(max(len(self.short_ids), 1), dtype=torch.uint8, device=dev)
        self.d_polar_msgs = torch.zeros(max(self.polar.nof_msg_words if self.polar else 0, 1), dtype=torch.int32, device=dev)
        self.d_polar_status = torch.zeros(max(len(self.polar_ids), 1), dtype=torch.uint8, device=dev)


class PucchF34Processor:
    """GPU counterpart of pucch_processor::process(grid, format3_configuration) and (grid, format4_configuration)
    (pucch_processor_impl.cpp:227 / :315) for a batch: process_batch(grids, pdus) returns one PucchF2Result per PDU
    (PucchF3 or PucchF4): the payload split into HARQ-ACK, SR and CSI Part 1, the status and the channel state combined
    as for Format 2. grids: (nof_grids, ports, 14, 12 PRBs) uint32 (re | im << 16, bf16)."""

    def __init__(self, ctx: Context, grid_nof_prb: int, grid_nof_ports: int = 4):
        self.ctx, self.grid_nof_prb, self.grid_nof_ports = ctx, grid_nof_prb, grid_nof_ports

    def process_batch(self, grids: np.ndarray, pdus):
        dev = torch.device("cuda", self.ctx.device)
        batch = PucchF34Batch(self.ctx, pdus, self.grid_nof_prb, self.grid_nof_ports, grids.shape[0])
        d_grids = torch.from_numpy(np.ascontiguousarray(grids).view(np.int32)).to(dev)
        batch.launch(d_grids)
        torch.cuda.synchronize(dev)
        out = batch.results()
        batch.close()
        return out
