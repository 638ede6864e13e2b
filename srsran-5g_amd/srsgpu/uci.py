"""UCI decoding: short-block fields of 1..11 bits (srsgpu_uci_decoder_plan) and polar-coded fields of 12..1706 bits
(srsgpu_uci_polar_decoder_plan)."""
import ctypes
from typing import Sequence

import numpy as np

from ._abi import Context, torch, _check, _cptr, _dptr, _Handle, _lib, _stream_handle


class UciFieldConfig(ctypes.Structure):
    """srsgpu_uci_field_config (include/srsgpu_phy.h): one UCI field of 1..11 bits, its modulation order, its input
    stream (0..2) and where its E encoded LLRs start there."""
    _fields_ = [
        ("nof_bits", ctypes.c_uint8),
        ("modulation_order", ctypes.c_uint8),
        ("source", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8),
        ("nof_enc_bits", ctypes.c_uint32),
        ("llr_offset", ctypes.c_uint32),
    ]


assert ctypes.sizeof(UciFieldConfig) == 12


class UciDecoderPlan(_Handle):
    """srsgpu_uci_decoder_plan: short-block UCI fields (1..11 bits) decoded in one launch. fields: UciFieldConfig
    entries, or (nof_bits, modulation_order, source, nof_enc_bits, llr_offset) tuples."""
    _destroy = "srsgpu_uci_decoder_plan_destroy"

    def __init__(self, ctx: Context, fields):
        self.ctx = ctx
        self.nof_fields = len(fields)
        arr = (UciFieldConfig * max(len(fields), 1))()
        for i, f in enumerate(fields):
            if isinstance(f, UciFieldConfig):
                arr[i] = f
            else:
                a = arr[i]
                a.nof_bits, a.modulation_order, a.source, a.nof_enc_bits, a.llr_offset = f
        self._create("srsgpu_uci_decoder_plan_create", ctx.handle, _cptr(arr), len(fields))

    def execute(self, d_harq, d_csi1, d_csi2, d_msgs, d_status, stream=None):
        """Inputs: the three int8 LLR streams (sources 0, 1, 2; None where no field reads one). Outputs: d_msgs
        (int16 / uint16, bit j = message bit j) and d_status (uint8, 1 valid) per field."""
        _check(_lib().srsgpu_uci_decoder_plan_execute(self.handle, _dptr(d_harq), _dptr(d_csi1), _dptr(d_csi2),
                                                      _dptr(d_msgs), _dptr(d_status), _stream_handle(stream)))


class UciDecoder:
    """GPU counterpart of srsran::short_block_detector::detect (short_block_detector_impl.cpp:186), which
    uci_decoder_impl::decode uses for messages of up to 11 bits: decode_batch() takes each field's LLRs, number of
    message bits and modulation order and returns (list of uint8 bit arrays, list of valid flags)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def decode_batch(self, llrs_list: Sequence[np.ndarray], nof_bits: Sequence[int],
                     modulation_orders: Sequence[int]):
        dev = torch.device("cuda", self.ctx.device)
        fields, o = [], 0
        for llrs, a, qm in zip(llrs_list, nof_bits, modulation_orders):
            fields.append((int(a), int(qm), 0, int(np.asarray(llrs).size), o))
            o += int(np.asarray(llrs).size)
        plan = UciDecoderPlan(self.ctx, fields)
        host = np.concatenate([np.asarray(x, np.int8).ravel() for x in llrs_list] + [np.zeros(4, np.int8)])
        d_in = torch.from_numpy(host).to(dev)
        d_msgs = torch.zeros(max(len(fields), 1), dtype=torch.int16, device=dev)
        d_status = torch.zeros(max(len(fields), 1), dtype=torch.uint8, device=dev)
        plan.execute(d_in, None, None, d_msgs, d_status)
        torch.cuda.synchronize(dev)
        msgs, status = d_msgs.cpu().numpy().view(np.uint16), d_status.cpu().numpy()
        plan.close()
        bits = [((int(m) >> np.arange(int(a))) & 1).astype(np.uint8) for m, a in zip(msgs, nof_bits)]
        return bits, [bool(v) for v in status[: len(fields)]]


class UciPolarFieldConfig(ctypes.Structure):
    """srsgpu_uci_polar_field_config (include/srsgpu_phy.h): one polar-coded UCI field of 12..1706 bits, its input
    stream (0..2), where its E encoded LLRs start there and its first output word."""
    _fields_ = [
        ("nof_bits", ctypes.c_uint16),
        ("source", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8),
        ("nof_enc_bits", ctypes.c_uint32),
        ("llr_offset", ctypes.c_uint32),
        ("msg_word_offset", ctypes.c_uint32),
    ]


assert ctypes.sizeof(UciPolarFieldConfig) == 16


def uci_polar_msg_word_offsets(nof_bits: Sequence[int]):
    """Packs the fields' output words back to back: (msg_word_offset per field, total words); a field of A bits owns
    ceil(A / 32) words."""
    offs, o = [], 0
    for a in nof_bits:
        offs.append(o)
        o += (int(a) + 31) // 32
    return offs, o


def uci_polar_unpack(words: np.ndarray, msg_word_offset: int, nof_bits: int) -> np.ndarray:
    """The nof_bits message bits of a field from the plan's output words (bit j mod 32 of word offset + j / 32)."""
    w = np.asarray(words).view(np.uint32)[msg_word_offset: msg_word_offset + (nof_bits + 31) // 32]
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(np.uint8).ravel()[:nof_bits]


class UciPolarDecoderPlan(_Handle):
    """srsgpu_uci_polar_decoder_plan: polar-coded UCI fields (12..1706 bits) decoded in one launch, one wavefront per
    codeblock. fields: UciPolarFieldConfig entries, or (nof_bits, source, nof_enc_bits, llr_offset, msg_word_offset)
    tuples; a msg_word_offset of None packs the fields' words back to back in field order (self.msg_word_offsets,
    self.nof_msg_words)."""
    _destroy = "srsgpu_uci_polar_decoder_plan_destroy"

    def __init__(self, ctx: Context, fields):
        self.ctx = ctx
        self.nof_fields = len(fields)
        arr = (UciPolarFieldConfig * max(len(fields), 1))()
        auto, _ = uci_polar_msg_word_offsets([f.nof_bits if isinstance(f, UciPolarFieldConfig) else f[0]
                                              for f in fields])
        for i, f in enumerate(fields):
            if isinstance(f, UciPolarFieldConfig):
                arr[i] = f
            else:
                a = arr[i]
                a.nof_bits, a.source, a.nof_enc_bits, a.llr_offset = f[:4]
                a.msg_word_offset = auto[i] if len(f) < 5 or f[4] is None else f[4]
        self.nof_bits = [int(arr[i].nof_bits) for i in range(len(fields))]
        self.msg_word_offsets = [int(arr[i].msg_word_offset) for i in range(len(fields))]
        self.nof_msg_words = max([o + (a + 31) // 32 for o, a in zip(self.msg_word_offsets, self.nof_bits)], default=0)
        self._create("srsgpu_uci_polar_decoder_plan_create", ctx.handle, _cptr(arr), len(fields))

    def execute(self, d_harq, d_csi1, d_csi2, d_msgs, d_status, stream=None):
        """Inputs: the three int8 LLR streams (sources 0, 1, 2; None where no field reads one). Outputs: d_msgs
        (int32 / uint32 words, see srsgpu_uci_polar_decoder_plan_execute) and d_status (uint8, 1 valid) per field."""
        _check(_lib().srsgpu_uci_polar_decoder_plan_execute(self.handle, _dptr(d_harq), _dptr(d_csi1), _dptr(d_csi2),
                                                            _dptr(d_msgs), _dptr(d_status), _stream_handle(stream)))


class UciPolarDecoder:
    """GPU counterpart of uci_decoder_impl::decode_codeword_polar (uci_decoder_impl.cpp:43), which uci_decoder::decode
    uses for messages of 12 bits and more: decode_batch() takes each field's LLRs and number of message bits and
    returns (list of uint8 bit arrays, list of valid flags). Both codeblocks of a two-codeblock field are decoded."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def decode_batch(self, llrs_list: Sequence[np.ndarray], nof_bits: Sequence[int]):
        dev = torch.device("cuda", self.ctx.device)
        fields, o = [], 0
        for llrs, a in zip(llrs_list, nof_bits):
            fields.append((int(a), 0, int(np.asarray(llrs).size), o, None))
            o += int(np.asarray(llrs).size)
        plan = UciPolarDecoderPlan(self.ctx, fields)
        host = np.concatenate([np.asarray(x, np.int8).ravel() for x in llrs_list] + [np.zeros(4, np.int8)])
        d_in = torch.from_numpy(host).to(dev)
        d_msgs = torch.zeros(max(plan.nof_msg_words, 1), dtype=torch.int32, device=dev)
        d_status = torch.zeros(max(len(fields), 1), dtype=torch.uint8, device=dev)
        plan.execute(d_in, None, None, d_msgs, d_status)
        torch.cuda.synchronize(dev)
        words, status = d_msgs.cpu().numpy().view(np.uint32), d_status.cpu().numpy()
        bits = [uci_polar_unpack(words, w, a) for w, a in zip(plan.msg_word_offsets, plan.nof_bits)]
        plan.close()
        return bits, [bool(v) for v in status[: len(fields)]]
