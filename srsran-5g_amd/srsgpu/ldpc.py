"""LDPC decoding: the codeblock decoder plan (srsgpu_ldpc_decoder_plan), the PUSCH codeblock plan with rate dematching
and HARQ combining (srsgpu_pusch_cb_plan) and their ldpc_decoder-shaped wrappers."""
import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from ._abi import Context, SrsGpuError, torch, _check, _cptr, _dptr, _Handle, _lib, _stream_handle


CRC24A, CRC24B, CRC24C, CRC16, CRC11, CRC6 = range(6)
CRC_NONE = 255
IMPL_GENERIC, IMPL_SIMD = 0, 1
IMPL_BY_NAME = {"generic": IMPL_GENERIC, "avx2": IMPL_SIMD, "avx512": IMPL_SIMD, "neon": IMPL_SIMD,
                "auto": IMPL_SIMD, "simd": IMPL_SIMD}
BG_K = {1: 22, 2: 10}
BG_N_SHORT = {1: 66, 2: 50}


class LdpcDecoderConfig(ctypes.Structure):
    """srsgpu_ldpc_decoder_config (include/srsgpu_phy.h)."""
    _fields_ = [
        ("base_graph", ctypes.c_uint8),
        ("crc_poly", ctypes.c_uint8),
        ("lifting_size", ctypes.c_uint16),
        ("nof_filler_bits", ctypes.c_uint16),
        ("nof_crc_bits", ctypes.c_uint8),
        ("max_iterations", ctypes.c_uint8),
        ("scaling_factor", ctypes.c_float),
        ("llr_offset", ctypes.c_uint32),
        ("nof_llrs", ctypes.c_uint32),
        ("out_offset", ctypes.c_uint32),
    ]


assert ctypes.sizeof(LdpcDecoderConfig) == 24


@dataclass
class CodeblockDecodeConfig:
    """Mirror of srsran::ldpc_decoder::configuration (ldpc_decoder.h:44) for one codeblock."""
    base_graph: int
    lifting_size: int
    nof_crc_bits: int = 16
    nof_filler_bits: int = 0
    max_iterations: int = 6
    scaling_factor: float = 0.8


def make_configs(cfgs: Sequence[CodeblockDecodeConfig], nof_llrs: Sequence[int], crc_polys: Sequence[int],
                 llr_offsets: Optional[Sequence[int]] = None, out_offsets: Optional[Sequence[int]] = None):
    """Packs per-codeblock configurations into the C array, with default contiguous offsets."""
    n = len(cfgs)
    arr = (LdpcDecoderConfig * n)()
    llr_off = 0
    out_off = 0
    for i, c in enumerate(cfgs):
        a = arr[i]
        a.base_graph = c.base_graph
        a.crc_poly = crc_polys[i]
        a.lifting_size = c.lifting_size
        a.nof_filler_bits = c.nof_filler_bits
        a.nof_crc_bits = c.nof_crc_bits
        a.max_iterations = c.max_iterations
        a.scaling_factor = c.scaling_factor
        a.nof_llrs = nof_llrs[i]
        a.llr_offset = llr_offsets[i] if llr_offsets is not None else llr_off
        a.out_offset = out_offsets[i] if out_offsets is not None else out_off
        llr_off += nof_llrs[i]
        out_off += (BG_K[c.base_graph] * c.lifting_size + 7) // 8
    return arr


class LdpcDecoderPlan(_Handle):
    """srsgpu_ldpc_decoder_plan: validated, device-resident batch of decoder work (hipGraph-capturable execute)."""
    _destroy = "srsgpu_ldpc_decoder_plan_destroy"

    def __init__(self, ctx: Context, impl: int, cfg_array):
        self.ctx = ctx
        self._create("srsgpu_ldpc_decoder_plan_create", ctx.handle, impl, _cptr(cfg_array), len(cfg_array))
        self.nof_cbs = len(cfg_array)

    def execute(self, d_llrs, d_out, d_iters, stream=None):
        _check(_lib().srsgpu_ldpc_decoder_plan_execute(self.handle, _dptr(d_llrs), _dptr(d_out), _dptr(d_iters),
                                                       _stream_handle(stream)))


def unpack_bits(packed: np.ndarray, nbits: int) -> np.ndarray:
    return np.unpackbits(np.asarray(packed, dtype=np.uint8))[:nbits]


class LdpcDecoder:
    """GPU implementation of srsran::ldpc_decoder (ldpc_decoder.h), created like
    create_ldpc_decoder_factory_sw(type)->create() (channel_coding_factories.h): type "generic" or "avx2"/"avx512"/
    "neon"/"auto" selects the arithmetic variant the results are bit-exact with."""

    def __init__(self, ctx: Context, dec_type: str = "auto"):
        if dec_type not in IMPL_BY_NAME:
            raise SrsGpuError(f"invalid LDPC decoder type '{dec_type}'")
        self.ctx = ctx
        self.impl = IMPL_BY_NAME[dec_type]

    def decode(self, llrs: np.ndarray, cfg: CodeblockDecodeConfig, crc_poly: Optional[int] = None,
               output_init: Optional[np.ndarray] = None):
        """Decodes one codeblock. Returns (nof_iterations or None, K*Z unpacked bits) like ldpc_decoder::decode."""
        res = self.decode_batch([llrs], [cfg], [crc_poly], None if output_init is None else [output_init])
        return res[0]

    def decode_batch(self, llrs_list: List[np.ndarray], cfgs: List[CodeblockDecodeConfig],
                     crc_polys: List[Optional[int]], output_inits=None):
        n = len(cfgs)
        nof_llrs = [int(np.asarray(x).size) for x in llrs_list]
        polys = [CRC_NONE if p is None else p for p in crc_polys]
        arr = make_configs(cfgs, nof_llrs, polys)
        flat = np.concatenate([np.asarray(x, dtype=np.int8) for x in llrs_list]) if n else np.zeros(0, np.int8)
        out_bytes = [(BG_K[c.base_graph] * c.lifting_size + 7) // 8 for c in cfgs]
        dev = torch.device("cuda", self.ctx.device)
        d_llrs = torch.from_numpy(flat).to(dev)
        if output_inits is not None:
            init = np.concatenate([np.packbits(np.asarray(o, dtype=np.uint8)) for o in output_inits])
            d_out = torch.from_numpy(init).to(dev)
        else:
            d_out = torch.zeros(sum(out_bytes), dtype=torch.uint8, device=dev)
        d_iters = torch.zeros(n, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev)
        _check(_lib().srsgpu_ldpc_decode(self.ctx.handle, self.impl, _cptr(arr), n, _dptr(d_llrs), _dptr(d_out),
                                         _dptr(d_iters), stream.cuda_stream))
        out = d_out.cpu().numpy()
        iters = d_iters.cpu().numpy()
        results = []
        off = 0
        for i, c in enumerate(cfgs):
            nb = BG_K[c.base_graph] * c.lifting_size
            bits = unpack_bits(out[off: off + out_bytes[i]], nb)
            off += out_bytes[i]
            results.append((None if iters[i] < 0 else int(iters[i]), bits))
        return results


class PuschCbConfig(ctypes.Structure):
    """srsgpu_pusch_cb_config (include/srsgpu_phy.h)."""
    _fields_ = [
        ("base_graph", ctypes.c_uint8),
        ("rv", ctypes.c_uint8),
        ("modulation_order", ctypes.c_uint8),
        ("crc_poly", ctypes.c_uint8),
        ("lifting_size", ctypes.c_uint16),
        ("nof_filler_bits", ctypes.c_uint16),
        ("nof_crc_bits", ctypes.c_uint8),
        ("max_iterations", ctypes.c_uint8),
        ("new_data", ctypes.c_uint8),
        ("use_early_stop", ctypes.c_uint8),
        ("scaling_factor", ctypes.c_float),
        ("Nref", ctypes.c_uint32),
        ("rm_length", ctypes.c_uint32),
        ("llr_offset", ctypes.c_uint32),
        ("harq_offset", ctypes.c_uint32),
        ("out_offset", ctypes.c_uint32),
    ]


assert ctypes.sizeof(PuschCbConfig) == 36


class PuschCbPlan(_Handle):
    """srsgpu_pusch_cb_plan: rate dematching + HARQ combining + LDPC decoding + CB CRC for a batch of codeblocks."""
    _destroy = "srsgpu_pusch_cb_plan_destroy"

    def __init__(self, ctx: Context, impl: int, cfg_array):
        self.ctx = ctx
        self._create("srsgpu_pusch_cb_plan_create", ctx.handle, impl, _cptr(cfg_array), len(cfg_array))
        self.nof_cbs = len(cfg_array)

    def execute(self, d_llrs, d_harq, d_out, d_iters, d_cb_crc_ok=None, stream=None):
        _check(_lib().srsgpu_pusch_cb_plan_execute(self.handle, _dptr(d_llrs), _dptr(d_harq), _dptr(d_out),
                                                   _dptr(d_iters), _dptr(d_cb_crc_ok), _stream_handle(stream)))


@dataclass
class PuschCodeblock:
    """One codeblock of a PUSCH transport block: hw_pusch_decoder_configuration (hw_accelerator_pusch_dec.h:30)."""
    base_graph: int
    lifting_size: int
    rv: int
    modulation_order: int
    rm_length: int
    nof_filler_bits: int = 0
    crc_poly: int = CRC24B
    nof_crc_bits: int = 24
    Nref: int = 0
    new_data: bool = True
    use_early_stop: bool = True
    max_iterations: int = 6
    scaling_factor: float = 0.8


def make_pusch_cb_configs(cbs: Sequence[PuschCodeblock]):
    """Packs codeblocks with contiguous LLR / HARQ / output offsets."""
    arr = (PuschCbConfig * len(cbs))()
    lo = ho = oo = 0
    for i, c in enumerate(cbs):
        a = arr[i]
        a.base_graph, a.rv, a.modulation_order, a.crc_poly = c.base_graph, c.rv, c.modulation_order, c.crc_poly
        a.lifting_size, a.nof_filler_bits, a.nof_crc_bits = c.lifting_size, c.nof_filler_bits, c.nof_crc_bits
        a.max_iterations, a.new_data, a.use_early_stop = c.max_iterations, int(c.new_data), int(c.use_early_stop)
        a.scaling_factor, a.Nref, a.rm_length = c.scaling_factor, c.Nref, c.rm_length
        a.llr_offset, a.harq_offset, a.out_offset = lo, ho, oo
        lo += c.rm_length
        ho += BG_N_SHORT[c.base_graph] * c.lifting_size
        oo += (BG_K[c.base_graph] * c.lifting_size + 7) // 8
    return arr, lo, ho, oo


class PuschCodeblockDecoder:
    """GPU counterpart of pusch_codeblock_decoder (pusch_codeblock_decoder.cpp:33) / hw_accelerator_pusch_dec with an
    external (device-resident) HARQ buffer: the caller owns d_harq and d_cb_crc_ok across retransmissions."""

    def __init__(self, ctx: Context, dec_type: str = "auto"):
        if dec_type not in IMPL_BY_NAME:
            raise SrsGpuError(f"invalid decoder type '{dec_type}'")
        self.ctx = ctx
        self.impl = IMPL_BY_NAME[dec_type]

    def decode(self, llrs_list, cbs: Sequence[PuschCodeblock], harq: np.ndarray = None, cb_crc_ok: np.ndarray = None):
        """Returns (results [(nof_iterations or None, K*Z bits)], updated harq buffer, updated crc flags)."""
        arr, nllr, nharq, nout = make_pusch_cb_configs(cbs)
        dev = torch.device("cuda", self.ctx.device)
        flat = np.concatenate([np.asarray(x, dtype=np.int8) for x in llrs_list])
        assert flat.size == nllr
        d_llrs = torch.from_numpy(flat).to(dev)
        d_harq = (torch.from_numpy(np.asarray(harq, dtype=np.int8).copy()).to(dev) if harq is not None
                  else torch.zeros(nharq, dtype=torch.int8, device=dev))
        d_crc = (torch.from_numpy(np.asarray(cb_crc_ok, dtype=np.uint8).copy()).to(dev) if cb_crc_ok is not None
                 else torch.zeros(len(cbs), dtype=torch.uint8, device=dev))
        d_out = torch.zeros(nout, dtype=torch.uint8, device=dev)
        d_iters = torch.zeros(len(cbs), dtype=torch.int32, device=dev)
        plan = PuschCbPlan(self.ctx, self.impl, arr)
        plan.execute(d_llrs, d_harq, d_out, d_iters, d_crc)
        torch.cuda.synchronize(dev)
        plan.close()
        out = d_out.cpu().numpy()
        iters = d_iters.cpu().numpy()
        res = []
        off = 0
        for i, c in enumerate(cbs):
            nb = BG_K[c.base_graph] * c.lifting_size
            ob = (nb + 7) // 8
            res.append((None if iters[i] < 0 else int(iters[i]), unpack_bits(out[off:off + ob], nb)))
            off += ob
        return res, d_harq.cpu().numpy(), d_crc.cpu().numpy()
