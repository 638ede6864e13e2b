"""The C ABI of libsrsgpu_phy.so as Python sees it: where the library lies and how it is loaded, the one table of
function prototypes (include/srsgpu_phy.h), the error and handle plumbing every plan shares, the context, and the
structures and helpers that more than one channel uses. tests/test_capi_symbols.py holds the table to the header."""
import ctypes
import os
from typing import Optional

import numpy as np

try:  # srsgpu/__init__.py has imported torch by now, before anything here can load the library.
    import torch
except ImportError:  # pragma: no cover - torch is part of the image
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
# SRSGPU_LIB selects another build of the library (e.g. an instrumented one under a different SRSGPU_OUT_DIR).
LIB_PATH = os.environ.get("SRSGPU_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libsrsgpu_phy.so"))

SRSGPU_OK = 0


class SrsGpuError(RuntimeError):
    pass


_P = ctypes.c_void_p        # every pointer: handles, host arrays, device addresses, streams
_OUT = ctypes.POINTER(_P)   # a handle the function gives back
_INT, _U32, _U64 = ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
_U32_OUT = ctypes.POINTER(_U32)
OPTIONAL = "optional"       # a row a side library loaded through SRSGPU_LIB may lack (built before the symbol existed)

# Every function include/srsgpu_phy.h declares: name -> (restype, argtypes[, OPTIONAL]). restype None is void.
PROTOTYPES = {
    "srsgpu_version": (_INT, []),
    "srsgpu_last_error": (ctypes.c_char_p, []),
    "srsgpu_context_create": (_INT, [_INT, _OUT]),
    "srsgpu_context_destroy": (None, [_P]),
    "srsgpu_context_device": (_INT, [_P]),
    "srsgpu_context_set_option": (_INT, [_P, _INT, _INT]),
    "srsgpu_context_get_option": (_INT, [_P, _INT, ctypes.POINTER(_INT)]),
    "srsgpu_ldpc_decoder_plan_create": (_INT, [_P, _INT, _P, _U32, _OUT]),
    "srsgpu_ldpc_decoder_plan_execute": (_INT, [_P, _P, _P, _P, _P]),
    "srsgpu_ldpc_decoder_plan_destroy": (None, [_P]),
    "srsgpu_ldpc_decode": (_INT, [_P, _INT, _P, _U32, _P, _P, _P, _P]),
    "srsgpu_pusch_cb_plan_create": (_INT, [_P, _INT, _P, _U32, _OUT]),
    "srsgpu_pusch_cb_plan_execute": (_INT, [_P, _P, _P, _P, _P, _P, _P]),
    "srsgpu_pusch_cb_plan_destroy": (None, [_P]),
    "srsgpu_pdsch_encoder_plan_create": (_INT, [_P, _P, _U32, _OUT]),
    "srsgpu_pdsch_encoder_plan_nof_codeblocks": (_U32, [_P]),
    "srsgpu_pdsch_encoder_plan_execute": (_INT, [_P, _P, _P, _P]),
    "srsgpu_pdsch_encoder_plan_destroy": (None, [_P]),
    "srsgpu_pdsch_encoder_plan_enable_timing": (_INT, [_P, _INT]),
    "srsgpu_pdsch_encoder_plan_stage_times": (_INT, [_P, _P, _U32_OUT]),
    "srsgpu_pdsch_modulator_plan_create": (_INT, [_P, _P, _U32, _U32, _U32, _OUT]),
    "srsgpu_pdsch_modulator_plan_create_ex": (_INT, [_P, _P, _P, _U32, _U32, _U32, _OUT]),
    "srsgpu_pdsch_modulator_plan_execute": (_INT, [_P, _P, _P, _P]),
    "srsgpu_pdsch_modulator_plan_destroy": (None, [_P]),
    "srsgpu_pdsch_dmrs_plan_create": (_INT, [_P, _P, _U32, _U32, _U32, _OUT]),
    "srsgpu_pdsch_dmrs_plan_create_ex": (_INT, [_P, _P, _P, _U32, _U32, _U32, _OUT]),
    "srsgpu_pdsch_dmrs_plan_execute": (_INT, [_P, _P, _P]),
    "srsgpu_pdsch_dmrs_plan_destroy": (None, [_P]),
    "srsgpu_pdcch_plan_create": (_INT, [_P, _P, _U32, _U32, _U32, _U32, _OUT]),
    "srsgpu_pdcch_plan_execute": (_INT, [_P, _P, _U64, _P, _P]),
    "srsgpu_pdcch_plan_destroy": (None, [_P]),
    "srsgpu_ssb_plan_create": (_INT, [_P, _P, _U32, _U32, _U32, _U32, _OUT]),
    "srsgpu_ssb_plan_execute": (_INT, [_P, _P, _U64, _P, _P]),
    "srsgpu_ssb_plan_destroy": (None, [_P]),
    "srsgpu_csi_rs_plan_create": (_INT, [_P, _P, _U32, _U32, _U32, _U32, _OUT]),
    "srsgpu_csi_rs_plan_execute": (_INT, [_P, _P, _P]),
    "srsgpu_csi_rs_plan_destroy": (None, [_P]),
    "srsgpu_pucch_detector_plan_create": (_INT, [_P, _P, _U32, _P, _U32, _P, _U32, _U32, _U32, _U32, _OUT]),
    "srsgpu_pucch_detector_plan_execute": (_INT, [_P, _P, _P, _P]),
    "srsgpu_pucch_detector_plan_destroy": (None, [_P]),
    "srsgpu_prach_detector_plan_create": (_INT, [_P, _P, _U32, _P, _U32, _U64, _OUT]),
    "srsgpu_prach_detector_plan_execute": (_INT, [_P, _P, _P, _P]),
    "srsgpu_prach_detector_plan_destroy": (None, [_P]),
    "srsgpu_prach_max_delay_samples": (_INT, [_U32, _U32, _U32, _U32_OUT]),
    "srsgpu_srs_estimator_plan_create": (_INT, [_P, _P, _U32, _U32, _U32, _U32, _OUT]),
    "srsgpu_srs_estimator_plan_execute": (_INT, [_P, _P, _P, _P]),
    "srsgpu_srs_estimator_plan_destroy": (None, [_P]),
    "srsgpu_pucch_f2_plan_create": (_INT, [_P, _P, _U32, _U32, _U32, _U32, _OUT]),
    "srsgpu_pucch_f2_plan_execute": (_INT, [_P, _P, _P, _P, _P]),
    "srsgpu_pucch_f2_plan_destroy": (None, [_P]),
    "srsgpu_pucch_f34_plan_create": (_INT, [_P, _P, _U32, _U32, _U32, _U32, _OUT]),
    "srsgpu_pucch_f34_plan_execute": (_INT, [_P, _P, _P, _P, _P]),
    "srsgpu_pucch_f34_plan_destroy": (None, [_P]),
    "srsgpu_ofdm_modulator_plan_create": (_INT, [_P, _P, _U32, _U32, _P, _OUT]),
    "srsgpu_ofdm_demodulator_plan_create": (_INT, [_P, _P, _U32, _U32, _P, _OUT]),
    "srsgpu_ofdm_modulator_symbols_plan_create": (_INT, [_P, _P, _U32, _U32, _U32, _U32, _OUT]),
    "srsgpu_ofdm_demodulator_symbols_plan_create": (_INT, [_P, _P, _U32, _U32, _U32, _U32, _OUT]),
    "srsgpu_ofdm_plan_concat": (_INT, [_P, _P, _U32, _OUT]),
    "srsgpu_ofdm_plan_get_jobs": (_INT, [_P, _P, _U32, _U32_OUT]),
    "srsgpu_ofdm_jobs_execute": (_INT, [_P, _P, _U32, _P, _P, _P]),
    "srsgpu_ofdm_jobs_execute_direct": (_INT, [_P, _P, _U32, _P]),
    "srsgpu_ofdm_plan_nof_grid_words": (_U64, [_P]),
    "srsgpu_ofdm_plan_nof_samples": (_U64, [_P]),
    "srsgpu_ofdm_plan_sample_offset": (_U64, [_P, _U32, _U32]),
    "srsgpu_ofdm_modulator_plan_execute": (_INT, [_P, _P, _P, _P]),
    "srsgpu_ofdm_modulator_plan_execute_twin": (_INT, [_P, _P, _P, _P, _P], OPTIONAL),
    "srsgpu_ofdm_demodulator_plan_execute": (_INT, [_P, _P, _P, _P]),
    "srsgpu_ofdm_plan_destroy": (None, [_P]),
    "srsgpu_pusch_chest_plan_create": (_INT, [_P, _P, _U32, _U32, _U32, _OUT]),
    "srsgpu_pusch_chest_plan_create_ex": (_INT, [_P, _P, _P, _U32, _U32, _U32, _OUT]),
    "srsgpu_pusch_chest_plan_execute": (_INT, [_P, _P, _P, _P, _P, _P]),
    "srsgpu_pusch_chest_plan_execute_copy": (_INT, [_P, _P, _P, _P, _P, _P, _U32, _U64, _P]),
    "srsgpu_pusch_chest_plan_destroy": (None, [_P]),
    "srsgpu_pusch_demodulator_plan_create": (_INT, [_P, _P, _U32, _U32, _U32, _OUT]),
    "srsgpu_pusch_demodulator_plan_create_ex": (_INT, [_P, _P, _P, _U32, _U32, _U32, _OUT]),
    "srsgpu_pusch_demodulator_plan_nof_llrs": (_U32, [_P, _U32]),
    "srsgpu_pusch_demodulator_plan_symbol_closed_form": (_INT, [_P, _U32]),
    "srsgpu_pusch_demodulator_plan_scrambling": (_INT, [_P, _U32, _P, _P]),
    "srsgpu_pusch_demodulator_plan_execute": (_INT, [_P, _P, _P, _P, _P, _P]),
    "srsgpu_pusch_demodulator_plan_execute_ex": (_INT, [_P, _P, _P, _P, _P, _P, _P]),
    "srsgpu_pusch_demodulator_plan_destroy": (None, [_P]),
    "srsgpu_ulsch_demux_plan_create": (_INT, [_P, _P, _U32, _OUT]),
    "srsgpu_ulsch_demux_plan_nof_llrs": (_U32, [_P, _U32, _U32]),
    "srsgpu_ulsch_demux_plan_symbol_llrs": (_INT, [_P, _U32, _U32, _P]),
    "srsgpu_ulsch_demux_plan_execute": (_INT, [_P, _P, _P, _P, _P, _P, _P]),
    "srsgpu_ulsch_demux_plan_destroy": (None, [_P]),
    "srsgpu_uci_decoder_plan_create": (_INT, [_P, _P, _U32, _OUT]),
    "srsgpu_uci_decoder_plan_execute": (_INT, [_P, _P, _P, _P, _P, _P, _P]),
    "srsgpu_uci_decoder_plan_destroy": (None, [_P]),
    "srsgpu_uci_polar_decoder_plan_create": (_INT, [_P, _P, _U32, _OUT]),
    "srsgpu_uci_polar_decoder_plan_execute": (_INT, [_P, _P, _P, _P, _P, _P, _P]),
    "srsgpu_uci_polar_decoder_plan_destroy": (None, [_P]),
    "srsgpu_pusch_decoder_plan_create": (_INT, [_P, _INT, _P, _U32, _OUT]),
    "srsgpu_pusch_decoder_plan_nof_codeblocks": (_U32, [_P]),
    "srsgpu_pusch_decoder_plan_decoder_input_llrs": (_U64, [_P]),
    "srsgpu_pusch_decoder_plan_execute": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "srsgpu_pusch_decoder_plan_execute_arena": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "srsgpu_pusch_decoder_plan_assemble": (_INT, [_P, _P, _P, _P, _P, _P]),
    "srsgpu_pusch_decoder_plan_destroy": (None, [_P]),
    "srsgpu_pusch_decoder_plan_enable_timing": (_INT, [_P, _INT]),
    "srsgpu_pusch_decoder_plan_stage_times": (_INT, [_P, _P, _U32_OUT]),
    "srsgpu_harq_copy": (_INT, [_P, _INT, _P, _U32, _P, _P, _U32, _P]),
    "srsgpu_harq_copy_arenas": (_INT, [_P, _INT, _P, _U32, _P, _P, _U32, _P]),
    "srsgpu_copy_spans": (_INT, [_P, _U32, _U64, _P]),
    "srsgpu_merge_spans": (_INT, [_P, _U32, _U64, _U32, _P], OPTIONAL),
    "srsgpu_debug_live_device_buffers": (ctypes.c_int64, []),
}
# Entry points of the instrumented builds only (csrc/capi.cpp under LDPC_DEC_PROFILE, CHEST_PROFILE, ENC_PROFILE), which
# the header does not declare: the phase-profile tools under tools/ read their stamps through these.
DEBUG_PROTOTYPES = {
    "srsgpu_debug_decoder_profile": (_INT, [_P, _U32, _INT], OPTIONAL),
    "srsgpu_debug_chest_profile": (_INT, [_P, _U32], OPTIONAL),
    "srsgpu_debug_encoder_profile": (_INT, [_P, _U32], OPTIONAL),
}
# Every symbol include/srsgpu_phy.h declares (checked by tests/test_capi_symbols.py).
EXPORTED_SYMBOLS = sorted(PROTOTYPES)

_loaded = None


def load_library(path: str = LIB_PATH):
    """Loads libsrsgpu_phy.so (raises if it has not been built) and types every function of the prototype tables."""
    global _loaded
    if _loaded is not None:
        return _loaded
    if not os.path.exists(path):
        raise SrsGpuError(f"{path} not built: run srsran-5g_amd/build.sh (or __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes, *mark) in {**PROTOTYPES, **DEBUG_PROTOTYPES}.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if OPTIONAL in mark:
                continue
            raise SrsGpuError(f"{path} does not export {name}") from None
        fn.restype, fn.argtypes = restype, argtypes
    _loaded = lib
    return lib


def _lib():
    """The loaded library, loading it on first use: the one way every module of the package reaches it."""
    return load_library()


def live_device_buffers() -> int:
    """srsgpu_debug_live_device_buffers: device allocations the library's contexts and plans hold right now."""
    return int(_lib().srsgpu_debug_live_device_buffers())


def _check(rc: int):
    if rc != SRSGPU_OK:
        raise SrsGpuError(f"srsgpu error {rc}: {_lib().srsgpu_last_error().decode()}")


def _cptr(array):
    """A host ctypes array as the void pointer the C ABI takes."""
    return ctypes.cast(array, ctypes.c_void_p)


def _stage_times(prefix, handle, n):
    ms = (ctypes.c_float * n)()
    cnt = ctypes.c_uint32()
    _check(getattr(_lib(), prefix + "_stage_times")(handle, _cptr(ms), ctypes.byref(cnt)))
    return list(ms), cnt.value


def _stream_handle(stream) -> Optional[int]:
    if stream is None:
        return torch.cuda.current_stream().cuda_stream if torch is not None else None
    if hasattr(stream, "cuda_stream"):
        return stream.cuda_stream
    return int(stream)


def _dptr(t) -> int:
    if t is None:
        return None
    if not t.is_cuda:
        raise SrsGpuError("expected a device (HIP) tensor")
    if not t.is_contiguous():
        raise SrsGpuError("expected a contiguous tensor")
    return t.data_ptr()


def span_list(spans):
    """The srsgpu_copy_span array of spans = [(src tensor, dst tensor)] (contiguous device tensors of the same byte
    size, a multiple of 16) on the device, and its byte counts."""
    arr = np.zeros(len(spans), np.dtype([("src", "<u8"), ("dst", "<u8"), ("bytes", "<u8")]))
    for i, (a, b) in enumerate(spans):
        n = a.numel() * a.element_size()
        if n != b.numel() * b.element_size():
            raise SrsGpuError("copy_spans: source and destination sizes differ")
        arr[i] = (_dptr(a), _dptr(b), n)
    return torch.from_numpy(arr.view(np.uint8).copy()).to(spans[0][0].device), arr["bytes"]


def copy_spans(spans, stream=None):
    """srsgpu_copy_spans: spans = [(src tensor, dst tensor)], each a contiguous device tensor of the same byte size (a
    multiple of 16). One launch copies them all."""
    d, nbytes = span_list(spans)
    _check(_lib().srsgpu_copy_spans(_dptr(d), len(spans), int(nbytes.max()), _stream_handle(stream)))
    return d  # keep alive until the stream has run the copies


def merge_spans(spans, sentinel=0xFFFFFFFF, stream=None):
    """srsgpu_merge_spans: as copy_spans, but a 32-bit source word replaces the destination's only when it is not
    `sentinel` (the multi-device PDSCH batch's gather of sentinel-filled shard grids)."""
    d, nbytes = span_list(spans)
    _check(_lib().srsgpu_merge_spans(_dptr(d), len(spans), int(nbytes.max()), int(sentinel), _stream_handle(stream)))
    return d


# srsgpu_option (include/srsgpu_phy.h): kernel-selection options of a context, read at plan creation.
OPTION_DECODER_SPLIT = 1          # -1 auto (default), 0 one-row-pair kernel, 1 edge-split kernel
OPTION_DECODER_PAIRS = 2          # 0 (default) / 1: Z = 144..192 codeblocks two per workgroup
OPTION_DECODER_FUSED_DEMATCH = 3  # 1 (default) / 0: every codeblock through the separate rate dematcher
OPTION_ENCODER_BYTE_KERNEL = 4    # 0 (default) / 1: the byte-per-bit encoder kernel for every codeblock
OPTION_ENCODER_ZERO_OUTPUT = 5    # 0 (default) / 1: the encoder always clears its output first
OPTION_DECODER_TB_FOLD = 6        # 1 (default) / 0: single-codeblock TBs always through the separate TB stage
OPTION_DEMOD_GENERAL_PATHS = 7    # 0 (default) / 1: the demodulator's symbol search and LLR-by-LLR packing throughout
OPTION_DEFAULTS = {OPTION_DECODER_SPLIT: -1, OPTION_DECODER_PAIRS: 0, OPTION_DECODER_FUSED_DEMATCH: 1,
                   OPTION_ENCODER_BYTE_KERNEL: 0, OPTION_ENCODER_ZERO_OUTPUT: 0, OPTION_DECODER_TB_FOLD: 1,
                   OPTION_DEMOD_GENERAL_PATHS: 0}
# The keyword names of Context.options().
OPTION_BY_NAME = {"decoder_split": OPTION_DECODER_SPLIT, "decoder_pairs": OPTION_DECODER_PAIRS,
                  "decoder_fused_dematch": OPTION_DECODER_FUSED_DEMATCH,
                  "encoder_byte_kernel": OPTION_ENCODER_BYTE_KERNEL, "encoder_zero_output": OPTION_ENCODER_ZERO_OUTPUT,
                  "decoder_tb_fold": OPTION_DECODER_TB_FOLD, "demod_general_paths": OPTION_DEMOD_GENERAL_PATHS}


class _Handle:
    """Owner of one C-ABI object: `handle`, given back once to the library function named by `_destroy`."""
    handle = None
    _destroy = None

    def _create(self, fn: str, *args):
        """Runs the library's create function `fn` as fn(*args, &handle), checks its code and owns the handle."""
        h = ctypes.c_void_p()
        _check(getattr(_lib(), fn)(*args, ctypes.byref(h)))
        self.handle = h

    def close(self):
        if self.handle:
            getattr(_lib(), self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


class Context(_Handle):
    """srsgpu_context: one per GPU (one process per GPU)."""
    _destroy = "srsgpu_context_destroy"

    def __init__(self, device: int = 0):
        load_library()
        if torch is None or not torch.cuda.is_available():
            raise SrsGpuError("no HIP device available (the srsgpu kernels need an MI355X)")
        self.device = device
        self._create("srsgpu_context_create", device)

    def set_option(self, option: int, value: int) -> None:
        """srsgpu_context_set_option: plans created afterwards use it."""
        _check(_lib().srsgpu_context_set_option(self.handle, option, value))

    def get_option(self, option: int) -> int:
        v = ctypes.c_int()
        _check(_lib().srsgpu_context_get_option(self.handle, option, ctypes.byref(v)))
        return v.value

    def options(self, **kw):
        """Context manager: the given options (OPTION_* names without the prefix, lower case) while inside, the
        previous values after."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            keys = {OPTION_BY_NAME[k.lower()]: v for k, v in kw.items()}
            old = {k: self.get_option(k) for k in keys}
            try:
                for k, v in keys.items():
                    self.set_option(k, v)
                yield self
            finally:
                for k, v in old.items():
                    self.set_option(k, v)
        return scope()


class RePatternC(ctypes.Structure):
    """srsgpu_re_pattern (include/srsgpu_phy.h)."""
    _fields_ = [("crb_mask", ctypes.c_void_p), ("re_mask", ctypes.c_uint16), ("symbol_mask", ctypes.c_uint16)]


class AllocExtC(ctypes.Structure):
    """srsgpu_alloc_ext (include/srsgpu_phy.h): CRB mask, reserved RE patterns and per-PRG precoding."""
    _fields_ = [("crb_mask", ctypes.c_void_p), ("reserved", ctypes.c_void_p), ("nof_reserved", ctypes.c_uint32),
                ("prg_size", ctypes.c_uint16), ("nof_prg", ctypes.c_uint16), ("prg_weights", ctypes.c_void_p)]


def make_crb_mask_exts(dmrs, grid_nof_prb: int):
    """srsgpu_alloc_ext array carrying CRB masks only (PDSCH DM-RS, PUSCH demodulator / estimator: objects with a
    `crb_mask`; None when every allocation is contiguous) + keep-alive list."""
    if not any(d.crb_mask is not None for d in dmrs):
        return None, []
    exts = (AllocExtC * len(dmrs))()
    keep = []
    for i, d in enumerate(dmrs):
        if d.crb_mask is not None:
            c = np.zeros(grid_nof_prb, np.uint8)
            src = np.asarray(d.crb_mask, np.uint8)[:grid_nof_prb]
            c[:src.size] = src
            keep.append(c)
            exts[i].crb_mask = c.ctypes.data
    return exts, keep


make_dmrs_exts = make_crb_mask_exts
