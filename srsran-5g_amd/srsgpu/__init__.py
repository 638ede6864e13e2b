"""srsgpu — Python host binding of libsrsgpu_phy.so (the MI355X 5G NR PHY kernels), over its C ABI
(include/srsgpu_phy.h).

The Python side mirrors the srsRAN interfaces it replaces (names, argument meaning and error behaviour) so the parity
tests read like the reference's own tests:

  * ``LdpcDecoder.decode(llrs, cfg)``  <->  srsran::ldpc_decoder::decode()
    (include/srsran/phy/upper/channel_coding/ldpc/ldpc_decoder.h:72)

Device memory and streams come from PyTorch (ROCm); PyTorch is plumbing only — every codeblock is processed by the
HIP kernels in libsrsgpu_phy.so. There is no CPU fallback: if the library or a HIP device is missing, the calls raise.

The package is one module per channel over _abi (the library, its prototype table, the context and the handle
plumbing); every public name of those modules is an attribute of the package, which is how callers use them.
"""
try:  # Import torch first: it loads its own libamdhip64.so.7, which our library then shares (one HIP runtime).
    import torch
except ImportError:  # pragma: no cover - torch is part of the image
    torch = None

from ._abi import *  # noqa: E402,F401,F403
from ._abi import _dptr  # noqa: E402,F401
from .ldpc import *  # noqa: E402,F401,F403
from .pdsch import *  # noqa: E402,F401,F403
from .pusch import *  # noqa: E402,F401,F403
from .uci import *  # noqa: E402,F401,F403
from .pucch import *  # noqa: E402,F401,F403
from .dl_signals import *  # noqa: E402,F401,F403
from .prach import *  # noqa: E402,F401,F403
from .srs import *  # noqa: E402,F401,F403
from .ofdm import *  # noqa: E402,F401,F403
