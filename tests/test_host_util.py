"""The host code that the control-channel plans share (srsran-5g_amd/csrc/host_util.h) in a stand-alone sanitizer
build: the Gold sequence and the roots of unity against numpy, the overlap search, the shared refusals, the UCI rules.
No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np

import pucch_f34_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GOLD_C_INITS = (0, 1, (1 << 31) - 1, 0x4601 * (1 << 15) + 500)
GOLD_FIRSTS = (0, 1, 31, 32, 33, 1599)
GOLD_COUNTS = (1, 8, 40)  # 8 from 31 and 40 from anywhere cross a word boundary
ROOT_SIZES = (12, 128, 192)


def test_host_code(tmp_path):
    """tools/host_util_check.cpp, built with the address and undefined-behaviour sanitizers: gold_bits against the
    restatement's Gold sequence (tests/pucch_f34_cases.py _gold) for every (c_init, first, count) above, gold_words
    against the packed gold_bits, unit_roots against numpy's cos / sin in double, and the hand-made part."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "host_util_check")
    csrc = os.path.join(ROOT, "srsran-5g_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{csrc}", "-o", exe, os.path.join(ROOT, "tools", "host_util_check.cpp")], check=True)
    dump = tmp_path / "cases.bin"
    with open(dump, "wb") as f:
        f.write(struct.pack("<I", len(GOLD_C_INITS) * len(GOLD_FIRSTS) * len(GOLD_COUNTS)))
        for c_init in GOLD_C_INITS:
            bits = np.asarray(C._gold(c_init, max(GOLD_FIRSTS) + max(GOLD_COUNTS))).astype(np.uint8)
            for first in GOLD_FIRSTS:
                for count in GOLD_COUNTS:
                    f.write(struct.pack("<3I", c_init, first, count))
                    f.write(bits[first: first + count].tobytes())
        f.write(struct.pack("<I", len(ROOT_SIZES)))
        for n in ROOT_SIZES:
            a = 2 * np.pi * np.arange(n, dtype=np.float64) / n
            f.write(struct.pack("<I", n))
            f.write(np.stack([np.cos(a), np.sin(a)], 1).astype(np.float64).tobytes())
    res = subprocess.run([exe, str(dump)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"{len(GOLD_C_INITS) * len(GOLD_FIRSTS) * len(GOLD_COUNTS)} Gold ranges, {len(ROOT_SIZES)} root tables" in res.stdout
    assert "\n0 failures" in res.stdout
