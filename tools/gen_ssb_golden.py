#!/usr/bin/env python3
"""Generates the SS/PBCH block fixture tests/golden/ssb.npz from the reference's own ssb_processor_impl: its PBCH
encoder and modulator, the PBCH DM-RS, PSS and SSS processors, the LUT modulation mapper and a resource grid.

Compiles tools/ref_ssb_driver.cpp together with the reference sources, where they lie in the reference tree (--ref, or
SRSRAN_REF), into a temporary directory outside this tree and runs it, with the flags of tools/gen_pdcch_golden.py
(-O3 -mavx2, no FMA). Nothing compiled and no reference text is kept: only the recorded PDU fields, the reference's
l_start / k_start, its 864 rate-matched bits and the grid words it wrote on a sentinel grid.

  --time   also times the reference processor on one host core over the fixture's blocks (profiles/dl_signals.md).
"""
import argparse
import concurrent.futures
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssb_cases as C  # noqa: E402

UP = "lib/phy/upper/"
POLAR = UP + "channel_coding/polar/"
REF_SOURCES = (UP + "channel_processors/ssb/ssb_processor_impl.cpp", UP + "channel_processors/ssb/pbch_encoder_impl.cpp",
               UP + "channel_processors/ssb/pbch_modulator_impl.cpp", UP + "signal_processors/dmrs_pbch_processor_impl.cpp",
               UP + "signal_processors/pss_processor_impl.cpp", UP + "signal_processors/sss_processor_impl.cpp",
               POLAR + "polar_code_impl.cpp", POLAR + "polar_encoder_impl.cpp", POLAR + "polar_allocator_impl.cpp",
               POLAR + "polar_rate_matcher_impl.cpp", POLAR + "polar_interleaver_impl.cpp",
               UP + "channel_coding/crc_calculator_generic_impl.cpp", UP + "channel_modulation/modulation_mapper_lut_impl.cpp",
               UP + "sequence_generators/pseudo_random_generator_impl.cpp", "lib/phy/support/resource_grid_impl.cpp",
               "lib/phy/support/resource_grid_writer_impl.cpp", "lib/phy/support/resource_grid_reader_impl.cpp",
               "lib/srsvec/bit.cpp", "lib/srsvec/sc_prod.cpp", "lib/srsvec/prod.cpp", "lib/srsvec/conversion.cpp",
               "lib/srsvec/compare.cpp", "lib/srsvec/dot_prod.cpp")
HEADER_FORMAT = "<10IfI4B24B2I"


def build_driver(ref, tmp):
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17", "-O3", "-DNDEBUG", "-DFMT_HEADER_ONLY", "-DASSERTS_ENABLED=0", "-mavx2", f"-I{ref}/include",
             f"-I{ref}/external/fmt/include", f"-I{ref}/external", f"-I{ref}", f"-I{ref}/lib/phy/upper/channel_coding"]
    sources = [os.path.join(ROOT, "tools", "ref_ssb_driver.cpp")] + [os.path.join(ref, s) for s in REF_SOURCES]
    objects = [os.path.join(tmp, f"{i}.o") for i in range(len(sources))]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(lambda so: subprocess.run([cxx] + flags + ["-c", so[0], "-o", so[1]], check=True),
                      zip(sources, objects)))
    exe = os.path.join(tmp, "ref_ssb_driver")
    subprocess.run([cxx, "-o", exe] + objects, check=True)
    return exe


def write_cases(path, cases):
    assert struct.calcsize(HEADER_FORMAT) == 84
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for cfg in cases:
            ports = list(cfg["ports"]) + [0] * (4 - len(cfg["ports"]))
            f.write(struct.pack(
                HEADER_FORMAT, cfg["phys_cell_id"], cfg["ssb_idx"], cfg["L_max"], cfg["pattern_case"], cfg["common_scs"],
                cfg["offset_to_pointA"], cfg["subcarrier_offset"], cfg["sfn"], cfg["slot_index"], cfg["hrf"],
                float(cfg["beta_pss_dB"]), len(cfg["ports"]), *ports, *[int(b) for b in cfg["payload"]],
                cfg["grid_nof_prb"], cfg["grid_nof_ports"]))


def ref_process(exe, tmp, cases, repeats=0):
    """-> per case (l_start, k_start, rate-matched bits, PSS amplitude, written rows)[, ns per pass]."""
    fin, fout = os.path.join(tmp, "cases.in"), os.path.join(tmp, "cases.out")
    write_cases(fin, cases)
    res = subprocess.run([exe, "process", fin, fout] + ([str(repeats)] if repeats else []), check=True,
                         capture_output=True, text=True)
    raw = open(fout, "rb").read()
    out, pos = [], 0
    for _ in cases:
        l_start, k_start = struct.unpack_from("<2I", raw, pos)
        enc = np.frombuffer(raw, np.uint8, C.E_BITS, pos + 8)
        pos += 8 + C.E_BITS
        (amp,) = struct.unpack_from("<f", raw, pos)
        (m,) = struct.unpack_from("<I", raw, pos + 4)
        rows = np.frombuffer(raw, np.uint32, 4 * m, pos + 8).reshape(m, 4)
        pos += 8 + 16 * m
        out.append((l_start, k_start, enc, amp, rows))
    assert pos == len(raw)
    return (out, float(res.stdout.split()[1])) if repeats else out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ref", default=os.environ.get("SRSRAN_REF", "/root/reference"))
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="ref_ssb_")
    try:
        exe = build_driver(args.ref, tmp)
        cases = C.golden_generator_cases(np.random.default_rng(20264))
        res = ref_process(exe, tmp, cases)
        rows = np.concatenate([r[4] for r in res])
        ports = np.zeros((len(cases), 4), np.uint8)
        for i, cfg in enumerate(cases):
            ports[i, : len(cfg["ports"])] = cfg["ports"]
        os.makedirs(os.path.dirname(C.GOLDEN), exist_ok=True)
        np.savez_compressed(
            C.GOLDEN, cfg=np.array([[cfg[k] for k in C.CFG_INT_KEYS] for cfg in cases], np.int64),
            beta_pss_dB=np.array([cfg["beta_pss_dB"] for cfg in cases], np.float32),
            pss_amplitude=np.array([r[3] for r in res], np.float32), ports=ports,
            nof_ports=np.array([len(cfg["ports"]) for cfg in cases], np.uint8),
            payload=np.array([cfg["payload"] for cfg in cases], np.uint8),
            l_start=np.array([r[0] for r in res], np.uint8), k_start=np.array([r[1] for r in res], np.uint16),
            encoded=np.packbits(np.array([r[2] for r in res], np.uint8), axis=1),
            nof_written=np.array([r[4].shape[0] for r in res], np.uint32), w_port=rows[:, 0].astype(np.uint8),
            w_symbol=rows[:, 1].astype(np.uint8), w_subcarrier=rows[:, 2].astype(np.uint16),
            w_word=rows[:, 3].astype(np.uint32))
        size = os.path.getsize(C.GOLDEN)
        assert size < 243 << 10, size
        print(f"wrote {C.GOLDEN}: {len(cases)} blocks, {rows.shape[0]} grid words, {size} bytes")
        if args.time:
            _, ns = ref_process(exe, tmp, cases, repeats=200)
            print(f"reference ssb_processor_impl, one core: the fixture's {len(cases)} blocks "
                  f"({sum(len(c['ports']) for c in cases)} port writes): {ns / 1e3:.1f} us per pass")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
