#!/usr/bin/env python3
"""Generates the NZP-CSI-RS fixture tests/golden/csi_rs.npz from the reference's own nzp_csi_rs_generator_impl: its
pattern builder, pseudo-random generator, the generic channel precoder, the resource grid mapper and a resource grid.

Compiles tools/ref_csi_rs_driver.cpp together with the reference sources, where they lie in the reference tree (--ref,
or SRSRAN_REF), into a temporary directory outside this tree and runs it, with the flags of tools/gen_pdcch_golden.py
(-O3 -mavx2, no FMA: the precoder's complex products round every term). Nothing compiled and no reference text is kept:
only the recorded configurations and the grid words the reference wrote on a sentinel grid.

  --time   also times the reference generator on one host core over the batch of profiles/dl_signals.md.
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
import csi_rs_cases as C  # noqa: E402

UP = "lib/phy/upper/"
REF_SOURCES = (UP + "signal_processors/nzp_csi_rs_generator_impl.cpp", "lib/ran/csi_rs/csi_rs_pattern.cpp",
               "lib/ran/csi_rs/csi_rs_config_helpers.cpp", UP + "sequence_generators/pseudo_random_generator_impl.cpp",
               "lib/phy/support/resource_grid_mapper_impl.cpp", "lib/phy/support/resource_grid_impl.cpp",
               "lib/phy/support/resource_grid_writer_impl.cpp", "lib/phy/support/resource_grid_reader_impl.cpp",
               "lib/phy/support/re_pattern.cpp", "lib/phy/generic_functions/precoding/channel_precoder_generic.cpp",
               "lib/phy/generic_functions/precoding/channel_precoder_impl.cpp", "lib/srsvec/bit.cpp", "lib/srsvec/sc_prod.cpp",
               "lib/srsvec/conversion.cpp", "lib/srsvec/compare.cpp", "lib/srsvec/dot_prod.cpp")
HEADER_FORMAT = "<12IfI32f2I"


def build_driver(ref, tmp):
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17", "-O3", "-DNDEBUG", "-DFMT_HEADER_ONLY", "-DASSERTS_ENABLED=0", "-mavx2", f"-I{ref}/include",
             f"-I{ref}/external/fmt/include", f"-I{ref}/external", f"-I{ref}"]
    sources = [os.path.join(ROOT, "tools", "ref_csi_rs_driver.cpp")] + [os.path.join(ref, s) for s in REF_SOURCES]
    objects = [os.path.join(tmp, f"{i}.o") for i in range(len(sources))]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(lambda so: subprocess.run([cxx] + flags + ["-c", so[0], "-o", so[1]], check=True),
                      zip(sources, objects)))
    exe = os.path.join(tmp, "ref_csi_rs_driver")
    subprocess.run([cxx, "-o", exe] + objects, check=True)
    return exe


def write_cases(path, cases):
    assert struct.calcsize(HEADER_FORMAT) == 192
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for cfg in cases:
            ports = C.ROW_PORTS[cfg["row"]]
            w = np.zeros((4, 4), np.complex64)
            w[:ports, :ports] = cfg["weights"]
            f.write(struct.pack(
                HEADER_FORMAT, cfg["numerology"], cfg["n_slot"], cfg["cp"], cfg["start_rb"], cfg["nof_rb"], cfg["row"],
                cfg["k_ref"], cfg["symbol_l0"], cfg["symbol_l1"], cfg["cdm"], cfg["freq_density"], cfg["scrambling_id"],
                float(cfg["amplitude"]), ports, *w.view(np.float32).ravel().tolist(), cfg["grid_nof_prb"],
                cfg["grid_nof_ports"]))


def ref_process(exe, tmp, cases, repeats=0):
    """-> per case the written rows (port, symbol, subcarrier, word)[, ns per pass]."""
    fin, fout = os.path.join(tmp, "cases.in"), os.path.join(tmp, "cases.out")
    write_cases(fin, cases)
    res = subprocess.run([exe, "process", fin, fout] + ([str(repeats)] if repeats else []), check=True,
                         capture_output=True, text=True)
    raw = open(fout, "rb").read()
    out, pos = [], 0
    for _ in cases:
        (m,) = struct.unpack_from("<I", raw, pos)
        out.append(np.frombuffer(raw, np.uint32, 4 * m, pos + 4).reshape(m, 4))
        pos += 4 + 16 * m
    assert pos == len(raw)
    return (out, float(res.stdout.split()[1])) if repeats else out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ref", default=os.environ.get("SRSRAN_REF", "/root/reference"))
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="ref_csi_rs_")
    try:
        exe = build_driver(args.ref, tmp)
        cases = C.golden_generator_cases(np.random.default_rng(20263))
        res = ref_process(exe, tmp, cases)
        rows = np.concatenate(res)
        os.makedirs(os.path.dirname(C.GOLDEN), exist_ok=True)
        np.savez_compressed(
            C.GOLDEN, cfg=np.array([[cfg[k] for k in C.CFG_INT_KEYS] for cfg in cases], np.int64),
            amplitude=np.array([cfg["amplitude"] for cfg in cases], np.float32),
            weights=np.concatenate([np.asarray(cfg["weights"], np.complex64).ravel() for cfg in cases]),
            nof_written=np.array([r.shape[0] for r in res], np.uint32), w_port=rows[:, 0].astype(np.uint8),
            w_symbol=rows[:, 1].astype(np.uint8), w_subcarrier=rows[:, 2].astype(np.uint16),
            w_word=rows[:, 3].astype(np.uint32))
        size = os.path.getsize(C.GOLDEN)
        assert size < 243 << 10, size
        print(f"wrote {C.GOLDEN}: {len(cases)} signals, {rows.shape[0]} grid words, {size} bytes")
        if args.time:
            batch = C.bench_cases(np.random.default_rng(7))
            _, ns = ref_process(exe, tmp, batch, repeats=50)
            print(f"reference nzp_csi_rs_generator_impl, one core: {len(batch)} signals (32 slots x two row-1 symbols and "
                  f"one row 4, 273 PRB): {ns / 1e3:.1f} us per pass")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
