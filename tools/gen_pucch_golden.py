#!/usr/bin/env python3
"""Generates the PUCCH fixture tests/golden/pucch_detector.npz from the reference's own pucch_detector_format0 and
pucch_detector_format1 with their low-PAPR sequence collection, pseudo-random generator and a resource grid (the
12-point transforms are the driver's own direct sums: the reference's generic DFT has no size 12).

Compiles tools/ref_pucch_driver.cpp together with the reference sources, where they lie in the reference tree (--ref,
or SRSRAN_REF), into a temporary directory outside this tree and runs it. Nothing compiled and no reference text is
kept: only the recorded inputs (the allocation's REs as bf16 words, not whole grids) and outputs.

  --time   also times the reference detectors on one host core over the fixture's cases (profiles/pucch_detector.md).
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
import pucch_cases as C  # noqa: E402

UP = "lib/phy/upper/"
REF_SOURCES = (UP + "channel_processors/pucch/pucch_detector_format0.cpp",
               UP + "channel_processors/pucch/pucch_detector_format1.cpp",
               UP + "sequence_generators/low_papr_sequence_collection_impl.cpp",
               UP + "sequence_generators/low_papr_sequence_generator_impl.cpp",
               UP + "sequence_generators/pseudo_random_generator_impl.cpp",
               "lib/phy/support/resource_grid_impl.cpp",
               "lib/phy/support/resource_grid_writer_impl.cpp", "lib/phy/support/resource_grid_reader_impl.cpp",
               "lib/srsvec/bit.cpp", "lib/srsvec/sc_prod.cpp", "lib/srsvec/conversion.cpp", "lib/srsvec/compare.cpp",
               "lib/srsvec/dot_prod.cpp", "lib/srsvec/prod.cpp", "lib/srsvec/add.cpp", "lib/srsvec/subtract.cpp",
               "lib/srsvec/modulus_square.cpp", "lib/support/math_utils.cpp")
F0_RESULT = np.dtype([("status", "<u4"), ("nof_sr", "<u4"), ("sr", "<u4"), ("nof_harq_ack", "<u4"), ("harq_ack", "<u4", (2,)),
                      ("sinr_db", "<f4"), ("epre_db", "<f4"), ("rsrp_db", "<f4")])
F1_RESULT = np.dtype([("status", "<u4"), ("harq_ack", "<u4", (2,)), ("metric", "<f4"), ("epre_db", "<f4"),
                      ("rsrp_db", "<f4"), ("sinr_db", "<f4")])


def build_driver(ref, tmp):
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17", "-O3", "-DNDEBUG", "-DFMT_HEADER_ONLY", "-DASSERTS_ENABLED=0", "-mavx2", "-mfma", f"-I{ref}/include",
             f"-I{ref}/external/fmt/include", f"-I{ref}/external", f"-I{ref}"]
    sources = [os.path.join(ROOT, "tools", "ref_pucch_driver.cpp")] + [os.path.join(ref, s) for s in REF_SOURCES]
    objects = [os.path.join(tmp, f"{i}.o") for i in range(len(sources))]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(lambda so: subprocess.run([cxx] + flags + ["-c", so[0], "-o", so[1]], check=True),
                      zip(sources, objects)))
    exe = os.path.join(tmp, "ref_pucch_driver")
    subprocess.run([cxx, "-o", exe] + objects, check=True)
    return exe


def write_cases(path, f0, f1):
    with open(path, "wb") as f:
        f.write(struct.pack("<2I", len(f0), len(f1)))
        for c, words, *_ in f0:
            ports = (list(c["ports"]) + [0] * 4)[:4]
            f.write(struct.pack("<17I", c["slot_index"], c["numerology"], c["cp_extended"], c["starting_prb"],
                                c["second_hop_prb"], c["start_symbol"], c["nof_symbols"], c["initial_cyclic_shift"],
                                c["n_id"], c["nof_harq_ack"], c["sr_opportunity"], len(c["ports"]), *ports,
                                c["grid_nof_ports"]))
            f.write(np.ascontiguousarray(words, np.uint32).tobytes())
        for c, words, *_ in f1:
            f.write(struct.pack("<10I", c["slot_index"], c["numerology"], c["cp_extended"], c["starting_prb"],
                                c["second_hop_prb"], c["start_symbol"], c["nof_symbols"], c["n_id"], c["nof_ports"],
                                len(c["entries"])))
            f.write(np.asarray(c["entries"], np.uint32).tobytes())
            f.write(np.ascontiguousarray(words, np.uint32).tobytes())


def ref_detect(exe, tmp, f0, f1, repeats=0):
    """-> (Format 0 results, per Format 1 case (noise variance, results))[, ns per pass]."""
    fin, fout = os.path.join(tmp, "cases.in"), os.path.join(tmp, "cases.out")
    write_cases(fin, f0, f1)
    res = subprocess.run([exe, fin, fout] + ([str(repeats)] if repeats else []), check=True, capture_output=True, text=True)
    raw = open(fout, "rb").read()
    r0 = np.frombuffer(raw, F0_RESULT, len(f0), 0)
    pos, r1 = len(f0) * F0_RESULT.itemsize, []
    for c, *_ in f1:
        noise = np.frombuffer(raw, np.float32, 1, pos)[0]
        rows = np.frombuffer(raw, F1_RESULT, len(c["entries"]), pos + 4)
        pos += 4 + rows.nbytes
        r1.append((noise, rows))
    assert pos == len(raw)
    return (r0, r1, float(res.stdout.split()[1])) if repeats else (r0, r1)


def ref_ncs(exe, tmp, queries):
    fin, fout = os.path.join(tmp, "ncs.in"), os.path.join(tmp, "ncs.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(queries)))
        f.write(np.asarray(queries, np.uint32).tobytes())
    subprocess.run([exe, "ncs", fin, fout], check=True)
    out = np.fromfile(fout, np.uint32)
    return out[: len(queries)], out[len(queries):]


def sent_code(sent):
    """What a PUCCH sent: -1 nothing, else its bits as b0 | b1 << 1 (no bits: 0)."""
    return -1 if sent is None else sum(int(b) << i for i, b in enumerate(sent))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ref", default=os.environ.get("SRSRAN_REF"), required="SRSRAN_REF" not in os.environ,
                    help="the reference source tree (default: $SRSRAN_REF)")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--seed", type=int, default=20266)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="ref_pucch_")
    try:
        exe = build_driver(args.ref, tmp)
        f0, f1 = C.golden_generator_cases(np.random.default_rng(args.seed))
        r0, r1 = ref_detect(exe, tmp, f0, f1)
        queries = sorted({(c["n_id"], C.nsymb_per_slot(c["cp_extended"]), c["slot_index"], c["start_symbol"] + i)
                          for c, *_ in list(f0) + list(f1) for i in range(c["nof_symbols"])})
        alpha, ncs = ref_ncs(exe, tmp, queries)
        f0_cfg, f1_cfg = C.cfg_rows(f0, f1)
        rows1 = np.concatenate([r[1] for r in r1])
        os.makedirs(os.path.dirname(C.GOLDEN), exist_ok=True)
        np.savez_compressed(
            C.GOLDEN, f0_cfg=f0_cfg.astype(np.int32), f0_words=np.concatenate([w.ravel() for _, w, *_ in f0]),
            f0_status=r0["status"].astype(np.uint8), f0_bits=np.stack([r0["sr"], r0["harq_ack"][:, 0], r0["harq_ack"][:, 1]], 1).astype(np.uint8),
            f0_nof_bits=np.stack([r0["nof_sr"], r0["nof_harq_ack"]], 1).astype(np.uint8),
            f0_sinr_db=r0["sinr_db"], f0_epre_db=r0["epre_db"], f0_rsrp_db=r0["rsrp_db"],
            f0_sent=np.array([-1 if s is None else s[0] | (sent_code(s[1]) << 1) for _, _, s, _ in f0], np.int8),
            f0_class=np.array([k for *_, k in f0], np.uint8),
            f1_cfg=f1_cfg.astype(np.int32), f1_entries=np.concatenate([np.asarray(c["entries"], np.uint8).reshape(-1, 3) for c, *_ in f1]),
            f1_words=np.concatenate([w.ravel() for _, w, *_ in f1]), f1_noise_var=np.array([r[0] for r in r1], np.float32),
            f1_status=rows1["status"].astype(np.uint8), f1_bits=rows1["harq_ack"].astype(np.uint8), f1_metric=rows1["metric"],
            f1_epre_db=rows1["epre_db"], f1_rsrp_db=rows1["rsrp_db"], f1_sinr_db=rows1["sinr_db"],
            f1_sent=np.array([sent_code(s) for _, _, sent, _ in f1 for s in sent], np.int8),
            f1_class=np.array([k for *_, k in f1], np.uint8),
            ncs_query=np.asarray(queries, np.uint16), ncs_value=ncs.astype(np.uint8), ncs_alpha=alpha.astype(np.uint8))
        size = os.path.getsize(C.GOLDEN)
        assert size < 1 << 20, size
        print(f"wrote {C.GOLDEN}: {len(f0)} Format 0 PDUs, {len(f1)} Format 1 resources with {rows1.size} entries, "
              f"{len(queries)} n_cs values, {size} bytes")
        if args.time:
            _, _, ns = ref_detect(exe, tmp, f0, f1, repeats=50)
            print(f"reference detectors, one core: {len(f0)} Format 0 PDUs and {len(f1)} Format 1 resources "
                  f"({rows1.size} entries): {ns / 1e3:.1f} us per pass")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
