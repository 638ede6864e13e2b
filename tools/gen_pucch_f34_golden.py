#!/usr/bin/env python3
"""Generates the PUCCH Format 3 / 4 fixture tests/golden/pucch_f34.npz from the reference's own receive path:
dmrs_pucch_estimator_formats3_4 over port_channel_estimator_average_impl (mean smoothing, average in time, no CFO
compensation), pucch_demodulator_format3 / format4 over the generic ZF equaliser, transform_precoder_dft_impl (over an
exact direct DFT) and the demodulation mapper, and uci_decoder_impl.

Compiles tools/ref_pucch_f34_driver.cpp together with the reference sources, where they lie in the reference tree
(--ref, or SRSRAN_REF), into a temporary directory outside this tree and runs it. Nothing compiled and no reference text
is kept: only the recorded inputs (the allocation's REs as bf16 words, not whole grids) and outputs, the reference's
DM-RS symbol masks and its Format 4 orthogonal sequences as data.

A case is `decidable` when the reference's decoder gives the same bits and status from the reference's LLRs and from
the LLRs of the float64 restatement (tests/pucch_f34_cases.py), which may lie one step apart. The tool refuses to write
a fixture in which fewer than 95 % of the cases are decidable or a sent high-SNR case is not.

  --time   also times the reference path on one host core over the fixture's cases, over a 32-slot batch of 8 PDUs
           per slot and over the largest PDU (profiles/pucch_formats_3_4.md).
"""
import argparse
import concurrent.futures
import glob
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pucch_f34_cases as C  # noqa: E402

UP, CODING = "lib/phy/upper/", "lib/phy/upper/channel_coding/"
REF_SOURCES = (UP + "signal_processors/pucch/dmrs_pucch_estimator_formats3_4.cpp",
               UP + "signal_processors/port_channel_estimator_average_impl.cpp",
               UP + "signal_processors/port_channel_estimator_helpers.cpp",
               UP + "channel_processors/pucch/pucch_demodulator_format3.cpp",
               UP + "channel_processors/pucch/pucch_demodulator_format4.cpp",
               UP + "channel_processors/uci/uci_decoder_impl.cpp",
               UP + "equalization/channel_equalizer_generic_impl.cpp",
               UP + "channel_modulation/demodulation_mapper_impl.cpp", UP + "channel_modulation/demodulation_mapper_qpsk.cpp",
               UP + "channel_modulation/demodulation_mapper_qam16.cpp", UP + "channel_modulation/demodulation_mapper_qam64.cpp",
               UP + "channel_modulation/demodulation_mapper_qam256.cpp",
               UP + "sequence_generators/pseudo_random_generator_impl.cpp",
               UP + "sequence_generators/low_papr_sequence_generator_impl.cpp", UP + "log_likelihood_ratio.cpp",
               CODING + "polar/polar_code_impl.cpp", CODING + "polar/polar_decoder_impl.cpp",
               CODING + "polar/polar_encoder_impl.cpp", CODING + "polar/polar_rate_dematcher_impl.cpp",
               CODING + "polar/polar_deallocator_impl.cpp", CODING + "short/short_block_detector_impl.cpp",
               CODING + "short/short_block_encoder_impl.cpp", CODING + "crc_calculator_generic_impl.cpp",
               "lib/phy/generic_functions/transform_precoding/transform_precoder_dft_impl.cpp",
               "lib/phy/support/interpolator/interpolator_linear_impl.cpp",
               "lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.cpp",
               "lib/phy/generic_functions/dft_processor_generic_impl.cpp", "lib/phy/support/resource_grid_impl.cpp",
               "lib/phy/support/resource_grid_writer_impl.cpp", "lib/phy/support/resource_grid_reader_impl.cpp",
               "lib/support/math_utils.cpp")
HEADER_FIELDS = ("format", "slot_index", "numerology", "cp_extended", "starting_prb", "second_hop_prb", "nof_prb",
                 "start_symbol", "nof_symbols", "additional_dmrs", "pi2_bpsk", "occ_length", "occ_index", "rnti",
                 "n_id_scrambling", "n_id_hopping")


def build_driver(ref, tmp):
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17", "-O3", "-DNDEBUG", "-DFMT_HEADER_ONLY", "-DASSERTS_ENABLED=0", "-mavx2", "-mfma", f"-I{ref}/include",
             f"-I{ref}/external/fmt/include", f"-I{ref}/external", f"-I{ref}", f"-I{ref}/lib/phy/upper/channel_coding"]
    sources = [os.path.join(ROOT, "tools", "ref_pucch_f34_driver.cpp")] + [os.path.join(ref, s) for s in REF_SOURCES]
    sources += sorted(glob.glob(os.path.join(ref, "lib", "srsvec", "*.cpp")))
    objects = [os.path.join(tmp, f"{i}.o") for i in range(len(sources))]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(lambda so: subprocess.run([cxx] + flags + ["-c", so[0], "-o", so[1]], check=True),
                      zip(sources, objects)))
    exe = os.path.join(tmp, "ref_pucch_f34_driver")
    subprocess.run([cxx, "-o", exe] + objects, check=True)
    return exe


def header_row(cfg):
    ports = (list(cfg["ports"]) + [0] * 4)[:4]
    return [cfg[k] for k in HEADER_FIELDS] + [len(cfg["ports"]), *ports, cfg["grid_nof_ports"], cfg["grid_nof_prb"],
                                               cfg["nof_uci_bits"]]


def ref_process(exe, tmp, cases, repeats=0):
    """cases: (cfg, words, ...) -> list of dicts (llrs, noise_var, rsrp, epre, ta, cfo_hz per port, csi = the combined
    (EPRE dB, RSRP dB, SINR dB, time alignment, CFO), bits, status)[, ns]."""
    fin, fout = os.path.join(tmp, "cases.in"), os.path.join(tmp, "cases.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for cfg, words, *_ in cases:
            f.write(struct.pack("<24I", *header_row(cfg)))
            f.write(np.ascontiguousarray(words, np.uint32).tobytes())
    res = subprocess.run([exe, "process", fin, fout] + ([str(repeats)] if repeats else []), check=True,
                         capture_output=True, text=True)
    raw = open(fout, "rb").read()
    port = np.dtype([("noise_var", "<f4"), ("rsrp", "<f4"), ("epre", "<f4"), ("ta", "<f8"), ("cfo_hz", "<f4")])
    assert port.itemsize == 24
    out, pos = [], 0
    for cfg, *_ in cases:
        n, P, a = C.nof_llrs(cfg), len(cfg["ports"]), cfg["nof_uci_bits"]
        llrs = np.frombuffer(raw, np.int8, n, pos).copy()
        rows = np.frombuffer(raw, port, P + 1, pos + n)  # the last row: the combined channel state information
        bits = np.frombuffer(raw, np.uint8, a + 1, pos + n + rows.nbytes)
        pos += n + rows.nbytes + a + 1
        rows, csi = rows[:P], rows[P]
        out.append(dict(csi=tuple(float(csi[k]) for k in ("noise_var", "rsrp", "epre", "ta", "cfo_hz")),  # EPRE, RSRP, SINR dB; s; Hz
                        llrs=llrs, noise_var=rows["noise_var"].copy(), rsrp=rows["rsrp"].copy(), epre=rows["epre"].copy(),
                        ta=rows["ta"].copy(), cfo_hz=rows["cfo_hz"].copy(), bits=bits[:a].copy(), status=int(bits[a])))
    assert pos == len(raw)
    return (out, float(res.stdout.split()[1])) if repeats else out


def ref_decode(exe, tmp, fields):
    """fields: (llrs, A, pi2_bpsk) -> list of (bits, status) of the reference's uci_decoder."""
    fin, fout = os.path.join(tmp, "dec.in"), os.path.join(tmp, "dec.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(fields)))
        for llrs, a, pi2 in fields:
            f.write(struct.pack("<III", a, len(llrs), pi2))
            f.write(np.ascontiguousarray(llrs, np.int8).tobytes())
    subprocess.run([exe, "decode", fin, fout], check=True)
    raw = np.fromfile(fout, np.uint8)
    out, pos = [], 0
    for _, a, _ in fields:
        out.append((raw[pos: pos + a].copy(), int(raw[pos + a])))
        pos += a + 1
    assert pos == raw.size
    return out


def ref_tables(exe, tmp):
    """(DM-RS masks (11, 2, 2) uint16 by nof_symbols - 4, hopping, additional_dmrs; w rows (6, 12) complex64: length 2
    n = 0, 1, then length 4 n = 0..3)."""
    fout = os.path.join(tmp, "tables.out")
    subprocess.run([exe, "tables", fout], check=True)
    raw = open(fout, "rb").read()
    masks = np.frombuffer(raw, "<u2", 44).reshape(11, 2, 2).copy()
    w = np.frombuffer(raw, "<f4", 6 * 12 * 2, 88).reshape(6, 12, 2)
    return masks, (w[..., 0] + 1j * w[..., 1]).astype(np.complex64)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ref", default=os.environ.get("SRSRAN_REF"), required="SRSRAN_REF" not in os.environ,
                    help="the reference source tree (default: $SRSRAN_REF)")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--seed", type=int, default=20343)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="ref_pucch_f34_")
    try:
        exe = build_driver(args.ref, tmp)
        masks, w_rows = ref_tables(exe, tmp)
        cases = C.golden_generator_cases(np.random.default_rng(args.seed))
        ref = ref_process(exe, tmp, cases)
        restated = [C.restate(cfg, C.grid_of(cfg, words)) for cfg, words, *_ in cases]
        again = ref_decode(exe, tmp, [(r["llrs"], cfg["nof_uci_bits"], cfg["pi2_bpsk"]) for r, (cfg, *_) in zip(restated, cases)])
        decidable = [int(np.array_equal(b, r["bits"]) and s == r["status"]) for (b, s), r in zip(again, ref)]
        share = sum(decidable) / len(cases)
        high = [d for d, (*_, b, k) in zip(decidable, cases) if k == C.CLASS_HIGH and b is not None]
        assert share >= 0.95 and all(high), (share, high.count(0))
        pad = lambda key, dt: np.array([list(r[key]) + [0] * (4 - len(r[key])) for r in ref], dt)  # noqa: E731
        os.makedirs(os.path.dirname(C.GOLDEN), exist_ok=True)
        np.savez_compressed(
            C.GOLDEN, cfg=np.array([C.cfg_row(c) for c, *_ in cases], np.int32),
            words=np.concatenate([np.asarray(w, np.uint32).ravel() for _, w, *_ in cases]),
            llrs=np.concatenate([r["llrs"] for r in ref]), noise_var=pad("noise_var", np.float32),
            rsrp=pad("rsrp", np.float32), epre=pad("epre", np.float32), ta=pad("ta", np.float64),
            cfo_hz=pad("cfo_hz", np.float32), bits=np.concatenate([r["bits"] for r in ref]),
            status=np.array([r["status"] for r in ref], np.uint8),
            csi=np.array([r["csi"] for r in ref], np.float64),
            sent=np.concatenate([np.zeros(c["nof_uci_bits"], np.uint8) if b is None else b for c, _, b, _ in cases]),
            snr_class=np.array([k for *_, k in cases], np.uint8), decidable=np.array(decidable, np.uint8),
            dmrs_masks=masks, w_rows=w_rows)
        size = os.path.getsize(C.GOLDEN)
        assert size < 1 << 20, size
        print(f"wrote {C.GOLDEN}: {len(cases)} PDUs, {sum(C.nof_llrs(c) for c, *_ in cases)} LLRs, "
              f"{len(cases) - sum(decidable)} undecidable, {size} bytes")
        if args.time:
            for name, batch in (("the fixture's PDUs", cases),
                                ("32 slots x 8 PDUs", C.bench_batch_cases(np.random.default_rng(C.BENCH_SEED))),
                                ("Format 3, 16 PRB x 14 symbols x 4 ports", [C.worst_case(np.random.default_rng(C.BENCH_SEED))])):
                _, ns = ref_process(exe, tmp, [c[:2] for c in batch], repeats=20)
                print(f"reference receive path, one core: {name} ({len(batch)}): {ns / 1e3:.1f} us per pass, "
                      f"{ns / 1e3 / len(batch):.2f} us per PDU")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
