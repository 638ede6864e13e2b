#!/usr/bin/env python3
"""Generates the SRS fixture tests/golden/srs_estimator.npz from the reference's own srs_estimator_generic_impl with its
low-PAPR sequence generator, its DFT time alignment estimator over generic IDFTs and a resource grid.

Compiles tools/ref_srs_driver.cpp together with the reference sources, where they lie in the reference tree (--ref, or
SRSRAN_REF), into a temporary directory outside this tree and runs it. Nothing compiled and no reference text is kept:
only the recorded inputs (the comb REs the estimator reads as bf16 words, the configuration, the reference's table of
(m_srs, N) by (C_SRS, B_SRS) as data) and outputs. Every case is redrawn until it is decidable (tests/srs_cases.py).

  --time   also times the reference's estimator on one host core over the resources of tools/srs_bench.py
           (profiles/srs_estimator.md).
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
import srs_cases as C  # noqa: E402

REF_SOURCES = ("lib/phy/upper/signal_processors/srs/srs_estimator_generic_impl.cpp",
               "lib/phy/upper/signal_processors/srs/srs_validator_generic_impl.cpp",
               "lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.cpp",
               "lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.cpp",
               "lib/phy/generic_functions/dft_processor_generic_impl.cpp", "lib/ran/srs/srs_information.cpp",
               "lib/ran/srs/srs_bandwidth_configuration.cpp", "lib/phy/support/resource_grid_impl.cpp",
               "lib/phy/support/resource_grid_writer_impl.cpp", "lib/phy/support/resource_grid_reader_impl.cpp",
               "lib/srsvec/add.cpp", "lib/srsvec/compare.cpp", "lib/srsvec/conversion.cpp", "lib/srsvec/dot_prod.cpp",
               "lib/srsvec/modulus_square.cpp", "lib/srsvec/prod.cpp", "lib/srsvec/sc_prod.cpp", "lib/srsvec/subtract.cpp",
               "lib/support/math_utils.cpp")
RESULT = np.dtype([("channel", "<f4", (4, 4, 2)), ("epre_dB", "<f4"), ("noise_var", "<f4"), ("time_alignment", "<f8"),
                   ("resolution", "<f8"), ("ta_min", "<f8"), ("ta_max", "<f8"), ("ta_port", "<f8", (4,))])


def build_driver(ref, tmp):
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17", "-O3", "-DNDEBUG", "-DFMT_HEADER_ONLY", "-DASSERTS_ENABLED=0", "-mavx2", "-mfma", f"-I{ref}/include",
             f"-I{ref}/external/fmt/include", f"-I{ref}/external", f"-I{ref}"]
    sources = [os.path.join(ROOT, "tools", "ref_srs_driver.cpp")] + [os.path.join(ref, s) for s in REF_SOURCES]
    objects = [os.path.join(tmp, f"{i}.o") for i in range(len(sources))]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(lambda so: subprocess.run([cxx] + flags + ["-c", so[0], "-o", so[1]], check=True),
                      zip(sources, objects)))
    exe = os.path.join(tmp, "ref_srs_driver")
    subprocess.run([cxx, "-o", exe] + objects, check=True)
    return exe


def ref_table(exe, tmp):
    out = os.path.join(tmp, "table.out")
    subprocess.run([exe, "table", out], check=True)
    return np.fromfile(out, "<u4").reshape(64, 4, 2)


def ref_estimate(exe, tmp, cases, words_of, repeats=0):
    fin, fout = os.path.join(tmp, "cases.in"), os.path.join(tmp, "cases.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c, words in zip(cases, words_of):
            f.write(struct.pack("<19I", *C.cfg_row(c), c["grid_nof_prb"]))
            f.write(np.ascontiguousarray(words, np.uint32).tobytes())
    res = subprocess.run([exe, "estimate", fin, fout] + ([str(repeats)] if repeats else []), check=True, capture_output=True,
                         text=True)
    out = np.fromfile(fout, RESULT)
    assert out.size == len(cases)
    return (out, float(res.stdout.split()[1])) if repeats else out


def as_reference(r):
    epre = 10.0 ** (float(r["epre_dB"]) / 10.0) if np.isfinite(r["epre_dB"]) else 0.0
    return dict(epre=epre, noise_var=float(r["noise_var"]), time_alignment=float(r["time_alignment"]),
                resolution=float(r["resolution"]))


def bench_cases(table):
    """The two resources tools/srs_bench.py times."""
    return [C.case(table, "bench_small", 48, 0, 4, 1, [0, 1, 2, 3], 1, 0, C.sig(15, 2.3)),
            C.case(table, "bench_wide", 272, 0, 2, 4, [0, 1, 2, 3], 4, 5, C.sig(15, 12.3))]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ref", default=os.environ.get("SRSRAN_REF"), required="SRSRAN_REF" not in os.environ,
                    help="the reference source tree (default: $SRSRAN_REF)")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--seed", type=int, default=20268)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="ref_srs_")
    try:
        exe = build_driver(args.ref, tmp)
        table = ref_table(exe, tmp)
        cases = C.golden_recipes(table)
        drawn = C.draw(cases, args.seed)
        words_of = [w for w, _ in drawn]
        results = ref_estimate(exe, tmp, cases, words_of)
        worst = dict(channel=0.0, epre=0.0, noise_var=0.0, time_alignment=0.0)
        for c, (words, want), r in zip(cases, drawn, results):
            nrx, nap = len(c["rx_ports"]), c["nof_antenna_ports"]
            got = dict(as_reference(r), channel=r["channel"][:nrx, :nap, 0] + 1j * r["channel"][:nrx, :nap, 1])
            dev = C.deviations(got, want)
            port_dev = max(abs(a - b) * want["derived"]["fs"] for a, b in zip(r["ta_port"][:nap], want["ta_port"]))
            for k in worst:
                worst[k] = max(worst[k], dev[k])
            print(f"{c['name']:24s} L {want['derived']['L']:4d} M {want['derived']['M']:4d} m {want['derived']['max_ta_samples']:3d} "
                  f"ta_idx {want['ta_idx']} gap {min(want['gap']):.2e} port {port_dev:.1e} "
                  + " ".join(f"{k} {v:.1e}" for k, v in dev.items()))
            assert port_dev < 1e-3, (c["name"], "a peak decision differs between the reference and the restatement")
        print("largest deviations of the reference from the restatement:", {k: f"{v:.2e}" for k, v in worst.items()})
        kinds = ("signal", "noise", "zero")
        os.makedirs(os.path.dirname(C.GOLDEN), exist_ok=True)
        np.savez_compressed(
            C.GOLDEN, names=np.array([c["name"] for c in cases]), table=table.astype(np.uint16),
            cfg=np.array([C.cfg_row(c) for c in cases], np.int32),
            kind=np.array([kinds.index(c["recipe"]["kind"]) for c in cases], np.uint8),
            delay=np.array([c["recipe"].get("delay", 0.0) for c in cases], np.float32),
            snr_db=np.array([c["recipe"].get("snr_db", 0.0) for c in cases], np.float32),
            words=np.concatenate([w.ravel() for w in words_of]).astype(np.uint32),
            channel=(results["channel"][..., 0] + 1j * results["channel"][..., 1]).astype(np.complex64),
            epre=np.array([as_reference(r)["epre"] for r in results]), noise_var=results["noise_var"],
            time_alignment=results["time_alignment"], resolution=results["resolution"], ta_min=results["ta_min"],
            ta_max=results["ta_max"], ta_port=results["ta_port"])
        size = os.path.getsize(C.GOLDEN)
        assert size < 1 << 20, size
        print(f"wrote {C.GOLDEN}: {len(cases)} resources, {size} bytes")
        if args.time:
            for c in bench_cases(table):
                rng = np.random.default_rng(args.seed)
                words = C.read_words(c, C.to_bf16_words(C.make_grid(c, rng)))
                _, ns = ref_estimate(exe, tmp, [c], [words], repeats=200)
                print(f"reference estimator, one core, {c['name']}: {c['nof_antenna_ports']} ports x {len(c['rx_ports'])} rx x "
                      f"{c['nof_symbols']} symbols x {c['row'][0][0]} PRB comb {c['comb_size']}: {ns / 1e3:.1f} us per resource")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
