#!/usr/bin/env python3
"""Generates the PRACH fixture tests/golden/prach_detector.npz from the reference's own prach_detector_generic_impl with
its generator, its generic IDFTs (1024 / 256 points, the factory's defaults) and a prach_buffer_impl.

Compiles tools/ref_prach_driver.cpp together with the reference sources, where they lie in the reference tree (--ref,
or SRSRAN_REF), into a temporary directory outside this tree and runs it. Nothing compiled and no reference text is
kept: only the recorded inputs and outputs. The values the reference derives from the PDU through its tables (N_cs,
threshold, margin) are recorded as data; the physical roots are recovered by matching the reference generator's output
against the restatement's sequence over all u.

  --time   also times the reference's detector on one host core over the occasions of tools/prach_bench.py
           (profiles/prach_detector.md).
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
import prach_cases as C  # noqa: E402

UP = "lib/phy/upper/channel_processors/"
REF_SOURCES = (UP + "prach_detector_generic_impl.cpp", UP + "prach_detector_generic_thresholds.cpp",
               UP + "prach_detector_phy_validator_impl.cpp", UP + "prach_generator_impl.cpp",
               "lib/phy/generic_functions/dft_processor_generic_impl.cpp", "lib/ran/prach/prach_cyclic_shifts.cpp",
               "lib/ran/prach/prach_preamble_information.cpp", "lib/srsvec/accumulate.cpp", "lib/srsvec/add.cpp",
               "lib/srsvec/compare.cpp", "lib/srsvec/conversion.cpp", "lib/srsvec/division.cpp", "lib/srsvec/dot_prod.cpp",
               "lib/srsvec/modulus_square.cpp", "lib/srsvec/prod.cpp", "lib/srsvec/sc_prod.cpp", "lib/support/math_utils.cpp")
RESULT = np.dtype([("rssi_dB", "<f4"), ("nof_preambles", "<u4"), ("time_resolution", "<f8"), ("time_advance_max", "<f8"),
                   ("index", "<u4", (64,)), ("metric", "<f4", (64,)), ("time_advance", "<f8", (64,))])
HEADER_KEYS = ("format", "ra_scs", "zcz", "rsi", "nof_ports", "start", "nof", "combine")


def build_driver(ref, tmp):
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17", "-O3", "-DNDEBUG", "-DFMT_HEADER_ONLY", "-DASSERTS_ENABLED=0", "-mavx2", "-mfma", f"-I{ref}/include",
             f"-I{ref}/external/fmt/include", f"-I{ref}/external", f"-I{ref}"]
    sources = [os.path.join(ROOT, "tools", "ref_prach_driver.cpp")] + [os.path.join(ref, s) for s in REF_SOURCES]
    objects = [os.path.join(tmp, f"{i}.o") for i in range(len(sources))]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(lambda so: subprocess.run([cxx] + flags + ["-c", so[0], "-o", so[1]], check=True),
                      zip(sources, objects)))
    exe = os.path.join(tmp, "ref_prach_driver")
    subprocess.run([cxx, "-o", exe] + objects, check=True)
    return exe


def header(c):
    return struct.pack("<8I", *(c[k] for k in HEADER_KEYS))


def ref_derive(exe, tmp, pdus):
    """Per PDU: (N_cs, threshold, margin, [the reference generator's root sequences])."""
    fin, fout = os.path.join(tmp, "derive.in"), os.path.join(tmp, "derive.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(pdus)) + b"".join(header(c) for c in pdus))
    subprocess.run([exe, "derive", fin, fout], check=True)
    raw, pos, out = open(fout, "rb").read(), 0, []
    for _ in pdus:
        n_cs, threshold, margin, nof_sequences, length = struct.unpack_from("<IfIII", raw, pos)
        pos += 20
        seqs = np.frombuffer(raw, np.complex64, nof_sequences * length, pos).reshape(nof_sequences, length)
        pos += seqs.nbytes
        out.append((n_cs, threshold, margin, seqs))
    assert pos == len(raw)
    return out


def ref_detect(exe, tmp, cases, repeats=0):
    fin, fout = os.path.join(tmp, "cases.in"), os.path.join(tmp, "cases.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(header(c))
            f.write(np.ascontiguousarray(c["words"], np.uint32).tobytes())
    res = subprocess.run([exe, "detect", fin, fout] + ([str(repeats)] if repeats else []), check=True, capture_output=True,
                         text=True)
    out = np.fromfile(fout, RESULT)
    assert out.size == len(cases)
    return (out, float(res.stdout.split()[1])) if repeats else out


def complete(exe, tmp, pdus):
    """The PDUs with the values the reference derives from them; the roots matched against the restatement."""
    cases, seqs_of = [], []
    for c, (n_cs, threshold, margin, seqs) in zip(pdus, ref_derive(exe, tmp, pdus)):
        assert threshold > 0 and margin > 0, ("the reference has no threshold for", c)
        d = C.derive(c["format"], c["ra_scs"], n_cs)
        assert seqs.shape == (d["nof_sequences"], d["L"]), (seqs.shape, d)
        roots = []
        for y in seqs:
            u, dist = C.find_root(d["L"], y)
            assert dist < C.ROOT_TOLERANCE[d["L"]], (c, u, dist)
            roots.append(u)
        cases.append(dict(c, n_cs=n_cs, threshold=float(threshold), margin=margin, roots=roots, nof_roots=len(roots)))
        seqs_of.append(seqs)
    return cases, seqs_of


def undecidable(cases, results, delta):
    """(monitored preambles, undecidable ones, undecidable sent ones, reference decisions that differ on decidable ones)."""
    total = bad = bad_sent = wrong = 0
    for c, r in zip(cases, results):
        want = C.detect(c, C.words_to_complex(c["words"]))
        found = {int(k): (ta, m) for k, ta, m in zip(r["index"][:r["nof_preambles"]], r["time_advance"], r["metric"])}
        for k, p in want["preambles"].items():
            total += 1
            if not C.decidable(p, c["threshold"], delta):
                bad += 1
                bad_sent += k in [s for s, _ in c["sent"]]
            elif p["detected"] != (k in found) or (p["detected"] and round(found[k][0] * want["derived"]["sample_rate"]) != p["delay"]):
                wrong += 1
    return total, bad, bad_sent, wrong


def bench_pdus():
    """The occasions tools/prach_bench.py times: Format 0 with N_cs = 13, and B4 with N_cs = 0 (64 roots), as in the fixture."""
    return [p for name, p, _ in C.GOLDEN_RECIPES if name in ("f0_ncs13", "b4_12symbols")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ref", default=os.environ.get("SRSRAN_REF"), required="SRSRAN_REF" not in os.environ,
                    help="the reference source tree (default: $SRSRAN_REF)")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--seed", type=int, default=20267)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="ref_prach_")
    try:
        exe = build_driver(args.ref, tmp)
        cases, seqs_of = complete(exe, tmp, [p for _, p, _ in C.GOLDEN_RECIPES])
        # Redrawn until the reference alone meets the condition on the fixture (tests/test_prach_oracle.py asserts it).
        for seed in range(args.seed, args.seed + 32):
            rng = np.random.default_rng(seed)
            for c, (name, _, recipe) in zip(cases, C.GOLDEN_RECIPES):
                c["name"] = name
                c["words"], c["sent"] = C.make_words(c, recipe, rng)
            results = ref_detect(exe, tmp, cases)
            # The deviation of the reference from the restatement, and the condition on the fixture.
            worst = 0.0
            for c, r in zip(cases, results):
                want = C.detect(c, C.words_to_complex(c["words"]))
                own = 0.0
                for k, m in zip(r["index"][:r["nof_preambles"]], r["metric"]):
                    if int(k) in want["preambles"]:
                        own = max(own, C.rel(want["preambles"][int(k)]["metric"], m))
                worst = max(worst, own)
                print(f"{c['name']:22s} deviation {own:.1e} N_cs {c['n_cs']:3d} threshold {c['threshold']:.3f} margin {c['margin']:2d} rssi {r['rssi_dB']:.2f} dB "
                      f"detected {[(int(k), round(float(m), 2)) for k, m in zip(r['index'][:r['nof_preambles']], r['metric'])]} sent {c['sent']}")
            delta = max(10 * worst, 1e-4)
            total, bad, bad_sent, wrong = undecidable(cases, results, delta)
            print(f"largest metric deviation {worst:.2e}, delta {delta:.2e}; {total} monitored preambles, {bad} undecidable "
                  f"({bad_sent} of them sent), {wrong} decidable ones decided otherwise by the reference")
            if bad <= 0.01 * total and bad_sent == 0 and wrong == 0:
                break
            print(f"seed {seed} does not meet the condition on the fixture: redrawing")
        else:
            raise SystemExit("no seed met the condition: change the recipes")
        by_name = {c["name"]: (c, s) for c, s in zip(cases, seqs_of)}
        root_lu, root_values = [], []
        for length, name, seq in C.ROOT_SAMPLES:
            c, seqs = by_name[name]
            root_lu.append((length, c["roots"][seq]))
            root_values.append(seqs[seq])
        n_ind = results["nof_preambles"]
        os.makedirs(os.path.dirname(C.GOLDEN), exist_ok=True)
        np.savez_compressed(
            C.GOLDEN, names=np.array([c["name"] for c in cases]),
            cfg=np.array([[c[k] for k in C.CFG_KEYS] for c in cases], np.int32),
            threshold=np.array([c["threshold"] for c in cases], np.float32),
            roots=np.concatenate([np.asarray(c["roots"], np.uint16) for c in cases]),
            words=np.concatenate([c["words"].ravel() for c in cases]).astype(np.uint32),
            rssi_dB=results["rssi_dB"], time_resolution=results["time_resolution"],
            time_advance_max=results["time_advance_max"], nof_indications=n_ind.astype(np.uint8),
            ind_index=np.concatenate([r["index"][:n] for r, n in zip(results, n_ind)]).astype(np.uint8),
            ind_time_advance=np.concatenate([r["time_advance"][:n] for r, n in zip(results, n_ind)]),
            ind_metric=np.concatenate([r["metric"][:n] for r, n in zip(results, n_ind)]).astype(np.float32),
            nof_sent=np.array([len(c["sent"]) for c in cases], np.uint8),
            sent=np.array([s for c in cases for s in c["sent"]], np.int32).reshape(-1, 2),
            root_lu=np.array(root_lu, np.int32), root_values=np.concatenate(root_values).astype(np.complex64))
        size = os.path.getsize(C.GOLDEN)
        assert size < 1 << 20, size
        print(f"wrote {C.GOLDEN}: {len(cases)} occasions, {int(n_ind.sum())} indications, {size} bytes")
        if args.time:
            timed, _ = complete(exe, tmp, bench_pdus())
            for c in timed:
                c["words"] = C.transmit(c, [(5, 3, 6.0)], rng)
                _, ns = ref_detect(exe, tmp, [c], repeats=200)
                print(f"reference detector, one core, Format {C.FORMATS[c['format']]} N_cs {c['n_cs']} {c['nof_ports']} ports: "
                      f"{ns / 1e3:.1f} us per occasion")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
