#!/usr/bin/env python3
"""Generates the polar-coded UCI fixture tests/golden/uci_polar.npz and the table header
srsran-5g_amd/csrc/polar_tables.h from the reference's own uci_decoder_impl, polar_*_impl and CRC calculator.

Compiles tools/ref_uci_polar_driver.cpp together with the reference sources, where they lie in the reference tree
(--ref, or SRSRAN_REF), into a temporary directory outside this tree, with the flags of oracle/build_chain.sh, and runs
it. Nothing compiled and no reference text is kept: only the recorded inputs / outputs and two tables of TS 38.212
(Table 5.3.1.2-1, the polar sequence, and Table 5.4.1.1-1, the sub-block interleaver pattern; specification data, read
from the reference build and checked to generate its tables of every size).

  --time   also times the reference decoder on one host core over the batches of profiles/uci_polar_decoder.md.
"""
import argparse
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import uci_polar_cases as C  # noqa: E402

CODING = "lib/phy/upper/channel_coding/"
REF_SOURCES = ("lib/phy/upper/channel_processors/uci/uci_decoder_impl.cpp", CODING + "polar/polar_code_impl.cpp",
               CODING + "polar/polar_decoder_impl.cpp", CODING + "polar/polar_encoder_impl.cpp",
               CODING + "polar/polar_rate_dematcher_impl.cpp", CODING + "polar/polar_deallocator_impl.cpp",
               CODING + "polar/polar_allocator_impl.cpp", CODING + "polar/polar_rate_matcher_impl.cpp",
               CODING + "short/short_block_detector_impl.cpp", CODING + "short/short_block_encoder_impl.cpp",
               CODING + "crc_calculator_generic_impl.cpp", "lib/phy/upper/log_likelihood_ratio.cpp",
               "lib/srsvec/bit.cpp", "lib/srsvec/dot_prod.cpp", "lib/srsvec/compare.cpp")


def build_driver(ref, tmp):
    exe = os.path.join(tmp, "ref_uci_polar_driver")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-DNDEBUG", "-DFMT_HEADER_ONLY", "-DASSERTS_ENABLED=0",
           "-mavx2", "-mfma", f"-I{ref}/include", f"-I{ref}/external/fmt/include", f"-I{ref}/external", f"-I{ref}",
           f"-I{ref}/lib/phy/upper/channel_coding", "-o", exe, os.path.join(ROOT, "tools", "ref_uci_polar_driver.cpp")]
    cmd += [os.path.join(ref, s) for s in REF_SOURCES]
    subprocess.run(cmd, check=True)
    return exe


def write_fields(path, fields):
    """fields: (payload as a uint8 or int8 array, A)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(fields)))
        for payload, a, e in fields:
            f.write(struct.pack("<II", a, e))
            f.write(np.ascontiguousarray(payload).tobytes())


def ref_decode(exe, tmp, fields, repeats=0):
    """fields: (llrs, A, ...) -> (list of bits with UNTOUCHED marks, list of valid[, ns per pass])."""
    fin, fout = os.path.join(tmp, "dec.in"), os.path.join(tmp, "dec.out")
    write_fields(fin, [(np.asarray(f[0], np.int8), f[1], len(f[0])) for f in fields])
    res = subprocess.run([exe, "decode", fin, fout] + ([str(repeats)] if repeats else []), check=True,
                         capture_output=True, text=True)
    raw = np.fromfile(fout, np.uint8)
    bits, valid, pos = [], [], 0
    for f in fields:
        bits.append(raw[pos: pos + f[1]].copy())
        valid.append(int(raw[pos + f[1]]))
        pos += f[1] + 1
    assert pos == raw.size
    return (bits, valid, float(res.stdout.split()[1])) if repeats else (bits, valid)


def ref_encode(exe, tmp, cases):
    """cases: (bits, E) -> list of the reference chain's codewords."""
    fin, fout = os.path.join(tmp, "enc.in"), os.path.join(tmp, "enc.out")
    write_fields(fin, [(np.asarray(b, np.uint8), len(b), e) for b, e in cases])
    subprocess.run([exe, "encode", fin, fout], check=True)
    raw = np.fromfile(fout, np.uint8)
    out, pos = [], 0
    for _, e in cases:
        out.append(raw[pos: pos + e].copy())
        pos += e
    assert pos == raw.size
    return out


def ref_codes(exe, tmp, codes):
    """codes: (K, E) -> list of (n, nPC, frozen mask, PC set, interleaver) as polar_code_impl::set leaves them."""
    fin, fout = os.path.join(tmp, "codes.in"), os.path.join(tmp, "codes.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(codes)))
        for k, e in codes:
            f.write(struct.pack("<II", k, e))
    subprocess.run([exe, "codes", fin, fout], check=True)
    raw = open(fout, "rb").read()
    out, pos = [], 0
    for _ in codes:
        n_log, npc = struct.unpack_from("<II", raw, pos)
        n = 1 << n_log
        pos += 8
        frozen = np.frombuffer(raw, np.uint8, n, pos)
        pos += n
        pc = np.frombuffer(raw, np.uint16, 3, pos)
        pos += 6
        jj = np.frombuffer(raw, np.uint16, n, pos)
        pos += 2 * n
        out.append((n_log, npc, frozen, pc, jj))
    assert pos == len(raw)
    return out


def ref_tables(exe, tmp):
    """(reliability sequence, 32-entry sub-block pattern), checked to generate the reference's tables for n = 5..10."""
    fout = os.path.join(tmp, "tables.out")
    subprocess.run([exe, "tables", fout], check=True)
    raw = np.fromfile(fout, np.uint16)
    sizes = [1 << n for n in range(5, 11)]
    seqs, pos = [], 0
    for s in sizes * 2:
        seqs.append(raw[pos: pos + s].astype(np.int64))
        pos += s
    assert pos == raw.size
    sequence, pattern = seqs[5], seqs[6]
    assert sorted(sequence) == list(range(1024)) and sorted(pattern) == list(range(32))
    for i, s in enumerate(sizes):
        assert np.array_equal(seqs[i], sequence[sequence < s]), s
        j = np.arange(s)
        assert np.array_equal(seqs[6 + i], pattern[(32 * j) // s] * (s // 32) + j % (s // 32)), s
    return sequence.astype(np.uint16), pattern.astype(np.uint16)


def write_header(sequence, pattern):
    def rows(values, per):
        return ["    " + ", ".join(str(int(v)) for v in values[i: i + per]) + "," for i in range(0, len(values), per)]
    lines = ["// TS 38.212 Table 5.3.1.2-1 (the polar sequence Q_0^1023, in ascending order of reliability) and Table",
             "// 5.4.1.1-1 (the sub-block interleaver pattern P(i)). Specification data, generated by",
             "// tools/gen_uci_polar_golden.py from the reference build's tables; do not edit.",
             "#pragma once", "#include <cstdint>", "", "namespace srsgpu {", "",
             "constexpr uint16_t kPolarReliabilitySequence[1024] = {"]
    lines += rows(sequence, 16)
    lines += ["};", "", "constexpr uint8_t kPolarSubblockPattern[32] = {"]
    lines += rows(pattern, 16)
    lines += ["};", "", "} // namespace srsgpu"]
    with open(os.path.join(ROOT, "srsran-5g_amd", "csrc", "polar_tables.h"), "w") as f:
        f.write("\n".join(lines) + "\n")


def timing_batches(rng):
    return (("64 UEs x (A=20 E=240, A=48 E=576)", C.slot_batch_fields(rng), 100),
            ("16 slots x 64 UEs x (A=20 E=240, A=48 E=576)", C.slot_batch_fields(rng, nof_slots=16), 8),
            ("16 fields of A=1706 E=16384", [C.noisy_field(rng, 1706, 16384, 20) for _ in range(16)], 20))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ref", default=os.environ.get("SRSRAN_REF", "/root/reference"))
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="ref_uci_polar_")
    try:
        exe = build_driver(args.ref, tmp)
        sequence, pattern = ref_tables(exe, tmp)
        write_header(sequence, pattern)
        os.makedirs(os.path.dirname(C.GOLDEN), exist_ok=True)
        np.savez(C.GOLDEN, reliability_sequence=sequence, subblock_pattern=pattern)  # the generators below need them
        C._tables = None
        rng = np.random.default_rng(20261)
        fields = C.golden_generator_fields(rng)
        bits, valid = ref_decode(exe, tmp, fields)
        enc_cases = [(rng.integers(0, 2, a).astype(np.uint8), e) for a, e in C.shape_sizes() if e < 8192]
        enc_cases += [(rng.integers(0, 2, 1706).astype(np.uint8), 16384), (rng.integers(0, 2, 12).astype(np.uint8), 8192)]
        enc = ref_encode(exe, tmp, enc_cases)
        codes = ref_codes(exe, tmp, list(C.CODE_LIST))
        np.savez_compressed(
            C.GOLDEN, reliability_sequence=sequence, subblock_pattern=pattern,
            llrs=np.concatenate([np.asarray(f[0], np.int8) for f in fields]),
            nof_enc_bits=np.array([len(f[0]) for f in fields], np.uint32),
            nof_bits=np.array([f[1] for f in fields], np.uint16), ref_bits=np.concatenate(bits),
            ref_valid=np.array(valid, np.uint8),
            enc_msg=np.concatenate([c[0] for c in enc_cases]), enc_nof_bits=np.array([len(c[0]) for c in enc_cases], np.uint16),
            enc_nof_enc_bits=np.array([c[1] for c in enc_cases], np.uint32), enc_out=np.concatenate(enc),
            code_k=np.array([c[0] for c in C.CODE_LIST], np.uint16), code_e=np.array([c[1] for c in C.CODE_LIST], np.uint16),
            code_n=np.array([c[0] for c in codes], np.uint8), code_npc=np.array([c[1] for c in codes], np.uint8),
            code_frozen=np.packbits(np.concatenate([c[2] for c in codes])),
            code_pc=np.array([c[3] for c in codes], np.uint16),
            code_interleaver=np.concatenate([c[4] for c in codes]).astype(np.uint16))
        size = os.path.getsize(C.GOLDEN)
        assert size < 1 << 20, size
        untouched = sum(int(np.any(b == C.UNTOUCHED)) for b in bits)
        print(f"wrote {C.GOLDEN}: {len(fields)} decoder fields ({sum(valid)} valid, {untouched} with untouched bits), "
              f"{len(enc_cases)} encoder cases, {len(codes)} codes, {size} bytes; polar_tables.h")
        if args.time:
            for name, batch, repeats in timing_batches(np.random.default_rng(5)):
                _, v, ns = ref_decode(exe, tmp, batch, repeats=repeats)
                print(f"reference decoder, one core: {len(batch)} fields ({name}): {ns / 1e3:.1f} us per pass, "
                      f"{sum(v)} valid")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
