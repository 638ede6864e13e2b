"""Pins the numpy restatement of the polar-coded UCI chain (tests/uci_polar_cases.py) to the reference's own decoder,
encoder chain and code construction as recorded in tests/golden/uci_polar.npz (tools/gen_uci_polar_golden.py), checks
the case generators' share conditions here on the CPU so that the GPU tests cannot pass by leaving cases out, and checks
the host code construction of srsran-5g_amd/csrc/polar_code.cpp in a stand-alone sanitizer-built program. No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import uci_polar_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(C.GOLDEN)


def golden_codes(g):
    """(K, E, n, nPC, frozen mask, PC set, interleaver) of the fixture's codes."""
    frozen = np.unpackbits(g["code_frozen"])
    fpos = 0
    for k, e, n_log, npc, pc in zip(g["code_k"], g["code_e"], g["code_n"], g["code_npc"], g["code_pc"]):
        n = 1 << int(n_log)
        yield int(k), int(e), int(n_log), int(npc), frozen[fpos: fpos + n], pc, g["code_interleaver"][fpos: fpos + n]
        fpos += n


def test_restated_decoder_equals_reference():
    """Bits and status of every fixture field; codeblock 1's bits where the reference wrote them."""
    untouched = 0
    for i, (llrs, a, ref_bits, ref_valid) in enumerate(C.golden_fields()):
        bits, valid, per_cb = C.decode(llrs, a)
        wrote = ref_bits != C.UNTOUCHED
        assert valid == ref_valid, (i, a, len(llrs), per_cb)
        assert np.array_equal(bits[wrote], ref_bits[wrote]), (i, a, len(llrs))
        if not wrote.all():
            # Only codeblock 1 of a two-codeblock field whose codeblock 0 failed is left untouched.
            assert C.nof_codeblocks(a, len(llrs)) == 2 and not per_cb[0]
            assert np.array_equal(np.flatnonzero(~wrote), np.arange(a // 2, a))
            untouched += 1
    assert untouched >= 3


def test_restated_encoder_equals_reference(golden):
    g = golden
    mpos = epos = 0
    for a, e in zip(g["enc_nof_bits"], g["enc_nof_enc_bits"]):
        a, e = int(a), int(e)
        want = g["enc_out"][epos: epos + e]
        assert np.array_equal(C.encode(g["enc_msg"][mpos: mpos + a], e), want), (a, e)
        mpos += a
        epos += e


def test_restated_code_construction_equals_reference(golden):
    seen_n, modes, wm = set(), set(), set()
    codes = list(golden_codes(golden))
    assert [(c[0], c[1]) for c in codes] == list(C.CODE_LIST)
    for k, e, n_log, npc, frozen, pc, jj in codes:
        code = C.polar_code(k, e)
        assert (code["n"], code["nPC"]) == (n_log, npc), (k, e)
        assert np.array_equal(code["frozen"], frozen.astype(bool)), (k, e)
        assert code["pc"] == [int(p) for p in pc[:npc]], (k, e)
        assert np.array_equal(code["interleaver"], jj), (k, e)
        seen_n.add(n_log)
        modes.add((code["mode"], e >= 2 * code["N"]))
        if npc:
            wm.add(e > k + 189)
    assert seen_n == {5, 6, 7, 8, 9, 10}
    assert modes >= {("puncture", False), ("shorten", False), ("repeat", False), ("repeat", True)}
    assert wm == {False, True}
    ks, es = {c[0] for c in codes}, {c[1] for c in codes}
    assert ks >= {18, 25, 31, 1023} and 8192 in es


def test_generator_shares():
    """The noise mix has 20-80 % valid fields in every size class; the partial failures fail where they should; the
    decoded bits of valid fields are the sent ones."""
    rng = np.random.default_rng(91)
    fields = C.noise_fields(rng)
    results = [C.decode(f[0], f[1]) for f in fields]
    shares = C.valid_shares(fields, results)
    assert all(0.2 <= s <= 0.8 for s in shares), shares
    assert all(np.array_equal(r[0], f[2]) for f, r in zip(fields, results) if r[1])
    partial = C.partial_failure_fields(np.random.default_rng(92))
    assert {f[3] for f in partial} == {(True, False), (False, True), (False, False)}
    for llrs, a, bits, fail in partial:
        got, valid, per_cb = C.decode(llrs, a)
        assert per_cb == [not fail[0], not fail[1]] and valid == (not any(fail))
        half = a // 2
        if not fail[0]:
            assert np.array_equal(got[:half], bits[:half])
        if not fail[1]:
            assert np.array_equal(got[half:], bits[half:])


def test_generator_shapes():
    """The shape list covers every mother code size with puncturing (impossible at N = 32: 16 K <= 7 E needs E >= 42),
    shortening, E = N, E = N + 1, and E >= 2 N + 5 and 8192 for the sizes a large E can have (N >= 256)."""
    seen = set()
    for a, e in C.shape_sizes():
        for _bits, _filler, k, e_cb in C.codeblocks(a, e):
            code = C.polar_code(k, e_cb)
            n = code["N"]
            kind = (code["mode"] if e_cb < n else "N" if e_cb == n else "N+1" if e_cb == n + 1
                    else "8192" if e_cb >= 8191 else "2N+5" if e_cb == 2 * n + 5 else "repeat")
            seen.add((code["n"], kind))
    for n_log in range(5, 11):
        assert {(n_log, "shorten"), (n_log, "N"), (n_log, "N+1")} <= seen, n_log
        assert n_log == 5 or (n_log, "puncture") in seen
        assert n_log < 8 or {(n_log, "2N+5"), (n_log, "8192")} <= seen, n_log
    sizes = set(C.shape_sizes())
    assert {(a, e) for a in (359, 360) for e in (1087, 1088)} <= sizes and (1706, 16384) in sizes
    assert any(C.nof_codeblocks(a, e) == 2 and a % 2 and e % 2 for a, e in sizes)
    assert any(C.nof_codeblocks(a, e) == 2 and (a // 2) % 32 for a, e in sizes)


def test_accumulation_order_matters():
    """promotion_sum is not associative: (100, 100, -100) gives 127 in the reference's order and 100 reversed."""
    assert C.accumulate([100, 100, -100]) == 127 and C.accumulate([100, 100, -100], reverse=True) == 100
    assert C.accumulate([120, 120, -127]) == 0 and C.accumulate([120, 120, -127], reverse=True) == -127
    # ... and the dematcher accumulates position p's LLRs p, p + N, p + 2 N in that order.
    code = C.polar_code(18, 3 * 256)
    e = np.zeros(3 * 256, np.int64)
    e[[5, 5 + 256, 5 + 512]] = (100, 100, -100)
    llrs = e[C.channel_interleaver(3 * 256)]
    assert C.rate_dematch(llrs, code)[code["interleaver"][5]] == 127


def test_ties_decide_one():
    """An all-zero field decodes to all-one hard decisions at the rate-1 leaves: `value <= 0` is bit 1."""
    code = C.polar_code(31, 64)
    u = C.sc_decode(np.zeros(64, np.int64), code["frozen"])
    assert u[63] == 1 and not u[code["frozen"]].any()


def test_host_code_construction(tmp_path, golden):
    """srsran-5g_amd/csrc/polar_code.cpp against the reference's n / nPC / F-set / PC set / interleaver for every fixture
    code, in a stand-alone program built with the address and undefined-behaviour sanitizers. The program also checks
    the composed dematching map against the three steps done one after the other, and the op list against a recursive
    walk."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "polar_code_check")
    csrc = os.path.join(ROOT, "srsran-5g_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{csrc}", "-o", exe, os.path.join(csrc, "polar_code.cpp"),
                    os.path.join(ROOT, "tools", "polar_code_check.cpp")], check=True)
    dump = tmp_path / "codes.bin"
    codes = list(golden_codes(golden))
    with open(dump, "wb") as f:
        f.write(struct.pack("<I", len(codes)))
        for k, e, n_log, npc, frozen, pc, jj in codes:
            f.write(struct.pack("<IIII", k, e, n_log, npc))
            f.write(frozen.astype(np.uint8).tobytes())
            f.write(np.asarray(pc, np.uint16).tobytes())
            f.write(np.asarray(jj, np.uint16).tobytes())
    res = subprocess.run([exe, str(dump)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"{len(codes)} codes" in res.stdout
