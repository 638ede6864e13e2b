"""The numpy restatement of the short-block UCI code (tests/uci_cases.py) against the reference's own detector and
encoder, recorded in tests/golden/uci_short_block.npz by tools/gen_uci_golden.py: every field, bits and validity,
exact. The GPU kernel is then held to the restatement and to the same fixture (tests/test_uci_decoder_gpu.py)."""
import os
import re

import numpy as np

import uci_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_covers_the_cases():
    fields = list(C.golden_fields())
    assert 300 <= len(fields) <= 1000 and os.path.getsize(C.GOLDEN) < 100 * 1024
    for a in range(1, 12):
        for qm in C.MODULATION_ORDERS:
            assert any(f[1] == a and f[2] == qm for f in fields)
    for a in range(3, 12):
        valid = [f[4] for f in fields if f[1] == a]
        assert 0.2 <= np.mean(valid) <= 0.8, (a, np.mean(valid))


def test_detector_restatement_equals_reference():
    ties = 0
    for llrs, a, qm, bits, valid in C.golden_fields():
        got_bits, got_valid, tied = C.detect(llrs, a, qm)
        assert np.array_equal(got_bits, bits) and got_valid == valid, (a, qm, llrs.size, got_bits, bits, got_valid, valid)
        ties += tied
    assert ties >= 10


def test_encoder_restatement_equals_reference():
    g = np.load(C.GOLDEN)
    pos = 0
    for msg, a, qm, e in zip(g["enc_msg"], g["enc_nof_bits"], g["enc_modulation_order"], g["enc_nof_enc_bits"]):
        assert np.array_equal(C.encode(msg[: int(a)], int(qm), int(e)), g["enc_out"][pos: pos + int(e)]), (a, qm, e)
        pos += int(e)
    assert pos == g["enc_out"].size


def test_basis_header_equals_fixture():
    text = open(os.path.join(ROOT, "srsran-5g_amd", "csrc", "uci_basis_words.h")).read()
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{8})u", text)]
    assert words == C.basis_words() and len(words) == 11


def test_round_trip_at_high_amplitude():
    """Every message of every size through the restatement's own encoder and detector, noise-free at amplitude 100,
    with one block and with repetitions that saturate."""
    for a in range(1, 12):
        for qm in C.MODULATION_ORDERS:
            n = C.block_length(a, qm)
            for value in range(1 << a) if a <= 6 else range(0, 1 << a, 37):
                bits = np.array([(value >> j) & 1 for j in range(a)], np.uint8)
                for e in (max(n, C.MIN_ENCODED_BITS[a - 1]), 3 * n + 1):
                    llrs = C.llrs_from_encoded(C.encode(bits, qm, e), 100, np.random.default_rng(0), sigma=0.0)
                    got, valid, _ = C.detect(llrs, a, qm)
                    assert np.array_equal(got, bits) and valid, (a, qm, value, e)
