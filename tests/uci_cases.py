"""Short-block UCI (1-11 bits) test infrastructure: a numpy restatement of the encoder of TS 38.212 sections 5.3.3.1-.3
with its rate matching (section 5.4.3) and of the reference's detector (short_block_detector_impl::detect,
lib/phy/upper/channel_coding/short/short_block_detector_impl.cpp:186: validation :60, rate dematching :160 with the
saturating LLR sum of log_likelihood_ratio.cpp:432, detect_2 :89, detect_3_11 :129), and seeded case generators.
The restatement is pinned to the reference's own detector and encoder by tests/test_uci_short_block_oracle.py through
tests/golden/uci_short_block.npz (tools/gen_uci_golden.py). TEST INFRASTRUCTURE ONLY."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uci_short_block.npz")

MODULATION_ORDERS = (1, 2, 4, 6, 8)
# calculate_uci_min_encoded_bits (include/srsran/ran/uci/uci_info.h:85) and the GLRT thresholds (:221).
MIN_ENCODED_BITS = (2, 3, 9, 10, 11, 12, 13, 14, 14, 15, 17)
THRESHOLDS = (0, 0, 12, 14, 16, 18, 20, 22, 24, 26, 29)
LLR_MAX = 120
PLACEHOLDER_X, PLACEHOLDER_Y = 255, 254  # "x": a one after scrambling; "y": the previous bit repeated

_basis = None
_signs = None


def basis_words():
    """TS 38.212 Table 5.3.3.3-1 as 11 words, bit n of word i = M_{n,i} (specification data, kept in the fixture)."""
    global _basis
    if _basis is None:
        _basis = [int(w) for w in np.load(GOLDEN)["basis_words"]]
    return _basis


def golden_fields():
    """The fixture's detector cases: (llrs, A, Qm, reference bits, reference validity)."""
    g = np.load(GOLDEN)
    pos = 0
    for e, a, qm, bits, valid in zip(g["nof_enc_bits"], g["nof_bits"], g["modulation_order"], g["ref_bits"],
                                     g["ref_valid"]):
        yield g["llrs"][pos: pos + int(e)], int(a), int(qm), bits[: int(a)], bool(valid)
        pos += int(e)


def block_length(nof_bits, qm):
    """Length N of the block before rate matching."""
    return qm if nof_bits == 1 else 3 * qm if nof_bits == 2 else 32


def encode_block(bits, qm):
    """Sections 5.3.3.1-.3: the N encoded bits (0 / 1 / PLACEHOLDER_X / PLACEHOLDER_Y) of message bits[0..A)."""
    a = len(bits)
    if a == 1:
        out = np.full(qm, PLACEHOLDER_X, np.uint8)
        out[0] = bits[0]
        if qm > 1:
            out[1] = PLACEHOLDER_Y
        return out
    if a == 2:
        c = (bits[0], bits[1], bits[0] ^ bits[1])
        if qm == 1:
            return np.array(c, np.uint8)
        out = np.full(3 * qm, PLACEHOLDER_X, np.uint8)
        out[0], out[1] = c[0], c[1]
        out[qm], out[qm + 1] = c[2], c[0]
        out[2 * qm], out[2 * qm + 1] = c[1], c[2]
        return out
    word = 0
    for i, b in enumerate(bits):
        if b:
            word ^= basis_words()[i]
    return np.array([(word >> n) & 1 for n in range(32)], np.uint8)


def encode(bits, qm, nof_enc):
    """Encoded and rate-matched (cyclic repetition) sequence of nof_enc entries."""
    block = encode_block([int(b) for b in bits], qm)
    return block[np.arange(nof_enc) % block.size]


def rate_dematch(llrs, n):
    """The first min(E, N) LLRs copied, every further block of up to N added with saturation after each block."""
    llrs = np.asarray(llrs, np.int32)
    t = np.zeros(n, np.int32)
    first = min(llrs.size, n)
    t[:first] = llrs[:first]
    for pos in range(n, llrs.size, n):
        b = min(n, llrs.size - pos)
        # int8 saturating add, then the clamp to +-LLR_MAX.
        t[:b] = np.clip(np.clip(t[:b] + llrs[pos: pos + b], -128, 127), -LLR_MAX, LLR_MAX)
    return t


def _sign_table():
    global _signs
    if _signs is None:
        k = np.arange(1024)
        words = np.zeros(1024, np.uint64)
        for j in range(1, 11):
            words ^= np.where((2 * k >> j) & 1, np.uint64(basis_words()[j]), np.uint64(0))
        bits = (words[:, None] >> np.arange(32, dtype=np.uint64)[None, :]) & np.uint64(1)
        _signs = 1 - 2 * bits.astype(np.int32)
    return _signs


def detect(llrs, nof_bits, qm):
    """short_block_detector_impl::detect. Returns (bits[nof_bits] uint8, valid bool, tied bool): tied = more than one
    codeword reaches the winning metric (only the lowest index may come out)."""
    llrs = np.asarray(llrs, np.int8)
    a = nof_bits
    if int(np.count_nonzero(llrs)) < MIN_ENCODED_BITS[a - 1] or (a <= 2 and llrs.size < qm):
        return np.ones(a, np.uint8), False, False
    t = rate_dematch(llrs, block_length(a, qm))
    if a == 1:
        return np.array([0 if t[0] > 0 else 1], np.uint8), True, False
    if a == 2:
        if qm == 1:
            x = [int(t[0]), int(t[1]), int(t[2])]
        else:
            x = [int(t[0] + t[qm + 1]), int(t[1] + t[2 * qm]), int(t[qm] + t[2 * qm + 1])]
        best, idx = 0, 0
        metrics = [sum(c * v for c, v in zip(cw, x)) for cw in ((1, 1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, 1))]
        for i, m in enumerate(metrics):
            if m > best:
                best, idx = m, i
        return np.array([idx & 1, idx >> 1], np.uint8), best > 0, metrics.count(best) > 1
    metrics = _sign_table()[: 1 << (a - 1)] @ t
    mag = np.abs(metrics)
    k = int(np.argmax(mag))  # the first of equal maxima: the reference's strictly-greater scan
    m = int(mag[k])
    value = 2 * k + int(metrics[k] < 0)
    n = int(np.dot(t, t))
    valid = m > 0 and 31 * m * m > THRESHOLDS[a - 1] * (32 * n - m * m)
    return np.array([(value >> j) & 1 for j in range(a)], np.uint8), valid, int(np.count_nonzero(mag == m)) > 1


def llrs_from_encoded(enc, amp, rng, sigma=20.0):
    """round(+-amp + N(0, sigma^2)) clipped to +-LLR_MAX: + for an encoded 0, - for a 1 or "x", the sign of the previous
    entry for "y" (what the demultiplexer's placeholder handling leaves)."""
    enc = np.asarray(enc)
    sign = np.where(enc == 0, 1.0, -1.0)
    for i in np.flatnonzero(enc == PLACEHOLDER_Y):
        sign[i] = sign[i - 1]
    return np.clip(np.rint(sign * amp + rng.normal(0.0, sigma, enc.size)), -LLR_MAX, LLR_MAX).astype(np.int8)


def encoded_lengths(nof_bits, qm, long_e=32 * 40 + 7):
    """The E of the random cases: below the minimum count, N - 1, N, N + 1, 2N, 2N + 5 and a long field."""
    n = block_length(nof_bits, qm)
    return (MIN_ENCODED_BITS[nof_bits - 1] - 1, n - 1, n, n + 1, 2 * n, 2 * n + 5, long_e)


def random_fields(rng, repeats=2, long_e=32 * 40 + 7):
    """Every A in 1..11 x every Qm x every encoded_lengths entry x repeats, amplitudes 2 / 6 / 20 / 60 in equal shares:
    list of (llrs int8, nof_bits, qm, sent bits)."""
    fields = []
    for a in range(1, 12):
        for qm in MODULATION_ORDERS:
            for e in encoded_lengths(a, qm, long_e):
                for _ in range(repeats):
                    amp = (2, 6, 20, 60)[len(fields) % 4]
                    bits = rng.integers(0, 2, a).astype(np.uint8)
                    fields.append((llrs_from_encoded(encode(bits, qm, e), amp, rng), a, qm, bits))
    return fields


def tie_fields(rng, per_size=24):
    """A >= 3, E = 32, LLRs uniform in {-1, 0, 1}: many codewords share the winning metric."""
    return [(rng.integers(-1, 2, 32).astype(np.int8), a, int(rng.choice(MODULATION_ORDERS)), None)
            for a in range(3, 12) for _ in range(per_size)]


def saturation_fields():
    """Blocks that saturate on the way: every position receives (100, 100, -100) -> 20 (a plain sum gives 100),
    (-100, -100, 100) -> -20 or (120, 120, 120, -100) -> 20, for A = 1, 2 and 7; with the same sign on every position and
    with alternating signs, and with a partial last block (only the first positions receive the last value, which
    changes their sign or size)."""
    fields = []
    for a in (1, 2, 7):
        for qm in (1, 4):
            n = block_length(a, qm)
            for pattern in ((100, 100, -100), (-100, -100, 100), (120, 120, 120, -100)):
                for alternate in (False, True):
                    sign = np.where(np.arange(n) % 2 == 1, -1, 1) if alternate else np.ones(n, int)
                    llrs = np.concatenate([sign * v for v in pattern]).astype(np.int8)
                    fields.append((llrs, a, qm, None))
                    if n > 1:
                        fields.append((llrs[: llrs.size - n + max(1, n // 2)].copy(), a, qm, None))
    return fields


def degenerate_fields():
    """All-zero LLRs, E = 0, A <= 2 with E < Qm, A = 2 with the three combined values cancelling to 0 (BPSK through the
    rate dematcher, QPSK through the combining), and perfectly correlated fields (zero GLRT denominator: valid)."""
    fields = [(np.zeros(32, np.int8), a, 2, None) for a in (1, 2, 5, 11)]
    fields += [(np.zeros(0, np.int8), a, 4, None) for a in (1, 2, 3, 11)]
    fields += [(np.full(3, 40, np.int8), 1, 4, None), (np.full(7, -40, np.int8), 2, 8, None)]
    fields += [(np.array([50, 30, 20, -50, -30, -20], np.int8), 2, 1, None),
               (np.array([50, -30, 20, -50, 30, -20], np.int8), 2, 2, None)]
    for a, value in ((3, 0), (5, 21), (8, 130), (11, 2047), (11, 1024)):
        bits = [(value >> j) & 1 for j in range(a)]
        fields.append(((77 * (1 - 2 * encode(bits, 1, 32).astype(int))).astype(np.int8), a, 1, None))
    fields.append((np.array([60, -60, -60], np.int8), 2, 1, None))
    return fields


def slot_batch_fields(rng, nof_slots=1, nof_ues=64):
    """The measured batch: per slot and UE a HARQ-ACK field (A = 4, E = 96) and a CSI Part 1 field (A = 11, E = 240),
    16QAM, amplitude 20."""
    fields = []
    for _ in range(nof_slots * nof_ues):
        for a, e in ((4, 96), (11, 240)):
            bits = rng.integers(0, 2, a).astype(np.uint8)
            fields.append((llrs_from_encoded(encode(bits, 4, e), 20, rng), a, 4, bits))
    return fields
