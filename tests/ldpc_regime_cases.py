"""Seeded LDPC decoder inputs that reach every layer class and class boundary at every lifting size, with LLRs off the
nominal amplitude: the regime grid and the scaling sweep of tests/test_ldpc_regimes_oracle.py (the conditions the
inputs meet, with the oracle alone), tests/test_oracle_vs_reference.py and tests/test_golden.py (the oracle held to
the reference on them) and tests/test_ldpc_decoder_regimes_gpu.py (the HIP decoder held to the oracle on them).

Grid: both base graphs x 51 lifting sizes x six input lengths (lengths(): 4, 8, 9, 16, 17 and all layers; the 9- and
17-layer inputs end one LLR into a lifted column). Every cell holds two codeblocks: one of an LLR family (FAMILIES,
rotated over the cells; 6 iterations, with a CRC except every second saturated one) and one noisy codeblock decoded
without CRC for 2 iterations, whose hard bits depend on the messages of every layer: its noise seed is the first one
at which the oracle's results change in both modes when the last layer is skipped.

Plain numpy; codewords are encoded by the oracle."""
import numpy as np

from oracle_lib import BG_K, BG_N_SHORT, CRC6, CRC16, CRC24B, CRC_LEN, DEFECTS, LIFTING_SIZES

FAMILIES = ["baseline", "low", "unit", "saturated", "two_valued", "pm127"]
# Noise scale by length: the shorter the input, the higher the code rate and the less noise it takes.
Q = [0.3, 0.55, 0.55, 0.85, 0.85, 1.0]
NOISY_BOOST = {"baseline": 1.9, "saturated": 2.2}
MAX_ITER = 6
MODES = [("avx2", 1), ("generic", 0)]  # (decoder type of the product, arithmetic mode of the oracle)
SWEEP_FACTORS = [0.5, 0.625, 0.75, 0.9, 0.99995]
SWEEP_SHAPES = [(1, 15), (2, 36), (1, 176), (1, 208)]
GOLDEN_Z = [2, 7, 15, 36, 104, 128, 144, 192, 208]
SKIP_LAST = DEFECTS.index("skip_last")


def lengths(bg, Z):
    """The six input lengths of a shape and the layers each runs (its last LLR being non-zero)."""
    K, N = BG_K[bg], BG_N_SHORT[bg]
    return [((K + 2) * Z, 4), ((K + 6) * Z, 8), ((K + 6) * Z + 1, 9), ((K + 14) * Z, 16), ((K + 14) * Z + 1, 17),
            (N * Z, N + 2 - K)]


def layer_class(bg, layers):
    """The compiled layer class of a layer count (capi.cpp layer_class): 8, 16 or all rows (0 here)."""
    return 8 if layers <= 8 else 16 if layers <= 16 else 0


def pick_crc(bg, Z, nof_filler):
    """CRC24B where the message holds it and 8 payload bits, else CRC16, else CRC6: (polynomial, nof_crc_bits)."""
    L = BG_K[bg] * Z - nof_filler
    poly = CRC24B if L >= 32 else CRC16 if L >= 24 else CRC6
    return poly, 16 if CRC_LEN[poly] < 24 else 24


def codeword(orc, rng, bg, Z, crc_poly, nof_filler):
    """Signs (+1 for a 0 bit) of a random message with its CRC before the fillers, encoded by the oracle."""
    K = BG_K[bg]
    L, clen = K * Z - nof_filler, CRC_LEN[crc_poly]
    msg = np.zeros(K * Z, np.uint8)
    msg[:L - clen] = rng.integers(0, 2, L - clen)
    crc = orc.crc_bits(crc_poly, msg[:L - clen])
    msg[L - clen:L] = [(crc >> (clen - 1 - i)) & 1 for i in range(clen)]
    return 1 - 2 * orc.ldpc_encode(bg, Z, msg).astype(np.int32)


def family_llrs(rng, family, sign, q):
    """The LLRs of a codeword (its signs) in one family, noise scaled by q. Four in ten of the baseline and of the
    saturated codeblocks get NOISY_BOOST times the noise: at the nominal one nearly all of them decode."""
    n = sign.size
    if family in NOISY_BOOST and rng.random() < 0.4:
        q = q * NOISY_BOOST[family]
    if family == "baseline":
        x = np.clip(np.round(12 * sign + rng.normal(0, 9 * q, n)), -120, 120)
    elif family == "low":
        x = np.clip(np.round(2 * sign + rng.normal(0, 1.6 * q, n)), -120, 120)
    elif family == "unit":
        x = sign
    elif family == "saturated":
        x = np.clip(np.round(64 * sign + rng.normal(0, 45 * q, n)), -120, 120)
    elif family == "two_valued":
        x = 10 * sign * np.where(rng.random(n) < 0.09 * q, -1, 1)
    elif family == "pm127":
        x = 127 * sign * np.where(rng.random(n) < 0.035 * q, -1, 1)
    else:
        raise ValueError(family)
    return x.astype(np.int8)


def _finish(llr, bg, Z, nof_filler, n_llr):
    """Fillers marked +infinity as the rate dematcher does, the input cut to its length, its last LLR non-zero."""
    K = BG_K[bg]
    if nof_filler:
        llr[(K - 2) * Z - nof_filler:(K - 2) * Z] = 127
    llr = llr[:n_llr].copy()
    if llr[-1] == 0:
        llr[-1] = 1
    return llr


def _case(bg, Z, li, layers, family, kind, llr, crc_poly, nof_crc_bits, nof_filler, max_iter, sf=0.8):
    return dict(bg=bg, Z=Z, li=li, layers=layers, family=family, kind=kind, llr=llr, crc_poly=crc_poly,
                nof_crc_bits=nof_crc_bits, filler=nof_filler, max_iter=max_iter, sf=sf)


def decode(orc, mode, c, defect=0):
    """The oracle's (iterations or -1, bits, census counters) of a case."""
    return orc.ldpc_decode_census(mode, c["bg"], c["Z"], c["llr"], nof_crc_bits=c["nof_crc_bits"],
                                  nof_filler=c["filler"], crc_poly=c["crc_poly"], max_iter=c["max_iter"],
                                  scaling=c["sf"], defect=defect)


def differs(a, b):
    return a[0] != b[0] or not np.array_equal(a[1], b[1])


def _two_iteration_case(orc, bg, Z, li, n_llr, layers, shape, nof_filler, crc_poly, nof_crc_bits):
    """A noisy codeblock decoded without CRC for 2 iterations. For more than 4 layers: the first noise seed at which
    skipping the last layer changes the oracle's bits in both modes (4-layer inputs run the core rows only)."""
    for attempt in range(400):
        rng = np.random.default_rng([7100, shape, li, attempt])
        sign = codeword(orc, rng, bg, Z, crc_poly, nof_filler)
        llr = np.clip(np.round(10 * sign + rng.normal(0, 9 + 3 * (attempt % 3), sign.size)), -120, 120)
        c = _case(bg, Z, li, layers, "noisy", "two_iter", _finish(llr.astype(np.int8), bg, Z, nof_filler, n_llr), -1,
                  nof_crc_bits, nof_filler, 2)
        if layers <= 4 or all(differs(decode(orc, m, c), decode(orc, m, c, SKIP_LAST)) for _, m in MODES):
            return c
    raise AssertionError(("no input sensitive to the last layer", bg, Z, li))


def build_grid(orc, sizes=LIFTING_SIZES):
    """The grid's cases, cell by cell (family case, then two-iteration case), for the lifting sizes `sizes`. A cell's
    cases depend on its own (bg, Z, length) only, so a subset of sizes yields the same cases as the whole grid."""
    cases = []
    for bg in (1, 2):
        for Z in sizes:
            shape = (bg - 1) * len(LIFTING_SIZES) + LIFTING_SIZES.index(Z)
            K = BG_K[bg]
            nof_filler = min(Z, (K - 2) * Z // 5) if shape % 2 else 0
            crc_poly, nof_crc_bits = pick_crc(bg, Z, nof_filler)
            for li, (n_llr, layers) in enumerate(lengths(bg, Z)):
                family = FAMILIES[(shape + li) % 6]
                rng = np.random.default_rng([7000, shape, li])
                sign = codeword(orc, rng, bg, Z, crc_poly, nof_filler)
                llr = _finish(family_llrs(rng, family, sign, Q[li]), bg, Z, nof_filler, n_llr)
                # Every second saturated case runs all its iterations: no CRC.
                use_crc = not (family == "saturated" and (shape // 6 + li) % 2)
                cases.append(_case(bg, Z, li, layers, family, "family", llr, crc_poly if use_crc else -1, nof_crc_bits,
                                   nof_filler, MAX_ITER))
                cases.append(_two_iteration_case(orc, bg, Z, li, n_llr, layers, shape, nof_filler, crc_poly,
                                                 nof_crc_bits))
    return cases


def build_sweep(orc):
    """Scaling factors on the low and two-valued families at four shapes, in the 8-layer and the all-layers class."""
    cases = []
    for si, (bg, Z) in enumerate(SWEEP_SHAPES):
        crc_poly, nof_crc_bits = pick_crc(bg, Z, 0)
        for li in (1, 5):
            n_llr, layers = lengths(bg, Z)[li]
            for fi, family in enumerate(("low", "two_valued")):
                for ki, sf in enumerate(SWEEP_FACTORS):
                    rng = np.random.default_rng([7200, si, li, fi, ki])
                    sign = codeword(orc, rng, bg, Z, crc_poly, 0)
                    llr = _finish(family_llrs(rng, family, sign, Q[li]), bg, Z, 0, n_llr)
                    cases.append(_case(bg, Z, li, layers, family, "sweep", llr, crc_poly, nof_crc_bits, 0, MAX_ITER,
                                       sf))
    return cases


def oracle_results(orc, cases, mode):
    """[(iterations or None, bits)] and the census counters (len(cases), len(CENSUS)) of the oracle."""
    res, cen = [], []
    for c in cases:
        r, bits, counters = decode(orc, mode, c)
        res.append((None if r < 0 else r, bits))
        cen.append(counters)
    return res, np.array(cen, np.uint64)


def product_batch(srsgpu, cases):
    """(llrs, configs, CRC polynomials) of the cases for LdpcDecoder.decode_batch."""
    cfgs = [srsgpu.CodeblockDecodeConfig(c["bg"], c["Z"], nof_crc_bits=c["nof_crc_bits"], nof_filler_bits=c["filler"],
                                         max_iterations=c["max_iter"], scaling_factor=c["sf"]) for c in cases]
    return [c["llr"] for c in cases], cfgs, [None if c["crc_poly"] < 0 else c["crc_poly"] for c in cases]


_CACHE = {}


def grid_with_results(orc):
    """(cases, {mode: (results, census)}) of the whole grid, built once per process."""
    if "grid" not in _CACHE:
        cases = build_grid(orc)
        _CACHE["grid"] = cases, {mode: oracle_results(orc, cases, mode) for _, mode in MODES}
    return _CACHE["grid"]


def sweep_with_results(orc):
    if "sweep" not in _CACHE:
        cases = build_sweep(orc)
        _CACHE["sweep"] = cases, {mode: oracle_results(orc, cases, mode) for _, mode in MODES}
    return _CACHE["sweep"]

