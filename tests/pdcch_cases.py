"""PDCCH test infrastructure: a numpy restatement of the reference's pdcch_processor_impl::process
(lib/phy/upper/channel_processors/pdcch/pdcch_processor_impl.cpp:79) in its four stages, its inverse over an identity
channel, and seeded case generators.

  CCE to PRB      lib/ran/pdcch/cce_to_prb_mapping.cpp (interleaver f(x) = (r C + c + n_shift) mod (N_REG / L), the sorted
                  REG list, the walk over the 6-PRB frequency resources; CORESET0 is L = 6, R = 2 offset by bwp_start_rb)
  encoding        pdcch_encoder_impl.cpp:33 (CRC24C over 24 ones and the payload, RNTI on the last 16 parity bits), the
                  downlink polar code: polar_code_impl.cpp:325-456 with nMax = 9, polar_interleaver_impl.cpp:45,
                  polar_allocator_impl.cpp:27, polar_encoder_impl.cpp, polar_rate_matcher_impl.cpp:100 (no channel
                  interleaver)
  modulation      pdcch_modulator_impl.cpp:32 (c_init = ((n_rnti << 16) + n_id) mod 2^31, QPSK of the LUT mapper, the
                  scaling when it is a normal float), resource_grid_mapper_impl.cpp:140 and channel_precoder_generic.cpp:27
                  (one complex product per port, every term rounded, bf16 half to even), REs k not in {1, 5, 9}
  DM-RS           dmrs_pdcch_processor_impl.cpp:32 (c_init per symbol, amplitude / sqrt 2, three pilots per PRB counted
                  from reference_point_k_rb, k = 1, 5, 9)

Pinned to the reference's own outputs by tests/test_pdcch_oracle.py through tests/golden/pdcch.npz
(tools/gen_pdcch_golden.py), which also holds the specification table read here. TEST INFRASTRUCTURE ONLY."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import uci_polar_cases as U  # noqa: E402
from pusch_demod_oracle import gold_sequence  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "pdcch.npz")
F = np.float32

CORESET0, NON_INTERLEAVED, INTERLEAVED = 0, 1, 2
LEVELS = (1, 2, 4, 8, 16)
K_MAX_IL = 164
CRC24C = 0x1B2B117
DATA_K = (0, 2, 3, 4, 6, 7, 8, 10, 11)
DMRS_K = (1, 5, 9)
SENTINEL = 0x7FC17FC1  # grid prefill of the GPU tests: a NaN pattern no product rounds to

_pattern = None


def interleaver_pattern():
    """TS 38.212 Table 5.3.1.1-1, the 164-entry input interleaver pattern."""
    global _pattern
    if _pattern is None:
        _pattern = np.load(GOLDEN)["input_interleaver_pattern"].astype(np.int64)
    return _pattern


# ---- CCE to PRB ------------------------------------------------------------------------------------------------

def popcount(v):
    return bin(int(v)).count("1")


def refusal(cfg, nof_payload_bits, grid_nof_prb, grid_nof_ports):
    """A word naming the rule of the reference (validator, mapper assertion, polar code limits) or of the grid that
    refuses the DCI, or None. The order is the plan's."""
    dur, al = cfg["duration"], cfg["aggregation_level"]
    inter = cfg["mapping"] == INTERLEAVED
    if not 1 <= dur <= 3:
        return "duration"
    if cfg["start_symbol"] + dur > 14:
        return "slot duration"
    if inter and cfg["reg_bundle_size"] != 6 and cfg["reg_bundle_size"] != (3 if dur == 3 else 2):
        return "REG bundle size"
    if inter and cfg["interleaver_size"] not in (2, 3, 6):
        return "interleaver size"
    if al not in LEVELS:
        return "aggregation level"
    if cfg["cce_index"] + al > popcount(cfg["frequency_resources"]) * dur:
        return "CORESET capacity"
    if nof_payload_bits == 0:
        return "Empty payload"
    k, e = nof_payload_bits + 24, 108 * al
    if not 36 <= k <= 164:
        return "K"
    if k >= e:
        return "does not fit"
    if cfg["mapping"] != NON_INTERLEAVED:
        l, r, nrb = (6, 2, cfg["bwp_size_rb"]) if cfg["mapping"] == CORESET0 else (
            cfg["reg_bundle_size"], cfg["interleaver_size"], 6 * popcount(cfg["frequency_resources"]))
        if nrb == 0 or (nrb * dur) % (l * r) or l % dur:
            return "multiple"
        if (cfg["cce_index"] + al) * 6 > nrb * dur:
            return "REGs of CORESET0"
    if not 1 <= cfg["nof_ports"] <= grid_nof_ports:
        return "ports"
    if max(cce_prbs(cfg)) >= min(grid_nof_prb, cfg["bwp_start_rb"] + cfg["bwp_size_rb"]):
        return "PRB"
    return None


def cce_prbs(cfg):
    """The PRBs of the DCI's CCEs, ascending (the set bits of pdcch_processor_impl::compute_rb_mask)."""
    dur, al, cce = cfg["duration"], cfg["aggregation_level"], cfg["cce_index"]
    if cfg["mapping"] == NON_INTERLEAVED:
        regs = list(range(6 * cce, 6 * (cce + al)))
    else:
        if cfg["mapping"] == CORESET0:
            l, r, shift, nrb = 6, 2, cfg["shift_index"], cfg["bwp_size_rb"]
        else:
            l, r, shift = cfg["reg_bundle_size"], cfg["interleaver_size"], cfg["shift_index"]
            nrb = 6 * popcount(cfg["frequency_resources"])
        nreg = nrb * dur
        c_rows = nreg // (l * r)
        regs = []
        for x in range(cce * 6 // l, (cce + al) * 6 // l):
            f = ((x % r) * c_rows + x // r + shift) % (nreg // l)
            regs += range(f * l, (f + 1) * l)
        regs.sort()
    first = regs[::dur]
    if cfg["mapping"] == CORESET0:
        return [g // dur + cfg["bwp_start_rb"] for g in first]
    prb_of = []
    for i in range(45):
        if (cfg["frequency_resources"] >> i) & 1:
            prb_of += range(6 * i + cfg["bwp_start_rb"], 6 * i + 6 + cfg["bwp_start_rb"])
    assert all(g % dur == 0 for g in first)
    return sorted(prb_of[g // dur] for g in first)


def prb_mask(cfg, size):
    mask = np.zeros(size, np.uint8)
    mask[cce_prbs(cfg)] = 1
    return mask


# ---- downlink polar code ---------------------------------------------------------------------------------------

def dl_code_size_log(k, e):
    el = 1
    while (1 << el) < e:
        el += 1
    n1 = el - 1 if (8 * e <= 9 * (1 << (el - 1)) and 16 * k < 9 * e) else el
    kl = 0
    while kl < 10 and (1 << kl) < k:
        kl += 1
    return max(5, min(n1, kl + 3, 9))


@functools.lru_cache(maxsize=None)
def dl_code(k, e):
    """The downlink code of (K, E): n, N, frozen mask, info positions (increasing), pi (input interleaver), gather
    (rate-matched bit j is encoded bit gather[j]), mode."""
    assert 36 <= k <= 164 and k < e
    n_log = dl_code_size_log(k, e)
    n = 1 << n_log
    assert k < n
    seq = U.tables()[0]
    seq = seq[seq < n]
    jj = U.subblock_interleaver(n_log)
    mode, candidates = "repeat", seq
    if e < n:
        if 16 * k <= 7 * e:
            mode, pre = "puncture", jj[: n - e]
            t = 3 * n // 4 - e // 2 - 1 if e >= 3 * n // 4 else 9 * n // 16 - e // 4
        else:
            mode, pre, t = "shorten", jj[e:], 0
        drop = set(pre.tolist())
        candidates = np.array([q for q in seq if q > t and q not in drop], np.int64)
    frozen = np.ones(n, bool)
    frozen[candidates[candidates.size - k:]] = False
    pat = interleaver_pattern()
    pi = pat[pat >= K_MAX_IL - k] - (K_MAX_IL - k)
    j = np.arange(e)
    gather = jj[j % n if mode == "repeat" else j + (n - e) if mode == "puncture" else j]
    return dict(n=n_log, N=n, K=k, E=e, frozen=frozen, info=np.flatnonzero(~frozen), pi=pi, gather=gather, mode=mode)


def all_codes():
    """(K, E) of every payload size 12..128 at every level with K < E, level outermost: the order of the fixture's
    code_n / code_frozen records."""
    return [(a + 24, 108 * al) for al in LEVELS for a in range(12, 129) if a + 24 < 108 * al]


def golden_codes():
    """(K, E, n, frozen mask) of the reference's downlink code for every all_codes() entry."""
    g = np.load(GOLDEN)
    for (k, e), n_log, packed in zip(all_codes(), g["code_n"], g["code_frozen"]):
        yield k, e, int(n_log), np.unpackbits(packed, bitorder="little")[: 1 << int(n_log)].astype(bool)


def crc24c_remainder(bits):
    reg = 0
    for b in bits:
        reg = (reg << 1) | int(b)
        if reg >> 24:
            reg ^= CRC24C
    return reg


def attach_crc(payload, rnti):
    """c: the payload and its 24 parity bits, the RNTI on the last 16 (TS 38.212 section 7.3.2)."""
    payload = [int(b) for b in payload]
    rem = crc24c_remainder([1] * 24 + payload + [0] * 24) ^ (rnti & 0xFFFF)
    return np.array(payload + [(rem >> (23 - i)) & 1 for i in range(24)], np.uint8)


def encode(payload, rnti, e):
    """The e rate-matched bits of pdcch_encoder_impl::encode."""
    c = attach_crc(payload, rnti)
    code = dl_code(c.size, e)
    u = np.zeros(code["N"], np.uint8)
    u[code["info"]] = c[code["pi"]]
    return U.polar_transform(u)[code["gather"]]


@functools.lru_cache(maxsize=None)
def _inverse(k, e):
    """Solves x[known] = u[info] G_N over GF(2) once per code: (for every distinct encoded position the first
    rate-matched index that carries it, the K x known matrix T with u[info] = T x[known])."""
    code = dl_code(k, e)
    n = code["N"]
    g = np.array([U.polar_transform(row) for row in np.eye(n, dtype=np.uint8)])
    pos, first = np.unique(code["gather"], return_index=True)
    a = g[code["info"]][:, pos]  # K x known
    aug = np.concatenate([a.T.copy(), np.eye(pos.size, dtype=np.uint8)], axis=1)
    for col in range(k):
        piv = col + int(np.argmax(aug[col:, col]))
        assert aug[piv, col], "the transmitted bits do not determine the message"
        aug[[col, piv]] = aug[[piv, col]]
        others = np.flatnonzero(aug[:, col])
        aug[others[others != col]] ^= aug[col]
    return first, aug[:k, k:]


def decode_hard(bits, nof_payload_bits, rnti):
    """Inverse of encode() on error-free bits: undoes the rate matching, inverts G_N on the positions that were sent,
    undoes the input interleaver; (payload, the CRC with the RNTI holds and the bits are a codeword)."""
    bits = np.asarray(bits, np.uint8)
    k = nof_payload_bits + 24
    code = dl_code(k, bits.size)
    first, t = _inverse(k, bits.size)
    c = np.zeros(k, np.uint8)
    c[code["pi"]] = (t.astype(np.int64) @ bits[first].astype(np.int64)) & 1
    payload = c[:nof_payload_bits]
    plain = c.copy()
    plain[-16:] ^= np.array([(rnti >> (15 - i)) & 1 for i in range(16)], np.uint8)
    ok = crc24c_remainder([1] * 24 + plain.tolist()) == 0
    return payload, ok and np.array_equal(encode(payload, rnti, bits.size), bits)


# ---- modulation, DM-RS and mapping -----------------------------------------------------------------------------

def to_bf16(v):
    u = np.asarray(v, F).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)


def precode(re, im, w):
    """One port: (re + j im) w with every term rounded to float32, then bf16 words re | im << 16."""
    wr, wi = F(np.real(w)), F(np.imag(w))
    sr = (re * wr).astype(F) - (im * wi).astype(F)
    si = (re * wi).astype(F) + (im * wr).astype(F)
    return to_bf16(sr) | (to_bf16(si) << 16)


def amplitudes(cfg):
    """(QPSK component amplitude, DM-RS component amplitude) as float32."""
    a = F(np.sqrt(0.5))
    s = F(cfg["data_scaling"])
    if np.isfinite(s) and abs(s) >= np.finfo(F).tiny:  # std::isnormal
        a = F(a * s)
    return a, F(np.sqrt(0.5) * np.float64(F(cfg["dmrs_amplitude"])))


def c_init_data(cfg):
    return ((cfg["n_rnti"] << 16) + cfg["n_id_data"]) % (1 << 31)


def c_init_dmrs(cfg, symbol):
    n_id = cfg["n_id_dmrs"]
    return ((14 * cfg["n_slot"] + symbol + 1) * (2 * n_id + 1) * (1 << 17) + 2 * n_id) % (1 << 31)


def process(cfg, payload):
    """(PRBs, rate-matched bits, written grid words as an array of (port, symbol, subcarrier, word) rows sorted by
    port, symbol, subcarrier)."""
    prbs = np.array(cce_prbs(cfg), np.int64)
    e = 108 * cfg["aggregation_level"]
    bits = encode(payload, cfg["rnti"], e)
    scr = bits ^ gold_sequence(c_init_data(cfg), e)
    a, ad = amplitudes(cfg)
    re = np.where(scr[0::2] == 1, -a, a).astype(F)
    im = np.where(scr[1::2] == 1, -a, a).astype(F)
    dur, start = cfg["duration"], cfg["start_symbol"]
    sym = np.repeat(np.arange(start, start + dur), 9 * prbs.size)
    sc = np.tile((12 * prbs[:, None] + np.array(DATA_K)[None, :]).ravel(), dur)
    assert sym.size == re.size
    ref = cfg["bwp_start_rb"] if cfg["mapping"] == CORESET0 else 0
    m = (3 * (prbs[:, None] - ref) + np.arange(3)[None, :]).ravel()
    dsc = (12 * prbs[:, None] + np.array(DMRS_K)[None, :]).ravel()
    dre, dim, dsym = [], [], []
    for l in range(start, start + dur):
        seq = gold_sequence(c_init_dmrs(cfg, l), int(2 * m.max() + 2))
        dre.append(np.where(seq[2 * m] == 1, -ad, ad).astype(F))
        dim.append(np.where(seq[2 * m + 1] == 1, -ad, ad).astype(F))
        dsym.append(np.full(m.size, l))
    re, im = np.concatenate([re] + dre), np.concatenate([im] + dim)
    sym, sc = np.concatenate([sym] + dsym), np.concatenate([sc] + [dsc] * dur)
    rows = []
    for p in range(cfg["nof_ports"]):
        rows.append(np.stack([np.full(sym.size, p), sym, sc, precode(re, im, cfg["weights"][p])], axis=1))
    rows = np.concatenate(rows).astype(np.int64)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    return prbs, bits, rows


def apply_rows(grid_words, rows):
    """Writes (port, symbol, subcarrier, word) rows into a (ports, 14, nsc) uint32 grid."""
    grid_words[rows[:, 0], rows[:, 1], rows[:, 2]] = rows[:, 3].astype(np.uint32)


def receive(cfg, nof_payload_bits, grid_words):
    """The inverse over an identity channel, from port 0 of a (ports, 14, nsc) uint32 grid: (payload, CRC holds, the
    DM-RS REs carry the expected signs). Needs a port-0 weight with a positive real part and no imaginary part."""
    prbs = np.array(cce_prbs(cfg), np.int64)
    dur, start = cfg["duration"], cfg["start_symbol"]
    words = []
    for l in range(start, start + dur):
        words.append(grid_words[0, l][(12 * prbs[:, None] + np.array(DATA_K)[None, :]).ravel()])
    words = np.concatenate(words)
    scr = np.empty(2 * words.size, np.uint8)
    scr[0::2] = (words >> 15) & 1  # the sign bit of the bf16 real part
    scr[1::2] = (words >> 31) & 1
    bits = scr ^ gold_sequence(c_init_data(cfg), scr.size)
    payload, ok = decode_hard(bits, nof_payload_bits, cfg["rnti"])
    ref = cfg["bwp_start_rb"] if cfg["mapping"] == CORESET0 else 0
    m = (3 * (prbs[:, None] - ref) + np.arange(3)[None, :]).ravel()
    dmrs_ok = True
    for l in range(start, start + dur):
        seq = gold_sequence(c_init_dmrs(cfg, l), int(2 * m.max() + 2))
        w = grid_words[0, l][(12 * prbs[:, None] + np.array(DMRS_K)[None, :]).ravel()]
        dmrs_ok &= np.array_equal((w >> 15) & 1, seq[2 * m]) and np.array_equal((w >> 31) & 1, seq[2 * m + 1])
    return payload, ok, bool(dmrs_ok)


# ---- case generators -------------------------------------------------------------------------------------------

HOLES = 0b10110111  # six frequency resources out of eight

# CORESET templates of the fixture: (name, fields, grid PRBs). Every one fits a 52-PRB grid but the last.
TEMPLATES = (
    dict(mapping=NON_INTERLEAVED, bwp_start_rb=0, bwp_size_rb=52, frequency_resources=0xFF, duration=1, start_symbol=0),
    dict(mapping=NON_INTERLEAVED, bwp_start_rb=2, bwp_size_rb=50, frequency_resources=HOLES, duration=2, start_symbol=1),
    dict(mapping=NON_INTERLEAVED, bwp_start_rb=4, bwp_size_rb=48, frequency_resources=HOLES, duration=3, start_symbol=2),
    dict(mapping=INTERLEAVED, bwp_start_rb=0, bwp_size_rb=52, frequency_resources=HOLES, duration=1, start_symbol=0,
         reg_bundle_size=2, interleaver_size=2, shift_index=0),
    dict(mapping=INTERLEAVED, bwp_start_rb=4, bwp_size_rb=48, frequency_resources=HOLES, duration=1, start_symbol=3,
         reg_bundle_size=2, interleaver_size=3, shift_index=5),
    dict(mapping=INTERLEAVED, bwp_start_rb=4, bwp_size_rb=48, frequency_resources=HOLES, duration=2, start_symbol=0,
         reg_bundle_size=2, interleaver_size=6, shift_index=17),
    dict(mapping=INTERLEAVED, bwp_start_rb=0, bwp_size_rb=52, frequency_resources=0x3F, duration=1, start_symbol=1,
         reg_bundle_size=6, interleaver_size=2, shift_index=101),
    dict(mapping=INTERLEAVED, bwp_start_rb=1, bwp_size_rb=51, frequency_resources=HOLES, duration=2, start_symbol=12,
         reg_bundle_size=6, interleaver_size=3, shift_index=3),
    dict(mapping=INTERLEAVED, bwp_start_rb=4, bwp_size_rb=48, frequency_resources=HOLES, duration=3, start_symbol=0,
         reg_bundle_size=6, interleaver_size=6, shift_index=0),
    dict(mapping=INTERLEAVED, bwp_start_rb=4, bwp_size_rb=48, frequency_resources=HOLES, duration=3, start_symbol=11,
         reg_bundle_size=3, interleaver_size=2, shift_index=274),
    dict(mapping=INTERLEAVED, bwp_start_rb=0, bwp_size_rb=52, frequency_resources=HOLES, duration=3, start_symbol=0,
         reg_bundle_size=3, interleaver_size=3, shift_index=7),
    dict(mapping=INTERLEAVED, bwp_start_rb=3, bwp_size_rb=49, frequency_resources=HOLES, duration=3, start_symbol=1,
         reg_bundle_size=3, interleaver_size=6, shift_index=1),
    dict(mapping=CORESET0, bwp_start_rb=10, bwp_size_rb=24, frequency_resources=0xF, duration=1, start_symbol=0,
         shift_index=37),
    dict(mapping=CORESET0, bwp_start_rb=3, bwp_size_rb=48, frequency_resources=0xFF, duration=2, start_symbol=0,
         shift_index=500),
    dict(mapping=CORESET0, bwp_start_rb=28, bwp_size_rb=24, frequency_resources=0xF, duration=3, start_symbol=0,
         shift_index=1006),
    dict(mapping=NON_INTERLEAVED, bwp_start_rb=10, bwp_size_rb=96, frequency_resources=0xFFFF, duration=1, start_symbol=0,
         grid_nof_prb=106),
)

# Payload sizes per level: 12 and the largest, both sides of K = 47 / 48 (16 K = 7 E at level 1), K = 64 / 65, and
# K = 94 / 95 (16 K = 7 E at level 2). K < E bounds level 1 to 83 bits.
PAYLOAD_SIZES = {1: (12, 23, 24, 40, 41, 83, 60), 2: (12, 70, 71, 128, 40, 41), 4: (12, 128, 41, 64, 23),
                 8: (12, 128, 77, 40), 16: (12, 128, 99)}
POWERS_DB = ((0.0, 0.0), (-3.0, 3.0), (1.5, -6.0), (0.0, 4.77), (6.0, 0.0))


def random_weights(rng, nof_ports):
    return ((rng.normal(size=nof_ports) + 1j * rng.normal(size=nof_ports)) / 2).astype(np.complex64)


def fill_dci(rng, cfg, nof_payload_bits):
    """Random identifiers and payload for a CORESET / level / CCE choice; returns (cfg, payload bits)."""
    cfg = dict(dict(reg_bundle_size=0, interleaver_size=0, shift_index=0, grid_nof_prb=52, grid_nof_ports=4), **cfg)
    cfg.update(n_slot=int(rng.integers(0, 20)), rnti=int(rng.integers(1, 65520)), n_id_dmrs=int(rng.integers(0, 65536)),
               n_id_data=int(rng.integers(0, 65536)), n_rnti=int(rng.integers(0, 65536)))
    return cfg, rng.integers(0, 2, nof_payload_bits).astype(np.uint8)


def nof_cces(cfg):
    return popcount(cfg["frequency_resources"]) * cfg["duration"]


def golden_generator_cases(rng):
    """The DCIs the fixture records: every template at every level it has room for, the payload sizes, port counts
    and powers taken in turn. Amplitudes are left as dB offsets; the reference's own conversion is recorded."""
    cases, turn = [], {l: 0 for l in LEVELS}
    i = 0
    for tpl in TEMPLATES:
        for al in LEVELS:
            if al > nof_cces(tpl):
                continue
            a = PAYLOAD_SIZES[al][turn[al] % len(PAYLOAD_SIZES[al])]
            turn[al] += 1
            cfg, payload = fill_dci(rng, dict(tpl, aggregation_level=al,
                                              cce_index=int(rng.integers(0, nof_cces(tpl) - al + 1))), a)
            ports = (1, 2, 4, 1)[i % 4]
            cfg["nof_ports"] = ports
            cfg["weights"] = np.ones(1, np.complex64) if i % 4 == 0 else random_weights(rng, ports)
            cfg["grid_nof_ports"] = ports if i % 3 == 0 else 4
            cfg["data_power_offset_dB"], cfg["dmrs_power_offset_dB"] = POWERS_DB[i % len(POWERS_DB)]
            cases.append((cfg, payload))
            i += 1
    return cases


CFG_INT_KEYS = ("bwp_size_rb", "bwp_start_rb", "start_symbol", "duration", "frequency_resources", "mapping",
                "reg_bundle_size", "interleaver_size", "shift_index", "n_slot", "rnti", "n_id_dmrs", "n_id_data", "n_rnti",
                "cce_index", "aggregation_level", "nof_ports", "grid_nof_prb", "grid_nof_ports")


def golden_cases():
    """The fixture's cases: (cfg with the reference's amplitudes, payload bits, PRB mask, rate-matched bits, written
    grid rows (port, symbol, subcarrier, word))."""
    g = np.load(GOLDEN)
    ppos = epos = mpos = wpos = 0
    for i in range(g["cfg"].shape[0]):
        cfg = {k: int(v) for k, v in zip(CFG_INT_KEYS, g["cfg"][i])}
        cfg["weights"] = g["weights"][i][: cfg["nof_ports"]].copy()
        cfg["data_scaling"], cfg["dmrs_amplitude"] = F(g["amplitudes"][i][0]), F(g["amplitudes"][i][1])
        a, e, nm, nw = int(g["nof_payload_bits"][i]), 108 * cfg["aggregation_level"], int(g["mask_size"][i]), int(g["nof_written"][i])
        rows = np.stack([g["w_port"][wpos: wpos + nw], g["w_symbol"][wpos: wpos + nw], g["w_subcarrier"][wpos: wpos + nw],
                         g["w_word"][wpos: wpos + nw]], axis=1).astype(np.int64)
        yield cfg, g["payload"][ppos: ppos + a], g["mask"][mpos: mpos + nm], g["encoded"][epos: epos + e], rows
        ppos, epos, mpos, wpos = ppos + a, epos + e, mpos + nm, wpos + nw


def pack_payloads(rng, payloads, guard=3):
    """Packs payload bit arrays MSB first at unaligned byte offsets with random guard bytes around each: (buffer,
    byte offsets)."""
    chunks, offsets, pos = [], [], 0
    for bits in payloads:
        g = rng.integers(0, 256, int(rng.integers(1, guard + 1))).astype(np.uint8)
        chunks.append(g)
        pos += g.size
        offsets.append(pos)
        packed = np.packbits(np.asarray(bits, np.uint8))
        if bits.size % 8:  # the unused low bits of the last byte are noise the kernel must ignore
            packed[-1] |= rng.integers(0, 1 << (8 - bits.size % 8))
        chunks.append(packed)
        pos += packed.size
    chunks.append(rng.integers(0, 256, guard).astype(np.uint8))
    return np.concatenate(chunks), offsets


def random_plan_cases(rng, nof_grids=4, per_grid=55):
    """About nof_grids x per_grid DCIs on disjoint CCEs of CORESETs that do not overlap within a grid (one CORESET per
    start symbol range), 52 PRB x 4 ports, linear amplitudes. Returns (cfg with grid_index, payload bits)."""
    out = []
    # CORESETs on disjoint symbols of a slot, all three mapping types.
    coresets = (dict(TEMPLATES[3], start_symbol=0), dict(TEMPLATES[1], start_symbol=1), dict(TEMPLATES[9], start_symbol=3),
                dict(TEMPLATES[13], start_symbol=6), dict(TEMPLATES[6], start_symbol=8), dict(TEMPLATES[11], start_symbol=9),
                dict(TEMPLATES[0], start_symbol=12), dict(TEMPLATES[12], start_symbol=13))
    for g in range(nof_grids):
        count = 0
        for cs in coresets:
            free, cce = nof_cces(cs), 0
            while cce < free and count < per_grid:
                fits = [l for l in LEVELS if cce + l <= free]
                if not fits:
                    break
                p = np.array([(0.6, 0.25, 0.1, 0.04, 0.01)[LEVELS.index(l)] for l in fits])
                al = int(rng.choice(fits, p=p / p.sum()))
                sizes = [a for a in (12, 23, 24, 33, 40, 41, 57, 70, 71, 83, 100, 128) if a + 24 < 108 * al]
                cfg, payload = fill_dci(rng, dict(cs, aggregation_level=al, cce_index=cce), int(rng.choice(sizes)))
                ports = int(rng.choice([1, 2, 4]))
                cfg.update(nof_ports=ports, weights=random_weights(rng, ports), grid_index=g,
                           data_scaling=F(rng.choice([1.0, 0.5, 1.4142135, 0.70794576])),
                           dmrs_amplitude=F(rng.choice([1.0, 2.0, 0.8912509, 1.4125375])))
                out.append((cfg, payload))
                cce += al
                count += 1
    return out


def bench_cases(rng, nof_dcis):
    """Mixed levels on a 273-PRB x 4-port grid per 8 DCIs (tools/pdcch_bench.py and --time of the generator)."""
    cs = dict(mapping=INTERLEAVED, bwp_start_rb=0, bwp_size_rb=273, frequency_resources=(1 << 45) - 1, duration=2,
              start_symbol=0, reg_bundle_size=6, interleaver_size=2, shift_index=0, grid_nof_prb=273, grid_nof_ports=4)
    out = []
    for i in range(nof_dcis):
        if i % 8 == 0:
            cce = 0
        al = (1, 2, 4, 8, 16, 4, 2, 8)[i % 8]
        cfg, payload = fill_dci(rng, dict(cs, aggregation_level=al, cce_index=cce), (40, 56, 64, 70, 41, 128, 77, 60)[i % 8])
        cce += al
        cfg.update(nof_ports=4, weights=random_weights(rng, 4), grid_index=i // 8, data_scaling=F(1.0),
                   dmrs_amplitude=F(1.0), data_power_offset_dB=0.0, dmrs_power_offset_dB=0.0)
        out.append((cfg, payload))
    return out
