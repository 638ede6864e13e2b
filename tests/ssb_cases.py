"""The SS/PBCH block (TS 38.211 sections 7.3.3, 7.4.2, 7.4.3; TS 38.212 section 7.1; TS 38.213 section 4.1) restated in
integers and float32: the 864 rate-matched PBCH bits, l_start / k_start and the exact bf16 grid words of
ssb_processor_impl::process, the cases of the fixture tests/golden/ssb.npz (tools/gen_ssb_golden.py records the
reference's values for them) and of the GPU tests.

A case is a dict: phys_cell_id, ssb_idx, L_max, pattern_case (0..4 = A..E), common_scs (numerology), offset_to_pointA,
subcarrier_offset (k_SSB), sfn, slot_index (within the half frame, in slots of the block's SCS), hrf, beta_pss_dB,
pss_amplitude (float32, linear), ports (list), payload (24 bits), grid_nof_prb, grid_nof_ports and, in a plan,
grid_index.

`perturb` names one deliberate error of the restatement (tests/test_ssb_oracle.py: the fixture must see it)."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import pdcch_cases as P  # noqa: E402
import uci_polar_cases as U  # noqa: E402
from pusch_demod_oracle import gold_sequence  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "ssb.npz")
F = np.float32
SENTINEL = 0x7FC17FC1  # grid prefill: a NaN pattern no product rounds to
CASE_A, CASE_B, CASE_C, CASE_D, CASE_E = range(5)
E_BITS = 864
# TS 38.212 Table 7.1.1-1: the PBCH payload interleaver pattern G(j).
G = (16, 23, 18, 17, 8, 30, 10, 6, 24, 7, 0, 5, 3, 2, 1, 4, 9, 11, 12, 13, 14, 15, 19, 20, 21, 22, 25, 26, 27, 28, 29, 31)
SSB_KHZ = (15, 30, 30, 120, 240)
# TS 38.213 section 4.1: first symbols of the candidate blocks in a half frame, and the n of cases D and E.
FIRST_SYMBOLS = ((2, 8), (4, 8, 16, 20), (2, 8), (4, 8, 16, 20), (8, 12, 16, 20, 32, 36, 40, 44))
PERIOD = (14, 28, 14, 28, 56)
N_FR2 = (0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 12, 13, 15, 16, 17, 18)
CFG_INT_KEYS = ("phys_cell_id", "ssb_idx", "L_max", "pattern_case", "common_scs", "offset_to_pointA", "subcarrier_offset",
                "sfn", "slot_index", "hrf", "grid_nof_prb", "grid_nof_ports")


def l_first(pattern_case, ssb_idx):
    """First symbol of the block in the half frame."""
    first = FIRST_SYMBOLS[pattern_case]
    n = ssb_idx // len(first)
    if pattern_case >= CASE_D:
        n = N_FR2[n]
    return first[ssb_idx % len(first)] + PERIOD[pattern_case] * n


def k_first(cfg):
    """First subcarrier of the block from point A in subcarriers of the block's SCS, or None when it is no integer."""
    fr2 = cfg["pattern_case"] >= CASE_D
    khz = (60 * 12 * cfg["offset_to_pointA"] + (15 << cfg["common_scs"]) * cfg["subcarrier_offset"]) if fr2 else \
        15 * (12 * cfg["offset_to_pointA"] + cfg["subcarrier_offset"])
    scs = SSB_KHZ[cfg["pattern_case"]]
    return khz // scs if khz % scs == 0 else None


def refusal(cfg, grid_nof_prb, grid_nof_ports):
    """The keyword of the first rule that refuses the block, in the plan's order; None when it is accepted."""
    if cfg["pattern_case"] > CASE_E:
        return "pattern case"
    if cfg["L_max"] not in (4, 8, 64):
        return "L_max"
    if cfg["ssb_idx"] >= cfg["L_max"]:
        return "ssb_idx"
    if cfg["phys_cell_id"] > 1007:
        return "phys_cell_id"
    fr2 = cfg["pattern_case"] >= CASE_D
    if cfg["common_scs"] > 4 or (cfg["common_scs"] < 2 if fr2 else cfg["common_scs"] > 2):
        return "Common SCS"
    if cfg["offset_to_pointA"] > 2199:
        return "offset to Point A"
    if cfg["subcarrier_offset"] > (11 if fr2 else 23):
        return "subcarrier offset"
    if k_first(cfg) is None:
        return "Unsupported combination"
    first = l_first(cfg["pattern_case"], cfg["ssb_idx"])
    if first // 14 != cfg["slot_index"]:
        return "slot index"
    if cfg["hrf"] > 1:
        return "hrf"
    if first % 14 + 4 > 14:
        return "symbols"
    if k_first(cfg) + 240 > 12 * grid_nof_prb:
        return "subcarriers"
    ports = list(cfg["ports"])
    if not 1 <= len(ports) <= 4:
        return "number of ports"
    if any(p >= grid_nof_ports for p in ports):
        return "port outside"
    if len(set(ports)) != len(ports):
        return "port twice"
    if not np.isfinite(cfg["pss_amplitude"]):
        return "pss_amplitude"
    return None


def payload_bits(cfg):
    """a: the 32 bits of TS 38.212 section 7.1.1."""
    a = np.zeros(32, np.uint8)
    j_sfn, j_other = 0, 14
    for i, b in enumerate(cfg["payload"]):
        if 1 <= i < 7:
            a[G[j_sfn]] = b
            j_sfn += 1
        else:
            a[G[j_other]] = b
            j_other += 1
    for shift in (3, 2, 1, 0):
        a[G[j_sfn]] = (cfg["sfn"] >> shift) & 1
        j_sfn += 1
    a[G[10]] = cfg["hrf"]
    if cfg["L_max"] == 64:
        a[G[11]], a[G[12]], a[G[13]] = (cfg["ssb_idx"] >> 5) & 1, (cfg["ssb_idx"] >> 4) & 1, (cfg["ssb_idx"] >> 3) & 1
    else:
        a[G[11]] = (cfg["subcarrier_offset"] >> 4) & 1
    return a


def first_scrambling(cfg, a, perturb=None):
    m = 26 if cfg["L_max"] == 64 else 29
    v = 2 * int(a[G[7]]) + int(a[G[8]])
    c = gold_sequence(cfg["phys_cell_id"], m * v + 32)[m * v:]
    plain = {G[10], G[7], G[8]} | ({G[11], G[12], G[13]} if cfg["L_max"] == 64 else set())
    if perturb == "hrf_scrambled":
        plain.discard(G[10])
    out, j = a.copy(), 0
    for i in range(32):
        if i not in plain:
            out[i] ^= c[j]
            j += 1
    return out


def encode(cfg, perturb=None):
    """The 864 rate-matched bits of pbch_encoder_impl::encode."""
    a_prime = first_scrambling(cfg, payload_bits(cfg), perturb)
    rem = P.crc24c_remainder([int(b) for b in a_prime] + [0] * 24)
    c = np.concatenate([a_prime, [(rem >> (23 - i)) & 1 for i in range(24)]]).astype(np.uint8)
    code = P.dl_code(56, E_BITS)
    u = np.zeros(code["N"], np.uint8)
    u[code["info"]] = c[code["pi"]]
    return U.polar_transform(u)[code["gather"]]


@functools.lru_cache(maxsize=None)
def m_sequences():
    """x of the PSS (TS 38.211 section 7.4.2.2.1) and x0, x1 of the SSS (7.4.2.3.1), 127 bits each."""
    def lfsr(init, tap):
        x = list(init)
        for i in range(127):
            x.append((x[i + tap] + x[i]) % 2)
        return np.array(x[:127], np.int64)
    return lfsr((0, 1, 1, 0, 1, 1, 1), 4), lfsr((1, 0, 0, 0, 0, 0, 0), 4), lfsr((1, 0, 0, 0, 0, 0, 0), 1)


def to_bf16(v):
    u = np.asarray(v, F).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)


def words(re, im):
    return to_bf16(re) | (to_bf16(im) << 16)


def dmrs_c_init(cfg, perturb=None):
    i_ssb = cfg["ssb_idx"] & 7
    if cfg["L_max"] == 4:
        i_ssb = (cfg["ssb_idx"] & 3) + (0 if perturb == "c_init_without_hrf" else 4 * cfg["hrf"])
    n_id = cfg["phys_cell_id"]
    return (((i_ssb + 1) * (n_id // 4 + 1)) << 11) + ((i_ssb + 1) << 6) + n_id % 4


def process(cfg, perturb=None):
    """(l_start, k_start, rate-matched bits, written grid words as (port, symbol, subcarrier, word) rows sorted by port,
    symbol, subcarrier)."""
    l0, k0 = l_first(cfg["pattern_case"], cfg["ssb_idx"]) % 14, k_first(cfg)
    bits = encode(cfg, perturb)
    n_id = cfg["phys_cell_id"]
    v = n_id % 4
    if perturb == "v_off_by_one":
        v = (v + 1) % 4
    # PBCH: second scrambling, QPSK, the REs of symbols 1, 2 (RBs 0-3 and 16-19) and 3 without the DM-RS subcarriers.
    skip = 0 if perturb == "no_ssb_idx_advance" else (cfg["ssb_idx"] & 7) * E_BITS
    scr = bits ^ gold_sequence(n_id, skip + E_BITS)[skip:]
    a = F(np.sqrt(0.5))
    sym, sc = [], []
    for l, ks in ((1, range(240)), (2, list(range(48)) + list(range(192, 240))), (3, range(240))):
        ks = np.array(ks)
        sym.append(np.full(ks.size, l))
        sc.append(ks)
    sym, sc = np.concatenate(sym), np.concatenate(sc)
    is_dmrs = sc % 4 == v
    assert (~is_dmrs).sum() == 432 and is_dmrs.sum() == 144
    re, im = np.zeros(sym.size, F), np.zeros(sym.size, F)
    re[~is_dmrs] = np.where(scr[0::2] == 1, -a, a)
    im[~is_dmrs] = np.where(scr[1::2] == 1, -a, a)
    # PBCH DM-RS: 144 values on v, v + 4, ... of the same REs.
    seq = gold_sequence(dmrs_c_init(cfg, perturb), 288)
    re[is_dmrs] = np.where(seq[0::2] == 1, -a, a)
    im[is_dmrs] = np.where(seq[1::2] == 1, -a, a)
    # PSS on symbol 0 and SSS on symbol 2, subcarriers 56..182.
    x, x0, x1 = m_sequences()
    nid1, nid2 = n_id // 3, n_id % 3
    n = np.arange(127)
    amp = F(cfg["pss_amplitude"])
    pss = (1 - 2 * x[(n + 43 * nid2) % 127]).astype(F)
    d0 = (1 - 2 * x0[(n + 15 * (nid1 // 112) + 5 * nid2) % 127]).astype(F)
    d1 = (1 - 2 * x1[(n + nid1 % 112) % 127]).astype(F)
    zero = F(0)
    # The reference scales (d, 0) by the amplitude, and multiplies the SSS's two sequences as complex numbers.
    ar, ai = (d0 * F(1)).astype(F), np.full(127, zero * F(1), F)
    sss_re = ((ar * d1).astype(F) - (ai * zero).astype(F)).astype(F)
    sss_im = ((ar * zero).astype(F) + (ai * d1).astype(F)).astype(F)
    sym = np.concatenate([sym, np.zeros(127, np.int64), np.full(127, 2)])
    sc = np.concatenate([sc, 56 + n, 56 + n])
    re = np.concatenate([re, (pss * amp).astype(F), sss_re])
    im = np.concatenate([im, np.full(127, zero * amp, F), sss_im])
    word = words(re, im)
    rows = [np.stack([np.full(sym.size, p), l0 + sym, k0 + sc, word], axis=1) for p in cfg["ports"]]
    rows = np.concatenate(rows).astype(np.int64)
    return l0, k0, bits, rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]


def apply_rows(grid_words, rows):
    """Writes (port, symbol, subcarrier, word) rows into a (ports, 14, nsc) uint32 grid."""
    grid_words[rows[:, 0], rows[:, 1], rows[:, 2]] = rows[:, 3].astype(np.uint32)


def expected_grid(cfg, grid_nof_prb=None, grid_nof_ports=None):
    """The (ports, 14, nsc) grid after the block alone on a sentinel-filled grid."""
    want = np.full((grid_nof_ports or cfg["grid_nof_ports"], 14, 12 * (grid_nof_prb or cfg["grid_nof_prb"])), SENTINEL,
                   np.uint32)
    apply_rows(want, process(cfg)[3])
    return want


def reserved_patterns(cfg):
    """The block's REs as (rb_begin, rb_end, rb_stride, re_mask, symbol_mask) patterns for a k_start that is a multiple
    of 12: what a PDSCH reserves, the REs the reference leaves untouched on symbols 0 and 2 included."""
    l0, k0 = l_first(cfg["pattern_case"], cfg["ssb_idx"]) % 14, k_first(cfg)
    assert k0 % 12 == 0
    return [(k0 // 12, k0 // 12 + 20, 1, 0xFFF, 0xF << l0)]


def pack_payload(cfg):
    """The four bytes the plan reads per block: the 24 payload bits MSB first, then sfn & 15."""
    return np.concatenate([np.packbits(np.asarray(cfg["payload"], np.uint8)), [cfg["sfn"] & 15]]).astype(np.uint8)


# ---- cases -------------------------------------------------------------------------------------------------------

L_MAX_OF = {CASE_A: (4, 8), CASE_B: (4, 8), CASE_C: (4, 8), CASE_D: (64,), CASE_E: (64,)}


def make_case(rng, pattern_case, L_max, ssb_idx, phys_cell_id=None, hrf=None, ports=(0,), beta_pss_dB=0.0,
              offset_to_pointA=None, subcarrier_offset=None, common_scs=None, grid_nof_prb=52, grid_nof_ports=4,
              grid_index=0):
    fr2 = pattern_case >= CASE_D
    if common_scs is None:
        common_scs = int(rng.integers(3, 5)) if fr2 else int(rng.integers(0, 2))
    cfg = dict(phys_cell_id=int(rng.integers(0, 1008)) if phys_cell_id is None else phys_cell_id, ssb_idx=ssb_idx,
               L_max=L_max, pattern_case=pattern_case, common_scs=common_scs, sfn=int(rng.integers(0, 1024)),
               slot_index=l_first(pattern_case, ssb_idx) // 14, hrf=int(rng.integers(0, 2)) if hrf is None else hrf,
               beta_pss_dB=F(beta_pss_dB), pss_amplitude=F(10 ** (np.float64(F(beta_pss_dB)) / 20)), ports=list(ports),
               payload=rng.integers(0, 2, 24).astype(np.uint8), grid_nof_prb=grid_nof_prb, grid_nof_ports=grid_nof_ports,
               grid_index=grid_index)
    while True:
        cfg["offset_to_pointA"] = int(rng.integers(0, 12)) if offset_to_pointA is None else offset_to_pointA
        cfg["subcarrier_offset"] = int(rng.integers(0, 12 if fr2 else 24)) if subcarrier_offset is None else subcarrier_offset
        k = k_first(cfg)
        if k is not None and k + 240 <= 12 * grid_nof_prb:
            return cfg
        assert offset_to_pointA is None or subcarrier_offset is None, cfg


# Block indices whose four symbols lie in one slot (case E starts two of every eight on symbol 12).
def usable_indices(pattern_case, L_max):
    return [i for i in range(L_max) if l_first(pattern_case, i) % 14 + 4 <= 14]


def golden_generator_cases(rng):
    """The fixture's cases: pattern cases A-E at every L_max they have, both half frames, all four v, N_id 0 and 1007,
    k_SSB below and from 16, ssb_idx from 8 on, port lists of one to four ports with a non-contiguous one, PSS
    amplitudes 1 and 10^(3/20)."""
    port_lists = ((0,), (1,), (0, 1), (3, 1), (0, 1, 2), (0, 2, 3), (0, 1, 2, 3), (2,))
    cases = []
    for pattern_case, l_maxes in L_MAX_OF.items():
        for L_max in l_maxes:
            usable = usable_indices(pattern_case, L_max)
            for t, idx in enumerate([usable[0], usable[-1]] + [int(i) for i in rng.choice(usable, 4)]):
                cases.append(make_case(rng, pattern_case, L_max, idx, hrf=t % 2, ports=port_lists[(len(cases)) % 8],
                                       beta_pss_dB=3.0 if t % 3 == 0 else 0.0))
    for n_id in (0, 1, 2, 3, 1004, 1005, 1006, 1007):
        cases.append(make_case(rng, CASE_A, 4, n_id % 4, phys_cell_id=n_id, hrf=(n_id // 2) % 2))
    for k_ssb, case in ((0, CASE_A), (15, CASE_A), (16, CASE_A), (23, CASE_A), (16, CASE_C), (22, CASE_B), (11, CASE_D)):
        cases.append(make_case(rng, case, L_MAX_OF[case][-1], 1, subcarrier_offset=k_ssb, common_scs=3 if case == CASE_D else None))
    cases.append(make_case(rng, CASE_E, 64, 63, offset_to_pointA=4, subcarrier_offset=0, ports=(0, 3), beta_pss_dB=3.0))
    # The last 20 PRBs of a 273-PRB grid at 30 kHz: 3036 subcarriers = 506 RBs of 15 kHz.
    cases.append(make_case(rng, CASE_C, 8, 7, offset_to_pointA=506, subcarrier_offset=0, grid_nof_prb=273,
                           grid_nof_ports=1))
    return cases


def golden_cases():
    """(cfg, l_start, k_start, rate-matched bits, written rows) of every fixture case."""
    z = np.load(GOLDEN)
    rows = np.stack([z["w_port"], z["w_symbol"], z["w_subcarrier"], z["w_word"]], axis=1).astype(np.int64)
    pos = 0
    for i in range(z["cfg"].shape[0]):
        cfg = {k: int(v) for k, v in zip(CFG_INT_KEYS, z["cfg"][i])}
        cfg["beta_pss_dB"], cfg["pss_amplitude"] = F(z["beta_pss_dB"][i]), F(z["pss_amplitude"][i])
        cfg["ports"] = [int(p) for p in z["ports"][i][: int(z["nof_ports"][i])]]
        cfg["payload"] = z["payload"][i].copy()
        n = int(z["nof_written"][i])
        yield cfg, int(z["l_start"][i]), int(z["k_start"][i]), np.unpackbits(z["encoded"][i]), rows[pos: pos + n]
        pos += n
    assert pos == rows.shape[0]


def random_plan_cases(rng, nof_grids=3, grid_nof_prb=52):
    """Two blocks per slot grid where the pattern has two in a slot, of every pattern case."""
    cases = []
    for g in range(nof_grids):
        pattern_case = int(rng.integers(0, 5))
        L_max = int(rng.choice(L_MAX_OF[pattern_case]))
        usable = usable_indices(pattern_case, L_max)
        first = int(rng.choice(usable))
        slot = l_first(pattern_case, first) // 14
        same = [i for i in usable if l_first(pattern_case, i) // 14 == slot]
        n_id, hrf = int(rng.integers(0, 1008)), int(rng.integers(0, 2))
        for idx in same[:2]:
            ports = sorted(int(p) for p in rng.choice(4, int(rng.integers(1, 5)), replace=False))
            cases.append(make_case(rng, pattern_case, L_max, idx, phys_cell_id=n_id, hrf=hrf, ports=ports,
                                   beta_pss_dB=float(rng.choice([0.0, 3.0])), grid_nof_prb=grid_nof_prb, grid_index=g))
    return cases
