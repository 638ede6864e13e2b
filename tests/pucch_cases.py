"""PUCCH Format 0 / 1 test infrastructure: a float64 numpy restatement of the reference's two detectors, the matching
transmitters (which the reference, being a gNB, does not have), a simple channel, and seeded case generators.

  n_cs, alpha     include/srsran/phy/upper/pucch_helper.h:81 (c_init = n_id, byte nsymb n_slot + symbol, bit-reversed),
                  :52 (u = n_id mod 30, v = 0)
  Format 0        lib/phy/upper/channel_processors/pucch/pucch_detector_format0.cpp:46 (tables), :69 (thresholds), :114
  Format 1        pucch_detector_format1.cpp:156 (detect), :512 (process_hop), :288 (combine_symbols), :334
                  (estimate_channels), :376 (estimate_noise), :406 (rebuilt DM-RS), :464 (contributions), :108
                  (detect_symbol); include/srsran/phy/upper/pucch_orthogonal_sequence.h:43 (w)
  transmitters    TS 38.211 sections 6.3.2.3 (Format 0), 6.3.2.4 and 6.4.1.3.1 (Format 1), TS 38.213 section 9.2.3 / 9.2.5

Pinned to the reference's own outputs by tests/test_pucch_oracle.py through tests/golden/pucch_detector.npz
(tools/gen_pucch_golden.py). TEST INFRASTRUCTURE ONLY."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
from low_papr_tables import PHI  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "pucch_detector.npz")
NO_HOP = 0xFFFF
NAN_WORD = 0x7FC07FC0   # bf16 NaN in both halves: grid prefill of the GPU tests
HUGE_WORD = 0x714A714A  # bf16 1e30 in both halves
PERTURBATIONS = ("rsrp_unweighted", "no_pruning", "noise_all_symbols", "w_not_conj", "ncs_no_reversal",
                 "hop1_first_dmrs", "f0_noise_no_12")

F0_KEYS = ("slot_index", "numerology", "cp_extended", "starting_prb", "second_hop_prb", "start_symbol", "nof_symbols",
           "initial_cyclic_shift", "n_id", "nof_harq_ack", "sr_opportunity", "nof_ports", "port0", "port1", "port2",
           "port3", "grid_nof_ports")
F1_KEYS = ("slot_index", "numerology", "cp_extended", "starting_prb", "second_hop_prb", "start_symbol", "nof_symbols",
           "n_id", "nof_ports", "nof_entries")
CLASS_NOISE, CLASS_THRESHOLD, CLASS_HIGH = 0, 1, 2

# pick_threshold's table (pucch_detector_format0.cpp:82): ((ports x symbols, sequences), threshold), sorted.
F0_THRESHOLDS = (((1, 1), 0.5373), ((1, 2), 0.6460), ((1, 4), 0.7556), ((1, 8), 1.6818), ((2, 1), 0.5273),
                 ((2, 2), 0.4038), ((2, 4), 0.7273), ((2, 8), 0.8364), ((4, 1), 0.3455), ((4, 2), 0.2800),
                 ((4, 4), 0.4455), ((4, 8), 0.5000), ((8, 1), 0.2545), ((8, 2), 0.2083), ((8, 4), 0.3000),
                 ((8, 8), 0.3273))
F1_THRESHOLDS = {1: 0.9, 2: 3.0, 4: 4.45, 8: 6.95}  # pucch_detector_format1.cpp:197, by ports x hops

# Candidates (m_cs, (sr, ack0, ack1)) in the order of the reference's tables (pucch_detector_format0.cpp:46-67).
F0_TABLES = {
    (0, 1): ((0, (1, 0, 0)),),
    (1, 0): ((0, (0, 0, 0)), (6, (0, 1, 0))),
    (2, 0): ((0, (0, 0, 0)), (3, (0, 0, 1)), (6, (0, 1, 1)), (9, (0, 1, 0))),
    (1, 1): ((0, (0, 0, 0)), (6, (0, 1, 0)), (3, (1, 0, 0)), (9, (1, 1, 0))),
    (2, 1): ((0, (0, 0, 0)), (3, (0, 0, 1)), (6, (0, 1, 1)), (9, (0, 1, 0)), (1, (1, 0, 0)), (4, (1, 0, 1)),
             (7, (1, 1, 1)), (10, (1, 1, 0))),
}


# ---- number formats --------------------------------------------------------------------------------------------

def to_bf16_words(x):
    """Complex array -> uint32 words re | im << 16, each part rounded from float32 to bf16 half to even."""
    def half(v):
        u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
        return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    x = np.asarray(x)
    return half(x.real) | (half(x.imag) << np.uint32(16))


def words_to_complex(words):
    w = np.asarray(words, np.uint32)
    re = (w << np.uint32(16)).view(np.float32).astype(np.float64)
    im = (w & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    return re + 1j * im


# ---- sequences -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gold_bytes(c_init):
    """The bits c(0 .. 8 * 14 * 160) of the TS 38.211 section 5.2.1 Gold sequence."""
    n = 8 * 14 * 160
    x1, x2 = 1, c_init & 0x7FFFFFFF
    out = np.zeros(n, np.uint8)
    for k in range(1600 + n):
        if k >= 1600:
            out[k - 1600] = (x1 ^ x2) & 1
        x1 = (x1 >> 1) | ((((x1 >> 3) ^ x1) & 1) << 30)
        x2 = (x2 >> 1) | ((((x2 >> 3) ^ (x2 >> 2) ^ (x2 >> 1) ^ x2) & 1) << 30)
    return out


def nsymb_per_slot(cp_extended):
    return 12 if cp_extended else 14


def n_cs(n_id, nsymb, n_slot, symbol, reverse=True):
    """pucch_helper.h:105: the byte nsymb n_slot + symbol of c (MSB first), then reverse_byte: n_cs = sum 2^m c(8 b + m)."""
    bits = _gold_bytes(n_id)[8 * (nsymb * n_slot + symbol):][:8]
    weights = (1 << np.arange(8)) if reverse else (1 << np.arange(7, -1, -1))
    return int(np.sum(bits.astype(np.int64) * weights))


def low_papr(u, alpha_idx):
    """r_{u,0}^{alpha}(n) = exp(j (phi(n) pi / 4 + 2 pi alpha_idx n / 12)), n = 0..11."""
    n = np.arange(12)
    return np.exp(1j * (np.asarray(PHI[12][u]) * np.pi / 4 + 2 * np.pi * alpha_idx * n / 12))


def w_sequence(n, i):
    """TS 38.211 Table 6.3.2.4.1-2: w_i(m) = exp(j 2 pi phi(m) / N)."""
    if n == 4:
        phi = ((0, 0, 0, 0), (0, 2, 0, 2), (0, 0, 2, 2), (0, 2, 2, 0))[i]
    else:
        phi = [(i * m) % n for m in range(n)]
    return np.exp(2j * np.pi * np.asarray(phi) / n)


def hop_split(nof_symbols, hopping, hop1_first_dmrs=False):
    """pucch_detector_format1.cpp:165 and :519-541 -> [(first allocated symbol, [is DM-RS per symbol])] per hop. Every
    other allocated symbol from the first is DM-RS, across the hop border."""
    mask = [(i % 2) == 0 for i in range(nof_symbols)]
    if not hopping:
        return [(0, mask)]
    half = nof_symbols // 2
    second = mask[half:]
    if hop1_first_dmrs:  # perturbation: the second hop numbered from its own first symbol
        second = [(i % 2) == 0 for i in range(nof_symbols - half)]
    return [(0, mask[:half]), (half, second)]


def alpha_indices(cfg, m0, reverse=True):
    nsymb = nsymb_per_slot(cfg["cp_extended"])
    return [(m0 + n_cs(cfg["n_id"], nsymb, cfg["slot_index"], cfg["start_symbol"] + i, reverse)) % 12
            for i in range(cfg["nof_symbols"])]


# ---- Format 0 --------------------------------------------------------------------------------------------------

def f0_threshold(nof_ports, nof_symbols, nof_sequences):
    """std::lower_bound over the pairs in lexicographic order (pucch_detector_format0.cpp:101)."""
    for key, value in F0_THRESHOLDS:
        if key >= (nof_ports * nof_symbols, nof_sequences):
            return float(np.float32(value))
    raise ValueError("past the table")


def detect_f0(cfg, x, perturb=()):
    """pucch_detector_format0.cpp:114. x: (nof_symbols, nof_ports, 12) complex. -> dict."""
    table = F0_TABLES[(cfg["nof_harq_ack"], cfg["sr_opportunity"])]
    nsym, nports = x.shape[0], x.shape[1]
    alphas = alpha_indices(cfg, cfg["initial_cyclic_shift"], "ncs_no_reversal" not in perturb)
    u = cfg["n_id"] % 30
    power = np.sum(np.abs(x) ** 2, axis=2) / 12                       # :203 average_power per (symbol, port)
    epre = float(np.sum(power) / (nsym * nports))                      # :162-168
    metrics, corrs, noises = [], [], []
    for m_cs, _ in table:
        sum_corr = sum_noise = 0.0
        for s in range(nsym):
            seq = low_papr(u, (alphas[s] + m_cs) % 12)                 # :189-195
            for p in range(nports):
                corr = np.sum(x[s, p] * np.conj(seq))                  # :206 dot_prod conjugates its second argument
                contribution = abs(corr) ** 2 / 12                     # :209
                sum_corr += contribution
                if "f0_noise_no_12" in perturb:
                    sum_noise += power[s, p] - contribution
                else:
                    sum_noise += power[s, p] * 12 - contribution       # :211
        normal = np.isfinite(sum_noise) and abs(sum_noise) >= np.finfo(np.float32).tiny
        metrics.append(sum_corr / sum_noise if normal else 0.0)        # :216-219
        corrs.append(sum_corr)
        noises.append(sum_noise)
    best, best_i = 0.0, None
    for i, m in enumerate(metrics):                                    # :222 the first strictly largest
        if m > best:
            best, best_i = m, i
    threshold = f0_threshold(nports, nsym, len(table))
    message = table[best_i][1] if best_i is not None else (0, 0, 0)
    ordered = sorted(metrics, reverse=True)
    gap = (ordered[0] - ordered[1]) / ordered[0] if len(ordered) > 1 and ordered[0] > 0 else 1.0
    return dict(sr=message[0], harq=message[1:], valid=best > threshold, metric=best, epre=epre,
                rsrp=corrs[best_i] if best_i is not None else 0.0,
                noise_var=noises[best_i] if best_i is not None else 0.0, threshold=threshold, gap=gap)


def f0_m_cs(nof_harq_ack, sr, harq):
    """TS 38.213 Tables 9.2.3-3 / -4 (no or negative SR) and 9.2.5-1 / -2 (positive SR); SR alone: m_cs = 0."""
    if nof_harq_ack == 0:
        return 0
    if nof_harq_ack == 1:
        return (0, 6)[harq[0]] + (3 if sr else 0)
    return {(0, 0): 0, (0, 1): 3, (1, 1): 6, (1, 0): 9}[tuple(harq)] + (1 if sr else 0)


def tx_f0(cfg, sr, harq):
    """TS 38.211 section 6.3.2.3: x(12 l + n) = r_{u,v}^{alpha, delta}(n) -> (nof_symbols, 12)."""
    m_cs = f0_m_cs(cfg["nof_harq_ack"], sr, harq)
    alphas = alpha_indices(cfg, cfg["initial_cyclic_shift"])
    return np.array([low_papr(cfg["n_id"] % 30, (a + m_cs) % 12) for a in alphas])


# ---- Format 1 --------------------------------------------------------------------------------------------------

def detect_symbol(nof_bits, cross):
    """pucch_detector_format1.cpp:108 -> (bits, metric_cross, margin). margin: what decides the bits, relative to |cross|."""
    a = np.sqrt(0.5)
    m1 = (complex(a, a) * cross).real
    mag = abs(cross) if abs(cross) > 0 else 1.0
    if nof_bits != 2:
        return ([0], m1, abs(m1) / mag) if m1 > 0 else ([1], -m1, abs(m1) / mag)
    m2 = (complex(a, -a) * cross).real
    bits, metric = [0, 0], m1
    if abs(m2) > abs(m1):
        bits, metric = [0, 1], m2
    margin = min(abs(abs(m1) - abs(m2)), abs(metric)) / mag
    if metric < 0:
        bits, metric = [1 - b for b in bits], -metric
    return bits, metric, margin


def process_hop(x, alphas, u, first, mask, occs, perturb=()):
    """pucch_detector_format1.cpp:512 for the hop's symbols x (n, ports, 12) -> (per OCC (main, cross, rsrp) arrays over
    the 12 shifts, EPRE sum and samples, noise sum and samples)."""
    nports = x.shape[1]
    n_idx, k_idx = np.meshgrid(np.arange(12), np.arange(12), indexing="ij")
    dft_m = np.exp(-2j * np.pi * n_idx * k_idx / 12)                   # unnormalised direct 12-point DFT, [n, k]
    lse = np.array([x[i] * np.conj(low_papr(u, alphas[first + i]))[None, :] for i in range(len(mask))])  # :567 / :580
    dft = lse @ dft_m                                                  # :569-572
    is_dmrs = np.asarray(mask, bool)
    dmrs_lse, dmrs_dft, data_dft = lse[is_dmrs], dft[is_dmrs], dft[~is_dmrs]
    nm, nd = dmrs_dft.shape[0], data_dft.shape[0]
    rebuilt = np.zeros_like(dmrs_lse)
    out = {}
    for occ in range(nd):                                              # :599
        if occ not in occs:
            continue
        wd, wm = w_sequence(nd, occ), w_sequence(nm, occ)
        wsd, wsm = (wd, wm) if "w_not_conj" in perturb else (np.conj(wd), np.conj(wm))  # :605 get_sequence_conj
        data = np.tensordot(wsd, data_dft, (0, 0)) / np.sqrt(nd)       # :612 combine_symbols -> (ports, 12)
        dmrs = np.tensordot(wsm, dmrs_dft, (0, 0)) / np.sqrt(nm)
        main = np.sum(np.abs(data) ** 2 + np.abs(dmrs) ** 2, axis=0)   # :495-505
        cross = np.sum(dmrs * np.conj(data), axis=0)                   # :499 prod_conj(dmrs, data)
        norm = 1.0 / (12 * (nm + nd))                                  # :621
        ch = dmrs / (np.sqrt(nm) * 12)                                 # :353
        energy = np.sum(np.abs(ch) ** 2, axis=0)                       # :356-359
        if "no_pruning" not in perturb:
            ch = np.where(energy > energy.max() / 10, ch, 0)           # :362-370
        out[occ] = (main * norm, cross * norm, energy / nports)        # :372
        idft = ch @ np.exp(2j * np.pi * np.outer(np.arange(12), np.arange(12)) / 12)  # :433-435, (ports, n)
        rebuilt += np.conj(wsm)[:, None, None] * idft[None, :, :]     # :440
    noise = float(np.sum(np.abs(dmrs_lse - rebuilt) ** 2))             # :401-403
    samples = dmrs_lse.size
    if "noise_all_symbols" in perturb:  # the data symbols, which nothing rebuilds, counted as noise too
        noise += float(np.sum(np.abs(lse[~is_dmrs]) ** 2))
        samples = lse.size
    return out, float(np.sum(np.abs(x) ** 2)), x.size, noise, samples


def detect_f1(cfg, x, perturb=()):
    """pucch_detector_format1.cpp:156. x: (nof_symbols, nof_ports, 12) complex -> (list of dict per entry, noise_var)."""
    hopping = cfg["second_hop_prb"] != NO_HOP
    alphas = alpha_indices(cfg, 0, "ncs_no_reversal" not in perturb)
    u = cfg["n_id"] % 30
    occs = {e[1] for e in cfg["entries"]}
    hops = []
    for first, mask in hop_split(cfg["nof_symbols"], hopping, "hop1_first_dmrs" in perturb):
        hops.append(process_hop(x[first: first + len(mask)], alphas, u, first, mask, occs, perturb))
    epre = sum(h[1] for h in hops) / sum(h[2] for h in hops)           # :189
    noise_var = sum(h[3] for h in hops) / sum(h[4] for h in hops)      # :190
    threshold = float(np.float32(F1_THRESHOLDS[x.shape[1] * len(hops)]))
    results = []
    for ics, occ, nof_bits in cfg["entries"]:
        main = sum(h[0][occ][0][ics] for h in hops)                    # :225-230
        cross = sum(h[0][occ][1][ics] for h in hops)
        if len(hops) == 2 and "rsrp_unweighted" not in perturb:
            n0, n1 = hops[0][4], hops[1][4]
            rsrp = (hops[0][0][occ][2][ics] * n0 + hops[1][0][occ][2][ics] * n1) / (n0 + n1)  # :231
        else:
            rsrp = sum(h[0][occ][2][ics] for h in hops) / len(hops)
        bits, detected, margin = detect_symbol(nof_bits, cross)       # :259
        metric = (main + 2 * detected) / noise_var                     # :260
        valid = metric > threshold                                     # :262
        if valid and nof_bits == 0:
            valid = bits[0] == 0                                       # :268
        results.append(dict(bits=bits, valid=bool(valid), metric=metric / threshold, epre=epre, rsrp=rsrp,
                            noise_var=noise_var, margin=margin))
    return results, noise_var


def modulate(bits):
    """TS 38.211 section 5.1.2 / 5.1.3; no bits (positive SR alone): d(0) of b(0) = 0."""
    if len(bits) == 2:
        return complex(1 - 2 * bits[0], 1 - 2 * bits[1]) / np.sqrt(2)
    b = bits[0] if len(bits) else 0
    return complex(1 - 2 * b, 1 - 2 * b) / np.sqrt(2)


def tx_f1(cfg, ics, occ, bits):
    """TS 38.211 section 6.3.2.4.1 (data on the odd allocated symbols: z = w_i(m) d r(n)) and 6.4.1.3.1.1 (DM-RS on
    the even ones: w_i(m) r(n)), the spreading lengths per hop from Tables 6.3.2.4.1-1 and 6.4.1.3.1.1-1
    -> (nof_symbols, 12)."""
    hopping = cfg["second_hop_prb"] != NO_HOP
    alphas = alpha_indices(cfg, ics)
    u = cfg["n_id"] % 30
    d = modulate(bits)
    out = np.zeros((cfg["nof_symbols"], 12), complex)
    for first, mask in hop_split(cfg["nof_symbols"], hopping):
        nm, nd = sum(mask), len(mask) - sum(mask)
        wd, wm = w_sequence(nd, occ), w_sequence(nm, occ)
        im = idata = 0
        for i, is_dmrs in enumerate(mask):
            r = low_papr(u, alphas[first + i])
            if is_dmrs:
                out[first + i] = wm[im] * r
                im += 1
            else:
                out[first + i] = wd[idata] * d * r
                idata += 1
    return out


# ---- channel ---------------------------------------------------------------------------------------------------

def channel(rng, tx, nof_ports, snr_db, hop_first=None, delay=None):
    """tx (nof_symbols, 12) -> (nof_symbols, nof_ports, 12) without noise: one flat unit-power gain per port (and per
    hop), a timing offset as a phase ramp over the 12 subcarriers, scaled to the SNR over unit-variance noise."""
    nsym = tx.shape[0]
    delay = rng.uniform(-0.15, 0.15) if delay is None else delay
    ramp = np.exp(-2j * np.pi * delay * np.arange(12) / 12)
    out = np.zeros((nsym, nof_ports, 12), complex)
    bounds = [(0, nsym)] if not hop_first else [(0, hop_first), (hop_first, nsym)]
    for a, b in bounds:
        h = np.exp(2j * np.pi * rng.random(nof_ports)) * rng.uniform(0.7, 1.3, nof_ports)
        h /= np.sqrt(np.mean(np.abs(h) ** 2))
        out[a:b] = tx[a:b, None, :] * h[None, :, None] * ramp[None, None, :]
    return out * 10 ** (snr_db / 20)


def awgn(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


# ---- case generators -------------------------------------------------------------------------------------------

def f1_occ_stop(nof_symbols, hopping):
    return min(len(m) - sum(m) for _, m in hop_split(nof_symbols, hopping))


def f1_threshold_snr_db(nof_ports, hopping):
    """Where the metric of a lone PUCCH crosses its threshold: about 24 SNR per contribution."""
    c = nof_ports * (2 if hopping else 1)
    return 10 * np.log10(F1_THRESHOLDS[c] / (24 * c))


def f0_threshold_snr_db(nof_ports, nof_symbols, nof_sequences):
    """Where (12 SNR + 1) / 11 crosses the threshold."""
    return 10 * np.log10(max(11 * f0_threshold(nof_ports, nof_symbols, nof_sequences) - 1, 0.05) / 12)


def make_f1_case(rng, nof_symbols, hopping, nof_ports, entries, snr_class, cp_extended=0, silent=(), snr_db=None):
    """One resource: entries [(ics, occ, nof_bits)]; every entry outside `silent` transmits random bits (SR-only: a
    positive SR). -> (cfg, words (nof_symbols, nof_ports, 12), sent [bits or None per entry], snr class)."""
    numerology = 2 if cp_extended else int(rng.integers(0, 4))
    nsymb = nsymb_per_slot(cp_extended)
    cfg = dict(slot_index=int(rng.integers(0, 10 << numerology)), numerology=numerology, cp_extended=cp_extended,
               starting_prb=int(rng.integers(0, 20)), second_hop_prb=int(rng.integers(0, 20)) if hopping else NO_HOP,
               start_symbol=int(rng.integers(0, min(10, nsymb - nof_symbols) + 1)), nof_symbols=nof_symbols,
               n_id=int(rng.integers(0, 1024)), nof_ports=nof_ports, entries=[tuple(e) for e in entries])
    x = np.zeros((nof_symbols, nof_ports, 12), complex)
    sent = []
    hop_first = nof_symbols // 2 if hopping else None
    for i, (ics, occ, nof_bits) in enumerate(cfg["entries"]):
        if i in silent or snr_class == CLASS_NOISE:
            sent.append(None)
            continue
        bits = [int(b) for b in rng.integers(0, 2, nof_bits)]
        if snr_db is not None:
            snr = snr_db
        elif snr_class == CLASS_HIGH:
            snr = 30.0
        else:
            # 5 dB below the lone-PUCCH estimate: the noise estimate, which the strongest shifts are taken out of, runs low.
            snr = f1_threshold_snr_db(nof_ports, hopping) - 5.0 + rng.uniform(-3.5, 3.5)
        x += channel(rng, tx_f1(cfg, ics, occ, bits), nof_ports, snr, hop_first)
        sent.append(bits)
    x += awgn(rng, x.shape)
    return cfg, to_bf16_words(x * 0.25), sent, snr_class


def random_entries(rng, nof_symbols, hopping, count, kinds=(0, 1, 2)):
    stop = f1_occ_stop(nof_symbols, hopping)
    pairs = [(ics, occ) for occ in range(stop) for ics in range(12)]
    pick = rng.permutation(len(pairs))[: min(count, len(pairs))]
    return [(pairs[i][0], pairs[i][1], int(rng.choice(kinds))) for i in sorted(pick)]


def make_f0_case(rng, nof_symbols, hopping, ports, nof_harq_ack, sr_opportunity, snr_class, grid_nof_ports=4):
    numerology = int(rng.integers(0, 4))
    cfg = dict(slot_index=int(rng.integers(0, 10 << numerology)), numerology=numerology, cp_extended=0,
               starting_prb=int(rng.integers(0, 20)), second_hop_prb=int(rng.integers(0, 20)) if hopping else NO_HOP,
               start_symbol=int(rng.integers(0, 14 - nof_symbols + 1)), nof_symbols=nof_symbols,
               initial_cyclic_shift=int(rng.integers(0, 12)), n_id=int(rng.integers(0, 1024)), nof_harq_ack=nof_harq_ack,
               sr_opportunity=sr_opportunity, ports=list(ports), grid_nof_ports=grid_nof_ports)
    nports = len(ports)
    x = awgn(rng, (nof_symbols, nports, 12))
    sent = None
    if snr_class != CLASS_NOISE:
        sr = int(rng.integers(0, 2)) if sr_opportunity and nof_harq_ack else sr_opportunity
        harq = [int(b) for b in rng.integers(0, 2, nof_harq_ack)]
        nseq = len(F0_TABLES[(nof_harq_ack, sr_opportunity)])
        snr = 30.0 if snr_class == CLASS_HIGH else f0_threshold_snr_db(nports, nof_symbols, nseq) + rng.uniform(-3.5, 3.5)
        x += channel(rng, tx_f0(cfg, sr, harq), nports, snr, 1 if hopping else None)
        sent = (sr if sr_opportunity else 0, harq)
    return cfg, to_bf16_words(x * 0.25), sent, snr_class


F0_PAYLOADS = ((0, 1), (1, 0), (2, 0), (1, 1), (2, 1))  # (nof_harq_ack, sr_opportunity): one per table of the reference
F0_PORT_LISTS = ((0,), (2,), (0, 1), (3, 1), (0, 1, 2), (2, 0, 3), (0, 1, 2, 3), (3, 2, 0, 1))


def golden_generator_cases(rng):
    """The fixture's cases: (Format 0 cases, Format 1 cases), each (cfg, words, sent, class)."""
    f1 = []
    # Every symbol count of the list with and without hopping, 1 / 2 / 4 ports, around the threshold and at 30 dB.
    for nof_symbols in (4, 5, 7, 10, 13, 14):
        for hopping in (False, True):
            for nof_ports in (1, 2, 4):
                for snr_class in (CLASS_THRESHOLD, CLASS_THRESHOLD, CLASS_HIGH):
                    count = int(rng.integers(1, 5))
                    f1.append(make_f1_case(rng, nof_symbols, hopping, nof_ports,
                                           random_entries(rng, nof_symbols, hopping, count), snr_class))
    # Pure noise: 10 to 14 symbols without hopping and one entry at OCC 0. With fewer symbols, or with more OCCs in
    # use, the reference's noise estimate (what is left after the strongest shifts of every OCC in use are rebuilt and
    # taken out) runs so low on pure noise that it reports valid messages far more often than 5 % of the time.
    for nof_ports in (1, 2, 4):
        for nof_symbols in (10, 11, 12, 13, 14, 10, 12, 14, 13, 11, 14, 12):
            f1.append(make_f1_case(rng, nof_symbols, False, nof_ports,
                                   [(int(rng.integers(0, 12)), 0, int(rng.integers(0, 3)))], CLASS_NOISE))
    # Extended CP once; all 84 entries; a single entry; an OCC gap; a silent entry next to strong ones.
    f1.append(make_f1_case(rng, 12, False, 2, random_entries(rng, 12, False, 5), CLASS_HIGH, cp_extended=1))
    f1.append(make_f1_case(rng, 14, False, 2, random_entries(rng, 14, False, 84), CLASS_HIGH, snr_db=12.0))
    f1.append(make_f1_case(rng, 9, False, 1, [(7, 2, 1)], CLASS_HIGH))
    f1.append(make_f1_case(rng, 14, True, 1, [(1, 0, 2), (5, 0, 0), (3, 2, 1), (9, 2, 2)], CLASS_HIGH))
    f1.append(make_f1_case(rng, 8, False, 2, [(0, 0, 1), (4, 0, 2), (4, 1, 0), (8, 1, 1)], CLASS_HIGH, silent=(1,)))
    f1.append(make_f1_case(rng, 11, True, 2, [(2, 0, 0), (6, 0, 1), (10, 1, 2), (3, 1, 0)], CLASS_HIGH, silent=(2,)))
    # Threshold cases of one entry each so that the per-port-count share of valid results is measured on many resources.
    for nof_ports in (1, 2, 4):
        for _ in range(8):
            hopping = bool(rng.integers(0, 2)) and nof_ports * 2 in F1_THRESHOLDS
            nof_symbols = int(rng.integers(4, 15))
            f1.append(make_f1_case(rng, nof_symbols, hopping, nof_ports,
                                   random_entries(rng, nof_symbols, hopping, int(rng.integers(1, 4)), kinds=(1, 2)),
                                   CLASS_THRESHOLD))
    f0 = []
    for payload in F0_PAYLOADS:
        for nof_symbols, hopping in ((1, False), (2, False), (2, True)):
            for ports in F0_PORT_LISTS:
                for snr_class in (CLASS_NOISE, CLASS_THRESHOLD, CLASS_HIGH):
                    f0.append(make_f0_case(rng, nof_symbols, hopping, ports, payload[0], payload[1], snr_class))
    return f0, f1


# ---- the fixture -----------------------------------------------------------------------------------------------

def cfg_rows(f0_cases, f1_cases):
    f0_rows = [[c["slot_index"], c["numerology"], c["cp_extended"], c["starting_prb"], c["second_hop_prb"],
                c["start_symbol"], c["nof_symbols"], c["initial_cyclic_shift"], c["n_id"], c["nof_harq_ack"],
                c["sr_opportunity"], len(c["ports"])] + (list(c["ports"]) + [0] * 4)[:4] + [c["grid_nof_ports"]]
               for c, *_ in f0_cases]
    f1_rows = [[c["slot_index"], c["numerology"], c["cp_extended"], c["starting_prb"], c["second_hop_prb"],
                c["start_symbol"], c["nof_symbols"], c["n_id"], c["nof_ports"], len(c["entries"])] for c, *_ in f1_cases]
    return np.array(f0_rows, np.int64).reshape(-1, len(F0_KEYS)), np.array(f1_rows, np.int64).reshape(-1, len(F1_KEYS))


@functools.lru_cache(maxsize=1)
def golden():
    """The fixture as (npz dict, Format 0 cases, Format 1 cases): each case a dict with cfg, words, the reference's
    results and what was sent."""
    g = dict(np.load(GOLDEN))
    f0, at = [], 0
    for i, row in enumerate(g["f0_cfg"]):
        c = dict(zip(F0_KEYS, (int(v) for v in row)))
        c["ports"] = [c.pop(f"port{p}") for p in range(4)][: c.pop("nof_ports")]
        n = c["nof_symbols"] * len(c["ports"]) * 12
        words = g["f0_words"][at: at + n].reshape(c["nof_symbols"], len(c["ports"]), 12)
        at += n
        f0.append(dict(cfg=c, words=words, status=int(g["f0_status"][i]), bits=g["f0_bits"][i], snr_class=int(g["f0_class"][i]),
                       metric=float(db_to_linear(g["f0_sinr_db"][i])), epre=float(db_to_linear(g["f0_epre_db"][i])),
                       rsrp=float(db_to_linear(g["f0_rsrp_db"][i])), sent=g["f0_sent"][i]))
    f1, at, ent = [], 0, 0
    for i, row in enumerate(g["f1_cfg"]):
        c = dict(zip(F1_KEYS, (int(v) for v in row)))
        ne = c.pop("nof_entries")
        c["entries"] = [tuple(int(v) for v in e) for e in g["f1_entries"][ent: ent + ne]]
        n = c["nof_symbols"] * c["nof_ports"] * 12
        words = g["f1_words"][at: at + n].reshape(c["nof_symbols"], c["nof_ports"], 12)
        at += n
        sl = slice(ent, ent + ne)
        f1.append(dict(cfg=c, words=words, noise_var=float(g["f1_noise_var"][i]), status=g["f1_status"][sl],
                       bits=g["f1_bits"][sl], metric=g["f1_metric"][sl].astype(np.float64),
                       epre=db_to_linear(g["f1_epre_db"][sl]), rsrp=db_to_linear(g["f1_rsrp_db"][sl]),
                       sinr=db_to_linear(g["f1_sinr_db"][sl]), sent=g["f1_sent"][sl], snr_class=int(g["f1_class"][i])))
        ent += ne
    return g, f0, f1


def db_to_linear(v):
    return 10.0 ** (np.asarray(v, np.float64) / 10.0)


# ---- plans for the GPU tests -----------------------------------------------------------------------------------

def place(cases0, cases1, grid_nof_prb, grid_nof_ports, nof_grids, fill=NAN_WORD, grid_of=None):
    """The grids (nof_grids, ports, 14, 12 PRBs) uint32 holding every case's REs, `fill` everywhere else; a case lies in
    grid grid_of(kind, i) (default: its number modulo nof_grids); two cases on the same REs are an error."""
    grids = np.full((nof_grids, grid_nof_ports, 14, 12 * grid_nof_prb), fill, np.uint32)
    taken = np.zeros(grids.shape, bool)

    def put(g, port, symbol, prb, words):
        sl = (g, port, symbol, slice(12 * prb, 12 * prb + 12))
        assert not taken[sl].any(), "two cases share REs"
        grids[sl], taken[sl] = words, True
    for i, (c, words) in enumerate(cases0):
        g = grid_of(0, i) if grid_of else i % nof_grids
        for s in range(c["nof_symbols"]):
            prb = c["second_hop_prb"] if (s and c["second_hop_prb"] != NO_HOP) else c["starting_prb"]
            for p, port in enumerate(c["ports"]):
                put(g, port, c["start_symbol"] + s, prb, words[s, p])
    for i, (c, words) in enumerate(cases1):
        g = grid_of(1, i) if grid_of else i % nof_grids
        for s in range(c["nof_symbols"]):
            hop1 = c["second_hop_prb"] != NO_HOP and s >= c["nof_symbols"] // 2
            for p in range(c["nof_ports"]):
                put(g, p, c["start_symbol"] + s, c["second_hop_prb"] if hop1 else c["starting_prb"], words[s, p])
    return grids


def random_plan_cases(rng, nof_f0=24, nof_f1=24):
    """Fresh shapes for the GPU tests: (Format 0 cases, Format 1 cases) as (cfg, words), PRBs below 20."""
    f0, f1 = [], []
    for _ in range(nof_f0):
        payload = F0_PAYLOADS[int(rng.integers(0, len(F0_PAYLOADS)))]
        nof_symbols = int(rng.integers(1, 3))
        ports = F0_PORT_LISTS[int(rng.integers(0, len(F0_PORT_LISTS)))]
        c = make_f0_case(rng, nof_symbols, nof_symbols == 2 and bool(rng.integers(0, 2)), ports, payload[0], payload[1],
                         int(rng.integers(0, 3)))
        f0.append((c[0], c[1]))
    for _ in range(nof_f1):
        nof_ports = int(rng.choice((1, 2, 4)))
        hopping = bool(rng.integers(0, 2)) and nof_ports * 2 in F1_THRESHOLDS
        nof_symbols = int(rng.integers(4, 15))
        c = make_f1_case(rng, nof_symbols, hopping, nof_ports,
                         random_entries(rng, nof_symbols, hopping, int(rng.integers(1, 9))), int(rng.integers(1, 3)))
        f1.append((c[0], c[1]))
    return f0, f1


# ---- tolerances and decidability (shared by the CPU and the GPU tests) -----------------------------------------

DEGENERATE = 1e-9  # noise variance over EPRE below which the variance is rounding noise (the fixture's gap: 1e-13 | 1e-3)


def rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-300)


def degenerate(case):
    """A fixture resource whose rebuilt DM-RS equals the received one: its noise variance is rounding noise."""
    return case["noise_var"] < DEGENERATE * case["epre"][0]


@functools.lru_cache(maxsize=1)
def restate_golden():
    """The restatement of every fixture case, computed once: ([Format 0 dict], [(Format 1 dicts, noise variance)])."""
    _, f0, f1 = golden()
    return ([detect_f0(c["cfg"], words_to_complex(c["words"])) for c in f0],
            [detect_f1(c["cfg"], words_to_complex(c["words"])) for c in f1])


def measured_deviations(restated):
    """The largest relative deviation of the restatement from the reference's recorded float32 results, per number."""
    _, f0, f1 = golden()
    dev = dict(f0_metric=0.0, f0_epre=0.0, f0_rsrp=0.0, f1_metric=0.0, f1_epre=0.0, f1_rsrp=0.0, f1_noise_var=0.0)
    for c, r in zip(f0, restated[0]):
        for key in ("metric", "epre", "rsrp"):
            dev["f0_" + key] = max(dev["f0_" + key], rel(r[key], c[key]))
    for c, (res, noise_var) in zip(f1, restated[1]):
        if not degenerate(c):
            dev["f1_noise_var"] = max(dev["f1_noise_var"], rel(noise_var, c["noise_var"]))
        for i, r in enumerate(res):
            dev["f1_epre"] = max(dev["f1_epre"], rel(r["epre"], c["epre"][i]))
            dev["f1_rsrp"] = max(dev["f1_rsrp"], rel(r["rsrp"], c["rsrp"][i]))
            if not degenerate(c):
                dev["f1_metric"] = max(dev["f1_metric"], rel(r["metric"], c["metric"][i]))
    return dev


def tolerances(restated):
    """Ten times what float rounding alone moves between the reference and the restatement, floored at 1e-4."""
    return {k: max(10 * v, 1e-4) for k, v in measured_deviations(restated).items()}


def decidable_f0(metric, restated_case, tol):
    """metric: the reference's (or the restatement's) best metric of the case."""
    return abs(metric / restated_case["threshold"] - 1) > tol and restated_case["gap"] > tol


def decidable_f1(metric, restated_entry, tol):
    """metric: the reference's (or the restatement's) metric over its threshold."""
    return abs(metric - 1) > tol and restated_entry["margin"] > tol
