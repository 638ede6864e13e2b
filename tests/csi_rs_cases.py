"""NZP-CSI-RS (TS 38.211 section 7.4.1.5) restated in integers and float32: the exact bf16 grid words of
nzp_csi_rs_generator_impl::map for rows 1-5 of Table 7.4.1.5.3-1, the cases of the fixture tests/golden/csi_rs.npz
(tools/gen_csi_rs_golden.py records the reference's words for them) and of the GPU tests.

A case is a dict: n_slot (in the frame), numerology, cp (0 normal, 1 extended), start_rb, nof_rb, row, k_ref, symbol_l0,
symbol_l1, cdm (0 none, 1 FD-CDM2, 2 CDM4, 3 CDM8), freq_density (0 0.5 on even RBs, 1 0.5 on odd RBs, 2 one, 3 three),
scrambling_id, amplitude (float32), weights ((ports, ports) complex64, [port, layer]), grid_nof_prb, grid_nof_ports
and, in a plan, grid_index.

`perturb` names one deliberate error of the restatement (tests/test_csi_rs_oracle.py: the fixture must see it)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
from pusch_demod_oracle import gold_sequence  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "csi_rs.npz")
F = np.float32
SENTINEL = 0x7FC17FC1  # grid prefill: a NaN pattern no product rounds to

NO_CDM, FD_CDM2, CDM4, CDM8 = 0, 1, 2, 3
DOT5_EVEN, DOT5_ODD, ONE, THREE = 0, 1, 2, 3
ROW_PORTS = {1: 1, 2: 1, 3: 2, 4: 4, 5: 4, 6: 8, 7: 8, 8: 8, 9: 12, 10: 12, 11: 16, 12: 16}
# Per row: (k_ref values, densities, CDM).
ROW_RULES = {1: (range(0, 4), (THREE,), NO_CDM), 2: (range(0, 12), (ONE, DOT5_EVEN, DOT5_ODD), NO_CDM),
             3: (range(0, 11), (ONE, DOT5_EVEN, DOT5_ODD), FD_CDM2), 4: (range(0, 9), (ONE,), FD_CDM2),
             5: (range(0, 11), (ONE,), FD_CDM2)}
CFG_INT_KEYS = ("numerology", "n_slot", "cp", "start_rb", "nof_rb", "row", "k_ref", "symbol_l0", "symbol_l1", "cdm",
                "freq_density", "scrambling_id", "grid_nof_prb", "grid_nof_ports")


def nof_symbols(cfg):
    return 12 if cfg["cp"] else 14


def refusal(cfg, grid_nof_prb, grid_nof_ports):
    """The keyword of the first rule that refuses the signal, in the plan's order; None when it is accepted."""
    row = cfg["row"]
    if row < 1 or row > 18:
        return "Invalid mapping table row"
    if row > 12:
        return "Unsupported mapping table row"
    if row > 5:
        return "grid ports"
    if cfg["cp"] > 1 or cfg["cdm"] > 3 or cfg["freq_density"] > 3:
        return "enumeration"
    k_refs, densities, cdm = ROW_RULES[row]
    if cfg["k_ref"] not in k_refs:
        return "k_0"
    if cfg["freq_density"] not in densities:
        return "invalid density"
    if cfg["cdm"] != cdm:
        return "invalid CDM type"
    if cfg["symbol_l0"] >= nof_symbols(cfg):
        return "l_0"
    if row == 5 and cfg["symbol_l0"] + 1 >= nof_symbols(cfg):
        return "l_0 + 1"
    ports = np.asarray(cfg["weights"]).shape
    if ports != (ROW_PORTS[row], ROW_PORTS[row]):
        return "precoding number of ports"
    if ROW_PORTS[row] > grid_nof_ports:
        return "grid number of ports"
    if cfg["start_rb"] + cfg["nof_rb"] > grid_nof_prb:
        return "RBs"
    if not np.isfinite(cfg["amplitude"]):
        return "amplitude"
    if cfg["scrambling_id"] > 1023:
        return "scrambling_id"
    return None


def rb_comb(cfg, perturb=None):
    """The RBs that carry the signal, ascending."""
    begin, end, stride = cfg["start_rb"], cfg["start_rb"] + cfg["nof_rb"], 1
    d = cfg["freq_density"]
    if d in (DOT5_EVEN, DOT5_ODD):
        stride = 2
        parity = 0 if d == DOT5_EVEN else 1
        if perturb == "comb_parity":
            parity ^= 1
        if begin % 2 != parity:
            begin += 1
    return np.arange(begin, end, stride, dtype=np.int64)


def seq_len(cfg):
    """Sequence elements per symbol (get_seq_len), with the rounding of an odd nof_rb at density 0.5."""
    n, d = cfg["nof_rb"], cfg["freq_density"]
    if d in (DOT5_EVEN, DOT5_ODD):
        n = cfg["nof_rb"] // 2
        if cfg["nof_rb"] % 2 and (cfg["start_rb"] % 2 == (1 if d == DOT5_ODD else 0)):
            n += 1
    elif d == THREE:
        n *= 3
    return 2 * n if cfg["cdm"] != NO_CDM else n


def skipped_elements(cfg):
    d, s = cfg["freq_density"], cfg["start_rb"]
    first = {ONE: s, THREE: s, DOT5_EVEN: s + s % 2, DOT5_ODD: s + (1 - s % 2)}[d]
    if d == THREE:
        return 3 * first
    if d == ONE:
        return first if cfg["row"] == 2 else 2 * first
    return first // 2 if cfg["row"] == 2 else first


def c_init(cfg, symbol):
    n_id = cfg["scrambling_id"]
    return ((1 << 10) * (nof_symbols(cfg) * cfg["n_slot"] + symbol + 1) * (2 * n_id + 1) + n_id) % (1 << 31)


def groups(cfg):
    """(symbol, first subcarrier of the RB) of each CDM group."""
    row, k, l = cfg["row"], cfg["k_ref"], cfg["symbol_l0"]
    if row == 4:
        return [(l, k), (l, k + 2)]
    if row == 5:
        return [(l, k), (l + 1, k)]
    return [(l, k)]


def to_bf16(v):
    u = np.asarray(v, F).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)


def process(cfg, perturb=None):
    """The written grid words as (port, symbol, subcarrier, word) rows sorted by port, symbol, subcarrier."""
    ports = ROW_PORTS[cfg["row"]]
    size = 2 if cfg["cdm"] == FD_CDM2 else 1
    w = np.asarray(cfg["weights"], np.complex64)
    rbs = rb_comb(cfg, perturb)
    n = seq_len(cfg)
    if cfg["row"] == 1:
        in_rb = np.array([0, 4, 8])
    else:
        in_rb = np.arange(size)
    if perturb == "comb_parity":
        n = rbs.size * in_rb.size
    assert n == rbs.size * in_rb.size, cfg
    amp = F(np.sqrt(0.5) * np.float64(F(cfg["amplitude"])))
    skip = skipped_elements(cfg)
    first_bit = skip if perturb == "skip_not_doubled" else 2 * skip
    bypass = ports == 1 and w[0, 0] == 1
    rows = []
    for g, (symbol, k_bar) in enumerate(groups(cfg)):
        seq = gold_sequence(c_init(cfg, symbol), first_bit + 2 * n)[first_bit:]
        re = np.where(seq[0::2] == 1, -amp, amp).astype(F)
        im = np.where(seq[1::2] == 1, -amp, amp).astype(F)
        sc = (12 * rbs[:, None] + k_bar + in_rb[None, :]).ravel()
        layers = [(re, im)]
        if size == 2:
            s = np.where(np.arange(n) % 2 == 1, F(-1), F(1)).astype(F)
            if perturb == "no_w_f":
                s = np.ones(n, F)
            layers.append(((s * re).astype(F), (s * im).astype(F)))
        for p in range(ports):
            if bypass:
                sr, si = re, im
            else:
                sr = si = None
                for q, (a, b) in enumerate(layers):
                    c = w[p, size * g + q]
                    wr, wi = F(c.real), F(c.imag)
                    tr = ((a * wr).astype(F) - (b * wi).astype(F)).astype(F)
                    ti = ((a * wi).astype(F) + (b * wr).astype(F)).astype(F)
                    sr, si = (tr, ti) if sr is None else ((sr + tr).astype(F), (si + ti).astype(F))
            word = to_bf16(sr) | (to_bf16(si) << 16)
            rows.append(np.stack([np.full(n, p), np.full(n, symbol), sc, word], axis=1))
    rows = np.concatenate(rows).astype(np.int64).reshape(-1, 4)
    return rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]


def apply_rows(grid_words, rows):
    """Writes (port, symbol, subcarrier, word) rows into a (ports, 14, nsc) uint32 grid."""
    grid_words[rows[:, 0], rows[:, 1], rows[:, 2]] = rows[:, 3].astype(np.uint32)


def reserved_patterns(cfg):
    """The signal's REs as (rb_begin, rb_end, rb_stride, re_mask, symbol_mask) per CDM group: what a PDSCH reserves."""
    rbs = rb_comb(cfg)
    in_rb = (0, 4, 8) if cfg["row"] == 1 else range(2 if cfg["cdm"] == FD_CDM2 else 1)
    stride = 2 if cfg["freq_density"] in (DOT5_EVEN, DOT5_ODD) else 1
    return [(int(rbs[0]), int(rbs[-1]) + 1, stride, sum(1 << (k_bar + j) for j in in_rb), 1 << symbol)
            for symbol, k_bar in groups(cfg)] if rbs.size else []


def expected_grid(cfg, grid_nof_prb=None, grid_nof_ports=None):
    want = np.full((grid_nof_ports or cfg["grid_nof_ports"], 14, 12 * (grid_nof_prb or cfg["grid_nof_prb"])), SENTINEL,
                   np.uint32)
    apply_rows(want, process(cfg))
    return want


# ---- cases -------------------------------------------------------------------------------------------------------

def random_weights(rng, ports):
    return ((rng.normal(size=(ports, ports)) + 1j * rng.normal(size=(ports, ports))) / 2).astype(np.complex64)


def make_case(rng, row, density, start_rb, nof_rb, k_ref=None, l0=None, cp=0, weights=None, grid_nof_prb=52,
              grid_nof_ports=4, amplitude=None, grid_index=0):
    k_refs, _, cdm = ROW_RULES[row]
    ports = ROW_PORTS[row]
    numerology = 2 if cp else int(rng.integers(0, 3))
    last = (12 if cp else 14) - (2 if row == 5 else 1)
    return dict(numerology=numerology, n_slot=int(rng.integers(0, 10 << numerology)), cp=cp, start_rb=start_rb,
                nof_rb=nof_rb, row=row, k_ref=int(rng.choice(list(k_refs))) if k_ref is None else k_ref,
                symbol_l0=int(rng.integers(0, last + 1)) if l0 is None else l0, symbol_l1=int(rng.integers(2, 13)),
                cdm=cdm, freq_density=density, scrambling_id=int(rng.integers(0, 1024)),
                amplitude=F(rng.choice([1.0, 0.5, 1.4125375, 2.0])) if amplitude is None else F(amplitude),
                weights=np.eye(ports, dtype=np.complex64) if weights is None else weights, grid_nof_prb=grid_nof_prb,
                grid_nof_ports=grid_nof_ports, grid_index=grid_index)


def golden_generator_cases(rng):
    """The fixture's cases: every (row, density) of rows 1-5, the k_ref and l0 extremes, the start_rb x nof_rb parities
    at both 0.5 densities (with single RBs of either parity: sequence lengths 0 and 1), identity and full complex
    precoding, one port with a weight that is not 1, both cyclic prefixes."""
    cases = []
    for row, (k_refs, densities, _) in ROW_RULES.items():
        ports = ROW_PORTS[row]
        for density in densities:
            for k_ref in (k_refs[0], k_refs[-1], None):
                cases.append(make_case(rng, row, density, int(rng.integers(0, 20)), int(rng.integers(4, 30)), k_ref))
            cases.append(make_case(rng, row, density, 3, 24, weights=random_weights(rng, ports)))
            cases.append(make_case(rng, row, density, 0, 52, l0=0, cp=1))
            cases.append(make_case(rng, row, density, 40, 12, l0=10 if row == 5 else 11, cp=1,
                                   weights=random_weights(rng, ports)))
        cases.append(make_case(rng, row, densities[0], 0, 52, l0=12 if row == 5 else 13))
        cases.append(make_case(rng, row, densities[0], 7, 9, l0=0, grid_nof_ports=ports))
    for row in (2, 3):
        for density in (DOT5_EVEN, DOT5_ODD):
            for start_rb in (4, 5):
                for nof_rb in (1, 6, 7):
                    cases.append(make_case(rng, row, density, start_rb, nof_rb,
                                           weights=random_weights(rng, ROW_PORTS[row]) if nof_rb == 7 else None))
    cases.append(make_case(rng, 2, ONE, 10, 20, weights=np.array([[0.5 - 0.25j]], np.complex64)))
    cases.append(make_case(rng, 1, THREE, 0, 273, grid_nof_prb=273, grid_nof_ports=1))
    cases.append(make_case(rng, 4, ONE, 200, 73, grid_nof_prb=273, weights=random_weights(rng, 4)))
    return cases


def golden_cases():
    """(cfg, written rows) of every fixture case."""
    z = np.load(GOLDEN)
    pos, wpos = 0, 0
    rows = np.stack([z["w_port"], z["w_symbol"], z["w_subcarrier"], z["w_word"]], axis=1).astype(np.int64)
    for i in range(z["cfg"].shape[0]):
        cfg = {k: int(v) for k, v in zip(CFG_INT_KEYS, z["cfg"][i])}
        ports = ROW_PORTS[cfg["row"]]
        cfg["amplitude"] = F(z["amplitude"][i])
        cfg["weights"] = z["weights"][wpos: wpos + ports * ports].reshape(ports, ports).copy()
        wpos += ports * ports
        n = int(z["nof_written"][i])
        yield cfg, rows[pos: pos + n]
        pos += n
    assert pos == rows.shape[0] and wpos == z["weights"].size


def random_plan_cases(rng, nof_grids=3, grid_nof_prb=52):
    """Signals of all rows over several grids, each on symbols and subcarriers of its own in its grid."""
    cases = []
    for g in range(nof_grids):
        pair = int(rng.integers(0, 13))  # row 5 takes two symbols
        symbols = [int(s) for s in rng.permutation(14) if s not in (pair, pair + 1)]
        for row in (5, 1, 1, 2, 2, 3, 3, 4):
            densities = ROW_RULES[row][1]
            l0 = pair if row == 5 else symbols.pop()
            start = int(rng.integers(0, grid_nof_prb - 1))
            nof = int(rng.integers(1, grid_nof_prb - start + 1))
            ports = ROW_PORTS[row]
            cases.append(make_case(rng, row, int(rng.choice(densities)), start, nof, l0=l0,
                                   weights=random_weights(rng, ports) if rng.integers(0, 2) else None,
                                   grid_nof_prb=grid_nof_prb, grid_index=g))
    return cases


def bench_cases(rng, nof_slots=32, grid_nof_prb=273):
    """Per slot a TRS-like set (row 1 on symbols 4 and 8) and one row-4 CSI-RS (symbol 13) over the whole grid."""
    cases = []
    for g in range(nof_slots):
        for row, l0 in ((1, 4), (1, 8), (4, 13)):
            cases.append(make_case(rng, row, ROW_RULES[row][1][0], 0, grid_nof_prb, l0=l0, grid_nof_prb=grid_nof_prb,
                                   grid_index=g))
    return cases
