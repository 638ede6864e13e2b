"""The PRACH detector restated in float64, the quantities it derives from the format, and the case generators of the
fixture tests/golden/prach_detector.npz (made by tools/gen_prach_golden.py from the reference's own detector) and of the
GPU tests.

Reference (behaviour, not code): lib/phy/upper/channel_processors/prach_detector_generic_impl.cpp:80 (detect),
lib/ran/prach/prach_preamble_information.cpp:30 / :46 (format rows, TS 38.211 Tables 6.3.3.1-1 / -2),
prach_generator_impl.cpp:97 (y_u, here the L-point DFT of x_u(i) = exp(-j pi u i (i + 1) / L)).

A case is a dict: the PDU fields (format and ra_scs as indices into FORMATS and SCS_HZ, zcz, rsi, nof_ports, start, nof,
combine), the values the reference derived from them (n_cs, roots, threshold, margin), and `words`, the samples as
uint32 (re | im << 16, bf16) of shape (ports, symbols, L)."""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "prach_detector.npz")
NAN_WORD = 0x7FC07FC0   # bf16 NaN in both halves
FORMATS = ("0", "1", "2", "3", "A1", "A2", "A3", "B1", "B4", "C0", "C2", "A1/B1", "A2/B2", "A3/B3")
SCS_HZ = (15000.0, 30000.0, 60000.0, 120000.0, 1250.0, 5000.0)
SCS_1_25, SCS_5 = 4, 5
T_C = 1.0 / (480000.0 * 4096.0)
LONG_ROWS = {0: (1, 3168, SCS_1_25), 1: (2, 21024, SCS_1_25), 2: (4, 4688, SCS_1_25), 3: (4, 3168, SCS_5)}
SHORT_ROWS = {4: (2, 288), 5: (4, 576), 6: (6, 864), 7: (2, 216), 8: (12, 936), 9: (1, 1240), 10: (4, 2048), 11: (2, 288),
              12: (4, 576), 13: (6, 864)}
PERTURBATIONS = ("window_off_by_one", "reference_no_wrap", "den_no_abs", "norm_by_n", "halves_swapped", "no_08")
CFG_KEYS = ("format", "ra_scs", "zcz", "rsi", "nof_ports", "start", "nof", "combine", "n_cs", "margin", "nof_roots")
# Ten times the largest relative deviation of the reference's metrics, RSSI and times from this restatement over the
# fixture (tests/test_prach_oracle.py measures it: MEASURED_DEVIATION), floored at 1e-4.
MEASURED_DEVIATION = 1.902e-4
DELTA = max(10 * MEASURED_DEVIATION, 1e-4)
# The kernel divides exactly, as this restatement does, so against the restatement only float32 rounding stands between
# the two: the longest sums have 1024 terms (the transform, the reference energy), and 1024 x 2^-24 = 6.1e-5 bounds
# their relative error linearly. 1e-4, the floor DELTA has, covers it. Every monitored preamble of the fixture is
# decidable at KERNEL_DELTA (tests/test_prach_oracle.py), so `detected` and `delay_samples` of the kernel must equal
# the restatement's on all of them.
KERNEL_DELTA = 1e-4
GUARD_WORDS = 64
ROOT_TOLERANCE = {839: 2e-4, 139: 7e-5}  # ten times the deviation of the reference's generator from a float64 DFT


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


def awgn(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


def on_tc_grid(seconds):
    """phy_time_unit::from_seconds(...).to_seconds(): the time rounded to a multiple of T_c, as the reference reports
    its times (phy_time_unit.h:262)."""
    tenths = int(seconds / T_C * 10)
    return (tenths // 10 + (tenths % 10) // 5) * T_C


def rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-300)


# ---- derived quantities ------------------------------------------------------------------------------------------

def derive(fmt, ra_scs, n_cs):
    """What detect() computes with before it touches a sample (:104-160); None for an undefined format / SCS pair."""
    if fmt in LONG_ROWS:
        nof_symbols, cp_kappa, scs = LONG_ROWS[fmt]
        if ra_scs != scs:
            return None
        L, N = 839, 1024
    elif fmt in SHORT_ROWS and 0 <= ra_scs <= 3:
        nof_symbols, cp_kappa = SHORT_ROWS[fmt]
        cp_kappa >>= ra_scs
        L, N = 139, 256
    else:
        return None
    scs_hz = SCS_HZ[ra_scs]
    nof_shifts, nof_sequences = 1, 64
    if n_cs > L:
        return None
    if n_cs != 0:
        nof_shifts = min(64, L // n_cs)
        nof_sequences = -(-64 // nof_shifts)
    cp_prach = int(np.floor(float(cp_kappa * 64) * T_C * L * scs_hz))
    win_width = (cp_prach if n_cs == 0 else min(n_cs, cp_prach)) * N // L
    max_delay = cp_prach if n_cs == 0 else min(max(n_cs, 1) - 1, cp_prach)
    max_delay = max_delay * N // L
    return dict(L=L, N=N, nof_symbols=nof_symbols, scs_hz=scs_hz, cp_kappa=cp_kappa, cp_prach=cp_prach, nof_shifts=nof_shifts,
                nof_sequences=nof_sequences, win_width=win_width, max_delay=max_delay,
                delay_end=int(np.ceil(float(np.float32(max_delay)) * 0.8)), sample_rate=N * scs_hz)


def window_start(d, n_cs, w):
    return (d["N"] - (n_cs * w * d["N"]) // d["L"]) % d["N"]


@functools.lru_cache(maxsize=None)
def root_sequence(L, u):
    """y_u: the L-point DFT of x_u(i) = exp(-j pi u i (i + 1) / L), the phase reduced modulo 2 L as an integer."""
    i = np.arange(L, dtype=np.int64)
    phase = (u * ((i * (i + 1)) % (2 * L))) % (2 * L)
    return np.fft.fft(np.exp(-1j * np.pi * phase / L))


def find_root(L, y):
    """The u whose restated sequence is nearest to y, and the distance."""
    best = min(range(1, L), key=lambda u: np.abs(root_sequence(L, u) - y).max())
    return best, float(np.abs(root_sequence(L, best) - y).max())


# ---- the detector ------------------------------------------------------------------------------------------------

def is_normal(v):
    a = np.abs(v)
    return np.isfinite(v) & (a >= 1.1754943508222875e-38)


def detect(cfg, x, perturb=()):
    """detect() in float64 on x (ports, symbols, L). -> dict(rssi, early, preambles: {index: dict(peak, delay, detected,
    metric, other)}) over the monitored preambles; `other` is the largest other sample of the preamble's window."""
    d = derive(cfg["format"], cfg["ra_scs"], cfg["n_cs"])
    L, N, S, P, n_cs = d["L"], d["N"], d["nof_symbols"], cfg["nof_ports"], cfg["n_cs"]
    ww, margin, ns = d["win_width"], cfg["margin"], d["nof_shifts"]
    x = np.asarray(x)[:P, :S]
    rssi = float((np.abs(x) ** 2).sum() / L / (P * S * L))
    out = dict(rssi=rssi, early=not bool(is_normal(np.float32(rssi))), preambles={}, derived=d)
    if out["early"]:
        return out
    first, end = cfg["start"], cfg["start"] + cfg["nof"]
    half = L // 2
    for seq in range(d["nof_sequences"]):
        lo, hi = seq * ns, min(64, (seq + 1) * ns)
        if hi <= first or lo >= end:
            continue
        y = root_sequence(L, int(cfg["roots"][seq]))
        num, den = np.zeros((ns, ww)), np.zeros((ns, ww))
        for p in range(P):
            for rnd in range(1 if cfg["combine"] else S):
                c = x[p].sum(0) if cfg["combine"] else x[p, rnd]
                nr = c * np.conj(y)
                inp = np.zeros(N, complex)
                if "halves_swapped" in perturb:
                    inp[:half + 1], inp[N - half:] = nr[:half + 1], nr[half + 1:]
                else:
                    inp[:half + 1], inp[N - half:] = nr[L - half - 1:], nr[:half]
                mod = np.abs(np.fft.ifft(inp) * N) ** 2 / (N if "norm_by_n" in perturb else N * L * L)
                for w in range(ns):
                    start = window_start(d, n_cs, w)
                    if "window_off_by_one" in perturb:
                        start = (start + 1) % N
                    i0 = (start + N - margin) % N
                    i1 = i0 + 2 * margin + ww
                    ref = mod[i0:min(i1, N)].sum()
                    if i1 > N and "reference_no_wrap" not in perturb:
                        ref += mod[:i1 - N].sum()
                    v = mod[(start + np.arange(ww)) % N] * (N / L)
                    diff = ref - v
                    diff[~is_normal(diff)] = 1e-9
                    num[w] += v
                    den[w] += diff
        for w in range(ns):
            k = lo + w
            if k >= 64 or not first <= k < end:
                continue
            m = num[w] / (den[w] if "den_no_abs" in perturb else np.abs(den[w]))
            delay = int(np.argmax(m))
            peak = float(m[delay])
            limit = float(d["max_delay"]) if "no_08" in perturb else float(np.float32(d["max_delay"])) * 0.8
            others = np.delete(m, delay)
            out["preambles"][k] = dict(peak=peak, delay=delay, detected=bool(peak > cfg["threshold"] and delay < limit),
                                       metric=peak / cfg["threshold"], other=float(others.max()) if others.size else 0.0)
    return out


def decidable(r, threshold, delta=None):
    """A monitored preamble whose decision and delay rounding within delta cannot turn."""
    delta = DELTA if delta is None else delta
    return abs(r["peak"] - threshold) > delta * threshold and r["other"] < r["peak"] * (1 - delta)


# ---- transmitters and case generators ------------------------------------------------------------------------------

def transmit(cfg, sent, rng, noise=1.0, dead_ports=(), scale=1.0):
    """The occasion's samples (ports, symbols, L) as bf16 words: for every (preamble index, delay in IDFT samples, target)
    of `sent` the preamble through one random unit-modulus gain per port, at the amplitude that brings its detection
    metric near `target` in unit-variance noise, plus `noise` x AWGN; dead ports are zero; all of it times `scale`."""
    d = derive(cfg["format"], cfg["ra_scs"], cfg["n_cs"])
    L, N, S, P = d["L"], d["N"], d["nof_symbols"], cfg["nof_ports"]
    x = noise * awgn(rng, (P, S, L))
    n = np.arange(L)
    length = 2 * cfg["margin"] + d["win_width"]
    for k, delay, target in sent:
        seq, v = divmod(k, d["nof_shifts"])
        y = root_sequence(L, int(cfg["roots"][seq])) / np.sqrt(L)
        y = y * np.exp(2j * np.pi * (v * cfg["n_cs"]) * n / L) * np.exp(-2j * np.pi * (n - L // 2) * delay / N)
        power = target * cfg["threshold"] * length / (N * (S if cfg["combine"] else 1))
        for p in range(P):
            x[p] += np.sqrt(power) * np.exp(2j * np.pi * rng.random()) * y
    for p in dead_ports:
        x[p] = 0
    return to_bf16_words(scale * x)


def pdu(fmt, ra_scs, zcz, rsi, nof_ports, start=0, nof=64, combine=1):
    return dict(format=FORMATS.index(fmt), ra_scs=ra_scs, zcz=zcz, rsi=rsi, nof_ports=nof_ports, start=start, nof=nof,
                combine=combine)


# (name, PDU, recipe): sent = [(preamble, delay as a fraction of max_delay, target)], plus noise / dead_ports / zero.
GOLDEN_RECIPES = (
    ("f0_ncs0_roots", pdu("0", SCS_1_25, 0, 22, 1), dict(sent=[(3, 0.3, 6.0), (40, 0.6, 8.0)])),
    ("f0_ncs13", pdu("0", SCS_1_25, 1, 700, 2), dict(sent=[(10, 0.5, 6.0), (11, 0.2, 6.0), (63, 0.7, 5.0)])),
    ("f0_ncs46_last_root", pdu("0", SCS_1_25, 8, 836, 1), dict(sent=[(17, 0.4, 6.0), (60, 0.1, 7.0)])),
    ("f0_range_inside_root", pdu("0", SCS_1_25, 8, 5, 2, start=5, nof=20), dict(sent=[(5, 0.5, 6.0), (24, 0.3, 6.0), (30, 0.3, 9.0)])),
    ("f0_delay_sides", pdu("0", SCS_1_25, 12, 100, 1), dict(sent=[(0, 0.75, 7.0), (1, 0.85, 7.0), (2, 0.0, 7.0)])),
    ("f0_noise_free", pdu("0", SCS_1_25, 12, 100, 1, nof=4), dict(sent=[(0, 0.25, 8.0)], noise=0.0)),
    ("f3_4symbols", pdu("3", SCS_5, 6, 400, 2), dict(sent=[(7, 0.4, 6.0), (50, 0.6, 0.4)])),
    ("b4_12symbols", pdu("B4", 1, 0, 10, 4), dict(sent=[(0, 0.5, 6.0), (63, 0.2, 6.0)])),
    ("b4_capped", pdu("B4", 1, 1, 130, 2), dict(sent=[(20, 0.0, 6.0), (21, 0.0, 6.0)])),
    ("a1", pdu("A1", 1, 11, 50, 1), dict(sent=[(4, 0.4, 6.0), (5, 0.9, 6.0), (33, 0.5, 0.5)])),
    ("c0", pdu("C0", 0, 13, 3, 2), dict(sent=[(1, 0.3, 6.0)])),
    ("c2", pdu("C2", 1, 14, 137, 4), dict(sent=[(2, 0.5, 6.0), (3, 0.95, 6.0)])),
    ("a2_noise", pdu("A2", 1, 9, 77, 2), dict(sent=[])),
    ("f0_noise", pdu("0", SCS_1_25, 1, 0, 1), dict(sent=[])),
    ("b4_zero", pdu("B4", 1, 11, 9, 2), dict(sent=[], zero=True)),
    ("b4_dead_port", pdu("B4", 1, 11, 9, 4), dict(sent=[(6, 0.4, 6.0)], dead_ports=(2,))),
    # So faint that the 1e-9 a dead port adds to the denominator counts: the one place where the normalisation shows.
    ("b4_dead_port_faint", pdu("B4", 1, 11, 9, 4), dict(sent=[(6, 0.4, 6.0)], dead_ports=(2,), scale=1e-4)),
    ("b4_no_combine", pdu("B4", 1, 11, 9, 2, combine=0), dict(sent=[(6, 0.4, 6.0), (40, 0.1, 6.0)])),
    ("f3_no_combine", pdu("3", SCS_5, 6, 400, 1, combine=0), dict(sent=[(7, 0.4, 6.0)])),
)
ROOT_SAMPLES = ((839, "f0_ncs0_roots", 0), (839, "f0_ncs0_roots", 63), (839, "f3_4symbols", 1), (139, "b4_12symbols", 0),
                (139, "b4_12symbols", 37), (139, "c2", 0))


def make_words(cfg, recipe, rng):
    d = derive(cfg["format"], cfg["ra_scs"], cfg["n_cs"])
    sent = [(k, round(f * d["max_delay"]), t) for k, f, t in recipe.get("sent", ())]
    words = transmit(cfg, sent, rng, recipe.get("noise", 1.0), recipe.get("dead_ports", ()), recipe.get("scale", 1.0))
    if recipe.get("zero"):
        words = np.zeros_like(words)
    return words, [(k, dl) for k, dl, _ in sent]


def random_occasion(rng, long_format=False):
    """A fresh occasion with random valid roots rather than table roots, and made-up but valid thresholds and margins."""
    while True:
        if long_format:
            fmt, ra_scs = (0, SCS_1_25) if rng.random() < 0.5 else (3, SCS_5)
            n_cs = int(rng.choice([0, 13, 26, 59, 119]))
        else:
            fmt, ra_scs = int(rng.choice([4, 7, 8, 9, 10, 12])), int(rng.integers(0, 3))
            n_cs = int(rng.choice([0, 2, 8, 13, 23, 46, 69]))
        d = derive(fmt, ra_scs, n_cs)
        margin = min(int(rng.integers(2, 12)), (d["N"] - d["win_width"]) // 2)
        if margin >= 1:  # (C2 with N_cs = 0 has a window as long as the IDFT)
            break
    start = int(rng.integers(0, 60))
    cfg = dict(format=fmt, ra_scs=ra_scs, zcz=-1, rsi=-1, nof_ports=int(rng.choice([1, 2, 3, 4])), start=start,
               nof=int(rng.integers(1, 64 - start + 1)), combine=int(rng.random() < 0.7), n_cs=n_cs, margin=margin,
               threshold=float(np.float32(rng.uniform(0.2, 2.0))),
               roots=[int(u) for u in rng.choice(np.arange(1, d["L"]), d["nof_sequences"], replace=False)])
    sent = [(int(rng.integers(cfg["start"], cfg["start"] + cfg["nof"])), int(rng.integers(0, max(d["max_delay"], 1))),
             float(rng.uniform(3.0, 9.0))) for _ in range(int(rng.integers(0, 3)))]
    cfg["words"] = transmit(cfg, sent, rng)
    return cfg


# ---- the fixture ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden():
    """-> (cases, root samples): every case with its cfg keys, words, and the reference's rssi (linear),
    time_resolution, time_advance_max, indications [(index, time advance, metric)] and sent [(index, delay)]."""
    g = np.load(GOLDEN)
    cases, at_root, at_word, at_ind, at_sent = [], 0, 0, 0, 0
    for i, name in enumerate(g["names"]):
        c = dict(zip(CFG_KEYS, (int(v) for v in g["cfg"][i])), name=str(name), threshold=float(g["threshold"][i]))
        d = derive(c["format"], c["ra_scs"], c["n_cs"])
        c["roots"] = [int(u) for u in g["roots"][at_root:at_root + c["nof_roots"]]]
        at_root += c["nof_roots"]
        size = c["nof_ports"] * d["nof_symbols"] * d["L"]
        c["words"] = g["words"][at_word:at_word + size].reshape(c["nof_ports"], d["nof_symbols"], d["L"])
        at_word += size
        c["rssi_dB"] = float(g["rssi_dB"][i])
        c["rssi"] = 0.0 if np.isneginf(g["rssi_dB"][i]) else float(10.0 ** (float(g["rssi_dB"][i]) / 10.0))
        c["time_resolution"], c["time_advance_max"] = float(g["time_resolution"][i]), float(g["time_advance_max"][i])
        n = int(g["nof_indications"][i])
        c["indications"] = [(int(g["ind_index"][at_ind + j]), float(g["ind_time_advance"][at_ind + j]),
                             float(g["ind_metric"][at_ind + j])) for j in range(n)]
        at_ind += n
        n = int(g["nof_sent"][i])
        c["sent"] = [(int(a), int(b)) for a, b in g["sent"][at_sent:at_sent + n]]
        at_sent += n
        cases.append(c)
    roots = [(int(L), int(u), y) for (L, u), y in zip(g["root_lu"], np.split(g["root_values"], np.cumsum(g["root_lu"][:, 0])[:-1]))]
    return cases, roots


@functools.lru_cache(maxsize=None)
def restate_golden():
    return [detect(c, words_to_complex(c["words"])) for c in golden()[0]]


def measured_deviation(restated=None):
    """The largest relative deviation of the reference's metrics, RSSI and times from the restatement over the fixture."""
    worst = 0.0
    for c, r in zip(golden()[0], restated or restate_golden()):
        d = r["derived"]
        worst = max(worst, rel(r["rssi"], c["rssi"]) if c["rssi"] > 0 else abs(r["rssi"]))
        worst = max(worst, rel(on_tc_grid(1.0 / d["sample_rate"]), c["time_resolution"]),
                    rel(on_tc_grid(0.8 * d["max_delay"] / d["sample_rate"]), c["time_advance_max"]) if d["max_delay"] else 0.0)
        for k, _, metric in c["indications"]:
            if k in r["preambles"]:
                worst = max(worst, rel(r["preambles"][k]["metric"], metric))
    return worst


# ---- what the GPU tests and tools/prach_bench.py share -----------------------------------------------------------------

def place(cases, seed=0):
    """The cases' samples in one input with odd offsets and strides, NaN everywhere else -> (words, [PrachOccasion])."""
    import srsgpu
    rng = np.random.default_rng(seed)
    chunks, occasions, at = [np.full(GUARD_WORDS, NAN_WORD, np.uint32)], [], GUARD_WORDS
    for c in cases:
        d = derive(c["format"], c["ra_scs"], c["n_cs"])
        L, S, P = d["L"], d["nof_symbols"], c["nof_ports"]
        symbol_stride = L + int(rng.integers(0, 4))
        port_stride = S * symbol_stride + 2 * int(rng.integers(0, 3)) + 1
        lead = int(rng.integers(0, 3))
        block = np.full(lead + P * port_stride, NAN_WORD, np.uint32)
        for p in range(P):
            for s in range(S):
                start = lead + p * port_stride + s * symbol_stride
                block[start:start + L] = c["words"][p, s]
        occasions.append(srsgpu.PrachOccasion(
            format=c["format"], ra_scs=c["ra_scs"], nof_rx_ports=P, n_cs=c["n_cs"], roots=c["roots"], threshold=c["threshold"],
            win_margin=c["margin"], sample_offset=at + lead, port_stride=port_stride, symbol_stride=symbol_stride,
            start_preamble_index=c["start"], nof_preamble_indices=c["nof"], combine_symbols=c["combine"]))
        chunks.append(block)
        at += block.size
    chunks.append(np.full(GUARD_WORDS, NAN_WORD, np.uint32))
    return np.concatenate(chunks), occasions


def new_deviation():
    return dict(rssi=0.0, peak=0.0, metric=0.0)


def compare(got, c, r, dev, reference=True, fresh_draw=False):
    """One occasion's PRACH_RESULT_DTYPE record against the restatement r and, for a fixture case, the reference.
    `detected` and `delay_samples` equal the restatement's on EVERY monitored preamble (each must be decidable at
    KERNEL_DELTA, or the comparison would hang on float32 rounding; with fresh_draw, a tool's draw that is not only has
    its decision checked against its own peak and delay) and the reference's on those decidable at DELTA.
    -> the number of monitored preambles undecidable at DELTA."""
    d, name = r["derived"], c.get("name")
    undecided = 0
    if r["early"]:
        assert got["early_stop"] == 1 and not np.asarray(got["preambles"]).view(np.uint8).any(), name
        assert got["rssi"] == np.float32(r["rssi"]) == 0, name
        return 0
    assert got["early_stop"] == 0
    dev["rssi"] = max(dev["rssi"], rel(got["rssi"], r["rssi"]))
    assert rel(got["rssi"], r["rssi"]) <= DELTA
    found = {k: (ta, m) for k, ta, m in c["indications"]} if reference else {}
    if reference:
        assert rel(got["rssi"], c["rssi"]) <= DELTA
    for k in range(64):
        p, want = got["preambles"][k], r["preambles"].get(k)
        if want is None:
            assert p["detected"] == 0 and p["delay_samples"] == 0 and p["metric"] == 0 and p["peak"] == 0, (name, k)
            continue
        dev["peak"] = max(dev["peak"], rel(p["peak"], want["peak"]))
        assert rel(p["peak"], want["peak"]) <= DELTA, (name, k, p, want)
        assert rel(p["metric"], want["metric"]) <= DELTA, (name, k, p, want)
        if decidable(want, c["threshold"], KERNEL_DELTA):
            assert (bool(p["detected"]), int(p["delay_samples"])) == (want["detected"], want["delay"]), (name, k, p, want)
        else:
            # Only a tool's fresh draw may come here; the tests' cases are all decidable at KERNEL_DELTA.
            assert fresh_draw, (name, k, "the case itself hangs on float32 rounding")
            follows = bool(p["peak"] > np.float32(c["threshold"]) and p["delay_samples"] < d["delay_end"])
            assert bool(p["detected"]) == follows, (name, k, p)
        sure = decidable(want, c["threshold"])
        undecided += not sure
        if reference and sure:
            assert bool(p["detected"]) == (k in found), (name, k)
        if k in found:
            dev["metric"] = max(dev["metric"], rel(p["metric"], found[k][1]))
            assert rel(p["metric"], found[k][1]) <= DELTA, (name, k)
            if sure:
                assert int(p["delay_samples"]) == int(round(found[k][0] * d["sample_rate"])), (name, k)
    return undecided
