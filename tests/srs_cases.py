"""SRS estimator test infrastructure: a float64 numpy restatement of the reference's estimator, a transmitter with a
flat channel per port pair and a delay (which the reference, being a gNB, does not have), seeded case generators, the
grid placement with a fill word and the tolerances.

  per-port information   lib/ran/srs/srs_information.cpp:38 (cyclic shift, k_TC, k0, u = n_ID mod 30, v = 0, L)
  estimator              lib/phy/upper/signal_processors/srs/srs_estimator_generic_impl.cpp:79 (LSE, EPRE :169-172, time
                         alignment :199-209, phase compensation :56-77 / :222-229, coefficients :232, noise :237-267)
  time alignment         lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.cpp:226 (IDFT size),
                         :245 (search range, peak, refinement :51)
  sequences              lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.cpp:243

The restatement computes in float64 except where the reference's float32 decides an integer: the phase table index
int(round(1024 (n ps + po) / 2 pi)) is evaluated in float32, operation by operation, with ps and po cast as the reference
casts them, because an index off by one is a 2 pi / 1024 phase error on that RE. The doubles that decide max_ta_samples
are evaluated in the reference's order.

Tolerances (tolerances()): each is ten times the largest deviation of the reference's recorded results from this
restatement over the fixture, floored at 1e-4 (MEASURED, held to the fixture by tests/test_srs_oracle.py); "kernel" is
the kernel's own deviation from the reference on the fixture, measured on an MI355X (tests/test_srs_estimator_gpu.py):
  channel matrix   |H - H'|_F / |H'|_F                      reference 6.7e-7 -> 1e-4   kernel 6.5e-7
  EPRE             relative                                  reference 4.2e-7 -> 1e-4   kernel 4.1e-7
  noise variance   relative to max(nv, 1e-6 EPRE)            reference 5.5e-7 -> 1e-4   kernel 5.7e-7
  time alignment   in units of 1 / fs, on equal ta_idx       reference 6.6e-7 -> 1e-4   kernel 6.3e-7
Below 1e-6 EPRE the noise variance is what float rounding leaves when the rebuilt signal equals the received one.

TEST INFRASTRUCTURE ONLY."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
from low_papr_tables import PHI  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "srs_estimator.npz")
NAN_WORD = 0x7FC07FC0   # bf16 NaN in both halves: grid prefill of the GPU tests
HUGE_WORD = 0x714A714A  # bf16 1e30 in both halves
T_C = 1.0 / (480000.0 * 4096.0)
TWOPI32 = np.float32(2.0) * np.float32(np.pi)
CEXP_SIZE = 1024
CFG_KEYS = ("c_srs", "numerology", "nof_antenna_ports", "nof_symbols", "start_symbol", "comb_size", "comb_offset",
            "cyclic_shift", "sequence_id", "bandwidth_index", "freq_position", "freq_shift", "nof_rx_ports", "rx0", "rx1",
            "rx2", "rx3", "grid_nof_ports")
PERTURBATIONS = ("cs_port0", "ktc_fixed", "noise_div_nap", "no_symbol_mean", "slope_sign", "rx_order")

# The largest deviations of the reference's results from the restatement over the fixture (tests/test_srs_oracle.py).
MEASURED = dict(channel=6.73e-7, epre=4.18e-7, noise_var=5.50e-7, time_alignment=6.57e-7)
NOISE_FLOOR = 1e-6  # of the EPRE
# Against the restatement only float32 rounding moves the kernel's correlation: the transform sums at most 2048 terms, so
# an amplitude is off by at most 2048 x 2^-24 = 1.2e-4 of the largest one, a power by twice that, and two taps are
# compared: 4.9e-4. A resource whose winning tap leads every other searched tap by more than this is decidable.
KERNEL_DELTA = 5e-4


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


def awgn(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


# ---- derived quantities and sequences --------------------------------------------------------------------------

def derive(c, perturb=()):
    """What estimate() computes with before it touches a sample. c["row"]: ((m_srs, N) x 4) of the C_SRS row."""
    comb, nap, cs = c["comb_size"], c["nof_antenna_ports"], c["cyclic_shift"]
    row = c["row"]
    n_cs_max = 12 if comb == 4 else 8
    L = row[c["bandwidth_index"]][0] * 12 // comb
    interleaved = nap == 4 and cs >= n_cs_max // 2
    total = 0
    for b in range(c["bandwidth_index"] + 1):
        m_srs, n = row[b]
        total += comb * (m_srs * 12 // comb) * (((4 * c["freq_position"]) // m_srs) % n)
    n_cs, k0 = [], []
    for p in range(nap):
        n_cs.append(cs if "cs_port0" in perturb else (cs + (n_cs_max * p) // nap) % n_cs_max)
        k_tc = c["comb_offset"]
        if interleaved and p in (1, 3) and "ktc_fixed" not in perturb:
            k_tc = (k_tc + comb // 2) % comb
        k0.append(c["freq_shift"] * 12 + k_tc + total)
    M = 128
    while M < L * 4096 // 3300:
        M *= 2
    khz = 15 << c["numerology"]
    half_cp = float((144 * 64) // (1 << (c["numerology"] + 1))) * T_C
    fs = float(M * khz * 1000 * comb)
    max_ta = 1.0 / float(n_cs_max * khz * 1000 * comb)
    max_ta_samples = min(int(np.floor(half_cp * fs)), int(np.floor(max_ta * fs)))
    return dict(L=L, n_cs_max=n_cs_max, u=c["sequence_id"] % 30, interleaved=interleaved, n_cs=n_cs, k0=k0, M=M, fs=fs,
                khz=khz, max_ta_samples=max_ta_samples)


def is_prime(x):
    return x > 1 and all(x % d for d in range(2, int(x ** 0.5) + 1))


@functools.lru_cache(maxsize=None)
def sequence(u, L, n_cs, n_cs_max):
    """r_{u,0}(n) e^{j 2 pi n_cs n / n_cs_max}, n = 0..L-1 (TS 38.211 section 5.2.2; the cyclic shift as the reference
    reads it from its 24-entry table)."""
    n = np.arange(L)
    if L in PHI:
        base = np.asarray(PHI[L][u]) * np.pi / 4
    else:
        assert L >= 36
        nzc = L - 1
        while not is_prime(nzc):
            nzc -= 1
        q_hat = np.float32(nzc) * np.float32(u + 1) / np.float32(31)
        q = int(np.float32(np.float64(q_hat) + 0.5))
        mm = n % nzc
        base = -np.pi * ((q * mm * (mm + 1)) % (2 * nzc)) / nzc
    step = n_cs * 24 // n_cs_max
    return np.exp(1j * (base + 2 * np.pi * ((n * step) % 24) / 24))


def phase_indices(L, ps, po):
    """The reference's float32 arithmetic, operation by operation; std::round rounds halves away from zero."""
    n = np.arange(L, dtype=np.float32)
    t = (np.float32(CEXP_SIZE) * (n * np.float32(ps) + np.float32(po))) / TWOPI32
    assert t.dtype == np.float32
    t = t.astype(np.float64)
    return (np.sign(t) * np.floor(np.abs(t) + 0.5)).astype(np.int64) & (CEXP_SIZE - 1)


def refine(corr, idx, max_ta_samples):
    """fractional_sample_delay with the reference's decimal weights."""
    M = corr.size
    if max_ta_samples > 2:
        num_w, den_w, k = (-0.4, -0.2, 0.0, 0.2, 0.4), (0.571429, -0.285714, -0.571429, -0.285714, 0.571429), 1.0
    else:
        num_w, den_w, k = (-0.5, 0.0, 0.5), (0.5, -1.0, 0.5), 0.5
    taps = np.array([corr[(idx + i - len(num_w) // 2) % M] for i in range(len(num_w))])
    num = float(np.dot(np.float32(num_w).astype(np.float64), taps))
    den = float(np.dot(np.float32(den_w).astype(np.float64), taps))
    with np.errstate(all="ignore"):
        r = np.float64(-k * num) / np.float64(den)
    return 0.0 if (np.isnan(r) or np.isinf(r) or abs(r) > 1.0) else float(r)


# ---- the estimator ---------------------------------------------------------------------------------------------

def estimate(c, grid, perturb=()):
    """c: the resource; grid: complex (ports, 14, subcarriers). -> dict(channel (nrx, nap), epre, noise_var,
    time_alignment, resolution, ta_max, ta_idx [nap], gap [nap]: by how much of itself the winning tap leads every other
    searched tap, runner_up [nap])."""
    d = derive(c, perturb)
    L, comb, nap, nsym, M, m = d["L"], c["comb_size"], c["nof_antenna_ports"], c["nof_symbols"], d["M"], d["max_ta_samples"]
    rx = list(range(len(c["rx_ports"]))) if "rx_order" in perturb else list(c["rx_ports"])
    nrx = len(rx)
    syms = range(c["start_symbol"], c["start_symbol"] + nsym)
    seqs = [sequence(d["u"], L, d["n_cs"][p], d["n_cs_max"]) for p in range(nap)]

    def received(r, p):  # (nof_symbols, L)
        return np.stack([grid[rx[r], s, d["k0"][p]: d["k0"][p] + L * comb: comb] for s in syms])
    owners = [0, 1] if d["interleaved"] else [0]
    epre = 0.0
    lse = np.zeros((nrx, nap, L), complex)
    ta_sum, ta_idx, ta_port, gaps, runner = 0.0, [], [], [], []
    for p in range(nap):
        corr = np.zeros(M)
        for r in range(nrx):
            y = received(r, p)
            if p in owners:
                epre += float((np.abs(y) ** 2).mean(axis=1).sum())
            lse[r, p] = (y * seqs[p].conj()).sum(axis=0) / (1 if "no_symbol_mean" in perturb else nsym)
            x = np.zeros(M, complex)
            x[:L] = lse[r, p]
            corr += np.abs(np.fft.ifft(x) * M) ** 2
        delayed, advanced = corr[:m], corr[M - m:]
        di, ai = int(np.argmax(delayed)), int(np.argmax(advanced))
        idx = di if delayed[di] >= advanced[ai] else -(m - ai)
        searched = np.concatenate([delayed, advanced])
        win = corr[idx % M]
        others = np.delete(searched, di if idx >= 0 else m + ai)
        gaps.append(float((win - others.max()) / win) if win > 0 else 0.0)
        second = int(np.argmax(np.where(np.arange(2 * m) == (di if idx >= 0 else m + ai), -np.inf, searched)))
        runner.append(second if second < m else second - 2 * m)
        ta_port.append((float(idx) + refine(corr, idx, m)) / d["fs"])
        ta_sum += ta_port[-1]
        ta_idx.append(idx)
    ta = ta_sum / nap
    twopi = float(TWOPI32)
    ps = np.float32(twopi * ta * d["khz"] * 1000 * comb)
    if "slope_sign" in perturb:
        ps = -ps
    table = np.exp(2j * np.pi * np.arange(CEXP_SIZE) / CEXP_SIZE)
    cexp = []
    for p in range(nap):
        po = ps * np.float32(d["k0"][p] % comb) / np.float32(comb)
        cexp.append(table[phase_indices(L, ps, po)])
    channel = np.zeros((nrx, nap), complex)
    noise = 0.0
    for r in range(nrx):
        helper = {}
        for p in range(nap):
            channel[r, p] = (lse[r, p] * cexp[p]).mean()
            q = p % 2 if d["interleaved"] else 0
            if q not in helper:
                helper[q] = received(r, q).sum(axis=0) * cexp[q]
            # srsvec::subtract takes its output first: subtract(noise_help, recovered, noise_help) leaves recovered -
            # noise_help (:249). The helper changes sign with every antenna port, so on a comb set with two or four
            # ports every other port's signal is added, not removed. Restated as it is.
            helper[q] = nsym * channel[r, p] * seqs[p] - helper[q]
        noise += sum(float((np.abs(h) ** 2).sum()) for h in helper.values())
    nof_estimates, correction = (2, 2) if d["interleaved"] else (nap, 1)
    if "noise_div_nap" in perturb:
        nof_estimates = nap
    noise /= float((nsym * L - nof_estimates) * correction * nrx)
    epre /= float(nsym * correction * nrx)
    return dict(channel=channel, epre=epre, noise_var=noise, time_alignment=ta, resolution=1.0 / d["fs"],
                ta_max=m / d["fs"], ta_idx=ta_idx, ta_port=ta_port, gap=gaps, runner_up=runner, derived=d)


def decidable(r, delta=KERNEL_DELTA):
    """Every antenna port's winning tap leads every other searched tap by more than delta of itself. An all-zero
    correlation counts: float32 leaves exact zeros exact, so the tie (tap 0, the delayed half) is the same everywhere."""
    return all(g > delta or (g == 0.0 and r["epre"] == 0.0) for g in r["gap"])


def applies(name, c, r):
    """Whether a hand-made error must show on the case: it changes what is computed there, and the case has a signal."""
    d = r["derived"]
    if c["recipe"]["kind"] != "signal":
        return False
    nap = c["nof_antenna_ports"]
    return {"cs_port0": nap > 1,
            "ktc_fixed": bool(d["interleaved"]),
            "noise_div_nap": bool(d["interleaved"]),
            "no_symbol_mean": c["nof_symbols"] > 1,
            "slope_sign": min(abs(t) for t in r["ta_idx"]) >= 1 and abs(r["time_alignment"]) * d["fs"] >= 1.0,
            "rx_order": list(c["rx_ports"]) != list(range(len(c["rx_ports"])))}[name]


# ---- the transmitter and the channel ---------------------------------------------------------------------------

def make_grid(c, rng, fill=0.0):
    """The complex grid (grid_nof_ports, 14, subcarriers of the smallest grid that holds the resource) with the resource
    through c["recipe"]: kind signal | noise | zero, snr_db, delay (taps of 1 / fs, positive = delayed)."""
    d, rec = derive(c), c["recipe"]
    comb, nap, nsym, L = c["comb_size"], c["nof_antenna_ports"], c["nof_symbols"], d["L"]
    nsc = 12 * c["grid_nof_prb"]
    grid = np.full((c["grid_nof_ports"], 14, nsc), fill, complex)
    k_all = sorted({d["k0"][p] for p in range(nap)})
    for port in c["rx_ports"]:
        for s in range(c["start_symbol"], c["start_symbol"] + nsym):
            for k0 in k_all:
                grid[port, s, k0: k0 + L * comb: comb] = 0.0
    if rec["kind"] == "zero":
        return grid
    amp = rec.get("amplitude", 1.0)
    tau = rec.get("delay", 0.0) / d["fs"]
    for r, port in enumerate(c["rx_ports"]):
        for p in range(nap):
            if rec["kind"] != "signal":
                break
            h = amp * (rng.standard_normal() + 1j * rng.standard_normal()) / np.sqrt(2)
            if abs(h) < 0.3 * amp:
                h *= 0.3 * amp / abs(h)
            k = d["k0"][p] + comb * np.arange(L)
            tx = h * sequence(d["u"], L, d["n_cs"][p], d["n_cs_max"]) * np.exp(-2j * np.pi * k * d["khz"] * 1000 * tau)
            for s in range(c["start_symbol"], c["start_symbol"] + nsym):
                grid[port, s, k] += tx
        sigma = amp * 10.0 ** (-rec.get("snr_db", 30.0) / 20.0)
        for s in range(c["start_symbol"], c["start_symbol"] + nsym):
            for k0 in k_all:
                grid[port, s, k0: k0 + L * comb: comb] += sigma * awgn(rng, L)
    return grid


def read_words(c, grid_words):
    """The words the estimator reads, (nof_rx_ports, nof_symbols, comb sets, L): all the fixture keeps of a grid."""
    d = derive(c)
    k_all = sorted({d["k0"][p] for p in range(c["nof_antenna_ports"])})
    return np.stack([np.stack([np.stack([grid_words[port, s, k0: k0 + d["L"] * c["comb_size"]: c["comb_size"]] for k0 in k_all])
                               for s in range(c["start_symbol"], c["start_symbol"] + c["nof_symbols"])])
                     for port in c["rx_ports"]])


def write_words(c, words, grid_words):
    """The inverse of read_words, into a (ports, 14, subcarriers) uint32 grid."""
    d = derive(c)
    k_all = sorted({d["k0"][p] for p in range(c["nof_antenna_ports"])})
    for r, port in enumerate(c["rx_ports"]):
        for i, s in enumerate(range(c["start_symbol"], c["start_symbol"] + c["nof_symbols"])):
            for q, k0 in enumerate(k_all):
                sl = (port, s, slice(k0, k0 + d["L"] * c["comb_size"], c["comb_size"]))
                grid_words[sl] = words[r, i, q]
    return grid_words


def min_grid_prb(c):
    d = derive(c)
    return (max(d["k0"]) + (d["L"] - 1) * c["comb_size"]) // 12 + 1


# ---- cases -----------------------------------------------------------------------------------------------------

def find_row(table, m_srs, b):
    """The first C_SRS whose row has m_SRS,b = m_srs; table: (64, 4, 2) of (m_srs, N)."""
    for c_srs in range(64):
        if table[c_srs][b][0] == m_srs:
            return c_srs
    raise KeyError((m_srs, b))


def case(table, name, m_srs, b, comb, nap, rx_ports, nsym, cs, recipe, comb_offset=0, numerology=1, n_id=None, n_rrc=0,
         n_shift=0, start=None, grid_nof_ports=4):
    c_srs = find_row(table, m_srs, b)
    c = dict(name=name, c_srs=c_srs, row=tuple((int(m), int(n)) for m, n in table[c_srs]), numerology=numerology,
             nof_antenna_ports=nap, nof_symbols=nsym, start_symbol=14 - nsym if start is None else start, comb_size=comb,
             comb_offset=comb_offset, cyclic_shift=cs, sequence_id=(7 * len(name) + 31 * m_srs + cs) % 1024 if n_id is None else n_id,
             bandwidth_index=b, freq_position=n_rrc, freq_shift=n_shift, rx_ports=tuple(rx_ports),
             grid_nof_ports=grid_nof_ports, recipe=recipe)
    c["grid_nof_prb"] = min_grid_prb(c)
    return c


def sig(snr_db, delay, amplitude=1.0):
    return dict(kind="signal", snr_db=snr_db, delay=delay, amplitude=amplitude)


def golden_recipes(table):
    """The fixture's cases: the smallest shapes at which each path can go wrong."""
    out = []
    add = lambda *a, **k: out.append(case(table, *a, **k))  # noqa: E731
    # Sequence lengths: 12 and 24 (tables, both combs), 36 and 48 (first Zadoff-Chu), 96 | 108, 120 (IDFT 128 | 256),
    # 816 (1024), 1632 (2048).
    add("L12_comb4", 4, 0, 4, 1, [0], 1, 0, sig(20, 0.0))
    add("L24_comb2", 4, 0, 2, 2, [1, 0], 2, 3, sig(15, 2.2), comb_offset=1)
    add("L24_comb4", 8, 0, 4, 4, [0, 1, 2, 3], 1, 2, sig(25, -1.3), comb_offset=3)
    add("L36_interleaved", 12, 0, 4, 4, [2, 0], 2, 7, sig(20, 1.7), comb_offset=1)
    add("L48_comb2_wrap", 8, 0, 2, 2, [0, 1], 4, 6, sig(10, -2.25), numerology=0)
    add("L48_interleaved_comb2", 8, 0, 2, 4, [3, 1, 0, 2], 1, 5, sig(30, 3.2), comb_offset=1, numerology=2)
    add("L96_idft128", 16, 0, 2, 1, [0, 1], 2, 1, sig(5, 4.3), numerology=3)
    add("L108_idft256", 36, 0, 4, 2, [1], 1, 11, sig(12, -5.7), comb_offset=2)
    add("L120_idft256", 20, 0, 2, 4, [0, 2], 1, 2, sig(18, 6.25), numerology=0)
    add("L816_idft1024", 136, 0, 2, 2, [0, 1], 1, 4, sig(8, 20.3))
    add("L1632_idft2048", 272, 0, 2, 1, [1, 3], 1, 0, sig(3, -33.7), comb_offset=1)
    # Every cyclic shift and comb offset, B_SRS 0..3 with a frequency position and shift, numerologies 0..3.
    for comb in (2, 4):
        for cs in range(12 if comb == 4 else 8):
            b = cs % 4
            m = {0: 16, 1: 8, 2: 4, 3: 4}[b]
            nap = (1, 2, 4)[cs % 3]
            rx = ([0], [2, 0], [3, 1, 0, 2], [1, 2])[(cs + comb) % 4]
            add(f"cs{cs}_comb{comb}", m, b, comb, nap, rx, (1, 2, 4)[(cs // 3 + comb) % 3], cs,
                sig(3.0 * (cs % 11), ((cs * 37) % 11 - 5) * 0.6 + 0.15), comb_offset=(cs + 1) % comb, numerology=cs % 4,
                n_rrc=5 + 3 * cs, n_shift=1 + 2 * cs, start=None if cs % 2 else (cs % 5))
    # The channel: delays near +-max_ta_samples and beyond the search range, pure noise, an all-zero grid, 0 and 30 dB.
    add("delay_near_max", 16, 0, 2, 1, [0, 1], 1, 0, sig(20, 7.8), numerology=0)
    add("advance_near_max", 16, 0, 2, 2, [0, 1], 2, 1, sig(20, -7.8), numerology=0)
    add("delay_beyond", 16, 0, 2, 1, [0, 1], 1, 0, sig(20, 30.3), numerology=0)
    add("zero_delay_0dB", 12, 0, 4, 4, [0, 1, 2, 3], 4, 9, sig(0, 0.0))
    add("zero_delay_30dB", 12, 0, 4, 4, [0, 1, 2, 3], 4, 3, sig(30, 0.0))
    add("small_amplitude", 8, 0, 2, 2, [0, 1], 2, 2, sig(20, 1.2, amplitude=1e-3))
    add("pure_noise", 8, 0, 2, 2, [0, 1], 2, 0, dict(kind="noise", snr_db=0.0))
    add("pure_noise_interleaved", 12, 0, 4, 4, [1, 0], 1, 8, dict(kind="noise", snr_db=0.0))
    add("all_zero", 8, 0, 4, 4, [0, 1], 2, 7, dict(kind="zero"))
    return out


def draw(cases, seed):
    """Every case's grid words, redrawn per case until the case is decidable. -> [(words as read_words, restatement)]."""
    out = []
    for i, c in enumerate(cases):
        for attempt in range(64):
            rng = np.random.default_rng([seed, i, attempt])
            words = to_bf16_words(make_grid(c, rng))
            r = estimate(c, words_to_complex(words))
            if decidable(r):
                break
        else:
            raise SystemExit(f"{c['name']}: no decidable draw")
        out.append((read_words(c, words), r))
    return out


def cfg_row(c):
    rx = (list(c["rx_ports"]) + [0] * 4)[:4]
    return [c["c_srs"], c["numerology"], c["nof_antenna_ports"], c["nof_symbols"], c["start_symbol"], c["comb_size"],
            c["comb_offset"], c["cyclic_shift"], c["sequence_id"], c["bandwidth_index"], c["freq_position"],
            c["freq_shift"], len(c["rx_ports"]), *rx, c["grid_nof_ports"]]


@functools.lru_cache(maxsize=1)
def golden():
    """(cases, table): every fixture case with its words and the reference's results; the reference's whole table of
    (m_srs, N) by (C_SRS, B_SRS), recorded as data."""
    z = np.load(GOLDEN)
    table = z["table"]
    cases, at, kinds = [], 0, ("signal", "noise", "zero")
    for i, name in enumerate(z["names"]):
        v = dict(zip(CFG_KEYS, (int(x) for x in z["cfg"][i])))
        c = dict(name=str(name), c_srs=v["c_srs"], row=tuple((int(m), int(n)) for m, n in table[v["c_srs"]]),
                 rx_ports=tuple(v[f"rx{k}"] for k in range(v["nof_rx_ports"])),
                 recipe=dict(kind=kinds[int(z["kind"][i])], delay=float(z["delay"][i]), snr_db=float(z["snr_db"][i])))
        c.update({k: v[k] for k in CFG_KEYS[1:12]})
        c["grid_nof_ports"] = v["grid_nof_ports"]
        c["grid_nof_prb"] = min_grid_prb(c)
        d = derive(c)
        shape = (len(c["rx_ports"]), c["nof_symbols"], 2 if d["interleaved"] else 1, d["L"])
        n = int(np.prod(shape))
        c["words"] = z["words"][at: at + n].reshape(shape)
        at += n
        nap = c["nof_antenna_ports"]
        c["ref"] = dict(channel=z["channel"][i][: shape[0], :nap], epre=float(z["epre"][i]), noise_var=float(z["noise_var"][i]),
                        time_alignment=float(z["time_alignment"][i]), resolution=float(z["resolution"][i]),
                        ta_max=float(z["ta_max"][i]), ta_min=float(z["ta_min"][i]),
                        ta_port=[float(t) for t in z["ta_port"][i][:nap]])
        cases.append(c)
    assert at == z["words"].size
    return cases, table


def case_grid_words(c, fill=0):
    """A fixture case's own grid (grid_nof_ports, 14, subcarriers) with `fill` in every word the estimator does not read."""
    g = np.full((c["grid_nof_ports"], 14, 12 * c["grid_nof_prb"]), fill, np.uint32)
    return write_words(c, c["words"], g)


@functools.lru_cache(maxsize=1)
def restate_golden():
    cases, _ = golden()
    return [estimate(c, words_to_complex(case_grid_words(c))) for c in cases]


# ---- comparison ------------------------------------------------------------------------------------------------

def rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-300)


def deviations(got, want):
    """got, want: dicts with channel, epre, noise_var, time_alignment, resolution. The four normalised deviations of
    got from want; the time alignment's is only meaningful on equal ta_idx."""
    h, hw = np.asarray(got["channel"]), np.asarray(want["channel"])
    norm = float(np.sqrt((np.abs(hw) ** 2).sum()))
    dev = dict(channel=float(np.sqrt((np.abs(h - hw) ** 2).sum())) / norm if norm > 0 else float(np.abs(h).max()),
               epre=rel(got["epre"], want["epre"]) if want["epre"] > 0 else abs(float(got["epre"])),
               time_alignment=abs(got["time_alignment"] - want["time_alignment"]) / want["resolution"])
    floor = max(want["noise_var"], NOISE_FLOOR * want["epre"])
    dev["noise_var"] = abs(got["noise_var"] - want["noise_var"]) / floor if floor > 0 else abs(float(got["noise_var"]))
    return dev


def reference_ta_idx(c, r):
    """The tap the reference's mean time alignment implies for a single antenna port (its fraction is within +-1)."""
    return c["ref"]["time_alignment"] * r["derived"]["fs"]


def measured_deviations(restated):
    cases, _ = golden()
    worst = dict(channel=0.0, epre=0.0, noise_var=0.0, time_alignment=0.0)
    for c, r in zip(cases, restated):
        for k, v in deviations(c["ref"], r).items():
            worst[k] = max(worst[k], v)
    return worst


def tolerances():
    """Ten times the measured deviation of the reference from the restatement, floored at 1e-4."""
    return {k: max(10 * v, 1e-4) for k, v in MEASURED.items()}


def record_as_dict(rec, c):
    """An SRS_RESULT_DTYPE record as the dict deviations() takes."""
    nrx, nap = len(c["rx_ports"]), c["nof_antenna_ports"]
    h = rec["channel"][:nrx, :nap, 0].astype(np.float64) + 1j * rec["channel"][:nrx, :nap, 1].astype(np.float64)
    return dict(channel=h, epre=float(rec["epre"]), noise_var=float(rec["noise_var"]),
                time_alignment=float(rec["time_alignment"]), resolution=float(rec["resolution"]),
                ta_max=float(rec["ta_max"]), ta_idx=[int(t) for t in rec["ta_idx"][:nap]])


def failures(got, want, tol, check_idx=True):
    """The quantities on which got misses want; empty when the comparison passes."""
    bad = []
    if check_idx and list(got["ta_idx"]) != list(want["ta_idx"]):
        bad.append("ta_idx")
    dev = deviations(got, want)
    same_idx = list(got["ta_idx"]) == list(want["ta_idx"])
    for k, v in dev.items():
        if k == "time_alignment" and not same_idx:
            continue
        if not v <= tol[k]:
            bad.append(k)
    return bad


# ---- plans for the GPU tests -----------------------------------------------------------------------------------

def place(cases, words_of, grid_nof_prb, grid_nof_ports, nof_grids, grid_of, fill=NAN_WORD):
    """The grids (nof_grids, ports, 14, 12 PRBs) uint32 holding every case's words, `fill` everywhere else; two cases on
    the same REs of a grid are an error."""
    grids = np.full((nof_grids, grid_nof_ports, 14, 12 * grid_nof_prb), fill, np.uint32)
    taken = np.zeros(grids.shape, bool)
    for i, (c, words) in enumerate(zip(cases, words_of)):
        mark = write_words(c, np.ones(words.shape, np.uint32), np.zeros(grids.shape[1:], np.uint32)).astype(bool)
        assert not (taken[grid_of[i]] & mark).any(), ("two cases share REs", c["name"])
        taken[grid_of[i]] |= mark
        write_words(c, words, grids[grid_of[i]])
    return grids


def pack(cases, grid_nof_prb, nof_grids_max=64):
    """grid_of: each case in the first grid where its REs are free (first fit), so several share a grid."""
    used, grid_of = [], []
    for c in cases:
        mark = write_words(c, np.ones(read_shape(c), np.uint32), np.zeros((4, 14, 12 * grid_nof_prb), np.uint32)).astype(bool)
        for g, u in enumerate(used):
            if not (u & mark).any():
                u |= mark
                grid_of.append(g)
                break
        else:
            used.append(mark)
            grid_of.append(len(used) - 1)
    assert len(used) <= nof_grids_max
    return grid_of, len(used)


def read_shape(c):
    d = derive(c)
    return (len(c["rx_ports"]), c["nof_symbols"], 2 if d["interleaved"] else 1, d["L"])


def random_plan_cases(table, rng, count=40):
    """Fresh resources for the GPU tests, grid of 272 PRBs x 4 ports: small ones with every parameter drawn, and one
    272-PRB 4 x 4 x 4-symbol interleaved resource."""
    out = [case(table, "wide_4x4x4_interleaved", 272, 0, 2, 4, [0, 1, 2, 3], 4, 5, sig(15, 12.3), comb_offset=1)]
    rx_lists = ([0], [3], [1, 0], [2, 0], [0, 1, 2, 3], [3, 1, 0, 2], [1, 2, 3])
    while len(out) < count:
        comb = int(rng.choice((2, 4)))
        b = int(rng.integers(0, 4))
        c_srs = int(rng.integers(0, 64))
        m = int(table[c_srs][b][0])
        if m > (48 if len(out) % 8 else 136):
            continue
        d_taps = float(rng.integers(-6, 7)) + float(rng.uniform(-0.3, 0.3))
        kind = sig(float(rng.uniform(0, 30)), d_taps, amplitude=float(10 ** rng.uniform(-2, 1)))
        if len(out) % 13 == 5:
            kind = dict(kind="noise", snr_db=0.0)
        nsym = int(rng.choice((1, 2, 4)))
        c = dict(name=f"random{len(out)}", c_srs=c_srs, row=tuple((int(x), int(n)) for x, n in table[c_srs]),
                 numerology=int(rng.integers(0, 4)), nof_antenna_ports=int(rng.choice((1, 2, 4))), nof_symbols=nsym,
                 start_symbol=int(rng.integers(0, 15 - nsym)), comb_size=comb, comb_offset=int(rng.integers(0, comb)),
                 cyclic_shift=int(rng.integers(0, 12 if comb == 4 else 8)), sequence_id=int(rng.integers(0, 1024)),
                 bandwidth_index=b, freq_position=int(rng.integers(0, 68)), freq_shift=int(rng.integers(0, 60)),
                 rx_ports=tuple(rx_lists[int(rng.integers(0, len(rx_lists)))]), grid_nof_ports=4, recipe=kind)
        c["grid_nof_prb"] = min_grid_prb(c)
        if c["grid_nof_prb"] > 272:
            continue
        out.append(c)
    return out
