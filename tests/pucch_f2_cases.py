"""PUCCH Format 2 front end: the float64 restatement of the reference's path from the grid to the descrambled LLRs and
the per-port channel state, the case generator of tests/golden/pucch_f2.npz, a transmitter, a float32 restatement of the
GPU kernel's own sequence of operations, and the hand-made errors the tests tell the kernel apart from.
TEST INFRASTRUCTURE ONLY.

Reference (behaviour, not code; paths under lib/phy/upper/):
  signal_processors/pucch/dmrs_pucch_estimator_format2.cpp:34/:43/:87  DM-RS c_init with n_id_0, advanced by 8 bits per
                                                    grid PRB, amplitude 1/sqrt(2); REs 1, 4, 7, 10 of every PRB
  signal_processors/port_channel_estimator_average_impl.cpp:77/:154     the hop loop: compute_hop once or twice, the
                                                    time alignment halved with hopping, RSRP / EPRE / noise normalised
                                                    over both hops, the noise floored at RSRP / 10^10
  signal_processors/port_channel_estimator_helpers.cpp:203/:246        filter smoothing, time alignment with stride 3
  channel_processors/pucch/pucch_demodulator_format2.cpp:92/:162       data REs k mod 3 != 1, symbol-major; ZF 1 x N;
                                                    QPSK; descrambling with c_init = rnti 2^15 + n_id

Two things the reference does and this file restates as they are:
  * get_data_re_ests (:185) reads the data REs of receive port i from grid port i, not from ports[i], while the
    estimator reads its pilots from ports[i] (port_channel_estimator_helpers.cpp:182). With a port list other than
    0..P-1 the data of one grid port is equalised with the channel of another.
  * The estimates the demodulator reads are bf16 (channel_estimate holds cbf16_t)."""
import functools
import os

import numpy as np

import pusch_chest_oracle as CH
import pusch_demod_oracle as D
import uci_cases as SB
import uci_polar_cases as PL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pucch_f2.npz")
NO_HOP = 0xFFFF
T_C = 1.0 / (480000 * 4096)
F = np.float32
CLASS_NOISE, CLASS_INFORMATIVE, CLASS_HIGH = 0, 1, 2
MAX_CODE_RATE = 0.8
PERTURBATIONS = ("filter_stride_2", "no_bf16", "hop1_from_hop0", "ta_not_halved", "dmrs_not_advanced",
                 "scrambling_n_id_0")
CFG_FIELDS = ("slot_index", "numerology", "cp_extended", "starting_prb", "second_hop_prb", "nof_prb", "start_symbol",
              "nof_symbols", "rnti", "n_id", "n_id_0", "nof_ports", "port0", "port1", "port2", "port3", "grid_nof_ports",
              "grid_nof_prb", "nof_uci_bits")


# ---- words ---------------------------------------------------------------------------------------------------------

def words_to_complex(words):
    w = np.asarray(words, np.uint32)
    re = (w << np.uint32(16)).view(np.float32).astype(np.float64)
    im = (w & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    return re + 1j * im


def to_bf16(v):
    u = np.asarray(v, F).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)


def complex_to_words(z):
    z = np.asarray(z)
    return to_bf16(z.real) | (to_bf16(z.imag) << np.uint32(16))


def round_bf16(z):
    return words_to_complex(complex_to_words(z))


# ---- derived quantities --------------------------------------------------------------------------------------------

def nsymb_per_slot(cp_extended):
    return 12 if cp_extended else 14


def crc_size(a):
    return 0 if a < 12 else 6 if a < 20 else 11


def code_rate(nof_prb, nof_symbols, a):
    """pucch_format2_code_rate (pucch_info.h:57): payload plus CRC bits over the channel bits, in float32."""
    ncb = 2 if (a >= 360 and 16 * nof_prb * nof_symbols >= 1088) or a >= 1013 else 1
    return F(a + ncb * crc_size(a)) / F(nof_prb * 8 * nof_symbols * 2)


def max_payload(nof_prb, nof_symbols):
    a = 3
    while a < 1706 and code_rate(nof_prb, nof_symbols, a + 1) <= F(MAX_CODE_RATE):
        a += 1
    return a


def nof_llrs(cfg):
    return 16 * cfg["nof_prb"] * cfg["nof_symbols"]


def hop_list(cfg):
    """[(symbols of the slot, first grid PRB)] per hop."""
    s0, n = cfg["start_symbol"], cfg["nof_symbols"]
    if cfg["second_hop_prb"] != NO_HOP:
        return [([s0], cfg["starting_prb"]), ([s0 + 1], cfg["second_hop_prb"])]
    return [(list(range(s0, s0 + n)), cfg["starting_prb"])]


def symbol_prb(cfg, i):
    """First grid PRB of the i-th symbol of the PDU."""
    return cfg["second_hop_prb"] if (i > 0 and cfg["second_hop_prb"] != NO_HOP) else cfg["starting_prb"]


def symbol_epochs(numerology, cp_extended):
    """initialize_symbol_start_epochs: CH.symbol_start_epochs for the normal CP; the extended CP is 512 kappa >> mu on
    every symbol (cyclic_prefix.h:98)."""
    if not cp_extended:
        return CH.symbol_start_epochs(numerology)
    d = (512 >> numerology) * 64 * T_C * (15 << numerology) * 1000
    return np.array([d + i * (d + 1.0) for i in range(12)])


@functools.lru_cache(maxsize=4096)
def _gold(c_init, n):
    return D.gold_sequence(c_init, n)


def dmrs_c_init(cfg, symbol):
    n_id = cfg["n_id_0"]
    return ((nsymb_per_slot(cfg["cp_extended"]) * cfg["slot_index"] + symbol + 1) * (2 * n_id + 1) * (1 << 17)
            + 2 * n_id) % (1 << 31)


def dmrs_sequence(cfg, symbol, prb, perturb=()):
    """The 4 nof_prb pilots of one symbol at grid PRB `prb` on."""
    skip = 0 if "dmrs_not_advanced" in perturb else 8 * prb
    n = 8 * cfg["nof_prb"]
    c = _gold(dmrs_c_init(cfg, symbol), 8 * ((skip + n + 7) // 8 + 1))[skip: skip + n].astype(np.float64)
    return ((1 - 2 * c[0::2]) + 1j * (1 - 2 * c[1::2])) / np.sqrt(2)


def scrambling_bits(cfg, perturb=()):
    n_id = cfg["n_id_0"] if "scrambling_n_id_0" in perturb else cfg["n_id"]
    return _gold(cfg["rnti"] * (1 << 15) + n_id, 512)[: nof_llrs(cfg)]


def data_subcarriers(nof_prb):
    k = np.arange(12 * nof_prb)
    return k[k % 3 != 1]


def to_tc(seconds):
    """phy_time_unit::from_seconds(...).to_seconds(): truncate ten times the T_c count, round half away."""
    tc10 = int(float(seconds) / T_C * 10.0)
    return (int(tc10 / 10) + int(np.fmod(tc10, 10) / 5)) * T_C


# ---- the restatement -----------------------------------------------------------------------------------------------

def hop_time_alignment(f, numerology):
    """time_alignment_estimator_dft_impl::estimate(symbols, stride 3) of one hop's smoothed pilots, unrounded, as the
    float the estimator adds up (port_channel_estimator_average_impl.cpp:307). At most 64 pilots: the 128-point IDFT,
    and a window of 13 samples on either side for every numerology."""
    M = CH.ta_dft_size(f.size)
    m, fs = CH.ta_max_samples(numerology, M, 3)
    assert M == 128 and m == 13
    x = np.zeros(M, np.complex128)
    x[: f.size] = f
    corr = np.abs(np.fft.ifft(x) * M) ** 2
    d_i, a_i = int(np.argmax(corr[:m])), int(np.argmax(corr[M - m:]))
    idx = d_i if corr[d_i] >= corr[M - m + a_i] else -(m - a_i)
    frac = CH.fractional_sample_delay(np.array([corr[(idx + i - 2) % M] for i in range(5)]))
    return F((idx + frac) / fs)


def estimate(cfg, grid, perturb=()):
    """dmrs_pucch_estimator_format2::estimate. grid (grid ports, 14, 12 grid PRBs) complex. Returns a dict: est (P,
    nof_symbols, 12 nof_prb) the estimates the demodulator reads, noise_var, rsrp, epre, ta (seconds on the T_c grid),
    ta_raw (before rounding), cfo_hz (NaN when no hop has two symbols), all (P,)."""
    ports, nprb, num = cfg["ports"], cfg["nof_prb"], cfg["numerology"]
    P, s0 = len(ports), cfg["start_symbol"]
    hops = hop_list(cfg)
    ep = symbol_epochs(num, cfg["cp_extended"])
    est = np.zeros((P, cfg["nof_symbols"], 12 * nprb), np.complex128)
    out = dict(noise_var=np.zeros(P), rsrp=np.zeros(P), epre=np.zeros(P), ta=np.zeros(P), ta_raw=np.zeros(P),
               cfo_hz=np.full(P, np.nan))
    stride = 2 if "filter_stride_2" in perturb else 3
    for i, port in enumerate(ports):
        rsrp = epre = noise = 0.0
        ta, cfo = F(0), None
        for h, (syms, prb) in enumerate(hops):
            read_prb = hops[0][1] if (h == 1 and "hop1_from_hop0" in perturb) else prb
            k = 12 * read_prb + 1 + 3 * np.arange(4 * nprb)
            rx = [grid[port, l, k] for l in syms]
            pil = [dmrs_sequence(cfg, l, prb, perturb) for l in syms]
            lse = [r * np.conj(q) for r, q in zip(rx, pil)]
            if len(syms) == 2:
                c = float(np.angle(np.dot(np.conj(lse[0]), lse[1]))) / (2 * np.pi) / (ep[syms[1]] - ep[syms[0]])
                cfo = c if cfo is None else (cfo + c) / 2
            f = CH.fd_smoothing(sum(lse) / len(syms), nprb, stride, "filter")
            epre += sum(float(np.sum(np.abs(r) ** 2)) for r in rx)
            rsrp += float(np.sum(np.abs(f) ** 2)) * len(syms)
            noise += sum(float(np.sum(np.abs(r - f * q) ** 2)) for r, q in zip(rx, pil))
            ta = F(ta + hop_time_alignment(f, num))
            fr = CH.interpolate(f, 1, 3, 12 * nprb)
            for l in syms:
                est[i, l - s0] = fr if "no_bf16" in perturb else round_bf16(fr)
        if len(hops) == 2 and "ta_not_halved" not in perturb:
            ta = F(ta / F(2))
        n = 4 * nprb * cfg["nof_symbols"]
        out["rsrp"][i], out["epre"][i] = rsrp / n, epre / n
        out["noise_var"][i] = max(rsrp / n / 1e10, noise / (n - 1))
        out["ta_raw"][i], out["ta"][i] = float(ta), to_tc(float(ta))
        if cfo is not None:
            out["cfo_hz"][i] = cfo * (15 << num) * 1000
    out["est"] = est
    return out


def data_res(cfg, grid, nof_ports):
    """get_data_re_ests: (P, n) data REs, symbol-major, read from grid ports 0..P-1 (see the module docstring)."""
    dk = data_subcarriers(cfg["nof_prb"])
    return np.stack([np.concatenate([grid[i, cfg["start_symbol"] + s, 12 * symbol_prb(cfg, s) + dk]
                                     for s in range(cfg["nof_symbols"])]) for i in range(nof_ports)])


def demodulate(cfg, grid, est, noise_var, perturb=()):
    """pucch_demodulator_format2::demodulate -> descrambled int8 LLRs."""
    P = len(cfg["ports"])
    dk = data_subcarriers(cfg["nof_prb"])
    rx = data_res(cfg, grid, P)
    H = np.stack([np.concatenate([est[i, s, dk] for s in range(cfg["nof_symbols"])]) for i in range(P)])
    eq, nvar = D.equalize(rx.astype(np.complex64), H[:, None, :].astype(np.complex64), np.asarray(noise_var, F))
    llr = D.demap(eq.reshape(-1), nvar.reshape(-1), 2).astype(np.int16)
    return np.where(scrambling_bits(cfg, perturb) == 1, -llr, llr).astype(np.int8)


def restate(cfg, grid, perturb=()):
    """The whole front end: estimate() plus llrs."""
    r = estimate(cfg, grid, perturb)
    r["llrs"] = demodulate(cfg, grid, r["est"], r["noise_var"], perturb)
    return r


def decode(llrs, a):
    """uci_decoder::decode of a Format 2 payload: (bits, valid)."""
    if a <= 11:
        bits, valid, _ = SB.detect(llrs, a, 2)
        return np.asarray(bits, np.uint8), bool(valid)
    bits, valid, _ = PL.decode(llrs, a)
    return bits, bool(valid)


# ---- the kernel's float32 sequence ---------------------------------------------------------------------------------

def filter_taps(nof_prb):
    """(float32 taps of filter_type(nof_prb, stride 3), renormalised in float32 as it does, n_v)."""
    # The oracle's formula at unit energy to seven decimals, as the reference tabulates it; its table holds n = 14 and
    # 16 one unit of the last decimal below the rounded value.
    rc = CH.rc_filter_taps()
    q = np.rint(rc / np.sqrt(np.sum(rc * rc)) * 1e7)
    q[[14, 16]] -= 1
    rc = (q / 1e7).astype(F)
    half = (min(nof_prb, 3) * 10 + 1) // 2 // 3
    taps = rc[15 - 3 * half: 15 + 3 * half + 1: 3]
    total = F(0)
    for t in taps:
        total = F(total + t)
    taps = (taps * (F(1) / total)).astype(F)
    return taps, (4 if nof_prb == 1 else min(12, taps.size // 2))


def _v_pilots_f32(base, is_start):
    n = base.size
    ab = np.abs(base).astype(F)
    ar = np.angle(base).astype(F)
    for j in range(1, n):  # unwrap
        d = F(ar[j] - ar[j - 1])
        ar[j:] = (ar[j:] - F(2 * np.pi) * F(np.round(d / F(2 * np.pi)))).astype(F)
    x = np.arange(n, dtype=F)
    mean_x = F(F(n * (n - 1)) / F(2) / F(n))
    den = F(F((n - 1) * n * (2 * n - 1)) / F(6) - F(n) * mean_x * mean_x)
    out = []
    for v in (ab, ar):
        mean = F(np.sum(v, dtype=F) / F(n))
        slope = F((np.sum(v * x, dtype=F) - mean_x * mean * F(n)) / den)
        out.append((slope, F(mean - slope * mean_x)))
    xv = (np.arange(n) + (-n if is_start else n)).astype(F)
    rho = (out[0][0] * xv + out[0][1]).astype(F)
    arg = (out[1][0] * xv + out[1][1] + np.where(rho > 0, F(0), F(np.pi))).astype(F)
    return (np.abs(rho) * (np.cos(arg).astype(F) + 1j * np.sin(arg).astype(F))).astype(np.complex64)


def restate_f32(cfg, grid):
    """The kernel's own sequence (srsran-5g_amd/csrc/pucch_f2.hip) in numpy float32, every product and sum rounded to
    float32: what float32 arithmetic alone moves against restate(). Returns the same dict (no est)."""
    C64 = np.complex64
    ports, nprb, num = cfg["ports"], cfg["nof_prb"], cfg["numerology"]
    P, s0, np_ = len(ports), cfg["start_symbol"], 4 * cfg["nof_prb"]
    hops = hop_list(cfg)
    ep = symbol_epochs(num, cfg["cp_extended"])
    taps, nv = filter_taps(nprb)
    est = np.zeros((P, cfg["nof_symbols"], 12 * nprb), np.complex128)
    out = dict(noise_var=np.zeros(P), rsrp=np.zeros(P), epre=np.zeros(P), ta=np.zeros(P), ta_raw=np.zeros(P),
               cfo_hz=np.full(P, np.nan))
    tw = np.exp(2j * np.pi * np.arange(128) / 128).astype(C64)
    n_all = np_ * cfg["nof_symbols"]
    for i, port in enumerate(ports):
        rsrp = epre = noise = F(0)
        ta, cfo = 0.0, None
        for syms, prb in hops:
            k = 12 * prb + 1 + 3 * np.arange(np_)
            rx = [grid[port, l, k].astype(C64) for l in syms]
            pil = [dmrs_sequence(cfg, l, prb).astype(C64) for l in syms]
            lse = [(r * np.conj(q)).astype(C64) for r, q in zip(rx, pil)]
            if len(syms) == 2:
                acc = np.sum((lse[1] * np.conj(lse[0])).astype(C64), dtype=C64)
                ph = F(np.arctan2(F(acc.imag), F(acc.real)))
                cfo = F(ph / F(2 * np.pi) / F(ep[syms[1]] - ep[syms[0]]))
            f = (sum(lse).astype(C64) * F(1.0 / len(syms))).astype(C64)
            big = np.concatenate([_v_pilots_f32(f[:nv], True), f, _v_pilots_f32(f[-nv:], False)]).astype(C64)
            h = taps.size // 2
            pad = np.concatenate([np.zeros(h, C64), big, np.zeros(h, C64)])
            sm = np.zeros(np_, C64)
            for t in range(taps.size):
                sm = (sm + pad[nv + t: nv + t + np_] * taps[t]).astype(C64)
            f = sm
            epre = F(epre + sum(np.sum((r.real * r.real + r.imag * r.imag).astype(F), dtype=F) for r in rx))
            rsrp = F(rsrp + np.sum((f.real * f.real + f.imag * f.imag).astype(F), dtype=F) * F(len(syms)))
            for r, q in zip(rx, pil):
                e = (r - (f * q).astype(C64)).astype(C64)
                noise = F(noise + np.sum((e.real * e.real + e.imag * e.imag).astype(F), dtype=F))
            m, fs = 13, 128 * (15 << num) * 1000.0 * 3
            corr = np.zeros(128, F)
            for n in list(range(m + 2)) + list(range(128 - m - 2, 128)):
                v = np.sum((f * tw[(np.arange(np_) * n) % 128]).astype(C64), dtype=C64)
                corr[n] = F(v.real * v.real + v.imag * v.imag)
            d_i, a_i = int(np.argmax(corr[:m])), int(np.argmax(corr[128 - m:]))
            idx = d_i if corr[d_i] >= corr[128 - m + a_i] else -(m - a_i)
            c5 = np.array([corr[(idx + j - 2) % 128] for j in range(5)], F)
            nu = F(np.dot(np.array([-0.4, -0.2, 0.0, 0.2, 0.4], F), c5))
            de = F(np.dot(np.array([0.571429, -0.285714, -0.571429, -0.285714, 0.571429], F), c5))
            with np.errstate(divide="ignore", invalid="ignore"):
                q = F(-nu / de)
            frac = 0.0 if (not np.isfinite(q) or abs(q) > 1) else float(q)
            ta += float(F((idx + frac) / fs))
            fr = np.empty(12 * nprb, C64)
            for kk in range(12 * nprb):
                j, r = divmod(kk - 1, 3)
                if kk < 1:
                    fr[kk] = f[0]
                elif j >= np_ - 1:
                    fr[kk] = f[np_ - 1]
                else:
                    fr[kk] = C64(f[j] + C64(C64(f[j + 1] - f[j]) * F(r / 3.0)))
            for l in syms:
                est[i, l - s0] = round_bf16(fr)
        if len(hops) == 2:
            ta = float(F(F(ta) / F(2)))
        out["rsrp"][i], out["epre"][i] = F(rsrp / F(n_all)), F(epre / F(n_all))
        out["noise_var"][i] = max(F(out["rsrp"][i] / 1e10), F(noise / F(n_all - 1)))
        out["ta_raw"][i], out["ta"][i] = ta, to_tc(ta)
        if cfo is not None:
            out["cfo_hz"][i] = F(cfo * F((15 << num) * 1000))
    out["llrs"] = demodulate(cfg, grid, est, out["noise_var"])
    return out


# ---- the transmitter -----------------------------------------------------------------------------------------------

def encode(bits, e):
    """uci_encoder for a Format 2 payload: short block (3..11 bits, QPSK) or polar."""
    if len(bits) <= 11:
        return np.asarray(SB.encode(bits, 2, e), np.uint8)
    return np.asarray(PL.encode(bits, e), np.uint8)


def awgn(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


def transmit(rng, cfg, bits, snr, delay_s=0.0, cfo_norm=0.0, gains=None, dead=()):
    """The grid (grid ports, 14, 12 grid PRBs) complex, rounded to bf16 values, of one PDU alone: encode, scramble, QPSK,
    map with the DM-RS, then per grid port a complex gain, the delay's phase ramp over the subcarriers, the CFO's phase
    over the symbols' start epochs and noise of variance 1 / snr per RE on the allocation (snr linear per port; bits
    None: noise only, variance 1). Grid ports in `dead` carry zeros."""
    pg, nsc = cfg["grid_nof_ports"], 12 * cfg["grid_nof_prb"]
    grid = np.zeros((pg, 14, nsc), np.complex128)
    ep = symbol_epochs(cfg["numerology"], cfg["cp_extended"])
    nprb = cfg["nof_prb"]
    if gains is None:
        gains = np.exp(2j * np.pi * rng.random(pg)) * rng.uniform(0.7, 1.3, pg)
    if bits is not None:
        c = encode(bits, nof_llrs(cfg)) ^ scrambling_bits(cfg)
        sym = ((1 - 2.0 * c[0::2]) + 1j * (1 - 2.0 * c[1::2])) / np.sqrt(2)
    dk = data_subcarriers(nprb)
    for s in range(cfg["nof_symbols"]):
        l, prb = cfg["start_symbol"] + s, symbol_prb(cfg, s)
        tx = np.zeros(12 * nprb, np.complex128)
        if bits is not None:
            tx[dk] = sym[s * dk.size: (s + 1) * dk.size]
            tx[1::3] = dmrs_sequence(cfg, l, prb)
        k = 12 * prb + np.arange(12 * nprb)
        ramp = np.exp(-2j * np.pi * k * (15 << cfg["numerology"]) * 1000.0 * delay_s) * np.exp(2j * np.pi * ep[l] * cfo_norm)
        for p in range(pg):
            if p in dead:
                continue
            sigma = 1.0 if bits is None else np.sqrt(1.0 / snr)
            grid[p, l, k] = gains[p] * tx * ramp + sigma * awgn(rng, k.size)
    return round_bf16(grid)


# ---- cases ---------------------------------------------------------------------------------------------------------

def make_cfg(rng, nof_prb, nof_symbols, hop, ports, a, numerology=1, cp_extended=0, start_symbol=None, grid_nof_ports=None,
             grid_nof_prb=24, lower_hop=False):
    nsl = nsymb_per_slot(cp_extended)
    if start_symbol is None:
        start_symbol = int(rng.integers(0, nsl - nof_symbols + 1))
    span = grid_nof_prb - nof_prb
    if hop:
        a0, a1 = sorted(int(v) for v in rng.choice(span + 1, 2, replace=False)) if span > 0 else (0, 0)
        first, second = (a1, a0) if lower_hop else ((a0, a1) if rng.random() < 0.5 else (a1, a0))
        if lower_hop and span == 0:
            raise ValueError("no room to hop")
    else:
        first, second = int(rng.integers(0, span + 1)), NO_HOP
    n_id = int(rng.integers(0, 1024))
    return dict(slot_index=int(rng.integers(0, 10 << numerology)), numerology=numerology, cp_extended=cp_extended,
                starting_prb=first, second_hop_prb=second, nof_prb=nof_prb, start_symbol=start_symbol,
                nof_symbols=nof_symbols, rnti=int(rng.integers(1, 65520)), n_id=n_id,
                n_id_0=int((n_id + rng.integers(1, 65535)) % 65536), ports=list(ports),
                grid_nof_ports=grid_nof_ports or max(max(ports) + 1, len(ports)), grid_nof_prb=grid_nof_prb,
                nof_uci_bits=a)


INFORMATIVE_SNR = 4.0  # post-equalisation: LLR = 10 SNR +- 10 sqrt(SNR) sits inside (0, 120)


def make_case(rng, cfg, cls, delay_samples=0.0, cfo_norm=0.0, dead=()):
    """-> (cfg, allocation words (grid ports, nof_symbols, 12 nof_prb), sent bits or None, class)."""
    a = cfg["nof_uci_bits"]
    live = max(1, len([p for p in cfg["ports"] if p not in dead]))
    bits = None if cls == CLASS_NOISE else rng.integers(0, 2, a).astype(np.uint8)
    snr = 1000.0 if cls == CLASS_HIGH else INFORMATIVE_SNR / live
    fs = 128 * (15 << cfg["numerology"]) * 1000.0 * 3
    grid = transmit(rng, cfg, bits, snr, delay_samples / fs, cfo_norm, dead=dead)
    return cfg, allocation_words(cfg, grid), bits, cls


def allocation_words(cfg, grid):
    return np.stack([[complex_to_words(grid[p, cfg["start_symbol"] + s,
                                            12 * symbol_prb(cfg, s): 12 * (symbol_prb(cfg, s) + cfg["nof_prb"])])
                      for s in range(cfg["nof_symbols"])] for p in range(cfg["grid_nof_ports"])])


def grid_of(cfg, words, fill=0.0):
    """The grid (grid ports, 14, 12 grid PRBs) with the allocation's words placed and `fill` elsewhere."""
    g = np.full((cfg["grid_nof_ports"], 14, 12 * cfg["grid_nof_prb"]), fill, np.complex128)
    z = words_to_complex(np.asarray(words).reshape(cfg["grid_nof_ports"], cfg["nof_symbols"], 12 * cfg["nof_prb"]))
    for s in range(cfg["nof_symbols"]):
        prb = symbol_prb(cfg, s)
        g[:, cfg["start_symbol"] + s, 12 * prb: 12 * (prb + cfg["nof_prb"])] = z[:, s]
    return g


def golden_generator_cases(rng):
    """The cases of tests/golden/pucch_f2.npz: every branch of the front end at its smallest shape. Most cases are
    informative (two draws of payload, channel and noise per shape for one at 30 dB, whose LLRs all sit at +-120)."""
    out = []

    def add(cfg, classes=(CLASS_INFORMATIVE, CLASS_INFORMATIVE, CLASS_HIGH), **kw):
        for cls in classes:
            out.append(make_case(rng, dict(cfg), cls, **kw))

    # 1 PRB x 1 symbol x 1 port: 4 pilots, n_v = 4, 3 taps, 16 LLRs; 2 PRB: 7 taps, n_v = 3; 3 PRB: 11 taps, n_v = 5.
    for a in (3, 11):
        for _ in range(3):
            add(make_cfg(rng, 1, 1, False, [0], a))
    for nprb, sizes in ((2, (4, 11, 12, 19)), (3, (7, 12, 19, 20, 27)), (4, (20, 40)), (5, (11, 50)), (7, (30,)),
                        (11, (60,))):
        for a in sizes:
            for ports in ([0], [0, 1]):
                add(make_cfg(rng, nprb, 1, False, ports, a))
    # The maximum: 16 PRB x 2 symbols x 4 ports with hopping, up to the largest payload the code rate admits.
    for a in (11, 12, 20, 200, max_payload(16, 2)):
        add(make_cfg(rng, 16, 2, True, [0, 1, 2, 3], a, grid_nof_prb=40))
    # Two symbols without hopping (CFO reported, symbols averaged) and with it, a hop into a lower PRB among them.
    for nprb, a, ports in ((1, 3, [0]), (1, 12, [0, 1]), (2, 19, [0]), (3, 20, [0, 1, 2]), (5, 64, [0, 1]), (16, 100, [0])):
        add(make_cfg(rng, nprb, 2, False, ports, a), cfo_norm=float(rng.uniform(-0.02, 0.02)))
        add(make_cfg(rng, nprb, 2, True, ports, a))
        add(make_cfg(rng, nprb, 2, True, ports, a, lower_hop=True), classes=(CLASS_INFORMATIVE,))
    # Extended CP at numerology 2; numerologies 0 and 3.
    for nsym, hop in ((1, False), (2, False), (2, True)):
        add(make_cfg(rng, 3, nsym, hop, [0, 1], 14, numerology=2, cp_extended=1), cfo_norm=0.01 * (nsym == 2 and not hop))
        add(make_cfg(rng, 2, nsym, hop, [0], 8, numerology=2, cp_extended=1, start_symbol=12 - nsym))
    for num in (0, 2, 3):
        add(make_cfg(rng, 4, 2, False, [0, 1], 24, numerology=num), cfo_norm=-0.015)
    # Port lists that are not 0..P-1 (the data REs then come from other grid ports than the pilots).
    for ports in ([2], [1, 3], [3, 0, 2], [1, 0], [3, 2, 1, 0]):
        add(make_cfg(rng, 2, 2, True, ports, 9, grid_nof_ports=4))
        add(make_cfg(rng, 3, 1, False, ports, 13, grid_nof_ports=4), classes=(CLASS_INFORMATIVE,))
    # A start symbol of 12 or 13.
    add(make_cfg(rng, 2, 2, False, [0], 6, start_symbol=12), cfo_norm=0.008)
    add(make_cfg(rng, 2, 2, True, [0, 1], 15, start_symbol=12))
    add(make_cfg(rng, 1, 1, False, [0], 5, start_symbol=13))
    add(make_cfg(rng, 6, 1, False, [0, 1], 33, start_symbol=13))
    # Delays of both signs up to the window of 13 samples.
    for d in (-12.6, -9.2, -4.5, -1.3, -0.4, 0.45, 1.7, 5.5, 8.8, 12.4):
        add(make_cfg(rng, 16, 1, False, [0], 40, grid_nof_prb=30), classes=(CLASS_INFORMATIVE,), delay_samples=d)
        add(make_cfg(rng, 6, 2, True, [0, 1], 21), classes=(CLASS_INFORMATIVE,), delay_samples=d)
        add(make_cfg(rng, 3, 2, False, [0], 12, numerology=int(rng.integers(0, 4))), classes=(CLASS_HIGH,), delay_samples=d)
    # A dead port.
    add(make_cfg(rng, 2, 1, False, [0, 1], 10), dead=(1,))
    add(make_cfg(rng, 4, 2, True, [0, 1, 2, 3], 25), dead=(0,))
    add(make_cfg(rng, 1, 2, False, [1, 0], 4, grid_nof_ports=2), dead=(1,))
    # Pure noise, polar payloads mostly: 64 of them, so that the few a 6-bit CRC lets through (1 in 64) stay a small share.
    for _ in range(16):
        for nprb, nsym, a in ((2, 1, 12), (3, 2, 19), (4, 1, 20), (8, 2, 64), (1, 1, 7)):
            hop = bool(nsym == 2 and rng.random() < 0.5)
            add(make_cfg(rng, nprb, nsym, hop, [0, 1][: int(rng.integers(1, 3))], a), classes=(CLASS_NOISE,))
    return out


NAN_WORD = 0x7FC07FC0   # bf16 NaN in both halves
HUGE_WORD = 0x714A714A  # bf16 1e30 in both halves


def allocation_mask(cfg, shape):
    """True on the REs of a (ports, 14, subcarriers) grid that the PDU occupies, on every grid port it was made for."""
    m = np.zeros(shape, bool)
    for s in range(cfg["nof_symbols"]):
        prb = symbol_prb(cfg, s)
        m[: cfg["grid_nof_ports"], cfg["start_symbol"] + s, 12 * prb: 12 * (prb + cfg["nof_prb"])] = True
    return m


def place(placed, grid_nof_prb, grid_nof_ports, nof_grids, fill=(NAN_WORD, HUGE_WORD)):
    """The grids (nof_grids, ports, 14, 12 PRBs) uint32 holding the allocation words of every (cfg, words, grid index)
    of `placed` and, in every other RE, the fill words in turn (NaN and 1e30); two PDUs on the same REs are an error."""
    shape = (nof_grids, grid_nof_ports, 14, 12 * grid_nof_prb)
    grids = np.where(np.arange(int(np.prod(shape))).reshape(shape) % 2 == 0, np.uint32(fill[0]), np.uint32(fill[-1]))
    grids = grids.astype(np.uint32)
    taken = np.zeros(shape, bool)
    for cfg, words, g in placed:
        mark = allocation_mask(cfg, shape[1:])
        assert not (taken[g] & mark).any(), ("two PDUs share REs", cfg)
        taken[g] |= mark
        w = np.asarray(words, np.uint32).reshape(cfg["grid_nof_ports"], cfg["nof_symbols"], 12 * cfg["nof_prb"])
        for s in range(cfg["nof_symbols"]):
            prb = symbol_prb(cfg, s)
            grids[g, : cfg["grid_nof_ports"], cfg["start_symbol"] + s, 12 * prb: 12 * (prb + cfg["nof_prb"])] = w[:, s]
    return grids


def grids_to_complex(grids):
    """uint32 grids -> complex128 (NaN and 1e30 where the fill words lie)."""
    return words_to_complex(grids)


def random_plan_cases(rng, count=60, grid_nof_prb=52, nof_grids=6):
    """Fresh PDUs for the GPU tests, several per grid of 52 PRBs x 4 ports on REs of their own: -> [(cfg, words, grid
    index, sent bits or None)]. Shapes, hops, port lists, numerologies, payloads, delays and the SNR class are drawn."""
    taken = np.zeros((nof_grids, 4, 14, 12 * grid_nof_prb), bool)
    port_lists = ([0], [0, 1], [0, 1, 2, 3], [0, 1, 2], [2], [1, 3], [3, 1, 0, 2])
    out = []
    while len(out) < count:
        nprb = int(rng.choice([1, 1, 2, 2, 3, 3, 4, 5, 8, 16]))
        nsym = int(rng.integers(1, 3))
        hop = bool(nsym == 2 and rng.random() < 0.5)
        ports = port_lists[int(rng.integers(0, len(port_lists)))]
        a = int(rng.integers(3, min(max_payload(nprb, nsym), 120) + 1))
        num = int(rng.integers(0, 4))
        cfg = make_cfg(rng, nprb, nsym, hop, ports, a, numerology=num, cp_extended=int(num == 2 and rng.random() < 0.3),
                       grid_nof_ports=4, grid_nof_prb=grid_nof_prb)
        g = int(rng.integers(0, nof_grids))
        mark = allocation_mask(cfg, taken.shape[1:])
        if (taken[g] & mark).any():
            continue
        taken[g] |= mark
        cls = (CLASS_INFORMATIVE, CLASS_INFORMATIVE, CLASS_HIGH, CLASS_NOISE)[int(rng.integers(0, 4))]
        cfg, words, bits, _ = make_case(rng, cfg, cls, delay_samples=float(rng.uniform(-12, 12)),
                                        cfo_norm=float(rng.uniform(-0.02, 0.02)) if (nsym == 2 and not hop) else 0.0)
        out.append((cfg, words, g, bits))
    return out


BENCH_SEED = 20274


def bench_batch_cases(rng, nof_slots=32, per_slot=8):
    """The batch of tools/pucch_f2_bench.py and of tools/gen_pucch_f2_golden.py --time: 32 slots of 52 PRBs x 4 ports,
    8 PDUs each on six PRBs of their own (1..3 PRB, hopping or not, or 4 PRB), 1..2 symbols, 4 ports, CSI-sized
    payloads -> [(cfg, words, grid index)]."""
    out = []
    for slot in range(nof_slots):
        for j in range(per_slot):
            nprb, nsym = int(rng.integers(1, 5)), int(rng.integers(1, 3))
            hop = bool(nsym == 2 and nprb <= 3 and rng.random() < 0.5)
            a = int(rng.integers(4, min(max_payload(nprb, nsym), 40) + 1))
            cfg = make_cfg(rng, nprb, nsym, hop, [0, 1, 2, 3], a, grid_nof_prb=52)
            cfg.update(starting_prb=6 * j, second_hop_prb=6 * j + 3 if hop else NO_HOP)
            cfg, words, _, _ = make_case(rng, cfg, CLASS_INFORMATIVE)
            out.append((cfg, words, slot))
    return out


def cfg_row(cfg):
    ports = (list(cfg["ports"]) + [0] * 4)[:4]
    return [cfg["slot_index"], cfg["numerology"], cfg["cp_extended"], cfg["starting_prb"], cfg["second_hop_prb"],
            cfg["nof_prb"], cfg["start_symbol"], cfg["nof_symbols"], cfg["rnti"], cfg["n_id"], cfg["n_id_0"],
            len(cfg["ports"]), *ports, cfg["grid_nof_ports"], cfg["grid_nof_prb"], cfg["nof_uci_bits"]]


def cfg_from_row(row):
    d = {k: int(v) for k, v in zip(CFG_FIELDS, row)}
    d["ports"] = [d.pop(f"port{i}") for i in range(4)][: d.pop("nof_ports")]
    return d


@functools.lru_cache(maxsize=1)
def golden():
    """The fixture as a list of dicts: cfg, words, grid-independent reference results (llrs, noise_var, rsrp, epre, ta,
    cfo_hz per port, bits, status, csi: the reference's combined channel state information, NaN for what it leaves
    unset), sent (None for noise), snr_class, decidable."""
    g = np.load(GOLDEN)
    cases, wpos, lpos, bpos = [], 0, 0, 0
    for i, row in enumerate(g["cfg"]):
        cfg = cfg_from_row(row)
        P, a = len(cfg["ports"]), cfg["nof_uci_bits"]
        nw, nl = cfg["grid_nof_ports"] * cfg["nof_symbols"] * 12 * cfg["nof_prb"], nof_llrs(cfg)
        cases.append(dict(cfg=cfg, words=g["words"][wpos: wpos + nw], llrs=g["llrs"][lpos: lpos + nl],
                          noise_var=g["noise_var"][i, :P], rsrp=g["rsrp"][i, :P], epre=g["epre"][i, :P],
                          ta=g["ta"][i, :P], cfo_hz=g["cfo_hz"][i, :P], bits=g["bits"][bpos: bpos + a],
                          status=int(g["status"][i]), sent=None if g["snr_class"][i] == CLASS_NOISE else g["sent"][bpos: bpos + a],
                          snr_class=int(g["snr_class"][i]), decidable=bool(g["decidable"][i]),
                          csi=dict(zip(("epre_db", "rsrp_db", "sinr_db", "time_alignment", "cfo_hz"), g["csi"][i]))))
        wpos, lpos, bpos = wpos + nw, lpos + nl, bpos + a
    assert wpos == g["words"].size and lpos == g["llrs"].size and bpos == g["bits"].size
    return cases


@functools.lru_cache(maxsize=1)
def restate_golden():
    """restate() of every fixture case, computed once and shared by the tests; nobody changes it."""
    return [restate(c["cfg"], grid_of(c["cfg"], c["words"])) for c in golden()]


@functools.lru_cache(maxsize=1)
def float32_deviations():
    """(share of the fixture's LLRs that restate_f32 moves against restate, the largest state_deviation per key)."""
    diff = total = 0
    dev = {}
    for c, r in zip(golden(), restate_golden()):
        f = restate_f32(c["cfg"], grid_of(c["cfg"], c["words"]))
        diff += llr_diff(f["llrs"], r["llrs"])[0]
        total += len(r["llrs"])
        for k, v in state_deviation(f, r).items():
            dev[k] = max(dev.get(k, 0.0), v)
    return diff / total, dev


def llr_share_bound():
    """The project's REF_PATHS_SHARE_BOUND rule: ten times the share float32 arithmetic alone moves, floored at 1e-3."""
    return max(10 * float32_deviations()[0], 1e-3)


# ---- comparisons ---------------------------------------------------------------------------------------------------

def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def llr_diff(a, b):
    """(number of LLRs that differ, largest difference)."""
    d = np.abs(np.asarray(a, np.int16) - np.asarray(b, np.int16))
    return int(np.count_nonzero(d)), int(d.max()) if d.size else 0


STATE_KEYS = ("noise_var", "rsrp", "epre")


def state_deviation(got, want):
    """Deviations of got from want (dicts with noise_var, rsrp, epre, ta, cfo_hz per port): the three powers relative
    to the port's EPRE (a dead port's powers are all zero: absolute there), the time alignment in T_c, the CFO
    relative to the subcarrier spacing / 1000 (1e-3 of a normalised CFO of 1)."""
    epre = np.maximum(np.asarray(want["epre"], np.float64), 1e-30)
    dev = {k: float(np.max(np.abs(np.asarray(got[k], np.float64) - np.asarray(want[k], np.float64)) / epre))
           for k in STATE_KEYS}
    dev["ta"] = float(np.max(np.abs(np.asarray(got["ta"], np.float64) - np.asarray(want["ta"], np.float64)))) / T_C
    g, w = np.asarray(got["cfo_hz"], np.float64), np.asarray(want["cfo_hz"], np.float64)
    if not np.array_equal(np.isnan(g), np.isnan(w)):
        dev["cfo"] = np.inf
    else:
        ok = ~np.isnan(w)
        dev["cfo"] = float(np.max(np.abs(g[ok] - w[ok]) / 15.0, initial=0.0))
    return dev


def measured_deviations(results, cases):
    """The largest state_deviation of `results` from the fixture's reference values per key, and the share of LLRs
    that differ."""
    dev = {k: 0.0 for k in STATE_KEYS + ("ta", "cfo")}
    diff = total = 0
    for r, c in zip(results, cases):
        for k, v in state_deviation(r, c).items():
            dev[k] = max(dev[k], v)
        diff += llr_diff(r["llrs"], c["llrs"])[0]
        total += len(c["llrs"])
    dev["llr_share"] = diff / max(total, 1)
    return dev


def tolerances(dev):
    """Ten times the measured reference-to-restatement deviation, floored at 1e-4; the time alignment within that
    margin or one T_c, whichever is larger."""
    tol = {k: max(10 * dev[k], 1e-4) for k in STATE_KEYS + ("cfo",)}
    tol["ta"] = max(10 * dev["ta"], 1.0)
    return tol


def perturbation_applies(name, cfg, true, pert):
    """Whether a hand-made error moves the restatement of a case far enough to be told apart: at least four LLRs, a
    power by 1 % of the EPRE, or the time alignment by two T_c."""
    if name in ("hop1_from_hop0", "ta_not_halved") and cfg["second_hop_prb"] == NO_HOP:
        return False
    if name == "dmrs_not_advanced" and cfg["starting_prb"] == 0 and cfg["second_hop_prb"] in (0, NO_HOP):
        return False
    return moved(true, pert)


def moved(a, b):
    dev = state_deviation(a, b)
    return llr_diff(a["llrs"], b["llrs"])[0] >= 4 or max(dev[k] for k in STATE_KEYS) > 1e-2 or dev["ta"] >= 2.0


def closer_to(got, true, pert):
    """got (the kernel's results) lies nearer the restatement than the perturbed restatement in what the perturbation
    moved: fewer differing LLRs, a smaller power deviation, a smaller time-alignment deviation."""
    dt, dp, d0 = state_deviation(got, true), state_deviation(got, pert), state_deviation(true, pert)
    ok = []
    if llr_diff(true["llrs"], pert["llrs"])[0] >= 4:
        ok.append(llr_diff(got["llrs"], true["llrs"])[0] < llr_diff(got["llrs"], pert["llrs"])[0])
    if max(d0[k] for k in STATE_KEYS) > 1e-2:
        ok.append(max(dt[k] for k in STATE_KEYS) < max(dp[k] for k in STATE_KEYS))
    if d0["ta"] >= 2.0:
        ok.append(dt["ta"] < dp["ta"])
    return bool(ok) and all(ok)


def informative_share(llrs):
    v = np.asarray(llrs, np.int16)
    return float(np.mean((v != 0) & (np.abs(v) != 120)))
