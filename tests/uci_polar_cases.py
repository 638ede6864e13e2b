"""Polar-coded UCI (12-1706 bits) test infrastructure: a numpy restatement of the reference's decoder chain
(uci_decoder_impl::decode_codeword_polar, lib/phy/upper/channel_processors/uci/uci_decoder_impl.cpp:43: segmentation
and CRC of TS 38.212 section 6.3.1.2.1, the code construction of polar_code_impl.cpp:325-490, the rate dematching of
polar_rate_dematcher_impl.cpp:100 with promotion_sum of log_likelihood_ratio.cpp:75, the simplified successive
cancellation decoder of polar_decoder_impl.cpp:335, the de-allocation of polar_deallocator_impl.cpp:27), of the
matching encoder chain, and seeded case generators. One rule differs from the reference on purpose: both codeblocks of
a two-codeblock field are always decoded (the reference leaves codeblock 1's bits untouched when codeblock 0 fails its
CRC), which is what the GPU plan does. The restatement is pinned to the reference's own outputs by
tests/test_uci_polar_oracle.py through tests/golden/uci_polar.npz (tools/gen_uci_polar_golden.py), which also holds
the two specification tables read here. TEST INFRASTRUCTURE ONLY."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uci_polar.npz")

LLR_MAX, LLR_INFTY = 120, 127
CRC_POLY = {6: 0x61, 11: 0xe21}
MAX_E_CB = 8192
UNTOUCHED = 2  # the fixture's mark for bits the reference decoder did not write

_tables = None


def tables():
    """(reliability sequence of TS 38.212 Table 5.3.1.2-1, sub-block interleaver pattern of Table 5.4.1.1-1)."""
    global _tables
    if _tables is None:
        g = np.load(GOLDEN)
        _tables = (g["reliability_sequence"].astype(np.int64), g["subblock_pattern"].astype(np.int64))
    return _tables


# ---- segmentation ----------------------------------------------------------------------------------------------

def nof_codeblocks(a, e):
    return 2 if (a >= 360 and e >= 1088) or a >= 1013 else 1


def crc_size(a):
    return 6 if a < 20 else 11


def codeblocks(a, e):
    """[(message bits, filler bits, K, E_cb)] of a field of a bits in e LLRs."""
    c, l = nof_codeblocks(a, e), crc_size(a)
    out = [(a // c, a % c, a // c + a % c + l, e // c)]
    if c == 2:
        out.append(((a + 1) // 2, 0, (a + 1) // 2 + l, e // c))
    return out


# ---- code construction -----------------------------------------------------------------------------------------

def code_size_log(k, e):
    el = 1
    while (1 << el) < e:
        el += 1
    n1 = el - 1 if (8 * e <= 9 * (1 << (el - 1)) and 16 * k < 9 * e) else el
    kl = 0
    while kl < 10 and (1 << kl) < k:
        kl += 1
    return max(5, min(n1, kl + 3, 10))


def code_refusal(k, e):
    """Why the reference's assertions refuse (K, E) (polar_code_impl.cpp:334-407), or None."""
    if e > MAX_E_CB:
        return "E"
    if k < 18 or 25 < k < 31 or k > 1023:
        return "K"
    if k + (3 if k <= 25 else 0) >= e:
        return "K + nPC"
    if k >= 1 << code_size_log(k, e):
        return "N"
    return None


def field_refusal(a, e):
    if not 12 <= a <= 1706:
        return "nof_bits"
    for _bits, _filler, k, e_cb in codeblocks(a, e):
        r = code_refusal(k, e_cb)
        if r:
            return r
    return None


def subblock_interleaver(n_log):
    n = 1 << n_log
    i = np.arange(n)
    return tables()[1][(32 * i) // n] * (n // 32) + i % (n // 32)


@functools.lru_cache(maxsize=None)
def channel_interleaver(e):
    """perm with f[i] = e[perm[i]] (polar_rate_matcher_impl.cpp:61): the triangle written by rows, read by columns."""
    t = 1
    while t * (t + 1) // 2 < e:
        t += 1
    perm = []
    for r in range(t):
        i_in = r
        for c in range(t - r):
            if i_in >= e:
                break
            perm.append(i_in)
            i_in += t - c
    return np.array(perm, np.int64)


@functools.lru_cache(maxsize=None)
def polar_code(k, e):
    """The code of (K, E), nMax = 10: dict with n, N, nPC, frozen (bool mask), pc (sorted positions), info (the K
    message positions, increasing, PC skipped), interleaver, and mode: 'repeat', 'puncture' or 'shorten'."""
    assert code_refusal(k, e) is None, (k, e, code_refusal(k, e))
    n_log = code_size_log(k, e)
    n = 1 << n_log
    npc = 3 if k <= 25 else 0
    nwm = 1 if npc and e > k + 189 else 0
    seq = tables()[0]
    seq = seq[seq < n]
    jj = subblock_interleaver(n_log)
    mode = "repeat"
    candidates = seq
    if e < n:
        if 16 * k <= 7 * e:
            mode = "puncture"
            pre = jj[: n - e]
            t = 3 * n // 4 - e // 2 - 1 if e >= 3 * n // 4 else 9 * n // 16 - e // 4
        else:
            mode = "shorten"
            pre = jj[e:]
            t = 0
        candidates = np.array([q for q in seq if q > t and q not in set(pre.tolist())], np.int64)
    k_set = candidates[candidates.size - k - npc:]
    pc = [int(q) for q in k_set[: npc - nwm]]
    if nwm:
        pc.append(252 if k <= 21 else 248)
    pc = sorted(pc)
    assert len(set(pc)) == npc and set(pc) <= set(k_set.tolist())
    frozen = np.ones(n, bool)
    frozen[k_set] = False
    info = np.array([q for q in np.flatnonzero(~frozen) if q not in pc], np.int64)
    assert info.size == k
    return dict(n=n_log, N=n, K=k, E=e, nPC=npc, frozen=frozen, pc=pc, info=info, interleaver=jj, mode=mode)


# ---- LLR arithmetic --------------------------------------------------------------------------------------------

def _special(a, b, r):
    r = np.where(np.abs(b) > LLR_MAX, b, r)
    r = np.where(np.abs(a) > LLR_MAX, a, r)
    return np.where(a == -b, 0, r)


def promotion_sum(a, b):
    """log_likelihood_ratio::promotion_sum (log_likelihood_ratio.cpp:75), element by element."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    s = a + b
    return _special(a, b, np.where(np.abs(s) > LLR_MAX, np.sign(s) * LLR_INFTY, s))


def saturated_sum(a, b):
    """log_likelihood_ratio::operator+= (log_likelihood_ratio.cpp:58), element by element."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return _special(a, b, np.clip(a + b, -LLR_MAX, LLR_MAX))


def soft_xor(a, b):
    return np.sign(a) * np.sign(b) * np.minimum(np.abs(a), np.abs(b))


# ---- decoder chain ---------------------------------------------------------------------------------------------

def accumulate(values, reverse=False):
    """The promotion sums of one position's repetitions in the reference's order (increasing k), or reversed."""
    values = list(values)[::-1] if reverse else list(values)
    acc = np.int64(values[0])
    for v in values[1:]:
        acc = promotion_sum(acc, v)
    return int(acc)


def rate_dematch(llrs, code):
    """polar_rate_dematcher_impl::rate_dematch (:100): the N LLRs of the mother code."""
    n, e = code["N"], code["E"]
    ee = np.zeros(e, np.int64)
    ee[channel_interleaver(e)] = np.asarray(llrs, np.int64)[:e]
    if code["mode"] == "repeat":
        y = ee[:n].copy()
        for r in range(1, (e + n - 1) // n):
            seg = ee[r * n: (r + 1) * n]
            y[: seg.size] = promotion_sum(y[: seg.size], seg)
    elif code["mode"] == "puncture":
        y = np.concatenate([np.zeros(n - e, np.int64), ee])
    else:
        y = np.concatenate([ee, np.full(n - e, LLR_INFTY, np.int64)])
    out = np.zeros(n, np.int64)
    out[code["interleaver"]] = y
    return out


def polar_transform(bits):
    x = np.array(bits, np.uint8)
    t = 1
    while t < x.size:
        v = x.reshape(-1, 2, t)
        v[:, 0, :] ^= v[:, 1, :]
        t *= 2
    return x


def sc_decode(llr, frozen):
    """polar_decoder_impl::decode (:335): the N decoded bits u. Rate-0 nodes give zeros, rate-1 nodes the hard decision
    `value <= 0` and its polar transform, rate-R nodes f, left, g, right, xor."""
    u = np.zeros(llr.size, np.uint8)
    nf = np.concatenate([[0], np.cumsum(frozen)])

    def node(l, lo, size):
        f = nf[lo + size] - nf[lo]
        if f == size:
            return np.zeros(size, np.uint8)
        if f == 0:
            x = (l <= 0).astype(np.uint8)
            u[lo: lo + size] = polar_transform(x)
            return x
        half = size // 2
        a, b = l[:half], l[half:]
        xl = node(soft_xor(a, b), lo, half)
        xr = node(np.where(xl == 0, saturated_sum(b, a), saturated_sum(b, -a)), lo + half, half)
        return np.concatenate([xl ^ xr, xr])

    node(np.asarray(llr, np.int64), 0, llr.size)
    return u


def crc_remainder(bits, size):
    poly, reg = CRC_POLY[size], 0
    for b in bits:
        reg = (reg << 1) | int(b)
        if reg >> size:
            reg ^= poly
    return reg


def crc_bits(bits, size):
    r = crc_remainder(list(bits) + [0] * size, size)
    return [(r >> (size - 1 - i)) & 1 for i in range(size)]


def decode_codeblock(llrs, k, e_cb):
    """(the K de-allocated bits, CRC remainder == 0)."""
    code = polar_code(k, e_cb)
    u = sc_decode(rate_dematch(llrs, code), code["frozen"])
    msg = u[code["info"]]
    return msg, crc_remainder(msg, 6 if k <= 25 else 11) == 0


def decode(llrs, a):
    """(bits, valid, per-codeblock validity) of a field of a bits, both codeblocks always decoded."""
    llrs = np.asarray(llrs, np.int64)
    l = crc_size(a)
    bits, ok, pos = [], [], 0
    for nbits, filler, k, e_cb in codeblocks(a, llrs.size):
        msg, good = decode_codeblock(llrs[pos: pos + e_cb], k, e_cb)
        bits.append(msg[filler: k - l])
        ok.append(bool(good))
        pos += e_cb
    return np.concatenate(bits).astype(np.uint8), all(ok), ok


# ---- encoder chain ---------------------------------------------------------------------------------------------

def encode_codeblock(msg, e_cb):
    code = polar_code(len(msg), e_cb)
    n = code["N"]
    u = np.zeros(n, np.uint8)
    if code["nPC"] == 0:
        u[code["info"]] = msg
    else:
        y, ik = [0] * 5, 0
        info = set(code["info"].tolist())
        for i in range(n):
            y = y[1:] + y[:1]
            if i in code["pc"]:
                u[i] = y[0]
            elif i in info:
                u[i] = msg[ik]
                y[0] ^= int(msg[ik])
                ik += 1
    y = polar_transform(u)[code["interleaver"]]
    if code["mode"] == "repeat":
        ee = y[np.arange(e_cb) % n]
    elif code["mode"] == "puncture":
        ee = y[n - e_cb:]
    else:
        ee = y[:e_cb]
    return ee[channel_interleaver(e_cb)]


def encode(bits, e):
    """The e encoded bits of a field (TS 38.212 sections 6.3.1.2.1-6.3.1.4.1); the e mod C bits left over are 0."""
    bits = [int(b) for b in bits]
    a, l = len(bits), crc_size(len(bits))
    out, taken = np.zeros(e, np.uint8), 0
    for r, (nbits, filler, _k, e_cb) in enumerate(codeblocks(a, e)):
        msg = [0] * filler + bits[taken: taken + nbits]
        taken += nbits
        out[r * e_cb: (r + 1) * e_cb] = encode_codeblock(msg + crc_bits(msg, l), e_cb)
    return out


# ---- case generators -------------------------------------------------------------------------------------------

def size_class(a, e):
    """0: one codeblock with K <= 25; 1: one codeblock with K >= 31; 2: two codeblocks."""
    return 2 if nof_codeblocks(a, e) == 2 else 0 if a < 20 else 1


def noisy_field(rng, a, e, amp, sigma=20.0):
    """(llrs, A, sent bits): a random message through the restated encoder, amplitude amp, N(0, sigma^2) noise."""
    bits = rng.integers(0, 2, a).astype(np.uint8)
    x = 1 - 2 * encode(bits, e).astype(np.float64)
    llrs = np.clip(np.rint(amp * x + rng.normal(0.0, sigma, e)), -LLR_MAX, LLR_MAX).astype(np.int8)
    return llrs, a, bits


# (K, E) list of the construction check: every n, puncturing, shortening, repetition with E >= 2N, nWmPC 0 / 1,
# K = 18, 25, 31 and 1023, E = 8192.
CODE_LIST = ((18, 22), (18, 30), (18, 32), (18, 33), (18, 69), (18, 100), (18, 207), (18, 208), (18, 240), (18, 8192),
             (21, 250), (22, 212), (25, 29), (25, 40), (25, 64), (25, 214), (25, 215), (25, 256), (25, 1000), (31, 32),
             (31, 36), (31, 60), (31, 64), (31, 100), (31, 517), (31, 8192), (40, 48), (40, 70), (59, 96), (59, 200),
             (64, 128), (65, 128), (65, 8192), (100, 110), (100, 127), (100, 128), (100, 129), (100, 180), (100, 500),
             (191, 544), (191, 543), (200, 230), (200, 300), (200, 576), (371, 380), (371, 543), (371, 544), (512, 600),
             (512, 1024), (512, 2053), (518, 1100), (864, 8192), (1000, 1024), (1023, 1024), (1023, 1025), (1023, 1087),
             (1023, 2048), (1023, 2053), (1023, 8192), (600, 700), (600, 1024), (300, 511), (300, 512), (150, 255))

# Field sizes per class (A, E) of the noise mix and the amplitudes tried on each.
NOISE_SIZES = (((12, 40), (15, 64), (19, 100), (19, 250), (14, 30)),
               ((20, 64), (30, 120), (48, 576), (100, 256), (200, 512), (359, 1087), (1012, 1030), (20, 240)),
               ((360, 1088), (361, 1201), (500, 2048), (1013, 2100), (1401, 3001), (1706, 3500)))
NOISE_AMPLITUDES = ((4, 8, 14, 22), (4, 8, 14, 22), (8, 14, 20, 30))


def noise_fields(rng, repeats=1):
    """Codewords at several amplitudes with N(0, 20^2) noise, every size class; (llrs, A, sent bits)."""
    out = []
    for sizes, amps in zip(NOISE_SIZES, NOISE_AMPLITUDES):
        for a, e in sizes:
            for amp in amps:
                for _ in range(repeats):
                    out.append(noisy_field(rng, a, e, amp))
    return out


def valid_shares(fields, results):
    """Share of valid fields per size class; results as decode() returns them."""
    return [float(np.mean([r[1] for f, r in zip(fields, results) if size_class(f[1], len(f[0])) == c]))
            for c in range(3)]


def partial_failure_fields(rng):
    """Two-codeblock fields at amplitude 60 where only codeblock 0 fails, only codeblock 1 fails, and both pass: the
    failing codeblock's LLRs are replaced by noise."""
    out = []
    for a, e in ((361, 1201), (1013, 2100)):
        for fail in ((True, False), (False, True), (False, False)):
            llrs, _, bits = noisy_field(rng, a, e, 60)
            half = e // 2
            for cb in range(2):
                if fail[cb]:
                    llrs[cb * half: (cb + 1) * half] = np.clip(np.rint(rng.normal(0, 20.0, half)), -120, 120)
            out.append((llrs, a, bits, fail))
    return out


def shape_sizes():
    """(A, E) of the smallest shapes where the kernel can go wrong (see tests/test_uci_polar_decoder_gpu.py)."""
    sizes = []
    # N = 32 .. 1024: punctured, shortened, E = N, N + 1, 2 N + 5 and 8192 where the construction allows them.
    for n_log, a_punct, a_short, a_rep in ((5, 12, 14, 12), (6, 12, 30, 13), (7, 20, 60, 20), (8, 20, 150, 30),
                                           (9, 40, 300, 60), (10, 100, 700, 200)):
        n = 1 << n_log
        sizes += [(a_punct, n - 3), (a_short, n - 3), (a_rep, n), (a_rep, n + 1)]
    sizes += [(19, 2 * 256 + 5), (20, 2 * 256 + 5), (50, 2 * 512 + 5), (200, 2 * 1024 + 5)]
    sizes += [(12, 8192), (19, 8192), (20, 8192), (50, 8192), (300, 8192)]
    # CRC6 / CRC11 and nPC boundary, the K gap.
    sizes += [(12, 60), (19, 60), (20, 60), (19, 250), (12, 208), (15, 211), (16, 212), (12, 30)]
    # One codeblock, K = 1023, long rate-1 nodes.
    sizes += [(1012, e) for e in (1024, 1025, 1056, 1087)]
    # Segmentation boundary, odd A (filler) and odd E with two codeblocks, the largest field.
    sizes += [(359, 1087), (359, 1088), (360, 1087), (360, 1088), (1013, 1100), (1013, 2047), (361, 1089), (777, 1999),
              (1706, 16384), (1705, 16383)]
    assert all(field_refusal(a, e) is None for a, e in sizes), [s for s in sizes if field_refusal(*s)]
    return sizes


def shape_fields(rng):
    """One field per shape_sizes() entry, amplitude 12 or 40 in turn; (llrs, A, sent bits)."""
    return [noisy_field(rng, a, e, (12, 40)[i % 2]) for i, (a, e) in enumerate(shape_sizes())]


def tie_fields(rng):
    """LLRs in {-1, 0, 1} and all-zero fields: the hard decision of 0 is bit 1."""
    out = []
    for a, e in ((12, 40), (19, 70), (20, 64), (48, 100), (100, 300), (360, 1088), (1012, 1030)):
        out.append((rng.integers(-1, 2, e).astype(np.int8), a, None))
        out.append((np.zeros(e, np.int8), a, None))
    return out


def saturation_fields(rng):
    """All +-120 fields with E >= 4 N (promotion to +-127 and the +-127 special sums in order), and fields built
    from the order-dependent pattern (100, 100, -100) per position."""
    out = []
    for a, e in ((12, 4 * 256 + 3), (20, 4 * 256), (30, 5 * 512 + 1), (100, 4 * 1024 + 7), (400, 8192)):
        out.append((np.where(rng.integers(0, 2, e) == 1, -120, 120).astype(np.int8), a, None))
        llrs, _, bits = noisy_field(rng, a, e, 60)
        out.append((np.where(llrs < 0, -120, 120).astype(np.int8), a, bits))
        out.append((rng.choice(np.array([100, -100, 127, -127, 60, 0], np.int8), e), a, None))
    return out


def slot_batch_fields(rng, nof_ues=64, nof_slots=1):
    """The slot-shaped batch of profiles/uci_polar_decoder.md: per UE a 20-bit HARQ-ACK in 240 LLRs and a 48-bit CSI
    Part 1 in 576, amplitude 20."""
    out = []
    for _ in range(nof_ues * nof_slots):
        out.append(noisy_field(rng, 20, 240, 20))
        out.append(noisy_field(rng, 48, 576, 20))
    return out


def golden_fields():
    """The fixture's decoder cases: (llrs, A, reference bits with UNTOUCHED marks, reference validity)."""
    g = np.load(GOLDEN)
    pos = bpos = 0
    for e, a, valid in zip(g["nof_enc_bits"], g["nof_bits"], g["ref_valid"]):
        yield g["llrs"][pos: pos + int(e)], int(a), g["ref_bits"][bpos: bpos + int(a)], bool(valid)
        pos += int(e)
        bpos += int(a)


def golden_generator_fields(rng):
    """The fields the fixture records (tools/gen_uci_polar_golden.py): the shapes, part of the noise mix, ties,
    saturation and partial failures; the number of E >= 8192 fields is bounded to keep the fixture small."""
    fields = shape_fields(rng) + noise_fields(rng) + tie_fields(rng) + saturation_fields(rng)[:9]
    fields += [f[:3] for f in partial_failure_fields(rng)]
    return [f for f in fields]
