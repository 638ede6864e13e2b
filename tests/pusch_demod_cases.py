"""PUSCH demodulator test configurations shared by the oracle-vs-reference tests, the golden-fixture generator and
the GPU parity tests. TEST INFRASTRUCTURE ONLY."""
import numpy as np

import ofdm_oracle
import pusch_demod_oracle as D

QAM_AMP = {2: 1 / np.sqrt(2), 4: 1 / np.sqrt(10), 6: 1 / np.sqrt(42), 8: 1 / np.sqrt(170)}


def bf16(x):
    return ofdm_oracle.complex_to_bf16(x)


def from_bf16(u):
    return ofdm_oracle.bf16_to_complex(u).astype(np.complex64)


def random_case(rng, grid_prb, nof_layers=None, nof_rx_ports=None, qm=None, snr_db=None, max_rb=None):
    """A transmission with random allocation / DM-RS pattern, a random flat-per-RE channel, QAM symbols through it plus
    noise. Returns (cfg, grid (P, 14, nsc, 2) bf16, ch_est (L, P, 14, nsc, 2) bf16, noise_var (P,) float32)."""
    L = int(nof_layers or rng.choice([1, 2]))
    P = int(nof_rx_ports or (rng.choice([1, 2, 3, 4]) if L == 1 else rng.choice([2, 4])))
    q = int(qm or rng.choice([2, 4, 6, 8]))
    nrb = int(rng.integers(1, min(grid_prb, max_rb or grid_prb) + 1))
    rb0 = int(rng.integers(0, grid_prb - nrb + 1))
    start = int(rng.integers(0, 3))
    nsym = int(rng.integers(3, 15 - start))
    mask = 0
    for s in range(start, start + nsym):
        if rng.random() < 0.2:
            mask |= 1 << s
    t2 = int(rng.integers(0, 2))
    cdm = int(rng.integers(1, 4 if t2 else 3))
    cfg = dict(rnti=int(rng.integers(1, 65536)), n_id=int(rng.integers(0, 1024)), qm=q, nof_layers=L, nof_rx_ports=P,
               start_symbol=start, nof_symbols=nsym, dmrs_symbol_mask=mask, dmrs_type2=t2,
               nof_cdm_groups_without_data=cdm, rb_start=rb0, nof_rb=nrb)
    nsc = 12 * grid_prb
    H = (rng.normal(size=(L, P, 14, nsc)) + 1j * rng.normal(size=(L, P, 14, nsc))) / np.sqrt(2)
    snr = float(snr_db if snr_db is not None else rng.uniform(5, 30))
    nv = (10 ** (-snr / 10) * rng.uniform(0.5, 1.5, P)).astype(np.float32)
    lv = np.arange(-(2 ** (q // 2) - 1), 2 ** (q // 2), 2) * QAM_AMP[q]
    x = rng.choice(lv, (L, 14, nsc)) + 1j * rng.choice(lv, (L, 14, nsc))
    Hq = from_bf16(bf16(H))
    y = np.einsum("lpsk,lsk->psk", Hq, x)
    y += (rng.normal(size=y.shape) + 1j * rng.normal(size=y.shape)) * np.sqrt(nv[:, None, None] / 2)
    return cfg, bf16(y), bf16(H), nv


def valid_tp_prbs(limit):
    """PRB counts a transform-precoded allocation may take (TS 38.211 section 6.3.1.4: 2^a 3^b 5^c)."""
    out = []
    for n in range(1, limit + 1):
        m = n
        for f in (2, 3, 5):
            while m % f == 0:
                m //= f
        if m == 1:
            out.append(n)
    return out


def random_general_case(rng, grid_prb, transform_precoding=False, mask=True, nof_rx_ports=None, qm=None,
                        snr_db=None, max_rb=None):
    """random_case with a general CRB mask (RBG runs or scattered CRBs; with transform precoding, a PRB count the DFT
    supports and DM-RS symbols without data). Returns (cfg, grid, ch_est, noise_var, crb_mask or None)."""
    cfg, grid, H, nv = random_case(rng, grid_prb, nof_layers=1 if transform_precoding else None,
                                   nof_rx_ports=nof_rx_ports, qm=qm, snr_db=snr_db, max_rb=max_rb)
    lim = min(grid_prb, max_rb or grid_prb)
    crb = None
    if transform_precoding:
        cfg["dmrs_type2"], cfg["nof_cdm_groups_without_data"] = 0, 2
        nrb = int(rng.choice(valid_tp_prbs(lim)))
    else:
        nrb = int(rng.integers(1, lim + 1))
    if mask:
        crb = np.zeros(grid_prb, np.uint8)
        crb[rng.choice(grid_prb, nrb, replace=False)] = 1
        rbs = np.flatnonzero(crb)
        cfg["rb_start"], cfg["nof_rb"] = int(rbs[0]), nrb
    else:
        cfg["rb_start"], cfg["nof_rb"] = int(rng.integers(0, grid_prb - nrb + 1)), nrb
    return cfg, grid, H, nv, crb


# ----------------------------------------------------------------------------------------------------------------------
# Multi-layer MMSE cases (the extension: held to the float64 restatement D.equalize_mmse only).
# ----------------------------------------------------------------------------------------------------------------------

# SNR per modulation at which most max-log LLRs are neither 0 nor clipped at +-120, so that a wrong scale, noise
# variance or unbiasing factor shows (at 25 dB half to all of them sit at +-120). For L = P; see mmse_case.
MMSE_SNR_DB = {2: 6.0, 4: 10.0, 6: 12.0, 8: 15.0}
BF16_NAN, BF16_1E30 = 0x7FC0, 0x714A


def informative_share(llrs):
    """Share of the LLRs that are neither 0 nor saturated."""
    a = np.abs(np.asarray(llrs).astype(np.int16))
    return float(np.mean((a != 0) & (a != D.LLR_MAX)))


def bounded_channel(rng, L, P, shape):
    """Per RE H = U diag(s) V^H with orthonormal U (P x L), unitary V (L x L) and singular values s in [0.5, 1.5]
    (condition number <= 3). Returns (L, P) + shape."""
    n = int(np.prod(shape))
    q, _ = np.linalg.qr(rng.normal(size=(n, P, L)) + 1j * rng.normal(size=(n, P, L)))
    v, _ = np.linalg.qr(rng.normal(size=(n, L, L)) + 1j * rng.normal(size=(n, L, L)))
    s = rng.uniform(0.5, 1.5, (n, 1, L))
    m = (q * s) @ np.conj(np.transpose(v, (0, 2, 1)))  # (n, P, L)
    return np.transpose(m, (2, 1, 0)).reshape((L, P) + tuple(shape))


def mmse_case(rng, grid_prb, L, P, qm, snr_db=None, bounded=False, garbage=None, nof_rb=None, dead_layer=None,
              scattered=False):
    """A transmission over all 14 symbols with one DM-RS symbol (random position, type and CDM groups), at the SNR of
    its modulation, already in the plan's slot layout: returns (cfg, grid (4, 14, nsc, 2) bf16, ch_est (4, 4, 14,
    nsc, 2) bf16, noise_var (4,) float32, crb_mask or None).

    bounded: bounded_channel instead of i.i.d. Gaussian entries. garbage "nan" / "big": the unused ports of the grid,
    the unused ports and layers of the estimates and noise_var[P:] hold bf16 NaN / 1e30 instead of zeros (nothing may
    read them). dead_layer: that layer's channel column is zero on every third subcarrier. scattered: a CRB mask of
    nof_rb scattered CRBs instead of a contiguous allocation."""
    nsc = 12 * grid_prb
    nrb = int(nof_rb or rng.integers(4, grid_prb + 1))
    crb = None
    if scattered:
        crb = np.zeros(grid_prb, np.uint8)
        crb[rng.choice(grid_prb, nrb, replace=False)] = 1
        rb0 = int(np.flatnonzero(crb)[0])
    else:
        rb0 = int(rng.integers(0, grid_prb - nrb + 1))
    t2 = int(rng.integers(0, 2))
    cfg = dict(rnti=int(rng.integers(1, 65536)), n_id=int(rng.integers(0, 1024)), qm=qm, nof_layers=L, nof_rx_ports=P,
               start_symbol=0, nof_symbols=14, dmrs_symbol_mask=1 << int(rng.integers(0, 14)), dmrs_type2=t2,
               nof_cdm_groups_without_data=int(rng.integers(1, 4 if t2 else 3)), rb_start=rb0, nof_rb=nrb)
    if bounded:
        H = bounded_channel(rng, L, P, (14, nsc))
    else:
        H = (rng.normal(size=(L, P, 14, nsc)) + 1j * rng.normal(size=(L, P, 14, nsc))) / np.sqrt(2)
    if dead_layer is not None:
        H[dead_layer, :, :, ::3] = 0
    # With i.i.d. entries the post-equalisation SINR grows with the P - L + 1 diversity order of a linear receiver:
    # taken off the input SNR (a bounded channel has no such gain).
    snr = MMSE_SNR_DB[qm] - (0 if bounded else 10 * np.log10(P - L + 1)) if snr_db is None else snr_db
    nv = (10 ** (-snr / 10) * rng.uniform(0.5, 1.5, P)).astype(np.float32)
    lv = np.arange(-(2 ** (qm // 2) - 1), 2 ** (qm // 2), 2) * QAM_AMP[qm]
    x = rng.choice(lv, (L, 14, nsc)) + 1j * rng.choice(lv, (L, 14, nsc))
    y = np.einsum("lpsk,lsk->psk", from_bf16(bf16(H)), x)
    y += (rng.normal(size=y.shape) + 1j * rng.normal(size=y.shape)) * np.sqrt(nv[:, None, None] / 2)
    fill = {None: 0, "nan": BF16_NAN, "big": BF16_1E30}[garbage]
    g = np.full((4, 14, nsc, 2), fill, np.uint16)
    g[:P] = bf16(y)
    h = np.full((4, 4, 14, nsc, 2), fill, np.uint16)
    h[:L, :P] = bf16(H)
    n4 = np.full(4, {None: 0.0, "nan": np.nan, "big": 1e30}[garbage], np.float32)
    n4[:P] = nv
    return cfg, g, h, n4, crb


def mmse_float32(rx, H, noise_var):
    """The GPU kernel's own sequence in numpy float32, every product and sum rounded separately: Gram matrix A = H^H H
    + nv I, Cholesky A = R^H R, T = R^-1, x = T T^H H^H y, [A^-1]_ll = sum_j |T_lj|^2, unbiasing by g = 1 - nv
    [A^-1]_ll. A measuring aid only (how far float32 alone moves the LLRs from the float64 restatement), never an
    expected value. rx (P, n), H (P, L, n) -> (eq (n, L) complex64, nvar (n, L) float32)."""
    C, F = np.complex64, np.float32
    P, L, n = H.shape
    rx, H = rx.astype(C), H.astype(C)
    nv = F(np.max(np.asarray(noise_var, F)[:P]))
    A = [[None] * L for _ in range(L)]
    m = [None] * L
    for i in range(L):
        A[i][i] = (nv + sum((H[p, i].real ** 2 + H[p, i].imag ** 2).astype(F) for p in range(P))).astype(F)
        for j in range(i + 1, L):
            A[i][j] = sum((np.conj(H[p, i]) * H[p, j]).astype(C) for p in range(P)).astype(C)
        m[i] = sum((np.conj(H[p, i]) * rx[p]).astype(C) for p in range(P)).astype(C)
    R = [[None] * L for _ in range(L)]
    rinv = [None] * L
    with np.errstate(all="ignore"):
        for i in range(L):
            d = A[i][i]
            for k in range(i):
                d = (d - (R[k][i].real ** 2 + R[k][i].imag ** 2).astype(F)).astype(F)
            rinv[i] = (F(1) / np.sqrt(np.maximum(d, F(0)))).astype(F)
            for j in range(i + 1, L):
                s = A[i][j]
                for k in range(i):
                    s = (s - (np.conj(R[k][i]) * R[k][j]).astype(C)).astype(C)
                R[i][j] = (s * rinv[i]).astype(C)
        T = [[None] * L for _ in range(L)]
        for i in range(L):
            T[i][i] = rinv[i].astype(C)
            for j in range(i + 1, L):
                s = (T[i][i] * R[i][j]).astype(C)
                for k in range(i + 1, j):
                    s = (s + (T[i][k] * R[k][j]).astype(C)).astype(C)
                T[i][j] = (s * (-rinv[j])).astype(C)
        z = []
        for j in range(L):
            z.append(sum((np.conj(T[i][j]) * m[i]).astype(C) for i in range(j + 1)).astype(C))
        eq = np.zeros((n, L), C)
        var = np.full((n, L), np.inf, F)
        for i in range(L):
            x = sum((T[i][j] * z[j]).astype(C) for j in range(i, L)).astype(C)
            aii = sum((T[i][j].real ** 2 + T[i][j].imag ** 2).astype(F) for j in range(i, L)).astype(F)
            naii = (nv * aii).astype(F)
            g = (F(1) - naii).astype(F)
            tiny = np.finfo(F).tiny
            ok = np.isfinite(g) & (g >= tiny) & np.isfinite(naii) & (np.abs(naii) >= tiny)
            rg = (F(1) / np.where(ok, g, F(1))).astype(F)
            eq[:, i] = np.where(ok, (x * rg).astype(C), 0)
            var[:, i] = np.where(ok, (naii * rg).astype(F), np.inf)
    return eq, var


MMSE_LP = [(2, 2), (2, 3), (2, 4), (3, 3), (3, 4), (4, 4)]
MMSE_SINGLES = [(L, P, qm) for L, P in MMSE_LP for qm in (2, 4, 6, 8)]
ONE_LAYER_EXTRAS = [(1, 1, 2), (1, 4, 2), (1, 2, 6), (1, 3, 6)]


def mmse_single_case(L, P, qm):
    """The case of one (layers, ports, modulation) instantiation: 4-6 PRB of a 6-PRB grid (one grid size, so that the
    same cases also share a plan), garbage in the unused slots."""
    seed = 1000 + 100 * L + 10 * P + qm
    return mmse_case(np.random.default_rng(seed), 6, L, P, qm, garbage=("nan", "big")[(seed // 2) % 2])


def mmse_wide_case(L, P, qm):
    """A 52-PRB transmission over the whole grid (the large-plan tests repeat a few of these)."""
    return mmse_case(np.random.default_rng(2000 + 10 * L + qm), 52, L, P, qm, nof_rb=52, garbage="nan")


# (layers, ports, modulation) of the large plans: L Qm in {24, 32} (chunks of <= 384 REs: 64 lanes) and in {12, 16, 18}
# (<= 768 REs: 128 lanes).
MMSE_WIDE_64 = [(3, 4, 8), (4, 4, 6), (4, 4, 8)]
MMSE_WIDE_128 = [(2, 2, 6), (3, 3, 4), (4, 4, 4), (2, 4, 8), (3, 4, 6)]


def mmse_crb_cases():
    """2-4 layers over scattered CRBs of a 24-PRB grid."""
    rng = np.random.default_rng(300)
    for L, P, qm in [(2, 3, 6), (3, 4, 2), (4, 4, 8)]:
        yield (L, P, qm), mmse_case(rng, 24, L, P, qm, nof_rb=int(rng.integers(5, 12)), scattered=True, garbage="nan")


def mmse_stats_cases():
    """2-4 layers x two modulations on bounded-condition channels (the statistics comparison: the mean noise variance
    of an i.i.d. channel is dominated by its few near-singular REs)."""
    rng = np.random.default_rng(400)
    for L, P in [(2, 2), (3, 4), (4, 4)]:
        for qm in (4, 6):
            yield (L, P, qm), mmse_case(rng, 6, L, P, qm, bounded=True)


# Share of the LLRs that float32 arithmetic alone (mmse_float32) moves by one step from the float64 restatement, worst
# case over every multi-layer case of the GPU suite (measured: 7.9e-5; test_pusch_demod_mmse_oracle.py re-measures).
# The GPU tolerance is ten times that (the kernel's 1-ulp v_rsq / v_rcp and its FMA contraction are not in numpy),
# floored at 1e-3.
MMSE_FLOAT32_SHARE = 1e-4
MMSE_SHARE_BOUND = max(10 * MMSE_FLOAT32_SHARE, 1e-3)


def demodulate_with(equalizer, cfg, grid, ch_est, noise_var, crb_mask=None):
    """D.demodulate with `equalizer(rx, H, noise_var) -> (eq, nvar)` in place of the restatement's (mmse_float32, or
    a perturbed restatement that a test must tell from the right one)."""
    res = D.data_res_mask(cfg["start_symbol"], cfg["nof_symbols"], cfg["dmrs_symbol_mask"], cfg["dmrs_type2"],
                          cfg["nof_cdm_groups_without_data"], D.allocated_rbs(cfg["rb_start"], cfg["nof_rb"], crb_mask))
    sym = np.array([r[0] for r in res])
    sc = np.array([r[1] for r in res])
    P, L = cfg["nof_rx_ports"], cfg["nof_layers"]
    e, v = equalizer(grid[:P, sym, sc], np.transpose(ch_est[:L, :P, sym, sc], (1, 0, 2)), noise_var)
    llr = D.demap(e.astype(np.complex64).reshape(-1), v.astype(np.float32).reshape(-1), cfg["qm"]).astype(np.int16)
    c = D.gold_sequence(cfg["rnti"] * (1 << 15) + cfg["n_id"], llr.size)
    return np.where(c == 1, -llr, llr).astype(np.int8)


# ----------------------------------------------------------------------------------------------------------------------
# The reference's own paths (ZF 1 x N, ZF 2 x N, one-layer MMSE, transform precoding) held to the restatement
# (D.equalize, D.transform_deprecode) at a tolerance derived from rounding.
# ----------------------------------------------------------------------------------------------------------------------

# Share of the LLRs that rounding alone moves by one step over the cases of the GPU suite: D.equalize (float32)
# against the same formulas in float64 (zf_equalize; measured: 1.0e-5 in the worst case, one LLR of the 97 344 of a
# 52-PRB transmission) and the kernel's inverse DFT restated in float32 (tp_float32) against D.transform_deprecode's
# complex128 one (measured: 2.9e-6 over the 53 sizes taken together, one LLR of 342 240; none on the extras);
# tests/test_pusch_demod_reference_paths_oracle.py re-measures both. The GPU tolerance follows the rule of the MMSE
# tests: ten times that (1-ulp hardware reciprocals and FMA contraction are not in numpy), floored at 1e-3.
REF_PATHS_FLOAT32_SHARE = 1e-4
REF_PATHS_SHARE_BOUND = max(10 * REF_PATHS_FLOAT32_SHARE, 1e-3)

REF_LP = [(1, 1), (1, 2), (1, 3), (1, 4), (2, 2), (2, 4)]
REF_SINGLES = [(L, P, qm) for L, P in REF_LP for qm in (2, 4, 6, 8)]


def zf_equalize(rx, H, noise_var, real=np.float32, variance="weighted", nv2="max"):
    """The formulas of D.equalize (ZF 1 x N, ZF 2 x N) evaluated in `real` arithmetic: np.float32 gives D.equalize bit
    for bit (the CPU tests assert it), np.float64 what rounding is measured against. The validity rules stay those of
    float32 numbers. Two hand-made errors for the perturbation tests: variance="max" takes the one-layer variance as
    max(nv) / sum |h|^2 instead of the weighted sum, nv2="mean" the two-layer noise variance as the mean over the
    ports instead of the largest."""
    cplx = np.complex64 if real == np.float32 else np.complex128
    P, L, n = H.shape
    nv = np.asarray(noise_var, np.float32)[:P]
    nvr = nv.astype(real)
    rx, H = rx.astype(cplx), H.astype(cplx)
    isn = D._isnormal
    with np.errstate(all="ignore"):
        if L == 1:
            ch, acc, out = np.zeros(n, real), np.zeros(n, real), np.zeros(n, cplx)
            for p in range(P):
                h = H[p, 0]
                norm = h.real * h.real + h.imag * h.imag
                ok = isn(norm) & bool(isn(nv[p]) and nv[p] > 0)
                ch = np.where(ok, ch + norm, ch)
                acc = np.where(ok, acc + norm * nvr[p], acc)
                out = np.where(ok, out + rx[p] * np.conj(h), out)
            good = isn(ch) & isn(acc)
            rcp = real(1) / np.where(good, ch, real(1))
            var = acc * rcp * rcp if variance == "weighted" else nvr.max() * rcp
            return np.where(good, out * rcp, 0)[:, None], np.where(good, var, np.inf)[:, None]
        assert L == 2 and P in (2, 4)
        nve = nvr.max() if nv2 == "max" else nvr.mean(dtype=real)
        if not (isn(nve) and nve >= 0):
            return np.zeros((n, 2), cplx), np.full((n, 2), np.inf, real)
        norm = [np.sum([H[p, l].real ** 2 + H[p, l].imag ** 2 for p in range(P)], axis=0) for l in range(2)]
        xi = np.sum([np.conj(H[p, 0]) * H[p, 1] for p in range(P)], axis=0)
        xi_mod_sq = xi.real * xi.real + xi.imag * xi.imag
        mi = [np.sum([np.conj(H[p, l]) * rx[p] for p in range(P)], axis=0) for l in range(2)]
        d_pinv = norm[0] * norm[1] - xi_mod_sq
        good = isn(d_pinv)
        rcp = real(1) / np.where(good, d_pinv, real(1))
        e0 = (norm[1] * mi[0] - xi * mi[1]) * rcp
        e1 = (norm[0] * mi[1] - np.conj(xi) * mi[0]) * rcp
        n0, n1 = nve * norm[1] * rcp, nve * norm[0] * rcp
        return (np.stack([np.where(good, e0, 0), np.where(good, e1, 0)], axis=1),
                np.stack([np.where(good, n0, np.inf), np.where(good, n1, np.inf)], axis=1))


def ref_single_case(L, P, qm):
    """The case of one instantiation of the reference's equalisers: 4-6 PRB of a 6-PRB grid over 14 symbols, garbage
    in the unused slots."""
    seed = 3000 + 100 * L + 10 * P + qm
    return mmse_case(np.random.default_rng(seed), 6, L, P, qm, garbage=("nan", "big")[(seed // 2) % 2])


def ref_wide_case(L, P, qm):
    """A 52-PRB transmission over the whole grid (the large-plan tests repeat a few of these)."""
    return mmse_case(np.random.default_rng(4000 + 100 * L + 10 * P + qm), 52, L, P, qm, nof_rb=52, garbage="nan")


# (layers, ports, modulation) of the large plans: one layer with L Qm in {2, 4, 6, 8} (chunks of 8192 LLRs hold more
# than 768 REs: 256 lanes, four or more REs each: the bench's ref profile) and two-layer ZF with L Qm in {12, 16}
# (<= 768 REs: 128 lanes).
REF_WIDE_256 = [(1, 1, 2), (1, 2, 4), (1, 3, 6), (1, 4, 8)]
REF_WIDE_128 = [(2, 2, 6), (2, 4, 8), (2, 4, 6)]


def tp_radix_sequence(m):
    """The radices of the kernel's Stockham passes over m points, in its order: 4 while divisible, then 2, 3, 5."""
    seq = []
    while m > 1:
        r = 4 if m % 4 == 0 else 2 if m % 2 == 0 else 3 if m % 3 == 0 else 5
        assert m % r == 0, "not a 2^a 3^b 5^c size"
        seq.append(r)
        m //= r
    return tuple(seq)


def tp_case(rng, grid_prb, nof_rb, qm, P, garbage=None, dead=False, rb_start=None, start_symbol=0, nof_symbols=1,
            dmrs_symbol_mask=0, scattered=False, slot=None, big_every_third=False):
    """A transform-precoded (DFT-s-OFDM) transmission in the plan's slot layout, same return as mmse_case: per data
    symbol M = 12 nof_rb QAM symbols spread by a unitary forward DFT, through an i.i.d. per-RE channel (bf16-rounded)
    on P ports, plus noise at MMSE_SNR_DB[qm] less the 10 log10 P diversity gain of the one-layer combiner. DM-RS
    symbols are type 1 with two CDM groups without data (no data RE: nothing of them is read).

    garbage: as mmse_case. dead: the channel of every port is zero on every third subcarrier of the allocation
    (infinite variance there: class TP_INF next to TP_VALID). big_every_third: the channel there is 2^40 instead, with
    which a noise variance of 1e-24 gives an equalised variance that underflows to zero (class TP_OTHER). scattered:
    a CRB mask of nof_rb scattered CRBs. slot: (grid, ch_est) of a slot shared with other transmissions, written only
    at this transmission's ports, data symbols and subcarriers."""
    nsc = 12 * grid_prb
    fill = {None: 0, "nan": BF16_NAN, "big": BF16_1E30}[garbage]
    g, h = slot if slot is not None else (np.full((4, 14, nsc, 2), fill, np.uint16),
                                          np.full((4, 4, 14, nsc, 2), fill, np.uint16))
    crb = None
    if scattered:
        crb = np.zeros(grid_prb, np.uint8)
        crb[rng.choice(grid_prb, nof_rb, replace=False)] = 1
        rb0 = int(np.flatnonzero(crb)[0])
    else:
        rb0 = int(rng.integers(0, grid_prb - nof_rb + 1)) if rb_start is None else rb_start
    cfg = dict(rnti=int(rng.integers(1, 65536)), n_id=int(rng.integers(0, 1024)), qm=qm, nof_layers=1, nof_rx_ports=P,
               start_symbol=start_symbol, nof_symbols=nof_symbols, dmrs_symbol_mask=dmrs_symbol_mask, dmrs_type2=0,
               nof_cdm_groups_without_data=2, rb_start=rb0, nof_rb=nof_rb)
    sc = (12 * np.array(D.allocated_rbs(rb0, nof_rb, crb))[:, None] + np.arange(12)).reshape(-1)
    m = sc.size
    snr = MMSE_SNR_DB[qm] - 10 * np.log10(P)
    nv = (10 ** (-snr / 10) * rng.uniform(0.5, 1.5, P)).astype(np.float32)
    lv = np.arange(-(2 ** (qm // 2) - 1), 2 ** (qm // 2), 2) * QAM_AMP[qm]
    h0 = h[0]
    for l in range(start_symbol, start_symbol + nof_symbols):
        if (dmrs_symbol_mask >> l) & 1:
            continue
        x = np.fft.fft(rng.choice(lv, m) + 1j * rng.choice(lv, m)) / np.sqrt(m)
        H = (rng.normal(size=(P, m)) + 1j * rng.normal(size=(P, m))) / np.sqrt(2)
        if dead:
            H[:, ::3] = 0
        if big_every_third:
            H[:, ::3] = 2.0 ** 40
        y = from_bf16(bf16(H)) * x
        y += (rng.normal(size=y.shape) + 1j * rng.normal(size=y.shape)) * np.sqrt(nv[:, None] / 2)
        g[:P, l, sc] = bf16(y)
        h0[:P, l, sc] = bf16(H)
    n4 = np.full(4, {None: 0.0, "nan": np.nan, "big": 1e30}[garbage], np.float32)
    n4[:P] = nv
    return cfg, g, h, n4, crb


def _f32_cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def _f32_small_idft(r, vr, vi):
    """The kernel's small_idft<R> on float32 arrays, every product and sum rounded separately."""
    f = np.float32
    if r == 2:
        return [vr[0] + vr[1], vr[0] - vr[1]], [vi[0] + vi[1], vi[0] - vi[1]]
    if r == 4:
        ar, ai, br, bi = vr[0] + vr[2], vi[0] + vi[2], vr[0] - vr[2], vi[0] - vi[2]
        cr, ci, dr, di = vr[1] + vr[3], vi[1] + vi[3], vr[1] - vr[3], vi[1] - vi[3]
        return [ar + cr, br - di, ar - cr, br + di], [ai + ci, bi + dr, ai - ci, bi - dr]
    if r == 3:
        c1, s1 = f(-0.5), f(0.866025404)
        tr, ti, dr, di = vr[1] + vr[2], vi[1] + vi[2], vr[1] - vr[2], vi[1] - vi[2]
        mr, mi = vr[0] + c1 * tr, vi[0] + c1 * ti
        jr, ji = -s1 * di, s1 * dr
        return [vr[0] + tr, mr + jr, mr - jr], [vi[0] + ti, mi + ji, mi - ji]
    c1, s1, c2, s2 = f(0.309016994), f(0.951056516), f(-0.809016994), f(0.587785252)
    t1r, t1i, d1r, d1i = vr[1] + vr[4], vi[1] + vi[4], vr[1] - vr[4], vi[1] - vi[4]
    t2r, t2i, d2r, d2i = vr[2] + vr[3], vi[2] + vi[3], vr[2] - vr[3], vi[2] - vi[3]
    m1r, m1i = vr[0] + c1 * t1r + c2 * t2r, vi[0] + c1 * t1i + c2 * t2i
    m2r, m2i = vr[0] + c2 * t1r + c1 * t2r, vi[0] + c2 * t1i + c1 * t2i
    n1r, n1i = s1 * d1r + s2 * d2r, s1 * d1i + s2 * d2i
    n2r, n2i = s2 * d1r - s1 * d2r, s2 * d1i - s1 * d2i
    return ([vr[0] + (t1r + t2r), m1r - n1i, m2r - n2i, m2r + n2i, m1r + n1i],
            [vi[0] + (t1i + t2i), m1i + n1r, m2i + n2r, m2i - n2r, m1i - n1r])


def _f32_block_mean(v, valid, threads=256):
    """The kernel's mean of the valid variances in float32: lane t sums its REs t, t + 256, ... in order, the 64 lanes
    of a wave an xor butterfly (offsets 32 .. 1), the four waves in order."""
    f = np.float32
    rows = -(-v.size // threads)
    a = np.zeros((2, rows * threads), f)
    a[0, :v.size] = np.where(valid, v, 0)
    a[1, :v.size] = valid
    acc = np.zeros((2, threads), f)
    for row in a.reshape(2, rows, threads).transpose(1, 0, 2):
        acc = acc + row
    acc = acc.reshape(2, threads // 64, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lane ^ off]
    tot = np.zeros(2, f)
    for w in range(threads // 64):
        tot = tot + acc[:, w, 0]
    return tot[0] / tot[1] if tot[1] > 0 else f(0)


def tp_float32(eq, nvar):
    """The transform-precoding kernel's own sequence in numpy float32, in place of D.transform_deprecode: Stockham
    passes with the radices in the kernel's order (tp_radix_sequence), twiddles from the float32 sin(pi x) / cos(pi x)
    of x = 2 r k / (Ns R) rounded to float32, every product and sum rounded separately, the 1 / sqrt(M) scale and the
    mean of the valid variances in float32 in the kernel's order. A measuring aid only (how far float32 alone moves
    the LLRs from the restatement), never an expected value."""
    f = np.float32
    m = eq.size
    sr, si = np.asarray(eq.real, f).copy(), np.asarray(eq.imag, f).copy()
    ns = 1
    with np.errstate(all="ignore"):
        for r in tp_radix_sequence(m):
            stride = m // r
            j = np.arange(stride)
            k = j % ns
            vr, vi = [sr[j]], [si[j]]
            for t in range(1, r):
                x = (f(2) * (t * k).astype(f) / f(ns * r)).astype(f)
                cs, sn = np.cos(np.pi * x.astype(np.float64)).astype(f), np.sin(np.pi * x.astype(np.float64)).astype(f)
                a, b = _f32_cmul(sr[j + t * stride], si[j + t * stride], cs, sn)
                tw = k != 0  # the kernel multiplies only where k != 0
                vr.append(np.where(tw, a, sr[j + t * stride]))
                vi.append(np.where(tw, b, si[j + t * stride]))
            vr, vi = _f32_small_idft(r, vr, vi)
            dr, di = np.empty(m, f), np.empty(m, f)
            o = (j // ns) * ns * r + k
            for t in range(r):
                dr[o + t * ns], di[o + t * ns] = vr[t], vi[t]
            sr, si, ns = dr, di, ns * r
        scale = f(1) / np.sqrt(f(m))
        v = np.asarray(nvar, f)
        valid = (v > 0) & np.isfinite(v)
        mean = _f32_block_mean(v, valid)
    return ((sr * scale) + 1j * (si * scale)).astype(np.complex64), np.where(valid, mean, v).astype(f)


def tp_demodulate_with(deprecode, cfg, grid, ch_est, noise_var, crb_mask=None, equalizer=D.equalize):
    """D.demodulate_ex's transform-precoded LLRs with `deprecode(eq, nvar) -> (symbols, variances)` in place of
    D.transform_deprecode (tp_float32, or a perturbed restatement that a test must tell from the right one) and,
    optionally, another one-layer equaliser."""
    rbs = D.allocated_rbs(cfg["rb_start"], cfg["nof_rb"], crb_mask)
    P = cfg["nof_rx_ports"]
    llrs = []
    for l in range(cfg["start_symbol"], cfg["start_symbol"] + cfg["nof_symbols"]):
        res = D.data_res_mask(l, 1, cfg["dmrs_symbol_mask"], cfg["dmrs_type2"], cfg["nof_cdm_groups_without_data"], rbs)
        if not res:
            continue
        sc = np.array([r[1] for r in res])
        e, v = equalizer(grid[:P, l, sc], np.transpose(ch_est[:1, :P, l, sc], (1, 0, 2)), noise_var)
        x, xv = deprecode(e.reshape(-1).astype(np.complex64), v.reshape(-1).astype(np.float32))
        llrs.append(D.demap(np.asarray(x, np.complex64), np.asarray(xv, np.float32), cfg["qm"]))
    llr = np.concatenate(llrs).astype(np.int16)
    c = D.gold_sequence(cfg["rnti"] * (1 << 15) + cfg["n_id"], llr.size)
    return np.where(c == 1, -llr, llr).astype(np.int8)


TP_GRID_PRB = 273
_tp_plan = []


def tp_size_plan():
    """Every valid transform-precoding size in ONE plan over a 273-PRB grid: the 53 M_RB = 2^a 3^b 5^c <= 273, the
    modulation rotating over them, plus the three other modulations at M_RB = 1 and at M_RB = 270 (M = 3240 = 4 2 3 3
    3 3 5: every pass kind), the ports rotating over 1 .. 4. Each is one data symbol, alone (empty DM-RS mask) or after
    / before a DM-RS symbol without data; the transmissions are packed first-fit at distinct (symbols, rb_start) of a
    few shared slots filled with bf16 NaN, which every unused port keeps. Built once.

    Returns (keys [(M_RB, qm, P)], cases [(cfg, grid, ch_est, noise_var (4,), None)], grid_index, slots [(grid,
    ch_est)])."""
    if _tp_plan:
        return _tp_plan[0]
    rng = np.random.default_rng(5300)
    sizes = valid_tp_prbs(TP_GRID_PRB)
    keys = [(n, (2, 4, 6, 8)[i % 4], 1 + (i // 2) % 4) for i, n in enumerate(sizes)]
    for n in (1, 270):
        have = next(q for m, q, _ in keys if m == n)
        keys += [(n, q, 1 + (q // 2 + n) % 4) for q in (2, 4, 6, 8) if q != have]
    nsc = 12 * TP_GRID_PRB
    slots, rows, place = [], [], []  # rows: [slot, first symbol, symbols, PRBs used]
    for i, (n, _, _) in enumerate(keys):
        nsym = 1 + i % 2
        row = next((r for r in rows if r[2] == nsym and r[3] + n <= TP_GRID_PRB), None)
        if row is None:
            first = rows[-1][1] + rows[-1][2] if rows else 0
            slot = rows[-1][0] if rows else 0
            if first + nsym > 14:
                slot, first = slot + 1, 0
            row = [slot, first, nsym, 0]
            rows.append(row)
        place.append((row[0], row[1], row[3]))
        row[3] += n
    for _ in range(rows[-1][0] + 1):
        slots.append((np.full((4, 14, nsc, 2), BF16_NAN, np.uint16), np.full((4, 4, 14, nsc, 2), BF16_NAN, np.uint16)))
    cases = []
    for i, ((n, qm, P), (slot, first, rb0)) in enumerate(zip(keys, place)):
        nsym = 1 + i % 2
        mask = 0 if nsym == 1 else 1 << (first + (i // 2) % 2)  # the DM-RS symbol before or after the data symbol
        cases.append(tp_case(rng, TP_GRID_PRB, n, qm, P, garbage="nan", rb_start=rb0, start_symbol=first,
                             nof_symbols=nsym, dmrs_symbol_mask=mask, slot=slots[slot]))
    _tp_plan.append((keys, cases, [p[0] for p in place], slots))
    return _tp_plan[0]


def tp_extra_cases():
    """Transform precoding beyond one contiguous symbol: scattered CRB masks (M_RB = 5, 27, 100), 14 symbols with two
    DM-RS symbols at M_RB = 48 (sym_cum offsets, descrambling positions across word boundaries), the `dead` case
    (classes TP_INF and TP_VALID in one symbol) and a zero noise variance (no valid variance: mean 0, every LLR 0), on
    a 106-PRB grid. Yields (name, case)."""
    rng = np.random.default_rng(5400)
    for n, qm, P in [(5, 4, 3), (27, 8, 2), (100, 6, 4)]:
        start = int(rng.integers(0, 13))
        yield f"crb{n}", tp_case(rng, 106, n, qm, P, garbage="big", scattered=True, start_symbol=start, nof_symbols=2)
    yield "multi", tp_case(rng, 106, 48, 6, 2, garbage="nan", nof_symbols=14, dmrs_symbol_mask=(1 << 2) | (1 << 11))
    yield "dead", tp_case(rng, 106, 20, 4, 2, garbage="nan", dead=True, nof_symbols=2)
    cfg, g, h, nv, crb = tp_case(rng, 106, 9, 6, 3, garbage="big", nof_symbols=2)
    nv[:3] = 0
    yield "zero", (cfg, g, h, nv, crb)
    # Class TP_OTHER next to TP_VALID: on every third subcarrier |h|^2 = 2^80 and nv = 1e-24, so that the equalised
    # variance nv / |h|^2 = 8e-49 underflows to zero, denormals kept or not (zero is kept: LLRs 0); the others' (about
    # 1e-24) are valid normal numbers.
    cfg, g, h, nv, crb = tp_case(rng, 106, 6, 2, 1, garbage="nan", big_every_third=True, nof_symbols=2)
    nv[:1] = 1e-24
    yield "other", (cfg, g, h, nv, crb)
