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
