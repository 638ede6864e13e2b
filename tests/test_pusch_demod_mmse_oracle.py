"""The float64 restatement of 2-4 layer MMSE equalisation (oracle/pusch_demod_oracle.py equalize_mmse) checked on its
own, without the kernel: it is unbiased, its variance is 1 / SINR by a formula that shares no inverse with it, it tends
to the reference's ZF 2 x N path as the noise vanishes, it reads the first P noise variances only, it follows the
project's validity rule, and its batched inverse is the per-RE one. The GPU tests then hold the kernel to it
(tests/test_pusch_demodulator_gpu.py, test_pusch_demod_mmse_*), on cases whose LLRs this file shows to be informative
and within the float32 share the tolerance is derived from."""
import numpy as np
import pytest

import pusch_demod_cases as K
import pusch_demod_oracle as D
from pusch_demod_cases import from_bf16

LP = [(1, 1), (1, 4), (2, 2), (2, 3), (2, 4), (3, 3), (3, 4), (4, 4)]


def gauss(rng, *shape):
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)) / np.sqrt(2)


@pytest.mark.parametrize("L,P", LP)
def test_unbiased(L, P):
    """y = H e_l, noise-free: layer l comes back as exactly 1, whatever the noise variance the equaliser is told."""
    rng = np.random.default_rng(10 * L + P)
    n = 300
    H = gauss(rng, P, L, n)
    for nv in (1e-3, 0.1, 1.0):
        for l in range(L):
            eq, _ = D.equalize_mmse(H[:, l, :], H, np.full(P, nv))
            assert np.max(np.abs(eq[:, l] - 1)) < 1e-12, (nv, l)


@pytest.mark.parametrize("L,P", LP)
def test_variance_is_inverse_sinr(L, P):
    """nvar_l h_l^H (H_-l H_-l^H + nv I)^-1 h_l == 1: the SINR of the MMSE receiver from the P x P interference-plus-
    noise covariance, not from the L x L inverse the restatement takes. Both sides lose cond(A) x 2^-53, so the
    1e-12 holds where cond(A) stays below a few hundred: i.i.d. channels at nv >= 0.1 (cond <= (lambda_max + nv) /
    nv), bounded-condition channels (cond <= 9) at nv = 1e-3."""
    rng = np.random.default_rng(100 + 10 * L + P)
    n = 300
    for nv in (1e-3, 0.1, 1.0):
        H = K.bounded_channel(rng, L, P, (n,)).transpose(1, 0, 2) if nv < 0.1 else gauss(rng, P, L, n)
        _, var = D.equalize_mmse(gauss(rng, P, n), H, np.full(P, nv))
        for i in range(n):
            h = H[:, :, i]
            for l in range(L):
                ho = np.delete(h, l, axis=1)
                sinr = np.real(h[:, l].conj() @ np.linalg.solve(ho @ ho.conj().T + nv * np.eye(P), h[:, l]))
                assert abs(var[i, l] * sinr - 1) < 1e-12, (nv, i, l)


@pytest.mark.parametrize("P", [2, 4])
def test_zero_forcing_limit(P):
    """Two layers, nv -> 1e-9: the restatement of the reference's ZF 2 x N path (float32), symbols within 1e-5 and
    nvar / nv within 1e-5 relative."""
    rng = np.random.default_rng(200 + P)
    n = 300
    H = K.bounded_channel(rng, 2, P, (n,)).transpose(1, 0, 2)  # (P, L, n)
    rx = np.einsum("pln,ln->pn", H, gauss(rng, 2, n))
    nv = np.full(P, 1e-9)
    eq, var = D.equalize_mmse(rx, H, nv)
    zeq, zvar = D.equalize(rx, H, nv, mmse=False)
    assert np.max(np.abs(eq - zeq)) < 1e-5
    np.testing.assert_allclose(var / 1e-9, zvar.astype(np.float64) / 1e-9, rtol=1e-5)


@pytest.mark.parametrize("L,P", [(2, 2), (2, 3), (3, 4), (4, 4)])
def test_noise_variance_is_the_maximum_over_the_ports(L, P):
    """Any order of the P noise variances gives the same result as their maximum on every port, and entries past the
    first P (NaN, 1e30) change nothing."""
    rng = np.random.default_rng(300 + 10 * L + P)
    n = 100
    H, rx = gauss(rng, P, L, n), gauss(rng, P, n)
    nv = rng.uniform(0.01, 0.1, P)
    want = D.equalize_mmse(rx, H, np.full(P, nv.max()))
    for _ in range(4):
        got = D.equalize_mmse(rx, H, rng.permutation(nv))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for junk in (np.nan, 1e30):
        got = D.equalize_mmse(rx, H, np.concatenate([nv, np.full(4 - P, junk)]))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def loop_mmse(rx, H, nv):
    """equalize_mmse RE by RE, as first written."""
    P, L, n = H.shape
    eq, var = np.zeros((n, L), np.complex128), np.zeros((n, L))
    for i in range(n):
        h = H[:, :, i].astype(np.complex128)
        Ai = np.linalg.inv(h.conj().T @ h + nv * np.eye(L))
        g = 1 - nv * np.real(np.diag(Ai))
        eq[i] = Ai @ (h.conj().T @ rx[:, i].astype(np.complex128)) / g
        var[i] = nv * np.real(np.diag(Ai)) / g
    return eq, var


@pytest.mark.parametrize("L,P", [(2, 2), (3, 4), (4, 4)])
def test_batched_inverse_is_the_loop(L, P):
    rng = np.random.default_rng(400 + 10 * L + P)
    H, rx = gauss(rng, P, L, 200), gauss(rng, P, 200)
    eq, var = D.equalize_mmse(rx, H, np.full(P, 0.05))
    leq, lvar = loop_mmse(rx, H, 0.05)
    assert np.max(np.abs(eq - leq)) < 1e-12 and np.max(np.abs(var / lvar - 1)) < 1e-12


@pytest.mark.parametrize("L,P", [(2, 2), (2, 4), (3, 3), (4, 4)])
def test_validity_rule_zero_noise(L, P):
    """noise_var = 0: nv [A^-1]_ll is not a normal positive number, so every symbol is 0 with an infinite variance and
    every LLR is 0; the statistics have no NaN where there is data (SINR +inf: no finite variance)."""
    cfg, g, h, nv, _ = K.mmse_case(np.random.default_rng(500 + L + P), 4, L, P, 4)
    zero = np.zeros(4, np.float32)
    eq, var = D.equalize_mmse(from_bf16(g)[:P, 0], np.transpose(from_bf16(h)[:L, :P, 0], (1, 0, 2)), zero)
    assert np.all(eq == 0) and np.all(np.isinf(var))
    llr, stats = D.demodulate_ex(cfg, from_bf16(g), from_bf16(h), zero, mmse=True)
    assert llr.size and not llr.any()
    assert not np.isnan(stats[14]).any() and np.isinf(stats[14, 0])


@pytest.mark.parametrize("L,P,dead", [(2, 2, 1), (3, 4, 0), (4, 4, 2)])
def test_validity_rule_dead_layer(L, P, dead):
    """A layer whose channel column is zero on every third subcarrier: its LLRs are 0 there, nothing is NaN or
    infinite, the statistics have no NaN where there is data, and the other REs are what they are without the dead
    ones (the equaliser works RE by RE)."""
    cfg, g, h, nv, _ = K.mmse_case(np.random.default_rng(600 + L + P), 4, L, P, 4, dead_layer=dead)
    llr, stats = D.demodulate_ex(cfg, from_bf16(g), from_bf16(h), nv, mmse=True)
    assert np.array_equal(llr, D.demodulate(cfg, from_bf16(g), from_bf16(h), nv, mmse=True))
    res = D.data_res(0, 14, cfg["dmrs_symbol_mask"], cfg["dmrs_type2"], cfg["nof_cdm_groups_without_data"],
                     cfg["rb_start"], cfg["nof_rb"])
    is_dead = np.array([k % 3 == 0 for _, k in res])
    per = llr.reshape(len(res), L, 4)
    assert is_dead.any() and not per[is_dead, dead].any()
    assert per[~is_dead, dead].any() and K.informative_share(per[~is_dead]) > 0.6
    rows = [l for l in range(14) if not np.isnan(stats[l, 1])]
    assert len(rows) >= 13 and not np.isnan(stats[rows]).any() and not np.isnan(stats[14]).any()


def all_gpu_cases():
    """Every case the GPU tests hold the kernel to (their builders, their seeds)."""
    for L, P, qm in K.MMSE_SINGLES:
        yield (L, P, qm, "single"), K.mmse_single_case(L, P, qm)
    for key, case in K.mmse_crb_cases():
        yield key + ("crb",), case
    for key, case in K.mmse_stats_cases():
        yield key + ("stats",), case
    for key in K.MMSE_WIDE_64 + K.MMSE_WIDE_128:
        yield key + ("wide",), K.mmse_wide_case(*key)


def test_gpu_cases_are_informative_and_float32_share():
    """On every multi-layer case of the GPU suite: at least 60 % of the restatement's LLRs are neither 0 nor +-120 (a
    wrong scale or variance then moves them), every (layers, modulation) pair occurs, and float32 arithmetic in the
    kernel's own sequence (mmse_float32) moves no LLR by more than one step and at most MMSE_FLOAT32_SHARE of them:
    the GPU tolerance MMSE_SHARE_BOUND is ten times that, floored at 1e-3."""
    worst, pairs = 0.0, set()
    for key, (cfg, g, h, nv, crb) in all_gpu_cases():
        want = K.demodulate_with(D.equalize_mmse, cfg, from_bf16(g), from_bf16(h), nv, crb).astype(np.int16)
        assert K.informative_share(want) >= 0.6, (key, K.informative_share(want))
        d = np.abs(K.demodulate_with(K.mmse_float32, cfg, from_bf16(g), from_bf16(h), nv, crb) - want)
        assert d.max() <= 1, key
        worst = max(worst, float(np.mean(d > 0)))
        pairs.add((cfg["nof_layers"], cfg["qm"]))
    print("float32 share, worst case:", worst)
    assert pairs == {(L, qm) for L in (2, 3, 4) for qm in (2, 4, 6, 8)}
    assert worst <= K.MMSE_FLOAT32_SHARE
    assert K.MMSE_SHARE_BOUND == max(10 * K.MMSE_FLOAT32_SHARE, 1e-3)
