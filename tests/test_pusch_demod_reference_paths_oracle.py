"""The restatement of the reference's own demodulator paths (oracle/pusch_demod_oracle.py: D.equalize for ZF 1 x N,
ZF 2 x N and one-layer MMSE, D.transform_deprecode for DFT-s-OFDM) checked on its own, without the kernel, and the
tolerance the GPU tests hold the kernel to (tests/test_pusch_demodulator_gpu.py, test_pusch_demod_ref_* and
test_pusch_demod_tp_*) derived from rounding alone:

  - D.transform_deprecode is an explicit float64 inverse-DFT matrix product scaled by 1 / sqrt(M), and replaces the
    valid noise variances (positive, finite) by their mean while keeping the others;
  - pusch_demod_cases.zf_equalize in float32 is D.equalize bit for bit, so that its float64 evaluation and its
    hand-made errors are those of the restatement;
  - float32 against float64 in D.equalize's formulas, and the kernel's float32 Stockham inverse DFT restated in numpy
    (pusch_demod_cases.tp_float32) against the restatement's complex128 one, move at most REF_PATHS_FLOAT32_SHARE of
    the LLRs by one step (measured here, printed): the GPU bound REF_PATHS_SHARE_BOUND is max(10 x that, 1e-3);
  - every GPU case is informative (>= 60 % of the restatement's LLRs neither 0 nor +-120);
  - each hand-made error (PERTURBATIONS below) moves more than REF_PATHS_SHARE_BOUND of the LLRs on every case it
    applies to, so a kernel within the bound of the restatement cannot hide any of them."""
import numpy as np
import pytest

import pusch_demod_cases as K
import pusch_demod_oracle as D
from pusch_demod_cases import from_bf16


def share(a, b):
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    return float(np.mean(d > 0)), int(d.max())


def cplx(case):
    cfg, g, h, nv, crb = case
    return cfg, from_bf16(g), from_bf16(h), nv, crb


_slots = {}


def tp_cplx(case):
    """As cplx, the conversion of a shared 273-PRB slot done once."""
    cfg, g, h, nv, crb = case
    if id(g) not in _slots:
        _slots[id(g)] = (g, from_bf16(g), from_bf16(h))
    return cfg, _slots[id(g)][1], _slots[id(g)][2], nv, crb


def f64(rx, H, nv):
    return K.zf_equalize(rx, H, nv, real=np.float64)


# ----------------------------------------------------------------------------------------------------------------------
# D.transform_deprecode on its own.
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [12, 60, 180, 3240])
def test_transform_deprecode_is_the_inverse_dft_matrix(m):
    rng = np.random.default_rng(m)
    x = (rng.normal(size=m) + 1j * rng.normal(size=m)).astype(np.complex64)
    k = np.arange(m)
    w = np.exp(2j * np.pi * (np.outer(k, k) % m) / m) / np.sqrt(m)  # the phase reduced exactly, in integers
    want = w @ x.astype(np.complex128)
    # The restatement rounds its result to complex64: compared before the rounding, through the same expression.
    got = np.fft.ifft(x.astype(np.complex128)) * m / np.sqrt(m)
    assert np.max(np.abs(got - want)) < 1e-12
    out, _ = D.transform_deprecode(x, np.ones(m, np.float32))
    assert np.array_equal(out, got.astype(np.complex64))
    # A unit impulse at position 1 comes back as the positive-exponent tone: the direction of the transform.
    e = np.zeros(m, np.complex64)
    e[1] = 1
    assert np.max(np.abs(D.transform_deprecode(e, np.ones(m, np.float32))[0] - w[:, 1])) < 1e-7


def test_transform_deprecode_noise_rule():
    v = np.array([0.5, 0.0, -1.0, np.inf, np.nan, 1.5, 0.25, -np.inf, 1e-30], np.float32)
    _, out = D.transform_deprecode(np.zeros(v.size, np.complex64), v)
    valid = np.array([1, 0, 0, 0, 0, 1, 1, 0, 1], bool)
    mean = np.float32((0.5 + 1.5 + 0.25 + 1e-30) / 4)
    assert np.all(out[valid] == mean)
    assert np.array_equal(out[~valid], v[~valid], equal_nan=True)
    # No valid variance: everything kept.
    w = np.array([0.0, np.inf, -2.0], np.float32)
    assert np.array_equal(D.transform_deprecode(np.zeros(3, np.complex64), w)[1], w)


def test_tp_radix_sequences():
    """The 53 valid sizes, and what the kernel's pass order makes of them: M = 3240 takes every pass kind."""
    sizes = K.valid_tp_prbs(273)
    assert len(sizes) == 53 and sizes[0] == 1 and sizes[-1] == 270
    assert K.tp_radix_sequence(3240) == (4, 2, 3, 3, 3, 3, 5)
    for n in sizes:
        seq = K.tp_radix_sequence(12 * n)
        assert int(np.prod(seq)) == 12 * n and seq[0] == 4 and list(seq[1:]) == sorted(seq[1:], key=(4, 2, 3, 5).index)
        assert seq.count(2) <= 1


def test_tp_float32_is_an_inverse_dft():
    """The aid itself: every size within float32 rounding (1e-5 relative to the RMS) of the restatement."""
    rng = np.random.default_rng(9)
    for n in K.valid_tp_prbs(273):
        m = 12 * n
        x = (rng.normal(size=m) + 1j * rng.normal(size=m)).astype(np.complex64)
        v = rng.uniform(0.1, 1, m).astype(np.float32)
        v[::5] = np.inf
        a, av = K.tp_float32(x, v)
        b, bv = D.transform_deprecode(x, v)
        assert np.max(np.abs(a - b)) < 1e-5, n
        assert np.array_equal(np.isinf(av), np.isinf(bv)) and np.allclose(av[::3], bv[::3], rtol=1e-6), n


# ----------------------------------------------------------------------------------------------------------------------
# The cases of the GPU suite: informative, and what float32 alone moves.
# ----------------------------------------------------------------------------------------------------------------------
def zf_gpu_cases():
    for key in K.REF_SINGLES:
        yield key + ("single",), K.ref_single_case(*key)
    for key in K.REF_WIDE_256 + K.REF_WIDE_128:
        yield key + ("wide",), K.ref_wide_case(*key)


def test_zf_equalize_float32_is_the_restatement():
    for key, case in zf_gpu_cases():
        cfg, g, h, nv, crb = cplx(case)
        want = D.demodulate_ex(cfg, g, h, nv, crb_mask=crb)[0]
        got = K.demodulate_with(K.zf_equalize, cfg, g, h, nv, crb)
        assert np.array_equal(got, want), key
        if cfg["nof_layers"] == 1:  # one-layer MMSE is ZF
            assert np.array_equal(D.demodulate_ex(cfg, g, h, nv, mmse=True, crb_mask=crb)[0], want), key


def test_zf_cases_are_informative_and_float32_share():
    """On every one- and two-layer ZF case of the GPU suite: >= 60 % informative LLRs, and float32 against float64 in
    the same formulas moves no LLR by more than one step and at most REF_PATHS_FLOAT32_SHARE of them."""
    worst = 0.0
    for key, case in zf_gpu_cases():
        cfg, g, h, nv, crb = cplx(case)
        want = K.demodulate_with(D.equalize, cfg, g, h, nv, crb)
        assert K.informative_share(want) >= 0.6, (key, K.informative_share(want))
        s, step = share(K.demodulate_with(f64, cfg, g, h, nv, crb), want)
        assert step <= 1, key
        worst = max(worst, s)
    print("ZF float32 share, worst case:", worst)
    assert worst <= K.REF_PATHS_FLOAT32_SHARE
    assert K.REF_PATHS_SHARE_BOUND == max(10 * K.REF_PATHS_FLOAT32_SHARE, 1e-3)


def tp_gpu_cases():
    keys, cases, _, _ = K.tp_size_plan()
    for key, case in zip(keys, cases):
        yield key, case
    for name, case in K.tp_extra_cases():
        yield name, case


def test_tp_cases_are_informative_and_float32_share():
    """On every transform-precoded case of the GPU suite (all 53 sizes): >= 60 % informative LLRs (but for the zero-
    noise and underflow cases, whose LLRs are all 0 or saturated by construction), the helper for perturbed
    restatements is D.demodulate_ex with the restatement's own parts, and the kernel's float32 sequence (tp_float32)
    moves no LLR by more than one step and at most REF_PATHS_FLOAT32_SHARE of them."""
    moved, total, seen, least = {}, {}, set(), 1.0
    for key, case in tp_gpu_cases():
        cfg, g, h, nv, crb = tp_cplx(case)
        want = D.demodulate_ex(cfg, g, h, nv, crb_mask=crb, transform_precoding=True)[0]
        assert np.array_equal(K.tp_demodulate_with(D.transform_deprecode, cfg, g, h, nv, crb), want), key
        if key not in ("zero", "other"):
            assert K.informative_share(want) >= 0.6, (key, K.informative_share(want))
            least = min(least, K.informative_share(want))
        s, step = share(K.tp_demodulate_with(K.tp_float32, cfg, g, h, nv, crb), want)
        assert step <= 1, key
        # The sizes are one symbol each, 24 to 25 920 LLRs: their share is taken over all of them together (one LLR of
        # the smallest would be 4 %), and so is that of the extras.
        group = "sizes" if isinstance(key, tuple) else "extras"
        moved[group] = moved.get(group, 0) + round(s * want.size)
        total[group] = total.get(group, 0) + want.size
        seen.add(cfg["nof_rb"])
    shares = {k: moved[k] / total[k] for k in moved}
    print("transform precoding float32 share:", shares, "LLRs:", total, "least informative share:", least)
    assert seen >= set(K.valid_tp_prbs(273))
    assert max(shares.values()) <= K.REF_PATHS_FLOAT32_SHARE


# ----------------------------------------------------------------------------------------------------------------------
# Hand-made errors: the restatement differs from each by more than the GPU bound on every case it applies to.
# ----------------------------------------------------------------------------------------------------------------------
def scaled(eq, factor):
    def f(rx, H, nv):
        e, v = eq(rx, H, nv)
        return e * np.float32(factor), v
    return f


def swapped(rx, H, nv):
    e, v = D.equalize(rx, H, nv)
    return e[:, ::-1], v[:, ::-1]


ZF_PERTURBATIONS = {
    # name: (equaliser, the (L, P) it applies to)
    "zf1 variance max(nv) / sum |h|^2": (lambda rx, H, nv: K.zf_equalize(rx, H, nv, variance="max"),
                                         lambda L, P: L == 1 and P >= 2),
    "zf2 mean noise variance": (lambda rx, H, nv: K.zf_equalize(rx, H, nv, nv2="mean"), lambda L, P: L == 2),
    "zf2 layers swapped": (swapped, lambda L, P: L == 2),
    "symbols x 1.02": (scaled(D.equalize, 1.02), lambda L, P: True),
}


def tp_scale(eq, nvar):
    x, v = D.transform_deprecode(eq, nvar)
    return x * np.float32(1.02), v


def tp_per_re_variance(eq, nvar):
    return D.transform_deprecode(eq, nvar)[0], nvar


def tp_mean_over_all(eq, nvar):
    x, _ = D.transform_deprecode(eq, nvar)
    v = np.asarray(nvar, np.float32)
    valid = (v > 0) & np.isfinite(v)
    with np.errstate(all="ignore"):
        return x, np.where(valid, np.float32(np.mean(v, dtype=np.float64)), v)


TP_PERTURBATIONS = {
    # name: (deprecode, equaliser, the cases it applies to)
    "tp symbols x 1.02 before the inverse DFT": (D.transform_deprecode, scaled(D.equalize, 1.02), lambda key: True),
    "tp inverse DFT scale x 1.02": (tp_scale, D.equalize, lambda key: True),
    "tp per-RE variances": (tp_per_re_variance, D.equalize, lambda key: True),
    "tp mean over all variances": (tp_mean_over_all, D.equalize, lambda key: key == "dead"),
}
PERTURBATIONS = list(ZF_PERTURBATIONS) + list(TP_PERTURBATIONS)


@pytest.mark.parametrize("name", list(ZF_PERTURBATIONS))
def test_zf_perturbations_show(name):
    eq, applies = ZF_PERTURBATIONS[name]
    n, least = 0, 1.0
    for key in K.REF_SINGLES:
        if not applies(key[0], key[1]):
            continue
        cfg, g, h, nv, crb = cplx(K.ref_single_case(*key))
        want = K.demodulate_with(D.equalize, cfg, g, h, nv, crb)
        s, _ = share(K.demodulate_with(eq, cfg, g, h, nv, crb), want)
        assert s > K.REF_PATHS_SHARE_BOUND, (name, key, s)
        n, least = n + 1, min(least, s)
    print(name, ":", n, "cases, least share moved", least)
    assert n >= 8


@pytest.mark.parametrize("name", list(TP_PERTURBATIONS))
def test_tp_perturbations_show(name):
    dep, eq, applies = TP_PERTURBATIONS[name]
    n, least = 0, 1.0
    for key, case in tp_gpu_cases():
        if key in ("zero", "other") or not applies(key):
            continue
        cfg, g, h, nv, crb = tp_cplx(case)
        want = K.tp_demodulate_with(D.transform_deprecode, cfg, g, h, nv, crb)
        s, _ = share(K.tp_demodulate_with(dep, cfg, g, h, nv, crb, equalizer=eq), want)
        assert s > K.REF_PATHS_SHARE_BOUND, (name, key, s)
        n, least = n + 1, min(least, s)
    print(name, ":", n, "cases, least share moved", least)
    assert n >= 1
