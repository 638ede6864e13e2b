"""GPU parity of the packed LDPC decoder's first iteration. Before iteration 0 every check-to-variable message is zero:
pass 1 of every layer rebuilds that zero from the layer state (sign bits, argmin, min1 / min2, the 8-layer class's
whole c2v words) and pass 2 creates the state that iteration 1 reads. A kernel that runs iteration 0 as a peeled copy
whose pass 1 takes the messages from the soft bits alone (profiles/valu_trim.md: measured, no gain in the headline, not
in the tree) has to pass these cases. Bits, iteration count and CRC outcome against the CPU oracle (orc_ldpc_decode),
bit-exact.

Cases, for BG1 and BG2, Z = 2 (the smallest packed size), 16, 208, 384 and inputs of the 8-, 16- and all-layer classes:
one iteration only with a CRC that passes and one that fails; two iterations without CRC (the second iteration reads
what the first one wrote); clean LLRs that stop after iteration 1 of 6; fillers and +/-127 LLRs (soft bits infinite
before the first message), two-valued LLRs, an all-zero tail (fewer layers than the input length suggests). Both
arithmetics; the one-codeblock, the edge-split and the two-codeblock kernels.

At the PUSCH plan level the same kernels with the fused dematching front end and with the separate rate dematcher, one
and two iterations, with and without early stop."""
import numpy as np
import pytest

import ldpc_regime_cases as R
from decoder_frontend_cases import _check_group, _geometry, _llrs
from oracle_lib import BG_K, Oracle
from test_ldpc_decoder_gpu import VARIANTS
from test_ldpc_decoder_regimes_gpu import _assert_equal, _decode, _plan_E, _plan_llrs

pytestmark = pytest.mark.gpu

SIZES = (2, 16, 208, 384)
KINDS = ("one_pass", "one_fail", "two_nocrc", "clean_stop", "pm127", "two_valued", "zero_tail")
LENGTHS = (1, 3, 5)  # ldpc_regime_cases.lengths: 8 layers, 16 layers, all rows


def _llr(rng, kind, sign):
    n = sign.size
    if kind in ("one_pass", "clean_stop"):
        return (10 * sign).astype(np.int8)
    if kind in ("one_fail", "two_nocrc"):
        return np.clip(np.round(10 * sign + rng.normal(0, 11, n)), -120, 120).astype(np.int8)
    if kind == "pm127":
        return (127 * sign * np.where(rng.random(n) < 0.02, -1, 1)).astype(np.int8)
    if kind == "two_valued":
        return (10 * sign * np.where(rng.random(n) < 0.05, -1, 1)).astype(np.int8)
    if kind == "zero_tail":
        return np.clip(np.round(12 * sign + rng.normal(0, 4, n)), -120, 120).astype(np.int8)
    raise ValueError(kind)


def build_cases(orc):
    """Every (BG, Z, layer class, kind). Fillers on every second shape, marked +127 as the rate dematcher does."""
    cases = []
    for bg in (1, 2):
        for zi, Z in enumerate(SIZES):
            K = BG_K[bg]
            for li in LENGTHS:
                n_llr, layers = R.lengths(bg, Z)[li]
                for ki, kind in enumerate(KINDS):
                    nof_filler = min(Z, (K - 2) * Z // 5) if (zi + li + ki) % 2 else 0
                    crc_poly, nof_crc_bits = R.pick_crc(bg, Z, nof_filler)
                    rng = np.random.default_rng([7300, bg, Z, li, ki])
                    sign = R.codeword(orc, rng, bg, Z, crc_poly, nof_filler)
                    llr = _llr(rng, kind, sign)
                    if kind == "zero_tail":
                        # The input's tail is zeros from the middle of a column two layers below the length on.
                        llr[n_llr - 2 * Z - Z // 2:] = 0
                        llr = llr[:n_llr].copy()
                        if nof_filler:
                            llr[(K - 2) * Z - nof_filler:(K - 2) * Z] = 127
                    else:
                        llr = R._finish(llr, bg, Z, nof_filler, n_llr)
                    max_iter = {"one_pass": 1, "one_fail": 1, "two_nocrc": 2}.get(kind, R.MAX_ITER)
                    use_crc = kind != "two_nocrc"
                    cases.append(R._case(bg, Z, li, layers, kind, kind, llr, crc_poly if use_crc else -1, nof_crc_bits,
                                         nof_filler, max_iter))
    return cases


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


@pytest.fixture(scope="module")
def cases(orc):
    cs = build_cases(orc)
    return cs, {mode: R.oracle_results(orc, cs, mode)[0] for _, mode in R.MODES}


def test_cases_reach_the_first_iteration_outcomes(cases):
    """The oracle's outcomes the cases are made for, in both arithmetics: the one-iteration cases pass (clean) and fail
    (noisy) their CRC, the clean six-iteration ones stop after iteration 1, and some case needs more than one."""
    cs, res = cases
    for _, mode in R.MODES:
        by_kind = {k: [r for (r, _), c in zip(res[mode], cs) if c["kind"] == k] for k in KINDS}
        assert all(r == 1 for r in by_kind["one_pass"])
        assert any(r is None for r in by_kind["one_fail"])
        assert all(r == 1 for r in by_kind["clean_stop"])
        assert any(r is not None and r > 1 for k in ("pm127", "two_valued", "zero_tail") for r in by_kind[k])


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("dec_type,mode", R.MODES)
def test_first_iteration_one_batch(ctx, cases, dec_type, mode, variant):
    """All cases in one batch per arithmetic and kernel variant."""
    cs, res = cases
    with ctx.options(**VARIANTS[variant]):
        _assert_equal(_decode(ctx, dec_type, cs), res[mode], cs, (variant,))


@pytest.mark.parametrize("dec_type,mode", R.MODES)
def test_first_iteration_single_size_batches(ctx, cases, dec_type, mode):
    """One lifting size per batch with the one-codeblock kernel pinned: the workgroup is sized for that Z."""
    cs, res = cases
    with ctx.options(**VARIANTS["plain"]):
        for Z in SIZES:
            sel = [i for i, c in enumerate(cs) if c["Z"] == Z]
            _assert_equal(_decode(ctx, dec_type, [cs[i] for i in sel]), [res[mode][i] for i in sel],
                          [cs[i] for i in sel], (Z,))


PLAN_SIZES = (36, 208, 384)
PLAN_BOUNDS = (8, 16, 0)
PLAN_ITERS = ((True, 1), (False, 1), (True, 2), (False, 2))  # (early stop, iteration limit)


def build_plan_cases(orc, srsgpu, bg, mode):
    rng = np.random.default_rng(7400 + 2 * bg + mode)
    cbs, llrs = [], []
    for Z in PLAN_SIZES:
        for bound in PLAN_BOUNDS:
            for qm, F in ((8, 0), (6, 0), (8, 4)):
                E = _plan_E(bg, Z, qm, F, bound)
                N, ninfo = _geometry(bg, Z, F)
                assert ninfo <= E <= N - F and E % qm == 0  # fusable
                for j, (early, max_iter) in enumerate(PLAN_ITERS):
                    # Clean enough to pass after one iteration, a noisy codeword, and noise alone (fails).
                    family, q = (("low", 0.1), ("baseline", 2.2), ("noise", 0.0))[(j + len(cbs) // 4) % 3]
                    cbs.append(srsgpu.PuschCodeblock(bg, Z, 0, qm, E, nof_filler_bits=F, new_data=True,
                                                     use_early_stop=early, max_iterations=max_iter))
                    if family == "noise":
                        llrs.append(_llrs(rng, E, False))
                    else:
                        llrs.append(_plan_llrs(orc, rng, bg, Z, qm, E, F, family, q))
    return cbs, llrs


@pytest.mark.parametrize("bg", [1, 2])
@pytest.mark.parametrize("dec_type,mode", R.MODES)
def test_first_iteration_plan_fused_and_unfused(orc, ctx, dec_type, mode, bg):
    """One and two iterations at the plan level: the fused front end (host-picked kernel and the one-codeblock kernel
    pinned), the separate rate dematcher and the two-codeblock plan against each other and the oracle composition
    (HARQ buffer, bits, iterations, CRC flag), in the 8-, 16- and all-layer classes."""
    import srsgpu
    cbs, llrs = build_plan_cases(orc, srsgpu, bg, mode)
    _check_group(orc, ctx, cbs, llrs, 7410 + 2 * bg + mode, dec_type, mode, pairs=True)
