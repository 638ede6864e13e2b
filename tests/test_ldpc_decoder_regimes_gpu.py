"""GPU parity of the LDPC decoder on the regime grid (tests/ldpc_regime_cases.py): every lifting size of both base graphs
in every compiled layer class (8, 16, all rows) and on the class boundaries (8 | 9, 16 | 17 layers, the latter inputs
ending one LLR into a lifted column), with six LLR families (nominal, amplitude 2, unit amplitude, saturated, two-valued,
+/-127 with wrong signs) in both arithmetics and every kernel variant. Bit-exact against the CPU oracle, which
tests/test_oracle_vs_reference.py holds to the reference on these same inputs; tests/test_ldpc_regimes_oracle.py shows
which regimes the inputs reach and that eight hand-made decoder errors would change their results.

At the PUSCH plan level the fused dematching front end gets a case in every layer class and on the class boundaries, on
off-nominal LLR families, at seven lifting sizes of both base graphs."""
import numpy as np
import pytest

import ldpc_regime_cases as R
from decoder_frontend_cases import _case, _check_group, _geometry, _pick_E
from oracle_lib import BG_K, BG_N_SHORT, CRC24B, Oracle
from test_ldpc_decoder_gpu import VARIANTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


@pytest.fixture(scope="module")
def grid(orc):
    return R.grid_with_results(orc)


@pytest.fixture(scope="module")
def sweep(orc):
    return R.sweep_with_results(orc)


@pytest.fixture(params=sorted(VARIANTS))
def variant(request, ctx):
    with ctx.options(**VARIANTS[request.param]):
        yield request.param


def _decode(ctx, dec_type, cases):
    import srsgpu
    return srsgpu.LdpcDecoder(ctx, dec_type).decode_batch(*R.product_batch(srsgpu, cases))


def _assert_equal(got, want, cases, note=()):
    assert len(got) == len(want) == len(cases)
    for i, ((r_g, b_g), (r_w, b_w), c) in enumerate(zip(got, want, cases)):
        key = note + (i, c["bg"], c["Z"], c["li"], c["layers"], c["family"], c["kind"], c["sf"])
        assert r_g == r_w, key + (r_g, r_w)
        assert np.array_equal(b_g, b_w), key


@pytest.mark.parametrize("dec_type,mode", R.MODES)
def test_regime_grid_one_batch(ctx, grid, dec_type, mode, variant):
    """The whole grid in ONE batch per arithmetic and kernel variant: every (BG, Z) decodes with 4, 8, 9, 16, 17 and all
    layers in the same launch group as every other size of its class."""
    cases, res = grid
    _assert_equal(_decode(ctx, dec_type, cases), res[mode][0], cases, (variant,))


@pytest.mark.parametrize("dec_type,mode", R.MODES)
def test_regime_grid_single_size_batches(ctx, grid, dec_type, mode):
    """The grid's codeblocks of one lifting size per batch: the workgroup is sized for that Z and not for the largest
    of a mixed batch. Z = 2, 10, 36, 64, 128, 144, 384, and the odd sizes 7 and 15 together. Equal to the mixed batch's
    results and to the oracle's."""
    cases, res = grid
    mixed = _decode(ctx, dec_type, cases)
    for sizes in ((2,), (10,), (36,), (64,), (128,), (144,), (384,), (7, 15)):
        sel = [i for i, c in enumerate(cases) if c["Z"] in sizes]
        assert len(sel) == 2 * 12 * len(sizes)
        got = _decode(ctx, dec_type, [cases[i] for i in sel])
        _assert_equal(got, [mixed[i] for i in sel], [cases[i] for i in sel], ("mixed",) + sizes)
        _assert_equal(got, [res[mode][0][i] for i in sel], [cases[i] for i in sel], ("oracle",) + sizes)


@pytest.mark.parametrize("dec_type,mode", R.MODES)
def test_regime_scaling_sweep(ctx, sweep, dec_type, mode, variant):
    """Scaling factors 0.5 .. 0.99995 on amplitude-2 and two-valued LLRs, where the two arithmetics' scaling rules
    differ most, at (BG1, 15), (BG2, 36), (BG1, 176), (BG1, 208) in the 8-layer and the all-rows class."""
    cases, res = sweep
    _assert_equal(_decode(ctx, dec_type, cases), res[mode][0], cases, (variant,))


def test_regime_golden_vectors(ctx, variant):
    """The GPU decoder against the reference's own recorded outputs on the grid's fixture subset
    (tests/golden/ldpc_decoder_regimes.npz), one batch per arithmetic."""
    import golden_lib as G
    cases = list(G.decoder_regime_cases())
    for impl, dec_type in ((0, "generic"), (1, "avx2")):
        want = [(None if c["iters"][impl] < 0 else c["iters"][impl], c["bits"][impl]) for c in cases]
        _assert_equal(_decode(ctx, dec_type, cases), want, cases, (variant, dec_type))


# ---- PUSCH plan level: the fused dematching front end in every layer class ------------------------------------------

PLAN_SIZES = (36, 104, 128, 144, 192, 208, 384)
PLAN_BOUNDS = (8, 9, 16, 17, 0)  # 0: all rows
PLAN_MODULATIONS = ((8, 0), (8, 4), (8, 6), (6, 0))  # (Qm, fillers): groups of four, symbol by symbol, 64QAM
PLAN_FAMILIES = ("low", "saturated", "pm127")
PLAN_Q = {8: 0.55, 9: 0.55, 16: 0.85, 17: 0.85, 0: 1.0}
# With 4 iterations or 1 (decoder_frontend_cases._case) the +/-127 family takes half the grid's share of wrong signs.
PLAN_FAMILY_Q = {"low": 1.0, "saturated": 1.0, "pm127": 0.5}


def _layer_bound(bg, Z, E, F):
    """The layer bound the host derives for a fused first transmission (capi.cpp add_pusch_cb, layer_class)."""
    return max(-(-(E + F) // Z) + 2, BG_K[bg] + 4) - BG_K[bg]


def _plan_E(bg, Z, qm, F, bound):
    """A fusable rate-matched length whose layer bound is `bound`; for all rows the longest aligned one (E = N - F
    where that is aligned: every layer runs, and where it is not, the HARQ tail is shorter than a column)."""
    N, _ = _geometry(bg, Z, F)
    if bound:
        return _pick_E(bg, Z, qm, F, lambda E: _layer_bound(bg, Z, E, F) == bound, rate=1.0)
    step = 32 if qm == 8 else 24
    E = (N - F) // step * step
    assert _layer_bound(bg, Z, E, F) == BG_N_SHORT[bg] + 2 - BG_K[bg]
    return E


def _plan_llrs(orc, rng, bg, Z, qm, E, F, family, q):
    """The rate-matched codeword of a random payload with its CRC24B, as LLRs of a regime family."""
    L = BG_K[bg] * Z - F
    msg = np.zeros(BG_K[bg] * Z, np.uint8)
    msg[:L - 24] = rng.integers(0, 2, L - 24)
    c = orc.crc_bits(CRC24B, msg[:L - 24])
    msg[L - 24:L] = [(c >> (23 - i)) & 1 for i in range(24)]
    cw = orc.rate_match(bg, Z, 0, qm, 0, F, orc.ldpc_encode(bg, Z, msg), E)
    return R.family_llrs(rng, family, 1 - 2 * cw.astype(np.int32), q)


@pytest.mark.parametrize("bg", [1, 2])
@pytest.mark.parametrize("dec_type,mode", R.MODES)
def test_plan_fused_front_end_layer_classes(orc, ctx, dec_type, mode, bg):
    """Z = 36, 104, 128, 144, 192, 208, 384 with the rate-matched length set for a layer bound of 8, 9, 16, 17 and all
    rows (every FUSED instantiation of every layer class, and both sides of each class boundary), 256QAM with 0 / 4 / 6
    fillers and 64QAM, each shape with an amplitude-2, a saturated and a +/-127 codeblock of random
    payload: fused against unfused, pinned-split and two-codeblock plans and against the oracle (HARQ buffer, bits,
    iterations, CRC flag)."""
    import srsgpu
    rng = np.random.default_rng(1700 + 2 * bg + mode)
    cbs, llrs = [], []
    for Z in PLAN_SIZES:
        for bound in PLAN_BOUNDS:
            for qm, F in PLAN_MODULATIONS:
                E = _plan_E(bg, Z, qm, F, bound)
                N, ninfo = _geometry(bg, Z, F)
                assert ninfo <= E <= N - F and E % qm == 0  # fusable
                for family in PLAN_FAMILIES:
                    cbs.append(_case(srsgpu, len(cbs), True, bg, Z, qm, E, F))
                    llrs.append(_plan_llrs(orc, rng, bg, Z, qm, E, F, family, PLAN_Q[bound] * PLAN_FAMILY_Q[family]))
    assert len(cbs) == 7 * 5 * 4 * 3
    _check_group(orc, ctx, cbs, llrs, 1710 + 2 * bg + mode, dec_type, mode, pairs=True)
