"""The estimator's time-alignment transform at every size that 1, 11 and 273 PRB reach, against the float64
restatement (oracle/pusch_chest_oracle.py) at the tolerances of tests/test_pusch_chest_gpu.py.

The sizes (time_alignment_estimator_dft_impl get_idft: the pilot span x 4096 / 3300, next power of two, at least 128):
1 PRB -> 128; 11 PRB -> 128 with DM-RS type 1 (66 pilots), 256 with type 2 (a span of 128 REs); 273 PRB -> 2048 with
type 1, 4096 with type 2 (the size without the quadratic refinement). 128 and 2048 have an odd number of radix-2
stages (the last one alone), 256 and 4096 an even number. Every case has a CFO and a delay, so that the peak is off
bin 0 and the refinement matters. A reformulation of the transform's twiddle angles (j / 2^k as a scaling by the power
of two) must leave all of this where it is; one was measured and left out (profiles/ul_front_end_trim.md)."""
import numpy as np
import pytest

import pusch_chest_oracle as C
from ofdm_oracle import bf16_to_complex
from pusch_chest_cases import random_case
from test_pusch_chest_gpu import CFO_TOL, T_C, pad4, region, to_est

pytestmark = pytest.mark.gpu

GRID_PRB = 273
# (PRB, DM-RS type 2, transform size)
SHAPES = [(1, 0, 128), (1, 1, 128), (11, 0, 128), (11, 1, 256), (273, 0, 2048), (273, 1, 4096)]


def ta_size(nof_rb, type2):
    """The transform size of a contiguous allocation (capi_pusch_chest.cpp: pilots of type 1, the RE span of type 2)."""
    return C.ta_dft_size((nof_rb - 1) * 12 + 8 if type2 else nof_rb * 6)


def test_shapes_reach_every_size():
    assert [ta_size(n, t2) for n, t2, _ in SHAPES] == [s for _, _, s in SHAPES]
    assert {s for _, _, s in SHAPES} == {ta_size(n, t2) for n in (1, 11, 273) for t2 in (0, 1)}


_memo = {}


def results(ctx):
    """One plan over the six cases (one 273-PRB slot each) and the restatement of each, computed once."""
    if not _memo:
        import srsgpu
        rng = np.random.default_rng(4242)
        cases = [random_case(rng, GRID_PRB, nof_rb=n, dmrs_type2=t2, cfo_hz=rng.uniform(-1500, 1500),
                             delay=rng.uniform(-25, 25), snr_db=25.0, dmrs_mask=(1 << 2) | (1 << 5))
                 for n, t2, _ in SHAPES]  # two DM-RS symbols inside every allocation random_case draws: a CFO exists
        grids = np.stack([pad4(g) for _, g, _ in cases])
        ests = [to_est(cfg, 2, 1, 0, 1) for cfg, _, _ in cases]  # filter, average, CFO compensated
        got = srsgpu.PuschChannelEstimator(ctx, GRID_PRB, 4).estimate_batch(grids, ests, list(range(len(cases))))
        want = [C.estimate(cfg, bf16_to_complex(grid), "filter", "average", True) for cfg, grid, _ in cases]
        _memo.update(cases=cases, got=got, want=want)
    return _memo


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[f"prb{n}-type{1 + t2}-dft{s}" for n, t2, s in SHAPES])
def test_time_alignment_size_vs_oracle(ctx, i):
    r = results(ctx)
    cfg = r["cases"][i][0]
    ce, nv, m = r["got"]
    ch, nvo, rsrp, epre, ex = r["want"][i]
    P = cfg["nof_rx_ports"]
    ls, ks = region(cfg)
    got = bf16_to_complex(ce[i, 0, :P])[:, ls, ks]
    w = ch[:, ls, ks]
    print("ta_s", m[i, :P, 4], ex["ta_s"], "cfo", m[i, :P, 5], ex["cfo_hz"])
    assert np.max(np.abs(got - w)) < CFO_TOL[0] * np.sqrt(np.mean(np.abs(w) ** 2)), cfg
    np.testing.assert_allclose(nv[i, :P], nvo, rtol=1e-3)
    np.testing.assert_allclose(m[i, :P, 0], rsrp, rtol=1e-3)
    np.testing.assert_allclose(m[i, :P, 1], epre, rtol=1e-3)
    np.testing.assert_allclose(m[i, :P, 4], ex["ta_s"], atol=2 * T_C)
    np.testing.assert_allclose(m[i, :P, 5], ex["cfo_hz"], atol=0.05)
