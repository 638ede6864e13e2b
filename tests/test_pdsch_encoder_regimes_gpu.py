"""GPU parity of both PDSCH encoder kernels on the regime grid of tests/pdsch_encoder_regime_cases.py: every lifting
size a one-codeblock TB selects, at every rv, buffer kind and Qm, with rate-matched lengths on each side of the wrap,
of the filler range and of the lifted columns that decide how many extension rows the encoder computes. What the cases
reach is held to its floors on the CPU by tests/test_pdsch_encoder_regimes_oracle.py.

Every codeword is compared bit for bit with the oracle composition of the other encoder tests (chain_lib), computed
once per module, and on the GOLDEN_Z subset with the reference's own codewords (tests/golden/pdsch_encoder_regimes.npz).
The output is pre-filled with 0xAB: the plan zeroes the range from its first to its last codeword word (the spare bits
of a codeword's last word and the gaps between codewords read zero, as test_pdsch_encoder_order_gpu.py holds) and writes
nothing behind it.

The tests are parametrised by base graph and kernel, not by case; an assertion names the first failing case and its
census."""
import numpy as np
import pytest

import golden_lib as G
import pdsch_encoder_regime_cases as R
from oracle_lib import Oracle
from test_pdsch_encoder_order_gpu import _encode_plan

pytestmark = pytest.mark.gpu
GAP_BYTES = 8
_RAW = {}  # output bytes of the grid plans, by (base graph, kernel)


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def grid(orc):
    """Cases, their TBs and the oracle's codewords, computed once."""
    cases, want = R.grid_with_expected(orc)
    return cases, [R.transport_block(c) for c in cases], want


@pytest.fixture(scope="module")
def multi(orc):
    cases, want = R.multi_with_expected(orc)
    return cases, [R.transport_block(c) for c in cases], want


def _cfg(c):
    import srsgpu
    return srsgpu.PdschTransportBlock(c["bg"], c["rv"], c["qm"], c["layers"], c["nsym"], c["Nref"])


def _run(ctx, cases, tbs, want, idx, kernel, gap=GAP_BYTES, tb_tail=16, zero_output=None, tiled=False):
    """One plan over the cases `idx` with the byte kernel forced or the plan's own choice: codewords bit-exact, zeros
    between them (0xAB kept when the plan is told its codewords tile the output), 0xAB behind the last one. Returns
    the output bytes."""
    opts = {"encoder_byte_kernel": 1} if kernel == "byte" else {}
    if zero_output is not None:
        opts["encoder_zero_output"] = zero_output
    with ctx.options(**opts):
        got, raw, ranges = _encode_plan(ctx, [tbs[i] for i in idx], [_cfg(cases[i]) for i in idx],
                                        [n % 4 for n in range(len(idx))], gap, tb_tail)
    for i, g in zip(idx, got):
        if not np.array_equal(g, want[i]):
            k = R.census(cases[i])
            bad = np.flatnonzero(g != want[i])
            raise AssertionError((kernel, R.key(cases[i]), "bits wrong", bad.size, "first", int(bad[0]),
                                  {x: k[x] for x in ("E", "v0", "V", "ninfo", "filler", "Ncb", "k0", "n_ext", "top",
                                                     "kernel")}, [x for x in R.CLASSES if k[x]]))
    end = ranges[-1][0] + (ranges[-1][1] - ranges[-1][0] + 3) // 4 * 4
    assert (raw[end:] == 0xAB).all(), (kernel, "a store behind the last codeword")
    if not tiled:
        for n, ((b, e), i) in enumerate(zip(ranges, idx)):
            nxt = ranges[n + 1][0] if n + 1 < len(ranges) else end
            spare = np.unpackbits(raw[e - 1:e])[(want[i].size - 1) % 8 + 1:]
            assert not spare.any() and not raw[e:nxt].any(), (kernel, R.key(cases[i]), "bits set outside the codeword")
    return raw


def _of(cases, bg, keep=lambda c: True):
    return [i for i, c in enumerate(cases) if c["bg"] == bg and keep(c)]


@pytest.mark.parametrize("bg", [1, 2])
def test_byte_kernel_grid(ctx, grid, bg):
    """Every shape of a base graph in one plan, all codeblocks on the byte kernel."""
    cases, tbs, want = grid
    assert len(_of(cases, bg)) > 3000
    _RAW[bg, "byte"] = _run(ctx, cases, tbs, want, _of(cases, bg), "byte")


@pytest.mark.parametrize("bg", [1, 2])
def test_default_kernel_grid(ctx, grid, bg):
    """The same plan with the plan's own choice: the packed shapes on the packed kernel, next to the byte kernel's.
    Bit-exact against the oracle and byte for byte what the byte kernel alone wrote."""
    cases, tbs, want = grid
    idx = _of(cases, bg)
    assert {R.census(cases[i])["kernel"] for i in idx} == {"byte", "packed"}
    raw = _run(ctx, cases, tbs, want, idx, "default")
    if (bg, "byte") not in _RAW:
        _RAW[bg, "byte"] = _run(ctx, cases, tbs, want, idx, "byte")
    assert np.array_equal(raw, _RAW[bg, "byte"])


@pytest.mark.parametrize("bg", [1, 2])
def test_packed_shapes_plan_hygiene(ctx, grid, bg):
    """The packed shapes alone (TB CRCs computed by the packed kernel's own workgroups), the TB buffer ending on the
    last TB's last byte, TB offsets 0 to 3 modulo 4 rotated over the TBs: at every rv, Qm and Nref of the grid."""
    cases, tbs, want = grid
    idx = _of(cases, bg, lambda c: c["Z"] % 32 == 0)
    assert idx and all(R.census(cases[i])["kernel"] == "packed" for i in idx)
    _run(ctx, cases, tbs, want, idx, "default", tb_tail=0)


@pytest.mark.parametrize("kernel", ["byte", "default"])
@pytest.mark.parametrize("bg", [1, 2])
def test_output_zeroing(ctx, grid, bg, kernel):
    """The cases whose codeblocks are whole output words, back to back: the plan may skip zeroing the output, and both
    settings of encoder_zero_output give the same codewords. (The plans of the other tests are not word aligned and
    always zero.)"""
    cases, tbs, want = grid
    idx = _of(cases, bg, lambda c: c["nsym"] * c["qm"] % 32 == 0)
    assert len(idx) >= 50 and {cases[i]["qm"] for i in idx} == set(R.QMS)
    a = _run(ctx, cases, tbs, want, idx, kernel, gap=0, zero_output=0, tiled=True)
    b = _run(ctx, cases, tbs, want, idx, kernel, gap=0, zero_output=1, tiled=True)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("kernel", ["byte", "default"])
def test_multi_codeblock_list(ctx, multi, kernel):
    """Two and three codeblocks of different E whose neighbours share an output word: each TB alone and all in one
    plan."""
    cases, tbs, want = multi
    for i in range(len(cases)):
        _run(ctx, cases, tbs, want, [i], kernel)
    _run(ctx, cases, tbs, want, list(range(len(cases))), kernel)


@pytest.mark.parametrize("shape", [(1, 2), (2, 4), (1, 3)], ids=lambda s: "bg%d-z%d" % s)
def test_one_shape_per_plan(ctx, grid, shape):
    """A small shape alone in its plan, and every third of its cases alone in one: a launch of one tiny codeblock does not depend on
    what a neighbour left in LDS."""
    cases, tbs, want = grid
    idx = [i for i, c in enumerate(cases) if (c["bg"], c["Z"]) == shape]
    assert idx
    _run(ctx, cases, tbs, want, idx, "default")
    for i in idx[::3]:
        _run(ctx, cases, tbs, want, [i], "default")


@pytest.mark.parametrize("kernel", ["byte", "default"])
def test_reference_codewords(ctx, grid, multi, kernel):
    """The reference's own codewords of the GOLDEN_Z subset and of the multi-codeblock list, from the committed file."""
    cases, tbs, _ = grid
    idx = R.golden_subset(cases)
    keys, want = G.pdsch_encoder_regime_codewords()
    assert np.array_equal(keys, np.array([R.key_numbers(c) for c in [cases[i] for i in idx] + multi[0]], np.int64))
    for bg in (1, 2):
        _run(ctx, cases, tbs, dict(zip(idx, want)), [i for i in idx if cases[i]["bg"] == bg], kernel)
    _run(ctx, multi[0], multi[1], want[len(idx):], list(range(len(multi[0]))), kernel)
