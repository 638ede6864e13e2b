"""What the regime grid (tests/ldpc_regime_cases.py) reaches, measured with the CPU oracle alone (its census counters and
its deliberate defects, oracle.cpp orc_ldpc_decode_census): the layer counts, the arithmetic regimes, the outcomes of
the LLR families and the sensitivity of the inputs to eight hand-made decoder errors. The GPU tests that decode the
same grid (tests/test_ldpc_decoder_regimes_gpu.py) inherit these properties. No GPU, no reference build.

The floors are fixed; when one is missed the inputs change, not the floor."""
import numpy as np
import pytest

import ldpc_regime_cases as R
from oracle_lib import BG_K, BG_N_SHORT, CEN, CENSUS, DEFECTS, LIFTING_SIZES, Oracle

MODES = [1, 0]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def grid(orc):
    return R.grid_with_results(orc)


def _share(cen, name, of):
    return float(cen[:, CEN[name]].sum()) / float(cen[:, CEN[of]].sum())


def test_grid_shape(grid):
    """612 family codeblocks and 612 two-iteration codeblocks; every input ends in a non-zero LLR; families rotate over
    lengths and sizes; fillers on every second shape."""
    cases, _ = grid
    assert len(cases) == 2 * 612
    assert [c["kind"] for c in cases[:4]] == ["family", "two_iter"] * 2
    assert all(c["llr"][-1] != 0 and c["llr"].dtype == np.int8 for c in cases)
    fam = [c for c in cases if c["kind"] == "family"]
    for k, c in enumerate(fam):
        assert c["family"] == R.FAMILIES[(k // 6 + c["li"]) % 6] and c["li"] == k % 6
        assert (c["filler"] > 0) == bool((k // 6) % 2)
        assert c["llr"].size == R.lengths(c["bg"], c["Z"])[c["li"]][0]
    for li in range(6):
        assert {c["family"] for c in fam if c["li"] == li} == set(R.FAMILIES)
    for Z in LIFTING_SIZES:
        assert len({c["family"] for c in fam if c["Z"] == Z}) == 6
    assert all(c["crc_poly"] < 0 and c["max_iter"] == 2 for c in cases if c["kind"] == "two_iter")
    sat = [c["crc_poly"] >= 0 for c in fam if c["family"] == "saturated"]
    assert 0.4 < sum(sat) / len(sat) < 0.6


@pytest.mark.parametrize("mode", MODES)
def test_layer_counts(grid, mode):
    """Condition 1: every (BG, Z) has codeblocks that run exactly 4, 8, 9, 16, 17 and all M layers, counted by the
    oracle (not derived from the input length), of the family and of the two-iteration kind."""
    cases, res = grid
    cen = res[mode][1]
    for kind in ("family", "two_iter"):
        seen = {}
        for c, row in zip(cases, cen):
            if c["kind"] == kind:
                assert int(row[CEN["layers"]]) == c["layers"]
                seen.setdefault((c["bg"], c["Z"]), set()).add(int(row[CEN["layers"]]))
        assert len(seen) == 102
        for (bg, Z), s in seen.items():
            assert s == {4, 8, 9, 16, 17, BG_N_SHORT[bg] + 2 - BG_K[bg]}, (bg, Z, s)


FLOORS = [("v2c_inf", "edges", 0.05), ("row_capped", "rows", 0.03), ("row_one_finite", "rows", 0.02),
          ("row_tie", "rows", 0.03), ("v2c_zero", "edges", 0.005), ("cancel", "edges", 5e-4), ("promote", "edges", 5e-3),
          ("conflict", "edges", 5e-3), ("v2c_clamp", "edges", 2e-4)]


@pytest.mark.parametrize("mode", MODES)
def test_regime_floors(grid, mode):
    """Condition 2: the share of edges / check rows of the grid in each regime, per mode, and every counter non-zero
    within each layer class. A positive minimum scaled to 0 exists in the SIMD arithmetic only (floor(0.8 * 1) = 0;
    the generic one rounds to nearest, and round(sf * 1) >= 1 for every admissible sf >= 0.5)."""
    cases, res = grid
    cen = res[mode][1]
    got = {name: _share(cen, name, of) for name, of, _ in FLOORS}
    got["min_to_zero"] = _share(cen, "min_to_zero", "rows")
    blocked = int((cen[:, CEN["stop_blocked"]] > 0).sum())
    print(mode, got, "blocked codeblocks", blocked, dict(zip(CENSUS, cen.sum(0).tolist())))
    for name, _, floor in FLOORS:
        assert got[name] >= floor, (name, got[name])
    if mode == 1:
        assert got["min_to_zero"] >= 0.02
    else:
        assert got["min_to_zero"] == 0
    assert blocked >= 3
    assert int(cen[:, CEN["input_clamp"]].sum()) > 0
    for cls in (8, 16, 0):
        sel = np.array([R.layer_class(c["bg"], c["layers"]) == cls for c in cases])
        for name in CENSUS:
            if name == "min_to_zero" and mode == 0:
                continue
            assert int(cen[sel][:, CEN[name]].sum()) > 0, (cls, name)


def test_family_outcomes(grid):
    """Condition 3: unit-amplitude noiseless codewords never decode in the SIMD arithmetic (no message moves) and
    decode at iteration 1 in the generic one, at every shape; every other family with a CRC has at least 15 % decoded
    and 15 % failed in one mode; every layer class shows at least 3 distinct stop iterations."""
    cases, res = grid
    for fam in R.FAMILIES:
        sel = [i for i, c in enumerate(cases) if c["family"] == fam and c["crc_poly"] >= 0]
        its = {mode: [res[mode][0][i][0] for i in sel] for mode in MODES}
        if fam == "unit":
            assert len({(cases[i]["bg"], cases[i]["Z"]) for i in sel}) == len(sel) == 102
            assert all(x is None for x in its[1])
            assert all(x == 1 for x in its[0])
            continue
        assert len(sel) >= 50
        ok = {mode: sum(x is not None for x in its[mode]) / len(sel) for mode in MODES}
        print(fam, len(sel), ok)
        assert any(0.15 <= ok[mode] <= 0.85 for mode in MODES), (fam, ok)
    for mode in MODES:
        for cls in (8, 16, 0):
            stops = {res[mode][0][i][0] for i, c in enumerate(cases)
                     if c["crc_poly"] >= 0 and R.layer_class(c["bg"], c["layers"]) == cls}
            assert len(stops - {None}) >= 3 and None in stops, (mode, cls, stops)


@pytest.mark.parametrize("mode", MODES)
def test_defect_sensitivity(orc, grid, mode):
    """Condition 4: each deliberate decoder error changes the bits or the iteration count of at least 5 codeblocks, and
    skipping the last layer changes a codeblock of every (BG, Z, length) that runs more than 4 layers."""
    cases, res = grid
    want = res[mode][0]
    changed = {}
    for d in range(1, len(DEFECTS)):
        hit = []
        for i, c in enumerate(cases):
            r, bits, _ = R.decode(orc, mode, c, d)
            if (None if r < 0 else r) != want[i][0] or not np.array_equal(bits, want[i][1]):
                hit.append(i)
        changed[DEFECTS[d]] = hit
    print(mode, {k: len(v) for k, v in changed.items()})
    for name, hit in changed.items():
        assert len(hit) >= 5, (name, len(hit))
    cells = {(cases[i]["bg"], cases[i]["Z"], cases[i]["li"]) for i in changed["skip_last"] if cases[i]["li"] > 0}
    assert len(cells) == 102 * 5, sorted(set((c["bg"], c["Z"], c["li"]) for c in cases if c["li"]) - cells)


def test_defect_zero_is_the_decoder(orc, grid):
    """ldpc_decode and ldpc_decode_census(defect=0) are one decoder."""
    cases, res = grid
    for mode in MODES:
        for i in range(0, len(cases), 7):
            c = cases[i]
            r, bits = orc.ldpc_decode(mode, c["bg"], c["Z"], c["llr"], nof_crc_bits=c["nof_crc_bits"],
                                      nof_filler=c["filler"], crc_poly=c["crc_poly"], max_iter=c["max_iter"],
                                      scaling=c["sf"])
            assert (None if r < 0 else r) == res[mode][0][i][0] and np.array_equal(bits, res[mode][0][i][1])


def test_scaling_sweep(orc):
    """The sweep's shapes and factors, both families, in the 8-layer and the all-layers class, with failures and
    several stop iterations in each mode."""
    cases, res = R.sweep_with_results(orc)
    assert len(cases) == 4 * 2 * 2 * 5
    assert {(c["bg"], c["Z"]) for c in cases} == set(R.SWEEP_SHAPES)
    assert {c["sf"] for c in cases} == set(R.SWEEP_FACTORS) and {c["family"] for c in cases} == {"low", "two_valued"}
    for mode in MODES:
        its = [r[0] for r in res[mode][0]]
        assert None in its and len(set(its)) >= 4, its
        cen = res[mode][1]
        assert int(cen[:, CEN["row_tie"]].sum()) > 0
