"""The PDSCH encoder's regime grid (tests/pdsch_encoder_regime_cases.py) held to its floors with the census alone, and
shown to tell a wrong encoder from a right one: a numpy restatement of bit selection and interleaving over the oracle's
full codeblock equals the oracle's rate matcher on every case, and each of seven hand-made errors in it changes the
codeword on at least one case of every shape on which the error's class is reachable. CPU only.

ERROR_COUNTS holds, per error, (cases changed, shapes changed) of the last run; DESIGN.md records them."""
import collections

import numpy as np
import pytest

import pdsch_encoder_regime_cases as R
from chain_lib import oracle_pdsch_encode
from oracle_lib import LIFTING_SIZES, Oracle

# Hand-made errors and the class of cases each one needs.
ERRORS = {
    "a_last_ext_column": "any_ext",            # the last extension column read is stale: n_ext one short
    "b_kmax_without_filler_skip": "filler_skip_moves_n_ext",
    "c_v0_before_fillers": "k0_in_filler",     # v0 = k0 - filler inside the filler range
    "d_window_across_ninfo": "window_straddles_ninfo",
    "e_window_across_wrap": "window_straddles_wrap",
    "f_ncb_whole_columns": "partial_and_multi_wrap",  # Ncb rounded down to a multiple of Z
    "g_single_wrap": "multi_wrap",             # if (v >= V) v -= V
}
ERROR_COUNTS = {}


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def grid():
    cases = R.build_grid()
    return cases, [R.census(c) for c in cases]


def _shapes(cases, cen, cls, qm=None):
    return {(c["bg"], c["Z"]) for c, k in zip(cases, cen) if k[cls] and (qm is None or c["qm"] == qm)}


def test_shapes_and_fillers(grid):
    """All 51 lifting sizes for BG1, all but 2, 3, 5, 9 and 13 for BG2; two TB sizes per shape, the smaller with
    fillers, and a filler-free one on at least 36 BG1 and 20 BG2 shapes."""
    cases, cen = grid
    shapes = R.single_codeblock_shapes()
    assert sorted(z for b, z in shapes if b == 1) == LIFTING_SIZES
    assert sorted(z for b, z in shapes if b == 2) == [z for z in LIFTING_SIZES if z not in (2, 3, 5, 9, 13)]
    assert {(c["bg"], c["Z"]) for c in cases} == set(shapes) and len(shapes) == 97
    zero = collections.Counter()
    for (bg, Z), (lo, hi) in shapes.items():
        mine = [(c, k) for c, k in zip(cases, cen) if (c["bg"], c["Z"]) == (bg, Z)]
        assert {c["tb_bytes"] for c, _ in mine} == {lo, hi}, (bg, Z)
        assert all(k["Z"] == Z and k["kernel"] == ("packed" if Z % 32 == 0 else "byte") for _, k in mine), (bg, Z)
        assert any(k["filler"] > 0 for _, k in mine), (bg, Z)
        zero[bg] += any(k["filler"] == 0 for _, k in mine)
    assert zero[1] >= 36 and zero[2] >= 20, zero
    assert {c["layers"] for c in cases} == {1} and {c["qm"] for c in cases} == set(R.QMS)
    assert len(cases) <= 9000  # the cap that keeps the GPU tests at seconds


def test_every_class_on_every_shape(grid):
    cases, cen = grid
    shapes = set(R.single_codeblock_shapes())
    packed = {s for s in shapes if s[1] % 32 == 0}
    assert len(packed) == 24
    for cls in R.CLASSES + list(R.PAIRS):
        got = _shapes(cases, cen, cls)
        if cls == "k0_in_filler":
            # Needs fillers over more than 3 Z (BG1, rv 1 or 3) or Z (BG2 under LBRM, rv 3): small Z and BG2 with Kb < 10.
            assert len(got) >= 30 and {(2, 32), (2, 64)} <= got, sorted(got)
            assert {k["kernel"] for k in cen if k[cls]} == {"byte", "packed"}
        elif cls in R.PACKED_ONLY:
            assert got == packed, (cls, sorted(packed - got))
        else:
            assert got == shapes, (cls, sorted(shapes - got))
    # Every edge is hit exactly (Qm = 1) on every shape.
    for cls in ("wrap", "multi_wrap", "exact_fit", "ends_in_systematic", "ends_on_column_last_bit",
                "ends_on_column_first_bit"):
        assert _shapes(cases, cen, cls, qm=1) == shapes, (cls, sorted(shapes - _shapes(cases, cen, cls, qm=1)))
    # Extension rows: none, one, two and all of them on every shape.
    for bg, Z in shapes:
        n_ext = {k["n_ext"] for c, k in zip(cases, cen) if (c["bg"], c["Z"]) == (bg, Z)}
        assert {0, 1, 2, (46 if bg == 1 else 42) - 4} <= n_ext, (bg, Z, sorted(n_ext))


# Pairs that cannot occur: rv 0 starts at 0; the full buffer and a multiple of Z are no partial column.
IMPOSSIBLE = {("k0_in_filler", 0), ("lbrm", "full"), ("ncb_partial_column", "full"),
              ("ncb_partial_column", "lbrm_multiple")}


def test_class_by_rv_kind_and_qm(grid):
    cases, cen = grid
    for cls in R.CLASSES:
        hit = [(c, k) for c, k in zip(cases, cen) if k[cls]]
        for rv in range(4):
            assert (cls, rv) in IMPOSSIBLE or any(c["rv"] == rv for c, _ in hit), (cls, rv)
        for kind in R.KINDS:
            assert (cls, kind) in IMPOSSIBLE or any(c["kind"] == kind for c, _ in hit), (cls, kind)
        # The packed kernel: no class empty, and every Qm at which the class can occur, on every packed shape.
        for bg, Z in sorted({(c["bg"], c["Z"]) for c, k in hit if k["kernel"] == "packed"}):
            for qm in R.QMS:
                assert not R.can_occur(cls, Z, qm) or any((c["bg"], c["Z"], c["qm"]) == (bg, Z, qm) for c, _ in hit), \
                    (cls, bg, Z, qm)
        nof_packed = len({(c["bg"], c["Z"]) for c, k in hit if k["kernel"] == "packed"})
        assert nof_packed >= 2 if cls == "k0_in_filler" else nof_packed == 24, (cls, nof_packed)
        # Both kernels at every Qm for the classes that are not the packed kernel's own.
        if cls not in R.PACKED_ONLY:
            for qm in R.QMS:
                assert any(c["qm"] == qm and k["kernel"] == "byte" for c, k in hit), (cls, qm)


def test_multi_codeblock_list():
    cases = R.build_multi()
    for c, (nb, bg, C, Z) in zip(cases[::2], R.MULTI):
        seg, _ = R.codeblock(c)
        assert (seg.nof_segments, seg.lifting_size, c["tb_bytes"], c["bg"]) == (C, Z, nb, bg) and Z >= 208
    for bg in (1, 2):
        mine = [c for c in cases if c["bg"] == bg]
        assert {c["rv"] for c in mine} == {0, 3} and {c["qm"] for c in mine} == {1, 2, 6}
        assert any(R.census(c)["lbrm"] for c in mine)
        assert {c["codeblocks"] for c in mine} == {2, 3}
        assert {R.census(c)["kernel"] for c in mine} == {"byte", "packed"}
    for c in cases:
        seg, _ = R.codeblock(c)
        assert c["nsym"] % seg.nof_segments and len({cb.rm_length for cb in seg.codeblocks}) > 1, R.key(c)
    E = [cb.rm_length for c in cases for cb in R.codeblock(c)[0].codeblocks]
    off = [cb.cw_offset for c in cases for cb in R.codeblock(c)[0].codeblocks]
    assert any(e % 32 for e in E) and any(o % 32 for o in off)


def restate(cb, k, err=None):
    """Bit selection and interleaving of the codeblock `cb` (N bits, the oracle's) for the census `k` of a case, with
    one of ERRORS made on purpose."""
    Z, K, F, E, qm, ninfo = (k[x] for x in ("Z", "K", "filler", "E", "qm", "ninfo"))
    v0, V = k["v0"], k["V"]
    if err == "c_v0_before_fillers" and k["k0_in_filler"]:
        v0 = k["k0"] - F
    if err == "f_ncb_whole_columns":
        g = R.geometry(k["bg"], Z, F, k["rv"], k["Ncb"] // Z * Z)
        v0, V = g["v0"], g["V"]
    v = v0 + np.arange(E)
    v = np.where(v >= V, v - V, v) if err == "g_single_wrap" else v % V
    p = np.where(v < ninfo, v, v + F)
    if err in ("d_window_across_ninfo", "e_window_across_wrap") and k["kernel"] == "packed":
        s, L = R.windows(E, qm, k["g0"])
        vs = (v0 + s) % V
        bad = (vs < ninfo) & (vs + L > ninfo) & (F > 0) if err[0] == "d" else vs + L > V
        for s_, L_, v_ in zip(s[bad], L[bad], vs[bad]):
            p[s_:s_ + L_] = v_ + (F if v_ >= ninfo else 0) + np.arange(L_)
    # Behind the codeblock lies whatever the memory holds: here the complement of the codeblock, repeated.
    src = np.concatenate([cb, 1 - np.resize(cb, 3 * cb.size)])
    stale = None
    if err == "a_last_ext_column" and k["n_ext"] >= 1:
        stale = (K + 4 + k["n_ext"] - 1 - 2) * Z, (K + 4 + k["n_ext"] - 2) * Z
    if err == "b_kmax_without_filler_skip" and E < V - v0:
        n_ext = max(0, (v0 + E - 1 + 2 * Z) // Z - (K + 4) + 1)
        stale = (K + 4 + n_ext - 2) * Z, cb.size
    if stale is not None:
        src[stale[0]:min(stale[1], cb.size)] ^= 1
    return src[p].reshape(qm, E // qm).T.ravel()


def test_grid_tells_wrong_encoders_from_the_right_one(orc, grid):
    cases, cen = grid
    blocks = {}
    changed = {e: collections.Counter() for e in ERRORS}
    reachable = {e: set() for e in ERRORS}
    for c, k in zip(cases, cen):
        tbk = (c["bg"], c["tb_bytes"])
        if tbk not in blocks:
            _, seg, msgs = oracle_pdsch_encode(orc, R.transport_block(c), c["bg"], 0, 1, 1, 0, 8)
            assert seg.lifting_size == c["Z"] and seg.nof_filler_bits == k["filler"]
            blocks[tbk] = orc.ldpc_encode(c["bg"], c["Z"], msgs[0])
            assert not blocks[tbk][k["ninfo"]:k["nsys"]].any()  # fillers are zeros in the codeblock
        cb = blocks[tbk]
        want = orc.rate_match(c["bg"], c["Z"], c["rv"], c["qm"], c["Nref"], k["filler"], cb, k["E"])
        assert np.array_equal(restate(cb, k), want), R.key(c)
        assert np.array_equal(R.expected(orc, c), want), R.key(c)
        for err, cls in ERRORS.items():
            if not (k["n_ext"] >= 1 if cls == "any_ext" else k[cls]):
                continue
            reachable[err].add((c["bg"], c["Z"]))
            if not np.array_equal(restate(cb, k, err), want):
                changed[err][c["bg"], c["Z"]] += 1
    for err in ERRORS:
        ERROR_COUNTS[err] = (sum(changed[err].values()), len(changed[err]))
        missing = sorted(reachable[err] - set(changed[err]))
        assert reachable[err] and not missing, (err, missing)
    print("hand-made errors (cases changed, shapes changed):", ERROR_COUNTS)
