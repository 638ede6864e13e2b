"""GPU parity of the PDSCH modulator with wideband precoding matrices that have (0, 0) entries: the plan records which
(port, layer) terms are not zero and the kernel computes only those (four layers on four ports with a diagonal matrix
as straight-line code, any other pattern through the mask); a matrix without zeros, one with an all-zero port row and
per-PRG weights keep every term. Grid words bit for bit against the oracle's modulator, whose sums run over every
layer: a skipped term is +/-0 and cannot change a sum that has a non-zero term.

Matrices: identity at L = P = 1..4, a scaled permutation, +/-j entries on a sparse pattern, rows with one to three
entries, negative zeros next to entries, dense, identity at L < P (all-zero rows: every term) and a PRG plan; contiguous
and general (RE map) allocations, every modulation order, several power scalings, all in one plan per test."""
import numpy as np
import pytest

from oracle_lib import Oracle, pdsch_modulate_general
from pdsch_mod_cases import crb_mask_test_side, random_config, random_general_config
from test_pdsch_modulator_gpu import to_general_mod, to_mod

pytestmark = pytest.mark.gpu

GRID_PRB = 24
GENERAL_PRB = 52


def _c(rows):
    return np.array(rows, dtype=np.complex64)


def matrices():
    """(name, P, L, weights (P x L))."""
    s = np.float32(0.5)
    out = [("identity%d" % n, n, n, np.eye(n, dtype=np.complex64)) for n in (1, 2, 3, 4)]
    out += [
        ("diagonal4", 4, 4, _c(np.diag([0.5, -1.25j, 0.7 + 0.1j, -0.3]))),
        ("permutation4", 4, 4, s * _c([[0, 0, 1, 0], [1, 0, 0, 0], [0, 0, 0, 1], [0, 1, 0, 0]])),
        ("permutation3", 3, 3, s * _c([[0, 1, 0], [0, 0, 1], [1, 0, 0]])),
        ("sparse_j", 4, 4, _c([[1j, 0, 0, -1j], [0, -1j, 0, 0], [0, 1j, 1j, 0], [-1j, 0, 0, 1j]])),
        ("rows123", 4, 4, _c([[0, 0, 0, 0.5], [0.5, 0, 0.25 - 0.5j, 0], [1, 1j, -1, 0], [0, 0.3, 0, 0]])),
        ("first_term_late", 4, 2, _c([[0, 1], [0, -1j], [0.5, 0.5], [0, 0.25]])),
        ("negative_zeros", 4, 4, _c([[1, -0.0, 0, complex(-0.0, -0.0)], [complex(0.0, -0.0), 1j, 0, 0],
                                     [0, 0, complex(-0.0, 1.0), 0], [0, 0, 0, complex(1.0, -0.0)]])),
        ("real_and_imaginary", 2, 2, _c([[1, 0], [0, 1j]])),
        ("dense4", 4, 4, _c([[1, 1, 1, 1], [1, -1j, -1, 1j], [1, -1, 1, -1], [1, 1j, -1, -1j]]) * s),
        ("identity_L2_P4", 4, 2, np.eye(4, 2, dtype=np.complex64)),   # ports 2 and 3 all zero: every term
        ("identity_L1_P2", 2, 1, np.eye(2, 1, dtype=np.complex64)),
        ("zero_row_between", 4, 4, _c([[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 1]])),
        ("all_zero", 2, 2, np.zeros((2, 2), np.complex64)),
    ]
    return out


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def contiguous_cases(orc):
    """Every matrix with every modulation order on contiguous allocations of random geometry: (PdschModulation,
    codeword, the oracle's grids, name)."""
    rng = np.random.default_rng(61)
    mods, cws, want, names = [], [], [], []
    for name, P, L, w in matrices():
        for qm in (2, 4, 6, 8):
            cfg, nbits, _ = random_config(rng, GRID_PRB, qm=qm, nof_layers=L, nof_ports=P)
            cw = rng.integers(0, 256, (nbits + 7) // 8).astype(np.uint8)
            g = np.zeros((4, 14, 12 * GRID_PRB, 2), np.uint16)
            orc.pdsch_modulate(cfg, w, cw, nbits, GRID_PRB, grid=g[:P])
            mods.append(to_mod(cfg, w))
            cws.append(cw)
            want.append(g)
            names.append((name, qm))
    return mods, cws, want, names


def general_cases(orc):
    """General allocations (the RE -> subcarrier map path) with the same matrices as wideband weights, and PRG plans,
    whose per-PRG weights (here with zeros as well) are not masked."""
    rng = np.random.default_rng(62)
    G_ = GENERAL_PRB
    mods, cws, want, names = [], [], [], []
    for name, P, L, w in matrices():
        for prg in (0, 4):
            cfg, nbits, _ = random_general_config(rng, G_, prg=prg)
            # The geometry of a random case with this matrix's ports and layers: the bit count follows the layers.
            nbits = nbits // cfg["nof_layers"] * L
            cfg.update(nof_layers=L, nof_ports=P)
            if prg:
                nof_prg = -(-G_ // prg)
                pw = np.repeat(w[None], nof_prg, axis=0).copy()
                pw[1::2] *= np.complex64(1j)   # another matrix on every second PRG, the same zeros
                cfg["prg_weights"] = pw
            crb = crb_mask_test_side(cfg, G_)
            cw = rng.integers(0, 256, (nbits + 7) // 8).astype(np.uint8)
            g = np.zeros((4, 14, 12 * G_, 2), np.uint16)
            pdsch_modulate_general(orc.lib, cfg, w, cw, nbits, G_, crb_mask=crb, grid=g[:P])
            mods.append(to_general_mod(cfg, w, crb, G_))
            cws.append(cw)
            want.append(g)
            names.append((name, prg))
    return mods, cws, want, names


def test_pdsch_modulator_sparse_weights(ctx, orc):
    """The contiguous cases in ONE plan."""
    import srsgpu
    mods, cws, want, names = contiguous_cases(orc)
    got = srsgpu.PdschModulator(ctx, GRID_PRB, 4).modulate_batch(cws, mods)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), names[i]


def test_pdsch_modulator_sparse_weights_general_and_prg(ctx, orc):
    """The general and PRG cases in ONE plan."""
    import srsgpu
    mods, cws, want, names = general_cases(orc)
    got = srsgpu.PdschModulator(ctx, GENERAL_PRB, 4).modulate_batch(cws, mods)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), names[i]
