"""Pins the numpy restatement of NZP-CSI-RS generation (tests/csi_rs_cases.py) to the reference's own
nzp_csi_rs_generator_impl as recorded in tests/golden/csi_rs.npz (tools/gen_csi_rs_golden.py), asserts what the fixture
has to contain so that the GPU tests cannot pass by leaving cases out, shows that the fixture sees each stage (a
restatement perturbed by hand differs), and checks the host construction of srsran-5g_amd/csrc/csi_rs_host.cpp in a
stand-alone sanitizer-built program. No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import csi_rs_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return list(C.golden_cases())


def test_restatement_equals_reference(cases):
    """Every written grid word of every fixture signal, exactly, and no other word."""
    for i, (cfg, rows) in enumerate(cases):
        assert C.refusal(cfg, cfg["grid_nof_prb"], cfg["grid_nof_ports"]) is None, i
        got = C.process(cfg)
        assert got.shape == rows.shape and np.array_equal(got, rows), (i, cfg)
        assert rows.shape[0] == C.seq_len(cfg) * len(C.groups(cfg)) * C.ROW_PORTS[cfg["row"]], i
        want = np.full((cfg["grid_nof_ports"], 14, 12 * cfg["grid_nof_prb"]), C.SENTINEL, np.uint32)
        C.apply_rows(want, rows)
        assert np.array_equal(C.expected_grid(cfg), want), i


def test_fixture_contents(cases):
    """What the fixture must hold."""
    kinds, k_refs, l0s, half, cps, zeros = set(), {}, {}, set(), set(), 0
    non_identity = scaled_single = top = other_group_zeros = False
    for cfg, rows in cases:
        row = cfg["row"]
        kinds.add((row, cfg["freq_density"], cfg["cdm"]))
        k_refs.setdefault(row, set()).add(cfg["k_ref"])
        l0s.setdefault(row, set()).add(cfg["symbol_l0"])
        cps.add(cfg["cp"])
        identity = np.array_equal(cfg["weights"], np.eye(C.ROW_PORTS[row]))
        non_identity |= row >= 3 and not identity and bool(np.all(cfg["weights"].real != 0) and np.all(cfg["weights"].imag != 0))
        scaled_single |= row <= 2 and not identity
        top |= cfg["start_rb"] + cfg["nof_rb"] == cfg["grid_nof_prb"]
        if cfg["freq_density"] in (C.DOT5_EVEN, C.DOT5_ODD):
            half.add((row, cfg["freq_density"], cfg["start_rb"] % 2, cfg["nof_rb"] % 2))
            zeros += C.seq_len(cfg) == 0 and rows.shape[0] == 0
        if row >= 4 and identity:
            # Finding: the mapper stores zeros on the ports of the other CDM group.
            other = rows[(rows[:, 0] >= 2) & (rows[:, 2] % 12 == cfg["k_ref"]) & (rows[:, 1] == cfg["symbol_l0"])]
            other_group_zeros |= other.shape[0] > 0 and bool(np.all((other[:, 3] & 0x7FFF7FFF) == 0))
    want = {(r, d, cdm) for r, (_, ds, cdm) in C.ROW_RULES.items() for d in ds}
    assert kinds == want and len(want) == 9
    for row, (ks, _, _) in C.ROW_RULES.items():
        assert {ks[0], ks[-1]} <= k_refs[row] and len(k_refs[row]) >= 3, row
        assert {0, 12 if row == 5 else 13} <= l0s[row] and len(l0s[row]) >= 4, row
    assert half == {(r, d, s, n) for r in (2, 3) for d in (C.DOT5_EVEN, C.DOT5_ODD) for s in (0, 1) for n in (0, 1)}
    assert zeros >= 2
    assert cps == {0, 1}  # the reference accepts extended CP: 12 symbols in c_init and the l_0 range
    assert non_identity and scaled_single and top and other_group_zeros
    assert any(cfg["grid_nof_prb"] == 273 for cfg, _ in cases)
    assert os.path.getsize(C.GOLDEN) < 243 << 10


PERTURBATIONS = {
    # w_f not applied: every FD-CDM2 signal that writes anything.
    "no_w_f": lambda cfg: cfg["cdm"] == C.FD_CDM2 and C.seq_len(cfg) > 0,
    # The skipped elements not doubled into bits: every signal that skips any. A sequence of at least 8 elements is asked
    # for: two Gold sequence windows of 16 bits or more at different offsets agree with probability 2^-16 or less, while
    # one element (two bits) would agree once in four.
    "skip_not_doubled": lambda cfg: C.skipped_elements(cfg) > 0 and C.seq_len(cfg) >= 8,
    # The density-0.5 comb on the other parity: every density-0.5 signal with an RB to write on either comb.
    "comb_parity": lambda cfg: cfg["freq_density"] in (C.DOT5_EVEN, C.DOT5_ODD) and cfg["nof_rb"] > 0,
}


@pytest.mark.parametrize("name", sorted(PERTURBATIONS))
def test_fixture_sees_each_stage(cases, name):
    """A restatement perturbed by hand differs from the fixture on every case the perturbation applies to."""
    applies = 0
    for i, (cfg, rows) in enumerate(cases):
        if not PERTURBATIONS[name](cfg):
            continue
        applies += 1
        got = C.process(cfg, perturb=name)
        assert got.shape != rows.shape or not np.array_equal(got, rows), (name, i, cfg)
    assert applies >= 12, (name, applies)


def test_refusals_of_the_restatement(cases):
    """Each rule refuses alone, in the plan's order."""
    by_row = {row: next(c for c, _ in cases if c["row"] == row and c["cp"] == 0) for row in range(1, 6)}
    for cfg, want in refusal_cases(by_row):
        assert C.refusal(cfg, 52, 4) == want, (cfg, want)
    for row in range(1, 6):
        assert C.refusal(dict(by_row[row], start_rb=40, nof_rb=12), 52, 4) is None


def refusal_cases(by_row):
    eye4 = np.eye(4, dtype=np.complex64)
    out = [(dict(by_row[1], row=0), "Invalid mapping table row"), (dict(by_row[1], row=19), "Invalid mapping table row"),
           (dict(by_row[1], row=13), "Unsupported mapping table row"), (dict(by_row[1], row=18), "Unsupported mapping table row")]
    out += [(dict(by_row[4], row=row), "grid ports") for row in range(6, 13)]
    out += [(dict(by_row[1], k_ref=4), "k_0"), (dict(by_row[2], k_ref=12), "k_0"), (dict(by_row[3], k_ref=11), "k_0"),
            (dict(by_row[4], k_ref=9), "k_0"), (dict(by_row[5], k_ref=11), "k_0"),
            (dict(by_row[1], freq_density=C.ONE), "invalid density"), (dict(by_row[2], freq_density=C.THREE), "invalid density"),
            (dict(by_row[3], freq_density=C.THREE), "invalid density"), (dict(by_row[4], freq_density=C.DOT5_EVEN), "invalid density"),
            (dict(by_row[5], freq_density=C.DOT5_ODD), "invalid density"),
            (dict(by_row[1], cdm=C.FD_CDM2), "invalid CDM type"), (dict(by_row[2], cdm=C.FD_CDM2), "invalid CDM type"),
            (dict(by_row[3], cdm=C.NO_CDM), "invalid CDM type"), (dict(by_row[4], cdm=C.CDM4), "invalid CDM type"),
            (dict(by_row[5], cdm=C.CDM8), "invalid CDM type"),
            (dict(by_row[2], symbol_l0=14), "l_0"), (dict(by_row[2], cp=1, numerology=2, symbol_l0=12), "l_0"),
            (dict(by_row[5], symbol_l0=13), "l_0 + 1"), (dict(by_row[5], cp=1, numerology=2, symbol_l0=11), "l_0 + 1"),
            (dict(by_row[3], weights=eye4), "precoding number of ports"),
            (dict(by_row[4], weights=eye4[:2, :2]), "precoding number of ports"),
            (dict(by_row[2], start_rb=40, nof_rb=13), "RBs"), (dict(by_row[2], start_rb=52, nof_rb=1), "RBs"),
            (dict(by_row[2], amplitude=C.F(np.inf)), "amplitude"), (dict(by_row[4], amplitude=C.F(np.nan)), "amplitude"),
            (dict(by_row[1], scrambling_id=1024), "scrambling_id")]
    return out


# The plan's message for each keyword of the restatement's refusals.
MESSAGES = {"Invalid mapping table row": "Invalid mapping table row", "Unsupported mapping table row": "Unsupported mapping table row",
            "grid ports": "grid ports and the grids of this library have at most 4", "k_0": "k_0", "invalid density": "invalid density",
            "invalid CDM type": "invalid CDM type", "l_0": "l_0, i.e.,", "l_0 + 1": "l_0 + 1", "precoding number of ports":
            "does not match the precoding number of ports", "grid number of ports": "exceeds the grid number of ports",
            "RBs": "exceed the grid", "amplitude": "amplitude is not finite", "scrambling_id": "scrambling_id",
            "k_ref count": "1 k_ref is needed", "enumeration": "enumeration"}


def record(cfg, grid_nof_prb, grid_nof_ports, tail):
    ports = np.asarray(cfg["weights"]).shape[0]
    return struct.pack("<16If", cfg["n_slot"], cfg["cp"], cfg["start_rb"], cfg["nof_rb"], cfg["row"], cfg["k_ref"],
                       cfg["symbol_l0"], cfg["symbol_l1"], cfg["cdm"], cfg["freq_density"], cfg["scrambling_id"], ports,
                       grid_nof_prb, grid_nof_ports, tail[0], tail[1], float(cfg["amplitude"]))


def test_host_construction(tmp_path, cases):
    """csi_rs_layout_of against the REs the reference wrote, the restatement's sequence length, skipped elements, c_init
    and amplitude for every fixture signal; every refusal with its message; and arbitrary field values, in a stand-alone
    program built with the address and undefined-behaviour sanitizers."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "csi_rs_host_check")
    csrc = os.path.join(ROOT, "srsran-5g_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{csrc}", "-o", exe, os.path.join(csrc, "csi_rs_host.cpp"),
                    os.path.join(ROOT, "tools", "csi_rs_host_check.cpp")], check=True)
    by_row = {row: next(c for c, _ in cases if c["row"] == row and c["cp"] == 0) for row in range(1, 6)}
    refusals = [(cfg, 52, 4, 1, MESSAGES[want]) for cfg, want in refusal_cases(by_row)]
    refusals += [(by_row[3], 52, 1, 1, MESSAGES["grid number of ports"]), (by_row[5], 52, 3, 1, MESSAGES["grid number of ports"]),
                 (by_row[1], 52, 4, 0, MESSAGES["k_ref count"]), (by_row[4], 52, 4, 2, MESSAGES["k_ref count"]),
                 (dict(by_row[1], cp=2), 52, 4, 1, MESSAGES["enumeration"]), (dict(by_row[1], cdm=4), 52, 4, 1, MESSAGES["enumeration"]),
                 (dict(by_row[1], freq_density=4), 52, 4, 1, MESSAGES["enumeration"])]
    dump = tmp_path / "csi_rs.bin"
    with open(dump, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for cfg, rows in cases:
            f.write(record(cfg, cfg["grid_nof_prb"], cfg["grid_nof_ports"], (C.seq_len(cfg), C.skipped_elements(cfg))))
            port0 = rows[rows[:, 0] == 0]
            res = np.stack([port0[:, 1], port0[:, 2], [C.c_init(cfg, int(l)) for l in port0[:, 1]]], axis=1) \
                if port0.shape[0] else np.zeros((0, 3))
            f.write(struct.pack("<I", res.shape[0]))
            f.write(res.astype(np.uint32).tobytes())
        f.write(struct.pack("<I", len(refusals)))
        for cfg, prb, ports, nof_k_ref, text in refusals:
            f.write(record(cfg, prb, ports, (nof_k_ref, 0)))
            f.write(struct.pack("<I", len(text)) + text.encode())
    res = subprocess.run([exe, str(dump)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"{len(cases)} signals, {len(refusals)} refusals" in res.stdout and " 0 failures" in res.stdout
