"""Pins the numpy restatement of the SS/PBCH block (tests/ssb_cases.py) to the reference's own ssb_processor_impl as
recorded in tests/golden/ssb.npz (tools/gen_ssb_golden.py), asserts what the fixture has to contain so that the GPU tests
cannot pass by leaving cases out, shows that the fixture sees each stage (a restatement perturbed by hand differs), and
checks the host construction of srsran-5g_amd/csrc/ssb_host.cpp and the (56, 864) downlink polar code of polar_code.cpp
in a stand-alone sanitizer-built program. No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import ssb_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return list(C.golden_cases())


def test_restatement_equals_reference(cases):
    """l_start, k_start, the 864 rate-matched bits and every written grid word of every fixture block, exactly, and no
    other word: 830 per port (127 PSS, 127 SSS, 432 PBCH, 144 DM-RS)."""
    for i, (cfg, l_start, k_start, encoded, rows) in enumerate(cases):
        assert C.refusal(cfg, cfg["grid_nof_prb"], cfg["grid_nof_ports"]) is None, i
        l0, k0, bits, got = C.process(cfg)
        assert (l0, k0) == (l_start, k_start), (i, cfg)
        assert np.array_equal(bits, encoded), (i, cfg)
        assert got.shape == rows.shape and np.array_equal(got, rows), (i, cfg)
        assert rows.shape[0] == 830 * len(cfg["ports"]) and set(rows[:, 0]) == set(cfg["ports"]), i
        assert np.float32(10 ** (np.float64(cfg["beta_pss_dB"]) / 20)) == cfg["pss_amplitude"], i
        want = np.full((cfg["grid_nof_ports"], 14, 12 * cfg["grid_nof_prb"]), C.SENTINEL, np.uint32)
        C.apply_rows(want, rows)
        assert np.array_equal(C.expected_grid(cfg), want), i
        # The reference leaves symbol l_start outside the PSS and the gaps beside the SSS untouched.
        first = rows[(rows[:, 0] == cfg["ports"][0])]
        assert set(first[first[:, 1] == l_start][:, 2] - k_start) == set(range(56, 183)), i
        assert set(first[first[:, 1] == l_start + 2][:, 2] - k_start) == set(range(48)) | set(range(56, 183)) | set(range(192, 240)), i


def test_fixture_contents(cases):
    """What the fixture must hold."""
    kinds, hrfs, vs, ids, ports, amps = set(), set(), set(), set(), set(), set()
    k_low = k_high = idx8 = top = False
    for cfg, _l, k_start, _enc, _rows in cases:
        kinds.add((cfg["pattern_case"], cfg["L_max"]))
        hrfs.add((cfg["L_max"], cfg["hrf"]))
        vs.add(cfg["phys_cell_id"] % 4)
        ids.add(cfg["phys_cell_id"])
        ports.add(tuple(cfg["ports"]))
        amps.add(float(cfg["pss_amplitude"]))
        k_low |= cfg["pattern_case"] < C.CASE_D and 0 < cfg["subcarrier_offset"] < 16
        k_high |= cfg["pattern_case"] < C.CASE_D and cfg["subcarrier_offset"] >= 16
        idx8 |= cfg["ssb_idx"] >= 8
        top |= k_start + 240 == 12 * cfg["grid_nof_prb"]
    assert {c for c, _ in kinds} == {C.CASE_A, C.CASE_B, C.CASE_C, C.CASE_D, C.CASE_E}
    assert {l for _, l in kinds} == {4, 8, 64}
    assert hrfs == {(l, h) for l in (4, 8, 64) for h in (0, 1)}
    assert vs == {0, 1, 2, 3} and {0, 1007} <= ids
    assert {len(p) for p in ports} == {1, 2, 3, 4} and any(list(p) != list(range(p[0], p[0] + len(p))) for p in ports)
    assert amps == {1.0, float(np.float32(10 ** (3 / 20)))}
    assert k_low and k_high and idx8 and top
    assert any(cfg["ssb_idx"] & 7 for cfg, *_ in cases) and any(cfg["ssb_idx"] & 7 == 0 for cfg, *_ in cases)
    assert os.path.getsize(C.GOLDEN) < 243 << 10


PERTURBATIONS = {
    # Second scrambling not advanced by ssb_idx: every block whose index has one of its three LSBs set.
    "no_ssb_idx_advance": lambda cfg: cfg["ssb_idx"] & 7 != 0,
    # The HRF position scrambled: every block (the position takes a sequence bit and moves all later ones by one).
    "hrf_scrambled": lambda cfg: True,
    # v off by one: every block (the DM-RS moves to other subcarriers).
    "v_off_by_one": lambda cfg: True,
    # c_init of L_max = 4 without the half frame bit: every L_max = 4 block of the second half frame.
    "c_init_without_hrf": lambda cfg: cfg["L_max"] == 4 and cfg["hrf"] == 1,
}


@pytest.mark.parametrize("name", sorted(PERTURBATIONS))
def test_fixture_sees_each_stage(cases, name):
    """A restatement perturbed by hand differs from the fixture on every case the perturbation applies to."""
    applies = 0
    for i, (cfg, _l, _k, encoded, rows) in enumerate(cases):
        if not PERTURBATIONS[name](cfg):
            continue
        applies += 1
        _, _, bits, got = C.process(cfg, perturb=name)
        assert not np.array_equal(got, rows), (name, i, cfg)
        if name == "hrf_scrambled":
            assert not np.array_equal(bits, encoded), (name, i, cfg)
    assert applies >= 5, (name, applies)


def refusal_cases(base):
    """(cfg, grid PRBs, grid ports, restatement's keyword, text of the plan's message)."""
    a = base[C.CASE_A]
    e = base[C.CASE_E]
    return [(dict(a, pattern_case=5), 52, 4, "pattern case", "Invalid SSB pattern case"),
            (dict(a, L_max=5), 52, 4, "L_max", "is not 4, 8 or 64"), (dict(a, L_max=0), 52, 4, "L_max", "is not 4, 8 or 64"),
            (dict(a, ssb_idx=a["L_max"]), 52, 4, "ssb_idx", "is not below L_max"),
            (dict(e, ssb_idx=64), 52, 4, "ssb_idx", "is not below L_max"),
            (dict(a, phys_cell_id=1008), 52, 4, "phys_cell_id", "exceeds 1007"),
            (dict(a, common_scs=3), 52, 4, "Common SCS", "Unsupported combination of FR1 and Common SCS"),
            (dict(e, common_scs=1), 52, 4, "Common SCS", "Unsupported combination of FR2 and Common SCS"),
            (dict(a, offset_to_pointA=2200), 275, 4, "offset to Point A", "Invalid offset to Point A"),
            (dict(a, subcarrier_offset=24), 52, 4, "subcarrier offset", "Invalid subcarrier offset 24 for FR1"),
            (dict(e, subcarrier_offset=12), 52, 4, "subcarrier offset", "Invalid subcarrier offset 12 for FR2"),
            (dict(base[C.CASE_B], offset_to_pointA=2, subcarrier_offset=3), 52, 4, "Unsupported combination", "offsetToPointA 2 and"),
            (dict(e, common_scs=2, offset_to_pointA=1, subcarrier_offset=2), 52, 4, "Unsupported combination", "offsetToPointA 1 and"),
            (dict(a, slot_index=a["slot_index"] + 1), 52, 4, "slot index", "Invalid slot index"),
            (dict(a, hrf=2), 52, 4, "hrf", "is not 0 or 1"),
            (dict(e, ssb_idx=1, slot_index=0), 52, 4, "symbols", "exceed the slot"),
            (dict(e, ssb_idx=6, slot_index=2), 52, 4, "symbols", "exceed the slot"),
            (dict(a, offset_to_pointA=32, subcarrier_offset=1), 52, 4, "subcarriers", "exceed the grid"),
            (dict(a, offset_to_pointA=32, subcarrier_offset=0), 51, 4, "subcarriers", "exceed the grid"),
            (dict(a, ports=[]), 52, 4, "number of ports", "outside 1..4"),
            (dict(a, ports=[0, 1, 2, 3, 0]), 52, 4, "number of ports", "outside 1..4"),
            (dict(a, ports=[0, 4]), 52, 4, "port outside", "is outside the grid"),
            (dict(a, ports=[1]), 52, 1, "port outside", "is outside the grid"),
            (dict(a, ports=[2, 0, 2]), 52, 4, "port twice", "listed twice"),
            (dict(a, pss_amplitude=np.float32(np.inf)), 52, 4, "pss_amplitude", "pss_amplitude is not finite")]


@pytest.fixture(scope="module")
def base(cases):
    return {case: next(dict(c) for c, *_ in cases if c["pattern_case"] == case and c["grid_nof_prb"] == 52)
            for case in range(5)}


def test_refusals_of_the_restatement(base):
    """Each rule refuses alone, in the plan's order."""
    for cfg, prb, ports, want, _text in refusal_cases(base):
        assert C.refusal(cfg, prb, ports) == want, (cfg, want)
    assert C.refusal(dict(base[C.CASE_A], offset_to_pointA=32, subcarrier_offset=0), 52, 4) is None


def record(cfg, grid_nof_prb, grid_nof_ports):
    ports = list(cfg["ports"])
    return struct.pack("<12IfI4B24B", cfg["phys_cell_id"], cfg["ssb_idx"], cfg["L_max"], cfg["pattern_case"], cfg["common_scs"],
                       cfg["offset_to_pointA"], cfg["subcarrier_offset"], cfg["sfn"], cfg["slot_index"], cfg["hrf"],
                       grid_nof_prb, grid_nof_ports, float(cfg["pss_amplitude"]), len(ports), *(ports + [0] * 4)[:4],
                       *[int(b) for b in cfg["payload"]])


def test_host_construction(tmp_path, cases, base):
    """For every fixture block: l_start, k_start and the DM-RS c_init, the 864 bits encoded in plain C++ from the
    descriptor and tables the plan uploads (payload layout, first scrambling masks, CRC weights, the (56, 864) code of
    polar_dl_code_build) against the reference's, and the PSS / SSS signs against the fixture's words; every refusal
    with its message; and arbitrary field values, in a stand-alone program built with the address and
    undefined-behaviour sanitizers."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "ssb_host_check")
    csrc = os.path.join(ROOT, "srsran-5g_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{csrc}", "-o", exe, os.path.join(csrc, "polar_code.cpp"), os.path.join(csrc, "ssb_host.cpp"),
                    os.path.join(ROOT, "tools", "ssb_host_check.cpp")], check=True)
    refusals = refusal_cases(base)
    dump = tmp_path / "ssb.bin"
    with open(dump, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for cfg, l_start, k_start, encoded, rows in cases:
            f.write(record(cfg, cfg["grid_nof_prb"], cfg["grid_nof_ports"]))
            f.write(struct.pack("<3I", l_start, k_start, C.dmrs_c_init(cfg)))
            f.write(np.packbits(encoded).tobytes())
            first = rows[rows[:, 0] == cfg["ports"][0]]
            pss = first[(first[:, 1] == l_start)][:, 3]
            sss = first[(first[:, 1] == l_start + 2) & (first[:, 2] >= k_start + 56) & (first[:, 2] < k_start + 183)][:, 3]
            assert pss.size == 127 and sss.size == 127
            for signs in ((pss >> 15) & 1, (sss >> 15) & 1, (sss >> 31) & 1):
                f.write(signs.astype(np.uint8).tobytes())
        f.write(struct.pack("<I", len(refusals)))
        for cfg, prb, ports, _want, text in refusals:
            f.write(record(cfg, prb, ports) if len(cfg["ports"]) <= 4 else record_with_count(cfg, prb, ports))
            f.write(struct.pack("<I", len(text)) + text.encode())
    res = subprocess.run([exe, str(dump)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"{len(cases)} blocks, {len(refusals)} refusals" in res.stdout and " 0 failures" in res.stdout


def record_with_count(cfg, grid_nof_prb, grid_nof_ports):
    """A record whose port count exceeds the four ports it can list."""
    raw = bytearray(record(dict(cfg, ports=list(cfg["ports"])[:4]), grid_nof_prb, grid_nof_ports))
    raw[52:56] = struct.pack("<I", len(cfg["ports"]))
    return bytes(raw)
