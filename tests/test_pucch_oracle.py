"""The float64 restatement of the PUCCH Format 0 / 1 detectors (tests/pucch_cases.py) against the reference's own
results (tests/golden/pucch_detector.npz, made by tools/gen_pucch_golden.py from pucch_detector_format0 /
pucch_detector_format1 built from their sources), the properties of the fixture's inputs that the GPU tests lean on,
and the plan's host code in a stand-alone sanitizer build. No GPU.

Measured on the fixture, the largest relative deviation between the reference's float32 results and the restatement:
Format 0 detection metric 1.8e-4 (at 30 dB its noise sum 12 power - |corr|^2 / 12 is a difference of numbers a
thousand times larger), EPRE 4.3e-7, RSRP 8.3e-7; Format 1 detection metric 2.2e-6, EPRE 4.8e-7, RSRP 3.0e-6, noise
variance 1.6e-6 (the bf16 grid keeps it at 1e-3 of the EPRE or more even at 30 dB). The tolerances (tolerances()) are
ten times the measured figures, floored at 1e-4.

Eight Format 1 resources of the fixture are degenerate: every shift of every OCC the symbols can hold is in use and
survives the 10 dB pruning (4 symbols with both OCCs, the 84-entry resource), so the rebuilt DM-RS equals the received
one and the noise variance is what rounding leaves, 1e-14 of the EPRE in float32. There the noise variance, the SINR
and the detection metric (a finite number over rounding noise) are no numbers to compare; bits and status still are."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import pucch_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


rel, degenerate, measured_deviations, tolerances = C.rel, C.degenerate, C.measured_deviations, C.tolerances


@pytest.fixture(scope="module")
def restated():
    return C.restate_golden()


def test_restatement_against_the_fixture(restated):
    """Bits and status equal the reference's on every case; the metrics within the measured tolerance, which itself
    stays within the figures of the module docstring."""
    _, f0, f1 = C.golden()
    dev = measured_deviations(restated)
    print({k: f"{v:.2e}" for k, v in dev.items()})
    for c, r in zip(f0, restated[0]):
        assert (int(r["valid"]), r["sr"], *r["harq"]) == (c["status"], *c["bits"]), c["cfg"]
    count = 0
    for c, (res, _) in zip(f1, restated[1]):
        for (ics, occ, nof_bits), r, status, bits in zip(c["cfg"]["entries"], res, c["status"], c["bits"]):
            assert int(r["valid"]) == status and list(r["bits"][:nof_bits]) == list(bits[:nof_bits]), (c["cfg"], ics, occ)
            count += 1
    assert len(f0) >= 300 and len(f1) >= 150 and count >= 400
    limits = dict(f0_metric=3e-4, f0_epre=1e-6, f0_rsrp=2e-6, f1_metric=5e-6, f1_epre=1e-6, f1_rsrp=6e-6, f1_noise_var=4e-6)
    for key, limit in limits.items():
        assert dev[key] < limit, (key, dev[key])
    # The SINR the reference reports is its RSRP over its noise variance, where that is a number.
    for c in f1:
        if not degenerate(c):
            assert np.allclose(c["sinr"], c["rsrp"] / c["noise_var"], rtol=1e-5)
    assert sum(degenerate(c) for c in f1) <= 10


def test_transmitters_come_back_at_30_db():
    """At 30 dB the reference returns every message that was sent, valid; an entry nobody transmitted on next to
    strong ones stays invalid."""
    _, f0, f1 = C.golden()
    sent0 = silent = sent1 = 0
    for c in f0:
        if c["snr_class"] == C.CLASS_HIGH:
            code = int(c["sent"])
            want = (code & 1, (code >> 1) & 1, (code >> 2) & 1)
            assert c["status"] == 1 and tuple(int(b) for b in c["bits"]) == want, c["cfg"]
            sent0 += 1
    for c in f1:
        if c["snr_class"] != C.CLASS_HIGH:
            continue
        for (ics, occ, nof_bits), status, bits, code in zip(c["cfg"]["entries"], c["status"], c["bits"], c["sent"]):
            if code < 0:
                assert status == 0, (c["cfg"], ics, occ)
                silent += 1
            else:  # (the 84-entry resource runs at 12 dB per PUCCH, still far above its threshold)
                assert status == 1 and [int(b) for b in bits[:nof_bits]] == [(code >> i) & 1 for i in range(nof_bits)]
                sent1 += 1
    assert sent0 >= 100 and sent1 >= 100 and silent >= 2


def test_pure_noise_is_rarely_valid():
    _, f0, f1 = C.golden()
    s0 = [c["status"] for c in f0 if c["snr_class"] == C.CLASS_NOISE]
    s1 = [s for c in f1 if c["snr_class"] == C.CLASS_NOISE for s in c["status"]]
    assert len(s0) >= 100 and len(s1) >= 30
    assert np.mean(s0) < 0.05 and np.mean(s1) < 0.05, (np.mean(s0), np.mean(s1))


def test_threshold_mix():
    """Around the threshold the reference's own status is valid for 20 to 80 % of the results of each format and port
    count: a detector that decided everything one way would not pass the GPU tests."""
    _, f0, f1 = C.golden()
    for nof_ports in (1, 2, 3, 4):
        s = [c["status"] for c in f0 if c["snr_class"] == C.CLASS_THRESHOLD and len(c["cfg"]["ports"]) == nof_ports]
        assert len(s) >= 25 and 0.2 <= np.mean(s) <= 0.8, (0, nof_ports, len(s), np.mean(s))
    for nof_ports in (1, 2, 4):
        s = [v for c in f1 if c["snr_class"] == C.CLASS_THRESHOLD and c["cfg"]["nof_ports"] == nof_ports for v in c["status"]]
        assert len(s) >= 50 and 0.2 <= np.mean(s) <= 0.8, (1, nof_ports, len(s), np.mean(s))


def test_generator_coverage():
    _, f0, f1 = C.golden()
    shapes = {(c["cfg"]["nof_symbols"], c["cfg"]["second_hop_prb"] != C.NO_HOP) for c in f1}
    assert shapes >= {(n, h) for n in (4, 5, 7, 10, 13, 14) for h in (False, True)}
    assert {c["cfg"]["nof_ports"] for c in f1} == {1, 2, 4}
    assert sum(c["cfg"]["cp_extended"] for c in f1) == 1
    sizes = [len(c["cfg"]["entries"]) for c in f1]
    assert 84 in sizes and 1 in sizes
    assert any({e[1] for e in c["cfg"]["entries"]} == {0, 2} for c in f1), "an OCC gap"
    assert any({e[2] for e in c["cfg"]["entries"]} == {0, 1, 2} for c in f1), "SR-only, 1-bit and 2-bit entries mixed"
    assert any(c["snr_class"] == C.CLASS_HIGH and (c["sent"] < 0).any() and (c["sent"] >= 0).any() for c in f1)
    assert {c["snr_class"] for c in f1} == {c["snr_class"] for c in f0} == {C.CLASS_NOISE, C.CLASS_THRESHOLD, C.CLASS_HIGH}
    # Format 0: every table of the reference, 1 and 2 symbols with and without hopping, 1 to 4 ports, a list out of order.
    assert {(c["cfg"]["nof_harq_ack"], c["cfg"]["sr_opportunity"]) for c in f0} == set(C.F0_TABLES)
    assert {(c["cfg"]["nof_symbols"], c["cfg"]["second_hop_prb"] != C.NO_HOP) for c in f0} == {(1, False), (2, False), (2, True)}
    assert {len(c["cfg"]["ports"]) for c in f0} == {1, 2, 3, 4}
    assert any(c["cfg"]["ports"] != sorted(c["cfg"]["ports"]) or c["cfg"]["ports"][0] != 0 for c in f0)
    assert os.path.getsize(C.GOLDEN) < 1 << 20


decidable_f0, decidable_f1 = C.decidable_f0, C.decidable_f1


def test_fixture_is_decidable(restated):
    """At most 2 % of a format's cases lie so close to a decision (the threshold, the best two Format 0 candidates, the
    Format 1 symbol's quadrant) that rounding within the metric tolerance may turn it."""
    _, f0, f1 = C.golden()
    tol = tolerances(restated)
    u0 = sum(not decidable_f0(c["metric"], r, tol["f0_metric"]) for c, r in zip(f0, restated[0]))
    n1 = u1 = 0
    for c, (res, _) in zip(f1, restated[1]):
        for i, r in enumerate(res):
            n1 += 1
            u1 += not decidable_f1(c["metric"][i], r, tol["f1_metric"])
    assert u0 <= 0.02 * len(f0) and u1 <= 0.02 * n1, (u0, len(f0), u1, n1)


def test_perturbations_change_the_restatement():
    """Each hand perturbation of the restatement moves at least one reported number on the fixture cases it applies
    to: the GPU test that tells the kernel from it is not vacuous."""
    _, f0, f1 = C.golden()
    for name in C.PERTURBATIONS:
        moved = 0
        if name == "f0_noise_no_12":
            cases = f0[:40]
            moved = sum(rel(C.detect_f0(c["cfg"], C.words_to_complex(c["words"]), (name,))["metric"], c["metric"]) > 1e-2
                        for c in cases)
        else:
            cases = f1[:60]
            for c in cases:
                res, noise_var = C.detect_f1(c["cfg"], C.words_to_complex(c["words"]), (name,))
                moved += (rel(noise_var, c["noise_var"]) > 1e-2 or
                          any(rel(r["rsrp"], v) > 1e-2 for r, v in zip(res, c["rsrp"])))
        assert moved >= 5, (name, moved)


def test_host_code(tmp_path):
    """srsran-5g_amd/csrc/pucch_host.cpp in a stand-alone program built with the address and undefined-behaviour
    sanitizers: n_cs against the reference's values of the fixture, the hop splits for every length with and without
    hopping, the threshold picks, the job descriptors and every refusal."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "a host C++ compiler is needed"
    g, _, _ = C.golden()
    exe = str(tmp_path / "pucch_host_check")
    csrc = os.path.join(ROOT, "srsran-5g_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}", "-o", exe, os.path.join(csrc, "pucch_host.cpp"),
                    os.path.join(ROOT, "tools", "pucch_host_check.cpp")], check=True)
    dump = tmp_path / "ncs.bin"
    queries = g["ncs_query"][::4]  # every fourth value: the Gold sequence is walked from its start for each
    with open(dump, "wb") as f:
        f.write(struct.pack("<I", len(queries)))
        for q, v in zip(queries, g["ncs_value"][::4]):
            f.write(struct.pack("<5I", *(int(x) for x in q), int(v)))
    for q, v, a in zip(g["ncs_query"], g["ncs_value"], g["ncs_alpha"]):
        assert C.n_cs(*(int(x) for x in q)) == int(v) and int(v) % 12 == int(a)
    res = subprocess.run([exe, str(dump)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"{len(queries)} n_cs values" in res.stdout and "0 failures" in res.stdout
