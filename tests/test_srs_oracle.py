"""The float64 restatement of the SRS estimator (tests/srs_cases.py) against the reference's own results
(tests/golden/srs_estimator.npz, made by tools/gen_srs_golden.py from srs_estimator_generic_impl built from its sources
with its low-PAPR generator, DFT time alignment estimator and generic IDFTs), the condition on the fixture that the GPU
tests lean on, and the plan's host code in a stand-alone sanitizer build. No GPU.

Measured on the fixture, the largest deviation of the reference's results from the restatement's: channel matrix 6.7e-7
of its Frobenius norm, EPRE 4.2e-7 relative, noise variance 5.5e-7 of max(nv, 1e-6 EPRE), time alignment 6.6e-7 of
1 / fs, each antenna port's own measurement 1.1e-6 of 1 / fs. Ten times each lies below the floor, so every tolerance
is 1e-4 (srs_cases.tolerances()). Every fixture case is decidable at KERNEL_DELTA = 5e-4; the smallest lead of a winning
tap is 8.8e-3 (cs11_comb4)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import srs_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def restated():
    return C.restate_golden()


def test_constants_are_the_measured_deviations(restated):
    measured = C.measured_deviations(restated)
    print("largest deviations of the reference from the restatement:", {k: f"{v:.3e}" for k, v in measured.items()})
    for k, v in measured.items():
        assert v <= C.MEASURED[k] * 1.05, (k, v)
        assert C.MEASURED[k] <= v * 1.05, (k, "the constant is staler than the fixture")
    assert C.tolerances() == {k: max(10 * v, 1e-4) for k, v in C.MEASURED.items()}


def test_restatement_against_the_fixture(restated):
    """Every quantity within its tolerance, every antenna port's own time alignment (so every peak decision) equal, and
    the derived resolution and range exact."""
    cases, _ = C.golden()
    tol = C.tolerances()
    for c, r in zip(cases, restated):
        ref, d = c["ref"], r["derived"]
        dev = C.deviations(ref, r)
        for k, v in dev.items():
            assert v <= tol[k], (c["name"], k, v)
        for p, (got, want) in enumerate(zip(ref["ta_port"], r["ta_port"])):
            assert abs(got - want) * d["fs"] <= tol["time_alignment"], (c["name"], p, got * d["fs"], want * d["fs"])
            assert abs(got * d["fs"] - r["ta_idx"][p]) <= 1.0 + tol["time_alignment"]
        assert ref["resolution"] == 1.0 / d["fs"] and ref["ta_max"] == d["max_ta_samples"] / d["fs"], c["name"]
        # The finding: the reference's lower bound is the smallest positive double, not -ta_max (:115 / :203).
        assert ref["ta_min"] == np.finfo(np.float64).tiny, c["name"]


def test_fixture_is_decidable(restated):
    """No case is left out: the winning tap of every antenna port leads every other searched tap by more than
    KERNEL_DELTA of itself (or the correlation is all zero, which float32 keeps exactly)."""
    cases, _ = C.golden()
    leads = []
    for c, r in zip(cases, restated):
        assert C.decidable(r), (c["name"], r["gap"])
        if r["epre"] > 0:
            leads.append((min(r["gap"]), c["name"]))
    print("smallest lead:", min(leads))
    assert min(leads)[0] > C.KERNEL_DELTA


def test_fixture_coverage(restated):
    cases, table = C.golden()
    by = {c["name"]: (c, r) for c, r in zip(cases, restated)}
    lengths = {(r["derived"]["L"], c["comb_size"]) for c, r in zip(cases, restated)}
    assert {(12, 4), (24, 2), (24, 4), (36, 4), (48, 2), (96, 2), (108, 4), (120, 2), (816, 2), (1632, 2)} <= lengths
    assert {r["derived"]["M"] for r in restated} == {128, 256, 1024, 2048}
    assert by["L96_idft128"][1]["derived"]["M"] == 128 and by["L108_idft256"][1]["derived"]["M"] == 256
    for comb, n_cs_max in ((2, 8), (4, 12)):
        assert {c["cyclic_shift"] for c in cases if c["comb_size"] == comb} == set(range(n_cs_max))
        assert {c["comb_offset"] for c in cases if c["comb_size"] == comb} == set(range(comb))
    # Cyclic shifts that wrap modulo n_cs_max, interleaved and not.
    assert any(max(r["derived"]["n_cs"]) > r["derived"]["n_cs"][-1] for r in restated)
    naps = {(c["nof_antenna_ports"], bool(r["derived"]["interleaved"])) for c, r in zip(cases, restated)}
    assert naps == {(1, False), (2, False), (4, False), (4, True)}
    assert {len(c["rx_ports"]) for c in cases} == {1, 2, 4}
    assert any(c["rx_ports"] == (2, 0) for c in cases) and any(c["rx_ports"] == (3, 1, 0, 2) for c in cases)
    assert {c["nof_symbols"] for c in cases if c["start_symbol"] + c["nof_symbols"] == 14} == {1, 2, 4}
    assert {c["bandwidth_index"] for c in cases if c["freq_position"] and c["freq_shift"]} == {0, 1, 2, 3}
    assert {c["numerology"] for c in cases} == {0, 1, 2, 3}
    idx = {name: r["ta_idx"] for name, (c, r) in by.items()}
    assert idx["L12_comb4"] == [0] and idx["L816_idft1024"] == [20, 20] and idx["L1632_idft2048"] == [-34]
    m = by["delay_near_max"][1]["derived"]["max_ta_samples"]
    assert idx["delay_near_max"] == [m - 1] and idx["advance_near_max"] == [-(m - 1)] * 2
    assert abs(by["delay_beyond"][0]["recipe"]["delay"]) > m
    assert by["pure_noise"][0]["recipe"]["kind"] == "noise" and by["all_zero"][0]["recipe"]["kind"] == "zero"
    zero = by["all_zero"]
    assert not zero[0]["words"].any() and zero[1]["noise_var"] == 0 and zero[1]["time_alignment"] == 0
    assert zero[0]["ref"]["noise_var"] == 0 and zero[0]["ref"]["time_alignment"] == 0 and not zero[0]["ref"]["channel"].any()
    snrs = [c["recipe"]["snr_db"] for c in cases if c["recipe"]["kind"] == "signal"]
    assert min(snrs) == 0 and max(snrs) == 30
    assert table.shape == (64, 4, 2) and tuple(table[63][0]) == (272, 1)
    assert os.path.getsize(C.GOLDEN) < 1 << 20


def test_the_noise_residual_alternates_its_sign(restated):
    """The finding recorded in DESIGN.md: with more than one antenna port on a comb set the reference's noise variance
    holds every other port's signal twice. It exceeds the noise the case was drawn with by far at 30 dB."""
    cases, _ = C.golden()
    by = {c["name"]: (c, r) for c, r in zip(cases, restated)}
    c, r = by["zero_delay_30dB"]
    assert c["nof_antenna_ports"] == 4 and not r["derived"]["interleaved"]
    assert c["ref"]["noise_var"] > 100 * 10 ** (-c["recipe"]["snr_db"] / 10) and r["noise_var"] > 0.5 * r["epre"]
    c, r = by["L96_idft128"]  # one antenna port: the sign does not matter
    assert c["nof_antenna_ports"] == 1 and r["noise_var"] < r["epre"]


def test_perturbations_change_the_restatement(restated):
    """Each hand-made error fails the comparison with the restatement on every fixture case it applies to, and applies
    to at least two: the GPU test that tells the kernel from it is not vacuous."""
    cases, _ = C.golden()
    tol = C.tolerances()
    for name in C.PERTURBATIONS:
        hit = 0
        for c, r in zip(cases, restated):
            if not C.applies(name, c, r):
                continue
            bent = C.estimate(c, C.words_to_complex(C.case_grid_words(c)), (name,))
            assert C.failures(bent, r, tol), (name, c["name"])
            hit += 1
        print(name, hit)
        assert hit >= 2, name


def config_bytes(c, grid_index=0, result_index=0):
    rx = (list(c["rx_ports"]) + [0] * 4)[:4]
    return struct.pack("<4H4B12B4B4H2I", *(m for m, _ in c["row"]), *(n for _, n in c["row"]), c["numerology"],
                       c["nof_antenna_ports"], c["nof_symbols"], c["start_symbol"], c["comb_size"], c["comb_offset"],
                       c["cyclic_shift"], c["bandwidth_index"], 3, 0, len(c["rx_ports"]), 0, *rx, c["sequence_id"],
                       c["freq_shift"], c["freq_position"], 0, grid_index, result_index)


def test_host_code(tmp_path, restated):
    """srsran-5g_amd/csrc/srs_host.cpp in a stand-alone program built with the address and undefined-behaviour
    sanitizers: the derived quantities of every fixture case and of a sweep over every table row, comb, numerology and
    antenna port count against the restatement, the sequences, the job descriptor and every refusal."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "srs_host_check")
    csrc = os.path.join(ROOT, "srsran-5g_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}", "-o", exe, os.path.join(csrc, "srs_host.cpp"),
                    os.path.join(ROOT, "tools", "srs_host_check.cpp")], check=True)
    cases, table = C.golden()
    resources = [c for c in cases]
    rng = np.random.default_rng(5)
    for c_srs in range(64):
        for b in range(4):
            for comb in (2, 4):
                nap = (1, 2, 4)[(c_srs + b) % 3]
                c = dict(c_srs=c_srs, row=tuple((int(m), int(n)) for m, n in table[c_srs]), numerology=(c_srs + comb) % 5,
                         nof_antenna_ports=nap, nof_symbols=1, start_symbol=13, comb_size=comb,
                         comb_offset=int(rng.integers(0, comb)), cyclic_shift=int(rng.integers(0, 12 if comb == 4 else 8)),
                         sequence_id=int(rng.integers(0, 1024)), bandwidth_index=b, freq_position=int(rng.integers(0, 68)),
                         freq_shift=int(rng.integers(0, 3)), rx_ports=(0,), grid_nof_ports=4)
                c["grid_nof_prb"] = C.min_grid_prb(c)
                if c["grid_nof_prb"] <= 275:
                    resources.append(c)
    sequences = set()
    for c in resources[: len(cases) + 40]:
        d = C.derive(c)
        sequences |= {(d["u"], d["L"], n_cs, d["n_cs_max"]) for n_cs in d["n_cs"]}
    sequences = sorted(sequences)
    dump = tmp_path / "srs.bin"
    with open(dump, "wb") as f:
        f.write(struct.pack("<I", len(resources)))
        for c in resources:
            d = C.derive(c)
            pad = lambda v: (list(v) + [0] * 4)[:4]  # noqa: E731
            log2m = int(d["M"]).bit_length() - 1
            f.write(config_bytes(c))
            f.write(struct.pack("<16Id", c["grid_nof_prb"], d["L"], d["n_cs_max"], d["u"], int(d["interleaved"]),
                                *pad(d["n_cs"]), *pad(d["k0"]), d["M"], log2m, d["max_ta_samples"], d["fs"]))
        f.write(struct.pack("<I", len(sequences)))
        for u, length, n_cs, n_cs_max in sequences:
            s = C.sequence(u, length, n_cs, n_cs_max)
            f.write(struct.pack("<4I", u, length, n_cs, n_cs_max))
            f.write(np.stack([s.real, s.imag], 1).astype("<f8").tobytes())
    res = subprocess.run([exe, str(dump)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"{len(resources)} resources, {len(sequences)} sequences, 0 failures" in res.stdout
    assert len(resources) > 400
