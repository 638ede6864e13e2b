"""The float64 restatement of the PUCCH Format 3 / 4 front end (tests/pucch_f34_cases.py) against the reference's own
results (tests/golden/pucch_f34.npz, made by tools/gen_pucch_f34_golden.py from dmrs_pucch_estimator_formats3_4,
pucch_demodulator_format3 / format4, transform_precoder_dft_impl and uci_decoder_impl built from their sources), the
properties of the fixture's inputs that the GPU tests lean on, and the plan's host code in a stand-alone sanitizer
build. No GPU.

Measured on the fixture (249 PDUs, 49914 LLRs), the reference's float32 results against the restatement: every LLR
equal or one step apart, 2.0e-3 of them apart; noise variance 1.5e-7, RSRP 6.6e-7 and EPRE 1.6e-7 of the port's EPRE;
time alignment 0 T_c (the reference reports 0 on every case); CFO 8.3e-5 of 15 Hz. The restatement of the kernel's
float32 sequence against the float64 one: 1 LLR of 49914 moves (2.0e-5), so the GPU test's bound on the share of
differing LLRs is the floor of 1e-3."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import pucch_f34_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def restated():
    return C.restate_golden()


def identity_ports(cfg):
    return cfg["ports"] == list(range(len(cfg["ports"])))


def test_restatement_against_the_fixture(restated):
    """LLRs equal or one step apart on every case; the share that differs and the deviations of the channel state are
    printed and stay within the figures of the module docstring."""
    cases = C.golden()
    dev = C.measured_deviations(restated, cases)
    print({k: f"{v:.2e}" for k, v in dev.items()})
    for r, c in zip(restated, cases):
        assert C.llr_diff(r["llrs"], c["llrs"])[1] <= 1, c["cfg"]
    assert len(cases) >= 240 and sum(len(c["llrs"]) for c in cases) >= 40000
    limits = dict(llr_share=5e-3, noise_var=1e-6, rsrp=2e-6, epre=5e-7, ta=0.5, cfo=3e-4)
    for key, limit in limits.items():
        assert dev[key] < limit, (key, dev[key])


def test_time_alignment_is_zero_in_the_reference():
    """Mean smoothing hands the time alignment estimator one constant per hop: the reference reports 0 on every port of
    every case, the delayed ones included, and the plan is held to that."""
    for c in C.golden():
        assert not np.any(c["ta"]) and c["csi"]["time_alignment"] == 0, c["cfg"]


def test_python_decoders_agree_with_the_reference():
    """The restated short-block and polar decoders give the reference's bits and status from the reference's LLRs,
    on invalid payloads too."""
    for c in C.golden():
        bits, valid = C.decode(c["llrs"], c["cfg"]["nof_uci_bits"], c["cfg"]["pi2_bpsk"])
        assert int(valid) == c["status"] and np.array_equal(bits, c["bits"]), c["cfg"]


def test_transmitters_come_back_at_high_snr():
    """At 30 dB per port the reference returns every payload that was sent, valid, on every case with the port list
    0..P-1."""
    n = 0
    for c in C.golden():
        if c["snr_class"] == C.CLASS_HIGH and identity_ports(c["cfg"]):
            assert c["status"] == 1 and np.array_equal(c["bits"], c["sent"]), c["cfg"]
            n += 1
    assert n >= 80, n


def test_reference_tables_as_recorded():
    """The DM-RS symbol mask of every length, the Format 4 orthogonal sequences and the LLR counts equal the reference's
    own, recorded as data."""
    masks, w = C.golden_tables()
    for n in range(4, 15):
        for hop in (0, 1):
            for add in (0, 1):
                assert masks[n - 4, hop, add] == C.dmrs_mask(n, bool(hop), bool(add)), (n, hop, add)
    for sf, first in ((2, 0), (4, 2)):
        for i in range(sf):
            assert np.allclose(w[first + i], C.w_row(sf, i), atol=1e-6), (sf, i)
    for c in C.golden():
        assert len(c["llrs"]) == C.nof_llrs(c["cfg"])
    assert {9, 15} <= {len(c["llrs"]) for c in C.golden()}


def test_generator_coverage():
    cases = C.golden()
    cfgs = [c["cfg"] for c in cases]

    def some(pred):
        return any(pred(c) for c in cfgs)

    f3, f4 = [c for c in cfgs if c["format"] == 3], [c for c in cfgs if c["format"] == 4]
    for n in range(4, 15):
        for hop in (False, True):
            assert any(c["nof_symbols"] == n and C.hopping(c) == hop and c["nof_prb"] == 1 for c in f3), (n, hop)
            if n >= 10:
                assert any(c["nof_symbols"] == n and C.hopping(c) == hop and c["additional_dmrs"] for c in f3), (n, hop)
    assert {c["nof_prb"] for c in f3 if c["nof_symbols"] == 4 and not C.hopping(c)} >= set(C.VALID_NOF_PRB)
    assert some(lambda c: (c["nof_prb"], c["nof_symbols"], len(c["ports"])) == (16, 14, 4))
    for sf in (2, 4):
        for occ in range(sf):
            for pi2 in (0, 1):
                for n in (4, 7):
                    assert any((c["occ_length"], c["occ_index"], c["pi2_bpsk"], c["nof_symbols"]) == (sf, occ, pi2, n)
                               for c in f4), (sf, occ, pi2, n)
    assert {len(c["ports"]) for c in cfgs} == {1, 2, 3, 4}
    assert some(lambda c: not identity_ports(c) and len(c["ports"]) == 1) and some(lambda c: c["ports"] == [3, 0, 2])
    assert some(lambda c: c["cp_extended"] and c["numerology"] == 2)
    assert {c["numerology"] for c in cfgs} == {0, 1, 2, 3}
    for pi2 in (0, 1):
        assert {c["nof_uci_bits"] for c in cfgs if c["pi2_bpsk"] == pi2} >= set(range(3, 12))
    assert {c["nof_uci_bits"] for c in cfgs} >= {12, 19, 20, 360}
    assert some(lambda c: c["nof_uci_bits"] >= 360 and C.nof_llrs(c) >= 1088)
    assert some(lambda c: C.hopping(c) and c["nof_symbols"] % 2 == 1)
    assert sum(bool(np.any(c["epre"] == 0)) for c in cases) >= 3, "dead ports"
    assert {c["snr_class"] for c in cases} == {C.CLASS_NOISE, C.CLASS_INFORMATIVE, C.CLASS_HIGH}
    assert any(np.isnan(c["cfo_hz"]).all() for c in cases) and any(not np.isnan(c["cfo_hz"]).any() for c in cases)
    assert os.path.getsize(C.GOLDEN) < 300 * 1024


def test_informative_cases():
    """At the informative cases' SNR, set per modulation, spreading factor and diversity order, at least 60 % of the
    reference's LLRs are neither 0 nor +-120, so that a wrong scale or offset shows."""
    cases = C.golden()
    inf = [c for c in cases if c["snr_class"] == C.CLASS_INFORMATIVE]
    pure = [c for c in inf if identity_ports(c["cfg"])]
    share = C.informative_share(np.concatenate([c["llrs"] for c in pure]))
    print(f"informative share {share:.3f} over {len(pure)} of {len(cases)} cases")
    assert len(inf) >= 0.45 * len(cases) and share >= 0.6
    assert np.mean([C.informative_share(c["llrs"]) >= 0.6 for c in pure]) >= 0.9


def test_pure_noise_is_invalid_for_polar_payloads():
    s = [c["status"] for c in C.golden() if c["snr_class"] == C.CLASS_NOISE and c["cfg"]["nof_uci_bits"] >= 12]
    assert len(s) >= 20 and np.mean(s) < 0.1, (len(s), np.mean(s))


def test_fixture_is_decidable():
    """decidable (recorded at generation): the reference's decoder gives the same bits and status from the reference's
    LLRs and from the restatement's. At least 95 % of the cases are, and every sent high-SNR case."""
    cases = C.golden()
    und = [c for c in cases if not c["decidable"]]
    assert len(und) <= 0.05 * len(cases), len(und)
    assert not [c["cfg"] for c in und if c["snr_class"] == C.CLASS_HIGH]


def test_perturbations_change_the_restatement(restated):
    """Each hand-made error changes the restatement on the fixture cases it applies to. Two apply to none by
    construction of the reference: with one estimate per hop every RE of a symbol has the same post-equalisation noise
    variance, so per-RE variances equal their mean up to the rounding of the mean's sum."""
    cases = C.golden()
    applies = dict(
        idft_scale=lambda c: True,
        per_re_noise=lambda c: False,
        f4_noise_div_sf=lambda c: c["format"] == 4,
        pi2_parity_per_symbol=lambda c: c["format"] == 4 and c["pi2_bpsk"] and c["occ_length"] == 4,
        m0_swapped=lambda c: c["format"] == 4 and c["occ_index"] in (1, 2),
        hop_ceil=lambda c: C.hopping(c) and c["nof_symbols"] % 2 == 1,
        no_bf16=lambda c: True,
        data_port_i=lambda c: not identity_ports(c))
    assert set(applies) == set(C.PERTURBATIONS)
    for name in C.PERTURBATIONS:
        count = 0
        for c, r in zip(cases, restated):
            if not applies[name](c["cfg"]) or c["snr_class"] != C.CLASS_INFORMATIVE:  # (at 30 dB every LLR is clipped)
                continue
            p = C.restate(c["cfg"], C.grid_of(c["cfg"], c["words"]), (name,))
            changed = (not np.array_equal(p["est"], r["est"]) or not np.array_equal(p["llrs"], r["llrs"])
                       or not np.array_equal(p["noise_var"], r["noise_var"]))
            assert changed, (name, c["cfg"])
            count += 1
        print(name, count)
        assert count >= (0 if name == "per_re_noise" else 5), (name, count)


def test_float32_share(restated):
    """What float32 arithmetic alone moves: the kernel's sequence of operations (its wave reductions and its direct
    inverse DFT included) restated in numpy float32 against the float64 restatement. Printed; the GPU test's bound is
    ten times the share of differing LLRs, floored at 1e-3."""
    share, dev = C.float32_deviations()
    print(f"float32 share {share:.2e}", {k: f"{v:.2e}" for k, v in dev.items()})
    assert share <= 1e-3
    assert max(dev[k] for k in C.STATE_KEYS) < 1e-5 and dev["ta"] == 0 and dev["cfo"] < 1e-3


def pack_config(c, grid_index, llr_offset):
    ports = (list(c["ports"]) + [0] * 4)[:4]
    return struct.pack("<H6B2H4B4HB4B3x2I", c["slot_index"], c["format"], c["numerology"], c["cp_extended"], c["nof_prb"],
                       c["start_symbol"], c["nof_symbols"], c["starting_prb"], c["second_hop_prb"], c["additional_dmrs"],
                       c["pi2_bpsk"], c["occ_length"], c["occ_index"], c["rnti"], c["n_id_scrambling"], c["n_id_hopping"],
                       c["nof_uci_bits"], len(c["ports"]), *ports, grid_index, llr_offset)


def test_host_code(tmp_path):
    """srsran-5g_amd/csrc/pucch_f34_host.cpp in a stand-alone program built with the address and undefined-behaviour
    sanitizers: DM-RS mask and sequences, scrambling words, w_n, epoch distances and the symbol split against the
    restatement's for every fourth fixture case, the code rates, every refusal with its message and the overlap
    search."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "pucch_f34_host_check")
    csrc = os.path.join(ROOT, "srsran-5g_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}", "-o", exe, os.path.join(csrc, "pucch_f34_host.cpp"),
                    os.path.join(ROOT, "tools", "pucch_f34_host_check.cpp")], check=True)
    cfgs = [c["cfg"] for c in C.golden()][::4]
    assert len(pack_config(cfgs[0], 0, 0)) == 40
    dump = tmp_path / "cases.bin"
    with open(dump, "wb") as f:
        f.write(struct.pack("<I", len(cfgs)))
        for i, c in enumerate(cfgs):
            f.write(pack_config(c, i % 3, 4608 * i))
            f.write(struct.pack("<2I", c["grid_nof_prb"], c["grid_nof_ports"]))
            dm = C.dmrs_symbols(c["nof_symbols"], C.hopping(c), c["additional_dmrs"])
            f.write(struct.pack("<3I", C.dmrs_mask(c["nof_symbols"], C.hopping(c), c["additional_dmrs"]), C.nof_llrs(c), len(dm)))
            for d in dm:
                seq = C.dmrs_sequence(c, c["start_symbol"] + d)
                f.write(struct.pack("<I", c["start_symbol"] + d))
                f.write(np.stack([seq.real, seq.imag], 1).astype(np.float32).tobytes())
            e = C.nof_llrs(c)
            nwords = (e + 31) // 32
            bits = C._gold(c["rnti"] * (1 << 15) + c["n_id_scrambling"], 32 * nwords).astype(np.uint64)
            f.write(struct.pack("<I", nwords))
            f.write(np.array([int(np.sum(bits[32 * w: 32 * w + 32] << np.arange(32, dtype=np.uint64))) for w in range(nwords)],
                             np.uint32).tobytes())
            if c["format"] == 4:
                w = C.w_row(c["occ_length"], c["occ_index"])
                f.write(np.stack([w.real, w.imag], 1).astype(np.float32).tobytes())
            ep = C.symbol_epochs(c["numerology"], c["cp_extended"])
            for syms, _ in (C.hop_lists(c) + [([], 0)])[:2]:
                f.write(struct.pack("<f", ep[syms[1]] - ep[syms[0]] if len(syms) >= 2 else 1.0))
            data = C.data_symbols(c)
            f.write(struct.pack("<I", len(data)))
            for d in data:
                f.write(struct.pack("<2B", c["start_symbol"] + d, C.hop_of(c, d)))
    res = subprocess.run([exe, str(dump)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"{len(cfgs)} dumped PDUs" in res.stdout and "0 failures" in res.stdout
