"""GPU parity of the PRACH detector plan (srsgpu_prach_detector_plan through the C ABI, one launch for every occasion)
against the reference's own results (tests/golden/prach_detector.npz) and against the float64 restatement
tests/prach_cases.py, which tests/test_prach_oracle.py pins to the same fixture. DELTA (prach_cases.DELTA, 1.9e-3) is ten
times the measured reference-to-restatement deviation, which is the reference's approximate reciprocal.

`detected` and `delay_samples` must equal the restatement's on every monitored preamble, detected or not (the kernel
divides exactly, as the restatement does; prach_cases.KERNEL_DELTA says why that is well posed), and the reference's on
every preamble decidable at DELTA, the reference's own tolerance. Peaks, metrics and RSSI lie within DELTA. The
input holds bf16 NaN in every word no occasion reads and guard words around it; the results are pre-filled with 0xFF
between guard records and every byte of them must be overwritten.

The kernel's own largest relative deviation on the fixture, measured on an MI355X (test_fixture_in_one_plan prints it):
metric against the reference 1.90e-4 (the reference's own approximate reciprocal), peak against the restatement 2.1e-5,
RSSI 8.8e-8; 5 of the 1048 monitored preambles are undecidable."""
import numpy as np
import pytest

import prach_cases as C

pytestmark = pytest.mark.gpu

GUARD = 0xA5
place, compare, new_deviation = C.place, C.compare, C.new_deviation


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


def run(ctx, cases, order=None, seed=0):
    """One plan and one launch over all cases -> PRACH_RESULT_DTYPE array in the cases' order."""
    import torch
    import srsgpu
    dev = torch.device("cuda", 0)
    words, occasions = place(cases, seed)
    if order is not None:
        for o, i in zip(occasions, order):
            o.result_index = int(i)
    plan = srsgpu.PrachDetectorPlan(ctx, occasions, words.size)
    size = srsgpu.PRACH_RESULT_DTYPE.itemsize
    d_input = torch.from_numpy(words.view(np.int32)).to(dev)
    d_buffer = torch.full((size * (len(cases) + 2),), GUARD, dtype=torch.uint8, device=dev)
    d_buffer[size:-size] = 0xFF
    plan.execute(d_input, d_buffer[size:-size])
    torch.cuda.synchronize(dev)
    plan.close()
    raw = d_buffer.cpu().numpy()
    assert (raw[:size] == GUARD).all() and (raw[-size:] == GUARD).all(), "a guard record was written"
    results = raw[size:-size].view(srsgpu.PRACH_RESULT_DTYPE)
    assert (results["reserved"] == 0).all()
    return results if order is None else results[np.asarray(order)]


@pytest.fixture(scope="module")
def fixture_run(ctx):
    cases, _ = C.golden()
    order = np.random.default_rng(3).permutation(len(cases))
    return run(ctx, cases, order)


@pytest.fixture(scope="module")
def random_run(ctx):
    rng = np.random.default_rng(411)
    cases = [C.random_occasion(rng, long_format=i >= 10) for i in range(12)]
    want = [C.detect(c, C.words_to_complex(c["words"])) for c in cases]
    return cases, want, run(ctx, cases, seed=7)


def test_fixture_in_one_plan(fixture_run):
    """All fixture occasions, long and short, in ONE plan and one launch, their results in a permuted order."""
    cases, _ = C.golden()
    dev, undecided, total = new_deviation(), 0, 0
    for c, r, got in zip(cases, C.restate_golden(), fixture_run):
        undecided += compare(got, c, r, dev)
        total += len(r["preambles"])
    print("kernel against the restatement (rssi, peak) and the reference (metric):", {k: f"{v:.2e}" for k, v in dev.items()},
          "undecidable", undecided, "of", total)
    assert undecided <= 0.01 * total


@pytest.mark.parametrize("index", range(len(C.GOLDEN_RECIPES)))
def test_fixture_case_alone(ctx, index):
    cases, _ = C.golden()
    c = cases[index]
    assert c["name"] == C.GOLDEN_RECIPES[index][0]
    compare(run(ctx, [c], seed=index)[0], c, C.restate_golden()[index], new_deviation())


def test_random_occasions_against_the_restatement(random_run):
    """Fresh occasions with random valid roots, made-up thresholds and margins: ten short ones and two long ones."""
    cases, want, results = random_run
    total = 0
    for c, r, got in zip(cases, want, results):
        compare(got, dict(c, indications=[]), r, new_deviation(), reference=False)
        total += len(r["preambles"])
    assert total >= 100
    assert sum(C.derive(c["format"], c["ra_scs"], c["n_cs"])["L"] == 839 for c in cases) == 2
    assert any(not c["combine"] for c in cases) and any(c["n_cs"] == 0 for c in cases)


def test_perturbed_restatements_are_told_apart(fixture_run, random_run):
    """Against the restatement perturbed by hand the kernel differs, in every peak the perturbation moves by more than
    1 % (by more than DELTA) and in every delay or decision that it changes, on every case it applies to."""
    cases, _ = C.golden()
    work = list(zip(cases, C.restate_golden(), fixture_run))
    random_cases, random_want, random_results = random_run
    work += list(zip(random_cases, random_want, random_results))[-3:]
    for name in C.PERTURBATIONS:
        applied = 0
        for c, r, got in work:
            if r["early"]:
                continue
            bent = C.detect(c, C.words_to_complex(c["words"]), (name,))
            for k, p in r["preambles"].items():
                b, g = bent["preambles"][k], got["preambles"][k]
                if C.rel(b["peak"], p["peak"]) > 1e-2:
                    applied += 1
                    assert C.rel(g["peak"], b["peak"]) > C.DELTA, (name, c.get("name"), k)
                if b["delay"] != p["delay"]:
                    applied += 1
                    assert int(g["delay_samples"]) != b["delay"], (name, c.get("name"), k)
                if b["detected"] != p["detected"]:
                    applied += 1
                    assert bool(g["detected"]) != b["detected"], (name, c.get("name"), k)
        assert applied >= 1, (name, applied)


def good_occasion(**changes):
    import srsgpu
    base = dict(format="0", ra_scs=C.SCS_1_25, nof_rx_ports=2, n_cs=46, roots=[129, 710, 140, 699], threshold=0.25, win_margin=5,
                sample_offset=3, port_stride=900, symbol_stride=839, start_preamble_index=5, nof_preamble_indices=20)
    return srsgpu.PrachOccasion(**dict(base, **changes))


WORDS = 3 + 900 + 839  # what the good occasion needs
# (what is wrong, the refusal's reason[, input words]): every case is refused for its own reason.
REFUSED = ((dict(nof_preamble_indices=0), "no preamble"), (dict(start_preamble_index=50), "past 64"),
           (dict(nof_rx_ports=0), "ports"), (dict(nof_rx_ports=5), "ports"), (dict(combine_symbols=2), "combine_symbols"),
           (dict(format=14), "no preamble information"), (dict(ra_scs=0), "no preamble information"),
           (dict(format="3"), "no preamble information"), (dict(format="B4"), "no preamble information"),
           (dict(ra_scs=6), "no preamble information"),
           (dict(n_cs=840, roots=list(range(1, 65))), "N_cs exceeds"), (dict(roots=[129, 710, 140]), "nof_roots"),
           (dict(roots=[129, 710, 140, 699, 120]), "nof_roots"), (dict(roots=[129, 0, 140, 699]), "root is outside"),
           (dict(roots=[129, 839, 140, 699]), "root is outside"), (dict(threshold=0.0), "threshold"),
           (dict(threshold=-1.0), "threshold"), (dict(threshold=float("nan")), "threshold"), (dict(win_margin=0), "margin is zero"),
           (dict(win_margin=490), "longer than the IDFT"),
           # Format 1 with N_cs = 0: a window of 875 samples; the input is long enough for its two symbols.
           (dict(format="1", n_cs=0, roots=list(range(1, 65)), win_margin=75, port_stride=2000), "longer than the IDFT", 8000),
           (dict(sample_offset=4), "outside the input"), (dict(port_stride=901), "outside the input"),
           (dict(result_index=1), "result_index"))


def test_refusals_leave_no_device_memory(ctx):
    import srsgpu
    before = srsgpu.live_device_buffers()
    for bad, reason, *words in REFUSED:
        with pytest.raises(srsgpu.SrsGpuError, match=reason):
            srsgpu.PrachDetectorPlan(ctx, [good_occasion(**bad)], words[0] if words else WORDS)
        assert srsgpu.live_device_buffers() == before, bad
    with pytest.raises(srsgpu.SrsGpuError, match="belongs to another occasion"):  # two occasions whose results overlap
        srsgpu.PrachDetectorPlan(ctx, [good_occasion(result_index=1), good_occasion(result_index=1)], WORDS)
    assert srsgpu.live_device_buffers() == before
    # The Format 1 occasion above is accepted once its margin fits: it was refused for the window alone.
    wide = dict(format="1", n_cs=0, roots=list(range(1, 65)), win_margin=74, port_stride=2000)
    plan = srsgpu.PrachDetectorPlan(ctx, [good_occasion(**wide)], 8000)
    plan.close()
    plan = srsgpu.PrachDetectorPlan(ctx, [good_occasion()], WORDS)
    assert srsgpu.live_device_buffers() == before + 3
    plan.close()
    assert srsgpu.live_device_buffers() == before


def test_max_delay_samples_for_every_format():
    """srsgpu_prach_max_delay_samples (what the Python mirror takes time_advance_max from) against the restatement, for
    every format, SCS and a set of N_cs; undefined pairs are refused."""
    import srsgpu
    checked = refused = 0
    for fmt in range(15):
        for ra_scs in range(7):
            for n_cs in (0, 1, 2, 13, 23, 46, 69, 119, 139, 419, 839, 840):
                o = srsgpu.PrachOccasion(format=fmt, ra_scs=ra_scs, nof_rx_ports=1, n_cs=n_cs, roots=[], threshold=1.0,
                                         win_margin=1, sample_offset=0, port_stride=0, symbol_stride=0)
                d = C.derive(fmt, ra_scs, n_cs)
                if d is None:
                    with pytest.raises(srsgpu.SrsGpuError):
                        srsgpu.prach_max_delay_samples(o)
                    refused += 1
                else:
                    assert srsgpu.prach_max_delay_samples(o) == d["max_delay"], (fmt, ra_scs, n_cs)
                    checked += 1
    assert checked >= 300 and refused >= 300


def test_graph_replay_equals_eager(ctx):
    """One torch.cuda.graph capture of execute() replayed on two other sets of samples: each replay equals eager
    execution bit for bit."""
    import torch
    import srsgpu
    dev = torch.device("cuda", 0)
    cases, _ = C.golden()
    picked = [c for c in cases if c["name"] in ("f0_ncs46_last_root", "a1", "b4_no_combine")]
    inputs, occasions = [], None
    for seed in (1, 2, 3):
        noise = np.random.default_rng(seed)
        noisy = [dict(c, words=C.to_bf16_words(C.words_to_complex(c["words"]) + 0.1 * C.awgn(noise, c["words"].shape))) for c in picked]
        words, occasions = place(noisy, seed=0)  # the same layout, other samples
        inputs.append(torch.from_numpy(words.view(np.int32)).to(dev))
    plan = srsgpu.PrachDetectorPlan(ctx, occasions, inputs[0].numel())
    size = srsgpu.PRACH_RESULT_DTYPE.itemsize * len(picked)
    eager = []
    for d_input in inputs:
        out = torch.full((size,), GUARD, dtype=torch.uint8, device=dev)
        plan.execute(d_input, out)
        torch.cuda.synchronize(dev)
        eager.append(out.cpu().numpy().copy())
    assert not np.array_equal(eager[0], eager[1]) and not np.array_equal(eager[1], eager[2])
    static_input = inputs[0].clone()
    static_out = torch.full((size,), GUARD, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.execute(static_input, static_out)
    for d_input, want in zip(inputs[1:], eager[1:]):
        static_input.copy_(d_input)
        static_out.fill_(GUARD)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert np.array_equal(static_out.cpu().numpy(), want)
    plan.close()


def test_python_detector_reports_the_references_indications(ctx):
    """srsgpu.PrachDetector.detect_batch on prach_buffer-like storage (ports x symbols x L, nothing between): the
    indications of the reference in its order, times in seconds, RSSI in dB."""
    import srsgpu
    cases, _ = C.golden()
    picked = [c for c in cases if c["name"] in ("f0_ncs13", "c2", "b4_zero", "f0_delay_sides")]
    occasions, at = [], 0
    for c in picked:
        _, S, L = c["words"].shape
        occasions.append(srsgpu.PrachOccasion(
            format=C.FORMATS[c["format"]], ra_scs=c["ra_scs"], nof_rx_ports=c["nof_ports"], n_cs=c["n_cs"], roots=c["roots"],
            threshold=c["threshold"], win_margin=c["margin"], sample_offset=at, port_stride=S * L, symbol_stride=L,
            start_preamble_index=c["start"], nof_preamble_indices=c["nof"], combine_symbols=c["combine"]))
        at += c["words"].size
    results = srsgpu.PrachDetector(ctx).detect_batch(np.concatenate([c["words"].ravel() for c in picked]), occasions)
    for c, r, got in zip(picked, [C.restate_golden()[cases.index(c)] for c in picked], results):
        assert abs(got.time_resolution - c["time_resolution"]) < 1e-12 and abs(got.time_advance_max - c["time_advance_max"]) < C.T_C
        if r["early"]:
            assert got.preambles == [] and got.rssi_dB == float("-inf") == c["rssi_dB"]
            continue
        assert abs(got.rssi_dB - c["rssi_dB"]) < 1e-2
        sure = {k for k, p in r["preambles"].items() if C.decidable(p, c["threshold"])}
        assert [p.preamble_index for p in got.preambles if p.preamble_index in sure] == [k for k, _, _ in c["indications"] if k in sure]
        want = {k: (ta, m) for k, ta, m in c["indications"]}
        for p in got.preambles:
            if p.preamble_index in sure:
                assert abs(p.time_advance - want[p.preamble_index][0]) < C.T_C, (c["name"], p)
                assert C.rel(p.detection_metric, want[p.preamble_index][1]) <= C.DELTA
