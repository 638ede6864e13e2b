"""GPU parity of the SRS estimator plan (srsgpu_srs_estimator_plan through the C ABI, one launch for every resource)
against the reference's own results (tests/golden/srs_estimator.npz) and against the float64 restatement
tests/srs_cases.py, which tests/test_srs_oracle.py pins to the same fixture.

ta_idx must equal the restatement's on every decidable resource (srs_cases.KERNEL_DELTA says why that is well posed;
every fixture case is decidable, and test_srs_oracle.py holds each antenna port's own time alignment of the reference to
the restatement's, so the restatement's taps are the reference's). The channel matrix, EPRE, noise variance and time
alignment lie within srs_cases.tolerances(): ten times the measured reference-to-restatement deviation, floored at 1e-4,
which is 1e-4 for all four. The grids hold bf16 NaN (or 1e30) in every word no resource reads; the results lie between
guard records, are pre-filled with 0xFF, and every byte of them must be overwritten.

The kernel's own largest deviations on the fixture, measured on an MI355X (test_fixture_in_one_plan prints them), against
the reference | the restatement: channel matrix 6.5e-7 | 2.8e-7, EPRE 4.1e-7 | 1.3e-7, noise variance 5.7e-7 | 2.0e-7, time
alignment 6.3e-7 | 6.1e-7 of 1 / fs (KERNEL_MEASURED below)."""
import numpy as np
import pytest

import srs_cases as C

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GRID_PRB, GRID_PORTS = 272, 4
# Measured on an MI355X, fixture in one plan: (against the reference, against the restatement).
KERNEL_MEASURED = dict(channel=(6.46e-7, 2.79e-7), epre=(4.07e-7, 1.30e-7), noise_var=(5.68e-7, 1.96e-7),
                       time_alignment=(6.26e-7, 6.12e-7))


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


def resources_of(cases, grid_of, order=None):
    import srsgpu
    return [srsgpu.SrsResource(table_row=c["row"], numerology=c["numerology"], nof_antenna_ports=c["nof_antenna_ports"],
                               nof_symbols=c["nof_symbols"], start_symbol=c["start_symbol"], comb_size=c["comb_size"],
                               comb_offset=c["comb_offset"], cyclic_shift=c["cyclic_shift"], sequence_id=c["sequence_id"],
                               bandwidth_index=c["bandwidth_index"], freq_position=c["freq_position"],
                               freq_shift=c["freq_shift"], rx_ports=c["rx_ports"], grid_index=grid_of[i],
                               result_index=None if order is None else int(order[i]))
            for i, c in enumerate(cases)]


def run(ctx, cases, words_of, fill=C.NAN_WORD, order=None, grid_prb=GRID_PRB):
    """One plan and one launch over all cases, several per grid -> SRS_RESULT_DTYPE array in the cases' order."""
    import torch
    import srsgpu
    dev = torch.device("cuda", 0)
    grid_of, nof_grids = C.pack(cases, grid_prb)
    grids = C.place(cases, words_of, grid_prb, GRID_PORTS, nof_grids, grid_of, fill)
    plan = srsgpu.SrsEstimatorPlan(ctx, resources_of(cases, grid_of, order), grid_prb, GRID_PORTS, nof_grids)
    size = srsgpu.SRS_RESULT_DTYPE.itemsize
    d_grids = torch.from_numpy(grids.view(np.int32)).to(dev)
    d_buffer = torch.full((size * (len(cases) + 2),), GUARD, dtype=torch.uint8, device=dev)
    d_buffer[size:-size] = 0xFF
    plan.execute(d_grids, d_buffer[size:-size])
    torch.cuda.synchronize(dev)
    plan.close()
    raw = d_buffer.cpu().numpy()
    assert (raw[:size] == GUARD).all() and (raw[-size:] == GUARD).all(), "a guard record was written"
    results = raw[size:-size].view(srsgpu.SRS_RESULT_DTYPE)
    assert (results["reserved"] == 0).all()
    results = results if order is None else results[np.asarray(order)]
    for c, rec in zip(cases, results):  # unused entries of the matrix and of ta_idx are zero
        used = np.zeros((4, 4), bool)
        used[: len(c["rx_ports"]), : c["nof_antenna_ports"]] = True
        assert not rec["channel"][~used].any() and not rec["ta_idx"][c["nof_antenna_ports"]:].any(), c["name"]
    return results, nof_grids


@pytest.fixture(scope="module")
def fixture_run(ctx):
    cases, _ = C.golden()
    order = np.random.default_rng(3).permutation(len(cases))
    return run(ctx, cases, [c["words"] for c in cases], C.NAN_WORD, order)


@pytest.fixture(scope="module")
def random_run(ctx):
    _, table = C.golden()
    rng = np.random.default_rng(412)
    cases = C.random_plan_cases(table, rng, 60)
    words_of, want = [], []
    for i, c in enumerate(cases):
        grid_words = C.to_bf16_words(C.make_grid(c, np.random.default_rng([412, i])))
        words_of.append(C.read_words(c, grid_words))
        want.append(C.estimate(c, C.words_to_complex(C.write_words(c, words_of[-1], np.zeros(grid_words.shape, np.uint32)))))
    results, nof_grids = run(ctx, cases, words_of)
    return cases, words_of, want, results, nof_grids


def test_fixture_in_one_plan(fixture_run):
    """All fixture resources in ONE plan and one launch, several per grid, their results in a permuted order: ta_idx
    equal, the rest within the tolerances of the reference's own results."""
    cases, _ = C.golden()
    results, nof_grids = fixture_run
    assert nof_grids < len(cases) / 2, "several resources per grid"
    tol = C.tolerances()
    worst_ref = dict(channel=0.0, epre=0.0, noise_var=0.0, time_alignment=0.0)
    worst_own = dict(worst_ref)
    for c, r, rec in zip(cases, C.restate_golden(), results):
        got = C.record_as_dict(rec, c)
        assert got["ta_idx"] == r["ta_idx"], (c["name"], got["ta_idx"], r["ta_idx"])
        assert got["resolution"] == c["ref"]["resolution"] and got["ta_max"] == c["ref"]["ta_max"], c["name"]
        for worst, want in ((worst_ref, c["ref"]), (worst_own, r)):
            for k, v in C.deviations(got, want).items():
                worst[k] = max(worst[k], v)
        print(c["name"], {k: f"{v:.1e}" for k, v in C.deviations(got, c["ref"]).items()})
        assert not C.failures(got, dict(c["ref"], ta_idx=r["ta_idx"]), tol), (c["name"], C.deviations(got, c["ref"]))
        assert not C.failures(got, r, tol), (c["name"], C.deviations(got, r))
    print("kernel against the reference:", {k: f"{v:.2e}" for k, v in worst_ref.items()})
    print("kernel against the restatement:", {k: f"{v:.2e}" for k, v in worst_own.items()})


def test_words_around_the_data_do_not_reach_the_results(ctx, fixture_run):
    """1e30 in place of NaN in every grid word the estimator does not read: the same bytes."""
    cases, _ = C.golden()
    order = np.random.default_rng(3).permutation(len(cases))
    huge, _ = run(ctx, cases, [c["words"] for c in cases], C.HUGE_WORD, order)
    assert np.array_equal(huge.view(np.uint8), fixture_run[0].view(np.uint8))
    assert np.isfinite(huge["channel"]).all() and np.isfinite(huge["noise_var"]).all()


def test_random_plan_against_the_restatement(random_run):
    """Fresh resources, one seed, 60 in one launch, several per grid, among them a 272-PRB 4 x 4 x 4-symbol interleaved
    one: ta_idx equal on decidable resources, at most 2 % undecidable and each of those on one of the restatement's two
    leading taps."""
    cases, _, want, results, nof_grids = random_run
    assert nof_grids < len(cases) / 2
    tol = C.tolerances()
    wide = [c for c, r in zip(cases, want) if r["derived"]["L"] == 1632 and r["derived"]["interleaved"]]
    assert wide and wide[0]["nof_symbols"] == 4 and len(wide[0]["rx_ports"]) == 4
    undecidable = 0
    for c, r, rec in zip(cases, want, results):
        got = C.record_as_dict(rec, c)
        if C.decidable(r):
            assert not C.failures(got, r, tol), (c["name"], got["ta_idx"], r["ta_idx"], C.deviations(got, r))
            continue
        undecidable += 1
        for p, idx in enumerate(got["ta_idx"]):
            assert idx in (r["ta_idx"][p], r["runner_up"][p]), (c["name"], p, idx)
        if got["ta_idx"] == r["ta_idx"]:
            assert not C.failures(got, r, tol), c["name"]
    print("undecidable:", undecidable, "of", len(cases))
    assert undecidable <= 0.02 * len(cases)
    assert {c["nof_antenna_ports"] for c in cases} == {1, 2, 4} and {c["comb_size"] for c in cases} == {2, 4}
    assert any(c["recipe"]["kind"] == "noise" for c in cases)


def test_perturbed_restatements_are_told_apart(fixture_run, random_run):
    """Against the restatement perturbed by hand the kernel fails the comparison, on every case the error applies to."""
    cases, _ = C.golden()
    tol = C.tolerances()
    work = [(c, C.case_grid_words(c), r, rec) for c, r, rec in zip(cases, C.restate_golden(), fixture_run[0])]
    random_cases, words_of, random_want, random_results, _ = random_run
    for c, w, r, rec in zip(random_cases, words_of, random_want, random_results):
        if C.decidable(r):
            grid = C.write_words(c, w, np.zeros((c["grid_nof_ports"], 14, 12 * c["grid_nof_prb"]), np.uint32))
            work.append((c, grid, r, rec))
    for name in C.PERTURBATIONS:
        applied = 0
        for c, grid, r, rec in work:
            if not C.applies(name, c, r):
                continue
            bent = C.estimate(c, C.words_to_complex(grid), (name,))
            assert C.failures(C.record_as_dict(rec, c), bent, tol), (name, c["name"])
            applied += 1
        print(name, applied)
        assert applied >= 3, (name, applied)


ROW = ((48, 1), (24, 2), (12, 2), (4, 3))  # C_SRS 13


def good_resource(**changes):
    import srsgpu
    base = dict(table_row=ROW, numerology=1, nof_antenna_ports=4, nof_symbols=2, start_symbol=12, comb_size=4, comb_offset=3,
                cyclic_shift=7, sequence_id=77, bandwidth_index=1, freq_position=7, freq_shift=3, rx_ports=(2, 0),
                grid_index=0, result_index=0)
    return srsgpu.SrsResource(**dict(base, **changes))


# (what is wrong, the refusal's reason): every case is refused for its own reason.
REFUSED = ((dict(comb_offset=4), "Invalid SRS resource"), (dict(cyclic_shift=12), "Invalid SRS resource"),
           (dict(comb_size=2, comb_offset=1, cyclic_shift=8), "Invalid SRS resource"),
           (dict(freq_hopping=0), "frequency hopping"), (dict(hopping=1), "group or sequence hopping"),
           (dict(hopping=2), "group or sequence hopping"), (dict(rx_ports=()), "Empty list of Rx ports"),
           (dict(freq_shift=200), "exceeds maximum bandwidth"), (dict(start_symbol=13), "exceeds the number of symbols"),
           (dict(rx_ports=(0, 4)), "outside the grid"), (dict(rx_ports=(1, 2, 1)), "listed twice"),
           (dict(table_row=((48, 1), (22, 2), (12, 2), (4, 3))), "Table row"), (dict(table_row=((48, 2), (24, 2), (12, 2), (4, 3))), "Table row"),
           (dict(table_row=((48, 1), (24, 2), (12, 3), (4, 3))), "Table row"), (dict(nof_antenna_ports=3), "antenna ports"),
           (dict(nof_symbols=3), "number of symbols"), (dict(comb_size=3), "comb size"), (dict(numerology=5), "numerology"),
           (dict(grid_index=1), "grid_index"), (dict(result_index=1), "result_index"))


def test_refusals_leave_no_device_memory(ctx):
    import srsgpu
    before = srsgpu.live_device_buffers()
    for bad, reason in REFUSED:
        with pytest.raises(srsgpu.SrsGpuError, match=reason):
            srsgpu.SrsEstimatorPlan(ctx, [good_resource(**bad)], 52, 4, 1)
        assert srsgpu.live_device_buffers() == before, bad
    with pytest.raises(srsgpu.SrsGpuError, match="exceeds maximum bandwidth"):
        srsgpu.SrsEstimatorPlan(ctx, [good_resource()], 50, 4, 1)
    with pytest.raises(srsgpu.SrsGpuError, match="belongs to another resource"):
        srsgpu.SrsEstimatorPlan(ctx, [good_resource(), good_resource(freq_shift=0)], 52, 4, 1)
    assert srsgpu.live_device_buffers() == before
    plan = srsgpu.SrsEstimatorPlan(ctx, [good_resource()], 51, 4, 1)
    assert srsgpu.live_device_buffers() == before + 3
    plan.close()
    assert srsgpu.live_device_buffers() == before


def test_create_execute_destroy_leave_nothing_behind(ctx):
    import torch
    import srsgpu
    dev = torch.device("cuda", 0)
    before = srsgpu.live_device_buffers()
    for _ in range(3):
        plan = srsgpu.SrsEstimatorPlan(ctx, [good_resource(), good_resource(result_index=1, rx_ports=(1,))], 52, 4, 1)
        out = plan.run(np.zeros((1, 4, 14, 12 * 52), np.uint32))
        assert out.shape == (2,) and not out["channel"].any() and (out["ta_idx"] == 0).all()
        plan.close()
        plan.close()  # closing twice gives the plan back once
        assert srsgpu.live_device_buffers() == before
    empty = srsgpu.SrsEstimatorPlan(ctx, [], 52, 4, 1)
    empty.execute(torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.uint8, device=dev))
    empty.close()
    assert srsgpu.live_device_buffers() == before


def test_graph_replay_equals_eager(ctx):
    """One torch.cuda.graph capture of execute() replayed on two other sets of grids: each replay equals eager execution
    bit for bit."""
    import torch
    import srsgpu
    dev = torch.device("cuda", 0)
    cases, _ = C.golden()
    picked = [c for c in cases if c["name"] in ("L36_interleaved", "L120_idft256", "cs5_comb2", "pure_noise")]
    grid_prb = max(c["grid_nof_prb"] for c in picked)
    grid_of, nof_grids = C.pack(picked, grid_prb)
    inputs = []
    for seed in (1, 2, 3):
        noise = np.random.default_rng(seed)
        noisy = [C.to_bf16_words(C.words_to_complex(c["words"]) + 0.1 * C.awgn(noise, c["words"].shape)) for c in picked]
        grids = C.place(picked, noisy, grid_prb, GRID_PORTS, nof_grids, grid_of)  # the same layout, other samples
        inputs.append(torch.from_numpy(grids.view(np.int32)).to(dev))
    plan = srsgpu.SrsEstimatorPlan(ctx, resources_of(picked, grid_of), grid_prb, GRID_PORTS, nof_grids)
    size = srsgpu.SRS_RESULT_DTYPE.itemsize * len(picked)
    eager = []
    for d_grids in inputs:
        out = torch.full((size,), GUARD, dtype=torch.uint8, device=dev)
        plan.execute(d_grids, out)
        torch.cuda.synchronize(dev)
        eager.append(out.cpu().numpy().copy())
    assert not np.array_equal(eager[0], eager[1]) and not np.array_equal(eager[1], eager[2])
    static_input = inputs[0].clone()
    static_out = torch.full((size,), GUARD, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.execute(static_input, static_out)
    for d_grids, want in zip(inputs[1:], eager[1:]):
        static_input.copy_(d_grids)
        static_out.fill_(GUARD)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert np.array_equal(static_out.cpu().numpy(), want)
    plan.close()
