"""srsgpu_pucch_f2_plan on the GPU: the fixture tests/golden/pucch_f2.npz in one plan against the reference (bits and
status through PucchF2Processor's three launches on the decidable cases, LLRs and channel state on all) and against the
float64 restatement (tests/pucch_f2_cases.py), a fresh random plan with NaN and 1e30 around every allocation and guard
bytes around the LLRs, the hand-made errors, the refusals, graph replay and the composition with the other uplink plans
on one grid.

Tolerances, none fixed in advance: LLRs equal or one step apart; the share that differs from the restatement below ten
times what float32 arithmetic alone moves, floored at 1e-3 (C.llr_share_bound()); from the reference below the PUSCH
demodulator's 5 %; the channel state within ten times the measured reference-to-restatement deviation, floored at 1e-4
(C.tolerances()); the time alignment within that margin or one T_c."""
import numpy as np
import pytest

import pucch_f2_cases as C

pytestmark = pytest.mark.gpu

GUARD = -128  # no LLR takes it: they are clipped to +-120
GRID_PORTS = 4
REF_SHARE_BOUND = 0.05


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


def to_pdu(cfg, grid_index, llr_offset=None):
    import srsgpu
    a = cfg["nof_uci_bits"]
    harq = min(a, 2)  # a split of the payload: HARQ-ACK, SR, CSI Part 1
    sr = 1 if a - harq >= 2 else 0
    return srsgpu.PucchF2(slot_index=cfg["slot_index"], starting_prb=cfg["starting_prb"], nof_prb=cfg["nof_prb"],
                          start_symbol_index=cfg["start_symbol"], nof_symbols=cfg["nof_symbols"], rnti=cfg["rnti"],
                          n_id=cfg["n_id"], n_id_0=cfg["n_id_0"], nof_harq_ack=harq, nof_sr=sr, nof_csi_part1=a - harq - sr,
                          ports=cfg["ports"], second_hop_prb=None if cfg["second_hop_prb"] == C.NO_HOP else cfg["second_hop_prb"],
                          numerology=cfg["numerology"], cp_extended=cfg["cp_extended"], grid_index=grid_index,
                          llr_offset=llr_offset)


def run(ctx, placed, grid_prb, nof_grids, llr_offsets=None):
    """One batch (three plans, three launches) over every (cfg, words, grid index) -> per PDU a dict in the
    restatement's layout plus bits and valid, and the PucchF2Result list. The LLR buffer is prefilled with GUARD and
    nothing outside the PDUs' ranges may change."""
    import torch
    import srsgpu
    dev = torch.device("cuda", 0)
    grids = C.place(placed, grid_prb, GRID_PORTS, nof_grids)
    pdus = [to_pdu(cfg, g, None if llr_offsets is None else llr_offsets[i]) for i, (cfg, _, g) in enumerate(placed)]
    batch = srsgpu.PucchF2Batch(ctx, pdus, grid_prb, GRID_PORTS, nof_grids)
    batch.d_llrs.fill_(GUARD)
    batch.d_results.fill_(0xA5)
    batch.launch(torch.from_numpy(grids.view(np.int32)).to(dev))
    torch.cuda.synchronize(dev)
    all_llrs = batch.d_llrs.cpu().numpy()
    _, raw = batch.raw()
    results = batch.results()
    offs = batch.front.llr_offsets
    batch.close()
    inside = np.zeros(all_llrs.size, bool)
    out = []
    for (cfg, *_), o, rec, res in zip(placed, offs, raw, results):
        n, P = C.nof_llrs(cfg), len(cfg["ports"])
        inside[o: o + n] = True
        for key in ("noise_var", "rsrp", "epre", "cfo_hz", "time_alignment"):
            assert not rec[key][P:].any(), (key, cfg)  # entries of ports past nof_ports are written as zero
        out.append(dict(llrs=all_llrs[o: o + n].copy(), noise_var=rec["noise_var"][:P].astype(np.float64),
                        rsrp=rec["rsrp"][:P].astype(np.float64), epre=rec["epre"][:P].astype(np.float64),
                        ta=rec["time_alignment"][:P].copy(), cfo_hz=rec["cfo_hz"][:P].astype(np.float64),
                        bits=res.payload, valid=res.valid, result=res))
    assert (all_llrs[~inside] == GUARD).all(), "an LLR outside every PDU's range was written"
    assert not (all_llrs[inside] == GUARD).any(), "an LLR of a PDU was not written"
    return out


@pytest.fixture(scope="module")
def fixture_run(ctx):
    cases = C.golden()
    placed = [(c["cfg"], c["words"], i) for i, c in enumerate(cases)]
    return run(ctx, placed, max(c["cfg"]["grid_nof_prb"] for c in cases), len(cases))


@pytest.fixture(scope="module")
def random_run(ctx):
    cases = C.random_plan_cases(np.random.default_rng(20273))
    placed = [(cfg, words, g) for cfg, words, g, _ in cases]
    grids = C.grids_to_complex(C.place(placed, 52, GRID_PORTS, 6))
    want = [C.restate(cfg, grids[g]) for cfg, _, g in placed]
    # Neighbouring PDUs adjacent in the LLR stream, four guard bytes after every third.
    offs, o = [], 8
    for i, (cfg, *_) in enumerate(placed):
        offs.append(o)
        o += C.nof_llrs(cfg) + (4 if i % 3 == 2 else 0)
    order = np.random.default_rng(5).permutation(len(placed))  # the PDUs' order is not the stream's order
    got = run(ctx, [placed[i] for i in order], 52, 6, [offs[i] for i in order])
    back = np.argsort(order)
    return placed, want, [got[i] for i in back]


def check_against(got, want, cases_cfg, tol, share_bound, what):
    diff = total = 0
    worst = {k: 0.0 for k in tol}
    for g, w, cfg in zip(got, want, cases_cfg):
        n, step = C.llr_diff(g["llrs"], w["llrs"])
        assert step <= 1, (what, cfg, step)
        diff, total = diff + n, total + len(w["llrs"])
        for k, v in C.state_deviation(g, w).items():
            worst[k] = max(worst[k], v)
            assert v <= tol[k], (what, k, v, tol[k], cfg)
    share = diff / total
    print(f"{what}: LLR share differing {share:.2e} of {total} (bound {share_bound:.2e});",
          {k: f"{v:.2e}" for k, v in worst.items()})
    assert share < share_bound, (what, share, share_bound)


def test_fixture_in_one_plan(fixture_run):
    """Every fixture PDU in one plan, one grid each. Against the restatement on every case and against the reference on
    every case for the LLRs, the per-port and the combined channel state; bits and status against the reference on the
    decidable cases.

    Measured on an MI355X: see DESIGN.md a6e-2."""
    cases, restated = C.golden(), C.restate_golden()
    tol = C.tolerances(C.measured_deviations(restated, cases))
    cfgs = [c["cfg"] for c in cases]
    check_against(fixture_run, restated, cfgs, tol, C.llr_share_bound(), "kernel vs restatement")
    check_against(fixture_run, cases, cfgs, tol, REF_SHARE_BOUND, "kernel vs reference")
    decided = 0
    for g, c in zip(fixture_run, cases):  # (the reference's decoder writes its bits on an invalid payload too)
        if not c["decidable"]:
            continue
        assert int(g["valid"]) == c["status"] and np.array_equal(g["bits"], c["bits"]), c["cfg"]
        decided += 1
    assert decided >= 0.98 * len(cases)
    # The combined channel state against what the reference's get_channel_state_information reported for the case. A
    # power within `tol` of the EPRE moves a ratio in dB by 10 log10(e) times its share of that power.
    db = 10 / np.log(10)
    for g, c in zip(fixture_run, cases):
        r, want, a = g["result"], c["csi"], c["cfg"]["nof_uci_bits"]
        epre, rsrp, nv = (float(np.sum(c[k], dtype=np.float64)) for k in ("epre", "rsrp", "noise_var"))
        with np.errstate(divide="ignore"):
            margins = dict(epre_db=db * tol["epre"], rsrp_db=db * tol["rsrp"] * epre / rsrp if rsrp > 0 else np.inf,
                           sinr_db=db * (tol["rsrp"] * epre / rsrp + tol["noise_var"] * epre / nv) if rsrp > 0 and nv > 0 else np.inf)
        for key, have in (("epre_db", r.epre_dB), ("rsrp_db", r.rsrp_dB), ("sinr_db", r.sinr_dB)):
            if np.isfinite(want[key]) and np.isfinite(margins[key]):
                assert abs(have - want[key]) <= margins[key] + 1e-5, (key, have, want[key], c["cfg"])
        assert abs(r.time_alignment - want["time_alignment"]) <= tol["ta"] * C.T_C, c["cfg"]
        if np.isnan(want["cfo_hz"]):
            assert np.isnan(r.cfo_hz), c["cfg"]
        else:
            assert abs(r.cfo_hz - want["cfo_hz"]) <= 15.0 * tol["cfo"], c["cfg"]
        assert len(r.harq_ack) + len(r.sr) + len(r.csi_part1) == a and len(r.harq_ack) == min(a, 2)


def test_processor_gives_the_batch_results(ctx, fixture_run):
    """PucchF2Processor.process_batch (plans created, three launches, plans closed) on every tenth fixture PDU, with
    LLR offsets of its own choosing: the same payloads, status and channel state as in the plan of all of them."""
    import srsgpu
    cases = C.golden()
    ids = list(range(0, len(cases), 10))
    placed = [(cases[i]["cfg"], cases[i]["words"], k) for k, i in enumerate(ids)]
    grid_prb = max(cfg["grid_nof_prb"] for cfg, *_ in placed)
    before = srsgpu.live_device_buffers()
    got = srsgpu.PucchF2Processor(ctx, grid_prb, GRID_PORTS).process_batch(
        C.place(placed, grid_prb, GRID_PORTS, len(placed)), [to_pdu(cfg, g) for cfg, _, g in placed])
    assert srsgpu.live_device_buffers() == before
    for r, i in zip(got, ids):
        want = fixture_run[i]["result"]
        assert r.valid == want.valid and np.array_equal(r.payload, want.payload), cases[i]["cfg"]
        for key in ("noise_var", "rsrp", "epre", "time_alignment_ports"):
            assert np.array_equal(getattr(r, key), getattr(want, key)), (key, cases[i]["cfg"])
        assert np.array_equal(r.cfo_hz_ports, want.cfo_hz_ports, equal_nan=True)


def test_random_plan_against_the_restatement(random_run):
    """About 60 fresh PDUs over six grids, NaN and 1e30 in every RE outside the allocations, guard bytes around the
    LLRs and neighbouring PDUs adjacent in the stream (run() checks that nothing outside a PDU's range is written)."""
    placed, want, got = random_run
    cases = C.golden()
    tol = C.tolerances(C.measured_deviations(C.restate_golden(), cases))
    assert len(placed) >= 60 and len({g for *_, g in placed}) >= 4
    check_against(got, want, [cfg for cfg, *_ in placed], tol, C.llr_share_bound(), "random plan vs restatement")
    for g in got:
        assert np.isfinite(g["noise_var"]).all() and np.isfinite(g["rsrp"]).all() and np.isfinite(g["epre"]).all()


def test_perturbed_restatements_are_told_apart(fixture_run):
    """Each of the six hand-made errors moves the restatement away from the kernel on every fixture case it applies to
    (C.perturbation_applies: it moves at least four LLRs, a power by 1 % of the EPRE or the time alignment by two
    T_c)."""
    cases, restated = C.golden(), C.restate_golden()
    for name in C.PERTURBATIONS:
        count = 0
        for c, true, got in zip(cases, restated, fixture_run):
            pert = C.restate(c["cfg"], C.grid_of(c["cfg"], c["words"]), (name,))
            if not C.perturbation_applies(name, c["cfg"], true, pert):
                continue
            assert C.closer_to(got, true, pert), (name, c["cfg"])
            count += 1
        print(name, count, "cases")
        assert count >= 10, (name, count)


def good_pdu(**changes):
    import srsgpu
    base = dict(slot_index=7, starting_prb=20, nof_prb=3, start_symbol_index=12, nof_symbols=2, rnti=0x4601, n_id=500,
                n_id_0=40000, nof_harq_ack=2, nof_sr=1, nof_csi_part1=17, ports=(2, 0), second_hop_prb=4, numerology=1,
                cp_extended=0, grid_index=1, llr_offset=64)
    base.update(changes)
    return srsgpu.PucchF2(**base)


REFUSALS = (
    (dict(nof_prb=0), "Invalid Number of PRB"),
    (dict(nof_prb=17, starting_prb=0, second_hop_prb=30), "Invalid Number of PRB"),
    (dict(nof_symbols=0), "Invalid Number of OFDM symbols"),
    (dict(nof_symbols=3, start_symbol_index=0), "Invalid Number of OFDM symbols"),
    (dict(nof_symbols=1, nof_csi_part1=5), "Frequency hopping requires 2"),
    (dict(starting_prb=50), "outside grid (first hop)"),
    (dict(second_hop_prb=50), "outside grid (second hop)"),
    (dict(start_symbol_index=13), "exceeding the number of symbols"),
    (dict(numerology=2, cp_extended=1, start_symbol_index=11), "extended CP"),
    (dict(ports=()), "cannot be zero"),
    (dict(ports=(0, 1, 2, 3, 3)), "exceeds the configured maximum"),
    (dict(nof_csi_part1=0, nof_sr=0), "Payload length must be 3 to 1706"),
    (dict(nof_csi_part1=1704), "effective code rate"),
    (dict(nof_csi_part1=63), "effective code rate"),
    (dict(ports=(2, 2)), "listed twice"),
    (dict(ports=(2, 4)), "outside the grid"),
    (dict(grid_index=2), "grid_index"),
    (dict(llr_offset=6), "multiple of 4"),
)


def test_refusals_leave_no_device_memory(ctx):
    import srsgpu
    before = srsgpu.live_device_buffers()
    for changes, message in REFUSALS:
        with pytest.raises(srsgpu.SrsGpuError, match=message.replace("(", r"\(").replace(")", r"\)")):
            srsgpu.PucchF2Plan(ctx, [good_pdu(llr_offset=0, nof_prb=2), good_pdu(**changes)], 52, GRID_PORTS, 2)
        assert srsgpu.live_device_buffers() == before, changes
    with pytest.raises(srsgpu.SrsGpuError, match="more ports|exceeds the configured maximum"):
        srsgpu.PucchF2Plan(ctx, [good_pdu(ports=(0, 1, 2))], 52, 2, 2)
    with pytest.raises(srsgpu.SrsGpuError, match="overlap"):
        srsgpu.PucchF2Plan(ctx, [good_pdu(), good_pdu(llr_offset=64 + 92)], 52, GRID_PORTS, 2)
    with pytest.raises(srsgpu.SrsGpuError, match="overlap"):
        srsgpu.PucchF2Plan(ctx, [good_pdu(), good_pdu()], 52, GRID_PORTS, 2)
    assert srsgpu.live_device_buffers() == before
    plan = srsgpu.PucchF2Plan(ctx, [good_pdu(), good_pdu(llr_offset=160), good_pdu(llr_offset=0, nof_prb=2)], 52, GRID_PORTS, 2)
    assert srsgpu.live_device_buffers() == before + 4
    plan.close()
    assert srsgpu.live_device_buffers() == before
    empty = srsgpu.PucchF2Plan(ctx, [], 52, GRID_PORTS, 1)  # nothing to do is no error
    empty.execute(None, None, None)
    empty.close()
    assert srsgpu.live_device_buffers() == before


def test_graph_replay_equals_eager(ctx):
    """One torch.cuda.graph capture of the three launches replayed on two other sets of grids: each replay equals eager
    execution bit for bit, LLRs, channel state and decoded payloads."""
    import torch
    import srsgpu
    dev = torch.device("cuda", 0)
    cases = C.golden()
    picked = [c for c in cases if c["snr_class"] == C.CLASS_INFORMATIVE][::9][:8]
    assert {c["cfg"]["nof_uci_bits"] <= 11 for c in picked} == {True, False}
    grid_prb = max(c["cfg"]["grid_nof_prb"] for c in picked)
    inputs = []
    for seed in (1, 2, 3):
        noise = np.random.default_rng(seed)
        placed = [(c["cfg"], C.complex_to_words(C.words_to_complex(c["words"]) + 0.2 * C.awgn(noise, c["words"].shape)), i)
                  for i, c in enumerate(picked)]
        inputs.append(torch.from_numpy(C.place(placed, grid_prb, GRID_PORTS, len(picked)).view(np.int32)).to(dev))
    batch = srsgpu.PucchF2Batch(ctx, [to_pdu(c["cfg"], i) for i, c in enumerate(picked)], grid_prb, GRID_PORTS, len(picked))
    outputs = (batch.d_llrs, batch.d_results, batch.d_short_msgs, batch.d_short_status, batch.d_polar_msgs,
               batch.d_polar_status)

    def snapshot():
        torch.cuda.synchronize(dev)
        return [t.cpu().numpy().copy() for t in outputs]

    eager = []
    for d_grids in inputs:
        for t in outputs:
            t.fill_(0x5A)
        batch.launch(d_grids)
        eager.append(snapshot())
    assert not np.array_equal(eager[0][0], eager[1][0]) and not np.array_equal(eager[1][0], eager[2][0])
    static_input = inputs[0].clone()
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        batch.launch(static_input)
    for d_grids, want in zip(inputs[1:], eager[1:]):
        static_input.copy_(d_grids)
        for t in outputs:
            t.fill_(0x5A)
        graph.replay()
        for have, w in zip(snapshot(), want):
            assert np.array_equal(have, w)
    del graph
    batch.close()


def test_composition_with_the_other_uplink_plans(ctx):
    """A slot with a Format 0 PDU, a Format 1 resource, Format 2 PDUs and an SRS resource on one grid: each plan gives,
    byte for byte, what it gives on a grid that holds its own allocation alone."""
    import torch
    import srsgpu
    import pucch_cases as PC
    import srs_cases as SC
    dev = torch.device("cuda", 0)
    grid_prb = 52
    _, f0, f1 = PC.golden()
    c0 = next(c for c in f0 if len(c["cfg"]["ports"]) == 2 and c["cfg"]["nof_symbols"] == 2)
    c1 = next(c for c in f1 if c["cfg"]["nof_ports"] == 2 and c["cfg"]["second_hop_prb"] != PC.NO_HOP)
    cfg0 = dict(c0["cfg"], starting_prb=0, second_hop_prb=1 if c0["cfg"]["second_hop_prb"] != PC.NO_HOP else PC.NO_HOP)
    cfg1 = dict(c1["cfg"], starting_prb=2, second_hop_prb=3)
    srs_cases, _ = SC.golden()
    srs = next(c for c in srs_cases if c["name"] == "L24_comb2")
    small = [c for c in C.golden() if c["snr_class"] == C.CLASS_INFORMATIVE and c["cfg"]["nof_prb"] <= 3
             and c["cfg"]["nof_symbols"] == 2]
    f2 = [c for c in small if c["cfg"]["nof_uci_bits"] <= 11][:1] + [c for c in small if c["cfg"]["nof_uci_bits"] >= 12][:2]
    assert len(f2) == 3
    f2_placed = []
    for j, c in enumerate(f2):  # PRBs 30.. and 40.., apart from the detector's PRBs 0..3
        cfg = dict(c["cfg"], starting_prb=30 + 3 * j, grid_nof_prb=grid_prb,
                   second_hop_prb=C.NO_HOP if c["cfg"]["second_hop_prb"] == C.NO_HOP else 40 + 3 * j)
        f2_placed.append((cfg, c["words"], 0))

    def pucch_grid():
        return PC.place([(cfg0, c0["words"])], [(cfg1, c1["words"])], grid_prb, GRID_PORTS, 1, PC.NAN_WORD,
                        grid_of=lambda kind, i: 0)

    def srs_grid():
        return SC.place([srs], [srs["words"]], grid_prb, GRID_PORTS, 1, [0], SC.NAN_WORD)

    alone = [pucch_grid(), C.place(f2_placed, grid_prb, GRID_PORTS, 1, fill=(C.NAN_WORD,)), srs_grid()]
    own = [g != np.uint32(C.NAN_WORD) for g in alone]
    assert not (own[0] & own[1]).any() and not (own[0] & own[2]).any() and not (own[1] & own[2]).any()
    both = np.full(alone[0].shape, C.NAN_WORD, np.uint32)
    for g, m in zip(alone, own):
        both[m] = g[m]

    detector = srsgpu.PucchDetectorPlan(ctx, [srsgpu.PucchF0(
        slot_index=cfg0["slot_index"], starting_prb=cfg0["starting_prb"], start_symbol_index=cfg0["start_symbol"],
        nof_symbols=cfg0["nof_symbols"], initial_cyclic_shift=cfg0["initial_cyclic_shift"], n_id=cfg0["n_id"],
        nof_harq_ack=cfg0["nof_harq_ack"], sr_opportunity=cfg0["sr_opportunity"], ports=cfg0["ports"],
        second_hop_prb=None if cfg0["second_hop_prb"] == PC.NO_HOP else cfg0["second_hop_prb"],
        numerology=cfg0["numerology"], cp_extended=cfg0["cp_extended"])], [srsgpu.PucchF1(
            slot_index=cfg1["slot_index"], starting_prb=cfg1["starting_prb"], start_symbol_index=cfg1["start_symbol"],
            nof_symbols=cfg1["nof_symbols"], n_id=cfg1["n_id"], nof_rx_ports=cfg1["nof_ports"], entries=cfg1["entries"],
            second_hop_prb=cfg1["second_hop_prb"], numerology=cfg1["numerology"], cp_extended=cfg1["cp_extended"])],
        grid_prb, GRID_PORTS, 1)
    estimator = srsgpu.SrsEstimatorPlan(ctx, [srsgpu.SrsResource(
        table_row=srs["row"], numerology=srs["numerology"], nof_antenna_ports=srs["nof_antenna_ports"],
        nof_symbols=srs["nof_symbols"], start_symbol=srs["start_symbol"], comb_size=srs["comb_size"],
        comb_offset=srs["comb_offset"], cyclic_shift=srs["cyclic_shift"], sequence_id=srs["sequence_id"],
        bandwidth_index=srs["bandwidth_index"], freq_position=srs["freq_position"], freq_shift=srs["freq_shift"],
        rx_ports=srs["rx_ports"])], grid_prb, GRID_PORTS, 1)
    batch = srsgpu.PucchF2Batch(ctx, [to_pdu(cfg, 0) for cfg, *_ in f2_placed], grid_prb, GRID_PORTS, 1)

    def run_all(g_detector, g_f2, g_srs):
        d = [torch.from_numpy(g.view(np.int32)).to(dev) for g in (g_detector, g_f2, g_srs)]
        d_det = torch.zeros(32 * detector.nof_results, dtype=torch.uint8, device=dev)
        d_srs = torch.zeros(srsgpu.SRS_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        detector.execute(d[0], d_det)
        batch.launch(d[1])
        estimator.execute(d[2], d_srs)
        torch.cuda.synchronize(dev)
        llrs, raw = batch.raw()
        return [d_det.cpu().numpy(), llrs.copy(), raw.tobytes(), batch.d_short_msgs.cpu().numpy(),
                batch.d_polar_msgs.cpu().numpy(), d_srs.cpu().numpy()]

    separate = run_all(*alone)
    together = run_all(both, both, both)
    for a, b in zip(separate, together):
        assert np.array_equal(np.frombuffer(a, np.uint8) if isinstance(a, bytes) else a,
                              np.frombuffer(b, np.uint8) if isinstance(b, bytes) else b)
    assert np.count_nonzero(separate[1]) > 0
    for plan in (detector, estimator):
        plan.close()
    batch.close()
