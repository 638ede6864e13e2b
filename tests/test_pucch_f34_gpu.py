"""srsgpu_pucch_f34_plan on the GPU: the fixture tests/golden/pucch_f34.npz in one plan against the reference (bits and
status through PucchF34Processor's three launches on the decidable cases, LLRs and channel state on all) and against
the float64 restatement (tests/pucch_f34_cases.py), a fresh random plan of both formats with NaN and 1e30 around every
allocation and in unused ports, guard bytes around the LLRs and odd LLR counts next to each other, the hand-made errors,
the refusals, destroy and re-create, graph replay and the composition with the Format 1 and Format 2 plans on one grid.

Tolerances, none fixed in advance: LLRs equal or one step apart; the share that differs from the restatement below ten
times what float32 arithmetic alone moves, floored at 1e-3 (C.llr_share_bound()); from the reference below the PUSCH
demodulator's 5 %; the channel state within ten times the measured reference-to-restatement deviation, floored at 1e-4
(C.tolerances()); the time alignment within that margin or one T_c (the reference reports 0 throughout)."""
import numpy as np
import pytest

import pucch_f34_cases as C

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
    common = dict(slot_index=cfg["slot_index"], starting_prb=cfg["starting_prb"], start_symbol_index=cfg["start_symbol"],
                  nof_symbols=cfg["nof_symbols"], rnti=cfg["rnti"], n_id_scrambling=cfg["n_id_scrambling"],
                  n_id_hopping=cfg["n_id_hopping"], nof_harq_ack=harq, nof_sr=sr, nof_csi_part1=a - harq - sr,
                  ports=cfg["ports"], second_hop_prb=None if cfg["second_hop_prb"] == C.NO_HOP else cfg["second_hop_prb"],
                  additional_dmrs=bool(cfg["additional_dmrs"]), pi2_bpsk=bool(cfg["pi2_bpsk"]), numerology=cfg["numerology"],
                  cp_extended=cfg["cp_extended"], grid_index=grid_index, llr_offset=llr_offset)
    if cfg["format"] == 4:
        return srsgpu.PucchF4(occ_length=cfg["occ_length"], occ_index=cfg["occ_index"], **common)
    return srsgpu.PucchF3(nof_prb=cfg["nof_prb"], **common)


def run(ctx, placed, grid_prb, nof_grids, llr_offsets=None):
    """One batch (three plans, three launches) over every (cfg, words, grid index) -> per PDU a dict in the
    restatement's layout plus bits and valid, and the PucchF2Result list. The LLR buffer is prefilled with GUARD:
    nothing outside the PDUs' ranges may change and every byte inside them must."""
    import torch
    import srsgpu
    dev = torch.device("cuda", 0)
    grids = C.place(placed, grid_prb, GRID_PORTS, nof_grids)
    pdus = [to_pdu(cfg, g, None if llr_offsets is None else llr_offsets[i]) for i, (cfg, _, g) in enumerate(placed)]
    for d, (cfg, *_) in zip(pdus, placed):
        assert d.nof_llrs == C.nof_llrs(cfg)
    batch = srsgpu.PucchF34Batch(ctx, pdus, grid_prb, GRID_PORTS, nof_grids)
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
        assert o % 4 == 0 and not inside[o: o + n].any()
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
    cases = C.random_plan_cases(np.random.default_rng(20345))
    placed = [(cfg, words, g) for cfg, words, g, _ in cases]
    grids = C.words_to_complex(C.place(placed, 52, GRID_PORTS, 8))
    want = [C.restate(cfg, grids[g]) for cfg, _, g in placed]
    # Neighbouring PDUs as close in the LLR stream as the alignment of 4 lets them be (odd counts leave 1..3 guard
    # bytes, whole counts none), four more guard bytes after every third.
    offs, o = [], 8
    for i, (cfg, *_) in enumerate(placed):
        offs.append(o)
        o += (C.nof_llrs(cfg) + 3) // 4 * 4 + (4 if i % 3 == 2 else 0)
    order = np.random.default_rng(5).permutation(len(placed))  # the PDUs' order is not the stream's order
    got = run(ctx, [placed[i] for i in order], 52, 8, [offs[i] for i in order])
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

    Measured on an MI355X: see DESIGN.md a6e-3."""
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
    assert decided >= 0.95 * len(cases)
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
        assert r.time_alignment == 0 and want["time_alignment"] == 0, c["cfg"]
        if np.isnan(want["cfo_hz"]):
            assert np.isnan(r.cfo_hz), c["cfg"]
        else:
            assert abs(r.cfo_hz - want["cfo_hz"]) <= 15.0 * tol["cfo"], c["cfg"]
        assert len(r.harq_ack) + len(r.sr) + len(r.csi_part1) == a and len(r.harq_ack) == min(a, 2)


def test_processor_gives_the_batch_results(ctx, fixture_run):
    """PucchF34Processor.process_batch (plans created, three launches, plans closed) on every tenth fixture PDU, with
    LLR offsets of its own choosing: the same payloads, status and channel state as in the plan of all of them."""
    import srsgpu
    cases = C.golden()
    ids = list(range(0, len(cases), 10))
    placed = [(cases[i]["cfg"], cases[i]["words"], k) for k, i in enumerate(ids)]
    grid_prb = max(cfg["grid_nof_prb"] for cfg, *_ in placed)
    before = srsgpu.live_device_buffers()
    got = srsgpu.PucchF34Processor(ctx, grid_prb, GRID_PORTS).process_batch(
        C.place(placed, grid_prb, GRID_PORTS, len(placed)), [to_pdu(cfg, g) for cfg, _, g in placed])
    assert srsgpu.live_device_buffers() == before
    for r, i in zip(got, ids):
        want = fixture_run[i]["result"]
        assert r.valid == want.valid and np.array_equal(r.payload, want.payload), cases[i]["cfg"]
        for key in ("noise_var", "rsrp", "epre", "time_alignment_ports"):
            assert np.array_equal(getattr(r, key), getattr(want, key)), (key, cases[i]["cfg"])
        assert np.array_equal(r.cfo_hz_ports, want.cfo_hz_ports, equal_nan=True)


def test_random_plan_against_the_restatement(random_run):
    """About 60 fresh PDUs of both formats over eight grids, NaN and 1e30 in every RE outside the allocations and in
    the ports no PDU lists, guard bytes around the LLRs and neighbouring PDUs next to each other in the stream in
    permuted order, odd counts among them (run() checks that nothing outside a PDU's range is written and every byte
    inside it is)."""
    placed, want, got = random_run
    cases = C.golden()
    tol = C.tolerances(C.measured_deviations(C.restate_golden(), cases))
    assert len(placed) >= 60 and len({g for *_, g in placed}) >= 4
    assert {cfg["format"] for cfg, *_ in placed} == {3, 4}
    assert sum(C.nof_llrs(cfg) % 4 != 0 for cfg, *_ in placed) >= 5
    check_against(got, want, [cfg for cfg, *_ in placed], tol, C.llr_share_bound(), "random plan vs restatement")
    for g in got:
        assert np.isfinite(g["noise_var"]).all() and np.isfinite(g["rsrp"]).all() and np.isfinite(g["epre"]).all()
        assert not g["ta"].any()


def test_perturbed_restatements_are_told_apart(fixture_run):
    """Each hand-made error moves the restatement away from the kernel on every fixture case it applies to
    (C.perturbation_applies: it moves at least four LLRs or a power by 1 % of the EPRE). Per-RE noise variances in place
    of the symbol mean apply to no case: with one estimate per hop every RE of a symbol has the same variance."""
    cases, restated = C.golden(), C.restate_golden()
    least = dict(idft_scale=100, per_re_noise=0, f4_noise_div_sf=30, pi2_parity_per_symbol=8, m0_swapped=30, hop_ceil=25,
                 no_bf16=40, data_port_i=8)
    assert set(least) == set(C.PERTURBATIONS)
    for name in C.PERTURBATIONS:
        count = 0
        for c, true, got in zip(cases, restated, fixture_run):
            pert = C.restate(c["cfg"], C.grid_of(c["cfg"], c["words"]), (name,))
            if not C.perturbation_applies(name, c["cfg"], true, pert):
                continue
            assert C.closer_to(got, true, pert), (name, c["cfg"])
            count += 1
        print(name, count, "cases")
        assert count >= least[name], (name, count)


def good_pdu(fmt=3, **changes):
    import srsgpu
    base = dict(slot_index=7, starting_prb=20, start_symbol_index=2, nof_symbols=8, rnti=0x4601, n_id_scrambling=500,
                n_id_hopping=400, nof_harq_ack=2, nof_sr=1, nof_csi_part1=17, ports=(2, 0), second_hop_prb=4, numerology=1,
                cp_extended=0, grid_index=1, llr_offset=1024)
    base.update(dict(nof_prb=3) if fmt == 3 else dict(occ_length=2, occ_index=1))
    base.update(changes)
    return (srsgpu.PucchF3 if fmt == 3 else srsgpu.PucchF4)(**base)


REFUSALS = (
    (3, dict(nof_prb=0), "outside the allowed range"),
    (3, dict(nof_prb=17, starting_prb=0, second_hop_prb=30), "outside the allowed range"),
    (3, dict(nof_prb=7), "not valid for the transform precoder"),
    (3, dict(nof_prb=11), "not valid for the transform precoder"),
    (3, dict(nof_prb=13), "not valid for the transform precoder"),
    (3, dict(nof_prb=14), "not valid for the transform precoder"),
    (3, dict(nof_symbols=3), "Invalid Number of OFDM symbols"),
    (3, dict(nof_symbols=15, start_symbol_index=0), "Invalid Number of OFDM symbols"),
    (4, dict(occ_length=3), "Invalid OCC length"),
    (4, dict(occ_length=4, occ_index=4), "Invalid sequence index"),
    (3, dict(starting_prb=50), "outside grid (first hop)"),
    (4, dict(second_hop_prb=52), "outside grid (second hop)"),
    (3, dict(start_symbol_index=7), "exceeding the number of symbols"),
    (3, dict(numerology=2, cp_extended=1, start_symbol_index=5), "extended CP"),
    (3, dict(numerology=1, cp_extended=1), "extended cyclic prefix"),
    (3, dict(slot_index=20), "slot index"),
    (3, dict(ports=()), "cannot be zero"),
    (3, dict(ports=(0, 1, 2, 3, 3)), "exceeds the configured maximum"),
    (3, dict(nof_csi_part1=0, nof_sr=0), "outside the supported range"),
    (3, dict(nof_csi_part1=1704), "effective code rate"),
    (4, dict(nof_csi_part1=120), "effective code rate"),
    (3, dict(ports=(2, 2)), "listed twice"),
    (3, dict(ports=(2, 4)), "outside the grid"),
    (3, dict(n_id_scrambling=1024), "outside 0..1023"),
    (4, dict(n_id_hopping=1024), "outside 0..1023"),
    (3, dict(grid_index=2), "grid_index"),
    (3, dict(llr_offset=1030), "multiple of 4"),
)


def test_refusals_leave_no_device_memory(ctx):
    import srsgpu
    before = srsgpu.live_device_buffers()
    for fmt, changes, message in REFUSALS:
        with pytest.raises(srsgpu.SrsGpuError, match=message.replace("(", r"\(").replace(")", r"\)")):
            srsgpu.PucchF34Plan(ctx, [good_pdu(llr_offset=0, nof_prb=2), good_pdu(fmt, **changes)], 52, GRID_PORTS, 2)
        assert srsgpu.live_device_buffers() == before, changes
    with pytest.raises(srsgpu.SrsGpuError, match="more ports|exceeds the configured maximum"):
        srsgpu.PucchF34Plan(ctx, [good_pdu(ports=(0, 1, 2))], 52, 2, 2)
    n = good_pdu().nof_llrs  # 3 PRB x 6 data symbols x QPSK
    assert n == 432 and good_pdu(4).nof_llrs == 72 and good_pdu(4, pi2_bpsk=True, occ_length=4, nof_symbols=4,
                                                                 second_hop_prb=None, nof_csi_part1=0).nof_llrs == 9
    with pytest.raises(srsgpu.SrsGpuError, match="overlap"):
        srsgpu.PucchF34Plan(ctx, [good_pdu(), good_pdu(llr_offset=1024 + n - 4)], 52, GRID_PORTS, 2)
    with pytest.raises(srsgpu.SrsGpuError, match="overlap"):
        srsgpu.PucchF34Plan(ctx, [good_pdu(), good_pdu(4)], 52, GRID_PORTS, 2)
    assert srsgpu.live_device_buffers() == before
    pdus = [good_pdu(), good_pdu(llr_offset=1024 + n), good_pdu(4, llr_offset=0)]
    for _ in range(2):  # destroy and re-create
        plan = srsgpu.PucchF34Plan(ctx, pdus, 52, GRID_PORTS, 2)
        assert srsgpu.live_device_buffers() == before + 4
        plan.close()
        assert srsgpu.live_device_buffers() == before
    empty = srsgpu.PucchF34Plan(ctx, [], 52, GRID_PORTS, 1)  # nothing to do is no error
    empty.execute(None, None, None)
    empty.close()
    assert srsgpu.live_device_buffers() == before


def test_recreated_plan_gives_the_same_results(ctx, fixture_run):
    """A plan destroyed and created again over every twentieth fixture PDU gives what the plan of all of them gave."""
    cases = C.golden()
    ids = list(range(0, len(cases), 20))
    placed = [(cases[i]["cfg"], cases[i]["words"], k) for k, i in enumerate(ids)]
    grid_prb = max(cfg["grid_nof_prb"] for cfg, *_ in placed)
    for _ in range(2):
        got = run(ctx, placed, grid_prb, len(placed))
        for g, i in zip(got, ids):
            assert np.array_equal(g["llrs"], fixture_run[i]["llrs"]) and np.array_equal(g["noise_var"], fixture_run[i]["noise_var"])


def test_graph_replay_equals_eager(ctx):
    """One torch.cuda.graph capture of the three launches replayed on two other sets of grids: each replay equals eager
    execution bit for bit, LLRs, channel state and decoded payloads."""
    import torch
    import srsgpu
    dev = torch.device("cuda", 0)
    cases = C.golden()
    picked = [c for c in cases if c["snr_class"] == C.CLASS_INFORMATIVE][::13][:9]
    assert {c["cfg"]["nof_uci_bits"] <= 11 for c in picked} == {True, False}
    assert {c["cfg"]["format"] for c in picked} == {3, 4}
    grid_prb = max(c["cfg"]["grid_nof_prb"] for c in picked)
    inputs = []
    for seed in (1, 2, 3):
        noise = np.random.default_rng(seed)
        placed = [(c["cfg"], C.complex_to_words(C.words_to_complex(c["words"]) + 0.2 * C.awgn(noise, c["words"].shape)), i)
                  for i, c in enumerate(picked)]
        inputs.append(torch.from_numpy(C.place(placed, grid_prb, GRID_PORTS, len(picked)).view(np.int32)).to(dev))
    batch = srsgpu.PucchF34Batch(ctx, [to_pdu(c["cfg"], i) for i, c in enumerate(picked)], grid_prb, GRID_PORTS, len(picked))
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


def test_composition_with_format_1_and_format_2(ctx):
    """A slot with a Format 1 resource, a Format 2 PDU and a Format 3 PDU on one grid, each through its own plan: each
    plan gives, byte for byte, what it gives on a grid that holds its own allocation alone, and the Format 3 PDU's
    LLRs are those of the fixture run's restatement."""
    import torch
    import srsgpu
    import pucch_cases as PC
    import pucch_f2_cases as C2
    dev = torch.device("cuda", 0)
    grid_prb = 52
    _, _, f1 = PC.golden()
    c1 = next(c for c in f1 if c["cfg"]["nof_ports"] == 2 and c["cfg"]["second_hop_prb"] != PC.NO_HOP)
    cfg1 = dict(c1["cfg"], starting_prb=2, second_hop_prb=3)
    c2 = next(c for c in C2.golden() if c["snr_class"] == C2.CLASS_INFORMATIVE and c["cfg"]["nof_prb"] <= 3
              and c["cfg"]["nof_symbols"] == 2 and c["cfg"]["second_hop_prb"] == C2.NO_HOP)
    cfg2 = dict(c2["cfg"], starting_prb=30, grid_nof_prb=grid_prb)
    c3 = next(c for c in C.golden() if c["snr_class"] == C.CLASS_INFORMATIVE and c["cfg"]["format"] == 3
              and c["cfg"]["nof_prb"] == 2 and C.hopping(c["cfg"]) and len(c["cfg"]["ports"]) == 2)
    cfg3 = dict(c3["cfg"], starting_prb=40, second_hop_prb=46, grid_nof_prb=grid_prb)
    alone = [PC.place([], [(cfg1, c1["words"])], grid_prb, GRID_PORTS, 1, PC.NAN_WORD, grid_of=lambda kind, i: 0),
             C2.place([(cfg2, c2["words"], 0)], grid_prb, GRID_PORTS, 1, fill=(C2.NAN_WORD,)),
             C.place([(cfg3, c3["words"], 0)], grid_prb, GRID_PORTS, 1, fill=(C.NAN_WORD,))]
    own = [g != np.uint32(C.NAN_WORD) for g in alone]
    assert not (own[0] & own[1]).any() and not (own[0] & own[2]).any() and not (own[1] & own[2]).any()
    both = np.full(alone[0].shape, C.NAN_WORD, np.uint32)
    for g, m in zip(alone, own):
        both[m] = g[m]
    detector = srsgpu.PucchDetectorPlan(ctx, [], [srsgpu.PucchF1(
        slot_index=cfg1["slot_index"], starting_prb=cfg1["starting_prb"], start_symbol_index=cfg1["start_symbol"],
        nof_symbols=cfg1["nof_symbols"], n_id=cfg1["n_id"], nof_rx_ports=cfg1["nof_ports"], entries=cfg1["entries"],
        second_hop_prb=cfg1["second_hop_prb"], numerology=cfg1["numerology"], cp_extended=cfg1["cp_extended"])],
        grid_prb, GRID_PORTS, 1)
    a2 = cfg2["nof_uci_bits"]
    batch2 = srsgpu.PucchF2Batch(ctx, [srsgpu.PucchF2(
        slot_index=cfg2["slot_index"], starting_prb=cfg2["starting_prb"], nof_prb=cfg2["nof_prb"],
        start_symbol_index=cfg2["start_symbol"], nof_symbols=cfg2["nof_symbols"], rnti=cfg2["rnti"], n_id=cfg2["n_id"],
        n_id_0=cfg2["n_id_0"], nof_harq_ack=2, nof_csi_part1=a2 - 2, ports=cfg2["ports"], numerology=cfg2["numerology"],
        cp_extended=cfg2["cp_extended"])], grid_prb, GRID_PORTS, 1)
    batch3 = srsgpu.PucchF34Batch(ctx, [to_pdu(cfg3, 0)], grid_prb, GRID_PORTS, 1)

    def run_all(g_detector, g_f2, g_f3):
        d = [torch.from_numpy(g.view(np.int32)).to(dev) for g in (g_detector, g_f2, g_f3)]
        d_det = torch.zeros(32 * detector.nof_results, dtype=torch.uint8, device=dev)
        detector.execute(d[0], d_det)
        batch2.launch(d[1])
        batch3.launch(d[2])
        torch.cuda.synchronize(dev)
        out = [d_det.cpu().numpy()]
        for b in (batch2, batch3):
            llrs, raw = b.raw()
            out += [llrs.copy(), np.frombuffer(raw.tobytes(), np.uint8), b.d_short_msgs.cpu().numpy(), b.d_polar_msgs.cpu().numpy()]
        return out, batch3.results()[0]

    separate, _ = run_all(*alone)
    together, res3 = run_all(both, both, both)
    for a, b in zip(separate, together):
        assert np.array_equal(a, b)
    want = C.restate(cfg3, C.grid_of(cfg3, c3["words"]))
    n, step = C.llr_diff(together[5], want["llrs"])
    assert step <= 1 and n <= max(2, 0.01 * len(want["llrs"])), (n, step)
    if c3["decidable"]:
        assert int(res3.valid) == c3["status"] and np.array_equal(res3.payload, c3["bits"])
    assert np.count_nonzero(together[1]) > 0
    detector.close()
    batch2.close()
    batch3.close()
