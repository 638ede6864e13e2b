"""GPU parity of the PDCCH plan (DCI encoding, scrambling, QPSK, precoding, RE mapping and DM-RS in one launch;
srsgpu_pdcch_plan through the C ABI) against the reference's own grid words (tests/golden/pdcch.npz, made by
pdcch_processor_impl built from its sources) and against the numpy restatement tests/pdcch_cases.py, which
tests/test_pdcch_oracle.py pins to the same fixture. Every comparison is exact: identical bf16 grid words, and every
word no DCI owns still holding the prefill."""
import numpy as np
import pytest

import pdcch_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(C.SENTINEL)


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


@pytest.fixture(scope="module")
def random_plan():
    """The random plan's DCIs and the grids the restatement expects, computed once."""
    cases = C.random_plan_cases(np.random.default_rng(41))
    want = np.full((4, 4, 14, 12 * 52), SENTINEL, np.uint32)
    for cfg, payload in cases:
        C.apply_rows(want[cfg["grid_index"]], C.process(cfg, payload)[2])
    return cases, want


def to_dci(cfg, payload, grid_index=None):
    import srsgpu
    return srsgpu.Pdcch(
        bwp_size_rb=cfg["bwp_size_rb"], bwp_start_rb=cfg["bwp_start_rb"], start_symbol=cfg["start_symbol"],
        duration=cfg["duration"], frequency_resources=cfg["frequency_resources"], mapping=cfg["mapping"],
        slot_index=cfg["n_slot"], rnti=cfg["rnti"], n_id_pdcch_dmrs=cfg["n_id_dmrs"], n_id_pdcch_data=cfg["n_id_data"],
        n_rnti=cfg["n_rnti"], cce_index=cfg["cce_index"], aggregation_level=cfg["aggregation_level"], payload=payload,
        weights=cfg["weights"], reg_bundle_size=cfg["reg_bundle_size"], interleaver_size=cfg["interleaver_size"],
        shift_index=cfg["shift_index"], data_scaling=float(cfg["data_scaling"]),
        dmrs_amplitude=float(cfg["dmrs_amplitude"]), grid_index=cfg.get("grid_index", 0) if grid_index is None else grid_index)


def run(ctx, dcis, grid_nof_prb, grid_nof_ports, nof_grids, payloads=None, offsets=None):
    """The grids (nof_grids, ports, 14, nsc) uint32 after one execute over sentinel-filled grids."""
    import torch
    import srsgpu
    dev = torch.device("cuda", 0)
    if payloads is None:
        payloads, offsets = srsgpu.pdcch_pack_payloads(dcis)
    plan = srsgpu.PdcchPlan(ctx, dcis, grid_nof_prb, grid_nof_ports, nof_grids, offsets)
    d_payloads = torch.from_numpy(np.ascontiguousarray(payloads)).to(dev)
    d_grids = torch.from_numpy(np.full((nof_grids, grid_nof_ports, 14, 12 * grid_nof_prb), SENTINEL, np.uint32)
                               .view(np.int32)).to(dev)
    plan.execute(d_payloads, d_grids)
    torch.cuda.synchronize(dev)
    plan.close()
    return d_grids.cpu().numpy().view(np.uint32)


def expected(rows, grid_nof_prb, grid_nof_ports):
    want = np.full((grid_nof_ports, 14, 12 * grid_nof_prb), SENTINEL, np.uint32)
    C.apply_rows(want, rows)
    return want


def test_pdcch_golden_each_alone(ctx):
    """Every fixture DCI in a plan of its own, in a grid of the case's PRBs and ports."""
    count = 0
    for cfg, payload, _mask, _enc, rows in C.golden_cases():
        got = run(ctx, [to_dci(cfg, payload)], cfg["grid_nof_prb"], cfg["grid_nof_ports"], 1)
        assert np.array_equal(got[0], expected(rows, cfg["grid_nof_prb"], cfg["grid_nof_ports"])), cfg
        count += 1
    assert count > 60


def test_pdcch_golden_one_plan(ctx):
    """All fixture DCIs in ONE plan and one launch, each in a grid of its own of 106 PRB x 4 ports."""
    cases = list(C.golden_cases())
    got = run(ctx, [to_dci(c[0], c[1], i) for i, c in enumerate(cases)], 106, 4, len(cases))
    for i, (cfg, _payload, _mask, _enc, rows) in enumerate(cases):
        assert np.array_equal(got[i], expected(rows, 106, 4)), (i, cfg)


def test_pdcch_random_plan(ctx, random_plan):
    """About 200 DCIs over 4 grids of 52 PRB x 4 ports, several per grid on disjoint CCEs of CORESETs of all three
    mapping types, payloads at unaligned byte offsets between random guard bytes; and the same DCIs packed again
    with other guard bytes, offsets and padding bits give the same grids."""
    cases, want = random_plan
    assert len(cases) >= 150 and {c["grid_index"] for c, _ in cases} == {0, 1, 2, 3}
    assert {c["aggregation_level"] for c, _ in cases} >= {1, 2, 4, 8}
    dcis = [to_dci(c, p) for c, p in cases]
    for seed in (1, 2):
        payloads, offsets = C.pack_payloads(np.random.default_rng(seed), [p for _, p in cases])
        assert any(o % 4 for o in offsets)
        got = run(ctx, dcis, 52, 4, 4, payloads, offsets)
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def smallest_shapes():
    rng = np.random.default_rng(43)
    single = dict(mapping=C.NON_INTERLEAVED, bwp_start_rb=0, bwp_size_rb=52, frequency_resources=0b100, duration=1,
                  start_symbol=13)
    top = dict(C.TEMPLATES[2], duration=1, start_symbol=0)  # six resources from PRB 4: CCE 5 ends on PRB 51
    shapes = (("level 1, 12 bits", dict(C.TEMPLATES[0], aggregation_level=1, cce_index=7), 12),
              ("one 6-PRB resource, duration 1", dict(single, aggregation_level=1, cce_index=0), 83),
              ("level 16, duration 3", dict(C.TEMPLATES[9], aggregation_level=16, cce_index=2), 128),
              ("level 16, duration 3, CORESET0", dict(C.TEMPLATES[13], duration=3, aggregation_level=16, cce_index=8), 12),
              ("highest PRB of the grid", dict(top, aggregation_level=1, cce_index=5), 40),
              ("highest PRB, interleaved", dict(C.TEMPLATES[8], aggregation_level=8, cce_index=10), 64))
    out = []
    for i, (name, base, a) in enumerate(shapes):
        cfg, payload = C.fill_dci(rng, base, a)
        ports = (1, 4, 2, 4, 1, 3)[i]
        cfg.update(nof_ports=ports, weights=C.random_weights(rng, ports), data_scaling=C.F(0.5 + i / 4),
                   dmrs_amplitude=C.F(1.25))
        out.append(pytest.param(cfg, payload, id=name))
    return out


@pytest.mark.parametrize("cfg,payload", smallest_shapes())
def test_pdcch_smallest_shapes(ctx, cfg, payload):
    assert C.refusal(cfg, payload.size, 52, 4) is None
    rows = C.process(cfg, payload)[2]
    got = run(ctx, [to_dci(cfg, payload)], 52, 4, 1)
    assert np.array_equal(got[0], expected(rows, 52, 4))


def test_pdcch_shapes_reach_the_edges():
    """The parametrised shapes hold what they are named for."""
    shapes = {p.id: p.values for p in smallest_shapes()}
    assert max(C.cce_prbs(shapes["highest PRB of the grid"][0])) == 51
    assert max(C.cce_prbs(shapes["highest PRB, interleaved"][0])) == 51
    assert len(C.cce_prbs(shapes["one 6-PRB resource, duration 1"][0])) == 6
    assert len(C.cce_prbs(shapes["level 16, duration 3"][0])) == 32


def test_pdcch_graph_replay_with_fresh_payloads(ctx):
    """One capture, replays with new payload bytes in the same device buffer: each replay equals the eager run."""
    import torch
    import srsgpu
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(44)
    cases = C.random_plan_cases(rng, nof_grids=1, per_grid=24)
    dcis = [to_dci(c, p) for c, p in cases]
    _, offsets = srsgpu.pdcch_pack_payloads(dcis)
    plan = srsgpu.PdcchPlan(ctx, dcis, 52, 4, 1, offsets)
    d_payloads = torch.zeros(plan.payload_bytes, dtype=torch.uint8, device=dev)
    d_grids = torch.zeros(4 * 14 * 12 * 52, dtype=torch.int32, device=dev)

    def result():
        torch.cuda.synchronize(dev)
        got = d_grids.cpu().numpy().view(np.uint32).copy()
        d_grids.fill_(int(np.int32(-7)))
        return got

    sets = []
    for _ in range(3):
        fresh = [rng.integers(0, 2, p.size).astype(np.uint8) for _, p in cases]
        packed = torch.from_numpy(np.concatenate([np.packbits(p) for p in fresh])).to(dev)
        want = np.full((4, 14, 12 * 52), np.uint32(0xFFFFFFF9), np.uint32)
        for (cfg, _), p in zip(cases, fresh):
            C.apply_rows(want, C.process(cfg, p)[2])
        sets.append((packed, want.ravel()))
    result()
    eager = []
    for packed, want in sets:
        d_payloads.copy_(packed)
        plan.execute(d_payloads, d_grids)
        eager.append(result())
        assert np.array_equal(eager[-1], want)
    assert not np.array_equal(eager[0], eager[1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.execute(d_payloads, d_grids)
    result()  # the capture does not execute; clear again
    for (packed, _), e in list(zip(sets, eager))[::-1]:
        d_payloads.copy_(packed)
        graph.replay()
        assert np.array_equal(result(), e)
    plan.close()


def test_pdcch_composes_with_pdsch(ctx):
    """One grid: two DCIs on symbols 0-1, a PDSCH with its DM-RS from symbol 2. Either launch order gives the
    PDSCH-only grid plus the PDCCH-only grid."""
    import torch
    import srsgpu
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(45)
    coreset = dict(C.TEMPLATES[5], start_symbol=0)  # interleaved, two symbols, PRBs 4..51
    dcis = []
    for cce, al, a in ((0, 4, 41), (4, 8, 100)):
        cfg, payload = C.fill_dci(rng, dict(coreset, aggregation_level=al, cce_index=cce), a)
        cfg.update(nof_ports=2, weights=C.random_weights(rng, 2), data_scaling=C.F(1), dmrs_amplitude=C.F(1))
        dcis.append(to_dci(cfg, payload))
    w = (rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2))).astype(np.complex64) / 2
    mod = srsgpu.PdschModulation(rnti=0x4601, n_id=77, modulation_order=4, nof_layers=2, nof_ports=2, bwp_start_rb=0,
                                 bwp_size_rb=52, rb_start=0, nof_rb=52, start_symbol=2, nof_symbols=12,
                                 dmrs_symbol_mask=1 << 2, dmrs_type=1, nof_cdm_groups_without_data=2, scaling=1.0, weights=w)
    dmrs = srsgpu.PdschDmrs(slot_index=3, scrambling_id=77, n_scid=0, dmrs_type=1, nof_layers=2, nof_ports=2,
                            dmrs_symbol_mask=1 << 2, reference_point_k_rb=0, rb_start=0, nof_rb=52, amplitude=1.0, weights=w)
    nbits = mod.nof_re(52) * 2 * 4
    d_cw = torch.from_numpy(rng.integers(0, 256, (nbits + 7) // 8 + 4).astype(np.uint8)).to(dev)
    mod_plan = srsgpu.PdschModulatorPlan(ctx, srsgpu.make_pdsch_mod_configs([mod], [0], [0], 52), 52, 4)
    dmrs_plan = srsgpu.PdschDmrsPlan(ctx, srsgpu.make_pdsch_dmrs_configs([dmrs], [0]), 52, 4)
    payloads, offsets = srsgpu.pdcch_pack_payloads(dcis)
    pdcch_plan = srsgpu.PdcchPlan(ctx, dcis, 52, 4, 1, offsets)
    d_payloads = torch.from_numpy(payloads).to(dev)

    def pdsch(g):
        mod_plan.execute(d_cw, g)
        dmrs_plan.execute(g)

    def pdcch(g):
        pdcch_plan.execute(d_payloads, g)

    def grid(*stages):
        g = torch.from_numpy(np.full(4 * 14 * 12 * 52, SENTINEL, np.uint32).view(np.int32)).to(dev)
        for stage in stages:
            stage(g)
        torch.cuda.synchronize(dev)
        return g.cpu().numpy().view(np.uint32)

    only_pdsch, only_pdcch = grid(pdsch), grid(pdcch)
    assert (only_pdsch != SENTINEL).any() and (only_pdcch != SENTINEL).sum() == 2 * 72 * (4 + 8)
    assert not ((only_pdsch != SENTINEL) & (only_pdcch != SENTINEL)).any()
    both = np.where(only_pdcch != SENTINEL, only_pdcch, only_pdsch)
    assert np.array_equal(grid(pdcch, pdsch), both)
    assert np.array_equal(grid(pdsch, pdcch), both)
    for plan in (mod_plan, dmrs_plan, pdcch_plan):
        plan.close()


def test_pdcch_loopback(ctx, random_plan):
    """The restatement's inverse recovers every payload of the random plan from the GPU's grids over an identity
    channel: the REs by PRB mask, DM-RS stripped (and checked against its sequence), hard decision, descrambling,
    rate matching undone, G_N inverted, the CRC checked with the RNTI. Port 0 carries a real positive weight."""
    cases, _ = random_plan
    cases = [(dict(c, weights=np.concatenate([[np.complex64(0.75)], c["weights"][1:]])), p) for c, p in cases]
    got = run(ctx, [to_dci(c, p) for c, p in cases], 52, 4, 4)
    for cfg, payload in cases:
        back, crc_ok, dmrs_ok = C.receive(cfg, payload.size, got[cfg["grid_index"]])
        assert crc_ok and dmrs_ok and np.array_equal(back, payload), cfg
    cfg, payload = cases[0]
    assert not C.receive(dict(cfg, rnti=cfg["rnti"] ^ 0x8000), payload.size, got[cfg["grid_index"]])[1]


def test_pdcch_rejections(ctx):
    """Every refusal raises with its message, names the DCI, and launches nothing (no plan exists to execute)."""
    import torch
    import srsgpu
    rng = np.random.default_rng(46)
    base, payload = C.fill_dci(rng, dict(C.TEMPLATES[0], aggregation_level=2, cce_index=0), 40)
    base.update(nof_ports=1, weights=np.ones(1, np.complex64), data_scaling=C.F(1), dmrs_amplitude=C.F(1))
    inter = dict(base, **{k: C.TEMPLATES[3][k] for k in ("mapping", "frequency_resources", "reg_bundle_size",
                                                         "interleaver_size", "shift_index")})
    c0 = dict(base, **{k: C.TEMPLATES[12][k] for k in ("mapping", "bwp_start_rb", "bwp_size_rb", "frequency_resources",
                                                       "shift_index")})
    good = to_dci(dict(base, start_symbol=5), payload)
    bits = lambda n: np.zeros(n, np.uint8)  # noqa: E731
    for cfg, p, text in ((dict(base, duration=0), payload, "CORESET duration"), (dict(base, duration=4), payload, "CORESET duration"),
                         (dict(base, start_symbol=14), payload, "exceeds the slot duration"),
                         (dict(inter, reg_bundle_size=3), payload, "Invalid REG bundle size"),
                         (dict(inter, duration=3, reg_bundle_size=2), payload, "Invalid REG bundle size"),
                         (dict(inter, interleaver_size=4), payload, "Invalid interleaver size"),
                         (dict(base, aggregation_level=3), payload, "Invalid aggregation level"),
                         (dict(base, cce_index=7), payload, "exceeds CORESET capacity"),
                         (base, bits(0), "Empty payload"), (base, bits(11), "outside 36..164"),
                         (base, bits(141), "outside 36..164"),
                         (dict(base, aggregation_level=1), bits(84), "does not fit the encoded bits"),
                         (dict(inter, frequency_resources=0b111), payload, "Invalid CORESET configuration"),
                         (dict(c0, bwp_size_rb=26), payload, "Invalid CORESET configuration"),
                         (dict(c0, bwp_size_rb=12, aggregation_level=4), payload, "REGs of CORESET0"),
                         (dict(base, bwp_start_rb=45), payload, "outside the BWP"),
                         (dict(base, nof_ports=5, weights=np.ones(5, np.complex64)), payload, "number of ports"),
                         (dict(base, mapping=3), payload, "cce_to_reg_mapping"),
                         (dict(base, grid_index=1), payload, "grid_index"),
                         (dict(base, start_symbol=5, cce_index=1), payload, "both write")):
        with pytest.raises(srsgpu.SrsGpuError, match=text) as err:
            srsgpu.PdcchPlan(ctx, [good, to_dci(cfg, p)], 52, 4, 1)
        assert "DCI" in str(err.value), str(err.value)
    with pytest.raises(srsgpu.SrsGpuError, match="number of ports"):
        srsgpu.PdcchPlan(ctx, [to_dci(dict(base, nof_ports=2, weights=np.ones(2, np.complex64)), payload)], 52, 1, 1)
    with pytest.raises(srsgpu.SrsGpuError, match="outside the BWP"):  # PRBs 0..11 fit 12 PRBs, not 11
        srsgpu.PdcchPlan(ctx, [to_dci(base, payload)], 11, 4, 1)
    srsgpu.PdcchPlan(ctx, [to_dci(base, payload)], 12, 4, 1).close()
    srsgpu.PdcchPlan(ctx, [], 52, 4, 1).close()
    # A payload buffer shorter than the plan reads is refused at execute, before any launch.
    plan = srsgpu.PdcchPlan(ctx, [good], 52, 4, 1)
    dev = torch.device("cuda", 0)
    d_grids = torch.full((4 * 14 * 12 * 52,), 5, dtype=torch.int32, device=dev)
    with pytest.raises(srsgpu.SrsGpuError, match="payload buffer"):
        plan.execute(torch.zeros(plan.payload_bytes - 1, dtype=torch.uint8, device=dev), d_grids)
    torch.cuda.synchronize(dev)
    assert bool((d_grids == 5).all())
    plan.close()
