"""GPU parity of the SS/PBCH block plan (PBCH encoding, both scramblings, QPSK, RE mapping, PBCH DM-RS, PSS and SSS of
every block in one launch; srsgpu_ssb_plan through the C ABI) against the reference's own grid words
(tests/golden/ssb.npz, made by ssb_processor_impl built from its sources) and against the numpy restatement
tests/ssb_cases.py, which tests/test_ssb_oracle.py pins to the same fixture. Every comparison is exact and of the whole
buffer: identical bf16 grid words where a block writes, the prefill everywhere else, guard words on both sides of the
grids included."""
import numpy as np
import pytest

import ssb_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(C.SENTINEL)
GUARD = 4096  # words on either side of the grids


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


def to_block(cfg, grid_index=None):
    import srsgpu
    return srsgpu.Ssb(phys_cell_id=cfg["phys_cell_id"], ssb_idx=cfg["ssb_idx"], L_max=cfg["L_max"],
                      pattern_case=cfg["pattern_case"], common_scs=cfg["common_scs"], offset_to_pointA=cfg["offset_to_pointA"],
                      subcarrier_offset=cfg["subcarrier_offset"], slot_index=cfg["slot_index"], hrf=cfg["hrf"],
                      payload=cfg["payload"], sfn=cfg["sfn"], ports=cfg["ports"], pss_amplitude=float(cfg["pss_amplitude"]),
                      grid_index=cfg.get("grid_index", 0) if grid_index is None else grid_index)


def guarded(nof_words):
    """A sentinel-filled device buffer with guard words on both sides, and the view of the grids inside it."""
    import torch
    buf = torch.from_numpy(np.full(nof_words + 2 * GUARD, SENTINEL, np.uint32).view(np.int32)).to(torch.device("cuda", 0))
    return buf, buf[GUARD: GUARD + nof_words]


def scattered_payloads(rng, cases):
    """The blocks' four bytes at unaligned offsets between random guard bytes: (buffer, offsets)."""
    chunks, offsets, pos = [], [], 0
    for cfg in cases:
        pad = rng.integers(0, 256, int(rng.integers(1, 4))).astype(np.uint8)
        # The high half of the SFN byte is not the plan's to read: fill it.
        four = C.pack_payload(cfg)
        four[3] |= int(rng.integers(0, 16)) << 4
        chunks += [pad, four]
        offsets.append(pos + pad.size)
        pos += pad.size + 4
    return np.concatenate(chunks + [rng.integers(0, 256, 3).astype(np.uint8)]), offsets


def run(ctx, cases, grid_nof_prb, grid_nof_ports, nof_grids, grid_indices=None, seed=0):
    """The grids (nof_grids, ports, 14, nsc) uint32 after one execute over sentinel-filled grids; the guards are checked."""
    import torch
    import srsgpu
    blocks = [to_block(c, None if grid_indices is None else grid_indices[i]) for i, c in enumerate(cases)]
    payloads, offsets = scattered_payloads(np.random.default_rng(seed), cases)
    plan = srsgpu.SsbPlan(ctx, blocks, grid_nof_prb, grid_nof_ports, nof_grids, offsets)
    n = nof_grids * grid_nof_ports * 14 * 12 * grid_nof_prb
    buf, grids = guarded(n)
    plan.execute(torch.from_numpy(payloads).to(grids.device), grids)
    torch.cuda.synchronize()
    plan.close()
    host = buf.cpu().numpy().view(np.uint32)
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all()
    return host[GUARD: GUARD + n].reshape(nof_grids, grid_nof_ports, 14, 12 * grid_nof_prb)


def expected(rows, grid_nof_prb, grid_nof_ports):
    want = np.full((grid_nof_ports, 14, 12 * grid_nof_prb), SENTINEL, np.uint32)
    C.apply_rows(want, rows)
    return want


def test_ssb_golden_each_alone(ctx):
    """Every fixture block in a plan of its own, in a grid of the case's PRBs and ports."""
    count = 0
    for cfg, _l, _k, _enc, rows in C.golden_cases():
        got = run(ctx, [cfg], cfg["grid_nof_prb"], cfg["grid_nof_ports"], 1, seed=count)
        assert np.array_equal(got[0], expected(rows, cfg["grid_nof_prb"], cfg["grid_nof_ports"])), cfg
        count += 1
    assert count > 60


def test_ssb_golden_one_plan(ctx):
    """All fixture blocks in ONE plan and one launch, each in a grid of its own of 273 PRB x 4 ports."""
    cases = list(C.golden_cases())
    got = run(ctx, [c[0] for c in cases], 273, 4, len(cases), grid_indices=list(range(len(cases))))
    for i, (cfg, _l, _k, _enc, rows) in enumerate(cases):
        assert np.array_equal(got[i], expected(rows, 273, 4)), (i, cfg)


@pytest.mark.parametrize("seed", (61, 62, 63))
def test_ssb_random_plan(ctx, seed):
    """Blocks of random pattern cases in three slot grids of 52 PRB x 4 ports, two per grid where the pattern puts two in
    a slot, against the restatement."""
    cases = C.random_plan_cases(np.random.default_rng(seed))
    assert {c["grid_index"] for c in cases} == {0, 1, 2} and len(cases) > 3
    want = np.full((3, 4, 14, 12 * 52), SENTINEL, np.uint32)
    for cfg in cases:
        C.apply_rows(want[cfg["grid_index"]], C.process(cfg)[3])
    got = run(ctx, cases, 52, 4, 3, seed=seed)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def smallest_shapes():
    rng = np.random.default_rng(64)
    one = C.make_case(rng, C.CASE_A, 4, 0, ports=(0,), offset_to_pointA=0, subcarrier_offset=0, grid_nof_prb=20,
                      grid_nof_ports=1)
    late = C.make_case(rng, C.CASE_B, 8, 1, ports=(1,), beta_pss_dB=3.0)             # symbols 8..11
    late_e = C.make_case(rng, C.CASE_E, 64, 61, ports=(0, 1))                        # case E's 36 + 56 n: symbols 8..11
    four = C.make_case(rng, C.CASE_C, 8, 5, ports=(3, 0, 2, 1), beta_pss_dB=3.0)
    sparse = C.make_case(rng, C.CASE_D, 64, 42, ports=(3, 1))
    return [pytest.param([one], 20, 1, id="one block on one port fills a 20-PRB grid's width"),
            pytest.param([late], 52, 4, id="the latest start symbol, case B"),
            pytest.param([late_e], 52, 4, id="the latest start symbol, case E"),
            pytest.param([four], 52, 4, id="four ports out of order"),
            pytest.param([sparse], 52, 4, id="a non-contiguous port list"),
            pytest.param([C.make_case(rng, C.CASE_A, 8, 2, phys_cell_id=501, hrf=1, ports=(0, 2)),
                          C.make_case(rng, C.CASE_A, 8, 3, phys_cell_id=501, hrf=1, ports=(0, 2))], 52, 4,
                         id="two blocks in one slot grid")]


@pytest.mark.parametrize("cases,grid_nof_prb,grid_nof_ports", smallest_shapes())
def test_ssb_smallest_shapes(ctx, cases, grid_nof_prb, grid_nof_ports):
    want = np.full((grid_nof_ports, 14, 12 * grid_nof_prb), SENTINEL, np.uint32)
    for cfg in cases:
        assert C.refusal(cfg, grid_nof_prb, grid_nof_ports) is None
        C.apply_rows(want, C.process(cfg)[3])
    got = run(ctx, cases, grid_nof_prb, grid_nof_ports, 1, seed=3)
    assert np.array_equal(got[0], want)


def test_ssb_shapes_reach_the_edges():
    """The parametrised shapes hold what they are named for."""
    shapes = {p.id: p.values for p in smallest_shapes()}
    one = shapes["one block on one port fills a 20-PRB grid's width"][0][0]
    rows = C.process(one)[3]
    assert C.k_first(one) == 0 and rows[:, 2].min() == 0 and rows[:, 2].max() == 239
    latest = max(C.l_first(p, i) % 14 for p in range(5) for i in C.usable_indices(p, C.L_MAX_OF[p][-1]))
    for name in ("the latest start symbol, case B", "the latest start symbol, case E"):
        cfg = shapes[name][0][0]
        assert C.l_first(cfg["pattern_case"], cfg["ssb_idx"]) % 14 == latest == 8
    two = shapes["two blocks in one slot grid"][0]
    assert two[0]["slot_index"] == two[1]["slot_index"] and two[0]["ssb_idx"] != two[1]["ssb_idx"]


def test_ssb_graph_replay_with_fresh_payloads(ctx):
    """One capture, replays with new payload and SFN bytes in the same device buffer: each replay equals the eager run
    and the restatement."""
    import torch
    import srsgpu
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(65)
    cases = C.random_plan_cases(rng, nof_grids=2)
    plan = srsgpu.SsbPlan(ctx, [to_block(c) for c in cases], 52, 4, 2)
    d_payloads = torch.zeros(plan.payload_bytes, dtype=torch.uint8, device=dev)
    d_grids = torch.zeros(2 * 4 * 14 * 12 * 52, dtype=torch.int32, device=dev)

    def result():
        torch.cuda.synchronize(dev)
        got = d_grids.cpu().numpy().view(np.uint32).copy()
        d_grids.fill_(-7)
        return got

    sets, vs = [], set()
    for r in range(4):
        fresh = [dict(c, payload=rng.integers(0, 2, 24).astype(np.uint8), sfn=(5 * r + i) % 1024) for i, c in enumerate(cases)]
        vs |= {(c["sfn"] >> 1) & 3 for c in fresh}
        want = np.full((2, 4, 14, 12 * 52), np.uint32(0xFFFFFFF9), np.uint32)
        for cfg in fresh:
            C.apply_rows(want[cfg["grid_index"]], C.process(cfg)[3])
        sets.append((torch.from_numpy(np.concatenate([C.pack_payload(c) for c in fresh])).to(dev), want.ravel()))
    assert vs == {0, 1, 2, 3}  # every offset of the first scrambling
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


def test_ssb_and_csi_rs_compose_with_pdsch(ctx):
    """One grid: a PDSCH over the whole slot whose reserved patterns cover an SS/PBCH block and three CSI-RS, then the SSB
    plan and the CSI-RS plan. Every launch order gives the union; inside the allocation no sentinel is left except the
    REs the reference leaves (the block's symbol 0 outside the PSS, the gaps beside the SSS, the ports a signal does not
    have); no word differs from the separate results."""
    import torch
    import srsgpu
    from srsgpu import alloc
    import csi_rs_cases as R
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(66)
    block = C.make_case(rng, C.CASE_C, 8, 1, ports=(0, 1, 2, 3), offset_to_pointA=48, subcarrier_offset=0)  # symbols 8..11
    assert C.k_first(block) == 288 and C.l_first(block["pattern_case"], block["ssb_idx"]) % 14 == 8
    signals = [R.make_case(rng, 1, R.THREE, 0, 52, k_ref=1, l0=4), R.make_case(rng, 1, R.THREE, 0, 24, k_ref=2, l0=9),
               R.make_case(rng, 4, R.ONE, 0, 52, k_ref=4, l0=13, weights=R.random_weights(rng, 4))]
    reserved = [alloc.ReservedPattern.from_range(*r, grid_nof_prb=52)
                for r in C.reserved_patterns(block) + [p for s in signals for p in R.reserved_patterns(s)]]
    w = (rng.normal(size=(4, 2)) + 1j * rng.normal(size=(4, 2))).astype(np.complex64) / 2
    mod = srsgpu.PdschModulation(rnti=0x4601, n_id=77, modulation_order=4, nof_layers=2, nof_ports=4, bwp_start_rb=0,
                                 bwp_size_rb=52, rb_start=0, nof_rb=52, start_symbol=0, nof_symbols=14,
                                 dmrs_symbol_mask=1 << 2, dmrs_type=1, nof_cdm_groups_without_data=2, scaling=1.0, weights=w,
                                 reserved=reserved)
    dmrs = srsgpu.PdschDmrs(slot_index=3, scrambling_id=77, n_scid=0, dmrs_type=1, nof_layers=2, nof_ports=4,
                            dmrs_symbol_mask=1 << 2, reference_point_k_rb=0, rb_start=0, nof_rb=52, amplitude=1.0, weights=w)
    nbits = mod.nof_re(52) * 2 * 4
    d_cw = torch.from_numpy(rng.integers(0, 256, (nbits + 7) // 8 + 4).astype(np.uint8)).to(dev)
    exts, keep = srsgpu.make_alloc_exts([mod], 52)
    mod_plan = srsgpu.PdschModulatorPlan(ctx, srsgpu.make_pdsch_mod_configs([mod], [0], [0], 52), 52, 4, exts)
    dmrs_plan = srsgpu.PdschDmrsPlan(ctx, srsgpu.make_pdsch_dmrs_configs([dmrs], [0]), 52, 4)
    ssb_plan = srsgpu.SsbPlan(ctx, [to_block(block)], 52, 4, 1)
    import test_csi_rs_gpu as T
    csi_plan = srsgpu.CsiRsPlan(ctx, [T.to_signal(s) for s in signals], 52, 4, 1)
    d_payloads = torch.from_numpy(C.pack_payload(block)).to(dev)
    del keep

    def pdsch(g):
        mod_plan.execute(d_cw, g)
        dmrs_plan.execute(g)

    def ssb(g):
        ssb_plan.execute(d_payloads, g)

    def grid(*stages):
        buf, g = guarded(4 * 14 * 12 * 52)
        for stage in stages:
            stage(g)
        torch.cuda.synchronize(dev)
        host = buf.cpu().numpy().view(np.uint32)
        assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all()
        return host[GUARD:-GUARD].copy()

    only_pdsch, only_ssb, only_csi = grid(pdsch), grid(ssb), grid(csi_plan.execute)
    want_ssb, want_csi = np.full((4, 14, 12 * 52), SENTINEL, np.uint32), np.full((4, 14, 12 * 52), SENTINEL, np.uint32)
    C.apply_rows(want_ssb, C.process(block)[3])
    for s in signals:
        R.apply_rows(want_csi, R.process(s))
    assert np.array_equal(only_ssb, want_ssb.ravel()) and np.array_equal(only_csi, want_csi.ravel())
    written = [only_pdsch != SENTINEL, only_ssb != SENTINEL, only_csi != SENTINEL]
    assert all(m.any() for m in written) and not (written[0] & written[1]).any() and not (written[0] & written[2]).any()
    assert not (written[1] & written[2]).any()
    both = np.where(written[1], only_ssb, np.where(written[2], only_csi, only_pdsch))
    for order in ((pdsch, ssb, csi_plan.execute), (csi_plan.execute, ssb, pdsch), (ssb, pdsch, csi_plan.execute)):
        assert np.array_equal(grid(*order), both)
    # What stays unwritten: the DM-RS REs of the CDM group without data or pilots (odd subcarriers of symbol 2), the
    # block's box outside the REs the reference writes, and the REs of the one-port signals on ports 1-3.
    holes = np.zeros((4, 14, 12 * 52), bool)
    holes[:, 2, 1::2] = True
    holes[:, 8, 288:288 + 56] = holes[:, 8, 288 + 183:288 + 240] = True
    holes[:, 10, 288 + 48:288 + 56] = holes[:, 10, 288 + 183:288 + 192] = True
    for s in signals[:2]:
        rows = R.process(s)
        # The second TRS-like signal crosses the block's symbol 9 on RBs 0..23, left of the block: no RE in common.
        holes[1:, rows[:, 1], rows[:, 2]] = True
    assert np.array_equal(both.reshape(4, 14, -1) == SENTINEL, holes)
    for plan in (mod_plan, dmrs_plan, ssb_plan, csi_plan):
        plan.close()


def test_ssb_rejections(ctx):
    """Every refusal raises with its reason, names the block, and leaves the live device buffers where they were; create
    and destroy return the count to its baseline."""
    import torch
    import srsgpu
    rng = np.random.default_rng(67)
    a = C.make_case(rng, C.CASE_A, 8, 2, offset_to_pointA=10, subcarrier_offset=0, hrf=0)
    e = C.make_case(rng, C.CASE_E, 64, 10, offset_to_pointA=2, subcarrier_offset=0, common_scs=4)
    b = C.make_case(rng, C.CASE_B, 8, 0, offset_to_pointA=2, subcarrier_offset=0)
    good = C.make_case(rng, C.CASE_A, 8, 3, offset_to_pointA=0, subcarrier_offset=0, ports=(0, 1))  # slot 1, symbols 8..11
    srsgpu.SsbPlan(ctx, [to_block(good)], 52, 4, 1).close()
    live = srsgpu.live_device_buffers()
    for cfg, text in ((dict(a, pattern_case=5), "Invalid SSB pattern case"), (dict(a, L_max=5), "is not 4, 8 or 64"),
                      (dict(a, L_max=0), "is not 4, 8 or 64"), (dict(a, ssb_idx=8), "is not below L_max"),
                      (dict(e, ssb_idx=64), "is not below L_max"), (dict(a, phys_cell_id=1008), "exceeds 1007"),
                      (dict(a, common_scs=3), "FR1 and Common SCS"), (dict(e, common_scs=1), "FR2 and Common SCS"),
                      (dict(a, offset_to_pointA=2200), "Invalid offset to Point A"),
                      (dict(a, subcarrier_offset=24), "Invalid subcarrier offset 24 for FR1"),
                      (dict(e, subcarrier_offset=12), "Invalid subcarrier offset 12 for FR2"),
                      (dict(b, subcarrier_offset=3), "Unsupported combination of SSB SCS 30kHz"),
                      (dict(a, slot_index=0), "Invalid slot index \\(0\\) for SSB index 2"), (dict(a, hrf=2), "hrf"),
                      (dict(e, ssb_idx=9, slot_index=4), "symbols \\(4 from 12\\) exceed the slot"),
                      (dict(a, offset_to_pointA=32, subcarrier_offset=1), "subcarriers \\(240 from 385\\) exceed the grid"),
                      (dict(a, ports=[]), "outside 1..4"), (dict(a, ports=[0, 1, 2, 3, 0]), "outside 1..4"),
                      (dict(a, ports=[0, 4]), "Port 4 is outside the grid"), (dict(a, ports=[2, 0, 2]), "Port 2 is listed twice"),
                      (dict(a, pss_amplitude=np.float32(np.nan)), "pss_amplitude is not finite"),
                      (dict(a, grid_index=1), "grid_index"),
                      (dict(good, phys_cell_id=5, ports=[1]), "both write"),
                      (dict(good, offset_to_pointA=19, ports=[1, 3]), "both write")):
        with pytest.raises(srsgpu.SrsGpuError, match=text) as err:
            srsgpu.SsbPlan(ctx, [to_block(good), to_block(cfg)], 52, 4, 1)
        assert "block" in str(err.value), str(err.value)
        assert srsgpu.live_device_buffers() == live, text
    with pytest.raises(srsgpu.SrsGpuError, match="Port 1 is outside the grid"):
        srsgpu.SsbPlan(ctx, [to_block(good)], 52, 1, 1)
    with pytest.raises(srsgpu.SrsGpuError, match="exceed the grid"):  # subcarriers 0..239 fit 20 PRBs, not 19
        srsgpu.SsbPlan(ctx, [to_block(good)], 19, 4, 1)
    with pytest.raises(srsgpu.SrsGpuError, match="2\\^32"):
        srsgpu.SsbPlan(ctx, [to_block(good)], 273, 4, 24000)
    assert srsgpu.live_device_buffers() == live
    # No overlap: the same REs on other ports, the other block of the slot, the neighbouring 20 PRBs.
    srsgpu.SsbPlan(ctx, [to_block(good), to_block(dict(good, ports=[2, 3])), to_block(dict(a, slot_index=1)),
                         to_block(dict(good, offset_to_pointA=20, ports=[0]))], 52, 4, 1).close()
    srsgpu.SsbPlan(ctx, [to_block(good)], 20, 4, 1).close()
    srsgpu.SsbPlan(ctx, [], 52, 4, 1).close()
    assert srsgpu.live_device_buffers() == live
    # A payload buffer shorter than the plan reads is refused at execute, before any launch.
    plan = srsgpu.SsbPlan(ctx, [to_block(good)], 52, 4, 1)
    assert srsgpu.live_device_buffers() == live + 2
    dev = torch.device("cuda", 0)
    d_grids = torch.full((4 * 14 * 12 * 52,), 5, dtype=torch.int32, device=dev)
    with pytest.raises(srsgpu.SrsGpuError, match="payload buffer"):
        plan.execute(torch.zeros(plan.payload_bytes - 1, dtype=torch.uint8, device=dev), d_grids)
    torch.cuda.synchronize(dev)
    assert bool((d_grids == 5).all())
    plan.close()
    assert srsgpu.live_device_buffers() == live
