"""GPU parity of the NZP-CSI-RS plan (sequence, w_f cover, precoding and RE mapping of every signal in one launch;
srsgpu_csi_rs_plan through the C ABI) against the reference's own grid words (tests/golden/csi_rs.npz, made by
nzp_csi_rs_generator_impl built from its sources) and against the numpy restatement tests/csi_rs_cases.py, which
tests/test_csi_rs_oracle.py pins to the same fixture. Every comparison is exact and of the whole buffer: identical bf16
grid words where a signal writes, the prefill everywhere else, guard words on both sides of the grids included."""
import numpy as np
import pytest

import csi_rs_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(C.SENTINEL)
GUARD = 4096  # words on either side of the grids


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


def to_signal(cfg, grid_index=None):
    import srsgpu
    return srsgpu.CsiRs(slot_index=cfg["n_slot"], start_rb=cfg["start_rb"], nof_rb=cfg["nof_rb"], row=cfg["row"],
                        k_ref=cfg.get("k_refs", [cfg["k_ref"]]), symbol_l0=cfg["symbol_l0"], cdm=cfg["cdm"],
                        freq_density=cfg["freq_density"], scrambling_id=cfg["scrambling_id"], amplitude=float(cfg["amplitude"]),
                        weights=cfg["weights"], symbol_l1=cfg["symbol_l1"], cp=cfg["cp"],
                        grid_index=cfg.get("grid_index", 0) if grid_index is None else grid_index)


def guarded(nof_words):
    """A sentinel-filled device buffer with guard words on both sides, and the view of the grids inside it."""
    import torch
    buf = torch.from_numpy(np.full(nof_words + 2 * GUARD, SENTINEL, np.uint32).view(np.int32)).to(torch.device("cuda", 0))
    return buf, buf[GUARD: GUARD + nof_words]


def run(ctx, signals, grid_nof_prb, grid_nof_ports, nof_grids):
    """The grids (nof_grids, ports, 14, nsc) uint32 after one execute over sentinel-filled grids; the guards are checked."""
    import torch
    import srsgpu
    plan = srsgpu.CsiRsPlan(ctx, signals, grid_nof_prb, grid_nof_ports, nof_grids)
    n = nof_grids * grid_nof_ports * 14 * 12 * grid_nof_prb
    buf, grids = guarded(n)
    plan.execute(grids)
    torch.cuda.synchronize()
    plan.close()
    host = buf.cpu().numpy().view(np.uint32)
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all()
    return host[GUARD: GUARD + n].reshape(nof_grids, grid_nof_ports, 14, 12 * grid_nof_prb)


def expected(rows, grid_nof_prb, grid_nof_ports):
    want = np.full((grid_nof_ports, 14, 12 * grid_nof_prb), SENTINEL, np.uint32)
    C.apply_rows(want, rows)
    return want


def test_csi_rs_golden_each_alone(ctx):
    """Every fixture signal in a plan of its own, in a grid of the case's PRBs and ports."""
    count = 0
    for cfg, rows in C.golden_cases():
        got = run(ctx, [to_signal(cfg)], cfg["grid_nof_prb"], cfg["grid_nof_ports"], 1)
        assert np.array_equal(got[0], expected(rows, cfg["grid_nof_prb"], cfg["grid_nof_ports"])), cfg
        count += 1
    assert count > 80


def test_csi_rs_golden_one_plan(ctx):
    """All fixture signals in ONE plan and one launch, each in a grid of its own of 273 PRB x 4 ports."""
    cases = list(C.golden_cases())
    got = run(ctx, [to_signal(c, i) for i, (c, _) in enumerate(cases)], 273, 4, len(cases))
    for i, (cfg, rows) in enumerate(cases):
        assert np.array_equal(got[i], expected(rows, 273, 4)), (i, cfg)


@pytest.mark.parametrize("seed", (51, 52))
def test_csi_rs_random_plan(ctx, seed):
    """Eight signals of all rows in each of three grids of 52 PRB x 4 ports, against the restatement."""
    cases = C.random_plan_cases(np.random.default_rng(seed))
    assert {c["row"] for c in cases} == {1, 2, 3, 4, 5} and {c["grid_index"] for c in cases} == {0, 1, 2}
    want = np.full((3, 4, 14, 12 * 52), SENTINEL, np.uint32)
    for cfg in cases:
        C.apply_rows(want[cfg["grid_index"]], C.process(cfg))
    got = run(ctx, [to_signal(c) for c in cases], 52, 4, 3)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def smallest_shapes():
    rng = np.random.default_rng(53)
    w2, w4 = C.random_weights(rng, 2), C.random_weights(rng, 4)
    shapes = (("row 1, one RB", C.make_case(rng, 1, C.THREE, 51, 1, k_ref=3), 3),
              ("row 2, one RB", C.make_case(rng, 2, C.ONE, 0, 1, k_ref=11), 1),
              ("row 2, 0.5 even over one odd RB", C.make_case(rng, 2, C.DOT5_EVEN, 7, 1), 0),
              ("row 3, 0.5 odd over one even RB", C.make_case(rng, 3, C.DOT5_ODD, 8, 1, weights=w2), 0),
              ("row 3, 0.5 odd, ends on the grid's last RB", C.make_case(rng, 3, C.DOT5_ODD, 44, 8, k_ref=10, weights=w2), 8),
              ("row 1, ends on the grid's last RB", C.make_case(rng, 1, C.THREE, 9, 43, l0=13), 129),
              ("row 5, l0 = 12", C.make_case(rng, 5, C.ONE, 0, 52, k_ref=10, l0=12, weights=w4), 104),
              ("row 4, k_ref = 8", C.make_case(rng, 4, C.ONE, 3, 49, k_ref=8, weights=w4), 98),
              ("row 1, 273 RB: four runs of 256 elements", C.make_case(rng, 1, C.THREE, 0, 273, grid_nof_prb=273), 819),
              ("row 4, 129 RB: two elements past one run", C.make_case(rng, 4, C.ONE, 144, 129, grid_nof_prb=273), 258))
    return [pytest.param(cfg, n, id=name) for name, cfg, n in shapes]


@pytest.mark.parametrize("cfg,nof_elements", smallest_shapes())
def test_csi_rs_smallest_shapes(ctx, cfg, nof_elements):
    prb = cfg["grid_nof_prb"]
    assert C.refusal(cfg, prb, 4) is None and C.seq_len(cfg) == nof_elements
    rows = C.process(cfg)
    assert rows.shape[0] == nof_elements * len(C.groups(cfg)) * C.ROW_PORTS[cfg["row"]]
    if nof_elements and cfg["start_rb"] + cfg["nof_rb"] == prb:
        assert rows[:, 2].max() // 12 == prb - 1
    got = run(ctx, [to_signal(cfg)], prb, 4, 1)
    assert np.array_equal(got[0], expected(rows, prb, 4))


def test_csi_rs_graph_replay(ctx):
    """One capture; every replay over a cleared buffer equals the eager run and the restatement."""
    import torch
    import srsgpu
    cases = C.random_plan_cases(np.random.default_rng(54), nof_grids=2)
    want = np.full((2, 4, 14, 12 * 52), np.uint32(0xFFFFFFF9), np.uint32)
    for cfg in cases:
        C.apply_rows(want[cfg["grid_index"]], C.process(cfg))
    plan = srsgpu.CsiRsPlan(ctx, [to_signal(c) for c in cases], 52, 4, 2)
    d_grids = torch.full((want.size,), -7, dtype=torch.int32, device=torch.device("cuda", 0))

    def result():
        torch.cuda.synchronize()
        got = d_grids.cpu().numpy().view(np.uint32).copy()
        d_grids.fill_(-7)
        return got

    plan.execute(d_grids)
    eager = result()
    assert np.array_equal(eager, want.ravel())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.execute(d_grids)
    result()  # the capture does not execute; clear again
    for _ in range(3):
        graph.replay()
        assert np.array_equal(result(), eager)
    plan.close()


def test_csi_rs_composes_with_pdsch(ctx):
    """One grid: a PDSCH over the whole slot whose reserved patterns cover a TRS-like row-1 pair and a row-4 CSI-RS,
    then the CSI-RS plan. Either launch order gives the union; no sentinel is left inside the allocation; no word
    differs from the separate results."""
    import torch
    import srsgpu
    from srsgpu import alloc
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(55)
    cases = [C.make_case(rng, 1, C.THREE, 0, 52, k_ref=1, l0=4), C.make_case(rng, 1, C.THREE, 0, 52, k_ref=1, l0=8),
             C.make_case(rng, 4, C.ONE, 0, 52, k_ref=4, l0=13, weights=C.random_weights(rng, 4)),
             C.make_case(rng, 3, C.DOT5_ODD, 5, 40, k_ref=6, l0=6, weights=C.random_weights(rng, 2))]
    reserved = [alloc.ReservedPattern.from_range(*r, grid_nof_prb=52) for c in cases for r in C.reserved_patterns(c)]
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
    csi_plan = srsgpu.CsiRsPlan(ctx, [to_signal(c) for c in cases], 52, 4, 1)
    del keep

    def pdsch(g):
        mod_plan.execute(d_cw, g)
        dmrs_plan.execute(g)

    def grid(*stages):
        buf, g = guarded(4 * 14 * 12 * 52)
        for stage in stages:
            stage(g)
        torch.cuda.synchronize(dev)
        host = buf.cpu().numpy().view(np.uint32)
        assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all()
        return host[GUARD:-GUARD].copy()

    only_pdsch, only_csi = grid(pdsch), grid(csi_plan.execute)
    want_csi = np.full((4, 14, 12 * 52), SENTINEL, np.uint32)
    for c in cases:
        C.apply_rows(want_csi, C.process(c))
    assert np.array_equal(only_csi, want_csi.ravel())
    assert (only_pdsch != SENTINEL).any() and not ((only_pdsch != SENTINEL) & (only_csi != SENTINEL)).any()
    both = np.where(only_csi != SENTINEL, only_csi, only_pdsch)
    assert np.array_equal(grid(csi_plan.execute, pdsch), both)
    assert np.array_equal(grid(pdsch, csi_plan.execute), both)
    # The PDSCH left exactly the reserved REs and the DM-RS REs of the CDM group without data or pilots (odd subcarriers
    # of symbol 2). The CSI-RS fills the reserved REs on the ports each signal has: rows 1 and 3 write port 0 and ports
    # 0-1, so their REs keep the sentinel on the other ports, as on the reference's grid. Nothing else is left unwritten.
    unused_dmrs = np.zeros((14, 12 * 52), bool)
    unused_dmrs[2, 1::2] = True
    csi_res, holes = np.zeros((14, 12 * 52), bool), np.zeros((4, 14, 12 * 52), bool)
    holes[:] = unused_dmrs
    for c in cases:
        rows = C.process(c)
        rows = rows[rows[:, 0] == 0]
        csi_res[rows[:, 1], rows[:, 2]] = True
        for p in range(C.ROW_PORTS[c["row"]], 4):
            holes[p, rows[:, 1], rows[:, 2]] = True
    assert np.array_equal(only_pdsch.reshape(4, 14, -1) == SENTINEL, np.broadcast_to(csi_res | unused_dmrs, (4, 14, 12 * 52)))
    assert np.array_equal(both.reshape(4, 14, -1) == SENTINEL, holes)
    for plan in (mod_plan, dmrs_plan, csi_plan):
        plan.close()


def test_csi_rs_rejections(ctx):
    """Every refusal raises with its reason, names the signal, and leaves the live device buffers where they were."""
    import srsgpu
    rng = np.random.default_rng(56)
    base = {row: C.make_case(rng, row, C.ROW_RULES[row][1][0], 4, 20, l0=3 + row) for row in range(1, 6)}
    good = to_signal(C.make_case(rng, 2, C.ONE, 0, 52, k_ref=0, l0=0))
    eye4 = np.eye(4, dtype=np.complex64)
    srsgpu.CsiRsPlan(ctx, [good], 52, 4, 1).close()
    live = srsgpu.live_device_buffers()
    for cfg, text in ((dict(base[1], row=0), "Invalid mapping table row"), (dict(base[1], row=13), "Unsupported mapping table row"),
                      (dict(base[4], row=6), "needs 8 grid ports"), (dict(base[4], row=12), "needs 16 grid ports"),
                      (dict(base[1], k_ref=4), "k_0"), (dict(base[4], k_ref=9), "k_0"), (dict(base[5], k_ref=11), "k_0"),
                      (dict(base[1], k_refs=[1, 2]), "1 k_ref is needed"), (dict(base[1], k_refs=[]), "1 k_ref is needed"),
                      (dict(base[1], freq_density=C.ONE), "Row 1: invalid density"),
                      (dict(base[4], freq_density=C.DOT5_EVEN), "Row 4: invalid density"),
                      (dict(base[2], cdm=C.FD_CDM2), "Row 2: invalid CDM type"), (dict(base[3], cdm=C.NO_CDM), "Row 3: invalid CDM type"),
                      (dict(base[5], cdm=C.CDM4), "Row 5: invalid CDM type"),
                      (dict(base[2], symbol_l0=14), "l_0, i.e., 14 outside the valid range"),
                      (dict(base[2], cp=1, symbol_l0=12), "l_0, i.e., 12 outside the valid range"),
                      (dict(base[5], symbol_l0=13), "Row 5: l_0 \\+ 1"),
                      (dict(base[3], weights=eye4), "does not match the precoding number of ports"),
                      (dict(base[2], start_rb=40, nof_rb=13), "exceed the grid"),
                      (dict(base[2], amplitude=C.F(np.inf)), "amplitude is not finite"),
                      (dict(base[4], amplitude=C.F(np.nan)), "amplitude is not finite"),
                      (dict(base[1], scrambling_id=1024), "scrambling_id"), (dict(base[1], n_slot=160), "slot_index"),
                      (dict(base[1], grid_index=1), "grid_index"),
                      (C.make_case(rng, 3, C.ONE, 51, 1, k_ref=0, l0=0), "both write"),
                      (C.make_case(rng, 1, C.THREE, 10, 1, k_ref=0, l0=0), "both write")):
        with pytest.raises(srsgpu.SrsGpuError, match=text) as err:
            srsgpu.CsiRsPlan(ctx, [good, to_signal(cfg)], 52, 4, 1)
        assert "signal" in str(err.value), str(err.value)
        assert srsgpu.live_device_buffers() == live, text
    with pytest.raises(srsgpu.SrsGpuError, match="exceeds the grid number of ports"):
        srsgpu.CsiRsPlan(ctx, [to_signal(base[4])], 52, 3, 1)
    with pytest.raises(srsgpu.SrsGpuError, match="exceed the grid"):  # RBs 4..23 fit 24 PRBs, not 23
        srsgpu.CsiRsPlan(ctx, [to_signal(base[2])], 23, 4, 1)
    with pytest.raises(srsgpu.SrsGpuError, match="2\\^32"):
        srsgpu.CsiRsPlan(ctx, [good], 273, 4, 24000)
    assert srsgpu.live_device_buffers() == live
    # Neighbours are no overlap: the same symbol on other subcarriers, the same subcarriers on another symbol.
    srsgpu.CsiRsPlan(ctx, [good, to_signal(C.make_case(rng, 2, C.ONE, 0, 52, k_ref=1, l0=0)),
                           to_signal(C.make_case(rng, 2, C.ONE, 0, 52, k_ref=0, l0=1))], 52, 4, 1).close()
    srsgpu.CsiRsPlan(ctx, [to_signal(base[2])], 24, 4, 1).close()
    srsgpu.CsiRsPlan(ctx, [], 52, 4, 1).close()
    # A signal with nothing to write makes a plan that launches nothing.
    empty = srsgpu.CsiRsPlan(ctx, [to_signal(C.make_case(rng, 2, C.DOT5_EVEN, 7, 1))], 52, 4, 1)
    empty.execute(guarded(4 * 14 * 12 * 52)[1])
    empty.close()
    assert srsgpu.live_device_buffers() == live
