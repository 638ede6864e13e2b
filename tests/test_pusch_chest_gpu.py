"""GPU parity of the PUSCH DM-RS channel estimator (srsgpu_pusch_chest_plan through the C ABI) against the reference's
own estimates (tests/golden/pusch_chest.npz, made by dmrs_pusch_estimator_impl) and the float64 restatement
(oracle/pusch_chest_oracle.py), plus the whole PUSCH receive chain (estimator -> demodulator) against the oracle chain.

Tolerances (floating point, stated as the north star asks): estimates on the allocated REs within 1e-2 x the RMS
channel magnitude (bf16 output: 2^-9 relative rounding; the reference's 7-decimal filter table vs taps from the
raised-cosine formula); noise variance, RSRP and EPRE within 1e-3 relative. Multi-layer estimation (extension, which
the reference cannot pin) is held to the float64 restatement C.estimate_layers at these same tolerances, per layer
(1e-2 x the layer's RMS with average and no CFO compensation, CFO_TOL[td] otherwise; metrics 1e-3, TA 2 Tc, CFO and the
compact layout's per-layer CFO word 0.05 Hz): none was raised. Largest measured estimate errors on the MI355X, all in
test_pusch_chest_multilayer_vs_oracle: 1.40e-2 of 1.5e-2 at case 34 (L = 3, type 2, 40 RB, 3 ports, 3 DM-RS symbols,
filter + average + CFO compensation: the estimate rounded to bf16, then rotated in bf16), 1.48e-2 of 2.5e-2 at case 41
(L = 4, type 2, 40 RB, interpolate), 5.2e-3 of 1e-2 at case 12 (L = 2, type 1, 16 RB); the wideband L = 4 case reaches
1.27e-2 of 1.5e-2; metrics within 7e-6. A failure of one of these by a small margin after a compiler change is float32
reordering; anything else is a regression. test_pusch_chest_multilayer keeps its older check
against the true channel: at 30 dB SNR below -15 dB of the channel power."""
import numpy as np
import pytest

import golden_lib as G
import pusch_chest_oracle as C
import pusch_demod_oracle as D
from ofdm_oracle import bf16_to_complex
from pusch_chest_cases import multilayer_case, random_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


def to_est(cfg, fd=2, layers=1, td=0, comp=0, layout=0):
    import srsgpu
    return srsgpu.PuschChannelEstimation(
        scrambling_id=cfg["scrambling_id"], n_scid=cfg["n_scid"], dmrs_type=2 if cfg["dmrs_type2"] else 1,
        nof_tx_layers=layers, nof_rx_ports=cfg["nof_rx_ports"], start_symbol=cfg["start_symbol"],
        nof_symbols=cfg["nof_symbols"], dmrs_symbol_mask=cfg["dmrs_symbol_mask"], rb_start=cfg["rb_start"],
        nof_rb=cfg["nof_rb"], slot_index=cfg["slot"], scaling=cfg["scaling"], fd_smoothing=fd, td_strategy=td,
        compensate_cfo=comp, estimate_layout=layout)


# Stated tolerances with CFO / TA / interpolate (see tests/test_golden.py): estimates within CFO_TOL[td] x RMS channel,
# noise variance / RSRP / EPRE 1e-3 relative, CFO 0.05 Hz, time alignment 2 Tc.
CFO_TOL = {0: 1.5e-2, 1: 2.5e-2}
T_C = 1.0 / (480000 * 4096)


def pad4(grid):
    g = np.zeros((4,) + grid.shape[1:], np.uint16)
    g[: grid.shape[0]] = grid
    return g


def region(cfg):
    return (slice(cfg["start_symbol"], cfg["start_symbol"] + cfg["nof_symbols"]),
            slice(cfg["rb_start"] * 12, (cfg["rb_start"] + cfg["nof_rb"]) * 12))


def test_pusch_chest_golden(ctx):
    """Every reference-made case in ONE plan (one slot each)."""
    import srsgpu
    cases = list(G.pusch_chest_cases())
    grids = np.stack([pad4(g) for _, _, g, _, _ in cases])
    ests = [to_est(cfg, fd) for cfg, fd, _, _, _ in cases]
    ce, nv, m = srsgpu.PuschChannelEstimator(ctx, 24, 4).estimate_batch(grids, ests, list(range(len(cases))))
    for i, (cfg, fd, _, want, stats) in enumerate(cases):
        P = cfg["nof_rx_ports"]
        ls, ks = region(cfg)
        got = bf16_to_complex(ce[i, 0, :P])[:, ls, ks]
        w = bf16_to_complex(want)[:, ls, ks]
        assert np.max(np.abs(got - w)) < 1e-2 * np.sqrt(np.mean(np.abs(w) ** 2)), (i, cfg)
        np.testing.assert_allclose(nv[i, :P], stats[0], rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 0], stats[1], rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 1], stats[2], rtol=1e-3)


def test_pusch_chest_random_vs_oracle(ctx):
    """40 random transmissions (1..40 RB, 1-3 DM-RS symbols, DM-RS types 1 and 2, every smoothing strategy), each in
    its own 40-PRB slot, in ONE plan, against the restatement."""
    import srsgpu
    rng = np.random.default_rng(77)
    cases = [random_case(rng, 40) for _ in range(40)]
    fds = [int(rng.integers(0, 3)) for _ in cases]
    grids = np.stack([pad4(g) for _, g, _ in cases])
    ests = [to_est(cfg, fd) for (cfg, _, _), fd in zip(cases, fds)]
    ce, nv, m = srsgpu.PuschChannelEstimator(ctx, 40, 4).estimate_batch(grids, ests, list(range(len(cases))))
    for i, ((cfg, grid, _), fd) in enumerate(zip(cases, fds)):
        P = cfg["nof_rx_ports"]
        ch, nvo, rsrp, epre, _ = C.estimate(cfg, bf16_to_complex(grid), ["none", "mean", "filter"][fd])
        ls, ks = region(cfg)
        got = bf16_to_complex(ce[i, 0, :P])[:, ls, ks]
        w = ch[:, ls, ks]
        assert np.max(np.abs(got - w)) < 1e-2 * np.sqrt(np.mean(np.abs(w) ** 2)), (i, cfg, fd)
        np.testing.assert_allclose(nv[i, :P], nvo, rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 0], rsrp, rtol=1e-3)


def test_pusch_chest_shared_slot_100mhz(ctx):
    """64 UEs sharing one 273-PRB slot (4-5 RB each, 4 rx ports, DM-RS in symbol 2) over one smooth channel: one plan
    writes disjoint parts of the slot's estimate buffer; every UE against the restatement."""
    import srsgpu
    from pusch_demod_cases import bf16
    rng = np.random.default_rng(3)
    nsc = 12 * 273
    cfgs, rb = [], 0
    for u in range(64):
        nrb = 5 if u < 17 else 4
        cfgs.append(dict(slot=5, scrambling_id=1234, n_scid=0, dmrs_type2=0, scaling=1.4125375,
                         dmrs_symbol_mask=1 << 2, start_symbol=0, nof_symbols=14, rb_start=rb, nof_rb=nrb,
                         nof_rx_ports=4))
        rb += nrb
    k = np.arange(nsc)
    H = sum((rng.normal(size=(4, 1)) + 1j * rng.normal(size=(4, 1))) / np.sqrt(6) *
            np.exp(-2j * np.pi * k * rng.uniform(0, 30) / 4096) for _ in range(3))
    x = (rng.choice([-1, 1], (14, nsc)) + 1j * rng.choice([-1, 1], (14, nsc))) / np.sqrt(2)
    x[2, :] = 0
    for cfg in cfgs:
        sc = np.array([(cfg["rb_start"] + r) * 12 + 2 * j for r in range(cfg["nof_rb"]) for j in range(6)])
        x[2, sc] = cfg["scaling"] * C.dmrs_sequence(5, 2, 1234, 0, 0, cfg["rb_start"], cfg["nof_rb"])
    y = H[:, None, :] * x[None] + (rng.normal(size=(4, 14, nsc)) + 1j * rng.normal(size=(4, 14, nsc))) * 0.05
    grid = bf16(y)
    ests = [to_est(cfg) for cfg in cfgs]
    ce, nv, _ = srsgpu.PuschChannelEstimator(ctx, 273, 4).estimate_batch(grid[None], ests, [0] * 64)
    for i, cfg in enumerate(cfgs):
        ch, nvo, _, _, _ = C.estimate(cfg, bf16_to_complex(grid), "filter")
        ls, ks = region(cfg)
        got = bf16_to_complex(ce[0, 0])[:, ls, ks]
        w = ch[:, ls, ks]
        assert np.max(np.abs(got - w)) < 1e-2 * np.sqrt(np.mean(np.abs(w) ** 2)), i
        np.testing.assert_allclose(nv[i], nvo, rtol=1e-3)


def test_pusch_chest_cfo_ta_golden(ctx):
    """The reference's estimates with CFO estimation / compensation, time alignment and both time-domain strategies
    (tests/golden/pusch_chest_cfo.npz: du_low's default filter + average + CFO compensation, and the alternatives),
    every case in ONE plan: estimates, noise variance / RSRP / EPRE, TA and CFO within the stated tolerances."""
    import srsgpu
    cases = list(G.pusch_chest_cfo_cases())
    grids = np.stack([pad4(c[4]) for c in cases])
    ests = [to_est(cfg, fd, 1, td, comp) for cfg, fd, td, comp, _, _, _ in cases]
    ce, nv, m = srsgpu.PuschChannelEstimator(ctx, 64, 4).estimate_batch(grids, ests, list(range(len(cases))))
    for i, (cfg, fd, td, comp, _, want, stats) in enumerate(cases):
        P = cfg["nof_rx_ports"]
        ks = slice(cfg["rb_start"] * 12, (cfg["rb_start"] + cfg["nof_rb"]) * 12)
        got = bf16_to_complex(ce[i, 0, :P])[:, :, ks]
        w = bf16_to_complex(want)[:, :, ks]
        assert np.max(np.abs(got - w)) < CFO_TOL[td] * np.sqrt(np.mean(np.abs(w) ** 2)), (i, cfg, td, comp)
        np.testing.assert_allclose(nv[i, :P], stats[0], rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 0], stats[1], rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 1], stats[2], rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 4], stats[3], atol=2 * T_C)
        np.testing.assert_allclose(m[i, :P, 5], stats[4], atol=0.05)


def test_pusch_chest_273_golden(ctx):
    """configs[4]'s wideband jobs (160-273 PRB: 1638 pilots per DM-RS symbol, more than one pilot per lane of the
    1024-lane workgroup) against the reference's estimates (tests/golden/pusch_chest_273.npz, du_low defaults: filter,
    average, CFO compensation; the bench's test-mode channel at 26 / 30 dB and delay-spread channels), all five in ONE
    plan: estimate rows, noise variance / RSRP / EPRE (1e-3), SNR, TA (2 Tc) and CFO (0.05 Hz)."""
    import srsgpu
    cases = list(G.pusch_chest_273_cases())
    grids = np.stack([c[1] for c in cases])
    ests = [to_est(cfg, 2, 1, 0, 1) for cfg, _, _, _ in cases]
    ce, nv, m = srsgpu.PuschChannelEstimator(ctx, 273, 4).estimate_batch(grids, ests, list(range(len(cases))))
    rows = list(G.PUSCH_CHEST_273_ROWS)
    for i, (cfg, _, want_rows, stats) in enumerate(cases):
        P = cfg["nof_rx_ports"]
        ks = slice(cfg["rb_start"] * 12, (cfg["rb_start"] + cfg["nof_rb"]) * 12)
        got = bf16_to_complex(ce[i, 0, :P])[:, rows, ks]
        w = bf16_to_complex(want_rows)[:, :, ks]
        assert np.max(np.abs(got - w)) < CFO_TOL[0] * np.sqrt(np.mean(np.abs(w) ** 2)), (i, cfg)
        np.testing.assert_allclose(nv[i, :P], stats[0], rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 0], stats[1], rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 1], stats[2], rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 3], stats[1] / cfg["scaling"] ** 2 / stats[0], rtol=2e-3)
        np.testing.assert_allclose(m[i, :P, 4], stats[3], atol=2 * T_C)
        np.testing.assert_allclose(m[i, :P, 5], stats[4], atol=0.05)


def test_pusch_chest_cfo_ta_random_vs_oracle(ctx):
    """48 random transmissions with CFO and delay (1..100 RB, 1-3 DM-RS symbols, every smoothing, both time
    strategies, compensation on / off), ONE plan, against the restatement within the stated tolerances."""
    import srsgpu
    rng = np.random.default_rng(78)
    cases, opts = [], []
    for i in range(48):
        nrb = [1, 2, 3, 5, 12, 24, 52, 100][i % 8]
        cases.append(random_case(rng, 104, nof_rb=nrb, dmrs_type2=0, cfo_hz=rng.uniform(-2000, 2000),
                                 delay=rng.uniform(-30, 30)))
        opts.append((int(rng.integers(0, 3)), i % 2, (i // 2) % 2))
    grids = np.stack([pad4(g) for _, g, _ in cases])
    ests = [to_est(cfg, fd, 1, td, comp) for (cfg, _, _), (fd, td, comp) in zip(cases, opts)]
    ce, nv, m = srsgpu.PuschChannelEstimator(ctx, 104, 4).estimate_batch(grids, ests, list(range(len(cases))))
    for i, ((cfg, grid, _), (fd, td, comp)) in enumerate(zip(cases, opts)):
        P = cfg["nof_rx_ports"]
        ch, nvo, rsrp, epre, ex = C.estimate(cfg, bf16_to_complex(grid), ["none", "mean", "filter"][fd],
                                             ["average", "interpolate"][td], bool(comp))
        ls, ks = region(cfg)
        got = bf16_to_complex(ce[i, 0, :P])[:, ls, ks]
        w = ch[:, ls, ks]
        assert np.max(np.abs(got - w)) < CFO_TOL[td] * np.sqrt(np.mean(np.abs(w) ** 2)), (i, cfg, fd, td, comp)
        np.testing.assert_allclose(nv[i, :P], nvo, rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 0], rsrp, rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 4], ex["ta_s"], atol=2 * T_C)
        np.testing.assert_allclose(m[i, :P, 5], ex["cfo_hz"], atol=0.05)


def test_pusch_chest_two_jobs_per_wave_vs_oracle(ctx):
    """Few-RB plans (at most 64 pilots per job) run two jobs per wave, one per 32-lane half: 37 random transmissions
    (1..10 RB, 1-3 DM-RS symbols, 1-4 rx ports, DM-RS types 1 and 2, every smoothing, both time strategies, CFO
    compensation on / off, CFO and delay) in ONE plan, so neighbouring halves run different stage sequences and the job
    count is odd; every transmission against the restatement within the stated tolerances."""
    import srsgpu
    rng = np.random.default_rng(79)
    cases, opts = [], []
    for i in range(37):
        nrb = [1, 2, 3, 4, 5, 7, 10][i % 7]
        cases.append(random_case(rng, 10, nof_rb=nrb, dmrs_type2=0, cfo_hz=rng.uniform(-2000, 2000),
                                 delay=rng.uniform(-30, 30)))
        opts.append((int(rng.integers(0, 3)), i % 2, (i // 2) % 2))
    grids = np.stack([pad4(g) for _, g, _ in cases])
    ests = [to_est(cfg, fd, 1, td, comp) for (cfg, _, _), (fd, td, comp) in zip(cases, opts)]
    ce, nv, m = srsgpu.PuschChannelEstimator(ctx, 10, 4).estimate_batch(grids, ests, list(range(len(cases))))
    for i, ((cfg, grid, _), (fd, td, comp)) in enumerate(zip(cases, opts)):
        P = cfg["nof_rx_ports"]
        ch, nvo, rsrp, epre, ex = C.estimate(cfg, bf16_to_complex(grid), ["none", "mean", "filter"][fd],
                                             ["average", "interpolate"][td], bool(comp))
        ls, ks = region(cfg)
        got = bf16_to_complex(ce[i, 0, :P])[:, ls, ks]
        w = ch[:, ls, ks]
        assert np.max(np.abs(got - w)) < CFO_TOL[td] * np.sqrt(np.mean(np.abs(w) ** 2)), (i, cfg, fd, td, comp)
        np.testing.assert_allclose(nv[i, :P], nvo, rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 0], rsrp, rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 4], ex["ta_s"], atol=2 * T_C)
        np.testing.assert_allclose(m[i, :P, 5], ex["cfo_hz"], atol=0.05)


def test_pusch_compact_cfo_equals_per_symbol(ctx):
    """Compact layout with CFO compensation (the demodulator rotates each symbol's estimate) gives the LLRs of the
    per-symbol layout (the estimator rotates), bit for bit: 1-4 layers, 4 rx ports, DM-RS in symbols 2 and 11."""
    import torch
    import srsgpu
    rng = np.random.default_rng(12)
    dev = torch.device("cuda", 0)
    for L in (1, 2, 4):
        cfg, grid, _ = multilayer_case(rng, 24, L, 4, 16, rb_start=3, dmrs_mask=(1 << 2) | (1 << 11)) if L > 1 else \
            random_case(rng, 24, nof_rx_ports=4, nof_rb=16, dmrs_type2=0, dmrs_mask=(1 << 2) | (1 << 11),
                        cfo_hz=700.0)[:2] + (None,)
        cfg.update(start_symbol=0, nof_symbols=14)
        g4 = torch.from_numpy(pad4(grid).view(np.int32).reshape(-1).copy()).to(dev)
        outs = []
        for layout in (srsgpu.CE_PER_SYMBOL, srsgpu.CE_COMPACT):
            est = srsgpu.PuschChannelEstimatorPlan(
                ctx, srsgpu.make_pusch_chest_configs([to_est(cfg, 2, L, 0, 1, layout)], [0]), 24, 4)
            arr, _, total = srsgpu.make_pusch_demod_configs([srsgpu.PuschDemodulation(
                rnti=0x4601, n_id=77, modulation_order=6, nof_tx_layers=L, nof_rx_ports=4, start_symbol=0,
                nof_symbols=14, dmrs_symbol_mask=cfg["dmrs_symbol_mask"], dmrs_type=1, nof_cdm_groups_without_data=2,
                rb_start=cfg["rb_start"], nof_rb=cfg["nof_rb"], equalizer=srsgpu.EQ_MMSE if L > 2 else srsgpu.EQ_ZF,
                estimate_layout=layout, cfo_compensated=1)], [0])
            dem = srsgpu.PuschDemodulatorPlan(ctx, arr, 24, 4)
            d_ce = torch.zeros(4 * 4 * 14 * 288, dtype=torch.int32, device=dev)
            d_nv = torch.zeros(4, dtype=torch.float32, device=dev)
            d_llr = torch.zeros(total, dtype=torch.int8, device=dev)
            est.execute(g4, d_ce, d_nv)
            dem.execute(g4, d_ce, d_nv, d_llr)
            torch.cuda.synchronize()
            outs.append(d_llr.cpu().numpy())
        assert np.array_equal(outs[0], outs[1]), (L, np.mean(outs[0] != outs[1]))


@pytest.mark.parametrize("L", [2, 4])
def test_pusch_chest_multilayer(ctx, L):
    """Extension: ports 1000..1003 (w_f cover codes removed over pilot pairs) on 4 rx ports, 2 DM-RS symbols, 20 RB:
    every layer's estimate within -15 dB of the true channel (30 dB SNR)."""
    import srsgpu
    rng = np.random.default_rng(90 + L)
    cfg, grid, H = multilayer_case(rng, 24, L, 4, 20, rb_start=2, dmrs_mask=(1 << 2) | (1 << 11))
    ce, nv, _ = srsgpu.PuschChannelEstimator(ctx, 24, 4).estimate_batch(grid[None], [to_est(cfg, 2, L)], [0])
    ks = slice(cfg["rb_start"] * 12, (cfg["rb_start"] + cfg["nof_rb"]) * 12)
    for ly in range(L):
        est = bf16_to_complex(ce[0, ly])[:, 5, ks]
        err = np.mean(np.abs(est - H[ly][:, ks]) ** 2) / np.mean(np.abs(H[ly][:, ks]) ** 2)
        assert 10 * np.log10(err) < -15, (ly, 10 * np.log10(err))
    assert np.all(nv[0] > 0)


FD_NAMES, TD_NAMES = ["none", "mean", "filter"], ["average", "interpolate"]
ML_NOF_RB = [1, 2, 3, 4, 7, 16, 40]
ML_SCALINGS = [1.0, 1.4125375, 0.7071]
ML_SNR_DB = [5.0, 10.0, 15.0, 20.0, 25.0, 30.0, 35.0]


def multilayer_cases(rng, grid_prb, nof_multi, rb_sizes, single=(), masked=()):
    """Transmissions for one multi-layer plan, built by cycling through the classes (index i of the multi-layer ones):
    L = 2 + i % 3, DM-RS type (i // 3) % 2 and smoothing (i // 6) % 3 give every (L, type, fd) in 18 consecutive i;
    td = (i // 3 + i // 18) % 2 and compensation (i // 6) % 2 give every (L, td, comp) in 12 and every (type, td) in
    36; rb_sizes[i % len], 1 + i % 4 rx ports, [1, 2, 3, 2, 3][i % 5] DM-RS symbols, n_scid (i // 4) % 2 and scaling
    (i // 5) % 3 run at other periods (assert_multilayer_classes checks what comes out). CFO (+-200..1500 Hz, sign
    alternating) and delay where there are two or more DM-RS symbols; SNR ML_SNR_DB[5 i % 7]. Multi-layer indices in
    `masked` take a random_crb_mask of at most their RB count; every second average + compensation case with a CFO
    takes the compact layout. `single`: RB counts of single-layer random_case transmissions appended with cycled
    options. Returns dicts cfg, grid, H, L, fd, td, comp, layout, mask, cfo, snr."""
    import srsgpu
    from pusch_chest_cases import random_crb_mask, random_multilayer_case
    out, compact = [], 0
    for i in range(nof_multi):
        L, t2, fd = 2 + i % 3, (i // 3) % 2, (i // 6) % 3
        td, comp = (i // 3 + i // 18) % 2, (i // 6) % 2
        nrb, nd = rb_sizes[i % len(rb_sizes)], [1, 2, 3, 2, 3][i % 5]
        mask = random_crb_mask(rng, grid_prb, nrb) if i in masked else None
        cfo = (-1) ** i * rng.uniform(200, 1500) if nd >= 2 else 0.0
        delay = rng.uniform(-20, 20) if nd >= 2 else 0.0
        snr = ML_SNR_DB[5 * i % 7]
        cfg, grid, H = random_multilayer_case(
            rng, grid_prb, L, nof_rx_ports=1 + i % 4, nof_rb=nrb, dmrs_type2=t2, snr_db=snr,
            nof_dmrs=nd, cfo_hz=cfo, delay=delay, crb_mask=mask, n_scid=(i // 4) % 2,
            scaling=ML_SCALINGS[(i // 5) % 3])
        layout = srsgpu.CE_PER_SYMBOL
        if td == 0 and comp and nd >= 2:
            compact += 1
            layout = srsgpu.CE_COMPACT if compact % 2 else srsgpu.CE_PER_SYMBOL
        out.append(dict(cfg=cfg, grid=grid, H=H, L=L, fd=fd, td=td, comp=comp, layout=layout, mask=mask, cfo=cfo,
                        snr=snr))
    for j, nrb in enumerate(single):
        cfo = (-1) ** j * rng.uniform(200, 1500)
        cfg, grid, H = random_case(rng, grid_prb, nof_rb=nrb, cfo_hz=cfo, delay=rng.uniform(-20, 20),
                                   **({"nof_rx_ports": 1} if j == 0 else {}))
        out.append(dict(cfg=cfg, grid=grid, H=H[None], L=1, fd=j % 3, td=j % 2, comp=(j // 2) % 2,
                        layout=srsgpu.CE_PER_SYMBOL, mask=None, cfo=cfo, snr=None))  # snr: drawn by random_case
    return out


def nof_dmrs(cfg):
    return bin(cfg["dmrs_symbol_mask"]).count("1")


def assert_multilayer_classes(cases, rb_sizes, nof_single, nof_masked):
    """Every class the multi-layer tests name is in the plan."""
    import srsgpu
    ml = [c for c in cases if c["L"] > 1]
    assert {(c["L"], c["cfg"]["dmrs_type2"], c["fd"]) for c in ml} == \
        {(L, t, f) for L in (2, 3, 4) for t in (0, 1) for f in (0, 1, 2)}
    assert {(c["L"], c["td"], c["comp"]) for c in ml} == \
        {(L, t, k) for L in (2, 3, 4) for t in (0, 1) for k in (0, 1)}
    assert {c["cfg"]["nof_rb"] for c in ml if c["mask"] is None} == set(rb_sizes)
    # 2 RB of type 2 under the filter: 8 pilots, fewer than the 10 virtual pilots per edge its 21 taps ask for
    assert any(c["cfg"]["dmrs_type2"] and c["cfg"]["nof_rb"] == 2 and c["fd"] == 2 for c in ml)
    assert {nof_dmrs(c["cfg"]) for c in ml} == {1, 2, 3}
    assert any(c["td"] == 1 and nof_dmrs(c["cfg"]) == 3 for c in ml)  # six planes in a two-layer group
    assert {c["cfg"]["nof_rx_ports"] for c in ml} == {1, 2, 3, 4}
    assert {c["cfg"]["n_scid"] for c in ml} == {0, 1}
    assert {c["cfg"]["scaling"] for c in ml} == set(ML_SCALINGS)
    assert all((abs(c["cfo"]) >= 200) == (nof_dmrs(c["cfg"]) >= 2) for c in ml)
    assert {np.sign(c["cfo"]) for c in ml} == {-1.0, 0.0, 1.0}
    assert {c["snr"] for c in ml} == set(ML_SNR_DB)
    assert sum(c["L"] == 1 for c in cases) >= nof_single
    assert sum(c["mask"] is not None for c in ml) >= nof_masked
    assert {c["L"] for c in ml if c["layout"] == srsgpu.CE_COMPACT} == {2, 3, 4}
    assert any(c["layout"] == srsgpu.CE_PER_SYMBOL and c["td"] == 0 and c["comp"] and nof_dmrs(c["cfg"]) >= 2
               for c in ml)


def chest_plan_lds_bytes(cases):
    """Dynamic LDS per job of the plan over `cases`: chest_job_lds_bytes (srsran-5g_amd/csrc/pusch_chest.hip) of the
    plan-wide maxima that srsgpu_pusch_chest_plan_create_ex takes, restated here because the C ABI does not report it
    (the launcher runs two jobs per wave when no job has more than 64 pilots and twice this fits 64 KiB)."""
    n = d = w = q = gl = 1
    dft = 128
    for c in cases:
        cfg, t2 = c["cfg"], c["cfg"]["dmrs_type2"]
        per_rb = 4 if t2 else 6
        rbs = np.flatnonzero(c["mask"]) if c["mask"] is not None else np.arange(cfg["nof_rb"])
        span_rb = int(rbs[-1] - rbs[0] + 1)
        masked = span_rb != len(rbs)
        ta_re = (span_rb - 1) * 12 + (7 if t2 else 10) + 1 if t2 or masked else cfg["nof_rb"] * per_rb
        n, d = max(n, cfg["nof_rb"] * per_rb), max(d, nof_dmrs(cfg))
        w = max(w, ((2 * int(rbs[0] if c["mask"] is not None else cfg["rb_start"]) * per_rb) % 32
                    + 2 * span_rb * per_rb + 31) // 32)
        q, gl = max(q, nof_dmrs(cfg) if c["td"] else 1), max(gl, min(2, c["L"]))
        dft = max(dft, C.ta_dft_size(ta_re))
    region = max((d * n + gl * (n + 2 * 12)) * 8, dft * (8 + 4))
    return (q * gl * n * 8 + region + d * w * 4 + 32 * 4 + 15) // 16 * 16


def check_multilayer_plan(ctx, grid_prb, cases):
    """ONE plan over the cases (one slot each) against estimate_layers within the stated tolerances: estimates on the
    allocated REs of every layer and symbol (per layer, x the layer's RMS), noise variance / RSRP / EPRE, TA, CFO, and
    for the compact layout the unrotated row of the first symbol and every layer's CFO word."""
    import srsgpu
    ests = []
    for c in cases:
        e = to_est(c["cfg"], c["fd"], c["L"], c["td"], c["comp"], c["layout"])
        e.crb_mask = c["mask"]
        ests.append(e)
    grids = np.stack([pad4(c["grid"]) for c in cases])
    ce, nv, m = srsgpu.PuschChannelEstimator(ctx, grid_prb, 4).estimate_batch(grids, ests, list(range(len(cases))))
    ep = C.symbol_start_epochs(1)
    scs_hz = 30000.0
    rows = []

    def rel(got, want):
        return float(np.max(np.abs(got / want - 1)))

    for i, c in enumerate(cases):
        cfg, L, td, comp = c["cfg"], c["L"], c["td"], c["comp"]
        P, first = cfg["nof_rx_ports"], cfg["start_symbol"]
        ch, nvo, rsrp, epre, ex = C.estimate_layers(cfg, bf16_to_complex(c["grid"]), L, FD_NAMES[c["fd"]],
                                                    TD_NAMES[td], bool(comp), 1, c["mask"])
        rbs = np.flatnonzero(c["mask"]) if c["mask"] is not None else \
            np.arange(cfg["rb_start"], cfg["rb_start"] + cfg["nof_rb"])
        ks = np.concatenate([np.arange(rb * 12, rb * 12 + 12) for rb in rbs])
        word_hz = 0.0
        if c["layout"] == srsgpu.CE_COMPACT:
            ls = slice(first, first + 1)
            cfo_g = np.repeat(ex["cfo_hz_groups"], 2, axis=0)[:L]  # (L, P): layer ly belongs to group ly // 2
            want = ch[:, :, ls][..., ks] * np.exp(-2j * np.pi * ep[first] * cfo_g / scs_hz)[:, :, None, None]
            word = np.ascontiguousarray(ce[i, :L, :P, first + 1, ks[0]]).view(np.float32)[..., 0]
            word_hz = float(np.max(np.abs(word * scs_hz - cfo_g)))
        else:
            ls = slice(first, first + cfg["nof_symbols"])
            want = ch[:, :, ls][..., ks]
        got = bf16_to_complex(ce[i, :L, :P, ls])[..., ks]
        assert np.isfinite(got.real).all() and np.isfinite(got.imag).all(), (i, cfg, L)
        # np.max, not max: a NaN in any layer must reach the assertion
        est = float(np.max([np.max(np.abs(got[ly] - want[ly])) / np.sqrt(np.mean(np.abs(want[ly]) ** 2))
                            for ly in range(L)]))
        has_cfo = np.isfinite(ex["cfo_hz"])
        assert np.array_equal(np.isfinite(m[i, :P, 5]), has_cfo), (i, cfg)
        rows.append(dict(
            tag=(i, L, cfg["dmrs_type2"], cfg["nof_rb"], P, nof_dmrs(cfg), c["fd"], td, comp, c["layout"],
                 c["mask"] is not None),
            est=est, tol=1e-2 if td == 0 and not comp else CFO_TOL[td], nv=rel(nv[i, :P], nvo),
            nvm=rel(m[i, :P, 2], nvo), rsrp=rel(m[i, :P, 0], rsrp), epre=rel(m[i, :P, 1], epre),
            ta=float(np.max(np.abs(m[i, :P, 4] - ex["ta_s"]))) / T_C,
            cfo=float(np.max(np.abs(m[i, :P, 5] - ex["cfo_hz"])[has_cfo], initial=0.0)), word=word_hz))
    for r in rows:  # every figure before any assertion
        print("chest multilayer (i, L, type2, rb, P, D, fd, td, comp, layout, masked)=%s est %.2e/%.1e nv %.1e %.1e "
              "rsrp %.1e epre %.1e ta %.2f Tc cfo %.3f Hz word %.3f Hz" %
              (r["tag"], r["est"], r["tol"], r["nv"], r["nvm"], r["rsrp"], r["epre"], r["ta"], r["cfo"], r["word"]))
    for r in rows:
        assert r["est"] < r["tol"], r
        for key in ("nv", "nvm", "rsrp", "epre"):  # each on its own: a NaN fails its comparison
            assert r[key] <= 1e-3, (key, r)
        assert r["ta"] <= 2 and r["cfo"] <= 0.05 and r["word"] <= 0.05, r


def test_pusch_chest_multilayer_vs_oracle(ctx):
    """48 transmissions in 40-PRB slots, ONE 4-port plan, against the float64 restatement of multi-layer estimation:
    42 of 2-4 layers cycling through every (L, DM-RS type, smoothing) and (L, time strategy, CFO compensation), 1 / 2 /
    3 / 4 / 7 / 16 / 40 RB (1 RB: nof_v = per_rb; 1-3 RB: the filter length), 1-3 DM-RS symbols (interpolate with 3 of
    them and two layers per group: six planes), 1-4 rx ports, CFO and delay, 5-35 dB SNR, both n_scid, three scalings,
    five CRB masks and the compact layout's CFO words; plus six single-layer transmissions, so that the plan of
    max_gl = 2 also lays out GL = 1 jobs."""
    rng = np.random.default_rng(95)
    cases = multilayer_cases(rng, 40, 42, ML_NOF_RB, single=[1, 3, 5, 12, 40, 2], masked=(4, 13, 22, 31, 40))
    assert len(cases) == 48
    assert_multilayer_classes(cases, ML_NOF_RB, 6, 4)
    check_multilayer_plan(ctx, 40, cases)


def test_pusch_chest_multilayer_two_jobs_per_wave(ctx):
    """Multi-layer transmissions of 1..10 RB only (at most 64 pilots per job: two jobs per wave, one per 32-lane half,
    neighbouring halves on different stage sequences and group sizes), the class cycling of
    test_pusch_chest_multilayer_vs_oracle, plus one 1-port single-layer transmission: the job count is odd. The
    launcher's other condition for that instantiation, two jobs' LDS within 64 KiB, is asserted from
    chest_plan_lds_bytes (6128 B per job here)."""
    rng = np.random.default_rng(96)
    sizes = [1, 2, 3, 4, 5, 7, 10]
    cases = multilayer_cases(rng, 10, 36, sizes, single=[3], masked=(4, 13, 22, 31))
    assert_multilayer_classes(cases, sizes, 1, 4)
    jobs = sum(c["cfg"]["nof_rx_ports"] * ((c["L"] + 1) // 2) for c in cases)
    assert jobs % 2 == 1 and max(c["cfg"]["nof_rb"] for c in cases) * 6 <= 64, jobs
    assert 2 * chest_plan_lds_bytes(cases) <= 64 * 1024, chest_plan_lds_bytes(cases)
    check_multilayer_plan(ctx, 10, cases)


def test_pusch_chest_multilayer_wideband(ctx):
    """One plan over a 273-PRB grid (the 1024-lane multi-wave instantiation, 1638 pilots per job) with L = 4, 2 ports,
    273 RB, type 1, 2 DM-RS symbols, filter + average + CFO compensation, and L = 2, 2 ports, 273 RB, 3 DM-RS symbols,
    filter + interpolate: six planes of 1638 pilots, 145904 B of LDS per job by chest_job_lds_bytes, the largest
    footprint under the plan's 160 KiB check (plan creation accepts it: no smaller nof_rb is needed)."""
    import srsgpu
    from pusch_chest_cases import random_multilayer_case
    rng = np.random.default_rng(97)
    cases = []
    for L, nd, td, comp, cfo in [(4, 2, 0, 1, 650.0), (2, 3, 1, 0, -420.0)]:
        cfg, grid, H = random_multilayer_case(rng, 273, L, nof_rx_ports=2, nof_rb=273, dmrs_type2=0, snr_db=20.0,
                                              nof_dmrs=nd, cfo_hz=cfo, delay=rng.uniform(-20, 20))
        cases.append(dict(cfg=cfg, grid=grid, H=H, L=L, fd=2, td=td, comp=comp, layout=srsgpu.CE_PER_SYMBOL,
                          mask=None, cfo=cfo, snr=20.0))
    assert [(c["L"], nof_dmrs(c["cfg"]), c["td"], c["comp"], c["cfg"]["nof_rb"]) for c in cases] == \
        [(4, 2, 0, 1, 273), (2, 3, 1, 0, 273)]
    assert chest_plan_lds_bytes(cases) == 145904
    check_multilayer_plan(ctx, 273, cases)


def test_pusch_receive_chain(ctx):
    """Single-layer PUSCH receive chain on the GPU (channel estimation -> equalization + demapping + descrambling)
    against the oracle chain, 1-4 rx ports, every modulation: LLRs within one step on >= 99 % (the estimates agree
    within the tolerance above, the LLRs inherit it)."""
    import torch
    import srsgpu
    rng = np.random.default_rng(11)
    for P, qm in [(1, 2), (2, 4), (4, 6), (4, 8)]:
        cfg, grid, H = random_case(rng, 24, nof_rx_ports=P, nof_rb=10, dmrs_type2=0, snr_db=28, dmrs_mask=1 << 2)
        cfg.update(start_symbol=0, nof_symbols=14)
        # Data REs: QAM symbols of the right order through the same channel.
        lv = np.arange(-(2 ** (qm // 2) - 1), 2 ** (qm // 2), 2) / np.sqrt({2: 2, 4: 10, 6: 42, 8: 170}[qm])
        y = bf16_to_complex(grid)
        nsc = 288
        x = rng.choice(lv, (14, nsc)) + 1j * rng.choice(lv, (14, nsc))
        k = np.arange(nsc)
        Hc = sum((rng.normal(size=(P, 1)) + 1j * rng.normal(size=(P, 1))) / np.sqrt(6) *
                 np.exp(-2j * np.pi * k * rng.uniform(0, 20) / 4096) for _ in range(3))
        sc = np.array([(cfg["rb_start"] + r) * 12 + 2 * j for r in range(cfg["nof_rb"]) for j in range(6)])
        x[2, :] = 0
        x[2, sc] = cfg["scaling"] * C.dmrs_sequence(cfg["slot"], 2, cfg["scrambling_id"], cfg["n_scid"], 0,
                                                    cfg["rb_start"], cfg["nof_rb"])
        y = Hc[:, None, :] * x[None] + (rng.normal(size=(P, 14, nsc)) + 1j * rng.normal(size=(P, 14, nsc))) * 0.03
        from pusch_demod_cases import bf16
        grid = bf16(y)
        dcfg = dict(rnti=0x4601, n_id=77, qm=qm, nof_layers=1, nof_rx_ports=P, start_symbol=0, nof_symbols=14,
                    dmrs_symbol_mask=1 << 2, dmrs_type2=0, nof_cdm_groups_without_data=2, rb_start=cfg["rb_start"],
                    nof_rb=cfg["nof_rb"])
        ch, nvo, _, _, _ = C.estimate(cfg, bf16_to_complex(grid), "filter")
        from pusch_demod_cases import bf16 as to_bf16
        want = D.demodulate(dcfg, bf16_to_complex(grid).astype(np.complex64),
                            bf16_to_complex(to_bf16(ch))[None].astype(np.complex64), nvo.astype(np.float32))
        dev = torch.device("cuda", 0)
        g4 = torch.from_numpy(pad4(grid).view(np.int32).reshape(-1).copy()).to(dev)
        d_ce = torch.zeros(4 * 4 * 14 * nsc, dtype=torch.int32, device=dev)
        d_nv = torch.zeros(4, dtype=torch.float32, device=dev)
        est = srsgpu.PuschChannelEstimatorPlan(ctx, srsgpu.make_pusch_chest_configs([to_est(cfg)], [0]), 24, 4)
        arr, _, total = srsgpu.make_pusch_demod_configs([srsgpu.PuschDemodulation(
            rnti=0x4601, n_id=77, modulation_order=qm, nof_tx_layers=1, nof_rx_ports=P, start_symbol=0, nof_symbols=14,
            dmrs_symbol_mask=1 << 2, dmrs_type=1, nof_cdm_groups_without_data=2, rb_start=cfg["rb_start"],
            nof_rb=cfg["nof_rb"])], [0])
        dem = srsgpu.PuschDemodulatorPlan(ctx, arr, 24, 4)
        d_llr = torch.zeros(total, dtype=torch.int8, device=dev)
        est.execute(g4, d_ce, d_nv)
        dem.execute(g4, d_ce, d_nv, d_llr)
        torch.cuda.synchronize()
        got = d_llr.cpu().numpy().astype(np.int16)
        d = np.abs(got - want.astype(np.int16))
        assert got.size == want.size and np.mean(d <= 1) >= 0.99, (P, qm, np.mean(d <= 1))


def test_pusch_chest_crb_mask_random_vs_oracle(ctx):
    """40 non-contiguous CRB masks (RBG runs / scattered CRBs over a 273-PRB grid, types 1 and 2, every smoothing, both
    time strategies, CFO compensation on / off, contiguous transmissions mixed in) in ONE plan against the
    restatement: estimates on every allocated CRB within the stated tolerance, noise variance / RSRP 1e-3, TA 2 Tc,
    CFO 0.05 Hz. (The restatement is pinned against the reference's metrics and written estimates in
    tests/test_oracle_vs_reference.py::test_pusch_chest_crb_mask_oracle_vs_reference.)"""
    import srsgpu
    from pusch_chest_cases import random_crb_mask
    rng = np.random.default_rng(79)
    cases, opts, masks = [], [], []
    for i in range(40):
        mask = random_crb_mask(rng, 273) if i % 5 else None
        cases.append(random_case(rng, 273, nof_rb=int(rng.integers(1, 40)), dmrs_type2=i % 3 == 2,
                                 cfo_hz=rng.uniform(-1500, 1500), delay=rng.uniform(-20, 20), crb_mask=mask))
        opts.append((int(rng.integers(0, 3)), i % 2, (i // 2) % 2))
        masks.append(mask)
    grids = np.stack([pad4(g) for _, g, _ in cases])
    ests = []
    for (cfg, _, _), (fd, td, comp), mask in zip(cases, opts, masks):
        e = to_est(cfg, fd, 1, td, comp)
        e.crb_mask = mask
        ests.append(e)
    ce, nv, m = srsgpu.PuschChannelEstimator(ctx, 273, 4).estimate_batch(grids, ests, list(range(len(cases))))
    for i, ((cfg, grid, _), (fd, td, comp), mask) in enumerate(zip(cases, opts, masks)):
        P = cfg["nof_rx_ports"]
        ch, nvo, rsrp, epre, ex = C.estimate(cfg, bf16_to_complex(grid), ["none", "mean", "filter"][fd],
                                             ["average", "interpolate"][td], bool(comp), crb_mask=mask)
        ls = slice(cfg["start_symbol"], cfg["start_symbol"] + cfg["nof_symbols"])
        rbs = np.flatnonzero(mask) if mask is not None else np.arange(cfg["rb_start"], cfg["rb_start"] + cfg["nof_rb"])
        ks = np.concatenate([np.arange(rb * 12, rb * 12 + 12) for rb in rbs])
        got = bf16_to_complex(ce[i, 0, :P])[:, ls][:, :, ks]
        w = ch[:, ls][:, :, ks]
        assert np.max(np.abs(got - w)) < CFO_TOL[td] * np.sqrt(np.mean(np.abs(w) ** 2)), (i, cfg, fd, td, comp)
        np.testing.assert_allclose(nv[i, :P], nvo, rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 0], rsrp, rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 1], epre, rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 4], ex["ta_s"], atol=2 * T_C)
        np.testing.assert_allclose(m[i, :P, 5], ex["cfo_hz"], atol=0.05)


def test_pusch_crb_mask_compact_cfo_chain(ctx):
    """A CRB-mask PUSCH through estimator -> demodulator: the compact layout with CFO compensation (the CFO word at the
    first allocated CRB) gives the per-symbol layout's LLRs bit for bit, and the LLRs match the oracle chain."""
    import torch
    import srsgpu
    from pusch_chest_cases import random_crb_mask
    rng = np.random.default_rng(13)
    dev = torch.device("cuda", 0)
    mask = random_crb_mask(rng, 51)
    cfg, grid, _ = random_case(rng, 51, nof_rx_ports=4, dmrs_type2=0, dmrs_mask=(1 << 2) | (1 << 11), cfo_hz=600.0,
                               crb_mask=mask, snr_db=30)
    cfg.update(start_symbol=0, nof_symbols=14)
    g4 = torch.from_numpy(pad4(grid).view(np.int32).reshape(-1).copy()).to(dev)
    outs = []
    for layout in (srsgpu.CE_PER_SYMBOL, srsgpu.CE_COMPACT):
        e = to_est(cfg, 2, 1, 0, 1, layout)
        e.crb_mask = mask
        exts, _k1 = srsgpu.make_crb_mask_exts([e], 51)
        est = srsgpu.PuschChannelEstimatorPlan(ctx, srsgpu.make_pusch_chest_configs([e], [0]), 51, 4, exts)
        d = srsgpu.PuschDemodulation(
            rnti=0x4601, n_id=77, modulation_order=6, nof_tx_layers=1, nof_rx_ports=4, start_symbol=0, nof_symbols=14,
            dmrs_symbol_mask=cfg["dmrs_symbol_mask"], dmrs_type=1, nof_cdm_groups_without_data=2,
            rb_start=cfg["rb_start"], nof_rb=cfg["nof_rb"], estimate_layout=layout, cfo_compensated=1, crb_mask=mask)
        arr, _, total = srsgpu.make_pusch_demod_configs([d], [0])
        dexts, _k2 = srsgpu.make_crb_mask_exts([d], 51)
        dem = srsgpu.PuschDemodulatorPlan(ctx, arr, 51, 4, dexts)
        d_ce = torch.zeros(4 * 4 * 14 * 612, dtype=torch.int32, device=dev)
        d_nv = torch.zeros(4, dtype=torch.float32, device=dev)
        d_llr = torch.zeros(total, dtype=torch.int8, device=dev)
        est.execute(g4, d_ce, d_nv)
        dem.execute(g4, d_ce, d_nv, d_llr)
        torch.cuda.synchronize()
        outs.append(d_llr.cpu().numpy())
        if layout == srsgpu.CE_PER_SYMBOL:
            ce_ps = d_ce.cpu().numpy().view(np.uint16).reshape(4, 4, 14, 612, 2)
            nv_ps = d_nv.cpu().numpy()
    assert np.array_equal(outs[0], outs[1]), np.mean(outs[0] != outs[1])
    dcfg = dict(rnti=0x4601, n_id=77, qm=6, nof_layers=1, nof_rx_ports=4, start_symbol=0, nof_symbols=14,
                dmrs_symbol_mask=cfg["dmrs_symbol_mask"], dmrs_type2=0, nof_cdm_groups_without_data=2,
                rb_start=cfg["rb_start"], nof_rb=cfg["nof_rb"])
    want, _ = D.demodulate_ex(dcfg, bf16_to_complex(pad4(grid)).astype(np.complex64),
                              bf16_to_complex(ce_ps[:1]).astype(np.complex64), nv_ps, crb_mask=mask)
    d = np.abs(outs[0].astype(np.int16) - want.astype(np.int16))
    assert d.max() <= 1 and np.mean(d > 0) < 0.01, (d.max(), np.mean(d > 0))


def test_pusch_chest_low_papr_random_vs_oracle(ctx):
    """Transform-precoding DM-RS (low-PAPR sequences: phase tables for 1-4 PRB, the length-30 formula, Zadoff-Chu)
    in ONE plan with pseudo-random transmissions, against the restatement (pinned against the reference's estimator by
    test_pusch_chest_low_papr_oracle_vs_reference): estimates, noise variance / RSRP, TA, CFO within the stated
    tolerances."""
    import srsgpu
    from pusch_demod_cases import valid_tp_prbs
    rng = np.random.default_rng(81)
    sizes = [1, 2, 3, 4, 5] + valid_tp_prbs(100)[5:]
    cases, opts, ids = [], [], []
    for i in range(36):
        lp = i % 4 != 3
        nid = int(rng.integers(0, 1008)) if lp else None
        cases.append(random_case(rng, 104, nof_rb=int(sizes[i % len(sizes)]), dmrs_type2=0,
                                 cfo_hz=rng.uniform(-1500, 1500), delay=rng.uniform(-20, 20), low_papr_id=nid))
        opts.append((int(rng.integers(0, 3)), i % 2, (i // 2) % 2))
        ids.append(nid)
    grids = np.stack([pad4(g) for _, g, _ in cases])
    ests = []
    for (cfg, _, _), (fd, td, comp), nid in zip(cases, opts, ids):
        e = to_est(cfg, fd, 1, td, comp)
        if nid is not None:
            e.dmrs_sequence, e.scrambling_id = srsgpu.DMRS_LOW_PAPR, nid
        ests.append(e)
    ce, nv, m = srsgpu.PuschChannelEstimator(ctx, 104, 4).estimate_batch(grids, ests, list(range(len(cases))))
    for i, ((cfg, grid, _), (fd, td, comp), nid) in enumerate(zip(cases, opts, ids)):
        P = cfg["nof_rx_ports"]
        ch, nvo, rsrp, epre, ex = C.estimate(cfg, bf16_to_complex(grid), ["none", "mean", "filter"][fd],
                                             ["average", "interpolate"][td], bool(comp), low_papr_id=nid)
        ls, ks = region(cfg)
        got = bf16_to_complex(ce[i, 0, :P])[:, ls, ks]
        w = ch[:, ls, ks]
        assert np.max(np.abs(got - w)) < CFO_TOL[td] * np.sqrt(np.mean(np.abs(w) ** 2)), (i, cfg, fd, td, comp)
        np.testing.assert_allclose(nv[i, :P], nvo, rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 0], rsrp, rtol=1e-3)
        np.testing.assert_allclose(m[i, :P, 4], ex["ta_s"], atol=2 * T_C)
        np.testing.assert_allclose(m[i, :P, 5], ex["cfo_hz"], atol=0.05)


def test_pusch_transform_precoding_receive_chain(ctx):
    """DFT-s-OFDM PUSCH end to end on the GPU: a transform-precoded 64QAM transmission (data DFT-spread over the
    allocation, low-PAPR DM-RS in symbols 2 and 11, frequency-selective channel, CFO, noise) through the estimator
    (low-PAPR, CFO compensation) and the demodulator (transform precoding) matches the oracle chain: LLRs within one
    step on >= 99 %, hard decisions of the clean data bits all correct."""
    import torch
    import srsgpu
    from pusch_demod_cases import QAM_AMP, bf16
    rng = np.random.default_rng(14)
    dev = torch.device("cuda", 0)
    G, nrb, rb0, P, qm, nid = 52, 12, 7, 4, 6, 321
    mask = (1 << 2) | (1 << 11)
    cfg, grid, H = random_case(rng, G, nof_rx_ports=P, nof_rb=nrb, dmrs_type2=0, dmrs_mask=mask, snr_db=30,
                               low_papr_id=nid)
    cfg.update(start_symbol=0, nof_symbols=14, rb_start=rb0)
    # Rebuild the grid with DFT-spread 64QAM data on the non-DM-RS symbols and the DM-RS at the allocation.
    nsc, M = 12 * G, 12 * nrb
    lv = np.arange(-7, 8, 2) * QAM_AMP[qm]
    x = np.zeros((14, nsc), np.complex128)
    data = {}
    for l in range(14):
        sc = np.arange(rb0 * 12, rb0 * 12 + M)
        if (mask >> l) & 1:
            x[l, sc[0::2]] = cfg["scaling"] * C.low_papr_sequence(nid % 30, M // 2)
        else:
            d = rng.choice(lv, M) + 1j * rng.choice(lv, M)
            data[l] = d
            x[l, sc] = np.fft.fft(d) / np.sqrt(M)
    y = H[:, None, :] * x[None]
    y += (rng.normal(size=y.shape) + 1j * rng.normal(size=y.shape)) * np.sqrt(10 ** (-3.0) / 2)
    grid = bf16(y)
    est = srsgpu.PuschChannelEstimation(
        scrambling_id=nid, n_scid=0, dmrs_type=1, nof_tx_layers=1, nof_rx_ports=P, start_symbol=0, nof_symbols=14,
        dmrs_symbol_mask=mask, rb_start=rb0, nof_rb=nrb, slot_index=3, scaling=cfg["scaling"],
        compensate_cfo=1, dmrs_sequence=srsgpu.DMRS_LOW_PAPR)
    dem = srsgpu.PuschDemodulation(
        rnti=0x4601, n_id=77, modulation_order=qm, nof_tx_layers=1, nof_rx_ports=P, start_symbol=0, nof_symbols=14,
        dmrs_symbol_mask=mask, dmrs_type=1, nof_cdm_groups_without_data=2, rb_start=rb0, nof_rb=nrb,
        transform_precoding=1)
    g4 = torch.from_numpy(pad4(grid).view(np.int32).reshape(-1).copy()).to(dev)
    eplan = srsgpu.PuschChannelEstimatorPlan(ctx, srsgpu.make_pusch_chest_configs([est], [0]), G, 4)
    arr, _, total = srsgpu.make_pusch_demod_configs([dem], [0])
    dplan = srsgpu.PuschDemodulatorPlan(ctx, arr, G, 4)
    d_ce = torch.zeros(4 * 4 * 14 * nsc, dtype=torch.int32, device=dev)
    d_nv = torch.zeros(4, dtype=torch.float32, device=dev)
    d_llr = torch.zeros(total, dtype=torch.int8, device=dev)
    eplan.execute(g4, d_ce, d_nv)
    dplan.execute(g4, d_ce, d_nv, d_llr)
    torch.cuda.synchronize()
    got = d_llr.cpu().numpy()
    ce = d_ce.cpu().numpy().view(np.uint16).reshape(4, 4, 14, nsc, 2)
    dcfg = dict(rnti=0x4601, n_id=77, qm=qm, nof_layers=1, nof_rx_ports=P, start_symbol=0, nof_symbols=14,
                dmrs_symbol_mask=mask, dmrs_type2=0, nof_cdm_groups_without_data=2, rb_start=rb0, nof_rb=nrb)
    want, _ = D.demodulate_ex(dcfg, bf16_to_complex(pad4(grid)).astype(np.complex64),
                              bf16_to_complex(ce[:1]).astype(np.complex64), d_nv.cpu().numpy(),
                              transform_precoding=True)
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert d.max() <= 1 and np.mean(d > 0) < 0.01, (d.max(), np.mean(d > 0))
    # Descramble and compare the hard decisions with the sent 64QAM symbols.
    c = D.gold_sequence(0x4601 * (1 << 15) + 77, got.size)
    llr = np.where(c == 1, -got.astype(np.int16), got.astype(np.int16))
    sent = np.concatenate([data[l] for l in sorted(data)])
    hard = D.modulate_bits((llr <= 0).astype(np.uint8), qm)
    assert np.mean(np.abs(hard - sent.astype(np.complex64)) > 1e-3) < 1e-3


def test_pusch_chest_execute_copy(ctx):
    """srsgpu_pusch_chest_plan_execute_copy (the slot batch's split grid copy): the wideband 273-PRB jobs estimated
    from grids holding only their DM-RS symbol rows while the same launch copies every other row in equal the plain
    execute over the complete grids bit for bit (estimates, noise variances, metrics), and the copied rows arrive."""
    import torch
    import srsgpu
    dev = torch.device("cuda", 0)
    cases = list(G.pusch_chest_273_cases())
    grids = np.ascontiguousarray(np.stack([c[1] for c in cases]), np.uint16)
    ests = [to_est(cfg, 2, 1, 0, 1) for cfg, _, _, _ in cases]
    S, Pg, L, nsc = grids.shape[:4]
    exts, _keep = srsgpu.make_crb_mask_exts(ests, 273)
    plan = srsgpu.PuschChannelEstimatorPlan(ctx, srsgpu.make_pusch_chest_configs(ests, list(range(S))), 273, Pg, exts)
    full = torch.from_numpy(grids.view(np.int32).reshape(-1).copy()).to(dev)
    part = torch.zeros_like(full)
    rows = full.view(S, Pg, L, nsc)
    prow = part.view(S, Pg, L, nsc)
    dmrs = {l for cfg, _, _, _ in cases for l in range(14) if (cfg["dmrs_symbol_mask"] >> l) & 1}
    g = torch.Generator().manual_seed(3)
    for l in range(L):
        if l not in dmrs:  # data rows (the golden grids hold only the DM-RS rows): something to copy
            rows[:, :, l] = torch.randint(-2**31, 2**31 - 1, (S, Pg, nsc), dtype=torch.int32, generator=g).to(dev)
    spans = []
    for s in range(S):
        for p in range(Pg):
            for l in range(L):
                if l in dmrs:
                    prow[s, p, l].copy_(rows[s, p, l])
                else:
                    spans.append((rows[s, p, l], prow[s, p, l]))
    outs = []
    for k in range(2):
        ce = torch.zeros(S * 4 * Pg * L * nsc, dtype=torch.int32, device=dev)
        nv = torch.zeros(4 * S, dtype=torch.float32, device=dev)
        m = torch.zeros(4 * srsgpu.CHEST_METRICS * S, dtype=torch.float32, device=dev)
        if k == 0:
            plan.execute(full, ce, nv, m)
        else:
            keep = plan.execute_copy(part, ce, nv, spans, m)
        outs.append((ce, nv, m))
    torch.cuda.synchronize(dev)
    del keep
    plan.close()
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    assert torch.equal(full, part)
