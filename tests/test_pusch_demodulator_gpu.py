"""GPU parity of the PUSCH demodulator (equalization + soft demapping + descrambling; srsgpu_pusch_demodulator_plan
through the C ABI) against the reference's own LLRs (tests/golden/pusch_demod.npz, made by pusch_demodulator_impl)
and the numpy restatement (oracle/pusch_demod_oracle.py).

Tolerances (soft LLRs, floating point): against the reference's own LLRs (the golden files) and in the random
batches kept from before, for the reference's paths (ZF 1 x N, ZF 2 x N, MMSE with one layer, transform precoding)
every LLR equal or one quantisation step (20 / 120) apart, < 5 % differing (the reference's AVX2 equalizer uses an
approximate reciprocal; the GPU divides exactly).

Against the restatement, which divides exactly and computes in the kernel's order, the same paths are held to
close_ref (test_pusch_demod_ref_*, test_pusch_demod_tp_*): every LLR equal or one step apart, fewer than
pusch_demod_cases.REF_PATHS_SHARE_BOUND = 1e-3 differing, the rule of the MMSE tests below: ten times what rounding
alone moves, floored at 1e-3. Rounding alone, measured without the kernel in
tests/test_pusch_demod_reference_paths_oracle.py: float32 against float64 in D.equalize's formulas 1.0e-5 in the worst
ZF case (one LLR of 97 344); the kernel's float32 Stockham inverse DFT restated in numpy (pusch_demod_cases.tp_float32)
against the restatement's complex128 one 2.9e-6 over the 53 sizes together (one LLR of 342 240); recorded as
REF_PATHS_FLOAT32_SHARE = 1e-4. The kernel's largest observed shares: ZF 1 x N, ZF 2 x N and one-layer MMSE 0 (no LLR
differs in any of the 24 instantiations, the mixed plan, the large plans and the degenerate cases); transform
precoding one LLR over all 53 sizes (5.6e-4 of its transmission's 1 800: M_RB = 75, QPSK), none in the extras. Every
case asserts first that at least 60 % of the restatement's LLRs are neither 0 nor +-120 (the SNRs of
pusch_demod_cases.MMSE_SNR_DB less the diversity gain). Against the restatement perturbed by hand, the kernel fails
close_ref on every case the perturbation applies to: ZF 1 x N variance as max(nv) / sum |h|^2 (12 of 12), ZF 2 x N
with the mean noise variance (8 of 8), its layers swapped (8 of 8), equalised symbols x 1.02 (24 of 24, and 64 of 64
transform-precoded), inverse-DFT scale x 1.02 (64 of 64), per-RE variances instead of their symbol mean (64 of 64),
the mean over all variances, invalid ones included, on the dead-subcarrier case (1 of 1). No defect was found in the
kernels by these tests; reading them found that the plan accepted grid indices whose estimates end beyond the kernels'
32-bit byte offsets, which it now refuses (test_pusch_demod_rejects_estimates_past_32bit_byte_offsets).

The multi-layer MMSE extension (float32 Cholesky on the GPU) has no reference: it is held to the float64 restatement
D.equalize_mmse (itself checked in tests/test_pusch_demod_mmse_oracle.py) with every LLR equal or one step apart and
fewer than pusch_demod_cases.MMSE_SHARE_BOUND = 1e-3 of them differing. The bound is ten times the share that float32
arithmetic alone moves, in the kernel's own sequence restated in numpy (pusch_demod_cases.mmse_float32: 7.9e-5 in the
worst of these tests' cases, rounded up to 1e-4), the factor covering the kernel's 1-ulp v_rsq / v_rcp and its FMA
contraction, floored at 1e-3. The kernel's largest observed share is 8.9e-5 on the informative cases (L = 3, P = 3,
64QAM: one LLR of 11 232) and 1.2e-4 on the 25 dB cases of test_pusch_demod_mmse_multilayer; no LLR is more than one step off. Every
case asserts first that at least 60 % of the restatement's LLRs are neither 0 nor +-120. Against the restatement
perturbed by hand, all 24 cases of test_pusch_demod_mmse_every_instantiation fail: the variance without the 1 / g
unbiasing, nv as the mean over the ports, layers 1 and 2 swapped, the symbols scaled by 1.02."""
import numpy as np
import pytest

import golden_lib as G
import pusch_demod_cases as K
import pusch_demod_oracle as D
from pusch_demod_cases import from_bf16, random_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


def to_demod(cfg, mmse=False):
    import srsgpu
    return srsgpu.PuschDemodulation(
        rnti=cfg["rnti"], n_id=cfg["n_id"], modulation_order=cfg["qm"], nof_tx_layers=cfg["nof_layers"],
        nof_rx_ports=cfg["nof_rx_ports"], start_symbol=cfg["start_symbol"], nof_symbols=cfg["nof_symbols"],
        dmrs_symbol_mask=cfg["dmrs_symbol_mask"], dmrs_type=2 if cfg["dmrs_type2"] else 1,
        nof_cdm_groups_without_data=cfg["nof_cdm_groups_without_data"], rb_start=cfg["rb_start"],
        nof_rb=cfg["nof_rb"], equalizer=srsgpu.EQ_MMSE if mmse else srsgpu.EQ_ZF)


def pad_slot(grid, H, nv, Pg=4):
    """One slot's buffers in the plan layout: grid (Pg, 14, nsc, 2), estimates (4, Pg, 14, nsc, 2), noise (4,)."""
    P, L = grid.shape[0], H.shape[0]
    g = np.zeros((Pg,) + grid.shape[1:], np.uint16)
    g[:P] = grid
    h = np.zeros((4, Pg) + H.shape[2:], np.uint16)
    h[:L, :P] = H
    n = np.zeros(4, np.float32)
    n[:P] = nv
    return g, h, n


def close(got, want, frac=0.05):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    return d.max() <= 1 and np.mean(d > 0) < frac, (int(d.max()), float(np.mean(d > 0)))


def test_pusch_demod_golden(ctx):
    """Every reference-made case, all in ONE plan (one slot each)."""
    import srsgpu
    cases = list(G.pusch_demod_cases())
    grids, hs, nvs, demods = [], [], [], []
    for cfg, mmse, grid, H, nv, _ in cases:
        g, h, n = pad_slot(grid, H, nv)
        grids.append(g)
        hs.append(h)
        nvs.append(n)
        demods.append(to_demod(cfg, mmse))
    got = srsgpu.PuschDemodulator(ctx, 24, 4).demodulate_batch(np.stack(grids), np.stack(hs), np.stack(nvs), demods,
                                                               list(range(len(cases))))
    for (cfg, mmse, _, _, _, want), llr in zip(cases, got):
        ok, stats = close(llr, want)
        assert llr.size == want.size and ok, (cfg, stats)


@pytest.mark.parametrize("qm", [2, 4, 6, 8])
def test_pusch_demod_demapper_golden(ctx, qm):
    """The demapper through the whole kernel: one layer, one port, unit channel (the equalizer passes the symbol
    through with nvar = the port's noise variance), the reference demapper vectors' symbols, against the oracle demapper
    (itself pinned to those vectors) with the descrambling applied."""
    import srsgpu
    for q, x, nv, want in G.demapper_cases():
        if q != qm:
            continue
        n = 3900  # 25 PRB x 13 symbols x 12 REs, one DM-RS symbol without data
        cfg = dict(rnti=0, n_id=0, qm=qm, nof_layers=1, nof_rx_ports=1, start_symbol=0, nof_symbols=14,
                   dmrs_symbol_mask=1 << 2, dmrs_type2=0, nof_cdm_groups_without_data=2, rb_start=0, nof_rb=25)
        res = D.data_res(0, 14, 1 << 2, 0, 2, 0, 25)
        assert len(res) == n
        grid = np.zeros((4, 14, 300, 2), np.uint16)
        H = np.zeros((4, 4, 14, 300, 2), np.uint16)
        # The ZF output is y conj(h) / |h|^2 with nvar = nv: feed y = x (as bf16) and h = 1.
        from pusch_demod_cases import bf16
        xs = x[:n]
        for i, (l, k) in enumerate(res):
            grid[0, l, k] = bf16(np.array([xs[i]]))[0]
        H[0, 0, :, :, 0] = 0x3F80  # 1.0
        nvar = np.array([0.1, 0, 0, 0], np.float32)
        got = srsgpu.PuschDemodulator(ctx, 25, 4).demodulate_batch(grid[None], H[None], nvar[None],
                                                                   [to_demod(cfg)], [0])[0]
        xq = from_bf16(bf16(xs))
        ref_llr = D.demap(xq, np.full(n, 0.1, np.float32), qm).astype(np.int16)
        c = D.gold_sequence(0, ref_llr.size)
        want2 = np.where(c == 1, -ref_llr, ref_llr)
        ok, stats = close(got, want2, frac=0.001)
        assert ok, stats


def test_pusch_demod_random_batch(ctx):
    """60 random transmissions (1-2 layers, 1-4 ports, ZF / MMSE, every modulation, random DM-RS patterns), each in
    its own 40-PRB slot, in ONE plan, against the oracle."""
    import srsgpu
    rng = np.random.default_rng(42)
    prb = 40
    grids, hs, nvs, demods, want = [], [], [], [], []
    for t in range(60):
        cfg, grid, H, nv = random_case(rng, prb)
        mmse = bool(t % 4 == 3 and cfg["nof_layers"] == 1)
        g, h, n = pad_slot(grid, H, nv)
        grids.append(g)
        hs.append(h)
        nvs.append(n)
        demods.append(to_demod(cfg, mmse))
        want.append(D.demodulate(cfg, from_bf16(grid), from_bf16(H), nv, mmse))
    got = srsgpu.PuschDemodulator(ctx, prb, 4).demodulate_batch(np.stack(grids), np.stack(hs), np.stack(nvs), demods,
                                                                list(range(60)))
    for i, (a, b) in enumerate(zip(got, want)):
        ok, stats = close(a, b)
        assert a.size == b.size and ok, (i, demods[i], stats)


def close_mmse(got, want):
    """The multi-layer MMSE tolerance: every LLR equal or one step apart, fewer than MMSE_SHARE_BOUND differing."""
    if got.size != want.size:
        return False, (got.size, want.size)
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    print("max step", int(d.max()), "share differing", float(np.mean(d > 0)))
    return d.max() <= 1 and np.mean(d > 0) < K.MMSE_SHARE_BOUND, (int(d.max()), float(np.mean(d > 0)))


@pytest.mark.parametrize("L", [2, 3, 4])
def test_pusch_demod_mmse_multilayer(ctx, L):
    """MMSE with 2-4 layers over 4 ports (extension beyond the open-source reference) against float64 numpy MMSE, at
    25 dB (most LLRs saturated: the informative cases are test_pusch_demod_mmse_every_instantiation's)."""
    import srsgpu
    rng = np.random.default_rng(50 + L)
    cfg, grid, H, nv = random_case(rng, 52, nof_layers=L, nof_rx_ports=4, snr_db=25)
    want = D.demodulate(cfg, from_bf16(grid), from_bf16(H), nv, mmse=True).astype(np.int16)
    g, h, n = pad_slot(grid, H, nv)
    got = srsgpu.PuschDemodulator(ctx, 52, 4).demodulate_batch(g[None], h[None], n[None], [to_demod(cfg, True)],
                                                               [0])[0].astype(np.int16)
    ok, st = close_mmse(got, want)
    assert ok, st
    assert np.mean(np.sign(got) == np.sign(want)) >= 0.995


# ----------------------------------------------------------------------------------------------------------------------
# 2-4 layer MMSE against the float64 restatement (pusch_demod_cases.mmse_case: informative SNRs, garbage in every slot
# the kernel must not read).
# ----------------------------------------------------------------------------------------------------------------------
GUARD = 64


def run_plan(ctx, prb, slots, demods, grid_index, with_stats=False, executes=1, noise=None):
    """One plan over `slots` [(grid (4, 14, nsc, 2), ch_est (4, 4, 14, nsc, 2), ...)] and one noise-variance row per
    transmission (`noise`, or its slot's), the LLR buffer filled with 77, every transmission at an odd or otherwise
    unaligned llr_offset with at least GUARD bytes of 77 before and after it, which must come back untouched. Returns the transmissions' LLRs (of
    the last execute) and, with_stats, the statistics of every execute; any NaN in a statistics row that has data
    fails."""
    import srsgpu
    import torch
    dev = torch.device("cuda", ctx.device)
    offs, off = [], GUARD
    for i, m in enumerate(demods):
        off += 1 + 2 * (i % 2) if i % 4 != 3 else 2  # alignments 1, 0, 1, 2, ... of the first byte (mod 4)
        offs.append(off)
        off += m.nof_llrs() + GUARD
    arr, offs, _ = srsgpu.make_pusch_demod_configs(demods, grid_index, llr_offsets=offs)
    exts, _keep = srsgpu.make_crb_mask_exts(demods, prb)
    plan = srsgpu.PuschDemodulatorPlan(ctx, arr, prb, 4, exts)
    flat = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t).reshape(-1).copy()).to(dev)  # noqa: E731
    g = flat(np.stack([s[0] for s in slots]).astype(np.uint16).view(np.int32), np.int32)
    h = flat(np.stack([s[1] for s in slots]).astype(np.uint16).view(np.int32), np.int32)
    nv = flat(np.stack(noise if noise is not None else [slots[gi][2] for gi in grid_index]), np.float32)
    out = torch.full((off,), 77, dtype=torch.int8, device=dev)
    stats = []
    for _ in range(executes):
        st = torch.full((len(demods) * srsgpu.DEMOD_STATS,), 55.0, dtype=torch.float32, device=dev) \
            if with_stats else None
        plan.execute(g, h, nv, out, d_stats=st)
        torch.cuda.synchronize(dev)
        if with_stats:
            stats.append(st.cpu().numpy().reshape(len(demods), 15, 2))
    n = [plan.nof_llrs(i) for i in range(len(demods))]
    plan.close()
    o = out.cpu().numpy()
    keep = np.ones(off, bool)
    for a, k, m in zip(offs, n, demods):
        assert k == m.nof_llrs()
        keep[a:a + k] = False
    assert (o[keep] == 77).all(), "a store outside a transmission's LLRs"
    for s in stats:
        assert not np.isnan(s[~np.isnan(s[:, :, 1])]).any(), "NaN in the statistics of a symbol with data"
        assert not np.isnan(s[:, 14]).any()
    llrs = [o[a:a + k].copy() for a, k in zip(offs, n)]
    return (llrs, stats) if with_stats else llrs


def restated(case, mmse=True):
    cfg, g, h, nv, crb = case
    return D.demodulate_ex(cfg, from_bf16(g), from_bf16(h), nv, mmse=mmse, crb_mask=crb)


def assert_informative(want, key):
    assert K.informative_share(want) >= 0.6, (key, K.informative_share(want))


def demod_of(case, mmse=True):
    d = to_demod(case[0], mmse)
    d.crb_mask = case[4]
    return d


_singles = {}


def single(ctx, key):
    """(case, restatement's LLRs, kernel's LLRs as a plan of its own) of one instantiation, computed once."""
    if key not in _singles:
        L, P, qm = key
        case = K.mmse_single_case(L, P, qm) if L > 1 else K.mmse_case(np.random.default_rng(sum(key)), 6, L, P, qm,
                                                                      garbage="nan")
        want, _ = restated(case)
        if L > 1:
            assert_informative(want, key)
        got = run_plan(ctx, 6, [case[1:4]], [demod_of(case)], [0])[0]
        _singles[key] = (case, want, got)
    return _singles[key]


def test_pusch_demod_mmse_cases_cover_every_instantiation():
    """Every (layers, modulation) pair of demod_res<L, QM>, ports below four, and the byte-store path (L Qm % 4 != 0)
    occur among the single-plan cases."""
    assert {(L, qm) for L, _, qm in K.MMSE_SINGLES} == {(L, qm) for L in (2, 3, 4) for qm in (2, 4, 6, 8)}
    assert {(L, P) for L, P, _ in K.MMSE_SINGLES} == {(2, 2), (2, 3), (2, 4), (3, 3), (3, 4), (4, 4)}
    assert {L * qm for L, _, qm in K.MMSE_SINGLES if (L * qm) % 4} == {6, 18}
    for L, P, qm in K.MMSE_SINGLES:
        cfg = K.mmse_single_case(L, P, qm)[0]
        assert cfg["start_symbol"] == 0 and cfg["nof_symbols"] == 14 and to_demod(cfg).nof_llrs() >= 600 * L * qm


@pytest.mark.parametrize("L,P,qm", K.MMSE_SINGLES)
def test_pusch_demod_mmse_every_instantiation(ctx, L, P, qm):
    """(a) Each (layers, ports, modulation) under MMSE as a plan of its own: garbage (bf16 NaN or 1e30) in the unused
    ports, layers and noise variances, guard bytes around the LLRs, an unaligned llr_offset."""
    case, want, got = single(ctx, (L, P, qm))  # asserts the informative share before it runs the kernel
    ok, st = close_mmse(got, want)
    assert ok, st


def test_pusch_demod_mmse_mixed_plan(ctx):
    """(b) The same 24 transmissions and four one-layer ones (L Qm = 2 and 6) in ONE plan: its chunks of 8 x 32 = 256
    words begin and end inside an RE for L Qm in {6, 12, 18, 24}. Every transmission equals its single-plan LLRs bit
    for bit and meets the tolerance (one layer: the reference paths' close_ref)."""
    keys = K.MMSE_SINGLES + K.ONE_LAYER_EXTRAS
    assert {L * qm for L, _, qm in keys} >= {2, 6, 12, 18, 24, 32}
    items = [single(ctx, k) for k in keys]
    got = run_plan(ctx, 6, [it[0][1:4] for it in items], [demod_of(it[0]) for it in items], list(range(len(items))))
    for key, (case, want, alone), llr in zip(keys, items, got):
        assert np.array_equal(llr, alone), key
        ok, st = close_mmse(llr, want) if key[0] > 1 else close_ref(llr, want)
        assert ok, (key, st)


def test_pusch_demod_zf_request_with_three_layers_is_mmse(ctx):
    """(c) EQ_ZF with 3 or 4 layers is MMSE (the plan's rule): byte for byte the EQ_MMSE request's LLRs. With 2 layers
    the two equalizers differ, in the restatement too, and the kernel follows the restatement in each."""
    for L in (3, 4):
        case, want, got = single(ctx, (L, 4, 4))
        zf = run_plan(ctx, 6, [case[1:4]], [demod_of(case, mmse=False)], [0])[0]
        assert np.array_equal(zf, got), L
    case, want, got = single(ctx, (2, 4, 4))
    want_zf, _ = restated(case, mmse=False)
    zf = run_plan(ctx, 6, [case[1:4]], [demod_of(case, mmse=False)], [0])[0]
    assert np.mean(want_zf != want) > 0.05 and np.mean(zf != got) > 0.05
    ok, st = close(zf, want_zf)
    assert ok, st
    ok, st = close_mmse(got, want)
    assert ok, st


def test_pusch_demod_mmse_crb_mask(ctx):
    """(d) 2-4 layers over scattered CRBs of a 24-PRB grid under MMSE, in one plan, with the statistics' rows present
    exactly where the restatement has data."""
    cases = list(K.mmse_crb_cases())
    got, stats = run_plan(ctx, 24, [c[1:4] for _, c in cases], [demod_of(c) for _, c in cases],
                          list(range(len(cases))), with_stats=True)
    for (key, case), llr, st in zip(cases, got, stats[0]):
        want, wst = restated(case)
        assert_informative(want, key)
        ok, s = close_mmse(llr, want)
        assert ok, (key, s)
        assert np.array_equal(np.isnan(st), np.isnan(wst)), key


def test_pusch_demod_mmse_stats(ctx):
    """(e) Post-equalisation SINR and EVM with 2-4 layers x two modulations on bounded-condition channels, executed
    twice on one plan (the accumulators reset), at check_stats' multi-layer limits."""
    cases = list(K.mmse_stats_cases())
    assert {c[0]["nof_layers"] for _, c in cases} == {2, 3, 4}
    got, stats = run_plan(ctx, 6, [c[1:4] for _, c in cases], [demod_of(c) for _, c in cases],
                          list(range(len(cases))), with_stats=True, executes=2)
    for i, (key, case) in enumerate(cases):
        want, wst = restated(case)
        assert_informative(want, key)
        ok, s = close_mmse(got[i], want)
        assert ok, (key, s)
        for st in stats:
            print(key, "SINR dB", st[i, 14, 0], wst[14, 0], "EVM", st[i, 14, 1], wst[14, 1])
            check_stats(st[i], wst, key[0])


@pytest.mark.parametrize("L,P", [(2, 2), (3, 4), (4, 4)])
def test_pusch_demod_mmse_degenerate(ctx, L, P):
    """(f) The validity rule on the kernel. noise_var = 0: every LLR is 0. A layer whose channel column is zero on
    every third subcarrier: its LLRs are 0 there, every other LLR is within tolerance of the restatement, and the
    statistics have no NaN. (The dead layer's SINR is not compared: its g = 1 - nv / nv is zero up to rounding, and
    whether its variance is huge or infinite is the rounding's choice, in float32 as in float64.)"""
    dead = L - 2
    case = K.mmse_case(np.random.default_rng(700 + L + P), 6, L, P, 4, dead_layer=dead, garbage="big")
    cfg = case[0]
    zero = np.zeros(4, np.float32)
    zero[P:] = case[3][P:]
    got, stats = run_plan(ctx, 6, [case[1:4], (case[1], case[2], zero)], [demod_of(case)] * 2, [0, 1],
                          with_stats=True)
    assert got[1].size == got[0].size and not got[1].any()
    want, _ = restated(case)
    res = D.data_res(0, 14, cfg["dmrs_symbol_mask"], cfg["dmrs_type2"], cfg["nof_cdm_groups_without_data"],
                     cfg["rb_start"], cfg["nof_rb"])
    is_dead = np.array([k % 3 == 0 for _, k in res])
    per = got[0].reshape(len(res), L, 4)
    assert is_dead.any() and not per[is_dead, dead].any()
    assert_informative(want.reshape(per.shape)[~is_dead], (L, P))
    ok, st = close_mmse(got[0], want)
    assert ok, st


def plan_chunk_threads(demods):
    """The plan's rule for the lanes of a chunk workgroup, restated (capi_pusch_demod.cpp): a plan of fewer than
    256 x 256 codeword words takes 256; otherwise chunks hold 8192 LLRs, and at most 384 REs in the largest take 64
    lanes, at most 768 take 128."""
    if sum((d.nof_llrs() + 31) // 32 for d in demods) < 256 * 256:
        return 256
    most = max(-(-8192 // (d.nof_tx_layers * d.modulation_order)) for d in demods)
    return 64 if most <= 384 else (128 if most <= 768 else 256)


@pytest.mark.parametrize("threads", [64, 128])
def test_pusch_demod_mmse_large_plan(ctx, threads):
    """(g) Off the small-plan path: the smallest cycle through a few distinct 52-PRB transmissions (shared grid_index)
    that reaches 65 536 codeword words, once with L Qm in {24, 32} (64 lanes per chunk) and once in {12, 16, 18}
    (128): the instantiations of the bench's mimo4 profile. Repeats equal their first occurrence bit for bit."""
    keys = K.MMSE_WIDE_64 if threads == 64 else K.MMSE_WIDE_128
    cases = [K.mmse_wide_case(*k) for k in keys]
    assert {k[0] * k[2] for k in keys} == ({24, 32} if threads == 64 else {12, 16, 18})
    demods, index = [], []
    while sum((d.nof_llrs() + 31) // 32 for d in demods) < 256 * 256:
        index.append(len(demods) % len(cases))
        demods.append(demod_of(cases[index[-1]]))
    assert plan_chunk_threads(demods) == threads and plan_chunk_threads(demods[:-1]) == 256
    got = run_plan(ctx, 52, [c[1:4] for c in cases], demods, index)
    for i, (key, case) in enumerate(zip(keys, cases)):
        want, _ = restated(case)
        assert_informative(want, key)
        ok, st = close_mmse(got[i], want)
        assert ok, (key, st)
    for i, gi in enumerate(index):
        assert np.array_equal(got[i], got[gi]), i


def test_pusch_demod_rejects_invalid(ctx):
    import srsgpu
    rng = np.random.default_rng(1)
    cfg, *_ = random_case(rng, 24, nof_layers=2, nof_rx_ports=2)
    for bad in [dict(nof_rx_ports=3), dict(qm=3), dict(rb_start=20, nof_rb=10), dict(nof_layers=3, nof_rx_ports=2)]:
        arr, _, _ = srsgpu.make_pusch_demod_configs([to_demod(dict(cfg, **bad))], [0])
        with pytest.raises(srsgpu.SrsGpuError):
            srsgpu.PuschDemodulatorPlan(ctx, arr, 24, 4)


def test_pusch_demod_rejects_estimates_past_32bit_byte_offsets(ctx):
    """The kernels address a slot's estimates (4 layers x 4 ports x 14 x nsc elements of 4 bytes) by unsigned 32-bit
    byte offsets: the plan takes the last grid_index whose estimates end within 4 GiB and refuses the next (plan
    creation only: no buffer of that size is made)."""
    import srsgpu
    cfg, *_ = random_case(np.random.default_rng(2), 273, nof_layers=1, nof_rx_ports=4)
    slot_bytes = 4 * 4 * 14 * 12 * 273 * 4
    last = (1 << 32) // slot_bytes - 1
    arr, _, _ = srsgpu.make_pusch_demod_configs([to_demod(cfg)], [last])
    srsgpu.PuschDemodulatorPlan(ctx, arr, 273, 4).close()
    arr, _, _ = srsgpu.make_pusch_demod_configs([to_demod(cfg)], [last + 1])
    with pytest.raises(srsgpu.SrsGpuError):
        srsgpu.PuschDemodulatorPlan(ctx, arr, 273, 4)


def to_demod_general(cfg, crb=None, tp=False):
    d = to_demod(cfg)
    d.crb_mask, d.transform_precoding = crb, int(tp)
    return d


def check_stats(got, want, nof_layers):
    """Statistics parity: the same rows present (NaN = no data), EVM per symbol 1e-2 relative and total 5e-3, SINR
    5e-3 dB with one layer and 0.1 dB with two (near-singular 2 x 2 REs dominate the mean; see test_golden.py)."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[:14, 1][ok[:14, 1]], want[:14, 1][ok[:14, 1]], rtol=1e-2)
    if ok[14, 1]:
        np.testing.assert_allclose(got[14, 1], want[14, 1], rtol=5e-3)
    np.testing.assert_allclose(got[:, 0][ok[:, 0]], want[:, 0][ok[:, 0]], atol=5e-3 if nof_layers == 1 else 0.1)


def test_pusch_demod_general_golden(ctx):
    """CRB masks, transform precoding and the post-equalization SINR / EVM against the reference's LLRs and statistics
    (tests/golden/pusch_demod_general.npz), every case in ONE plan; executed twice (the plan's accumulators reset)."""
    import srsgpu
    cases = list(G.pusch_demod_general_cases())
    grids, hs, nvs, demods = [], [], [], []
    for cfg, tp, crb, grid, H, nv, _, _ in cases:
        g, h, n = pad_slot(grid, H, nv)
        grids.append(g)
        hs.append(h)
        nvs.append(n)
        demods.append(to_demod_general(cfg, crb, tp))
    dem = srsgpu.PuschDemodulator(ctx, 32, 4)
    for _ in range(2):
        got, stats = dem.demodulate_batch(np.stack(grids), np.stack(hs), np.stack(nvs), demods,
                                          list(range(len(cases))), with_stats=True)
        for i, (cfg, tp, crb, _, _, _, want, wstats) in enumerate(cases):
            ok, st = close(got[i], want)
            assert got[i].size == want.size and ok, (cfg, tp, st)
            check_stats(stats[i], wstats, cfg["nof_layers"])


def test_pusch_demod_general_random_vs_oracle(ctx):
    """48 random transmissions (CRB masks or contiguous, with and without transform precoding, 1..273 PRB) in ONE
    plan over 273-PRB grids, against the restatement (LLRs within one step on < 5 %, statistics as above)."""
    import srsgpu
    from pusch_demod_cases import random_general_case
    rng = np.random.default_rng(77)
    items = []
    for i in range(48):
        tp = i % 3 == 0
        items.append((random_general_case(rng, 273, transform_precoding=tp, mask=i % 2 == 0), tp))
    grids, hs, nvs, demods = [], [], [], []
    for (cfg, grid, H, nv, crb), tp in items:
        g, h, n = pad_slot(grid, H, nv)
        grids.append(g)
        hs.append(h)
        nvs.append(n)
        demods.append(to_demod_general(cfg, crb, tp))
    got, stats = srsgpu.PuschDemodulator(ctx, 273, 4).demodulate_batch(np.stack(grids), np.stack(hs), np.stack(nvs),
                                                                        demods, list(range(len(items))),
                                                                        with_stats=True)
    for i, ((cfg, grid, H, nv, crb), tp) in enumerate(items):
        want, wstats = D.demodulate_ex(cfg, from_bf16(grid), from_bf16(H), nv, crb_mask=crb, transform_precoding=tp)
        ok, st = close(got[i], want)
        assert got[i].size == want.size and ok, (cfg, tp, st)
        check_stats(stats[i], wstats, cfg["nof_layers"])


def test_pusch_demod_general_rejects_invalid(ctx):
    """Transform precoding with two layers or a PRB count that is not 2^a 3^b 5^c, and reserved patterns, fail at plan
    creation (the reference asserts, pusch_demodulator_impl.cpp:347, transform_precoder_dft_impl.cpp)."""
    import srsgpu
    rng = np.random.default_rng(5)
    from pusch_demod_cases import random_case
    cfg, _, _, _ = random_case(rng, 24, nof_layers=2, nof_rx_ports=2)
    cfg.update(rb_start=0, nof_rb=4, dmrs_type2=0, nof_cdm_groups_without_data=2)
    bad = [to_demod_general(cfg, tp=True)]
    cfg1 = dict(cfg, nof_layers=1, nof_rb=7)
    bad.append(to_demod_general(cfg1, tp=True))
    for d in bad:
        arr, _, _ = srsgpu.make_pusch_demod_configs([d], [0])
        with pytest.raises(srsgpu.SrsGpuError):
            srsgpu.PuschDemodulatorPlan(ctx, arr, 24, 4)
    d = to_demod_general(dict(cfg1, nof_rb=8), crb=np.ones(24, np.uint8))
    arr, _, _ = srsgpu.make_pusch_demod_configs([d], [0])
    exts, _keep = srsgpu.make_crb_mask_exts([d], 24)
    exts[0].nof_reserved = 1
    with pytest.raises(srsgpu.SrsGpuError):
        srsgpu.PuschDemodulatorPlan(ctx, arr, 24, 4, exts)


# ----------------------------------------------------------------------------------------------------------------------
# The reference's own paths against the restatement at the rounding tolerance: ZF 1 x N, ZF 2 x N, one-layer MMSE
# (pusch_demod_cases.REF_SINGLES and ref_*_case: informative SNRs, garbage in every slot the kernel must not read).
# ----------------------------------------------------------------------------------------------------------------------
def close_ref(got, want):
    """The reference paths' tolerance against the restatement: every LLR equal or one step apart, fewer than
    REF_PATHS_SHARE_BOUND differing."""
    if got.size != want.size:
        return False, (got.size, want.size)
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    print("max step", int(d.max()), "share differing", float(np.mean(d > 0)), "of", d.size)
    return d.max() <= 1 and np.mean(d > 0) < K.REF_PATHS_SHARE_BOUND, (int(d.max()), float(np.mean(d > 0)))


_ref_singles = {}


def ref_single(ctx, key):
    """(case, restatement's LLRs, kernel's LLRs as an EQ_ZF plan of its own) of one instantiation, computed once."""
    if key not in _ref_singles:
        case = K.ref_single_case(*key)
        want, _ = restated(case, mmse=False)
        assert_informative(want, key)
        got = run_plan(ctx, 6, [case[1:4]], [demod_of(case, mmse=False)], [0])[0]
        _ref_singles[key] = (case, want, got)
    return _ref_singles[key]


def test_pusch_demod_ref_cases_cover_every_instantiation():
    """demod_res<1, QM> and the ZF demod_res<2, QM> for every QM, every port count the reference's equalisers take,
    and the byte-store path (L Qm % 4 != 0) occur among the single-plan cases."""
    assert len(K.REF_SINGLES) == 24
    assert {(L, qm) for L, _, qm in K.REF_SINGLES} == {(L, qm) for L in (1, 2) for qm in (2, 4, 6, 8)}
    assert {(L, P) for L, P, _ in K.REF_SINGLES} == {(1, 1), (1, 2), (1, 3), (1, 4), (2, 2), (2, 4)}
    assert {(L, P, qm) for L, P, qm in K.REF_SINGLES} == {(L, P, qm) for L, P in K.REF_LP for qm in (2, 4, 6, 8)}
    assert {L * qm for L, _, qm in K.REF_SINGLES if (L * qm) % 4} == {2, 6}
    for L, P, qm in K.REF_SINGLES:
        cfg = K.ref_single_case(L, P, qm)[0]
        assert cfg["start_symbol"] == 0 and cfg["nof_symbols"] == 14 and 4 <= cfg["nof_rb"] <= 6
        assert to_demod(cfg).nof_llrs() >= 600 * L * qm


@pytest.mark.parametrize("L,P,qm", K.REF_SINGLES)
def test_pusch_demod_ref_every_instantiation(ctx, L, P, qm):
    """Each (layers, ports, modulation) under EQ_ZF as a plan of its own: garbage (bf16 NaN or 1e30) in the unused
    ports, layers and noise variances, guard bytes around the LLRs, an unaligned llr_offset."""
    case, want, got = ref_single(ctx, (L, P, qm))  # asserts the informative share before it runs the kernel
    ok, st = close_ref(got, want)
    assert ok, st


def test_pusch_demod_ref_one_layer_mmse_is_zf(ctx):
    """EQ_MMSE with one layer is ZF 1 x N (channel_equalizer_generic_impl.cpp:343): byte for byte the EQ_ZF LLRs, for
    every port count and modulation, in one plan."""
    keys = [k for k in K.REF_SINGLES if k[0] == 1]
    assert len(keys) == 16
    items = [ref_single(ctx, k) for k in keys]
    got = run_plan(ctx, 6, [it[0][1:4] for it in items], [demod_of(it[0], mmse=True) for it in items],
                   list(range(len(items))))
    for key, (case, want, alone), llr in zip(keys, items, got):
        assert np.array_equal(llr, alone), key


def test_pusch_demod_ref_mixed_plan(ctx):
    """The same 24 transmissions in ONE plan: its chunks of 8 x 16 = 128 words begin and end inside an RE for L Qm in
    {6, 12}. Every transmission equals its single-plan LLRs bit for bit (and so meets the tolerance)."""
    keys = K.REF_SINGLES
    assert {L * qm for L, _, qm in keys} == {2, 4, 6, 8, 12, 16}
    items = [ref_single(ctx, k) for k in keys]
    assert all(4096 % (k[0] * k[2]) for k in keys if k[0] * k[2] in (6, 12))
    got = run_plan(ctx, 6, [it[0][1:4] for it in items], [demod_of(it[0], mmse=False) for it in items],
                   list(range(len(items))))
    for key, (case, want, alone), llr in zip(keys, items, got):
        assert np.array_equal(llr, alone), key
        ok, st = close_ref(llr, want)
        assert ok, (key, st)


def plan_words(demods):
    return sum((d.nof_llrs() + 31) // 32 for d in demods)


@pytest.mark.parametrize("threads", [256, 128])
def test_pusch_demod_ref_large_plan(ctx, threads):
    """Off the small-plan path: the smallest cycle through a few distinct 52-PRB transmissions (shared grid_index) that
    reaches 65 536 codeword words, once with one layer and L Qm in {2, 4, 6, 8} (chunks of 1 024 to 4 096 REs on 256
    lanes, four or more REs per lane: the shape of the bench's ref profile) and once with two-layer ZF at 64QAM and
    256QAM (chunks of at most 683 REs: 128 lanes). Repeats equal their first occurrence bit for bit."""
    keys = K.REF_WIDE_256 if threads == 256 else K.REF_WIDE_128
    cases = [K.ref_wide_case(*k) for k in keys]
    assert {k[0] * k[2] for k in keys} == ({2, 4, 6, 8} if threads == 256 else {12, 16})
    assert {k[0] for k in keys} == ({1} if threads == 256 else {2})
    demods, index = [], []
    while plan_words(demods) < 256 * 256:
        index.append(len(demods) % len(cases))
        demods.append(demod_of(cases[index[-1]], mmse=False))
    assert plan_words(demods) >= 256 * 256 > plan_words(demods[:-1])
    assert plan_chunk_threads(demods) == threads and plan_chunk_threads(demods[:-1]) == 256
    if threads == 256:
        assert min(-(-8192 // (d.nof_tx_layers * d.modulation_order)) for d in demods) >= 4 * 256
    got = run_plan(ctx, 52, [c[1:4] for c in cases], demods, index)
    for i, (key, case) in enumerate(zip(keys, cases)):
        want, _ = restated(case, mmse=False)
        assert_informative(want, key)
        ok, st = close_ref(got[i], want)
        assert ok, (key, st)
    for i, gi in enumerate(index):
        assert np.array_equal(got[i], got[gi]), i


def test_pusch_demod_ref_degenerate_noise(ctx):
    """ZF 1 x 4 with a noise variance of zero on one port: that port is skipped (the LLRs are those of the restatement,
    which differ from the four-port ones), and with zero on all ports: every LLR is 0. No NaN in the statistics."""
    case = K.mmse_case(np.random.default_rng(810), 6, 1, 4, 4, garbage="big")
    cfg, g, h, nv, _ = case
    one = nv.copy()
    one[2] = 0
    zero = np.zeros(4, np.float32)
    got, stats = run_plan(ctx, 6, [(g, h, one), (g, h, zero)], [demod_of(case, mmse=False)] * 2, [0, 1],
                          with_stats=True)
    want, wst = restated((cfg, g, h, one, None), mmse=False)
    assert_informative(want, "one port without noise variance")
    assert np.mean(want != restated(case, mmse=False)[0]) > 0.05
    ok, st = close_ref(got[0], want)
    assert ok, st
    check_stats(stats[0][0], wst, 1)
    assert got[1].size == want.size and not got[1].any()
    assert np.isinf(stats[0][1][14, 0])


def test_pusch_demod_ref_degenerate_dead_subcarriers(ctx):
    """ZF 1 x 1 with a zero channel on every third subcarrier: LLRs 0 there (infinite variance), every other LLR within
    tolerance of the restatement, no NaN in the statistics."""
    case = K.mmse_case(np.random.default_rng(820), 6, 1, 1, 6, dead_layer=0, garbage="nan")
    cfg = case[0]
    got, stats = run_plan(ctx, 6, [case[1:4]], [demod_of(case, mmse=False)], [0], with_stats=True)
    want, wst = restated(case, mmse=False)
    res = D.data_res(0, 14, cfg["dmrs_symbol_mask"], cfg["dmrs_type2"], cfg["nof_cdm_groups_without_data"],
                     cfg["rb_start"], cfg["nof_rb"])
    is_dead = np.array([k % 3 == 0 for _, k in res])
    per = got[0].reshape(len(res), 6)
    assert is_dead.any() and not per[is_dead].any()
    assert_informative(want.reshape(per.shape)[~is_dead], "dead subcarriers")
    ok, st = close_ref(got[0], want)
    assert ok, st
    check_stats(stats[0][0], wst, 1)


@pytest.mark.parametrize("P", [2, 4])
def test_pusch_demod_ref_degenerate_equal_columns(ctx, P):
    """ZF 2 x N with the two channel columns equal on every third subcarrier: the Gram determinant is not a normal
    number there, so both layers' LLRs are 0; every other LLR within tolerance of the restatement, no NaN in the
    statistics."""
    cfg, g, h, nv, _ = K.mmse_case(np.random.default_rng(830 + P), 6, 2, P, 4, garbage="big")
    h = h.copy()
    h[1, :P, :, ::3] = h[0, :P, :, ::3]
    case = (cfg, g, h, nv, None)
    got, stats = run_plan(ctx, 6, [case[1:4]], [demod_of(case, mmse=False)], [0], with_stats=True)
    want, wst = restated(case, mmse=False)
    res = D.data_res(0, 14, cfg["dmrs_symbol_mask"], cfg["dmrs_type2"], cfg["nof_cdm_groups_without_data"],
                     cfg["rb_start"], cfg["nof_rb"])
    is_dead = np.array([k % 3 == 0 for _, k in res])
    per = got[0].reshape(len(res), 2, 4)
    assert is_dead.any() and not want.reshape(per.shape)[is_dead].any() and not per[is_dead].any()
    assert_informative(want.reshape(per.shape)[~is_dead], ("equal columns", P))
    ok, st = close_ref(got[0], want)
    assert ok, st
    assert np.array_equal(np.isnan(stats[0][0]), np.isnan(wst))


# ----------------------------------------------------------------------------------------------------------------------
# Transform precoding against the restatement at the rounding tolerance, on every size the inverse DFT takes.
# ----------------------------------------------------------------------------------------------------------------------
_tp_slots = {}


def tp_restated(case):
    """D.demodulate_ex with transform precoding; the bf16 conversion of a shared slot is done once."""
    cfg, g, h, nv, crb = case
    if id(g) not in _tp_slots:
        _tp_slots[id(g)] = (g, from_bf16(g), from_bf16(h))
    _, gc, hc = _tp_slots[id(g)]
    return D.demodulate_ex(cfg, gc, hc, nv, crb_mask=crb, transform_precoding=True)


def test_pusch_demod_tp_every_size(ctx):
    """All 53 valid M_RB <= 273 (and every modulation at M_RB = 1 and 270) in ONE plan over shared 273-PRB slots
    (pusch_demod_cases.tp_size_plan): one data symbol each, 1-4 ports with bf16 NaN in the unused ones, guard bytes
    around the LLRs (the kernel stores bytes straight to global memory), unaligned llr_offsets; executed twice with
    the statistics (the accumulators reset). The cases cover every size and every radix sequence of the kernel's
    Stockham passes."""
    keys, cases, index, slots = K.tp_size_plan()
    sizes = K.valid_tp_prbs(273)
    assert len(sizes) == 53 and sorted({n for n, _, _ in keys}) == sizes
    assert {K.tp_radix_sequence(12 * c[0]["nof_rb"]) for c in cases} == {K.tp_radix_sequence(12 * n) for n in sizes}
    assert K.tp_radix_sequence(12 * 270) == (4, 2, 3, 3, 3, 3, 5)
    assert {r for c in cases for r in K.tp_radix_sequence(12 * c[0]["nof_rb"])} == {4, 2, 3, 5}
    assert {(n, qm) for n, qm, _ in keys} >= {(n, qm) for n in (1, 270) for qm in (2, 4, 6, 8)}
    assert {qm for _, qm, _ in keys} == {2, 4, 6, 8} and {P for _, _, P in keys} == {1, 2, 3, 4}
    where = [(gi, c[0]["start_symbol"], c[0]["rb_start"]) for gi, c in zip(index, cases)]
    assert len(set(where)) == len(where) and len(slots) <= 6
    demods = [to_demod_general(c[0], None, True) for c in cases]
    got, stats = run_plan(ctx, 273, [s + (None,) for s in slots], demods, index, with_stats=True, executes=2,
                          noise=[c[3] for c in cases])
    failed = []
    for key, case, llr, st0, st1 in zip(keys, cases, got, stats[0], stats[1]):
        want, wst = tp_restated(case)
        assert_informative(want, key)
        print(key, end=" ")
        ok, s = close_ref(llr, want)
        if not ok:
            failed.append((key, s))
        check_stats(st0, wst, 1)
        check_stats(st1, wst, 1)
    assert not failed, failed


def test_pusch_demod_tp_extras(ctx):
    """Transform precoding over scattered CRB masks (M_RB = 5, 27, 100), over 14 symbols with two DM-RS symbols
    (M_RB = 48), with dead subcarriers (classes TP_INF and TP_VALID in one symbol), with a zero noise variance (no
    valid variance: every LLR 0) and with variances that underflow to zero (class TP_OTHER next to TP_VALID), in one
    plan with the statistics."""
    items = list(K.tp_extra_cases())
    assert [n for n, _ in items] == ["crb5", "crb27", "crb100", "multi", "dead", "zero", "other"]
    demods = [to_demod_general(c[0], c[4], True) for _, c in items]
    got, stats = run_plan(ctx, 106, [c[1:4] for _, c in items], demods, list(range(len(items))), with_stats=True)
    for (name, case), llr, st in zip(items, got, stats[0]):
        want, wst = tp_restated(case)
        if name == "zero":
            assert llr.size == want.size and not want.any() and not llr.any()
        elif name == "other":
            per = want.reshape(-1, 12 * case[0]["nof_rb"], 2)
            assert not per[:, ::3].any() and np.mean(np.abs(per[:, 1::3]) == 120) > 0.9
        else:
            assert_informative(want, name)
        print(name, end=" ")
        ok, s = close_ref(llr, want)
        assert ok, (name, s)
        check_stats(st, wst, 1)
