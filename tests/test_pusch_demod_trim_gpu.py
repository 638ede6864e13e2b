"""The PUSCH demodulator's trimmed paths against its general ones and against the restatement.

The chunked kernel finds an RE's OFDM symbol by a closed form where the host has proved that every symbol with data
carries the same number of REs and no DM-RS symbol carries data (capi_pusch_demod.cpp demod_symbol_form), and
descrambles and packs four LLRs at a time where layers x Qm is a multiple of 4. SRSGPU_OPTION_DEMOD_GENERAL_PATHS
forces the search through the cumulative RE counts and LLR-by-LLR packing for every transmission of a plan.

Every case runs in one plan created twice, once with the option at its default and once forced: the two outputs must
be equal byte for byte, the bytes around every transmission untouched, and both must meet the restatement
(oracle/pusch_demod_oracle.py demodulate_ex) at the reference paths' tolerance (test_pusch_demodulator_gpu.close_ref:
every LLR equal or one step apart, fewer than pusch_demod_cases.REF_PATHS_SHARE_BOUND differing). The plan reports per
transmission which form it chose (srsgpu_pusch_demodulator_plan_symbol_closed_form); the cases pin that too, so that a
layout the closed form cannot describe is seen to be refused, not merely to give the right bytes."""
import numpy as np
import pytest

import pusch_demod_cases as K
from pusch_demod_cases import from_bf16
import pusch_demod_oracle as D
from test_pusch_demodulator_gpu import GUARD, close_ref, demod_of

pytestmark = pytest.mark.gpu

GRID_PRB = 6
POS1 = (1 << 2) | (1 << 11)  # two DM-RS symbols, as the bench's slots
NO_DATA = dict(dmrs_type2=0, nof_cdm_groups_without_data=2)  # type 1, both CDM groups: DM-RS symbols carry no data


def _case(seed, L, P, qm, nof_rb, scattered=False, snr_db=None, **cfg):
    """pusch_demod_cases.mmse_case (data on every RE of the slot) with the allocation fields of `cfg` set afterwards:
    the demodulator and the restatement read the REs the changed configuration names."""
    case = K.mmse_case(np.random.default_rng(seed), GRID_PRB, L, P, qm, nof_rb=nof_rb, scattered=scattered,
                       snr_db=snr_db, garbage="nan")
    case[0].update(dict(dmrs_symbol_mask=POS1, **NO_DATA))
    case[0].update(cfg)
    return case


def _cases():
    """name -> (case, closed form expected)."""
    out = {}
    seed = 9000
    # 1 and 3 PRB x one and two layers x every modulation: L Qm = 2 and 6 take the byte stores, 12 words that straddle
    # the layers, the others whole words per layer.
    for nrb in (1, 3):
        for L in (1, 2):
            for qm in (2, 4, 6, 8):
                seed += 1
                out[f"prb{nrb}-L{L}-qm{qm}"] = (_case(seed, L, 2, qm, nrb), True)
    # DM-RS symbols that carry data (one CDM group without data: 6 REs per PRB there, 12 elsewhere): refused.
    out["dmrs-data-L1-qm4"] = (_case(9101, 1, 2, 4, 3, nof_cdm_groups_without_data=1), False)
    out["dmrs-data-L2-qm6"] = (_case(9102, 2, 2, 6, 3, nof_cdm_groups_without_data=1), False)
    out["dmrs-data-type2-L2-qm8"] = (_case(9103, 2, 4, 8, 2, dmrs_type2=1, nof_cdm_groups_without_data=2), False)
    # Every allocated symbol a DM-RS symbol with data: equal counts, yet not the 12-per-PRB layout: refused.
    out["all-dmrs-L1-qm4"] = (_case(9104, 1, 1, 4, 3, start_symbol=2, nof_symbols=2, dmrs_symbol_mask=0b1100,
                                    nof_cdm_groups_without_data=1), False)
    # CRB-mask allocations (scattered CRBs), closed form and search.
    out["crb-mask-L1-qm8"] = (_case(9111, 1, 2, 8, 3, scattered=True), True)
    out["crb-mask-L2-qm4"] = (_case(9112, 2, 2, 4, 4, scattered=True), True)
    out["crb-mask-dmrs-data-L2-qm2"] = (_case(9113, 2, 2, 2, 3, scattered=True, nof_cdm_groups_without_data=1), False)
    # Start symbols above 0: a DM-RS symbol first (the first data symbol is 3), one in front of the allocation, and
    # an allocation that ends on one.
    out["start2-L1-qm8"] = (_case(9121, 1, 2, 8, 3, start_symbol=2, nof_symbols=10), True)
    out["start3-L2-qm4"] = (_case(9122, 2, 2, 4, 1, start_symbol=3, nof_symbols=11), True)
    out["start1-end11-L1-qm4"] = (_case(9123, 1, 1, 4, 2, start_symbol=1, nof_symbols=11), True)
    out["start5-one-symbol-L1-qm2"] = (_case(9124, 1, 1, 2, 1, start_symbol=5, nof_symbols=1), True)
    # Runs of symbols without data: a double-symbol DM-RS (one run of two), three runs (more than the form holds).
    out["double-dmrs-L2-qm8"] = (_case(9131, 2, 2, 8, 3, dmrs_symbol_mask=(3 << 2) | (3 << 10)), True)
    out["three-runs-L1-qm8"] = (_case(9132, 1, 2, 8, 3, dmrs_symbol_mask=(1 << 2) | (1 << 6) | (1 << 10)), False)
    out["no-dmrs-L1-qm6"] = (_case(9133, 1, 2, 6, 3, dmrs_symbol_mask=0), True)
    # LLRs at +-120 (most of them, at 22 and 40 dB): the negated bytes of -120 and of +120 in the packed words.
    out["saturated-L1-qm4"] = (_case(9141, 1, 2, 4, 3, snr_db=22.0), True)
    out["saturated-L2-qm8"] = (_case(9142, 2, 2, 8, 1, snr_db=40.0), True)
    return out


CASES = _cases()
NAMES = list(CASES)


def _run(ctx, names, forced, with_stats=False):
    """One plan over the named cases (one slot each); transmission i begins at a byte offset of alignment i mod 4, so
    that every alignment occurs, the LLR buffer pre-filled with 77. Returns ({name: LLRs}, {name: closed form})."""
    import srsgpu
    import torch
    dev = torch.device("cuda", ctx.device)
    demods = [demod_of(CASES[n][0], mmse=False) for n in names]
    offs, off = [], GUARD
    for i, m in enumerate(demods):
        off += (i % 4 - off) % 4
        offs.append(off)
        off += m.nof_llrs() + GUARD
    assert {o % 4 for o in offs} == ({0, 1, 2, 3} if len(offs) >= 4 else {o % 4 for o in offs})
    with ctx.options(demod_general_paths=int(forced)):
        arr, offs, _ = srsgpu.make_pusch_demod_configs(demods, list(range(len(names))), llr_offsets=offs)
        exts, _keep = srsgpu.make_crb_mask_exts(demods, GRID_PRB)
        plan = srsgpu.PuschDemodulatorPlan(ctx, arr, GRID_PRB, 4, exts)
    flat = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t).reshape(-1).copy()).to(dev)  # noqa: E731
    g = flat(np.stack([CASES[n][0][1] for n in names]).astype(np.uint16).view(np.int32), np.int32)
    h = flat(np.stack([CASES[n][0][2] for n in names]).astype(np.uint16).view(np.int32), np.int32)
    nv = flat(np.stack([CASES[n][0][3] for n in names]), np.float32)
    out = torch.full((off,), 77, dtype=torch.int8, device=dev)
    st = torch.zeros(len(names) * srsgpu.DEMOD_STATS, dtype=torch.float32, device=dev) if with_stats else None
    plan.execute(g, h, nv, out, d_stats=st)
    torch.cuda.synchronize(dev)
    closed = {n: plan.symbol_closed_form(i) for i, n in enumerate(names)}
    sizes = [plan.nof_llrs(i) for i in range(len(names))]
    plan.close()
    o = out.cpu().numpy()
    keep = np.ones(off, bool)
    for a, k, m in zip(offs, sizes, demods):
        assert k == m.nof_llrs()
        keep[a:a + k] = False
    assert (o[keep] == 77).all(), "a store outside a transmission's LLRs"
    return {n: o[a:a + k].copy() for n, a, k in zip(names, offs, sizes)}, closed


_memo = {}


def results(ctx):
    """(trimmed LLRs, forced LLRs, closed-form flags of both plans, the restatement's LLRs), computed once."""
    if not _memo:
        trim, closed = _run(ctx, NAMES, forced=False)
        gen, closed_gen = _run(ctx, NAMES, forced=True)
        want = {}
        for n in NAMES:
            cfg, g, h, nv, crb = CASES[n][0]
            want[n] = D.demodulate_ex(cfg, from_bf16(g), from_bf16(h), nv, mmse=False, crb_mask=crb)[0]
        _memo.update(trim=trim, gen=gen, closed=closed, closed_gen=closed_gen, want=want)
    return _memo


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


def test_cases_cover_the_paths():
    """What the cases are chosen for: 1 and 3 PRB, every modulation with one and two layers, the byte path (L Qm = 2,
    6), a word that straddles two layers (12), start symbols above 0, CRB masks, refused layouts."""
    cfgs = {n: c[0][0] for n, c in CASES.items()}
    lq = {c["nof_layers"] * c["qm"] for c in cfgs.values()}
    assert {2, 4, 6, 8, 12, 16} <= lq
    assert {(c["nof_rb"], c["nof_layers"], c["qm"]) for c in cfgs.values()} >= {
        (nrb, L, qm) for nrb in (1, 3) for L in (1, 2) for qm in (2, 4, 6, 8)}
    assert any(c["start_symbol"] > 0 for c in cfgs.values())
    assert any(CASES[n][0][4] is not None and CASES[n][1] for n in NAMES)
    assert any(CASES[n][0][4] is not None and not CASES[n][1] for n in NAMES)
    assert sum(not c[1] for c in CASES.values()) >= 5
    assert GUARD % 4 == 0  # _run's offsets then take every alignment


@pytest.mark.parametrize("name", NAMES)
def test_trimmed_equals_general_and_restatement(ctx, name):
    r = results(ctx)
    trim, gen, want = r["trim"][name], r["gen"][name], r["want"][name]
    assert trim.size == want.size and np.array_equal(trim, gen), \
        (name, int(np.count_nonzero(trim != gen)), np.flatnonzero(trim != gen)[:8])
    ok, st = close_ref(trim, want)
    assert ok, (name, st)
    ok, st = close_ref(gen, want)
    assert ok, (name, st)
    assert r["closed"][name] == CASES[name][1], "the closed form of the symbol: chosen / refused"
    assert not r["closed_gen"][name], "the option forces the search"


def test_saturated_cases_hold_both_limits(ctx):
    """The +-120 cases do carry +120, -120 and LLRs in between, before and after descrambling flips half of them."""
    r = results(ctx)
    for name in ("saturated-L1-qm4", "saturated-L2-qm8"):
        v = r["trim"][name]
        assert (v == 120).sum() > v.size // 20 and (v == -120).sum() > v.size // 20 and (np.abs(v) < 120).any(), name
        assert np.abs(v.astype(np.int16)).max() == 120


def test_trimmed_equals_general_with_statistics(ctx):
    """The statistics instantiation (its own kernel) packs the same bytes on both paths."""
    names = ["prb3-L1-qm8", "prb3-L2-qm6", "prb3-L2-qm4", "dmrs-data-L2-qm6", "crb-mask-L2-qm4", "saturated-L2-qm8"]
    trim, _ = _run(ctx, names, forced=False, with_stats=True)
    gen, _ = _run(ctx, names, forced=True, with_stats=True)
    r = results(ctx)
    for n in names:
        assert np.array_equal(trim[n], gen[n]) and np.array_equal(trim[n], r["trim"][n]), n


def test_trimmed_equals_general_large_plan(ctx):
    """Off the small-plan path (65 536 codeword words: chunks of 8 192 LLRs on 128 lanes, the bench's instantiation;
    the forced plan runs 256): a cycle through three 52-PRB two-layer transmissions, byte for byte the forced plan's
    LLRs, the first occurrences against the restatement."""
    from test_pusch_demodulator_gpu import plan_chunk_threads, restated, run_plan
    keys = K.REF_WIDE_128
    cases = [K.ref_wide_case(*k) for k in keys]
    cases[1][0].update(dict(dmrs_symbol_mask=POS1, **NO_DATA))  # the bench's layout: the closed form on 128 lanes
    demods, index = [], []
    while sum((d.nof_llrs() + 31) // 32 for d in demods) < 256 * 256:
        index.append(len(demods) % len(cases))
        demods.append(demod_of(cases[index[-1]], mmse=False))
    assert plan_chunk_threads(demods) == 128
    trim = run_plan(ctx, 52, [c[1:4] for c in cases], demods, index)
    with ctx.options(demod_general_paths=1):
        gen = run_plan(ctx, 52, [c[1:4] for c in cases], demods, index)
    for i, (a, b) in enumerate(zip(trim, gen)):
        assert np.array_equal(a, b), i
    for i, case in enumerate(cases):
        ok, st = close_ref(trim[i], restated(case, mmse=False)[0])
        assert ok, (keys[i], st)
