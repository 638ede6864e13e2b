"""GPU parity of the packed LDPC decoder's code around the min-sum iterations: the fused rate-dematching front end (groups
of four positions, ldpc_decoder_pk.hip soft_put_x4, and its per-byte fallback), the CRC early-stop check, the
hard-decision output (write_hard_bits_pk: one 16-byte LDS read per output byte when Z % 16 == 0) and single-codeblock
transport blocks written by the decoder (SRSGPU_OPTION_DECODER_TB_FOLD).

Every codeblock is compared bit for bit (HARQ soft buffer, iteration count, decoded bits, CRC flag) with the CPU oracle
composition (chain_lib.oracle_pusch_cb_decode) and with the unfused plan (decoder_fused_dematch=0). The shapes are the
small ones at which a path changes: Z % 16 == 0 (all fast paths), Z % 8 == 0 only (Z = 104: groups of four, per-bit hard
decisions), Z % 8 != 0 (per-byte front end), fillers that are / are not multiples of 4 (the latter leave the dword
path), 64QAM (never the dword path). The two-codeblock kernel shares the front end: its lifting sizes (Z = 144..192)
run it with two codeblocks, and with one and an empty slot, per workgroup.

A PUSCH plan hands the decoder whole lifted columns (capi.cpp add_pusch_cb: the input length is rounded up to a
multiple of Z), so for these plans every group of four lies below `full`; where the rate-matched length ends relative
to a group and to a column is varied all the same, because it sets where the HARQ tail zeroing starts and how many
layers run."""
import numpy as np
import pytest

from chain_lib import bits_to_llrs, oracle_pdsch_encode
from decoder_frontend_cases import _case, _check_group, _geometry, _llrs, _payload_llrs, _pick_E
from oracle_lib import BG_K, BG_N_SHORT, Oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


def _visit_index(n, E, qm):
    """Input index of visit n of the symbol-major dematching (bit j of symbol r is visit j R + r): visit n lands on
    position n, or n + F once past the systematic part."""
    R = E // qm
    return (n % R) * qm + n // R


@pytest.mark.parametrize("dec_type,mode", [("avx2", 1), ("generic", 0)])
def test_lifting_sizes_and_modulations(orc, ctx, dec_type, mode):
    """Z = 208, 384, 112 (multiples of 16), 104 (H = 52: groups of four, per-bit hard decisions), 36, 44, 20 (per-byte
    front end), both base graphs, 256QAM with 0 / 4 fillers, and 64QAM: a decodable all-zero, a noise and a decodable
    random-payload codeblock of each (the last with 4 iterations; most of them must decode)."""
    import srsgpu
    rng = np.random.default_rng(1200 + mode)
    cbs, llrs = [], []
    shapes = [(bg, Z, 8, 4 * ((k + bg) & 1)) for k, Z in enumerate((208, 104, 112, 384, 36, 44, 20)) for bg in (1, 2)]
    shapes += [(1, 208, 6, 0), (2, 36, 6, 4)]
    for bg, Z, qm, F in shapes:
        E = _pick_E(bg, Z, qm, F)
        for good in (True, False):
            cbs.append(_case(srsgpu, len(cbs) // 3, good, bg, Z, qm, E, F))
            llrs.append(_llrs(rng, E, good))
        cbs.append(_case(srsgpu, len(cbs) // 3 & 1, True, bg, Z, qm, E, F))
        llrs.append(_payload_llrs(orc, rng, bg, Z, qm, E, F))
    oks = _check_group(orc, ctx, cbs, llrs, 1201, dec_type, mode)
    assert sum(oks[2::3]) >= 12, oks[2::3]


def test_two_codeblock_workgroups(orc, ctx):
    """The fused front end in the two-codeblock kernel (decoder_pairs=1), which shares it with the one-codeblock kernel:
    Z = 144, 160, 176, 192 (every lifting size that kernel takes), both base graphs in both of its layer classes (the
    code rate sets the class), each with 256QAM and 4 fillers (groups of four), 256QAM and 6 fillers (symbol by symbol,
    one 8-byte read per symbol) and 64QAM (symbol by symbol, byte reads). Nine codeblocks per Z, decodable and noise
    mixed: codeblocks pair when they share Z, early stop and iteration limit, so some workgroups carry two codeblocks
    and, the count being odd, at least one has an empty slot."""
    import srsgpu
    rng = np.random.default_rng(1250)
    cbs, llrs = [], []
    for k, (bg, Z, rate, layers) in enumerate(((1, 144, 0.6, 16), (2, 160, 0.4, 16), (1, 176, 0.75, 8), (2, 192, 0.6, 8))):
        for g, (qm, F) in enumerate(((8, 4), (8, 6), (6, 0))):
            E = _pick_E(bg, Z, qm, F, rate=rate)
            # The layer class the host derives (capi.cpp add_pusch_cb, layer_class); above 16 layers the one-codeblock
            # kernel would take the codeblock.
            bound = max(-(-(E + F) // Z) + 2, BG_K[bg] + 4) - BG_K[bg]
            assert (8 if bound <= 8 else 16 if bound <= 16 else 0) == layers, (bg, Z, bound)
            for good in (True, False, True):
                cbs.append(_case(srsgpu, 3 * k + g, good, bg, Z, qm, E, F))
                llrs.append(_payload_llrs(orc, rng, bg, Z, qm, E, F) if good and len(cbs) % 3 == 0
                            else _llrs(rng, E, good))
    for Z in (144, 160, 176, 192):
        keys = [(c.use_early_stop, c.max_iterations) for c in cbs if c.lifting_size == Z]
        assert len(keys) % 2 == 1 and max(keys.count(x) for x in keys) >= 2, keys
    _check_group(orc, ctx, cbs, llrs, 1251, pairs=True)


def test_input_end_and_fillers(orc, ctx):
    """Where the rate-matched part ends (E + F): on a column boundary, on a group boundary inside a column that is not a
    multiple of 8, inside a group of four (fillers not a multiple of 4, and 64QAM), at the very end of the buffer
    (E = N - F), and short of the message (no decoding); fillers 0, 4 and 6; E + F < N with a HARQ tail that is 16-byte
    aligned at neither end (BG2 Z = 36, 44: N = 50 Z)."""
    import srsgpu
    rng = np.random.default_rng(1300)
    specs = []
    for bg, Z in ((1, 208), (2, 112), (1, 104)):
        N4, _ = _geometry(bg, Z, 4)
        specs += [(bg, Z, 8, 0, _pick_E(bg, Z, 8, 0, lambda E: E % Z == 0)),                 # column boundary
                  (bg, Z, 8, 4, _pick_E(bg, Z, 8, 4, lambda E: (E + 4) % Z % 8 == 4)),       # group boundary, odd group
                  (bg, Z, 8, 6, _pick_E(bg, Z, 8, 6)),                                       # (E + F) % 4 == 2: inside a group
                  (bg, Z, 6, 6, _pick_E(bg, Z, 6, 6)),                                       # 64QAM, inside a group
                  (bg, Z, 8, 4, _pick_E(bg, Z, 8, 4, lambda E: E >= N4 - 4 - 31, rate=1.0))]  # the last column
    for bg, Z in ((2, 36), (2, 44), (1, 20)):
        # N % 16 == 8 and (E + 4) % 16 == 4: with these in the batch the tails start and end off 16-byte boundaries.
        specs += [(bg, Z, 8, 0, _pick_E(bg, Z, 8, 0)), (bg, Z, 8, 4, _pick_E(bg, Z, 8, 4))]
    # E = N - F exactly (the whole buffer is written: no tail) and E < ninfo + 2 Z (input shorter than the message).
    N0, ninfo0 = _geometry(1, 208, 0)
    specs += [(1, 208, 8, 0, N0), (1, 208, 8, 0, _pick_E(1, 208, 8, 0, rate=1.0))]
    assert specs[-1][4] < ninfo0 + 2 * 208
    cbs, llrs = [], []
    for bg, Z, qm, F, E in specs:
        for good in (True, False):
            cbs.append(_case(srsgpu, len(cbs) // 2, good, bg, Z, qm, E, F))
            llrs.append(_llrs(rng, E, good))
    _check_group(orc, ctx, cbs, llrs, 1301)


def test_saturated_groups(orc, ctx):
    """+/-127, +/-65, +/-64 and +/-63 inside groups of four (the +/-64 clamp of whole columns, all at once in the group
    path and per byte in the fallback), in the systematic part and past the fillers."""
    import srsgpu
    rng = np.random.default_rng(1400)
    # The decodable (all-zero) codeblocks get one saturated wrong bit per run, so that they still decode; the noise
    # codeblocks also get every run negated.
    runs = np.array([[127, -127, 65, 64, 63, 127, 65, 64], [65, 127, -65, 64, 127, 63, 66, 120],
                     [64, -64, 127, 65, 121, 126, 63, 127]], np.int8)
    cbs, llrs = [], []
    for bg, Z, qm, F in ((1, 208, 8, 4), (1, 104, 8, 0), (2, 112, 8, 4), (2, 44, 8, 0), (1, 208, 8, 6), (1, 208, 6, 0)):
        E = _pick_E(bg, Z, qm, F)
        _, ninfo = _geometry(bg, Z, F)
        for good in (True, False):
            llr = _llrs(rng, E, good)
            # Visits inside the systematic part, across its end (the filler shift) and past it.
            for first, run in zip((64, ninfo - 4, ninfo + 40), runs):
                for k, v in enumerate(run):
                    llr[_visit_index(first + k, E, qm)] = v
                    if not good:
                        llr[_visit_index(first + 16 + k, E, qm)] = -v
            cbs.append(_case(srsgpu, len(cbs) // 2, good, bg, Z, qm, E, F))
            llrs.append(llr)
    _check_group(orc, ctx, cbs, llrs, 1401)


def test_trailing_zero_llrs(orc, ctx):
    """The last 1, 3, 4 and 17 LLRs of the input zero, with the rate-matched part ending 4 positions into a column: the
    index of the last non-zero LLR (taken per group from the dword's highest non-zero byte) sets the number of layers,
    so the last two drop one."""
    import srsgpu
    rng = np.random.default_rng(1500)
    cbs, llrs = [], []
    for bg, Z, qm, F in ((1, 208, 8, 4), (2, 112, 8, 4), (1, 44, 8, 4)):
        E = _pick_E(bg, Z, qm, F, lambda E: (E + F) % Z == 4)
        for t in (1, 3, 4, 17):
            for good in (True, False):
                llr = _llrs(rng, E, good)
                llr[llr == 0] = 1  # only the chosen tail is zero
                for n in range(E - t, E):
                    llr[_visit_index(n, E, qm)] = 0
                cbs.append(_case(srsgpu, len(cbs) // 2, good, bg, Z, qm, E, F))
                llrs.append(llr)
    _check_group(orc, ctx, cbs, llrs, 1501)


def _tb_plan_outputs(srsgpu, ctx, cfgs, nof_cbs, cb_len, llrs, fold, split):
    """One execute of a TB-level plan created with decoder_tb_fold = fold and decoder_split = split, over a TB buffer
    prefilled with 0xA5."""
    import torch
    dev = torch.device("cuda", 0)
    arr, nllr, nharq, ncb, ntb = srsgpu.make_pusch_tb_configs(cfgs, nof_cbs, cb_len)
    d_llrs = torch.from_numpy(np.concatenate(llrs).astype(np.int8)).to(dev)
    assert d_llrs.numel() == nllr
    with ctx.options(decoder_tb_fold=fold, decoder_split=split):
        plan = srsgpu.PuschDecoderPlan(ctx, srsgpu.IMPL_BY_NAME["avx2"], arr)
    out = dict(harq=torch.zeros(nharq, dtype=torch.int8, device=dev),
               crc=torch.zeros(ncb, dtype=torch.uint8, device=dev),
               msgs=torch.zeros(ncb * srsgpu.CB_MSG_STRIDE, dtype=torch.uint8, device=dev),
               iters=torch.zeros(ncb, dtype=torch.int32, device=dev),
               tbs=torch.full((ntb,), 0xA5, dtype=torch.uint8, device=dev),
               ok=torch.full((len(cfgs),), 7, dtype=torch.uint8, device=dev))
    plan.execute(d_llrs, out["harq"], out["crc"], out["msgs"], out["iters"], out["tbs"], out["ok"])
    torch.cuda.synchronize(dev)
    plan.close()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("plan_kind", ["single", "with_segmented", "with_rv2"])
def test_single_codeblock_tbs_written_by_decoder(orc, ctx, plan_kind):
    """Four single-codeblock TBs, two clean and two pure noise: with SRSGPU_OPTION_DECODER_TB_FOLD the decoder writes the
    TB bytes and flags and no TB stage runs; alone, with a segmented TB in the plan (the TB stage must still run) and
    with a single-codeblock TB sent as rv 2 (not dematched by the decoder: the fold must be off). TB bytes, TB and
    codeblock flags, messages, iteration counts and HARQ buffers equal those of the plan with the separate TB stage; the
    clean TBs are the sent bytes, the failed ones leave their 0xA5 prefill untouched."""
    import srsgpu
    from srsgpu import sch
    rng = np.random.default_rng(1600)
    grants = [(sch.UeGrant(4, 1, 8, 948), 0, True), (sch.UeGrant(5, 1, 8, 948), 0, False),
              (sch.UeGrant(2, 1, 6, 600.0), 0, True), (sch.UeGrant(3, 2, 8, 682.5), 0, False)]
    if plan_kind == "with_segmented":
        grants.insert(2, (sch.UeGrant(30, 2, 8, 682.5), 0, True))
    if plan_kind == "with_rv2":
        grants.insert(1, (sch.UeGrant(4, 1, 8, 682.5), 2, True))
    cfgs, segs, tbs, llrs = [], [], [], []
    for g, rv, clean in grants:
        seg = g.segmentation()
        tb = rng.integers(0, 256, seg.tbs // 8).astype(np.uint8)
        cw, _, _ = oracle_pdsch_encode(orc, tb, seg.base_graph, rv, g.qm, g.nof_layers, 0, g.nof_ch_symbols)
        llrs.append(bits_to_llrs(rng, cw, amp=10.0, noise=2.0) if clean
                    else np.clip(np.round(4.0 * rng.standard_normal(cw.size)), -120, 120).astype(np.int8))
        cfgs.append(srsgpu.PuschTransportBlock(seg.tbs // 8, seg.base_graph, rv, g.qm, g.nof_layers, g.nof_ch_symbols,
                                               new_data=True, nof_ldpc_iterations=6))
        segs.append(seg)
        tbs.append(tb)
    nof_cbs = [s.nof_segments for s in segs]
    assert sorted(nof_cbs)[-2] == 1 and (max(nof_cbs) > 1) == (plan_kind == "with_segmented")
    cb_len = [BG_N_SHORT[s.base_graph] * s.lifting_size for s in segs]
    off = _tb_plan_outputs(srsgpu, ctx, cfgs, nof_cbs, cb_len, llrs, 0, -1)
    # The fold in the edge-split kernel (the host's choice for so few codeblocks) and in the one-row-pair kernel.
    for split in (-1, 0):
        on = _tb_plan_outputs(srsgpu, ctx, cfgs, nof_cbs, cb_len, llrs, 1, split)
        for k in on:
            assert np.array_equal(on[k], off[k]), (k, split)
    # A clean rv 2 transmission alone does not carry the systematic bits: it may fail; the others are as sent.
    o = 0
    for (g, rv, clean), tb, ok in zip(grants, tbs, on["ok"]):
        assert ok in (0, 1)
        if rv == 0:
            assert bool(ok) == clean, (g, ok)
        got = on["tbs"][o:o + tb.size]
        assert np.array_equal(got, tb) if ok else bool((got == 0xA5).all()), (g, ok)
        o += tb.size
    assert int(on["ok"].sum()) >= 2 and int((on["ok"] == 0).sum()) >= 2
