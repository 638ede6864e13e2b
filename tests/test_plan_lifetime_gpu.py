"""Lifetime of the device memory behind the C-ABI plans and contexts. Every plan type and the context hold their device
allocations through srsgpu::device_buffer (csrc/capi_internal.h), and srsgpu_debug_live_device_buffers() counts the
allocations that are alive. For each plan type, on the smallest configuration that fills every buffer the type has:
create / destroy cycles return the count exactly to where it was, a live plan holds the number of buffers its
configuration calls for, and a create that is refused leaves the count unchanged. A second context gives back all it
took. Plans are only created here, never executed: the kernels are not what is tested."""
import gc

import numpy as np
import pytest

import pdcch_cases
import uci_polar_cases
from ofdm_cases import CASES as OFDM_CASES
from pdsch_mod_cases import random_general_config, crb_mask_test_side
from pusch_chest_cases import random_case as chest_case, random_crb_mask
from pusch_demod_cases import random_general_case
from ulsch_demux_cases import random_config as demux_config

pytestmark = pytest.mark.gpu

CYCLES = 32


class Case:
    """make() -> the plans it created (closed by the test, last first); buffers: device allocations they hold while
    alive (None: at least min_buffers); refuse(): a create that the library refuses."""

    def __init__(self, make, refuse, buffers=None, min_buffers=1):
        self.make, self.refuse, self.buffers, self.min_buffers = make, refuse, buffers, min_buffers


def close_all(plans):
    for p in reversed(plans):
        p.close()


def decoder_cases(ctx, srsgpu):
    from srsgpu import sch
    simd = srsgpu.IMPL_BY_NAME["avx2"]
    # LDPC decoder, two-codeblock workgroups on: the two Z = 192 codeblocks make a pairs group, Z = 384 a plain packed
    # group (same base graph and layer class), the odd Z = 7 the unpacked kernel's group: three descriptor buffers.
    Zs = (192, 192, 384, 7)
    cbs = [srsgpu.CodeblockDecodeConfig(1, Z, nof_crc_bits=24) for Z in Zs]
    ldpc = srsgpu.make_configs(cbs, [24 * Z for Z in Zs], [srsgpu.CRC24B] * 4)
    bad_ldpc = srsgpu.make_configs(cbs[:1] + [srsgpu.CodeblockDecodeConfig(1, 17, nof_crc_bits=24)], [24 * 192, 24 * 17],
                                   [srsgpu.CRC24B] * 2)

    def with_pairs(create):
        def make():
            with ctx.options(decoder_pairs=1):
                return [create()]
        return make

    # PUSCH codeblocks: a first transmission of Z = 192 and one of Z = 384 are dematched by the decoder itself (fused:
    # descriptors and dematcher descriptors per group), the first in a pairs group, the second in a plain one; the
    # retransmission stays on the rate dematcher (the plan's d_dm) and in a plain group of its own. 2 + 2 + 1 + 1.
    pcb = [srsgpu.PuschCodeblock(1, 192, 0, 2, 24 * 192), srsgpu.PuschCodeblock(1, 384, 0, 2, 24 * 384),
           srsgpu.PuschCodeblock(1, 192, 1, 2, 24 * 192, new_data=False)]
    cb_arr = srsgpu.make_pusch_cb_configs(pcb)[0]
    bad_cb = srsgpu.make_pusch_cb_configs(pcb[:1] + [srsgpu.PuschCodeblock(1, 192, 0, 3, 24 * 192)])[0]

    # PUSCH transport block of 273 PRB of 256QAM: segmented, byte-aligned and above the inline size, so the plan takes
    # the sliced TB stage (d_slices, d_tb_acc) beside d_tb and the decoder's groups. Building it is host arithmetic
    # and a cached CRC table: a few milliseconds.
    def tb_configs(grants, bad_qm=None):
        tbs, segs = [], []
        for i, g in enumerate(grants):
            seg = g.segmentation()
            qm = bad_qm if (bad_qm is not None and i == len(grants) - 1) else g.qm
            tbs.append(srsgpu.PuschTransportBlock(seg.tbs // 8, seg.base_graph, 0, qm, g.nof_layers, g.nof_ch_symbols))
            segs.append(seg)
        return srsgpu.make_pusch_tb_configs(tbs, [s.nof_segments for s in segs],
                                            [srsgpu.BG_N_SHORT[s.base_graph] * s.lifting_size for s in segs])[0], segs
    big = sch.UeGrant(273, 1, 8, 948)
    tb_arr, segs = tb_configs([big])
    assert segs[0].nof_segments > 1 and segs[0].tbs // 8 > 16384
    bad_tb = tb_configs([sch.UeGrant(4, 1, 2, 300), sch.UeGrant(4, 1, 2, 300)], bad_qm=3)[0]

    # PDSCH encoder: one TB of each base graph, so both descriptor arrays exist beside d_tb, d_tb_crc and d_slices.
    grants = [sch.UeGrant(4, 1, 2, 120), sch.UeGrant(6, 1, 6, 800)]
    enc_segs = [g.segmentation() for g in grants]
    assert sorted(s.base_graph for s in enc_segs) == [1, 2]
    enc_tbs = [srsgpu.PdschTransportBlock(s.base_graph, 0, g.qm, g.nof_layers, g.nof_ch_symbols)
               for g, s in zip(grants, enc_segs)]
    enc_arr = srsgpu.make_pdsch_configs([s.tbs // 8 for s in enc_segs], enc_tbs)[0]
    bad_enc = srsgpu.make_pdsch_configs([s.tbs // 8 for s in enc_segs], enc_tbs)[0]
    bad_enc[1].rv = 4
    return {
        "ldpc_decoder": Case(with_pairs(lambda: srsgpu.LdpcDecoderPlan(ctx, simd, ldpc)),
                             lambda: srsgpu.LdpcDecoderPlan(ctx, simd, bad_ldpc), buffers=3),
        "pusch_cb": Case(with_pairs(lambda: srsgpu.PuschCbPlan(ctx, simd, cb_arr)),
                         lambda: srsgpu.PuschCbPlan(ctx, simd, bad_cb), buffers=6),
        "pusch_decoder": Case(lambda: [srsgpu.PuschDecoderPlan(ctx, simd, tb_arr)],
                              lambda: srsgpu.PuschDecoderPlan(ctx, simd, bad_tb), min_buffers=4),
        "pdsch_encoder": Case(lambda: [srsgpu.PdschEncoderPlan(ctx, enc_arr)],
                              lambda: srsgpu.PdschEncoderPlan(ctx, bad_enc), buffers=5),
    }


def downlink_cases(ctx, srsgpu):
    from test_pdcch_gpu import to_dci
    from test_pdsch_modulator_gpu import to_general_mod
    rng = np.random.default_rng(5)
    G = 24
    # PDSCH modulator through _create_ex: a CRB mask (d_sc_map) and two PRGs of 12 PRB (d_prg_w) beside d_desc,
    # d_chunks and d_seq.
    cfg, _nbits, w = random_general_config(rng, G, interleave=0, prg=12, nof_reserved=0)
    mod = to_general_mod(cfg, w, crb_mask_test_side(cfg, G), G)
    assert mod.prg_weights.shape[0] == 2 and mod.crb_mask is not None
    exts, keep = srsgpu.make_alloc_exts([mod], G)
    mod_arr = srsgpu.make_pdsch_mod_configs([mod], [0], [0], G)
    bad_mod = srsgpu.make_pdsch_mod_configs([mod], [0], [0], G)
    bad_mod[0].nof_bits -= 32

    w2 = np.eye(2, dtype=np.complex64)
    mask = np.zeros(G, np.uint8)
    mask[[3, 4, 9]] = 1
    dmrs = srsgpu.PdschDmrs(slot_index=3, scrambling_id=77, n_scid=0, dmrs_type=1, nof_layers=2, nof_ports=2,
                            dmrs_symbol_mask=1 << 2, reference_point_k_rb=0, rb_start=3, nof_rb=3, amplitude=1.0,
                            weights=w2, crb_mask=mask)
    dmrs_arr = srsgpu.make_pdsch_dmrs_configs([dmrs], [0])
    dmrs_exts, dmrs_keep = srsgpu.make_dmrs_exts([dmrs], G)
    bad_exts, bad_keep = srsgpu.make_dmrs_exts([dmrs], G)
    bad_exts[0].prg_size = 4

    base, payload = pdcch_cases.fill_dci(rng, dict(pdcch_cases.TEMPLATES[0], aggregation_level=2, cce_index=0), 40)
    base.update(nof_ports=1, weights=np.ones(1, np.complex64), data_scaling=pdcch_cases.F(1),
                dmrs_amplitude=pdcch_cases.F(1))
    dci = to_dci(base, payload)
    return {
        "pdsch_modulator": Case(lambda: [srsgpu.PdschModulatorPlan(ctx, mod_arr, G, 4, exts)],
                                lambda: srsgpu.PdschModulatorPlan(ctx, bad_mod, G, 4, exts), buffers=5),
        "pdsch_dmrs": Case(lambda: [srsgpu.PdschDmrsPlan(ctx, dmrs_arr, G, 4, dmrs_exts)],
                           lambda: srsgpu.PdschDmrsPlan(ctx, dmrs_arr, G, 4, bad_exts), buffers=2),
        # Two DCIs on the same REs are refused.
        "pdcch": Case(lambda: [srsgpu.PdcchPlan(ctx, [dci], 52, 4, 1)],
                      lambda: srsgpu.PdcchPlan(ctx, [dci, dci], 52, 4, 1), buffers=6),
        "_keep_downlink": (keep, dmrs_keep, bad_keep),  # what the extension structures point to
    }


def ofdm_cases(ctx, srsgpu):
    mu, rb, N, ext, scale, fc, slot, _woff = next(c for c in OFDM_CASES if c[2] == 128)
    smu, srb, sN, sext, sscale, sfc, sslot, _ = next(c for c in OFDM_CASES if c[2] == 9216)

    def small(bw=rb, symbol=0):
        return srsgpu.OfdmPlan(ctx, True, mu, bw, N, scale, fc, [slot], 1, cp_extended=ext, symbols=(symbol, 1))

    def concat():
        members = [small(symbol=0), small(symbol=5)]
        return members + [srsgpu.OfdmPlan.concat(members)]

    def refuse_concat():
        members = [small(), small(bw=rb - 1)]
        try:
            srsgpu.OfdmPlan.concat(members)
        finally:
            close_all(members)
    return {
        "ofdm": Case(lambda: [srsgpu.OfdmPlan(ctx, False, mu, rb, N, scale, fc, [slot], 2, cp_extended=ext)],
                     lambda: srsgpu.OfdmPlan(ctx, True, mu, rb, 3000, scale, fc, [slot], 1), buffers=1),
        # A split size: the jobs and one N-point row per job of scratch. A slot index beyond the subframe is refused
        # after the plan object exists.
        "ofdm_split": Case(lambda: [srsgpu.OfdmPlan(ctx, True, smu, srb, sN, sscale, sfc, [sslot], 1, cp_extended=sext)],
                           lambda: srsgpu.OfdmPlan(ctx, True, smu, srb, sN, sscale, sfc, [1 << smu], 1), buffers=2),
        "ofdm_concat": Case(concat, refuse_concat, buffers=3),
    }


def uplink_cases(ctx, srsgpu):
    from test_pusch_chest_gpu import to_est
    from test_pusch_demodulator_gpu import to_demod_general
    from test_ulsch_demux_gpu import to_demux
    rng = np.random.default_rng(6)
    G = 24
    # Demodulator: one transform-precoded transmission (d_tp_jobs) and one on a CRB mask (d_chunks, d_crbs), beside
    # d_desc, d_tables, d_seq and d_acc.
    tp_cfg, _, _, _, _ = random_general_case(rng, G, transform_precoding=True, mask=False)
    cm_cfg, _, _, _, crb = random_general_case(rng, G, transform_precoding=False, mask=True)
    demods = [to_demod_general(tp_cfg, None, True), to_demod_general(cm_cfg, crb, False)]
    dem_arr = srsgpu.make_pusch_demod_configs(demods, [0, 1])[0]
    dem_exts, dem_keep = srsgpu.make_crb_mask_exts(demods, G)
    bad_dem = srsgpu.make_pusch_demod_configs(demods, [0, 1])[0]
    bad_dem[1].modulation_order = 3

    # Estimator: low-PAPR DM-RS (d_lp) and a CRB mask (d_crbs), beside d_jobs and d_seq.
    lp_cfg, _, _ = chest_case(rng, G, nof_rb=4, dmrs_type2=0, low_papr_id=321)
    mask = random_crb_mask(rng, G)
    cm_est, _, _ = chest_case(rng, G, crb_mask=mask)
    ests = [to_est(lp_cfg), to_est(cm_est)]
    ests[0].dmrs_sequence, ests[0].scrambling_id = srsgpu.DMRS_LOW_PAPR, 321
    ests[1].crb_mask = mask
    est_arr = srsgpu.make_pusch_chest_configs(ests, [0, 1])
    est_exts, est_keep = srsgpu.make_crb_mask_exts(ests, G)
    bad_est = srsgpu.make_pusch_chest_configs(ests, [0, 1])
    bad_est[1].fd_smoothing = 3

    cfg, c2b, c2e, c_init = demux_config(rng, max_prb=4)
    demux = to_demux(cfg, c2b, c2e, c_init)
    bad_demux = to_demux(dict(cfg, nof_harq_ack_bits=5, nof_enc_harq_ack_bits=10 ** 6, nof_harq_ack_rvd=0), c2b, c2e,
                         c_init)

    # A polar field of two codeblocks beside a one-codeblock field (two codes in the tables).
    two_cb = (400, 0, 1200, 0, 0)
    assert uci_polar_cases.nof_codeblocks(two_cb[0], two_cb[2]) == 2
    assert uci_polar_cases.field_refusal(two_cb[0], two_cb[2]) is None
    polar = [two_cb, (20, 1, 240, 0, 13)]
    return {
        "pusch_demodulator": Case(lambda: [srsgpu.PuschDemodulatorPlan(ctx, dem_arr, G, 4, dem_exts)],
                                  lambda: srsgpu.PuschDemodulatorPlan(ctx, bad_dem, G, 4, dem_exts), buffers=7),
        "pusch_chest": Case(lambda: [srsgpu.PuschChannelEstimatorPlan(ctx, est_arr, G, 4, est_exts)],
                            lambda: srsgpu.PuschChannelEstimatorPlan(ctx, bad_est, G, 4, est_exts), buffers=4),
        "ulsch_demux": Case(lambda: [srsgpu.UlschDemuxPlan(ctx, [demux], [0])],
                            lambda: srsgpu.UlschDemuxPlan(ctx, [bad_demux], [0]), buffers=4),
        "uci_decoder": Case(lambda: [srsgpu.UciDecoderPlan(ctx, [(4, 2, 0, 32, 0), (11, 2, 1, 64, 0)])],
                            lambda: srsgpu.UciDecoderPlan(ctx, [(4, 2, 0, 32, 0), (12, 2, 0, 64, 0)]), buffers=1),
        "uci_polar_decoder": Case(lambda: [srsgpu.UciPolarDecoderPlan(ctx, polar)],
                                  lambda: srsgpu.UciPolarDecoderPlan(ctx, [polar[1], (11, 0, 64, 0, 0)]), buffers=4),
        "_keep_uplink": (dem_keep, est_keep),
    }


PLAN_TYPES = ("ldpc_decoder", "pusch_cb", "pusch_decoder", "pdsch_encoder", "pdsch_modulator", "pdsch_dmrs", "pdcch",
              "ofdm", "ofdm_split", "ofdm_concat", "pusch_demodulator", "pusch_chest", "ulsch_demux", "uci_decoder",
              "uci_polar_decoder")


@pytest.fixture(scope="module")
def lifetime():
    """The context, the cases of every plan type, and each plan created and destroyed once: the context's lazily built
    tables (Gold sequences, DFT twiddles, cached CRC tables) exist before any count is taken."""
    import srsgpu
    ctx = srsgpu.Context(0)
    cases = {}
    for group in (decoder_cases, downlink_cases, ofdm_cases, uplink_cases):
        cases.update(group(ctx, srsgpu))
    assert set(PLAN_TYPES) == {k for k in cases if not k.startswith("_")}
    for name in PLAN_TYPES:
        close_all(cases[name].make())
    yield srsgpu, ctx, cases
    ctx.close()


def settled_count(srsgpu):
    """The live count once plans that earlier tests dropped without closing have been collected."""
    gc.collect()
    return srsgpu.live_device_buffers()


@pytest.mark.parametrize("name", PLAN_TYPES)
def test_create_destroy_cycles_leak_nothing(lifetime, name):
    srsgpu, _ctx, cases = lifetime
    case = cases[name]
    before = settled_count(srsgpu)
    for _ in range(CYCLES):
        plans = case.make()
        held = srsgpu.live_device_buffers() - before
        close_all(plans)
        if case.buffers is not None:
            assert held == case.buffers, (name, held)
        assert held >= case.min_buffers, (name, held)
        assert srsgpu.live_device_buffers() == before, name
    assert srsgpu.live_device_buffers() == before


@pytest.mark.parametrize("name", PLAN_TYPES)
def test_refused_create_allocates_nothing(lifetime, name):
    srsgpu, _ctx, cases = lifetime
    before = settled_count(srsgpu)
    with pytest.raises(srsgpu.SrsGpuError):
        cases[name].refuse()
    assert srsgpu.live_device_buffers() == before, name
    # The refusal left the context whole: the same plan type still builds and still gives everything back.
    close_all(cases[name].make())
    assert srsgpu.live_device_buffers() == before, name


def test_second_context_gives_back_its_tables(lifetime):
    """A second context with its own LDPC / CRC tables, Gold tables (PDCCH plan) and DFT twiddles (OFDM plan), created
    and closed while the first lives."""
    srsgpu, ctx, cases = lifetime
    before = settled_count(srsgpu)
    other = srsgpu.Context(0)
    own = srsgpu.live_device_buffers() - before
    assert own == 12  # per base graph: shifts, 32-bit shifts, two pair-address tables, core plans; CRC arena and slices
    mu, rb, N, ext, scale, fc, slot, _ = next(c for c in OFDM_CASES if c[2] == 128)
    srsgpu.OfdmPlan(other, True, mu, rb, N, scale, fc, [slot], 1, cp_extended=ext).close()
    srsgpu.PdcchPlan(other, [], 52, 4, 1).close()
    assert srsgpu.live_device_buffers() - before == own + 4  # twiddles and the three Gold tables
    other.close()
    assert srsgpu.live_device_buffers() == before
    assert ctx.handle  # the first context is untouched
    close_all(cases["pdcch"].make())
    assert srsgpu.live_device_buffers() == before
