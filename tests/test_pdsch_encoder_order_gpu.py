"""GPU parity of PDSCH encoder plans in which the descriptor order and the packed kernel's shared LDS region matter:
the packed codeblocks that carry their TB's CRC are uploaded first, and such a codeblock stages the TB CRC's tables
where its codeblock words and edge table go afterwards. It computes the TB CRC from preloaded chunks when the TB has at
most 4096 bytes and 4-byte aligned offset and size, else chunk by chunk from memory.

Every plan is compared bit for bit with the oracle composition the other encoder tests use (chain_lib), and with the
same TBs encoded one TB per plan, which no order can change. Plans: TBs of one to five codeblocks in one plan (packed
kernel only, so the TB CRCs are computed inline), and byte-kernel codeblocks (Z = 208) of both base graphs next to
packed ones (the TB CRCs come from their own kernel); each with codewords that tile the output (no memset) and with
gaps between them (memset)."""
import numpy as np
import pytest

from chain_lib import oracle_pdsch_encode
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

# (TB bytes, base graph, codeblocks, Z, TB offset modulo 4). Z % 32 == 0: packed kernel; Z = 208: byte kernel.
SEGMENTATION_PLAN = [
    (400, 1, 1, 160, 0),    # one codeblock, CRC16: TB CRC only
    (484, 1, 1, 192, 0),    # one codeblock, CRC24A
    (992, 1, 1, 384, 0),    # one codeblock of the largest lifting size
    (1137, 1, 2, 224, 0),   # two codeblocks: an odd size, as every such TB with byte-aligned codeblocks has
    (2112, 1, 3, 288, 0),   # three codeblocks of the benchmark's sizes
    (2640, 1, 3, 352, 0),
    (2112, 1, 3, 288, 1),   # the same at an offset that is no multiple of 4
    (2106, 1, 3, 288, 0),   # size no multiple of 4
    (3144, 1, 3, 384, 0),   # more CB CRC chunks (132) than lanes, the last one partial
    (4097, 1, 4, 384, 0),   # just over 4096 bytes
    (4232, 1, 5, 320, 0),   # over 4096 bytes with size and offset multiples of 4
    (112, 2, 1, 96, 0),     # BG2, one codeblock, CRC16
    (960, 2, 3, 288, 0),    # BG2, three and five codeblocks, size a multiple of 4
    (1912, 2, 5, 320, 0),
]
KERNELS_PLAN = [
    (560, 1, 1, 208, 0),    # byte kernel, BG1
    (2112, 1, 3, 288, 0),   # packed, BG1
    (255, 2, 1, 208, 0),    # byte kernel, BG2
    (960, 2, 3, 288, 0),    # packed, BG2
    (1101, 1, 2, 208, 0),   # byte kernel, two codeblocks
    (484, 1, 1, 192, 0),    # packed, one codeblock
    (1912, 2, 5, 320, 3),   # packed, BG2, odd TB offset
    (1137, 1, 2, 224, 0),   # packed, two codeblocks
]
PLANS = {"segmentation": SEGMENTATION_PLAN, "kernels": KERNELS_PLAN}
GAP_BYTES = 8


def _nof_ch_symbols(nbytes, qm, nof_layers, nof_cbs):
    """Code rate about 2/3, every codeblock the same whole number of 32-bit words for every Qm (a multiple of 3
    words, so 6 bits per symbol divide it too)."""
    step = 96 * nof_cbs * nof_layers
    return (nbytes * 12 // qm + step - 1) // step * step


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


@pytest.fixture(scope="module")
def cases():
    """Per (plan, mode): TBs, configurations and the oracle's codewords, computed once."""
    import srsgpu
    from srsgpu import sch
    orc = Oracle()
    out = {}
    for p, (name, shapes) in enumerate(PLANS.items()):
        for mode in ("tiled", "gaps"):
            rng = np.random.default_rng(100 + 2 * p + (mode == "gaps"))
            tbs, cfgs, want = [], [], []
            for i, (nb, bg, nof_cbs, z, _) in enumerate(shapes):
                # Tiled: whole words per codeblock (4 layers of 256QAM). Gaps: every Qm, rv and layer count.
                qm, nl, rv = (8, 4, 0) if mode == "tiled" else ((2, 4, 6, 8)[i % 4], 1 + i % 4, i % 4)
                nsym = _nof_ch_symbols(nb, qm, nl, nof_cbs)
                seg = sch.segment(nb * 8, bg, qm, nl, nsym)
                assert (seg.nof_segments, seg.lifting_size) == (nof_cbs, z), (nb, bg)
                assert all(cb.rm_length % 32 == 0 for cb in seg.codeblocks), (nb, bg, qm, nl)
                tb = rng.integers(0, 256, nb).astype(np.uint8)
                cw, _, _ = oracle_pdsch_encode(orc, tb, bg, rv, qm, nl, 0, nsym)
                tbs.append(tb)
                cfgs.append(srsgpu.PdschTransportBlock(bg, rv, qm, nl, nsym))
                want.append(cw)
            out[name, mode] = (tbs, cfgs, want)
    return out


def _encode_plan(ctx, tbs, cfgs, tb_mod4, gap, tb_tail=16):
    """One plan over all TBs: TB i at a byte offset congruent to tb_mod4[i] modulo 4 (random bytes between TBs and
    `tb_tail` of them behind the last), codewords `gap` bytes apart, each at the next multiple of 4 bytes, in an output
    pre-filled with 0xAB. Returns the unpacked codewords (a last byte's spare bits cut off), the output bytes and the
    codewords' byte ranges."""
    import srsgpu
    import torch
    arr, _, _, _ = srsgpu.make_pdsch_configs([t.size for t in tbs], cfgs)
    to = co = 0
    ranges, nbits = [], []
    for a, t, c, m in zip(arr, tbs, cfgs, tb_mod4):
        to = (to + 3) // 4 * 4 + m
        a.tb_offset, a.cw_offset = to, co
        nbits.append(c.nof_ch_symbols * c.modulation_order)
        nbytes = (nbits[-1] + 7) // 8
        ranges.append((co, co + nbytes))
        to += t.size
        co = (co + nbytes + gap + 3) // 4 * 4
    buf = np.random.default_rng(5).integers(0, 256, to + tb_tail).astype(np.uint8)
    for a, t in zip(arr, tbs):
        buf[a.tb_offset: a.tb_offset + t.size] = t
    dev = torch.device("cuda", ctx.device)
    d_tbs = torch.from_numpy(buf).to(dev)
    d_cw = torch.full((co + 16,), 0xAB, dtype=torch.uint8, device=dev)
    plan = srsgpu.PdschEncoderPlan(ctx, arr)
    plan.execute(d_tbs, d_cw)
    torch.cuda.synchronize(dev)
    plan.close()
    raw = d_cw.cpu().numpy()
    return [np.unpackbits(raw[b:e])[:n] for (b, e), n in zip(ranges, nbits)], raw, ranges


@pytest.mark.parametrize("mode", ["tiled", "gaps"])
@pytest.mark.parametrize("name", list(PLANS))
def test_pdsch_encoder_plan_order(ctx, cases, name, mode):
    import srsgpu
    tbs, cfgs, want = cases[name, mode]
    gap = GAP_BYTES if mode == "gaps" else 0
    got, raw, ranges = _encode_plan(ctx, tbs, cfgs, [s[4] for s in PLANS[name]], gap)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (name, mode, i, PLANS[name][i])
    # Outside the codewords: the gaps are zeroed with the output range, nothing is written past its end.
    for (_, e), (b, _) in zip(ranges[:-1], ranges[1:]):
        assert not raw[e:b].any(), (name, mode, e, b)
    assert (raw[ranges[-1][1]:] == 0xAB).all()
    # The same TBs, one TB per plan.
    enc = srsgpu.PdschEncoder(ctx)
    for i, (tb, cfg) in enumerate(zip(tbs, cfgs)):
        assert np.array_equal(enc.encode(tb, cfg), got[i]), (name, mode, i, PLANS[name][i])
