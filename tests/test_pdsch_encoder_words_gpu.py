"""GPU parity of the PDSCH packed encoder's message path: a codeblock's span of the transport block is read as the
aligned 32-bit words that hold at least one of its bytes (two neighbours realigned when the span does not start on a
word), written to the message by words, and the bytes after the TB's (TB CRC, zero padding, CRC slot, fillers) are
masked to zero in the boundary word. Every message byte reaches the codeword, so the codewords are compared bit for bit
with the oracle composition of the other encoder tests (chain_lib), in an output pre-filled with 0xAB.

Shapes: TB offsets 0, 1, 2 and 3 modulo 4 (the realignment by 0 to 3 bytes); TB sizes whose last word is partial and
whole; one codeblock (the carrier of the TB CRC alone), two and three (codeblocks that carry none of it before the one
that does, spans that start off a word inside the TB); fillers present and absent; both base graphs; Z = 32, 64 and
288, all multiples of 32 with byte-aligned codeblocks, which is what the packed kernel takes. The TB buffer ends with
the last TB's last byte: nothing the kernel may load lies behind it."""
import numpy as np
import pytest

from chain_lib import oracle_pdsch_encode
from oracle_lib import Oracle
from test_pdsch_encoder_order_gpu import _nof_ch_symbols

pytestmark = pytest.mark.gpu

# (TB bytes, base graph, codeblocks, Z, TB offset modulo 4, fillers)
SHAPES = [
    (84, 1, 1, 32, 0, True), (85, 1, 1, 32, 1, True), (82, 1, 1, 32, 2, True), (83, 1, 1, 32, 3, True),
    (86, 1, 1, 32, 1, False),
    (165, 1, 1, 64, 2, True), (170, 1, 1, 64, 3, True), (174, 1, 1, 64, 0, False),
    (705, 1, 1, 288, 1, True), (1401, 1, 2, 288, 3, True), (1403, 1, 2, 288, 0, True), (2106, 1, 3, 288, 2, True),
    (2364, 1, 3, 288, 1, False),
    (21, 2, 1, 32, 0, True), (30, 2, 1, 32, 3, True),
    (61, 2, 1, 64, 1, True), (62, 2, 1, 64, 2, True), (59, 2, 1, 64, 0, True),
    (323, 2, 1, 288, 2, True), (633, 2, 2, 288, 1, True), (635, 2, 2, 288, 2, True), (954, 2, 3, 288, 3, True),
    (1068, 2, 3, 288, 0, False),
]
IDS = ["%d-bg%d-%dcb-z%d-o%d" % s[:5] for s in SHAPES]


def segmentation(nb, bg, nof_cbs):
    from srsgpu import sch
    nsym = _nof_ch_symbols(nb, 8, 4, nof_cbs)
    return nsym, sch.segment(nb * 8, bg, 8, 4, nsym)


def test_shapes_are_what_they_are_named():
    """Lifting size, codeblock count, fillers and byte-aligned codeblocks of every shape, and the coverage the module
    states."""
    for nb, bg, nof_cbs, z, off, fill in SHAPES:
        _, seg = segmentation(nb, bg, nof_cbs)
        assert (seg.nof_segments, seg.lifting_size) == (nof_cbs, z), (nb, bg, seg.nof_segments, seg.lifting_size)
        assert (seg.nof_filler_bits > 0) == fill and seg.nof_filler_bits % 8 == 0, (nb, bg, seg.nof_filler_bits)
        assert all(cb.rm_length % 32 == 0 and cb.tb_offset % 8 == 0 and cb.nof_info_bits % 8 == 0
                   for cb in seg.codeblocks), (nb, bg)
    for bg in (1, 2):
        for z in (32, 64, 288):
            mine = [s for s in SHAPES if s[1] == bg and s[3] == z]
            assert {s[0] % 4 for s in mine} >= {1, 2} and len({s[4] for s in mine}) >= 2, (bg, z)
        assert {s[2] for s in SHAPES if s[1] == bg} == {1, 2, 3}
        assert {s[5] for s in SHAPES if s[1] == bg} == {True, False}
    assert {s[4] for s in SHAPES} == {0, 1, 2, 3} and {s[0] % 4 for s in SHAPES} == {0, 1, 2, 3}


def _encode(ctx, tbs, cfgs, tb_mod4):
    """One plan over the TBs: TB i at a byte offset congruent to tb_mod4[i] modulo 4 (random bytes between TBs), the
    TB buffer ending with the last TB, the codewords back to back in an output pre-filled with 0xAB."""
    import srsgpu
    import torch
    arr, _, _, _ = srsgpu.make_pdsch_configs([t.size for t in tbs], cfgs)
    to = co = 0
    ranges = []
    for a, t, c, m in zip(arr, tbs, cfgs, tb_mod4):
        to = (to + 3) // 4 * 4 + m
        a.tb_offset, a.cw_offset = to, co
        nbytes = c.nof_ch_symbols * c.modulation_order // 8
        ranges.append((co, co + nbytes))
        to += t.size
        co += nbytes
    buf = np.random.default_rng(5).integers(0, 256, to).astype(np.uint8)
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
    assert (raw[co:] == 0xAB).all(), "a store past the last codeword"
    return [np.unpackbits(raw[b:e]) for b, e in ranges]


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


@pytest.fixture(scope="module")
def cases():
    """TBs, configurations and the oracle's codewords, computed once."""
    import srsgpu
    orc = Oracle()
    rng = np.random.default_rng(777)
    tbs, cfgs, want = [], [], []
    for nb, bg, nof_cbs, _, _, _ in SHAPES:
        nsym, _ = segmentation(nb, bg, nof_cbs)
        tb = rng.integers(0, 256, nb).astype(np.uint8)
        tb[-4:] = 0xFF  # the TB's last bytes set: a byte masked off or read from the wrong place shows
        cw, _, _ = oracle_pdsch_encode(orc, tb, bg, 0, 8, 4, 0, nsym)
        tbs.append(tb)
        cfgs.append(srsgpu.PdschTransportBlock(bg, 0, 8, 4, nsym))
        want.append(cw)
    return tbs, cfgs, want


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_pdsch_encoder_words_one_tb(ctx, cases, i):
    """One TB per plan, at its offset modulo 4, ending at the end of the TB buffer."""
    tbs, cfgs, want = cases
    got = _encode(ctx, [tbs[i]], [cfgs[i]], [SHAPES[i][4]])
    assert np.array_equal(got[0], want[i]), SHAPES[i]


def test_pdsch_encoder_words_mixed_plan(ctx, cases):
    """All of them in one plan, carriers and other codeblocks in the same launches, the last TB (an odd size) ending
    at the end of the TB buffer."""
    tbs, cfgs, want = cases
    order = list(range(len(SHAPES)))
    order.append(order.pop(9))  # 1401 bytes at offset 3 last: its last word is partial
    got = _encode(ctx, [tbs[i] for i in order], [cfgs[i] for i in order], [SHAPES[i][4] for i in order])
    for i, a in zip(order, got):
        assert np.array_equal(a, want[i]), (i, SHAPES[i])
