"""GPU parity of the PDSCH encoder's CRC arithmetic: the packed kernel moves every chunk remainder of the TB CRC and of
the codeblock CRC to the end of its message with a byte-wise GF(2) product reduced through the staged byte table, and
reads the codeblock CRC's whole chunks as aligned words. Every CRC is part of the codeword, so the codewords are compared
bit for bit with the oracle composition of the other encoder tests (chain_lib), TB by TB and as one plan of all of them.

TB sizes (bytes) by what they reach in the TB CRC (16-byte chunks, two per lane preloaded up to 4 096 bytes when offset
and size are multiples of 4, else chunk by chunk) and in the codeblock CRC (8-byte chunks of the codeblock's bytes):
last chunk full and partial, at most 16 bytes and at most two chunks, both sides of the 4 096-byte limit, sizes and
offsets that are no multiple of 4, CRC16 (at most 3 824 bits) and CRC24A on both sides of that limit, one codeblock (no
CRC24B) and two to five, both base graphs. Z % 32 == 0 is the packed kernel; the TBs of at most 16 bytes have no such
lifting size and take the byte kernel, whose CRCs keep the shift-and-add product."""
import numpy as np
import pytest

from chain_lib import oracle_pdsch_encode
from oracle_lib import Oracle
from test_pdsch_encoder_order_gpu import _encode_plan, _nof_ch_symbols

pytestmark = pytest.mark.gpu

# (TB bytes, base graph, codeblocks, Z, TB offset modulo 4)
SHAPES = [
    (12, 2, 1, 20, 0),      # at most 16 bytes: one partial chunk (byte kernel)
    (16, 2, 1, 24, 0),      # exactly one chunk (byte kernel)
    (21, 2, 1, 32, 0),      # packed, two chunks, the second partial, size no multiple of 4: CRC16
    (30, 2, 1, 32, 2),      # the same at an offset that is no multiple of 4
    (400, 1, 1, 160, 0),    # BG1, CRC16, last chunk full (25 chunks)
    (472, 2, 1, 384, 0),    # BG2, CRC16, last chunk partial (8 bytes)
    (478, 2, 1, 384, 0),    # 3 824 bits: the largest CRC16 TB, size no multiple of 4
    (482, 1, 1, 192, 0),    # 3 856 bits: CRC24A, size no multiple of 4, one codeblock
    (484, 1, 1, 192, 0),    # CRC24A, multiple of 4, last chunk partial (4 bytes)
    (992, 1, 1, 384, 0),    # CRC24A, last chunk full, one codeblock of the largest size
    (1137, 1, 2, 224, 0),   # two codeblocks, odd size
    (2112, 1, 3, 288, 0),   # three codeblocks, last chunk full
    (2112, 1, 3, 288, 3),   # the same at an odd offset (chunk by chunk from memory)
    (3144, 1, 3, 384, 0),   # more codeblock CRC chunks than lanes, the last one partial
    (4092, 1, 4, 384, 0),   # just below the limit, last chunk partial
    (4096, 1, 4, 384, 0),   # at the limit: every lane two full chunks
    (4097, 1, 4, 384, 0),   # just above, size no multiple of 4
    (4100, 1, 4, 384, 0),   # just above, size and offset multiples of 4
    (960, 2, 3, 288, 0),    # BG2 segmented
    (1912, 2, 5, 320, 0),   # BG2, five codeblocks
]


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


@pytest.fixture(scope="module")
def cases():
    """TBs, configurations and the oracle's codewords, computed once."""
    import srsgpu
    from srsgpu import sch
    orc = Oracle()
    rng = np.random.default_rng(4242)
    tbs, cfgs, want = [], [], []
    for nb, bg, nof_cbs, z, _ in SHAPES:
        nsym = _nof_ch_symbols(nb, 8, 4, nof_cbs)
        seg = sch.segment(nb * 8, bg, 8, 4, nsym)
        assert (seg.nof_segments, seg.lifting_size) == (nof_cbs, z), (nb, bg, seg.nof_segments, seg.lifting_size)
        assert all(cb.rm_length % 32 == 0 for cb in seg.codeblocks), (nb, bg)
        tb = rng.integers(0, 256, nb).astype(np.uint8)
        cw, _, _ = oracle_pdsch_encode(orc, tb, bg, 0, 8, 4, 0, nsym)
        tbs.append(tb)
        cfgs.append(srsgpu.PdschTransportBlock(bg, 0, 8, 4, nsym))
        want.append(cw)
    return tbs, cfgs, want


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["%d-bg%d-%dcb-z%d-o%d" % s for s in SHAPES])
def test_pdsch_encoder_crc_one_tb(ctx, cases, i):
    """One TB per plan, at its offset modulo 4."""
    tbs, cfgs, want = cases
    got, _, _ = _encode_plan(ctx, [tbs[i]], [cfgs[i]], [SHAPES[i][4]], 0)
    assert np.array_equal(got[0], want[i]), SHAPES[i]


def test_pdsch_encoder_crc_mixed_plan(ctx, cases):
    """All of them in one plan: both CRC polynomials of the TB, preloaded and chunk-by-chunk TB CRCs, carriers and
    other codeblocks, packed and byte kernel in the same launches."""
    tbs, cfgs, want = cases
    got, _, _ = _encode_plan(ctx, tbs, cfgs, [s[4] for s in SHAPES], 0)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (i, SHAPES[i])
