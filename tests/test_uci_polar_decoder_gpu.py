"""GPU parity of the polar-coded UCI decoder (srsgpu_uci_polar_decoder_plan through the C ABI) against the reference's
own decoder outputs (tests/golden/uci_polar.npz) and against the restatement tests/uci_polar_cases.py, which
tests/test_uci_polar_oracle.py pins to that fixture. Integer decoding: every comparison is exact, bits and status, and
no field is left out."""
import numpy as np
import pytest

import uci_polar_cases as C
import ulsch_demux_oracle as U
from ulsch_demux_cases import nof_llrs, random_config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


def nof_words(a):
    return (a + 31) // 32


def run_plan(ctx, fields, rng, gaps=True):
    """Decodes fields = [(llrs, A, ...)] in ONE plan: the fields spread over the three sources at unaligned offsets,
    0x55 guard bytes around each, the output words of some fields adjacent and of others a word apart (gaps=False: all
    adjacent), outputs pre-filled. Returns (bits list, valid list) after checking that only the planned words and
    status bytes were written."""
    import srsgpu
    import torch
    dev = torch.device("cuda", ctx.device)
    streams, cfgs, sizes, word = [[], [], []], [], [0, 0, 0], 3
    for i, f in enumerate(fields):
        s = i % 3
        guard = int(rng.integers(1, 8))
        streams[s].append(np.full(guard, 0x55, np.int8))
        sizes[s] += guard
        word += int(rng.integers(0, 2)) if gaps else 0
        cfgs.append((f[1], s, len(f[0]), sizes[s], word))
        word += nof_words(f[1])
        streams[s].append(np.asarray(f[0], np.int8))
        sizes[s] += len(f[0])
    d_src = [torch.from_numpy(np.concatenate(s + [np.full(9, 0x55, np.int8)])).to(dev) for s in streams]
    plan = srsgpu.UciPolarDecoderPlan(ctx, cfgs)
    assert plan.nof_msg_words == word
    n = len(fields)
    d_msgs = torch.full((word + 5,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    d_status = torch.full((n + 8,), 0xa5, dtype=torch.uint8, device=dev)
    plan.execute(d_src[0], d_src[1], d_src[2], d_msgs, d_status[4:])
    torch.cuda.synchronize(dev)
    msgs, status = d_msgs.cpu().numpy().view(np.uint32), d_status.cpu().numpy()
    plan.close()
    planned = np.zeros(word + 5, bool)
    for c in cfgs:
        planned[c[4]: c[4] + nof_words(c[0])] = True
    assert np.all(msgs[~planned] == 0x5a5a5a5a)
    assert np.all(status[:4] == 0xa5) and np.all(status[n + 4:] == 0xa5)
    status = status[4: n + 4]
    assert np.all(status <= 1)
    for c in cfgs:  # the last word whole, zeros above bit A - 1
        assert c[0] % 32 == 0 or int(msgs[c[4] + nof_words(c[0]) - 1]) >> (c[0] % 32) == 0
    return [srsgpu.uci_polar_unpack(msgs, c[4], c[0]) for c in cfgs], [bool(v) for v in status]


def assert_equals_restatement(ctx, fields, rng, gaps=True):
    bits, valid = run_plan(ctx, fields, rng, gaps)
    want = [C.decode(f[0], f[1]) for f in fields]
    for i, (f, b, v, w) in enumerate(zip(fields, bits, valid, want)):
        assert v == w[1] and np.array_equal(b, w[0]), (i, f[1], len(f[0]), v, w[1], w[2])
    return want


def test_uci_polar_decoder_golden(ctx):
    """The reference's own decoder outputs, every field of the fixture in one plan; codeblock 1's bits where the
    reference wrote them."""
    fields = list(C.golden_fields())
    bits, valid = run_plan(ctx, fields, np.random.default_rng(1))
    for i, (f, b, v) in enumerate(zip(fields, bits, valid)):
        wrote = f[2] != C.UNTOUCHED
        assert v == f[3] and np.array_equal(b[wrote], f[2][wrote]), (i, f[1], len(f[0]), v, f[3])


def test_uci_polar_decoder_shapes(ctx):
    """The smallest shapes where the kernel can go wrong (uci_polar_cases.shape_sizes, whose coverage
    test_uci_polar_oracle.py::test_generator_shapes asserts), one plan."""
    rng = np.random.default_rng(101)
    fields = C.shape_fields(rng)
    want = assert_equals_restatement(ctx, fields, rng)
    assert any(w[1] for w in want) and not all(w[1] for w in want)


def test_uci_polar_decoder_shared_words(ctx):
    """Two-codeblock fields whose codeblock boundary falls inside an output word, every field's words adjacent to its
    neighbours'."""
    rng = np.random.default_rng(102)
    sizes = [(361, 1089), (12, 40), (777, 1999), (1013, 2400), (40, 100), (1705, 4000), (360, 1088), (33, 90),
             (1025, 2300), (64, 200)]
    assert sum(C.nof_codeblocks(a, e) == 2 and (a // 2) % 32 != 0 for a, e in sizes) >= 5
    fields = [C.noisy_field(rng, a, e, 60) for a, e in sizes]
    want = assert_equals_restatement(ctx, fields, rng, gaps=False)
    assert all(w[1] for w in want) and all(np.array_equal(w[0], f[2]) for f, w in zip(fields, want))


def test_uci_polar_decoder_noise_mix(ctx):
    """Codewords at several amplitudes with N(0, 20^2) noise: 20-80 % valid in every size class, and two-codeblock
    fields where only codeblock 0 fails, only codeblock 1 fails and both pass."""
    rng = np.random.default_rng(91)
    fields = C.noise_fields(rng)
    partial = C.partial_failure_fields(np.random.default_rng(92))
    want = assert_equals_restatement(ctx, fields + partial, rng)
    shares = C.valid_shares(fields, want[: len(fields)])
    assert all(0.2 <= s <= 0.8 for s in shares), shares
    assert {tuple(w[2]) for w in want[len(fields):]} == {(False, True), (True, False), (True, True)}


def test_uci_polar_decoder_ties_and_saturation(ctx):
    """LLRs in {-1, 0, 1} and all-zero fields (the hard decision of 0 is bit 1); all +-120 fields with E >= 4 N
    (promotion to +-127, the special sums in order); and an order-dependent repetition pattern."""
    rng = np.random.default_rng(103)
    fields = C.tie_fields(rng) + C.saturation_fields(rng)
    # Position 5 of the de-interleaved block of an 18-in-768 code receives (100, 100, -100): 127 in the reference's
    # order, 100 in the reverse one (asserted on the CPU); every other LLR is +-3, so the decoding depends on it.
    assert C.accumulate([100, 100, -100]) != C.accumulate([100, 100, -100], reverse=True)
    for seed in range(4):
        llrs, a, _ = C.noisy_field(np.random.default_rng(seed), 12, 768, 3, sigma=1.0)
        e = np.zeros(768, np.int64)
        e[C.channel_interleaver(768)] = llrs
        for p in range(0, 256, 7):
            e[[p, p + 256, p + 512]] = (100, 100, -100)
        fields.append((e[C.channel_interleaver(768)].astype(np.int8), a, None))
    want = assert_equals_restatement(ctx, fields, rng)
    zero = [w for f, w in zip(fields, want) if not np.any(f[0])]
    assert zero and not any(w[1] for w in zero)


def test_uci_polar_decoder_sharing(ctx):
    """64 fields of the same (K, E), 64 all different, and both mixed, in one plan each: the results equal the one-field
    plans (and the restatement)."""
    rng = np.random.default_rng(104)
    same = [C.noisy_field(rng, 48, 576, 10) for _ in range(64)]
    different = [C.noisy_field(rng, 12 + 5 * i, 150 + 31 * i, 12) for i in range(64)]
    assert len({(f[1], len(f[0])) for f in different}) == 64
    mixed = [f for pair in zip(same[:32], different[:32]) for f in pair]
    alone = {}
    for f in same + different:
        b, v = run_plan(ctx, [f], rng)
        alone[id(f)] = (b[0], v[0])
    for group in (same, different, mixed):
        bits, valid = run_plan(ctx, group, rng)
        for f, b, v in zip(group, bits, valid):
            assert v == alone[id(f)][1] and np.array_equal(b, alone[id(f)][0])
    want = [C.decode(f[0], f[1]) for f in same + different]
    assert all(w[1] == alone[id(f)][1] and np.array_equal(w[0], alone[id(f)][0]) for f, w in zip(same + different, want))
    assert 0 < sum(w[1] for w in want) < len(want)


def test_uci_polar_decoder_decode_batch(ctx):
    """The one-shot binding (UciPolarDecoder.decode_batch) over the slot-shaped batch."""
    import srsgpu
    fields = C.slot_batch_fields(np.random.default_rng(105), nof_ues=8)
    bits, valid = srsgpu.UciPolarDecoder(ctx).decode_batch([f[0] for f in fields], [f[1] for f in fields])
    for f, b, v in zip(fields, bits, valid):
        w = C.decode(f[0], f[1])
        assert np.array_equal(b, w[0]) and v == w[1]
        assert np.array_equal(b, f[2]) and v


def to_demux(cfg, c2b, c2e, c_init):
    import srsgpu
    return srsgpu.UlschDemultiplexing(
        modulation_order=cfg["qm"], nof_layers=cfg["nof_layers"], nof_prb=cfg["nof_prb"],
        start_symbol=cfg["start_symbol"], nof_symbols=cfg["nof_symbols"], dmrs_symbol_mask=cfg["dmrs_symbol_mask"],
        dmrs_type=2 if cfg["dmrs_type2"] else 1, nof_cdm_groups_without_data=cfg["nof_cdm_groups_without_data"],
        rnti=c_init >> 15, n_id=c_init & 0x7fff, nof_harq_ack_rvd=cfg["nof_harq_ack_rvd"],
        nof_harq_ack_bits=cfg["nof_harq_ack_bits"], nof_enc_harq_ack_bits=cfg["nof_enc_harq_ack_bits"],
        nof_csi_part1_bits=cfg["nof_csi_part1_bits"], nof_enc_csi_part1_bits=cfg["nof_enc_csi_part1_bits"],
        nof_csi_part2_bits=c2b, nof_enc_csi_part2_bits=c2e)


KINDS = ("harq", "csi1", "csi2")


def polar_fields_of(cfg, c2b, c2e):
    """(source, kind, A, E) of the transmission's polar-coded fields that pass the plan's validation."""
    sizes = ((cfg["nof_harq_ack_bits"], cfg["nof_enc_harq_ack_bits"]),
             (cfg["nof_csi_part1_bits"], cfg["nof_enc_csi_part1_bits"]), (c2b, c2e))
    return [(s, KINDS[s], a, e) for s, (a, e) in enumerate(sizes) if a >= 12 and C.field_refusal(a, e) is None]


def chain_transmissions(rng, count):
    """random_config transmissions with at least one polar-coded field (20-bit HARQ-ACK, 30-bit CSI Part 1, 40-bit CSI
    Part 2) that passes the plan's validation."""
    out = []
    while len(out) < count:
        cfg, c2b, c2e, _ = random_config(rng)
        if polar_fields_of(cfg, c2b, c2e):
            c_init = int(rng.integers(0, 1 << 16)) << 15 | int(rng.integers(0, 1024))
            out.append((cfg, c2b, c2e, c_init))
    return out


def chain_codeword(rng, cfg, c2b, c2e, amp=60):
    """Codeword LLRs (descrambled, as the demodulator writes them) of a transmission whose polar-coded UCI fields carry
    random messages encoded by the restatement's encoder; everything else is noise. Returns (llrs, sent by kind)."""
    lq = cfg["qm"] * cfg["nof_layers"]
    n = nof_llrs(cfg)
    llrs = np.clip(np.rint(rng.normal(0.0, 20.0, n)), -120, 120)
    where = {k: [] for k in KINDS}
    pos = 0
    for _l, M, sets in U.symbol_plan(cfg, c2e):
        for kind in where:
            for r in sets[kind]:
                where[kind].extend(range(pos + r * lq, pos + (r + 1) * lq))
        pos += M * lq
    sent = {}
    for _s, kind, a, e in polar_fields_of(cfg, c2b, c2e):
        idx = np.array(where[kind])
        assert idx.size == e
        bits = rng.integers(0, 2, a).astype(np.uint8)
        x = 1 - 2 * C.encode(bits, e).astype(np.float64)
        llrs[idx] = np.clip(np.rint(amp * x + rng.normal(0.0, 20.0, e)), -120, 120)
        sent[kind] = bits
    return llrs.astype(np.int8), sent


def test_uci_polar_decoder_chains_after_demultiplexer(ctx):
    """The demultiplexer plan runs straight into the polar plan on its output buffers (sources 0 / 1 / 2 = d_harq /
    d_csi1 / d_csi2 at the demultiplexer's offsets): eager, then a captured graph replayed on the same inputs and on
    fresh ones. The decoded bits equal the sent ones at amplitude 60 and the replays equal the eager runs."""
    import srsgpu
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(106)
    txs = chain_transmissions(rng, 24)
    offs = np.concatenate([[0], np.cumsum([nof_llrs(t[0]) for t in txs])]).astype(int)
    demux = srsgpu.UlschDemuxPlan(ctx, [to_demux(*t) for t in txs], [int(o) for o in offs[:-1]])
    fields, owners = [], []
    for i, (cfg, c2b, c2e, _c) in enumerate(txs):
        for s, kind, a, e in polar_fields_of(cfg, c2b, c2e):
            fields.append((a, s, e, demux.offsets[kind][i], None))
            owners.append((i, kind))
    assert {f[0] for f in fields} == {20, 30, 40}
    uci = srsgpu.UciPolarDecoderPlan(ctx, fields)

    def inputs():
        cws, sent = zip(*[chain_codeword(rng, t[0], t[1], t[2]) for t in txs])
        return torch.from_numpy(np.concatenate(cws)).to(dev), [sent[i][kind] for i, kind in owners]

    d_in = torch.zeros(int(offs[-1]), dtype=torch.int8, device=dev)
    outs = {k: torch.zeros(max(demux.totals[k], 4), dtype=torch.int8, device=dev) for k in demux.totals}
    d_msgs = torch.zeros(uci.nof_msg_words, dtype=torch.int32, device=dev)
    d_status = torch.zeros(len(fields), dtype=torch.uint8, device=dev)

    def pipeline():
        demux.execute(d_in, outs["sch"], outs["harq"], outs["csi1"], outs["csi2"])
        uci.execute(outs["harq"], outs["csi1"], outs["csi2"], d_msgs, d_status)

    def result():
        torch.cuda.synchronize(dev)
        got = (d_msgs.cpu().numpy().view(np.uint32).copy(), d_status.cpu().numpy().copy())
        d_msgs.fill_(-1)
        d_status.fill_(7)
        return got

    def check_sent(got, sent):
        for f, w, v, bits in zip(fields, uci.msg_word_offsets, got[1], sent):
            assert v == 1 and np.array_equal(srsgpu.uci_polar_unpack(got[0], w, f[0]), bits), (f, v)

    first, sent_first = inputs()
    second, sent_second = inputs()
    d_in.copy_(first)
    pipeline()
    eager_first = result()
    check_sent(eager_first, sent_first)
    d_in.copy_(second)
    pipeline()
    eager_second = result()
    check_sent(eager_second, sent_second)
    assert not np.array_equal(eager_first[0], eager_second[0])
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pipeline()
    result()  # the capture does not execute; clear again
    for src, eager in ((first, eager_first), (second, eager_second)):
        d_in.copy_(src)
        graph.replay()
        got = result()
        assert np.array_equal(got[0], eager[0]) and np.array_equal(got[1], eager[1])
    uci.close()
    demux.close()


def test_uci_polar_decoder_rejections(ctx):
    """Plan creation refuses what the reference's assertions refuse, and says why; the two plans split the sizes at
    11 / 12 bits."""
    import srsgpu
    good = (20, 0, 240, 0, 0)
    for field, text in (((11, 0, 64, 0, 4), "nof_bits"), ((0, 0, 64, 0, 4), "nof_bits"), ((1707, 0, 16384, 0, 4), "nof_bits"),
                        ((20, 3, 240, 0, 4), "source"), ((20, 0, 8193, 0, 4), "8192 encoded bits"),
                        ((1706, 0, 16386, 0, 4), "8192 encoded bits"),
                        ((12, 0, 21, 0, 4), "K . nPC"), ((20, 0, 31, 0, 4), "K . nPC"), ((1012, 0, 1023, 0, 4), "K . nPC"),
                        ((20, 0, 0, 0, 4), "K . nPC"), ((1013, 0, 1036, 0, 4), "K . nPC"),
                        ((20, 0, 240, 0, 0), "overlap"), ((40, 1, 240, 0, 0), "overlap")):
        with pytest.raises(srsgpu.SrsGpuError, match=text) as err:
            srsgpu.UciPolarDecoderPlan(ctx, [good, field])
        assert "field" in str(err.value)
    # A 33-bit field owns two words: the next field may start at word 2, not at word 1.
    with pytest.raises(srsgpu.SrsGpuError, match="overlap"):
        srsgpu.UciPolarDecoderPlan(ctx, [(33, 0, 240, 0, 0), (20, 0, 240, 0, 1)])
    srsgpu.UciPolarDecoderPlan(ctx, [(33, 0, 240, 0, 0), (20, 0, 240, 0, 2), (12, 2, 22, 0, 3)]).close()
    srsgpu.UciPolarDecoderPlan(ctx, []).close()
    with pytest.raises(srsgpu.SrsGpuError, match="polar"):
        srsgpu.UciDecoderPlan(ctx, [(12, 2, 0, 64, 0)])
    srsgpu.UciDecoderPlan(ctx, [(11, 2, 0, 64, 0)]).close()
