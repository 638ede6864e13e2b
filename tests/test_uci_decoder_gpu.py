"""GPU parity of the short-block UCI decoder (srsgpu_uci_decoder_plan through the C ABI) against the reference's own
detector outputs (tests/golden/uci_short_block.npz) and against the restatement tests/uci_cases.py, which
tests/test_uci_short_block_oracle.py pins to that fixture. Integer detection: every comparison is exact, bits and
validity, and no field is left out."""
import numpy as np
import pytest

import uci_cases as C
import ulsch_demux_oracle as U
import pusch_demod_oracle as D
from ulsch_demux_cases import nof_llrs, random_config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import srsgpu
    return srsgpu.Context(0)


def run_plan(ctx, fields, rng):
    """Decodes fields = [(llrs, A, Qm, ...)] in ONE plan: the fields spread over the three sources at unaligned
    offsets, 0x55 guard bytes around each, outputs pre-filled. Returns (bits list, valid list) after checking that only
    the planned output words were written."""
    import srsgpu
    import torch
    dev = torch.device("cuda", ctx.device)
    streams, cfgs = [[], [], []], []
    sizes = [0, 0, 0]
    for i, f in enumerate(fields):
        s = i % 3
        guard = int(rng.integers(1, 8))
        streams[s].append(np.full(guard, 0x55, np.int8))
        sizes[s] += guard
        cfgs.append((f[1], f[2], s, len(f[0]), sizes[s]))
        streams[s].append(np.asarray(f[0], np.int8))
        sizes[s] += len(f[0])
    d_src = [torch.from_numpy(np.concatenate(s + [np.full(9, 0x55, np.int8)])).to(dev) for s in streams]
    plan = srsgpu.UciDecoderPlan(ctx, cfgs)
    n = len(fields)
    d_msgs = torch.full((n + 8,), 0x5a5a, dtype=torch.int16, device=dev)
    d_status = torch.full((n + 8,), 0xa5, dtype=torch.uint8, device=dev)
    plan.execute(d_src[0], d_src[1], d_src[2], d_msgs[4:], d_status[4:])
    torch.cuda.synchronize(dev)
    msgs, status = d_msgs.cpu().numpy().view(np.uint16), d_status.cpu().numpy()
    plan.close()
    assert np.all(msgs[:4] == 0x5a5a) and np.all(msgs[n + 4:] == 0x5a5a)
    assert np.all(status[:4] == 0xa5) and np.all(status[n + 4:] == 0xa5)
    msgs, status = msgs[4: n + 4], status[4: n + 4]
    assert np.all(status <= 1) and all(int(m) >> f[1] == 0 for m, f in zip(msgs, fields))
    return [((int(m) >> np.arange(f[1])) & 1).astype(np.uint8) for m, f in zip(msgs, fields)], [bool(v) for v in status]


def assert_equals_restatement(ctx, fields, rng):
    bits, valid = run_plan(ctx, fields, rng)
    want = [C.detect(f[0], f[1], f[2]) for f in fields]
    for i, (f, b, v, w) in enumerate(zip(fields, bits, valid, want)):
        assert np.array_equal(b, w[0]) and v == w[1], (i, f[1], f[2], len(f[0]), b, v, w)
    return want


def test_uci_decoder_golden(ctx):
    """The reference's own detector outputs, every field of the fixture in one plan."""
    fields = list(C.golden_fields())
    bits, valid = run_plan(ctx, fields, np.random.default_rng(1))
    for i, (f, b, v) in enumerate(zip(fields, bits, valid)):
        assert np.array_equal(b, f[3]) and v == f[4], (i, f[1], f[2], len(f[0]), b, v, f[3], f[4])


def test_uci_decoder_random_vs_restatement(ctx):
    """770 fields in one plan: every A in 1..11 x every Qm x E in {below the minimum count, N - 1, N, N + 1, 2N, 2N + 5,
    32 * 40 + 7} x amplitudes 2 / 6 / 20 / 60 with N(0, 20^2) noise. For every A >= 3 at least 20 % of the fields must
    be valid and at least 20 % invalid (the reference gives 48-57 % valid with this mix)."""
    rng = np.random.default_rng(77)
    fields = C.random_fields(rng)
    want = assert_equals_restatement(ctx, fields, rng)
    for a in range(3, 12):
        share = np.mean([w[1] for f, w in zip(fields, want) if f[1] == a])
        assert 0.2 <= share <= 0.8, (a, share)


def test_uci_decoder_ties(ctx):
    """LLRs in {-1, 0, 1}: at least 20 % of the fields have several codewords at the winning metric, of which the
    lowest index and its sign must come out."""
    rng = np.random.default_rng(78)
    fields = C.tie_fields(rng)
    want = assert_equals_restatement(ctx, fields, rng)
    assert np.mean([w[2] for w in want]) >= 0.2
    for a in (3, 11):
        assert np.mean([w[2] for f, w in zip(fields, want) if f[1] == a]) >= 0.2


def test_uci_decoder_saturation_order(ctx):
    """The dematcher's sum saturates after every block: (100, 100, -100) -> 20, not 100; partial last blocks."""
    fields = C.saturation_fields()
    assert np.array_equal(C.rate_dematch(np.array([100, 100, -100]), 1), [20])
    assert_equals_restatement(ctx, fields, np.random.default_rng(79))


def test_uci_decoder_degenerate(ctx):
    """All-zero LLRs, E = 0, A <= 2 with E < Qm, cancelling 2-bit fields (all invalid) and perfectly correlated fields
    (zero GLRT denominator: valid)."""
    fields = C.degenerate_fields()
    want = assert_equals_restatement(ctx, fields, np.random.default_rng(80))
    assert not any(w[1] for w in want[:12]) and all(w[1] for w in want[12:])
    assert all(np.all(w[0] == 1) for w in want[:10]) and all(np.all(w[0] == 0) for w in want[10:12])


def test_uci_decoder_decode_batch(ctx):
    """The one-shot binding (UciDecoder.decode_batch) over the slot-shaped batch."""
    import srsgpu
    fields = C.slot_batch_fields(np.random.default_rng(81), nof_ues=8)
    bits, valid = srsgpu.UciDecoder(ctx).decode_batch([f[0] for f in fields], [f[1] for f in fields],
                                                      [f[2] for f in fields])
    for f, b, v in zip(fields, bits, valid):
        w = C.detect(f[0], f[1], f[2])
        assert np.array_equal(b, w[0]) and v == w[1]
        assert np.array_equal(b, f[3]) and v


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


def chain_transmissions(rng, count):
    """random_config transmissions whose HARQ-ACK and CSI Part 1 are short-block fields (<= 11 bits) of at least one
    whole block, with their demultiplexer configuration."""
    out = []
    while len(out) < count:
        cfg, c2b, c2e, _ = random_config(rng)
        ok = True
        for a, e in ((cfg["nof_harq_ack_bits"], cfg["nof_enc_harq_ack_bits"]),
                     (cfg["nof_csi_part1_bits"], cfg["nof_enc_csi_part1_bits"])):
            ok = ok and a <= 11 and (a == 0 or e >= max(C.block_length(a, cfg["qm"]), C.MIN_ENCODED_BITS[a - 1]))
        if ok and (cfg["nof_harq_ack_bits"] or cfg["nof_csi_part1_bits"]):
            c_init = int(rng.integers(0, 1 << 16)) << 15 | int(rng.integers(0, 1024))
            out.append((cfg, c2b, c2e, c_init))
    return out


def chain_codeword(rng, cfg, c2e, c_init, amp=60):
    """Codeword LLRs (descrambled, as the demodulator writes them) of a transmission that carries random HARQ-ACK and
    CSI Part 1 messages encoded by the restatement's encoder; everything else is noise. A placeholder "x" is sent as a
    scrambled 1 and "y" as the previous scrambled bit (TS 38.211 section 6.3.1.1), so after the receiver's
    descrambling they carry the scrambling sequence that the demultiplexer takes off again. Returns (llrs, sent)."""
    lq = cfg["qm"] * cfg["nof_layers"]
    n = nof_llrs(cfg)
    seq = D.gold_sequence(c_init, n).astype(np.int64)
    llrs = np.clip(np.rint(rng.normal(0.0, 20.0, n)), -120, 120)
    where = {"harq": [], "csi1": []}
    pos = 0
    for _l, M, sets in U.symbol_plan(cfg, c2e):
        for kind in where:
            for r in sets[kind]:
                where[kind].extend(range(pos + r * lq, pos + (r + 1) * lq))
        pos += M * lq
    sent = {}
    for kind, a in (("harq", cfg["nof_harq_ack_bits"]), ("csi1", cfg["nof_csi_part1_bits"])):
        if a == 0:
            continue
        idx = np.array(where[kind])
        bits = rng.integers(0, 2, a).astype(np.uint8)
        enc = C.encode(bits, cfg["qm"], idx.size)
        scrambled = np.where(enc == C.PLACEHOLDER_X, 1, enc.astype(np.int64) ^ seq[idx])
        for i in np.flatnonzero(enc == C.PLACEHOLDER_Y):
            scrambled[i] = scrambled[i - 1]
        noise = rng.normal(0.0, 20.0, idx.size)
        llrs[idx] = np.clip(np.rint(amp * (1 - 2 * scrambled) * (1 - 2 * seq[idx]) + noise), -120, 120)
        sent[kind] = bits
    return llrs.astype(np.int8), sent


def test_uci_decoder_chains_after_demultiplexer(ctx):
    """The demultiplexer plan runs straight into a UCI plan on its output buffers (sources 0 / 1 = d_harq / d_csi1 at
    the demultiplexer's offsets): eager, then a captured graph replayed on the same inputs and on fresh ones. The
    decoded bits equal the sent ones at amplitude 60 and the replays equal the eager runs."""
    import srsgpu
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(82)
    txs = chain_transmissions(rng, 24)
    offs = np.concatenate([[0], np.cumsum([nof_llrs(t[0]) for t in txs])]).astype(int)
    demux = srsgpu.UlschDemuxPlan(ctx, [to_demux(*t) for t in txs], [int(o) for o in offs[:-1]])
    fields, owners = [], []
    for i, (cfg, _c2b, _c2e, _c) in enumerate(txs):
        for s, kind, a, e in ((0, "harq", cfg["nof_harq_ack_bits"], cfg["nof_enc_harq_ack_bits"]),
                              (1, "csi1", cfg["nof_csi_part1_bits"], cfg["nof_enc_csi_part1_bits"])):
            if a:
                fields.append((a, cfg["qm"], s, e, demux.offsets[kind][i]))
                owners.append((i, kind))
    assert {f[0] for f in fields} >= {1, 2, 5, 7, 11}
    uci = srsgpu.UciDecoderPlan(ctx, fields)

    def inputs():
        cws, sent = zip(*[chain_codeword(rng, t[0], t[2], t[3]) for t in txs])
        return torch.from_numpy(np.concatenate(cws)).to(dev), [sent[i][kind] for i, kind in owners]

    d_in = torch.zeros(int(offs[-1]), dtype=torch.int8, device=dev)
    outs = {k: torch.zeros(max(demux.totals[k], 4), dtype=torch.int8, device=dev) for k in demux.totals}
    d_msgs = torch.zeros(len(fields), dtype=torch.int16, device=dev)
    d_status = torch.zeros(len(fields), dtype=torch.uint8, device=dev)

    def pipeline():
        demux.execute(d_in, outs["sch"], outs["harq"], outs["csi1"], outs["csi2"])
        uci.execute(outs["harq"], outs["csi1"], None, d_msgs, d_status)

    def result():
        torch.cuda.synchronize(dev)
        got = (d_msgs.cpu().numpy().view(np.uint16).copy(), d_status.cpu().numpy().copy())
        d_msgs.fill_(-1)
        d_status.fill_(7)
        return got

    def check_sent(got, sent):
        for f, m, v, bits in zip(fields, got[0], got[1], sent):
            assert int(m) == sum(int(b) << j for j, b in enumerate(bits)) and v == 1, (f, m, v, bits)

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
    assert any(a != b for a, b in zip(eager_first[0], eager_second[0]))
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


def test_uci_decoder_rejections(ctx):
    """Plan creation refuses what the kernel does not decode, and says why; a 12-bit field names the polar code."""
    import srsgpu
    for field, text in (((0, 2, 0, 32, 0), "nof_bits"), ((3, 3, 0, 32, 0), "modulation_order"),
                        ((3, 0, 0, 32, 0), "modulation_order"), ((3, 2, 3, 32, 0), "source"),
                        ((12, 2, 0, 64, 0), "polar"), ((40, 2, 0, 64, 0), "polar"),
                        ((3, 2, 0, (1 << 24) + 1, 0), "nof_enc_bits")):
        with pytest.raises(srsgpu.SrsGpuError, match=text):
            srsgpu.UciDecoderPlan(ctx, [(4, 2, 0, 32, 0), field])
    srsgpu.UciDecoderPlan(ctx, [(11, 8, 2, 0, 0)]).close()
