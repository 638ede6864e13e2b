"""Cases and the checker of the PUSCH-plan-level decoder tests (tests/test_decoder_frontend_gpu.py and the plan-level part
of tests/test_ldpc_decoder_regimes_gpu.py): rate-matched lengths, codeblock configurations, LLRs, and _check_group, which
holds the fused plan to the unfused, pinned-split and pairs plans and to the CPU oracle composition."""
import numpy as np

from chain_lib import bits_to_llrs, oracle_pusch_cb_decode
from oracle_lib import BG_K, BG_N_SHORT, CRC24B


def _geometry(bg, Z, F):
    """(N, ninfo): HARQ buffer length and systematic positions without fillers."""
    return BG_N_SHORT[bg] * Z, (BG_K[bg] - 2) * Z - F


def _pick_E(bg, Z, qm, F, want=None, rate=0.6):
    """The smallest fusable rate-matched length (ninfo <= E <= N - F) of at least ninfo / rate LLRs that is a multiple of
    32 (256QAM: four symbols per lane) or 24 (64QAM: keeps the next codeblock's LLRs 8-byte aligned) and satisfies
    `want`."""
    N, ninfo = _geometry(bg, Z, F)
    step = 32 if qm == 8 else 24
    E = -(-int(ninfo / rate) // step) * step
    while E <= N - F:
        if want is None or want(E):
            return E
        E += step
    raise AssertionError("no rate-matched length for this case")


def _llrs(rng, E, good):
    """A noisy all-zero codeword (amplitude 10, sigma 4: decodes, its CRC passes) or pure noise (fails)."""
    return np.clip(np.round((10.0 if good else 0.0) + 4.0 * rng.standard_normal(E)), -127, 127).astype(np.int8)


def _payload_llrs(orc, rng, bg, Z, qm, E, F):
    """A noisy codeword of random payload bits with their CRC24B (the codeblock CRC of PuschCodeblock's default): unlike
    the all-zero codeword its CRC sum XORs table words of every column and its hard decisions are real bits."""
    L = BG_K[bg] * Z - F
    msg = np.zeros(BG_K[bg] * Z, np.uint8)
    msg[:L - 24] = rng.integers(0, 2, L - 24)
    c = orc.crc_bits(CRC24B, msg[:L - 24])
    msg[L - 24:L] = [(c >> (23 - i)) & 1 for i in range(24)]
    cw = orc.rate_match(bg, Z, 0, qm, 0, F, orc.ldpc_encode(bg, Z, msg), E)
    return bits_to_llrs(rng, cw, amp=10.0, noise=4.0)


def _case(srsgpu, shape, good, bg, Z, qm, E, F):
    """The decodable or the noise codeblock of a group's shape number `shape`: early stop on / off and 4 / 1 iterations by
    turns (with one iteration the hard decisions usually follow a failed CRC, also of a decodable codeblock; a quarter
    of the decodable ones get it)."""
    i = (0, 1, 0, 1, 2, 0, 1, 3)[shape % 8] if good else shape % 4
    early, max_iter = ((True, 4), (False, 4), (True, 1), (False, 1))[i]
    return srsgpu.PuschCodeblock(bg, Z, 0, qm, E, nof_filler_bits=F, new_data=True, use_early_stop=early,
                                 max_iterations=max_iter)


def _check_group(orc, ctx, cbs, llrs, seed, dec_type="avx2", mode=1, pairs=False):
    """Fused and unfused plans over a HARQ buffer of random old content against each other and the oracle; the fused plan
    with the kernel the host picks for so few codeblocks (the edge-split one) and with the one-row-pair kernel of large
    launches pinned (decoder_split=0); with `pairs` also the fused plan of two-codeblock workgroups (decoder_pairs=1,
    decoder_split=0: Z = 144..192 go to ldpc_decode_pairs_kernel). Returns the oracle's CRC outcomes."""
    import srsgpu
    rng = np.random.default_rng(seed)
    inits = [rng.integers(-127, 128, BG_N_SHORT[c.base_graph] * c.lifting_size).astype(np.int8) for c in cbs]
    init = np.concatenate(inits)
    dec = srsgpu.PuschCodeblockDecoder(ctx, dec_type)
    res_f, harq_f, crc_f = dec.decode(llrs, cbs, harq=init.copy())
    with ctx.options(decoder_split=0):
        res_p, harq_p, crc_p = dec.decode(llrs, cbs, harq=init.copy())
    with ctx.options(decoder_fused_dematch=0):
        res_u, harq_u, crc_u = dec.decode(llrs, cbs, harq=init.copy())
    others = [(res_p, harq_p, crc_p), (res_u, harq_u, crc_u)]
    if pairs:
        with ctx.options(decoder_pairs=1, decoder_split=0):
            others.append(dec.decode(llrs, cbs, harq=init.copy()))
    for _, harq_x, crc_x in others:
        assert np.array_equal(harq_f, harq_x)
        assert np.array_equal(np.asarray(crc_f), np.asarray(crc_x))
    off, oks = 0, []
    for i, (c, llr, h0) in enumerate(zip(cbs, llrs, inits)):
        r, bits, h2, ok = oracle_pusch_cb_decode(orc, mode, c, llr, h0, False)
        N = h0.size
        assert np.array_equal(harq_f[off:off + N], h2), (i, c)
        off += N
        for res in [res_f] + [o[0] for o in others]:
            r_g, bits_g = res[i]
            assert (r_g if r_g is not None else -1) == r, (i, c, r_g, r)
            if bits is not None:
                assert np.array_equal(bits_g, bits), (i, c)
        assert bool(crc_f[i]) == ok, (i, c)
        oks.append(bool(ok))
    assert any(oks) and not all(oks), oks
    return oks
