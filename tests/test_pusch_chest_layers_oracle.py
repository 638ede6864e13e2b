"""The float64 restatement of 2-4 layer PUSCH channel estimation (oracle/pusch_chest_oracle.py estimate_layers) checked
on its own, without the kernel: it is the single-layer restatement for one layer, it recovers frequency-flat noise-free
channels exactly (the cover-code removal assumes exactly that), and on the inputs of the GPU suite's true-channel test
it stays below that test's -15 dB bound. The GPU tests then hold the kernel to it
(tests/test_pusch_chest_gpu.py::test_pusch_chest_multilayer_vs_oracle)."""
import itertools

import numpy as np
import pytest

import pusch_chest_oracle as C
from ofdm_oracle import bf16_to_complex
from pusch_chest_cases import multilayer_case, multilayer_tx, random_case, random_crb_mask


def test_one_layer_is_estimate():
    """estimate_layers(..., 1, ...) is estimate, bit for bit: 12 random_case inputs over every smoothing, both time
    strategies, CFO compensation on / off, two of them CRB-masked."""
    rng = np.random.default_rng(5)
    for i in range(12):
        mask = random_crb_mask(rng, 24) if i % 6 == 5 else None
        cfg, grid, _ = random_case(rng, 24, cfo_hz=rng.uniform(-1500, 1500), delay=rng.uniform(-20, 20), crb_mask=mask)
        fd, td, comp = ["none", "mean", "filter"][i % 3], ["average", "interpolate"][i % 2], bool((i // 2) % 2)
        y = bf16_to_complex(grid)
        ch, nv, rsrp, epre, ex = C.estimate(cfg, y, fd, td, comp, 1, mask)
        chl, nvl, rsrpl, eprel, exl = C.estimate_layers(cfg, y, 1, fd, td, comp, 1, mask)
        assert chl.shape == (1,) + ch.shape
        assert np.array_equal(chl[0], ch)
        assert np.array_equal(nvl, nv) and np.array_equal(rsrpl, rsrp) and np.array_equal(eprel, epre)
        assert np.array_equal(exl["ta_s"], ex["ta_s"])
        assert np.array_equal(exl["cfo_hz"], ex["cfo_hz"], equal_nan=True)
        assert np.array_equal(exl["cfo_hz_groups"], ex["cfo_hz"][None], equal_nan=True)


@pytest.mark.parametrize("L,t2", list(itertools.product([2, 3, 4], [0, 1])))
def test_flat_noise_free_recovery(L, t2):
    """A frequency-flat, noise-free channel per (layer, port), zero CFO: every layer's estimate is its channel
    coefficient within 1e-9 relative on every RE of the allocation, and the noise variance sits at its RSRP / 1e10
    floor (or below 1e-12 x EPRE). fd none / mean, and for type 1 the filter too (its virtual pilots extend a flat band
    exactly; 1-2 RB of type 2 hold fewer pilots than half the filter, whose edge taps then see zeros, as in the
    reference's 1-RB rule), both time strategies, 1 and 2 DM-RS symbols, 1 / 2 / 5 RB."""
    rng = np.random.default_rng(40 + 2 * L + t2)
    P = 3
    fds = ["none", "mean"] + ([] if t2 else ["filter"])
    for fd, td, dmrs_mask, nrb in itertools.product(fds, ["average", "interpolate"], [1 << 3, (1 << 2) | (1 << 9)],
                                                    [1, 2, 5]):
        cfg = dict(slot=int(rng.integers(0, 20)), scrambling_id=int(rng.integers(0, 65536)),
                   n_scid=int(rng.integers(0, 2)), dmrs_type2=t2, scaling=float(rng.choice([1.0, 1.4125375, 0.7071])),
                   dmrs_symbol_mask=dmrs_mask, start_symbol=1, nof_symbols=12, rb_start=int(rng.integers(0, 8 - nrb)),
                   nof_rb=nrb, nof_rx_ports=P)
        c = rng.normal(size=(L, P)) + 1j * rng.normal(size=(L, P))
        y = np.einsum("lp,lsk->psk", c, multilayer_tx(rng, cfg, L, 8))
        ch, nv, rsrp, epre, ex = C.estimate_layers(cfg, y, L, fd, td, False, 1, None)
        ks = slice(cfg["rb_start"] * 12, (cfg["rb_start"] + nrb) * 12)
        got = ch[:, :, 1:13, ks]
        assert np.max(np.abs(got - c[:, :, None, None]) / np.abs(c)[:, :, None, None]) < 1e-9, (fd, td, dmrs_mask, nrb)
        assert np.all((nv == rsrp / 1e10) | (nv < 1e-12 * epre)), (nv, rsrp, epre)
        np.testing.assert_allclose(rsrp, cfg["scaling"] ** 2 * np.abs(c[0]) ** 2, rtol=1e-9)
        assert ex["cfo_hz_groups"].shape == ((L + 1) // 2, P)


def test_filter_never_takes_more_virtual_pilots_than_pilots():
    """2 RB of type 2: 8 pilots under a 21-tap filter that asks for 10 virtual pilots per edge. The smoothing takes 8:
    a flat band comes back flat wherever every non-zero tap sees a pilot or a virtual pilot (the outermost taps, at
    t = +-1 of the raised cosine, are zero: pilots 1..6 of the span -8..15), symmetric about the band centre, and
    short of it at the two edge pilots (their taps past the virtual pilots see zeros, as with 1 RB)."""
    v = 0.6 - 0.3j
    out = C.fd_smoothing(np.full(8, v), 2, 1, "filter")
    assert out.shape == (8,)
    np.testing.assert_allclose(out[1:7], v, rtol=1e-12)
    np.testing.assert_allclose(out, out[::-1], rtol=1e-12)
    assert np.all(np.abs(out[[0, 7]]) < abs(v)) and np.all(np.abs(out) > 0.9 * abs(v))


@pytest.mark.parametrize("L", [2, 4])
def test_restatement_within_true_channel_bound(L):
    """The inputs of test_pusch_chest_multilayer (seeds 92 and 94): the restatement alone is within that test's
    -15 dB of the true channel on every layer."""
    rng = np.random.default_rng(90 + L)
    cfg, grid, H = multilayer_case(rng, 24, L, 4, 20, rb_start=2, dmrs_mask=(1 << 2) | (1 << 11))
    ch, nv, _, _, _ = C.estimate_layers(cfg, bf16_to_complex(grid), L, "filter", "average", False, 1, None)
    ks = slice(cfg["rb_start"] * 12, (cfg["rb_start"] + cfg["nof_rb"]) * 12)
    for ly in range(L):
        err = np.mean(np.abs(ch[ly][:, 5, ks] - H[ly][:, ks]) ** 2) / np.mean(np.abs(H[ly][:, ks]) ** 2)
        assert 10 * np.log10(err) < -15, (ly, 10 * np.log10(err))
    assert np.all(nv > 0)
