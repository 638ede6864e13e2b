"""bench.py's command line and its --dump-outputs writer, on host tensors (no GPU): a plain run is the default and
--full is opt-in; the dump is float32, whole for the small outputs, a fixed seeded sample for sample arrays that do not
fit, under 64 MB in all, and the same from call to call."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_is_the_default(bench):
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def _input_set(n_samples, n_dl=1):
    g = torch.Generator().manual_seed(5)
    ul = types.SimpleNamespace(d_tbs=torch.randint(0, 256, (1000,), generator=g, dtype=torch.uint8),
                               d_tb_ok=torch.tensor([1, 0, 1], dtype=torch.uint8))
    dls = [types.SimpleNamespace(d_samples=torch.randn(n_samples, generator=g)) for _ in range(n_dl)]
    return types.SimpleNamespace(ul=ul, dls=dls)


def test_dump_outputs_whole_when_they_fit(bench, tmp_path):
    st = _input_set(4096, n_dl=2)
    bench.dump_outputs(str(tmp_path), st, 0)
    assert sorted(os.listdir(tmp_path)) == ["dl_samples.npy", "dl_samples_1.npy", "ul_tb_ok.npy", "ul_tbs.npy"]
    for name, t in (("dl_samples", st.dls[0].d_samples), ("dl_samples_1", st.dls[1].d_samples),
                    ("ul_tbs", st.ul.d_tbs), ("ul_tb_ok", st.ul.d_tb_ok)):
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float32
        assert np.array_equal(a, t.numpy().astype(np.float32))


def test_dump_outputs_samples_a_large_output(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * (1003 + 500))  # the small outputs and 500 samples
    st = _input_set(4096)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), st, 0)
    a, b = np.load(tmp_path / "a" / "dl_samples.npy"), np.load(tmp_path / "b" / "dl_samples.npy")
    assert a.dtype == np.float32 and a.size == 500 and np.array_equal(a, b)
    idx = np.sort(np.random.default_rng(0).choice(4096, 500, replace=False))
    assert np.array_equal(a, st.dls[0].d_samples.numpy()[idx])
    assert sum(np.load(tmp_path / "a" / f).nbytes for f in os.listdir(tmp_path / "a")) <= bench.DUMP_MAX_BYTES
