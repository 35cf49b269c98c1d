"""bench.py's own options: --dump-outputs (what the timed path returned in its last step, as .npy files) and the plain run that
does only what the headline line needs (every untimed leg is behind --full).  The GPU test starts bench.py as a child process;
this module makes no GPU call itself."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def load_bench(monkeypatch):
    # bench.py sets OPENBLAS_NUM_THREADS at import: keep that out of this session's environment
    monkeypatch.setenv("OPENBLAS_NUM_THREADS", os.environ.get("OPENBLAS_NUM_THREADS", "1"))
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample(tmp_path, monkeypatch):
    b = load_bench(monkeypatch)
    small = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    dbl = torch.linspace(0, 1, 5, dtype=torch.float64)
    half = torch.full((3,), 0.5, dtype=torch.float16)
    big = torch.randn(b.DUMP_MAX_ELEMENTS + 1001, generator=torch.Generator().manual_seed(3))
    b.dump_outputs(str(tmp_path / "a"), {"small": small, "dbl": dbl, "half": half, "big": big})
    b.dump_outputs(str(tmp_path / "b"), {"big": big})
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (2, 3, 4) and np.array_equal(s, small.numpy())
    d = np.load(tmp_path / "a" / "dbl.npy")
    assert d.dtype == np.float64 and np.array_equal(d, dbl.numpy())
    h = np.load(tmp_path / "a" / "half.npy")
    assert h.dtype == np.float32 and np.array_equal(h, np.full(3, 0.5, np.float32))
    # a larger array: DUMP_MAX_ELEMENTS positions drawn from seed 0, the same in every run
    ba, bb = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    idx = np.sort(np.random.Generator(np.random.PCG64(0)).integers(0, big.numel(), b.DUMP_MAX_ELEMENTS))
    assert ba.dtype == np.float32 and ba.shape == (b.DUMP_MAX_ELEMENTS,) and np.array_equal(ba, bb)
    assert np.array_equal(ba, big.numpy()[idx])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20


def test_bench_lists_full_and_dump_outputs():
    p = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout and "--steps" in p.stdout


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, BENCH, "--steps", "3", "--warmup", "1", "--spinup-s", "0.05", "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=500)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[:600]
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["unit"] == "MP/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["ms_per_step"] > 0 and rec["value"] == pytest.approx(10 * 1024 * 1024 / 1e6 / (rec["ms_per_step"] * 1e-3), rel=1e-2)
    assert rec["flags"] & 3 == 0
    assert not {"roofline", "trace", "cpu_baseline", "parity", "soak", "one_stream", "dropin_api", "latency_ms_p50"} & rec.keys()
    st = np.load(out / "stack.npy")
    assert st.dtype == np.float32 and st.shape == (1 << 22,) and np.isfinite(st).all() and float(np.abs(st).mean()) > 0.05
