"""bench.py as a caller runs it: a plain run (no --full) at the reduced size, in fresh child processes, with --dump-outputs."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _bench(out: Path, steps: int, warmup: int):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--tiny", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), {f.stem: np.load(f) for f in out.glob("*.npy")}


def test_plain_bench_line_and_dumped_outputs(dev, tmp_path):
    """The line of a plain run carries the headline fields and none of the --full measurements, and --dump-outputs writes the last step's
    arrays.  The dump is the state after warmup + steps steps on seeded inputs, and every gradient is accumulated in a fixed order: 1 + 3 and
    2 + 2 steps in two processes write the same predictions, parameters and gradients bit for bit (the loss sum, which feeds nothing, is
    accumulated by float atomics and may differ in rounding)."""
    line, a = _bench(tmp_path / "a", steps=3, warmup=1)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["unit"] == "samples/s" and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1e3 * line["config"]["global_batch"] / line["ms_per_step"], rel=1e-9)
    assert line["roofline"] is None and line["inference_batch1"] is None and line["cpu_baseline"] is None and line["measured_baselines"] is None
    assert sorted(a) == ["grads", "loss_sum", "params", "pred"] and all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["pred"].size == 8 * 8 * 7 and np.abs(a["grads"]).max() > 0
    _, b = _bench(tmp_path / "b", steps=2, warmup=2)
    for k in ("pred", "params", "grads"):
        assert np.array_equal(a[k], b[k]), f"{k} differs between two processes after the same 4 steps"
    np.testing.assert_allclose(a["loss_sum"], b["loss_sum"], rtol=1e-6)
