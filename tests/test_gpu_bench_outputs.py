"""GPU: a plain `bench.py` run times exactly --steps steps, reports ms_per_step and none of the --full side readings, and
`--dump-outputs DIR` writes what the last timed step computed -- the same arrays run after run (seeded inputs, parity mode),
float32 / float64 only, at most 64 MB."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _bench(out_dir, steps):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--sustained", "0", "--dump-outputs", str(out_dir)],
                       cwd=str(ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_every_run(tmp_path):
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d, steps in zip(dirs, (3, 4)):
        line = _bench(d, steps)
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "actions/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert not {"sustained", "fast_mode", "also", "cpu_baseline", "parity_gate"} & set(line)
    N, D, K = 4096 * 128, 64, 1024                                   # the default workload, cfg2
    names = sorted(p.name for p in dirs[0].iterdir())
    assert names == ["code_usage.npy", "indices.npy", "z_latent.npy"]
    assert sum((dirs[0] / n).stat().st_size for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype in (np.float32, np.float64), n
        assert np.array_equal(a, b), f"{n} differs between two runs with the same arguments"
    idx, usage, zq = (np.load(dirs[0] / n) for n in ("indices.npy", "code_usage.npy", "z_latent.npy"))
    assert idx.shape == (N,) and usage.shape == (K,) and zq.shape[1] == D and 0 < zq.shape[0] < N
    assert np.array_equal(idx, np.round(idx)) and idx.min() >= 0 and idx.max() < K
    # the dumped histogram is the last timed step's: one count per row, at that row's code
    assert np.array_equal(np.bincount(idx.astype(np.int64), minlength=K), usage.astype(np.int64))
