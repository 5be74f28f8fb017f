"""bench.py's plain run (no --full): the headline MSM stream alone, in its own
process at a reduced size (2^17 pairs).  The result line carries the headline
figure and none of the other legs, `--steps` is the number of timed steps, and
`--dump-outputs` writes the last timed step's result: the stream alternates
two scalar vectors (seeds 2 and 7), so step 4 of 4 ran the second, whose MSM
the C port recomputes here from the bench's own inputs."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_plain_run_dumps_last_step(tmp_path):
    import bench
    from oracle import cport
    cport.build()
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--log2n", "17",
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["metric"] == "Ristretto MSM scalar-point pairs/sec" and d["unit"] == "pairs/s"
    assert d["higher_is_better"] is True and d["steps"] == 4 and d["config"]["pairs"] == 1 << 17
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx((1 << 17) / (d["ms_per_step"] * 1e-3))
    for leg in ("cpu_baseline", "proofs", "verify_batch", "msm_2e22", "config2", "host_scalars", "stage_ms",
                "latency_ms_per_msm", "result_ok"):
        assert leg not in d
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["msm_result.npy"]
    got = np.load(tmp_path / "out" / "msm_result.npy")
    assert got.dtype == np.float32 and got.shape == (32,)
    n = 1 << 17
    want = cport.msm(bench.synth_scalars(n, 7), cport.from_uniform(bench.synth_point_bytes(n, 3)))
    assert got.astype(np.uint8).tobytes() == want
