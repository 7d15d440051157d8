"""bench.py's headline run: `--steps` K scores K distinct matrices, a plain run does only the timed
work, `--full` adds the legs outside the headline, `--dump-outputs` writes the timed pass's results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the BLIP-2 shape's 588 prunable matrices: 39 ViT-g blocks of 4, 24 FlanT5 encoder blocks of 7,
# 24 decoder blocks of 11
BLOCK_STARTS = ([4 * i for i in range(39)] + [156 + 7 * i for i in range(24)]
                + [324 + 11 * i for i in range(24)])


def test_strided_sample_is_k_distinct_matrices_for_every_k():
    import bench
    for k in range(1, 589):
        ids = bench.strided(588, k, block_starts=BLOCK_STARTS)
        assert len(ids) == k and len(set(ids)) == k, k
        assert all(0 <= i < 588 for i in ids), k


def test_strided_headline_sample_is_runs_of_six_at_block_starts():
    import bench
    assert bench.strided(588, 20, block_starts=BLOCK_STARTS) == (
        list(range(72, 78)) + list(range(212, 218)) + list(range(357, 363)) + [500, 501])


def _bench(args, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--toy",
                        "--steps", "4", "--warmup", "1"] + args, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _arrays(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_run_dumps_reproducible_outputs_and_full_adds_the_extra_legs(tmp_path):
    d1, d2 = tmp_path / "a", tmp_path / "b"
    line = _bench(["--dump-outputs", str(d1)])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 4 and len(set(line["config"]["layers_timed"])) == 4
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert "cpu_baseline" not in line and "z_modes" not in line
    a = _arrays(d1)
    assert set(a) == {"sparsity", "importance", "loss_table", "weights_sample"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(os.path.join(d1, f)) for f in os.listdir(d1)) <= 64 << 20
    assert a["sparsity"].shape == (4,) and a["importance"].shape == (4,)
    assert a["weights_sample"].shape[0] == 4 and np.isfinite(a["loss_table"]).all()
    # the same arguments: the same inputs, the same outputs
    _bench(["--dump-outputs", str(d2)])
    b = _arrays(d2)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    full = _bench(["--full"])
    assert "cpu_baseline" in full and "z_modes" in full
    assert full["roofline"]["box_fill_gbs"] > 0
