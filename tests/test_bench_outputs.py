"""bench.py --dump-outputs: what the last timed step returned, written as DIR/<name>.npy so that two builds can be compared
output for output.  The writer is checked on the CPU; the bench run itself (same arguments twice -> same outputs, the
shapes, --steps) on the GPU."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def test_dump_outputs_writes_float64_and_ignores_itself(tmp_path):
    a = np.arange(12, dtype=np.int32).reshape(3, 4)
    bench.dump_outputs(tmp_path / "d", {"x": a, "y": np.array([7], np.int32)})
    x = np.load(tmp_path / "d" / "x.npy")
    assert x.dtype == np.float64 and x.shape == (3, 4) and np.array_equal(x, a)
    assert np.load(tmp_path / "d" / "y.npy").tolist() == [7.0]
    assert (tmp_path / "d" / ".gitignore").read_text() == "*\n"
    bench.dump_outputs(tmp_path / "d", {"x": a}, "_rank1")
    assert np.array_equal(np.load(tmp_path / "d" / "x_rank1.npy"), a)


def test_dump_outputs_samples_what_exceeds_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1600)            # share per array: 400 bytes = 50 float64
    a = np.arange(1000, dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, {"big": a, "small": a[:10]})
    for d in ("a", "b"):                                             # a fixed sample: the same every time
        idx = np.load(tmp_path / d / "big_sample_index.npy")
        big = np.load(tmp_path / d / "big.npy")
        assert idx.shape == (50,) and np.all(np.diff(idx) > 0) and np.array_equal(big, a[idx.astype(np.int64)])
        assert np.array_equal(np.load(tmp_path / d / "small.npy"), a[:10])
        assert not (tmp_path / d / "small_sample_index.npy").exists()
    assert np.array_equal(np.load(tmp_path / "a" / "big_sample_index.npy"), np.load(tmp_path / "b" / "big_sample_index.npy"))
    total = sum(f.stat().st_size for f in (tmp_path / "a").glob("*.npy"))
    assert total <= 1600 + 3 * 128                                   # + the .npy headers


def test_steps_below_one_is_refused():
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--steps" in p.stderr


def _bench(out_dir, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--batch", "3", "--prompt", "64",
                        "--gen", "5", "--warmup", "0", "--no-cpu-baseline", "--dump-outputs", str(out_dir), *extra],
                       capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return lines[0], {f.stem: np.load(f) for f in sorted(Path(out_dir).glob("*.npy"))}


@pytest.mark.gpu
@pytest.mark.parametrize("decode", ["fused", "stepwise", "sampled"])
def test_bench_dumps_the_same_outputs_for_the_same_arguments(gpu, tmp_path, decode):
    r1, o1 = _bench(tmp_path / "a", "--steps", "2", "--decode", decode)
    r2, o2 = _bench(tmp_path / "b", "--steps", "3", "--decode", decode)
    assert r1["steps"] == 2 and r2["steps"] == 3
    assert sorted(o1) == ["decode_tokens", "prefill_next_token"]
    assert o1["prefill_next_token"].shape == (3,) and o1["decode_tokens"].shape == (5, 3)
    V = gpu.synth.FULL_CONFIGS["llama-3.2-1b"]["vocab_size"]
    for name, a in o1.items():
        assert a.dtype == np.float64 and np.all(a == np.round(a)) and a.min() >= 0 and a.max() < V, name
        assert np.array_equal(a, o2[name]), name                    # every step recomputes the same batch from scratch
