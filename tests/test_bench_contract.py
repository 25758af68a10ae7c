"""bench.py's accounting on the CPU (no GPU): the algorithmic bytes it
prices the roofline with match BASELINE.md's table, the per-octave split sums
to the pass, the metric label follows BASELINE.json for the metric's
configuration, and the host-core parsing tolerates OpenMP list values;
--dump-outputs writes the records exactly.  On the GPU: one plain run on a
small image (the result line's fields, the dumped keypoint list)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("W,H,O,gb", [(1920, 1080, 4, 0.669), (3840, 2160, 4, 2.677), (7680, 4320, 6, 10.75)])
def test_alg_bytes_match_baseline_table(W, H, O, gb):
    """BASELINE.md 'MI355X targets': B_alg = 4WH + sum 4P(S+3) + sum 4P(S+2)."""
    b = _bench()
    assert abs(b.alg_bytes(W, H, O, 5, False) / 1e9 - gb) < 0.006


def test_octave_bytes_sum_to_pass():
    b = _bench()
    for skip in (False, True):
        assert sum(b.octave_bytes(3840, 2160, 4, 5, skip)) == b.alg_bytes(3840, 2160, 4, 5, skip)
    assert b.oct0_bytes(3840, 2160, 5, False) == 2023833600


def test_metric_label_is_baselines_for_its_configuration():
    b = _bench()
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        metric = json.load(f)["metric"]
    assert b.metric_name(3840, 2160, 4, 5) == metric
    assert "1920x1080" in b.metric_name(1920, 1080, 4, 5, batch=8)


def _records(n, seed):
    import numpy as np
    import sift_amd
    rng = np.random.default_rng(seed)
    kp = np.zeros(n, dtype=sift_amd.KEYPOINT_DTYPE)
    for f in kp.dtype.names:
        kp[f] = rng.integers(0, 4000, n) if kp.dtype[f].kind == "i" else rng.standard_normal(n)
    return kp


def test_dump_outputs_is_exact_float64(tmp_path):
    """--dump-outputs: every field of every record, exactly, in list order."""
    import numpy as np
    b = _bench()
    kp = _records(1000, 1)
    counts = dict(candidates=1500, low_contrast=400, keypoints=1000, singular=0, exact=7)
    b.dump_outputs(str(tmp_path / "d"), kp, counts)
    a = np.load(tmp_path / "d" / "keypoints.npy")
    assert a.dtype == np.float64 and a.shape == (1000, len(kp.dtype.names))
    for j, f in enumerate(kp.dtype.names):
        assert (a[:, j] == kp[f]).all() and (a[:, j].astype(kp.dtype[f]) == kp[f]).all()
    assert (np.load(tmp_path / "d" / "keypoint_rows.npy") == np.arange(1000)).all()
    assert np.load(tmp_path / "d" / "counts.npy").tolist() == [1000, 1000, 1500, 400, 1000, 0, 7]


def test_dump_outputs_caps_with_a_fixed_sample(tmp_path, monkeypatch):
    """A list over the size cap is cut to the same rows on every run."""
    import numpy as np
    b = _bench()
    monkeypatch.setattr(b, "DUMP_CAP_BYTES", 64 * 300)
    kp = _records(1000, 2)
    rows = []
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), kp)
        r = np.load(tmp_path / d / "keypoint_rows.npy").astype(np.int64)
        a = np.load(tmp_path / d / "keypoints.npy")
        assert a.shape == (300, 8) and a.nbytes <= 64 * 300
        assert (np.diff(r) > 0).all() and 0 <= r[0] and r[-1] < 1000
        assert (a[:, 4] == kp["abs_x"][r]).all()
        assert np.load(tmp_path / d / "counts.npy").tolist() == [1000, 300]
        rows.append(r)
    assert (rows[0] == rows[1]).all()


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_keypoints(gpu_ctx, tmp_path):
    """A plain run on a small image: --steps sets the timed steps, what takes
    runs of its own stays null without --full, and --dump-outputs holds the
    keypoint list a synchronous detection of the same seeded image gives."""
    import subprocess
    import sys
    import numpy as np
    import sift_amd
    from sift_amd.synth import blob_image
    W, H, O, S = 160, 120, 4, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--width", str(W), "--height", str(H), "--octaves", str(O), "--scales", str(S),
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 4 and d["ms_per_step"] > 0 and d["full"] is False
    assert d["unit"] == "Mpix/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert abs(d["value"] - W * H / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * d["value"]
    for k in ("sustained", "verified", "roofline", "cpu_baseline", "cpu_baseline_all_cores", "cpu_baseline_js"):
        assert d[k] is None, k
    kp = gpu_ctx.detect(blob_image(W, H, seed=42), sift_amd.make_params(O, S))
    a = np.load(tmp_path / "out" / "keypoints.npy")
    assert a.dtype == np.float64 and a.shape == (kp.shape[0], 8) and kp.shape[0] == d["keypoints"] > 0
    for j, f in enumerate(kp.dtype.names):
        assert (a[:, j] == kp[f]).all(), f


def test_host_cores_parses_openmp_lists(monkeypatch):
    b = _bench()
    monkeypatch.setenv("OMP_NUM_THREADS", "8,2")
    assert 1 <= b.host_cores() <= 8
    monkeypatch.setenv("OMP_NUM_THREADS", "junk")
    assert b.host_cores() >= 1
