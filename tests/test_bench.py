"""bench.py's workload table and host-CPU accounting (CPU only: no GPU is touched)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_default_is_the_metric_workload():
    a = bench.parse([])
    assert (a.config, a.scene, a.width, a.height, a.method, a.photon_launch) == (
        2, "SyntheticHall", 1920, 1080, "ppm", 2048)
    assert a.scaling == "strong"


def test_configs_match_baseline():
    # BASELINE.json configs[0..4]
    want = {0: ("Cornell", 256, 256, "pt"), 1: ("Cornell", 1024, 1024, "ppm"),
            2: ("SyntheticHall", 1920, 1080, "ppm"), 3: ("SyntheticHall", 1920, 1080, "vcm"),
            4: ("SyntheticConference", 3840, 2160, "ppm")}
    for c, w in want.items():
        a = bench.parse(["--config", str(c)])
        assert (a.scene, a.width, a.height, a.method) == w
    assert bench.parse(["--config", "4"]).photon_launch ** 2 == 16777216
    assert bench.parse(["--config", "2"]).photon_launch ** 2 == 4194304
    assert bench.parse(["--config", "1"]).photon_launch ** 2 == 1048576


def test_overrides_win():
    a = bench.parse(["--config", "4", "--width", "640", "--scaling", "weak"])
    assert a.width == 640 and a.height == 2160 and a.scaling == "weak"


def test_plain_run_is_lean_and_full_is_opt_in():
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "2"])
    assert (a.steps, a.warmup) == (3, 2)
    assert not a.full and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"
    # the switches that trim a --full run are still accepted
    a = bench.parse(["--full", "--no-cpu-baseline", "--no-serial-pass-times"])
    assert a.full and a.no_cpu_baseline and a.no_serial_pass_times


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import numpy as np

    out = np.arange(5 * 7 * 3, dtype=np.float32).reshape(5, 7, 3)
    bench.dump_outputs(str(tmp_path / "a"), out)
    got = np.load(tmp_path / "a" / "output.npy")
    assert got.dtype == np.float32 and np.array_equal(got, out)
    # above the limit: a fixed sample of whole pixels, the same from run to run
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10 * 12)
    bench.dump_outputs(str(tmp_path / "b"), out)
    bench.dump_outputs(str(tmp_path / "c"), out)
    b, c = np.load(tmp_path / "b" / "output.npy"), np.load(tmp_path / "c" / "output.npy")
    assert b.shape == (10, 3) and b.nbytes <= 10 * 12 and np.array_equal(b, c)
    px = out.reshape(-1, 3)
    assert all((px == row).all(axis=1).any() for row in b)
    assert (np.diff(b[:, 0]) > 0).all()


def test_host_cpu_accounting():
    n, info = bench.host_cpu()
    assert 1 <= n <= info["affinity_cpus"]
    if info["omp_num_threads"]:
        assert n <= info["omp_num_threads"]
