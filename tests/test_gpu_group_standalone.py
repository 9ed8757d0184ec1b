"""integration/standalone_group.cpp on the device: an N-rank frame with no Python in the rendering
process, against the committed oracle fixtures (tests/golden/cornell_*.npz: Cornell 32x32, two
iterations, seed 1645301512), as tests/test_integration.py test_shim_matches_golden: PPM rel-L2 <=
1e-4, PT bit-exact.

The RCCL communicator is loaded only here, in child processes marked fresh_process (they start
before this process has made a HIP call; torch carries its own copy of the library, so librccl
never enters the pytest process).  World 1 is the only RCCL world a one-GPU box can host."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oppositerenderer_amd", "standalone_group")
GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu


def binary():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "integration")])
    return BIN


def run(tmp_path, method, P, extra, env=None):
    out = tmp_path / "out.f32"
    r = subprocess.run([binary(), "--method", method, "--width", "32", "--height", "32", "--photon-launch", str(P),
                        "--iterations", "2", "--seed", "1645301512", "--out", str(out)] + extra,
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr + r.stdout
    assert f"photons {P * P} " in r.stdout, r.stdout
    return np.fromfile(out, np.float32), r.stdout


def compare(got, case, method):
    ref = np.load(os.path.join(GOLDEN, case + ".npz"))["OUTPUT"]
    assert got.shape == ref.shape and got.mean() > 0
    if method == "pt":
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    else:
        err = np.sqrt(((got.astype(np.float64) - ref) ** 2).sum() / (ref.astype(np.float64) ** 2).sum())
        print(f"{case}: rel-L2 {err:.3e}")
        assert err < 1e-4, err


@pytest.mark.parametrize("case,method,P", [("cornell_ppm", "ppm", 64), ("cornell_pt", "pt", 32)])
def test_four_local_ranks_match_golden(case, method, P, tmp_path):
    got, stdout = run(tmp_path, method, P, ["--ranks", "4", "--partition", "rows", "--comm", "local"])
    assert "communicator local world 4" in stdout
    if method == "ppm":
        assert "pipelined 1" in stdout
    compare(got, case, method)


@pytest.mark.fresh_process
@pytest.mark.parametrize("case,method,P,partition", [("cornell_ppm", "ppm", 64, "rows"), ("cornell_ppm", "ppm", 64, "batch"),
                                                      ("cornell_pt", "pt", 32, "rows")])
def test_rccl_world1_matches_golden(case, method, P, partition, tmp_path):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("ORX_PIPELINE", None)
    got, stdout = run(tmp_path, method, P, ["--ranks", "1", "--partition", partition, "--comm", "rccl"], env=env)
    assert "communicator rccl world 1" in stdout, stdout
    if method == "ppm" and partition == "rows":
        assert "pipelined 1" in stdout
    compare(got, case, method)
