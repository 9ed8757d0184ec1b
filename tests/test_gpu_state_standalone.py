"""--save-state / --load-state of the stand-alone hosts (integration/standalone_cornell.cpp through the
OptixRenderer shim, integration/standalone_group.cpp through the group API): no Python in the rendering
process (TEST: GPU).  Each host runs three ways, one process after another, each under its own time limit:
four iterations writing the frame; two iterations with --save-state; --load-state and two more writing the
frame.  The frames agree within rel-L2 <= 1e-5 (PPM: fp32 summation order only), PT bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from oppositerenderer_amd.renderer import state_info

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = {"cornell": (os.path.join(ROOT, "oppositerenderer_amd", "standalone_cornell"), []),
        "group": (os.path.join(ROOT, "oppositerenderer_amd", "standalone_group"),
                  ["--ranks", "2", "--partition", "rows", "--comm", "local"])}
W, H, P = 40, 25, 32

pytestmark = pytest.mark.gpu


def host(which, method, iterations, extra):
    path, args = BINS[which]
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "integration")])
    r = subprocess.run([path, "--method", method, "--width", str(W), "--height", str(H), "--photon-launch", str(P),
                        "--iterations", str(iterations), "--seed", "1645301512"] + args + extra,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    return r.stdout


@pytest.mark.parametrize("which", ["cornell", "group"])
@pytest.mark.parametrize("method", ["ppm", "pt"])
def test_hosts_save_and_resume(which, method, tmp_path):
    full, part, state = tmp_path / "full.f32", tmp_path / "resumed.f32", tmp_path / "state.bin"
    host(which, method, 4, ["--out", str(full)])
    host(which, method, 2, ["--save-state", str(state)])
    info = state_info(state.read_bytes())
    assert (info.kind, info.width, info.height, info.iteration_number) == (0, W, H, 1)
    assert (info.photon_launch_width, info.photon_launch_height) == (P, P)
    stdout = host(which, method, 2, ["--load-state", str(state), "--out", str(part)])
    assert "iterations 2" in stdout
    want, got = np.fromfile(full, np.float32), np.fromfile(part, np.float32)
    assert want.shape == got.shape == (W * H * 3,) and want.mean() > 0
    if method == "pt":
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    else:
        err = float(np.sqrt(((got.astype(np.float64) - want) ** 2).sum() / (want.astype(np.float64) ** 2).sum()))
        print(f"{which} {method}: resumed vs straight rel-L2 {err:.3e}")
        assert err <= 1e-5, err
    # the state of one host continues on the other: both blobs are frames of the same scene
    other = "group" if which == "cornell" else "cornell"
    cross = tmp_path / "cross.f32"
    host(other, method, 2, ["--load-state", str(state), "--out", str(cross)])
    got = np.fromfile(cross, np.float32)
    if method == "pt":
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    else:
        err = float(np.sqrt(((got.astype(np.float64) - want) ** 2).sum() / (want.astype(np.float64) ** 2).sum()))
        print(f"{which} -> {other} {method}: rel-L2 {err:.3e}")
        assert err <= 1e-5, err
