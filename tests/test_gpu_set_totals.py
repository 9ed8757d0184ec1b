"""The running totals in stats() (valid_photons_total, timed_iterations) across the pipelined PPM
buffer sets: every set accumulates the iterations it held, stats() sums them and reset_timing()
zeroes them in every set.  bench.py derives its per-iteration photon average, and from it the
roofline bytes, from valid_photons_total."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_CHILD = r'''
import json, sys, numpy as np
sys.path.insert(0, "tests")
import oracle_lib
from oppositerenderer_amd import _abi, scenes
from oppositerenderer_amd.renderer import OptixRenderer, RenderRequestDetails, next_ppm_radius
serial = sys.argv[1] == "1"
scene = scenes.cornell()
W, H, P = 64, 48, 96
mk = lambda: _abi.default_config(seed=1645301512, photon_launch_width=P, photon_launch_height=P, photon_map=0)
gpu = OptixRenderer(mk()); gpu.initialize(0); gpu.initScene(scene)
if serial:
    gpu.set_iteration_pipelining(0)
ora = oracle_lib.OracleRenderer(mk())
ora.init_scene(scene)
cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
det = RenderRequestDetails(cam, scene.name, _abi.PROGRESSIVE_PHOTON_MAPPING, W, H)
r = scene.initial_ppm_radius()
valid = []
for it in range(6):
    if it == 2:
        gpu.reset_timing()
    gpu.renderNextIteration(it, it, r, True, det)  # no read between the iterations of a region
    ora.render_next_iteration(it, it, r, det.to_abi())
    valid.append(int(ora.stats().valid_photons))
    r = next_ppm_radius(r, it)
s = gpu.stats()
pipelined = gpu.pipelined()
g, o = gpu.getOutputBuffer().astype(np.float64), ora.output().astype(np.float64)
err = float(np.sqrt(((g - o) ** 2).sum() / (o ** 2).sum()))
gpu.reset_timing()
s2 = gpu.stats()
print(json.dumps({"oracle_valid": valid, "total": int(s.valid_photons_total), "timed": int(s.timed_iterations),
                  "valid": int(s.valid_photons), "pipelined": pipelined, "err": err,
                  "total_after_reset": int(s2.valid_photons_total), "valid_after_reset": int(s2.valid_photons)}))
'''


@pytest.mark.parametrize("variant", ["sets3", "sets2", "serial"])
def test_set_totals_after_reset(variant):
    """Cornell 64x48, 96x96 photons, uniform grid: two iterations, reset_timing(), four more with no
    read in between, stats().  The totals cover exactly those four iterations whichever buffer sets
    held them (three sets by default, two with ORX_PIPE_SETS=2, one when serial), and a second
    reset_timing() clears them without touching the last iteration's own figures."""
    env = dict(os.environ)
    for k in ("ORX_PIPELINE", "ORX_PIPE_SETS", "ORX_GRID_ASYNC"):
        env.pop(k, None)
    if variant == "sets2":
        env["ORX_PIPE_SETS"] = "2"
    out = subprocess.run([sys.executable, "-c", _CHILD, "1" if variant == "serial" else "0"], env=env,
                         capture_output=True, text=True, timeout=110,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(variant, res)
    assert res["total"] == sum(res["oracle_valid"][2:]), res
    assert res["timed"] == 4, res
    assert res["valid"] == res["oracle_valid"][-1], res
    assert res["pipelined"] == (variant != "serial"), res  # no silent fallback to the serial schedule
    assert res["err"] < 1e-5, res
    assert res["total_after_reset"] == 0 and res["valid_after_reset"] == res["oracle_valid"][-1], res
