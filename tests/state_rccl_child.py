"""Child of tests/test_gpu_state_group.py::test_rccl_world1_round_trip: a fresh process in which liborx opens
librccl (no torch here: torch carries its own copy of the library).  World 1 is the only RCCL world a one-GPU
box can host; the ranks of an RCCL group do not share a device, so save and restore take the per-rank path
(rows compact on the rank's device, row by row through the host).

Cornell PPM 40x25, 32x34 photons, seed 1645301512: four iterations straight on the group; two, save, a fresh
group, restore, two more; and the same save restored into a plain renderer.  Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oppositerenderer_amd import _abi, scenes  # noqa: E402
from oppositerenderer_amd.group import OptixRendererGroup  # noqa: E402
from oppositerenderer_amd.renderer import OptixRenderer, RenderRequestDetails, next_ppm_radius  # noqa: E402

SEED, W, H, PW, PH, N, K = 1645301512, 40, 25, 32, 34, 4, 2


def config():
    return _abi.default_config(seed=SEED, photon_launch_width=PW, photon_launch_height=PH)


def group(scene):
    g = OptixRendererGroup(config(), _abi.default_group_config(partition=_abi.GROUP_ROWS, comm=_abi.COMM_RCCL))
    g.initialize([0])
    g.initScene(scene)
    return g


def run(r, det, radii, first, count):
    for i in range(first, first + count):
        r.renderNextIteration(i, i, radii[i], True, det)


def main():
    scene = scenes.cornell()
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
    det = RenderRequestDetails(cam, scene.name, _abi.PROGRESSIVE_PHOTON_MAPPING, W, H)
    radii = [scene.initial_ppm_radius()]
    for i in range(N - 1):
        radii.append(next_ppm_radius(radii[-1], i))

    full = group(scene)
    comm, world = full.comm_name(), full.world()
    run(full, det, radii, 0, N)
    want_rng = full.renderer(0).read_buffer(_abi.BUF_RNG, np.uint32).copy()
    want_out = full.getOutputBuffer().copy()
    full.destroy()

    a = group(scene)
    run(a, det, radii, 0, K)
    blob = a.saveState()
    a.destroy()
    b = group(scene)
    b.restoreState(blob)
    again = b.saveState()
    run(b, det, radii, K, N - K)
    got_rng = b.renderer(0).read_buffer(_abi.BUF_RNG, np.uint32).copy()
    got_out = b.getOutputBuffer().copy()
    b.destroy()

    single = OptixRenderer(config())
    single.initialize(0)
    single.initScene(scene)
    single.restoreState(blob)
    run(single, det, radii, K, N - K)
    single_rng = single.read_buffer(_abi.BUF_RNG, np.uint32).copy()
    single.destroy()

    d = got_out.astype(np.float64) - want_out
    print(json.dumps({"comm": comm, "world": world, "blob_round_trip": again == blob,
                      "rng_bit_equal": bool(np.array_equal(got_rng, want_rng)),
                      "rng_matches_single": bool(np.array_equal(single_rng, want_rng)),
                      "output_rel_l2": float(np.sqrt((d * d).sum() / (want_out.astype(np.float64) ** 2).sum())),
                      "mean": float(got_out.mean())}))


if __name__ == "__main__":
    main()
