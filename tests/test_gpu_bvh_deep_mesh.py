"""A mesh whose BVH sits at the builders' depth cap, end to end through the ABI against the oracle.

The mesh is a geometric strip: triangle k is (s, 0, z), (1.5 s, 0, z), (s, 0.5 s, z) with s = 300 / 1.01^(1999 - k),
2000 of them standing on the Cornell box's floor in the plane z = 300, the largest 150 wide and high, each
overlapping some forty of its neighbours in that plane.  Every SAH split peels a few triangles off one end, so
the binned build ends with median splits (depth 20 here) and the treelet sweeps used to deepen it past
ORX_BVH_STACK, upon which orx_init_scene refused the scene ("BVH deeper than the traversal stack"); now both
builders keep the binned tree for such a mesh.  Its stack bound of 54 is far past the 16 LDS entries of
the photon and shadow kernels' StackH, so their global-memory continuation carries real traversals here."""
import numpy as np
import pytest

import oracle_lib
from oppositerenderer_amd import _abi, scenes
from oppositerenderer_amd.renderer import next_ppm_radius
from test_gpu_parity import check_ppm_iteration, check_vcm_iteration, make_pair

pytestmark = pytest.mark.gpu
W = H = 48


def cornell_with_strip():
    sc = scenes.cornell()
    sc.name = "CornellStrip"
    blue = sc.add_material(scenes.Diffuse((0.1, 0.1, 0.9)))
    red = sc.add_material(scenes.Diffuse((0.9, 0.1, 0.1)))
    n = 2000
    s = (300.0 / 1.01 ** (n - 1 - np.arange(n, dtype=np.float64)))
    z = np.full(n, 300.0)
    zero = np.zeros(n)
    v = np.stack([np.stack([s, zero, z], 1), np.stack([1.5 * s, zero, z], 1), np.stack([s, 0.5 * s, z], 1)], 1)
    tri_mat = np.where(np.arange(n) % 2 == 0, blue, red)
    sc.set_mesh(v.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.uint32).reshape(n, 3), tri_mat)
    return sc


def render_pt(scene, iterations=2):
    gpu, ora, det = make_pair(scene, W, H, 32, _abi.PATH_TRACING)
    req = det.to_abi()
    for it in range(iterations):
        gpu.renderNextIteration(it, it, 1.0, True, det)
        ora.render_next_iteration(it, it, 1.0, req)
        assert np.array_equal(gpu.read_buffer(_abi.BUF_RNG, np.uint32), ora.read_buffer(_abi.BUF_RNG, np.uint32))
    g, o = gpu.getOutputBuffer(), ora.output()
    entries = gpu.stats().bvh_stack_entries
    gpu.destroy()
    ora.close()
    # no order-dependent sums in PT: bit-exact
    assert np.array_equal(g.view(np.uint32), o.view(np.uint32))
    return g, entries


@pytest.mark.parametrize("host_builder", ["0", "1"])
def test_deep_strip_in_cornell_matches_oracle(host_builder, monkeypatch):
    monkeypatch.setenv("ORX_BVH_HOST", host_builder)
    scene = cornell_with_strip()
    with_mesh, entries = render_pt(scene)
    assert 16 < entries <= 97, entries
    # the strip is in view: it changes more than 1 % of the pixels (the oracle alone: 20.6 % of 48 x 48)
    without, _ = render_pt(scenes.cornell())
    changed = np.any(with_mesh.reshape(H * W, -1) != without.reshape(H * W, -1), axis=1)
    assert changed.mean() >= 0.01, changed.mean()

    gpu, ora, det = make_pair(scene, W, H, 64, _abi.PROGRESSIVE_PHOTON_MAPPING)
    radius = scene.initial_ppm_radius()
    req = det.to_abi()
    for it in range(2):
        gpu.renderNextIteration(it, it, radius, True, det)
        ora.render_next_iteration(it, it, radius, req)
        check_ppm_iteration(gpu, ora)
        radius = next_ppm_radius(radius, it)
    gpu.destroy()
    ora.close()

    gpu, ora, det = make_pair(scene, W, H, 64, _abi.VCM_BIDIRECTIONAL_PATH_TRACING)
    radius = scene.initial_ppm_radius()
    gpu.renderNextIteration(0, 0, radius, True, det)
    ora.render_next_iteration(0, 0, radius, det.to_abi())
    check_vcm_iteration(gpu, ora)
    gpu.destroy()
    ora.close()
