"""A scene that orx_init_scene refuses changes nothing: the renderer, or every rank of a group, goes on with the scene
it had, and the next iteration equals, bit for bit, that of a renderer which never saw the refused scene.

The other half of the rule, that a failure after the first device write leaves no scene at all (scene_ready false, the
next iteration ORX_ERR_STATE), needs a scene that passes validation and defeats the BVH builder; no test reaches it,
it is verified by reading orx::init_scene_checked."""
import numpy as np
import pytest

from oppositerenderer_amd import _abi, scenes
from oppositerenderer_amd.group import OptixRendererGroup
from oppositerenderer_amd.renderer import OptixRenderer, OrxError, RenderRequestDetails

pytestmark = pytest.mark.gpu
SEED = 1645301512
W = H = 32


def config():
    return _abi.default_config(seed=SEED, photon_launch_width=32, photon_launch_height=32)


def single():
    r = OptixRenderer(config())
    r.initialize(0)
    return r


def rows_group():
    g = OptixRendererGroup(config(), _abi.default_group_config(partition=_abi.GROUP_ROWS, comm=_abi.COMM_LOCAL))
    return g.initialize([0, 0])


def bad_mesh_scene():
    """Cornell with a two-triangle mesh whose last vertex index is n_vertices."""
    sc = scenes.cornell()
    sc.set_mesh([[100, 100, 100], [200, 100, 100], [100, 200, 100], [200, 200, 100]], [[0, 1, 2], [1, 2, 4]], [0, 0])
    return sc


@pytest.mark.parametrize("make", [single, rows_group], ids=["renderer", "rows_group_of_two"])
def test_refused_scene_changes_nothing(make):
    scene = scenes.cornell()
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
    det = RenderRequestDetails(cam, scene.name, _abi.PATH_TRACING, W, H)

    ref = make()
    ref.initScene(scene)
    for it in range(2):
        ref.renderNextIteration(it, it, 1.0, True, det)
    want = np.array(ref.getOutputBuffer(), copy=True)
    ref.destroy()
    assert want.any()

    r = make()
    r.initScene(scene)
    r.renderNextIteration(0, 0, 1.0, True, det)
    with pytest.raises(OrxError) as e:
        r.initScene(bad_mesh_scene())
    assert e.value.status == _abi.ORX_ERR_INVALID_ARGUMENT
    assert "triangle vertex index out of range" in str(e.value)
    r.renderNextIteration(1, 1, 1.0, True, det)
    got = r.getOutputBuffer()
    assert np.array_equal(got.view(np.uint32).ravel(), want.view(np.uint32).ravel())
    r.destroy()
