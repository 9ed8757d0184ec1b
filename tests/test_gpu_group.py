"""Render groups on the device (include/orx.h orx_create_group, csrc/orx_group.hip): N ranks on ONE
MI355X behind one handle, the LOCAL communicator (csrc/orx_group_comm.hip: device-to-device all-gather, k_group_reduce_scatter,
k_group_reduce, k_group_assemble_rows), no torch collective anywhere.

Tolerances are the project's (tests/test_gpu_sharded.py): rel-L2 <= 1e-5 against
the ORACLE's single renderer for summed estimates (the gather is linear in the photon set, the VCM
splats sum over ranks: fp32 summation order only), PT bit-exact.  The LOCAL sums add in rank order
in fp32, so they are bit-equal to the same sum taken by NumPy."""
import functools

import numpy as np
import pytest

from oppositerenderer_amd import _abi, multigpu, scenes
from oppositerenderer_amd.group import OptixRendererGroup
from oppositerenderer_amd.renderer import OrxError, RenderRequestDetails, next_ppm_radius

pytestmark = pytest.mark.gpu
SEED = 1645301512
ITERS = 3
METHODS = {"ppm": _abi.PROGRESSIVE_PHOTON_MAPPING, "vcm": _abi.VCM_BIDIRECTIONAL_PATH_TRACING, "pt": _abi.PATH_TRACING}


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b * b).sum()))


def request(scene, method, W, H):
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
    return RenderRequestDetails(cam, scene.name, METHODS[method], W, H)


@functools.lru_cache(maxsize=None)
def oracle_image(scene_name, method, W, H, P, PH, photon_map=0, world=1):
    """The oracle's single renderer (world > 1: the photon-batch partition's float64 sum of `world`
    renderers seeded multigpu.batch_seed(SEED, g) with the dealt iterations and radii, as
    tests/rccl_world1_child.py oracle_image).  Computed once per configuration; read-only."""
    import oracle_lib

    scene = scenes.scene_by_name(scene_name)
    req = request(scene, method, W, H).to_abi()
    radii = multigpu.radius_sequence(scene.initial_ppm_radius(), ITERS * world)
    out = None
    for g in range(world):
        ora = oracle_lib.OracleRenderer(_abi.default_config(seed=multigpu.batch_seed(SEED, g), photon_launch_width=P,
                                                            photon_launch_height=PH, photon_map=photon_map))
        ora.init_scene(scene)
        for i in range(ITERS):
            it = multigpu.batch_iteration(i, g, world)
            ora.render_next_iteration(it, i, radii[it], req)
        o = ora.output().astype(np.float64 if world > 1 else np.float32)
        out = o if out is None else out + o
        ora.close()
    out.setflags(write=False)
    return out


def make_group(world, partition, P=32, PH=None, pipeline=1, photon_map=0, reduce_every=8, scene=None):
    cfg = _abi.default_config(seed=SEED, photon_launch_width=P, photon_launch_height=PH or P, photon_map=photon_map)
    g = OptixRendererGroup(cfg, _abi.default_group_config(partition=partition, comm=_abi.COMM_LOCAL, pipeline=pipeline,
                                                          reduce_every=reduce_every))
    g.initialize([0] * world)
    if scene is not None:
        g.initScene(scene)
    return g


def render(g, scene, det, iters=ITERS, first=0):
    """the caller's loop for ONE renderer: render(i, i, radius_i)"""
    radii = multigpu.radius_sequence(scene.initial_ppm_radius(), first + iters)
    for i in range(first, first + iters):
        g.renderNextIteration(i, i, radii[i], True, det)


@pytest.mark.parametrize("world,W,H,P,PH,pipeline,photon_map",
                         [(1, 51, 41, 48, 48, 1, 0), (3, 51, 41, 48, 50, 0, 0), (4, 96, 80, 128, 128, 1, 0),
                          (8, 100, 75, 96, 101, 1, 0), (2, 64, 48, 64, 64, 1, 2)])
def test_rows_ppm_matches_oracle(world, W, H, P, PH, pipeline, photon_map):
    """(3, 51, 41): uneven pixel and photon rows, blocks of 14 * 51 * 3 = 2142 floats, so the
    reduce-scatter's block k starts 8 bytes off 16-byte alignment"""
    scene = scenes.cornell()
    g = make_group(world, _abi.GROUP_ROWS, P, PH, pipeline, photon_map, scene=scene)
    assert g.world() == world and g.comm_name() == "local"
    render(g, scene, request(scene, "ppm", W, H))
    assert g.pipelined() == bool(pipeline)
    got = g.getOutputBuffer()
    assert g.renderer(world - 1).stats().valid_photons > 0
    ref = oracle_image("Cornell", "ppm", W, H, P, PH, photon_map)
    err = rel_l2(got, ref)
    print(f"rows ppm world {world} {W}x{H} pipeline {pipeline} map {photon_map}: rel-L2 {err:.3e}")
    assert got.shape == (H, W, 3) and np.isfinite(got).all() and ref.mean() > 0
    assert err <= 1e-5, err
    again = g.getOutputBuffer()  # reading the output changes nothing
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    g.destroy()


def test_rows_stochastic_hash_is_single_device():
    g = OptixRendererGroup(_abi.default_config(seed=SEED, photon_launch_width=32, photon_launch_height=32, photon_map=1),
                           _abi.default_group_config(partition=_abi.GROUP_ROWS, comm=_abi.COMM_LOCAL))
    with pytest.raises(OrxError) as e:
        g.initialize([0, 0])
    assert e.value.status == _abi.ORX_ERR_UNSUPPORTED


@pytest.mark.parametrize("world,W,H", [(2, 64, 48), (3, 51, 41)])
def test_rows_vcm_matches_oracle(world, W, H):
    scene = scenes.cornell()
    g = make_group(world, _abi.GROUP_ROWS, scene=scene)
    render(g, scene, request(scene, "vcm", W, H))
    got = g.getOutputBuffer()
    ref = oracle_image("Cornell", "vcm", W, H, 32, 32)
    err = rel_l2(got, ref)
    print(f"rows vcm world {world} {W}x{H}: rel-L2 {err:.3e}")
    assert np.isfinite(got).all() and got.mean() > 0
    assert err <= 1e-5, err
    g.destroy()


def test_rows_pt_bit_exact():
    world, W, H = 3, 51, 41
    scene = scenes.scene_by_name("CornellSmallSmallSpheres")
    g = make_group(world, _abi.GROUP_ROWS, scene=scene)
    render(g, scene, request(scene, "pt", W, H))
    got = g.getOutputBuffer()
    ref = oracle_image("CornellSmallSmallSpheres", "pt", W, H, 32, 32)
    assert got.mean() > 0
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    g.destroy()


@pytest.mark.parametrize("world", [2, 3])
def test_batch_ppm_matches_oracle_sum(world):
    """reduce_every = 2 and 3 iterations per rank: one periodic merge, then the one of getOutputBuffer"""
    W, H, P = 51, 41, 48
    scene = scenes.cornell()
    g = make_group(world, _abi.GROUP_BATCH, P, reduce_every=2, scene=scene)
    render(g, scene, request(scene, "ppm", W, H), iters=ITERS * world)
    got = g.getOutputBuffer()
    again = g.getOutputBuffer()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))  # no double accumulation
    ref = oracle_image("Cornell", "ppm", W, H, P, P, 0, world)
    err = rel_l2(got, ref)
    print(f"batch ppm world {world}: rel-L2 {err:.3e}")
    assert err <= 1e-5, err
    imgs = [g.renderer(k).getOutputBuffer().copy() for k in range(world)]  # whole frames, own RNG streams
    for a in range(world):
        assert imgs[a].shape == (H, W, 3)
        for b in range(a + 1, world):
            assert rel_l2(imgs[a], imgs[b]) > 1e-3
    total = imgs[0].copy()  # the merge itself: the float32 sum in rank order, bit for bit
    for im in imgs[1:]:
        total += im
    assert np.array_equal(total.view(np.uint32), g.getOutputBuffer().view(np.uint32))
    g.destroy()


def test_batch_pt_world1_bit_exact():
    W, H = 51, 41
    scene = scenes.scene_by_name("CornellSmallSmallSpheres")
    g = make_group(1, _abi.GROUP_BATCH, scene=scene)
    render(g, scene, request(scene, "pt", W, H))
    got = g.getOutputBuffer()
    ref = oracle_image("CornellSmallSmallSpheres", "pt", W, H, 32, 32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    g.destroy()


def test_rows_resize_equals_fresh_group():
    world, P, PH = 3, 48, 50
    scene = scenes.cornell()
    g = make_group(world, _abi.GROUP_ROWS, P, PH, scene=scene)
    render(g, scene, request(scene, "ppm", 48, 36), iters=2)
    small = g.getOutputBuffer()
    assert small.shape == (36, 48, 3) and small.mean() > 0
    render(g, scene, request(scene, "ppm", 48, 36), iters=1, first=2)  # a finish outstanding at the resize
    render(g, scene, request(scene, "ppm", 51, 41))
    got = g.getOutputBuffer()
    g.destroy()
    fresh = make_group(world, _abi.GROUP_ROWS, P, PH, scene=scene)
    render(fresh, scene, request(scene, "ppm", 51, 41))
    ref = fresh.getOutputBuffer()
    fresh.destroy()
    err = rel_l2(got, ref)
    print(f"resize: rel-L2 {err:.3e}")
    assert got.shape == (41, 51, 3)
    assert err <= 1e-5, err
    assert rel_l2(got, oracle_image("Cornell", "ppm", 51, 41, P, PH)) <= 1e-5


def mixed(rng, shape):
    """random float32 with magnitudes from 1e-6 to 1e6 and both signs: the sum depends on its order"""
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-6, 7, shape)).astype(np.float32)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_local_collectives_bit_equal_numpy(world):
    rng = np.random.default_rng(1234 + world)
    g = make_group(world, _abi.GROUP_ROWS)
    for block in (1, 3, 5, 2142, 4099):
        x = mixed(rng, (world, world * block))
        ref = x[0].copy()
        for r in range(1, world):
            ref += x[r]  # float32, rank order
        got = g.debug_reduce_scatter(x)
        assert got.shape == (world, block)
        assert np.array_equal(got.view(np.uint32), ref.reshape(world, block).view(np.uint32)), (world, block)
        y = mixed(rng, (world, block))
        ref = y[0].copy()
        for r in range(1, world):
            ref += y[r]
        assert np.array_equal(g.debug_reduce(y).view(np.uint32), ref.view(np.uint32)), (world, block)
    g.destroy()


def test_render_before_init_scene_is_state_error():
    scene = scenes.cornell()
    g = make_group(2, _abi.GROUP_ROWS)
    with pytest.raises(OrxError) as e:
        render(g, scene, request(scene, "ppm", 32, 32), iters=1)
    assert e.value.status == _abi.ORX_ERR_STATE
    g.destroy()
