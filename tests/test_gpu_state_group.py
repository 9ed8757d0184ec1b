"""Checkpoint / resume of render groups (include/orx.h orx_group_save_state / orx_group_restore_state,
csrc/orx_group_state.hip), LOCAL communicator, every rank on device 0 (TEST: GPU).

A ROWS group's blob is the frame of one renderer: a save from one renderer continues on a group of three
ranks and back.  The frame is 40x25 with a 32x34 photon launch (rng 40x34): with world 3 the image rows
split 9/8/8 and the RNG rows 12/11/11.  Bars as tests/test_gpu_group.py: each rank's RNG rows bit-equal to
the rows of a straight single renderer, summed outputs rel-L2 <= 1e-5 against the ORACLE's straight render
(fp32 summation order only), PT bit-equal.  A BATCH group's blob is a container of its ranks' frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oppositerenderer_amd import _abi, scenes
from oppositerenderer_amd.group import OptixRendererGroup
from oppositerenderer_amd.renderer import OrxError, state_info
from test_gpu_group import oracle_image
from test_gpu_state import H, PH, PW, W, bits, config, oracle, rel_l2, renderer, request, run, straight

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def group(world, partition, scene=None, pw=PW, ph=PH, **gkw):
    g = OptixRendererGroup(config(pw, ph), _abi.default_group_config(partition=partition, comm=_abi.COMM_LOCAL, **gkw))
    g.initialize([0] * world)
    if scene is not None:
        g.initScene(scene)
    return g


def rank_rows(canonical_words, rng_height, rng_width, rank, world):
    """rank's rows (global row rank + j * world) of a canonical [rng_height][rng_width][6] RNG array"""
    return canonical_words.reshape(rng_height, rng_width * 6)[rank::world].reshape(-1)


def status_of(fn, *args):
    with pytest.raises(OrxError) as e:
        fn(*args)
    return e.value.status


@pytest.mark.parametrize("method,world,photons", [("ppm", 3, _abi.PHOTONS_ROWS), ("vcm", 3, _abi.PHOTONS_ROWS),
                                                   ("ppm", 2, _abi.PHOTONS_SLABS)])
def test_rows_across_worlds(method, world, photons):
    """one renderer -> a ROWS group (pipelined schedule) and the reverse.  Fails when a rank loads rows other
    than its own, and for VCM when the estimate flag or the pixel size factor is not restored on the ranks."""
    n, k = 4, 2
    scene = scenes.cornell()
    det = request(scene, method)
    ref = straight("Cornell", method, n, PW, PH, 0, 1)
    ora = oracle("Cornell", method, n, PW, PH)
    RW, RH = max(PW, W), max(PH, H)

    single = renderer(config(), scene)
    run(single, scene, det, 0, k, n)
    blob1 = single.saveState()
    single.destroy()
    g = group(world, _abi.GROUP_ROWS, scene, photon_partition=photons)
    g.restoreState(blob1)
    assert g.saveState() == blob1  # the ranks hold exactly the frame's rows
    run(g, scene, det, k, n - k, n)
    if method == "ppm":
        assert g.pipelined()
    got = g.getOutputBuffer()
    for r in range(world):
        words = g.renderer(r).read_buffer(_abi.BUF_RNG, np.uint32)
        assert np.array_equal(words, rank_rows(ref[_abi.BUF_RNG], RH, RW, r, world)), f"rank {r}"
    err = rel_l2(got, ora["output"])
    print(f"{method} 1 -> {world} ranks: output rel-L2 {err:.3e}")
    assert got.shape == (H, W, 3) and ora["output"].mean() > 0
    assert err <= 1e-5, err
    g.destroy()

    g = group(world, _abi.GROUP_ROWS, scene, photon_partition=photons)
    run(g, scene, det, 0, k, n)
    blob2 = g.saveState()
    g.destroy()
    i1, i2 = state_info(blob1), state_info(blob2)
    assert i2.kind == _abi.STATE_KIND_FRAME and len(blob2) == len(blob1)
    for name, _ in _abi.OrxStateInfo._fields_:
        assert getattr(i1, name) == getattr(i2, name), name
    nr = RW * RH * 24
    assert blob2[128:128 + nr] == blob1[128:128 + nr]  # the same RNG frame from either
    single = renderer(config(), scene)
    single.restoreState(blob2)
    run(single, scene, det, k, n - k, n)
    assert np.array_equal(single.read_buffer(_abi.BUF_RNG, np.uint32), ref[_abi.BUF_RNG])
    err = rel_l2(single.getOutputBuffer(), ora["output"])
    print(f"{method} {world} ranks -> 1: output rel-L2 {err:.3e}")
    assert err <= 1e-5, err
    single.destroy()


def test_pt_across_worlds_bit_equal():
    n, k, name = 4, 2, "CornellSmallSmallSpheres"
    scene = scenes.scene_by_name(name)
    det = request(scene, "pt")
    one = group(1, _abi.GROUP_ROWS, scene)
    run(one, scene, det, 0, k, n)
    blob = one.saveState()
    one.destroy()
    g = group(3, _abi.GROUP_ROWS, scene)
    g.restoreState(blob)
    run(g, scene, det, k, n - k, n)
    got = g.getOutputBuffer()
    ora = oracle(name, "pt", n, PW, PH)
    assert got.mean() > 0
    assert np.array_equal(bits(got), bits(ora["output"]))
    g.destroy()


def test_batch_container():
    """world 2, reduce_every 2: six calls straight against three, save, a fresh group, restore, three"""
    world, Wb, Hb, P = 2, 51, 41, 48  # the configuration of test_gpu_group.py's oracle_image(world=2)
    scene = scenes.cornell()
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(Wb) / np.float32(Hb)))
    from oppositerenderer_amd.renderer import RenderRequestDetails
    det = RenderRequestDetails(cam, scene.name, _abi.PROGRESSIVE_PHOTON_MAPPING, Wb, Hb)
    full = group(world, _abi.GROUP_BATCH, scene, P, P, reduce_every=2)
    run(full, scene, det, 0, 6, 6)
    want_rng = [full.renderer(r).read_buffer(_abi.BUF_RNG, np.uint32).copy() for r in range(world)]
    full.destroy()

    a = group(world, _abi.GROUP_BATCH, scene, P, P, reduce_every=2)
    run(a, scene, det, 0, 3, 6)
    blob = a.saveState()
    a.destroy()
    info = state_info(blob)
    assert (info.kind, info.world, info.calls, info.iteration_number) == (_abi.STATE_KIND_BATCH, world, 3, 2)
    first = state_info(blob[128:])
    second = state_info(blob[128 + first.total_bytes:])
    assert (first.kind, first.local_iteration_number, first.iteration_number) == (0, 1, 2)  # rank 0: calls 0 and 2
    assert (second.kind, second.local_iteration_number, second.iteration_number) == (0, 0, 1)  # rank 1: call 1
    assert len(blob) == 128 + first.total_bytes + second.total_bytes == info.total_bytes

    b = group(world, _abi.GROUP_BATCH, scene, P, P, reduce_every=2)
    b.restoreState(blob)
    assert b.saveState() == blob
    run(b, scene, det, 3, 3, 6)
    got = b.getOutputBuffer()
    for r in range(world):
        assert np.array_equal(b.renderer(r).read_buffer(_abi.BUF_RNG, np.uint32), want_rng[r]), f"rank {r}"
    err = rel_l2(got, oracle_image("Cornell", "ppm", Wb, Hb, P, P, 0, world))
    print(f"batch world {world}: merged output rel-L2 {err:.3e}")
    assert err <= 1e-5, err
    frame = b.renderer(0).saveState()  # a rank is a whole-frame renderer: its own frame
    assert state_info(frame).kind == _abi.STATE_KIND_FRAME
    assert status_of(b.restoreState, frame) == _abi.ORX_ERR_INVALID_ARGUMENT  # a frame into a BATCH group
    b.destroy()

    three = group(3, _abi.GROUP_BATCH, scene, P, P)
    assert status_of(three.restoreState, blob) == _abi.ORX_ERR_INVALID_ARGUMENT  # another world
    three.destroy()
    rows = group(2, _abi.GROUP_ROWS, scene, P, P)
    assert status_of(rows.restoreState, blob) == _abi.ORX_ERR_INVALID_ARGUMENT  # a container into a ROWS group
    assert status_of(rows.saveState) == _abi.ORX_ERR_STATE  # no frame yet
    rows.destroy()
    plain = renderer(config(P, P), scene)
    assert status_of(plain.restoreState, blob) == _abi.ORX_ERR_INVALID_ARGUMENT  # and into a renderer
    plain.destroy()


@pytest.mark.fresh_process
def test_rccl_world1_round_trip(tmp_path):
    """tests/state_rccl_child.py in a fresh process (librccl is opened there, never in this process): a world-1
    ROWS group over RCCL moves its rows through the host"""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("ORX_PIPELINE", None)
    out = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "state_rccl_child.py")], env=env,
                         capture_output=True, text=True, timeout=170, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["comm"] == "rccl" and res["world"] == 1, res
    assert res["blob_round_trip"] and res["rng_bit_equal"] and res["rng_matches_single"], res
    assert res["output_rel_l2"] <= 1e-5, res
