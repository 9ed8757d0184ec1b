"""Photon slabs behind the render group (include/orx.h orx_group_config.photon_partition = ORX_PHOTONS_SLABS,
csrc/orx_group.hip slab_exchange, csrc/orx_group_comm.hip k_group_all_to_all, csrc/orx_slab_plan.cpp): N ranks on
ONE MI355X, the LOCAL communicator, planner and photon all-to-all inside liborx.so, no torch collective and no NumPy
planner anywhere.

Scene, seed and iteration count are those of tests/test_gpu_group.py, the reference is the ORACLE's single
renderer, and the tolerance is the project's for summed estimates: rel-L2 <= 1e-5 (each hit
point's indirect comes whole from its slab's owner, so only the fp32 order inside its window differs); PT
bit-exact.  The all-to-all moves bits, so it is bit-equal to the NumPy rearrangement."""
import os
import subprocess

import numpy as np
import pytest

from oppositerenderer_amd import _abi, scenes
from oppositerenderer_amd.group import OptixRendererGroup
from oppositerenderer_amd.renderer import OrxError
from test_gpu_group import ITERS, SEED, oracle_image, rel_l2, render, request

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oppositerenderer_amd", "standalone_group")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def make_group(world, P=32, PH=None, pipeline=1, scene=None, photons=_abi.PHOTONS_SLABS):
    cfg = _abi.default_config(seed=SEED, photon_launch_width=P, photon_launch_height=PH or P)
    g = OptixRendererGroup(cfg, _abi.default_group_config(partition=_abi.GROUP_ROWS, comm=_abi.COMM_LOCAL,
                                                          pipeline=pipeline, photon_partition=photons))
    g.initialize([0] * world)
    if scene is not None:
        g.initScene(scene)
    return g


def all_to_all_numpy(x, counts):
    """send buffers back to back (rank s: its records for d = 0, 1, ... in turn) -> receive buffers back to back
    (rank d: what s = 0, 1, ... sent, in turn)"""
    n = len(counts)
    start = np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64).reshape(-1))])
    runs = [[x[start[s * n + d]:start[s * n + d + 1]] for d in range(n)] for s in range(n)]
    return np.concatenate([runs[s][d] for d in range(n) for s in range(n)])


@pytest.mark.parametrize("counts", [[[0, 1, 7], [0, 0, 0], [5000, 3, 0]], [[41]]])
def test_local_all_to_all_bit_equal_numpy(counts):
    """world 3: an empty row, single records that put the following runs off 16-byte alignment (36-byte records),
    and a 5000-record run (45000 dwords) that spans several workgroups; world 1: one self-run"""
    counts = np.asarray(counts, np.uint64)
    world = len(counts)
    rng = np.random.default_rng(99 + world)
    x = rng.integers(0, 2 ** 32, (int(counts.sum()), 9), dtype=np.uint64).astype(np.uint32).view(np.float32)
    g = make_group(world)
    got = g.debug_all_to_all(x, counts)
    want = all_to_all_numpy(x, counts)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    again = g.debug_all_to_all(x, counts)  # the run table is reused
    assert np.array_equal(again.view(np.uint32), want.view(np.uint32))
    g.destroy()


@pytest.mark.parametrize("world,W,H,P,PH,pipeline", [(2, 64, 48, 64, 64, 0), (3, 51, 41, 48, 50, 0),
                                                     (4, 96, 80, 128, 128, 1), (8, 100, 75, 96, 101, 1)])
def test_slabs_ppm_matches_oracle(world, W, H, P, PH, pipeline):
    """the uneven-row and misaligned-block shapes of test_rows_ppm_matches_oracle"""
    scene = scenes.cornell()
    g = make_group(world, P, PH, pipeline, scene)
    assert g.world() == world and g.comm_name() == "local"
    render(g, scene, request(scene, "ppm", W, H))
    assert g.pipelined() == bool(pipeline)
    got = g.getOutputBuffer()
    ref = oracle_image("Cornell", "ppm", W, H, P, PH)
    err = rel_l2(got, ref)
    axis, bin_dest, counts = g.slab_plan()
    print(f"slabs ppm world {world} {W}x{H} pipeline {pipeline}: rel-L2 {err:.3e}, axis {axis}, "
          f"received {counts.sum(0).tolist()}")
    assert got.shape == (H, W, 3) and np.isfinite(got).all() and ref.mean() > 0
    assert err <= 1e-5, err
    again = g.getOutputBuffer()  # reading the output changes nothing
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    # the exchange really ran: photons crossed ranks and at least two ranks received some
    assert axis in (0, 1, 2) and bin_dest.shape == (1024,) and (np.diff(bin_dest.astype(int)) >= 0).all()
    assert bin_dest.max() < world and counts.shape == (world, world)
    assert (counts.sum() - np.trace(counts)) > 0 and (counts.sum(0) > 0).sum() >= 2
    g.destroy()


def test_one_rank_with_slabs_runs_the_rows_path():
    W, H, P = 51, 41, 48
    scene = scenes.cornell()
    g = make_group(1, P, scene=scene)
    render(g, scene, request(scene, "ppm", W, H))
    got = g.getOutputBuffer()
    assert g.pipelined()
    assert rel_l2(got, oracle_image("Cornell", "ppm", W, H, P, P)) <= 1e-5
    with pytest.raises(OrxError) as e:  # one slab: nothing was exchanged
        g.slab_plan()
    assert e.value.status == _abi.ORX_ERR_STATE
    g.destroy()


def test_slabs_resize():
    """two iterations at 64x48, then a restart (local iteration 0) at 51x41: the histogram and record buffers
    follow the resize"""
    world, P, PH = 3, 48, 50
    scene = scenes.cornell()
    g = make_group(world, P, PH, scene=scene)
    render(g, scene, request(scene, "ppm", 64, 48), iters=2)
    render(g, scene, request(scene, "ppm", 51, 41))
    got = g.getOutputBuffer()
    err = rel_l2(got, oracle_image("Cornell", "ppm", 51, 41, P, PH))
    print(f"slabs resize: rel-L2 {err:.3e}")
    assert got.shape == (41, 51, 3)
    assert err <= 1e-5, err
    g.destroy()


def test_slabs_leave_pt_bit_exact():
    world, W, H = 3, 51, 41
    scene = scenes.scene_by_name("CornellSmallSmallSpheres")
    g = make_group(world, scene=scene)
    render(g, scene, request(scene, "pt", W, H))
    got = g.getOutputBuffer()
    ref = oracle_image("CornellSmallSmallSpheres", "pt", W, H, 32, 32)
    assert got.mean() > 0
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    with pytest.raises(OrxError):
        g.slab_plan()
    g.destroy()


def run_standalone(tmp_path, extra, env=None):
    out = tmp_path / "out.f32"
    r = subprocess.run([BIN, "--method", "ppm", "--width", "32", "--height", "32", "--photon-launch", "64",
                        "--iterations", "2", "--seed", "1645301512", "--photons", "slabs", "--out", str(out)] + extra,
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "photon-partition slabs" in r.stdout and "photons 4096 " in r.stdout, r.stdout
    got = np.fromfile(out, np.float32)
    ref = np.load(os.path.join(GOLDEN, "cornell_ppm.npz"))["OUTPUT"]
    assert got.shape == ref.shape and got.mean() > 0
    err = rel_l2(got, ref)
    print(f"standalone {extra}: rel-L2 {err:.3e}")
    assert err < 1e-4, err  # tests/test_gpu_group_standalone.py compare()
    return r.stdout


def test_standalone_four_local_ranks_slabs_match_golden(tmp_path):
    stdout = run_standalone(tmp_path, ["--ranks", "4", "--partition", "rows", "--comm", "local"])
    assert "communicator local world 4" in stdout and "pipelined 1" in stdout


@pytest.mark.fresh_process
def test_standalone_rccl_world1_slabs_match_golden(tmp_path):
    """one rank: the rows path, no send or receive call; librccl is loaded only in the child process"""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("ORX_PIPELINE", None)
    stdout = run_standalone(tmp_path, ["--ranks", "1", "--partition", "rows", "--comm", "rccl"], env=env)
    assert "communicator rccl world 1" in stdout and "pipelined 1" in stdout
