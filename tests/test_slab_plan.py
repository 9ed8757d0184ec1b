"""The slab planner on the CPU (oppositerenderer_amd/csrc/orx_slab_plan.cpp, include/orx.h orx_slab_plan).

1. tests/slab_plan_check.cpp is built with the planner's source and nothing else (no HIP, no liborx.so) under
   AddressSanitizer + UndefinedBehaviorSanitizer and run as a program of its own; what it asserts is listed at the
   top of that file.
2. Through liborx.so (no device is needed) orx_slab_plan returns the (axis, bin_dest, counts) of
   multigpu.slab_plan.  The two differ only in the rounding of the normalised weights (NumPy sums pairwise), so
   the inputs are chosen with room for it, and the test asserts that room first: no bin's mid * world / total
   within 1e-6 of an integer on any axis, and the three axis costs more than 1e-9 apart (relative)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oppositerenderer_amd import _abi, multigpu, renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oppositerenderer_amd", "csrc")
V = multigpu.SLAB_VOXELS


def test_slab_planner_under_sanitizers(tmp_path):
    exe = str(tmp_path / "slab_plan_check")
    # the sanitizer runtimes are linked into the program, as tests/test_bvh_host.py does
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "slab_plan_check.cpp"),
                           os.path.join(CSRC, "orx_slab_plan.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-4000:]
    assert "all checks passed" in run.stdout


def random_hists(seed, world, nb):
    """one rank's orx_ppm_slab_histogram words after the other: photons and hit points as points with a bin per
    axis (so the per-axis counts and the voxel counts describe one set), a uniform part that leaves no bin
    empty and a cluster per rank"""
    rng = np.random.default_rng(seed)
    layer = nb // V
    words = np.zeros((world, multigpu.slab_hist_words(nb)), np.uint32)
    for s in range(world):
        for kind, n_uniform, n_cluster in ((0, 3000, 5000), (1, 12000 // world + 4000, 3000)):
            centre = rng.uniform(0.1, 0.9, 3) * nb
            pts = np.concatenate([rng.integers(0, nb, (n_uniform, 3)),
                                  np.clip(rng.normal(centre, 0.07 * nb, (n_cluster, 3)), 0, nb - 1).astype(np.int64)])
            for a in range(3):
                words[s, (3 * kind + a) * nb:(3 * kind + a + 1) * nb] = np.bincount(pts[:, a], minlength=nb)
            v = pts // layer
            words[s, 6 * nb + 6 + kind * V ** 3:6 * nb + 6 + (kind + 1) * V ** 3] = np.bincount(
                v[:, 0] + V * (v[:, 1] + V * v[:, 2]), minlength=V ** 3)
        box = np.sort(rng.integers(0, 2 ** 32, (2, 3), dtype=np.uint64), axis=0).astype(np.uint32)
        words[s, 6 * nb:6 * nb + 6] = box.reshape(6)
    return words


def plan_margins(hists, vox, world):
    """multigpu.slab_plan's per-axis weights again: (the least distance of any bin's mid * world / total from an
    integer, the three largest-slab costs)"""
    h = np.asarray(hists, np.float64)
    nb = h.shape[-1]
    ph, hp = h[:, 0].sum(0), h[:, 1].sum(0)
    v = np.asarray(vox, np.float64).reshape(world, 2, V, V, V).sum(0)
    cost = v[0] * v[1]
    dist, costs = np.inf, []
    for a in range(3):
        other = tuple(k for k in range(3) if k != (2, 1, 0)[a])
        lc, lh = cost.sum(axis=other), v[1].sum(axis=other)
        per_hp = np.divide(lc, lh, out=np.zeros_like(lc), where=lh > 0)
        w = np.zeros(nb)
        for part, weight in ((hp[a] * np.repeat(per_hp, nb // V), 0.8), (ph[a], 0.15), (hp[a], 0.05)):
            w += weight * part / part.sum()
        x = (np.cumsum(w) - 0.5 * w) * world / w.sum()
        dist = min(dist, float(np.abs(x - np.rint(x)).min()))
        dest = np.minimum(np.floor(x), world - 1).astype(np.int64)
        costs.append(float(np.bincount(dest, weights=w, minlength=world).max()))
    return dist, costs


@pytest.mark.parametrize("seed,world,halo", [(11, 2, (3, 5, 4)), (12, 5, (2, 9, 6)), (13, 8, (7, 3, 5)),
                                             (14, 8, (0, 0, 0)), (15, 5, (40, 2, 17)), (16, 2, (1, 1, 1))])
def test_orx_slab_plan_matches_python(seed, world, halo):
    nb = multigpu.SLAB_BINS
    words = random_hists(seed, world, nb)
    hists, vox, box = multigpu.split_slab_hists(words, world, nb)
    dist, costs = plan_margins(hists, vox, world)
    print(f"seed {seed} world {world}: least distance to an integer {dist:.3e}, axis costs {costs}")
    assert dist > 1e-6, dist
    cs = sorted(costs)
    assert min((cs[1] - cs[0]) / cs[1], (cs[2] - cs[1]) / cs[2]) > 1e-9, costs
    axis, bin_dest, counts = multigpu.slab_plan(hists, world, vox, list(halo))

    lib = renderer.load_library()
    assert lib.orx_slab_histogram_words(nb) == multigpu.slab_hist_words(nb)
    c_axis = C.c_uint32(99)
    c_dest = np.full(nb, 0xFF, np.uint8)
    c_counts = np.zeros((world, world), np.uint64)
    c_box = np.zeros(6, np.uint32)
    c_halo = (C.c_uint32 * 3)(*halo)
    st = lib.orx_slab_plan(words.ctypes.data, world, nb, c_halo, C.byref(c_axis), c_dest.ctypes.data,
                           c_counts.ctypes.data, c_box.ctypes.data)
    assert st == _abi.ORX_OK
    assert c_axis.value == axis
    assert np.array_equal(c_dest, bin_dest)
    assert np.array_equal(c_counts.astype(np.int64), counts)
    assert np.array_equal(c_box, box)
    assert counts.sum() >= hists[:, 0, axis].sum() and len(set(bin_dest.tolist())) == world
    for r in range(world):  # slab_owned's ranges are the table's
        lo, hi = multigpu.slab_owned(bin_dest, r)
        assert (c_dest[lo:hi + 1] == r).all() and (c_dest == r).sum() == hi - lo + 1


@pytest.mark.parametrize("world,nbins", [(0, 1024), (65, 1024), (2, 0), (2, 48), (2, 2048)])
def test_orx_slab_plan_rejects_bad_sizes(world, nbins):
    lib = renderer.load_library()
    words = np.zeros(2 * multigpu.slab_hist_words(1024), np.uint32)
    axis = C.c_uint32()
    dest = np.zeros(2048, np.uint8)
    counts = np.zeros((65, 65), np.uint64)
    st = lib.orx_slab_plan(words.ctypes.data, world, nbins, None, C.byref(axis), dest.ctypes.data, counts.ctypes.data,
                           None)
    assert st == _abi.ORX_ERR_INVALID_ARGUMENT
