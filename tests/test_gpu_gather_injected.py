"""The device's photon grid build and gather on injected photons and hit points (tests/gather_cases.py) against
the float64 brute force: k_grid_setup, k_bs_*, k_grid_permute, k_gather_tiles and the gather kernels, through
orx_ppm_slab_import and orx_ppm_gather_external, in both photon layouts (gather_variant 1: cell order, NSUB = 1;
2: sub-rows) and, in child processes, the other kernel instantiations (ORX_GATHER_DFORM=0: DF = false;
ORX_GATHER_KERNEL=2: the per-lane k_ppm_gather<1> / <4>).

One renderer per (photon launch edge, layout) serves every case in turn, so an import must leave nothing behind
for the next one (a dense cell, an empty import, a grid that was too large).  After every import the grid is
checked on its own (gather_cases.check_grid) and against the oracle's grid over the same records (sizes, cell,
origin and offsets bit-equal), then the gather against the reference over the imported records, which
check_grid has shown to be the device's photons bit for bit: a grid fault and a gather fault fail different
assertions."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gather_cases as gc
from oppositerenderer_amd import _abi, multigpu, scenes
from oppositerenderer_amd.renderer import OptixRenderer, OrxError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = (1, 2)
_SHARDS = {}


def device_shard(P, variant):
    if (P, variant) not in _SHARDS:
        r = OptixRenderer(_abi.default_config(seed=gc.SEED, photon_launch_width=P, photon_launch_height=P,
                                              gather_variant=variant))
        r.initialize(0)
        r.initScene(scenes.cornell())
        b = multigpu.DeviceShard(r, torch, torch.device("cuda", 0))
        b.enable_slab()
        _SHARDS[(P, variant)] = b
    return _SHARDS[(P, variant)]


@pytest.fixture(scope="module", autouse=True)
def _renderers():
    yield
    for b in _SHARDS.values():
        b.r.destroy()
    _SHARDS.clear()


def to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).to(torch.device("cuda", 0))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def check_grid_against_oracle(case, b, label):
    from test_gather_cases_cpu import oracle_shard, to_cpu

    o = oracle_shard(case.P)
    gc.import_case(o, case, to_cpu)
    gs, os_ = b.r.stats(), o.r.stats()
    assert list(gs.grid_size) == list(os_.grid_size), (label, case.name, list(gs.grid_size), list(os_.grid_size))
    assert same_bits([gs.cell_size], [os_.cell_size]), (label, case.name, gs.cell_size, os_.cell_size)
    assert same_bits(list(gs.world_origin), list(os_.world_origin)), (label, case.name)
    assert gs.valid_photons == os_.valid_photons
    assert np.array_equal(b.r.read_buffer(_abi.BUF_GRID_OFFSETS, np.uint32),
                          o.r.read_buffer(_abi.BUF_GRID_OFFSETS, np.uint32)), (label, case.name, "cell offsets")


def run_device(case, variant):
    b = device_shard(case.P, variant)
    label = f"device layout {variant}"
    got = gc.run_case(b, case, to_device)
    desc = gc.check_grid(case, b.r.stats(), b.r.read_buffer(_abi.BUF_PHOTONS),
                         b.r.read_buffer(_abi.BUF_GRID_OFFSETS, np.uint32), label)
    check_grid_against_oracle(case, b, label)
    if case.box is not None:  # origin and cell follow the caller's box
        lo = np.array([float(v) for v in b.r.stats().world_origin], np.float32)
        assert np.array_equal(lo, gc.ord2f(case.box[:3]) - np.float32(0.0000001)), desc  # padAABB
    worst = gc.check_estimate(case, got, label)
    print(f"{label} {case.name}: {desc}; worst |got - lo| / bound {worst:.3f}")
    for k, r in enumerate(gc.expected(case)):  # exact zeros: unflagged, not owned, no photon in reach
        zero = (r.lo == 0) & (r.amb == 0)
        assert (got[k][zero] == 0).all(), (label, case.name)
    return got


CASES = [n for n in gc.all_cases() if n != "grid_too_large"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", CASES)
def test_device_case(name, variant):
    case = gc.all_cases()[name]
    got = run_device(case, variant)
    if case.n == 0:  # an empty import: all zeros, status OK
        assert (got == 0).all()
        b = device_shard(case.P, variant)
        assert b.r.stats().valid_photons == 0
        b.r.getOutputBuffer()


@pytest.mark.parametrize("variant", VARIANTS)
def test_device_chord_edge(variant):
    """a chord start within rounding of a quarter-cell face (gather_cases.chord_edge_case): the grid of the
    caller's box is read back from the device, then the case is built for that grid"""
    probe = gc.chord_probe_case()
    b = device_shard(probe.P, variant)
    gc.import_case(b, probe, to_device)
    s = b.r.stats()
    case = gc.chord_edge_case(s.world_origin[0], s.cell_size)
    run_device(case, variant)
    s2 = b.r.stats()
    assert (list(s2.grid_size), np.float32(s2.cell_size)) == (list(s.grid_size), np.float32(s.cell_size))


@pytest.mark.parametrize("variant", VARIANTS)
def test_device_grid_too_large(variant):
    """500 photons on the plane z = 100: the reference's cell-size arithmetic overflows the cell budget.  The
    import and the gather return OK, the gather writes exact zeros, orx_get_output reports
    ORX_ERR_GRID_TOO_LARGE; the next import on the same renderer is unaffected.  (The grid is left with G = 0:
    k_bs_count keys nothing, the scans and k_bs_cells see no bucket, k_gather_tiles and both gather kernels
    test g.G before they form a window.)"""
    case = gc.all_cases()["grid_too_large"]
    b = device_shard(case.P, variant)
    got = gc.run_case(b, case, to_device)
    assert (got == 0).all()
    with pytest.raises(OrxError) as e:
        b.r.getOutputBuffer()
    assert e.value.status == _abi.ORX_ERR_GRID_TOO_LARGE
    run_device(gc.all_cases()["random_s1"], variant)
    b.r.getOutputBuffer()


SETTINGS = {"dform0": {"ORX_GATHER_DFORM": "0"}, "lane": {"ORX_GATHER_KERNEL": "2"}}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_device_cases_other_kernels(setting, tmp_path):
    """ORX_GATHER_DFORM and ORX_GATHER_KERNEL are read once per process: a child (tests/gather_cases_child.py)
    runs gather_cases.SETTING_CASES in both layouts, checks each grid and stores the estimates; the bound is
    asserted here, against this process's references"""
    out = tmp_path / "got.npz"
    env = dict(os.environ, **SETTINGS[setting])
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "gather_cases_child.py"), str(out)], env=env,
                       capture_output=True, text=True, timeout=150, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["env"] == SETTINGS[setting]
    got = np.load(out)
    for variant in VARIANTS:
        for name in gc.SETTING_CASES:
            case = gc.all_cases()[name]
            label = f"device {setting} layout {variant}"
            worst = gc.check_estimate(case, got[f"{variant}/{name}"], label)
            print(f"{label} {name}: {res['grids'][f'{variant}/{name}']}; worst |got - lo| / bound {worst:.3f}")
