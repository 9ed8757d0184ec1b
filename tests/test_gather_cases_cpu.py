"""The injected photon-grid and gather cases (tests/gather_cases.py) on the CPU oracle: every case meets its
caps (conditions on the inputs, asserted by the reference), the oracle's grid passes the structure check and
its gather lies inside the derived bound.  So a machine without a GPU proves that the inputs the device test
uses keep the reference inside its caps, and the oracle's own gather is tested at the same edges.  Two
closed-form checks pin the reference itself."""
import numpy as np
import pytest
import torch

import gather_cases as gc
import oracle_lib
from oppositerenderer_amd import _abi, scenes

_ORACLES = {}


def oracle_shard(P):
    if P not in _ORACLES:
        r = oracle_lib.OracleRenderer(_abi.default_config(seed=gc.SEED, photon_launch_width=P, photon_launch_height=P))
        r.init_scene(scenes.cornell())
        b = oracle_lib.OracleShard(r, torch)
        b.set_shard(0, 1)
        _ORACLES[P] = b
    return _ORACLES[P]


def to_cpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).copy())


def run_oracle(case):
    b = oracle_shard(case.P)
    got = gc.run_case(b, case, to_cpu)
    desc = gc.check_grid(case, b.r.stats(), b.r.read_buffer(_abi.BUF_PHOTONS),
                         b.r.read_buffer(_abi.BUF_GRID_OFFSETS, np.uint32), "oracle")
    worst = gc.check_estimate(case, got, "oracle")
    print(f"oracle {case.name}: {desc}; worst |got - lo| / bound {worst:.3f}")
    return got, worst


CASES = [n for n in gc.all_cases() if n != "grid_too_large"]


@pytest.mark.parametrize("name", CASES)
def test_oracle_case(name):
    case = gc.all_cases()[name]
    got, _ = run_oracle(case)
    exp = gc.expected(case)
    for k, r in enumerate(exp):  # exact zeros: unflagged, not owned, no photon
        zero = (r.lo == 0) & (r.amb == 0)
        assert (got[k][zero] == 0).all(), name
    if case.n == 0:
        assert (got == 0).all()


def test_oracle_chord_edge():
    """two phases: the grid of the caller's box is read back, then the case is built for that grid"""
    probe = gc.chord_probe_case()
    b = oracle_shard(probe.P)
    gc.import_case(b, probe, to_cpu)
    s = b.r.stats()
    case = gc.chord_edge_case(s.world_origin[0], s.cell_size)
    got, _ = run_oracle(case)
    assert gc.case_reference(case).n_acc.tolist() == [2] * (case.W * case.H)  # on the sphere, and one unit inside
    assert same_grid(b.r.stats(), s)


def same_grid(a, b):
    return (list(a.grid_size), np.float32(a.cell_size), [np.float32(v) for v in a.world_origin]) == \
           (list(b.grid_size), np.float32(b.cell_size), [np.float32(v) for v in b.world_origin])


def test_oracle_grid_too_large_then_random():
    """500 photons on the plane z = 100: the reference's own cell-size arithmetic overflows the cell budget and
    the oracle refuses the import; the next import on the same renderer is unaffected"""
    case = gc.all_cases()["grid_too_large"]
    with pytest.raises(RuntimeError, match="Too many cells"):
        gc.run_case(oracle_shard(case.P), case, to_cpu)
    run_oracle(gc.all_cases()["random_s1"])


def test_random_case_is_what_the_issue_sizes():
    c = gc.all_cases()["random_s3"]
    assert (c.n, c.W, c.H, c.segments, c.P) == (16000, 50, 37, 3, 64)
    assert gc.export_plane(c.W, c.H) == 1852 and len(gc.pack_hitpoints(c)) == 3 * 1852 * 7
    ref = gc.case_reference(c)
    assert 15 < ref.n_acc[c.flagged].mean() < 40 and (~c.flagged).sum() > 100
    for c in gc.all_cases().values():
        assert c.n * c.W * c.H <= gc.MAX_PAIRS, c.name


def test_lattice_twins_lose_exactly_the_photon_on_the_sphere():
    """on each axis line the hit point at the centre accepts the 11 photons at distances 0..5 (d^2 == 25
    included); moved one ulp either way it loses the one photon that is now outside"""
    c = gc.all_cases()["lattice_boundary"]
    ref = gc.case_reference(c)
    assert ref.n_acc[:9].tolist() == [11, 10, 10] * 3
    assert (ref.n_amb == 0).all() and (ref.n_acc[9:23] > 20).all()


def one_photon_reference(dist, radius=5.0, P=64):
    ph = gc._records([[200.0 + dist, 300.0, 250.0]], [[0.0, -1.0, 0.0]], [[0.5, 0.25, 1.0]])
    return gc.reference(ph, [[200.0, 300.0, 250.0]], [[0.0, 1.0, 0.0]], [True], radius, P, margin=0.0)


def test_reference_one_photon_at_distance_zero():
    """u = 0: w = alpha exactly; indirect = alpha * power / (pi 25) / 4096"""
    ref = one_photon_reference(0.0)
    want = 1.818 * np.array([0.5, 0.25, 1.0]) / (np.pi * 25.0) / 4096.0
    assert ref.n_acc[0] == 1 and (ref.amb == 0).all()
    np.testing.assert_allclose(ref.lo[0], want, rtol=1e-15)
    # bound: b(0) = 2e-6 + 8 eps + 12 eps |c0| / alpha, plus (1 + 4) eps, relative to the estimate
    b0 = 2e-6 + 8 * gc.EPS + 12 * gc.EPS * gc.w5_abs_coefficients()[0] / 1.818
    np.testing.assert_allclose(ref.bound[0] / ref.lo[0], b0 + 5 * gc.EPS, rtol=1e-12)


def test_reference_one_photon_on_the_sphere():
    """d^2 == r2 (u = 1) is accepted: w = alpha (1 - (1 - e^(-beta/2)) / (1 - 0.141847)); one ulp further out
    along the axis that carries the distance is rejected"""
    ref = one_photon_reference(5.0)
    w1 = 1.818 * (1.0 - (1.0 - np.exp(-1.953 / 2.0)) / (1.0 - 0.141847))
    assert abs(w1 - 0.49731) < 1e-4  # evaluated by hand
    assert ref.n_acc[0] == 1
    np.testing.assert_allclose(ref.lo[0], w1 * np.array([0.5, 0.25, 1.0]) / (np.pi * 25.0) / 4096.0, rtol=1e-15)
    out = one_photon_reference(float(np.nextafter(np.float32(205.0), np.float32(300.0))) - 200.0)
    assert out.n_acc[0] == 0 and (out.lo == 0).all() and (out.amb == 0).all()
    # facing away, and a hit point without the flag
    ph = gc._records([[203.0, 300.0, 250.0]], [[0.0, 1.0, 0.0]], [[1.0, 1.0, 1.0]])
    assert gc.reference(ph, [[200.0, 300.0, 250.0]], [[0.0, 1.0, 0.0]], [True], 5.0, 64, margin=0.0).n_acc[0] == 0
    ph[0, 3:6] = [1.0, 0.0, 0.0]  # n.d == 0 is accepted
    assert gc.reference(ph, [[200.0, 300.0, 250.0]], [[0.0, 1.0, 0.0]], [True], 5.0, 64, margin=0.0).n_acc[0] == 1
    assert gc.reference(ph, [[200.0, 300.0, 250.0]], [[0.0, 1.0, 0.0]], [False], 5.0, 64, margin=0.0).n_acc[0] == 0
