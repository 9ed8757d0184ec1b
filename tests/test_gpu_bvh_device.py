"""tests/bvh_device_check.hip on the device: the device BVH builder's trees walked node by node, compared with the
host builder's, and the traversal loops of orx_traverse.h (trace_closest, trace_closest_t over StackH<16> and
StackH<4>, trace_any, trace_any_t, trace_any_chain) against a brute-force search with the product's triangle
formula, bit for bit, on deep, flat, far, huge, identical-triangle, zero-area and tiny meshes under five option
sets.  What it asserts per mesh and option set is listed at the top of that file; it is a program of its own, built
by the Makefile of oppositerenderer_amd/csrc, so a HIP error ends it without touching this process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oppositerenderer_amd", "csrc")
BIN = os.path.join(ROOT, "oppositerenderer_amd", "bvh_device_check")

pytestmark = pytest.mark.gpu

MESHES = 5 + 13   # one triangle and four jittered grids, then bvh_check_common.h's degenerate_cases()
OPTION_SETS = 5


def binary():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", CSRC, "../bvh_device_check"])
    return BIN


def test_device_bvh_structure_and_traversal_match_brute_force():
    r = subprocess.run([binary()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "all checks passed", r.stdout[-4000:]
    cases = [line for line in lines if " triangles " in line and " nodes depth " in line]
    assert len(cases) == MESHES * OPTION_SETS, len(cases)
    assert not any("RAYS DIFFER" in line for line in cases)
