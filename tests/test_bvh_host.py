"""The host BVH builder (oppositerenderer_amd/csrc/orx_bvh_host.cpp) on the CPU: tests/bvh_host_check.cpp is built
with the builder's source and nothing else (no HIP, no liborx.so) under AddressSanitizer + UndefinedBehaviorSanitizer
and run as a program of its own.  What it asserts per mesh and option set is listed at the top of that file."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oppositerenderer_amd", "csrc")


def test_host_bvh_builder_structure_and_closest_hits(tmp_path):
    exe = str(tmp_path / "bvh_host_check")
    # the sanitizer runtimes are linked into the program: it then starts whatever else the environment preloads
    # (the shared runtime refuses to start unless it is the first library loaded)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "bvh_host_check.cpp"),
                           os.path.join(CSRC, "orx_bvh_host.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:]
    assert "all checks passed" in run.stdout
