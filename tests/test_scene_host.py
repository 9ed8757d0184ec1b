"""Scene preparation on the host (oppositerenderer_amd/csrc/orx_scene_host.cpp) on the CPU: tests/scene_host_check.cpp is
built with that source and nothing else (no HIP, no liborx.so) under AddressSanitizer + UndefinedBehaviorSanitizer and
run as a program of its own.  What it asserts is listed at the top of that file."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oppositerenderer_amd", "csrc")


def test_scene_validation_conversion_leaf_arrays_and_texture_layout(tmp_path):
    exe = str(tmp_path / "scene_host_check")
    # the sanitizer runtimes are linked into the program: it then starts whatever else the environment preloads
    # (the shared runtime refuses to start unless it is the first library loaded)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "scene_host_check.cpp"),
                           os.path.join(CSRC, "orx_scene_host.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:]
    assert "all checks passed" in run.stdout
