"""What the convergence statistics and the display resolve cost on ONE GPU (not a gate; bench.py measures
the project).

Runs the hall 1080p PPM bench schedule (BASELINE.json configs[2]: the single-device pipelined path bench.py
times) with orx_set_convergence off and on, alternating in one process so that drift hits both alike.  Each
timed region is `steps` iterations plus one output readback.  Reports the frame time both ways,
orx_stats.pass_ms[ORX_PASS_CONVERGENCE] per iteration (HIP events around the update on the gather stream) and
the wall time of one orx_get_convergence and one orx_get_display (each synchronous, after the frame is
finished), and writes profiles/convergence_hall.json.

--bench-this / --bench-parent take files that hold the JSON result line of `python bench.py` on this tree
and on the parent commit: both lines are recorded in the same profile, since the default path (statistics
off) launches nothing new and the two should agree within the run-to-run spread.

    python tools/convergence_bench.py [--steps 32] [--warmup 4] [--repeats 3]
                                      [--bench-this FILE --bench-parent FILE] [--out profiles/convergence_hall.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SEED = 1645301512


def last_json_line(path):
    """the last line of `path` that parses as a JSON object (bench.py prints one result line)"""
    found = None
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith("{"):
                try:
                    found = json.loads(line)
                except ValueError:
                    pass
    return found


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=32)
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--photon-launch", type=int, default=2048)
    p.add_argument("--scene", default="SyntheticHall")
    p.add_argument("--floor", type=float, default=1e-3)
    p.add_argument("--threshold", type=float, default=0.05)
    p.add_argument("--bench-this", help="file with bench.py's result line on this tree")
    p.add_argument("--bench-parent", help="file with bench.py's result line on the parent commit")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "convergence_hall.json"))
    a = p.parse_args()

    from oppositerenderer_amd import _abi, multigpu, scenes
    from oppositerenderer_amd.renderer import OptixRenderer, RenderRequestDetails

    W, H, P = a.width, a.height, a.photon_launch
    scene = scenes.scene_by_name(a.scene)
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
    det = RenderRequestDetails(cam, scene.name, _abi.PROGRESSIVE_PHOTON_MAPPING, W, H)
    n = a.warmup + a.steps
    radii = multigpu.radius_sequence(scene.initial_ppm_radius(), n)

    res = {False: {"ms": []}, True: {"ms": [], "pass_ms": [], "query_ms": [], "display_ms": [], "mean_error": []}}
    images = {False: [], True: []}
    for _ in range(a.repeats):
        for on in (False, True):
            r = OptixRenderer(_abi.default_config(seed=SEED, photon_launch_width=P, photon_launch_height=P))
            r.initialize(0)
            r.initScene(scene)
            r.setConvergence(on)
            for i in range(a.warmup):
                r.renderNextIteration(i, i, radii[i], False, det)
            r.getOutputBuffer()
            r.reset_timing()
            t0 = time.perf_counter()
            for i in range(a.warmup, n):
                r.renderNextIteration(i, i, radii[i], False, det)
            images[on].append(r.getOutputBuffer().copy())
            res[on]["ms"].append((time.perf_counter() - t0) * 1e3 / a.steps)
            assert r.pipelined()
            if on:
                res[on]["pass_ms"].append(float(r.stats().pass_ms[_abi.PASS_CONVERGENCE]) / a.steps)
                r.getConvergence(a.floor, a.threshold)  # first call allocates its planes
                t0 = time.perf_counter()
                c = r.getConvergence(a.floor, a.threshold)
                res[on]["query_ms"].append((time.perf_counter() - t0) * 1e3)
                res[on]["mean_error"].append(float(c.mean_error))
                assert c.iterations == n
            r.getDisplayBuffer(1.0 / n)
            t0 = time.perf_counter()
            r.getDisplayBuffer(1.0 / n, 1.0 / 2.2, _abi.DISPLAY_BGRA8)
            res[True]["display_ms"].append((time.perf_counter() - t0) * 1e3)
            r.destroy()
            print(f"convergence {'on ' if on else 'off'}: {res[on]['ms'][-1]:.4f} ms/step", flush=True)

    def rel_l2(x, y):
        x, y = x.astype(np.float64), y.astype(np.float64)
        return float(np.sqrt(((x - y) ** 2).sum() / (y ** 2).sum()))

    # The statistics only read the sum.  At this size the frame is not bit-reproducible from run to run (the grid
    # build places a cell's photons in the order its atomics resolve, so the gather's fp32 sums differ in the last
    # bits), so on is compared with off against the spread between the off runs themselves.
    off_off = max([rel_l2(x, images[False][0]) for x in images[False][1:]] or [0.0])
    on_off = max(rel_l2(x, images[False][0]) for x in images[True])
    bits = images[False][0].tobytes()
    same_off = all(x.tobytes() == bits for x in images[False][1:])
    same_on = all(x.tobytes() == bits for x in images[True])

    def med(v):
        return round(float(np.median(v)), 4)

    off, on = med(res[False]["ms"]), med(res[True]["ms"])
    out = {
        "what": "one MI355X, one process: the pipelined PPM frame with orx_set_convergence off and on, alternating",
        "workload": f"{scene.name} {W}x{H} PPM, {P * P:,} photons/iter", "steps": a.steps, "warmup": a.warmup,
        "timed_region": "steps iterations + one output readback",
        "off_ms_per_step": [round(v, 4) for v in res[False]["ms"]], "on_ms_per_step": [round(v, 4) for v in res[True]["ms"]],
        "off_ms_per_step_median": off, "on_ms_per_step_median": on, "on_over_off": round(on / off, 4),
        "convergence_pass_ms_per_step": [round(v, 5) for v in res[True]["pass_ms"]],
        "convergence_pass_ms_per_step_median": round(float(np.median(res[True]["pass_ms"])), 5),
        "convergence_pass_bytes_per_step": W * H * 52,
        "get_convergence_ms": [round(v, 4) for v in res[True]["query_ms"]], "get_convergence_ms_median": med(res[True]["query_ms"]),
        "get_display_ms": [round(v, 4) for v in res[True]["display_ms"]], "get_display_ms_median": med(res[True]["display_ms"]),
        "mean_error_after_steps": res[True]["mean_error"][-1],
        "rel_l2_off_vs_off": off_off, "rel_l2_on_vs_off": on_off,
        "bit_equal_off_vs_off": same_off, "bit_equal_on_vs_off": same_on,
    }
    for key, path in (("bench_this_tree", a.bench_this), ("bench_parent_commit", a.bench_parent)):
        if path:
            out[key] = last_json_line(path)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
