#!/usr/bin/env python3
"""VCM with and without vertex merging (orx_config.vcm_merging) on the 1080p hall, the bench's
configs[3] scene: ms/frame of both, alternated in one process, the two merging passes' device time,
and, from a separate untimed run with debug counters, the candidate and accepted pairs and the
algorithmic bytes of the merge kernel.  Writes profiles/vcm_merging_hall.json.

    python tools/vcm_merge_bench.py [--steps 20] [--warmup 5] [--width 1920 --height 1080]

The two bounds the merge kernel is held against:
  bytes  camera records (64 B) + light records once (48 B) + 16 B per candidate (the first plane of a
         light record) + 32 B per accepted pair (the other two), at the 6.29 TB/s a float4 copy reaches
  issue  VALU lane-instructions at the chip's fp32 vector rate (157.3 TFLOPS / 2 per FMA): about
         VALU_PER_CANDIDATE per distance test and VALU_PER_ACCEPTED per accepted pair, counted from the
         kernel's source (no divergence or latency in it: a floor, not a model)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12
LANE_INSTR_PER_S = 157.3e12 / 2
VALU_PER_CANDIDATE = 14     # load issue, 3 sub, 3 mul, 2 add, compare, counter, loop
VALU_PER_ACCEPTED = 150     # frame transform, vcm_f of one or two lobes, the two weights, a division, 9 fma-less mul/add


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--rounds", type=int, default=2, help="off/on alternations; --steps is split over them")
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--scene", default="SyntheticHall")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcm_merging_hall.json"))
    a = p.parse_args(argv)
    if a.steps < 20 or a.warmup < 5:
        print("note: fewer than 20 timed / 5 warm-up iterations", file=sys.stderr)

    from oppositerenderer_amd import _abi, scenes
    from oppositerenderer_amd.renderer import OptixRenderer, RenderRequestDetails, next_ppm_radius

    scene = scenes.scene_by_name(a.scene)
    W, H = a.width, a.height
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
    det = RenderRequestDetails(cam, scene.name, _abi.VCM_BIDIRECTIONAL_PATH_TRACING, W, H)

    def renderer(merging, debug):
        r = OptixRenderer(_abi.default_config(seed=1645301512, photon_launch_width=2048, photon_launch_height=2048,
                                              vcm_merging=merging, debug_counters=debug))
        r.initialize(0)
        r.initScene(scene)
        return r

    class Run:
        def __init__(self, merging):
            self.r = renderer(merging, 0)
            self.it = 0
            self.radius = scene.initial_ppm_radius()
            self.wall = 0.0
            self.steps = 0

        def go(self, n, timed):
            if timed:
                self.r.stats()  # synchronise
                t0 = time.perf_counter()
            for _ in range(n):
                self.r.renderNextIteration(self.it, self.it, self.radius, False, det)
                self.radius = next_ppm_radius(self.radius, self.it)
                self.it += 1
            if timed:
                self.r.stats()  # synchronise
                self.wall += time.perf_counter() - t0
                self.steps += n

    runs = {0: Run(0), 1: Run(1)}
    for m in (0, 1):
        runs[m].go(a.warmup, False)
        runs[m].r.stats()
        runs[m].r.reset_timing()
    per_round = [a.steps // a.rounds + (1 if i < a.steps % a.rounds else 0) for i in range(a.rounds)]
    for n in per_round:
        for m in (0, 1):
            runs[m].go(n, True)
    st = runs[1].r.stats()
    n_it = max(1, st.timed_iterations)
    passes = {name: st.pass_ms[i] / n_it for i, name in enumerate(_abi.PASS_NAMES) if st.pass_ms[i] > 0}
    grid_ms = st.pass_ms[_abi.PASS_VCM_GRID] / n_it
    merge_ms = st.pass_ms[_abi.PASS_VCM_MERGE] / n_it
    last_radius = runs[1].radius
    ms = {m: runs[m].wall * 1e3 / max(1, runs[m].steps) for m in (0, 1)}
    for m in (0, 1):
        runs[m].r.destroy()

    # the pair counts: one untimed iteration sequence with debug counters, up to the timed region's middle
    dbg = renderer(1, 1)
    radius = scene.initial_ppm_radius()
    mid = a.warmup + a.steps // 2
    for it in range(mid + 1):
        dbg.renderNextIteration(it, it, radius, False, det)
        if it < mid:
            radius = next_ppm_radius(radius, it)
    cand = int(dbg.read_buffer(_abi.BUF_VCM_MERGE_CANDIDATES, np.uint32).astype(np.int64).sum())
    acc = int(dbg.read_buffer(_abi.BUF_VCM_MERGE_COUNT, np.uint32).astype(np.int64).sum())
    ncam = int(dbg.read_buffer(_abi.BUF_VCM_CAMERA_VERTEX_COUNT, np.uint32).astype(np.int64).sum())
    nlight = int(np.minimum(dbg.read_buffer(_abi.BUF_VCM_VERTEX_COUNT, np.uint32), 9).astype(np.int64).sum())
    dbg.destroy()
    alg_bytes = ncam * 64 + nlight * 48 + cand * 16 + acc * 32
    bytes_ms = alg_bytes / HBM_BYTES_PER_S * 1e3
    issue_ms = (cand * VALU_PER_CANDIDATE + acc * VALU_PER_ACCEPTED) / LANE_INSTR_PER_S * 1e3
    res = {
        "workload": f"{a.scene} {W}x{H} VCM, seed 1645301512, radius schedule from the scene's initial PPM radius",
        "timing": "builder-timed: host wall clock around the timed iterations, ending in a synchronise; "
                  "pass times from HIP events",
        "warmup": a.warmup, "steps": runs[0].steps, "rounds": a.rounds,
        "ms_per_frame_merging_off": round(ms[0], 4), "ms_per_frame_merging_on": round(ms[1], 4),
        "vcm_grid_ms": round(grid_ms, 4), "vcm_merge_ms": round(merge_ms, 4),
        "pass_ms_merging_on": {k: round(v, 4) for k, v in passes.items()},
        "counted_at_iteration": mid, "radius_there": radius, "radius_after_timed_region": last_radius,
        "camera_vertices": ncam, "light_vertices": nlight, "candidate_pairs": cand, "accepted_pairs": acc,
        "merge_algorithmic_bytes": alg_bytes,
        "merge_bytes_bound_ms": round(bytes_ms, 4), "merge_issue_bound_ms": round(issue_ms, 4),
        "merge_nearer_bound": "issue" if abs(merge_ms - issue_ms) < abs(merge_ms - bytes_ms) else "bytes",
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
