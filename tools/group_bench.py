"""What the render-group layer costs on ONE GPU (not a gate; bench.py measures the project).

Times the hall 1080p PPM frame (BASELINE.json configs[2]) in one process through a plain
OptixRenderer (orx_render_next_iteration: the single-device pipelined path bench.py times) and
through a world-1 ROWS group (orx_create_group, pipelined schedule, LOCAL communicator: the phase
API with the hit-point all-gather, the reduce-scatter and the finish stream, each over one rank).
Both timed regions are `steps` iterations plus one output readback, which synchronises either
path.  Writes both figures to profiles/group_world1_hall.json.

The pipelined group keeps the compute, aux, gather, finish and communication streams busy at once;
like bench.py's multi-GPU paths (bench.py hw_queues) the tool therefore raises GPU_MAX_HW_QUEUES to
16 before the first HIP call when it is below 8 or unset (--hw-queues 0 keeps the caller's value),
for both renderers, and records the value used.

--ranks N puts N ranks on the one device (still LOCAL), and --photons rows|slabs|both chooses what the ranks
gather against (orx_group_config.photon_partition; both: the two groups interleaved in every repeat, so that
drift hits them alike).  Each group prints every rank's ORX_PASS_PPM_GATHER milliseconds per iteration (HIP
events on the rank's gather stream) and their sum.  All ranks share one GPU, so this prices the per-rank gather
work of a partition, not a multi-GPU frame: the ranks' kernels time-slice one device and there is no xGMI.

    python tools/group_bench.py [--steps 32] [--warmup 4] [--hw-queues 16] [--out profiles/group_world1_hall.json]
    python tools/group_bench.py --ranks 8 --photons both --out profiles/group_world8_hall_photons.json
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


def timed(r, det, radii, warmup, steps, after_warmup=None):
    """ms per iteration over `steps` iterations + one output readback, and that image"""
    for i in range(warmup):
        r.renderNextIteration(i, i, radii[i], False, det)
    r.getOutputBuffer()
    if after_warmup:
        after_warmup()
    t0 = time.perf_counter()
    for i in range(warmup, warmup + steps):
        r.renderNextIteration(i, i, radii[i], False, det)
    img = r.getOutputBuffer()
    return (time.perf_counter() - t0) * 1e3 / steps, img


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=32)
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--photon-launch", type=int, default=2048)
    p.add_argument("--scene", default="SyntheticHall")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_world1_hall.json"))
    p.add_argument("--hw-queues", type=int, default=16, help="GPU_MAX_HW_QUEUES when the caller's is below 8 (0: keep)")
    p.add_argument("--ranks", type=int, default=1, help="ranks of the group, all on device 0")
    p.add_argument("--photons", choices=("rows", "slabs", "both"), default="rows",
                   help="orx_group_config.photon_partition of the group(s)")
    p.add_argument("--serial", action="store_true", help="the group's serial phases (pipeline = 0)")
    a = p.parse_args()
    inherited = os.environ.get("GPU_MAX_HW_QUEUES")
    if a.hw_queues and (inherited is None or int(inherited or 0) < 8):
        os.environ["GPU_MAX_HW_QUEUES"] = str(a.hw_queues)  # before liborx.so makes its first HIP call

    from oppositerenderer_amd import _abi, multigpu, scenes
    from oppositerenderer_amd.group import OptixRendererGroup
    from oppositerenderer_amd.renderer import OptixRenderer, RenderRequestDetails

    W, H, P = a.width, a.height, a.photon_launch
    scene = scenes.scene_by_name(a.scene)
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
    det = RenderRequestDetails(cam, scene.name, _abi.PROGRESSIVE_PHOTON_MAPPING, W, H)
    radii = multigpu.radius_sequence(scene.initial_ppm_radius(), a.warmup + a.steps)

    def cfg():
        return _abi.default_config(seed=SEED, photon_launch_width=P, photon_launch_height=P)

    modes = ["rows", "slabs"] if a.photons == "both" else [a.photons]
    part = {"rows": _abi.PHOTONS_ROWS, "slabs": _abi.PHOTONS_SLABS}
    per_mode = {m: {"ms": [], "gather": [], "err": None} for m in modes}
    plain = []
    for _ in range(a.repeats):  # interleaved, so that drift hits both alike
        r = OptixRenderer(cfg())
        r.initialize(0)
        r.initScene(scene)
        ms, ref = timed(r, det, radii, a.warmup, a.steps)
        ref = ref.copy()
        plain.append(ms)
        r.destroy()
        for m in modes:
            g = OptixRendererGroup(cfg(), _abi.default_group_config(partition=_abi.GROUP_ROWS, comm=_abi.COMM_LOCAL,
                                                                    pipeline=0 if a.serial else 1,
                                                                    photon_partition=part[m]))
            g.initialize([0] * a.ranks)
            g.initScene(scene)
            ranks = [g.renderer(k) for k in range(a.ranks)]
            ms, img = timed(g, det, radii, a.warmup, a.steps, lambda: [r.reset_timing() for r in ranks])
            assert g.pipelined() == (not a.serial) and g.comm_name() == "local"
            gather = [float(r.stats().pass_ms[_abi.PASS_NAMES.index("ppm_gather")]) / a.steps for r in ranks]
            print(f"photons {m}: {ms:.4f} ms/step; ORX_PASS_PPM_GATHER ms per rank "
                  f"{[round(v, 4) for v in gather]} sum {sum(gather):.4f}", flush=True)
            per_mode[m]["ms"].append(ms)
            per_mode[m]["gather"].append(gather)
            g.destroy()
            per_mode[m]["err"] = float(np.sqrt(((img.astype(np.float64) - ref) ** 2).sum()
                                               / (ref.astype(np.float64) ** 2).sum()))
    group, err = per_mode[modes[0]]["ms"], per_mode[modes[0]]["err"]
    paths = W * H + P * P
    out = {
        "what": f"one MI355X, one process: plain renderer against a world-{a.ranks} ROWS render group "
                f"({'serial' if a.serial else 'pipelined'}, LOCAL, photons {modes[0]})",
        "ranks": a.ranks,
        "workload": f"{scene.name} {W}x{H} PPM, {P * P:,} photons/iter", "steps": a.steps, "warmup": a.warmup,
        "timed_region": "steps iterations + one output readback",
        "hw_queues": {"inherited": inherited, "used": os.environ.get("GPU_MAX_HW_QUEUES")},
        "plain_ms_per_step": [round(v, 4) for v in plain], "group_ms_per_step": [round(v, 4) for v in group],
        "plain_ms_per_step_median": round(float(np.median(plain)), 4),
        "group_ms_per_step_median": round(float(np.median(group)), 4),
        "plain_mpaths_per_s": round(paths / float(np.median(plain)) / 1e3, 1),
        "group_mpaths_per_s": round(paths / float(np.median(group)) / 1e3, 1),
        "group_over_plain": round(float(np.median(group)) / float(np.median(plain)), 4),
        "rel_l2_group_vs_plain": err,
        "photons": {m: {"ms_per_step": [round(v, 4) for v in d["ms"]],
                        "ms_per_step_median": round(float(np.median(d["ms"])), 4),
                        "gather_ms_per_rank_median": [round(float(v), 4) for v in np.median(d["gather"], axis=0)],
                        "gather_ms_sum_median": round(float(np.median(np.sum(d["gather"], axis=1))), 4),
                        "rel_l2_vs_plain": d["err"]} for m, d in per_mode.items()},
        "note": "one-GPU figures: the ranks share one device, so the per-rank gather times price the partition's "
                "gather work under time-slicing, not a multi-GPU frame; a group of N > 1 ranks over RCCL/xGMI is "
                "unmeasured on hardware",
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
