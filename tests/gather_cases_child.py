"""Child process of tests/test_gpu_gather_injected.py::test_device_cases_other_kernels (TEST INFRASTRUCTURE;
needs a GPU).  ORX_GATHER_DFORM and ORX_GATHER_KERNEL are read once per process, so each setting runs in a
process of its own: gather_cases.SETTING_CASES in both photon layouts, each grid checked here
(gather_cases.check_grid), the gather outputs stored in the .npz named by argv[1] for the parent, which holds
the references.  Prints one JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

import gather_cases as gc  # noqa: E402
import test_gpu_gather_injected as t  # noqa: E402
from oppositerenderer_amd import _abi  # noqa: E402


def main():
    out, grids = {}, {}
    for variant in t.VARIANTS:
        for name in gc.SETTING_CASES:
            case = gc.all_cases()[name]
            b = t.device_shard(case.P, variant)
            got = gc.run_case(b, case, t.to_device)
            grids[f"{variant}/{name}"] = gc.check_grid(case, b.r.stats(), b.r.read_buffer(_abi.BUF_PHOTONS),
                                                       b.r.read_buffer(_abi.BUF_GRID_OFFSETS, np.uint32),
                                                       f"child layout {variant}")
            out[f"{variant}/{name}"] = got
    for b in t._SHARDS.values():
        b.r.destroy()
    np.savez(sys.argv[1], **out)
    env = {k: os.environ[k] for k in ("ORX_GATHER_DFORM", "ORX_GATHER_KERNEL") if k in os.environ}
    print(json.dumps({"env": env, "grids": grids}), flush=True)


if __name__ == "__main__":
    main()
