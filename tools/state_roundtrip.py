"""How long orx_save_state and orx_restore_state take, so that a host can decide how often to save.

    python tools/state_roundtrip.py [--configs 2 4] [--repeats 3] [--out profiles/state_roundtrip.json]

For each bench.py config named, a Cornell renderer with that config's frame size and photon launch (the
blob's size depends on nothing else) renders one path-tracing iteration, then saves into a preallocated
host buffer and restores from it `repeats` times.  Both calls are synchronous (they end in a stream
synchronise), so a host clock around them is the call's wall time: device copy kernels, the transfers and
the FNV-1a checksums over the sections on the host.  The checksum is timed on its own as well
(orx_state_info_read over the blob).  The restored state is saved again and must equal the blob."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oppositerenderer_amd import _abi, scenes  # noqa: E402
from oppositerenderer_amd.renderer import OptixRenderer, RenderRequestDetails  # noqa: E402

SIZES = {2: (1920, 1080, 2048), 4: (3840, 2160, 4096)}  # bench.py CONFIGS: width, height, photon launch


def measure(config, repeats):
    W, H, P = SIZES[config]
    scene = scenes.cornell()
    r = OptixRenderer(_abi.default_config(seed=1645301512, photon_launch_width=P, photon_launch_height=P))
    r.initialize(0)
    r.initScene(scene)
    cam = scene.default_camera.set_aspect_ratio(W / H)
    r.renderNextIteration(0, 0, scene.initial_ppm_radius(), True, RenderRequestDetails(cam, scene.name, _abi.PATH_TRACING, W, H))
    r.getOutputBuffer()
    lib, h = r._lib, r._h
    n = lib.orx_state_bytes(h)
    buf, again = C.create_string_buffer(n), C.create_string_buffer(n)
    info = _abi.OrxStateInfo()
    save, restore, check = [], [], []
    for _ in range(repeats + 1):  # the first round warms the copy kernels' code objects and is dropped
        t0 = time.perf_counter()
        r._check(lib.orx_save_state(h, buf, n))
        t1 = time.perf_counter()
        assert lib.orx_state_info_read(buf, n, C.byref(info)) == _abi.ORX_OK
        t2 = time.perf_counter()
        r._check(lib.orx_restore_state(h, buf, n))
        t3 = time.perf_counter()
        save.append(t1 - t0)
        check.append(t2 - t1)
        restore.append(t3 - t2)
    r._check(lib.orx_save_state(h, again, n))
    assert buf.raw == again.raw, "a restore must leave exactly the saved state"
    r.destroy()
    med = lambda v: sorted(v[1:])[len(v[1:]) // 2]  # noqa: E731
    return {"config": config, "width": W, "height": H, "photon_launch": P, "blob_bytes": n,
            "rng_bytes": int(info.rng_width) * int(info.rng_height) * 24, "output_bytes": W * H * 12,
            "save_ms": round(med(save) * 1e3, 2), "restore_ms": round(med(restore) * 1e3, 2),
            "checksum_ms": round(med(check) * 1e3, 2),
            "save_ms_all": [round(v * 1e3, 2) for v in save[1:]], "restore_ms_all": [round(v * 1e3, 2) for v in restore[1:]]}


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--configs", type=int, nargs="+", choices=sorted(SIZES), default=[2, 4])
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out")
    a = p.parse_args()
    res = {"command": "python tools/state_roundtrip.py --configs " + " ".join(map(str, a.configs)) + f" --repeats {a.repeats}",
           "results": [measure(c, a.repeats) for c in a.configs]}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
