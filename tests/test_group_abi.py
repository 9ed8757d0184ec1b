"""CPU-side checks of the render-group API (include/orx.h, orx_create_group): the ctypes mirror of
orx_group_config matches the C layout (compiled probe), orx_batch_seed restates
multigpu.batch_seed, every argument check happens before the first HIP call (so it is testable
without a device), and integration/standalone_group.cpp builds against include/orx.h alone and
fails cleanly without a device."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from oppositerenderer_amd import _abi, multigpu, renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oppositerenderer_amd", "standalone_group")


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def binary():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "integration")])
    return BIN


def test_group_config_layout_matches_c():
    probe = r"""
#include <stdio.h>
#include <stddef.h>
#include "orx.h"
int main(void){
 orx_group_config c; orx_group_config* p = &c; (void)p;
 printf("%zu %zu %zu %zu %zu %zu %d %d %d %d %d\n", sizeof(orx_group_config), offsetof(orx_group_config, partition),
        offsetof(orx_group_config, comm), offsetof(orx_group_config, reduce_every), offsetof(orx_group_config, pipeline),
        offsetof(orx_group_config, reserved), (int)ORX_GROUP_BATCH, (int)ORX_GROUP_ROWS, (int)ORX_COMM_AUTO,
        (int)ORX_COMM_LOCAL, (int)ORX_COMM_RCCL);
 return 0;}
"""
    d = tempfile.mkdtemp()
    c = os.path.join(d, "g.c")
    exe = os.path.join(d, "g")
    open(c, "w").write(probe)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    vals = [int(v) for v in subprocess.check_output([exe]).split()]
    G = _abi.OrxGroupConfig
    py = [C.sizeof(G), G.partition.offset, G.comm.offset, G.reduce_every.offset, G.pipeline.offset, G.reserved.offset,
          _abi.GROUP_BATCH, _abi.GROUP_ROWS, _abi.COMM_AUTO, _abi.COMM_LOCAL, _abi.COMM_RCCL]
    assert vals == py


def test_default_group_config_matches_python():
    lib = renderer.load_library()
    c = _abi.OrxGroupConfig()
    C.memset(C.byref(c), 0xFF, C.sizeof(c))
    lib.orx_default_group_config(C.byref(c))
    d = _abi.default_group_config()
    assert bytes(c) == bytes(d)
    assert (c.partition, c.comm, c.reduce_every, c.pipeline) == (_abi.GROUP_BATCH, _abi.COMM_AUTO, 8, 1)


CLOCKS = (1_700_000_000_123_456_789, 0xFFFFFFFF_00000001)


@pytest.mark.parametrize("seed", [0, 1, 1645301512, 0xFFFFFFFF])
@pytest.mark.parametrize("rank", [0, 1, 2, 7, 63])
@pytest.mark.parametrize("clock", CLOCKS)
def test_batch_seed_matches_python(seed, rank, clock):
    lib = renderer.load_library()
    assert lib.orx_batch_seed(seed, rank, clock) == multigpu.batch_seed(seed, rank, clock)


@pytest.mark.parametrize("rank", [1, 7])
def test_batch_seed_never_zero(rank):
    """a seed (and, with seed 0, a clock) whose rank offset wraps to 0: both sides give 1"""
    lib = renderer.load_library()
    seed = (-0x9E3779B9 * rank) & 0xFFFFFFFF
    assert multigpu.batch_seed(seed, rank, 5) == 1  # the case exists
    assert lib.orx_batch_seed(seed, rank, 5) == 1
    clock = seed  # seed 0: t ^ (t >> 32) folds to the same value
    assert multigpu.batch_seed(0, rank, clock) == 1
    assert lib.orx_batch_seed(0, rank, clock) == 1


def create(n, devices, cfg=True, gcfg=None, out=True):
    lib = renderer.load_library()
    h = C.c_void_p(0xDEAD)
    devs = (C.c_int * max(1, len(devices)))(*devices) if devices is not None else None
    c = _abi.default_config(photon_launch_width=16, photon_launch_height=16, seed=1)
    if isinstance(cfg, dict):
        for k, v in cfg.items():
            setattr(c, k, v)
    st = lib.orx_create_group(n, devs, C.byref(c) if cfg else None, C.byref(gcfg) if gcfg is not None else None,
                              C.byref(h) if out else None)
    return st, h


@pytest.mark.parametrize("n,devices", [(0, []), (65, [0] * 65), (2, None), (1, [-1])])
def test_create_rejects_bad_counts_and_pointers(n, devices):
    st, h = create(n, devices)
    assert st == _abi.ORX_ERR_INVALID_ARGUMENT and not h.value
    assert renderer.load_library().orx_group_last_error(None)


def test_create_rejects_null_out():
    st, _ = create(1, [0], out=False)
    assert st == _abi.ORX_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("field,value", [("partition", 2), ("comm", 3), ("partition", 0xFFFFFFFF)])
def test_create_rejects_unknown_enums(field, value):
    st, h = create(2, [0, 0], gcfg=_abi.default_group_config(**{field: value}))
    assert st == _abi.ORX_ERR_INVALID_ARGUMENT and not h.value


def test_local_comm_needs_one_device():
    """decided before any HIP call: the same answer with and without a device"""
    st, h = create(2, [0, 1], gcfg=_abi.default_group_config(comm=_abi.COMM_LOCAL))
    assert st == _abi.ORX_ERR_UNSUPPORTED and not h.value
    assert b"one device" in renderer.load_library().orx_group_last_error(None)


@pytest.mark.parametrize("cfg", [{"photon_map": 1, "photon_launch_width": 16, "photon_launch_height": 16},
                                 {"enable_media": 1}])
def test_rows_rejects_single_device_features(cfg):
    st, h = create(2, [0, 0], cfg=cfg, gcfg=_abi.default_group_config(partition=_abi.GROUP_ROWS))
    assert st == _abi.ORX_ERR_UNSUPPORTED and not h.value


def test_null_group_calls_are_invalid():
    lib = renderer.load_library()
    req = _abi.OrxRequest()
    scene = _abi.OrxScene()
    assert lib.orx_group_init_scene(None, C.byref(scene)) == _abi.ORX_ERR_INVALID_ARGUMENT
    assert lib.orx_group_render_next_iteration(None, 0, 0, 1.0, 1, C.byref(req)) == _abi.ORX_ERR_INVALID_ARGUMENT
    buf = (C.c_float * 3)()
    assert lib.orx_group_get_output(None, buf, 12) == _abi.ORX_ERR_INVALID_ARGUMENT
    assert lib.orx_group_debug_reduce(None, buf, 3, buf) == _abi.ORX_ERR_INVALID_ARGUMENT
    assert lib.orx_group_debug_reduce_scatter(None, buf, 3, buf) == _abi.ORX_ERR_INVALID_ARGUMENT
    assert lib.orx_group_world(None) == 0 and not lib.orx_group_renderer(None, 0)
    assert lib.orx_group_pipelined(None) == 0
    lib.orx_group_destroy(None)


def test_no_gpu_create_group_fails_cleanly():
    if has_gpu():
        pytest.skip("a GPU is present")
    for part in (_abi.GROUP_BATCH, _abi.GROUP_ROWS):
        st, h = create(2, [0, 0], gcfg=_abi.default_group_config(partition=part))
        assert st == _abi.ORX_ERR_DEVICE and not h.value
    st, h = create(1, [0], cfg=None, gcfg=None)  # NULL configs: the defaults
    assert st == _abi.ORX_ERR_DEVICE and not h.value


def test_python_group_raises_without_device():
    if has_gpu():
        pytest.skip("a GPU is present")
    from oppositerenderer_amd.group import OptixRendererGroup
    g = OptixRendererGroup(_abi.default_config(), _abi.default_group_config(partition=_abi.GROUP_ROWS))
    with pytest.raises(renderer.OrxError) as e:
        g.initialize([0, 0])
    assert e.value.status == _abi.ORX_ERR_DEVICE


def test_group_symbols_registered():
    names = {"orx_default_group_config", "orx_create_group", "orx_group_init_scene", "orx_group_render_next_iteration",
             "orx_group_get_output", "orx_group_world", "orx_group_renderer", "orx_group_pipelined",
             "orx_group_comm_name", "orx_group_last_error", "orx_group_destroy", "orx_batch_seed",
             "orx_group_debug_reduce_scatter", "orx_group_debug_reduce"}
    assert names <= set(renderer.EXPORTED_SYMBOLS)
    lib = renderer.load_library()
    hdr = open(os.path.join(ROOT, "include", "orx.h")).read()
    for s in names:
        assert hasattr(lib, s) and f"{s}(" in hdr, s


def test_liborx_does_not_link_rccl():
    out = subprocess.run(["readelf", "-d", renderer.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in out and "rccl" not in out.lower() and "nccl" not in out.lower()


def test_standalone_group_links_only_declared_symbols():
    nm = subprocess.run(["nm", "-D", "--undefined-only", binary()], capture_output=True, text=True, check=True)
    used = sorted({l.split()[-1] for l in nm.stdout.splitlines() if l.split()[-1].startswith("orx_")})
    hdr = open(os.path.join(ROOT, "include", "orx.h")).read()
    assert "orx_create_group" in used and "orx_group_get_output" in used
    assert all(f"{s}(" in hdr for s in used), used


def test_standalone_group_no_device_fails_cleanly():
    if has_gpu():
        pytest.skip("a GPU is present")
    r = subprocess.run([binary(), "--ranks", "2", "--partition", "rows", "--comm", "local", "--out", os.devnull],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "error:" in r.stderr


def test_standalone_group_rejects_bad_arguments():
    """argument errors need no device: LOCAL over two devices"""
    r = subprocess.run([binary(), "--ranks", "2", "--devices", "0,1", "--comm", "local"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1 and "error:" in r.stderr and "one device" in r.stderr
