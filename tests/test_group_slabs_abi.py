"""CPU-side checks of the render group's photon partition (include/orx.h orx_group_config.photon_partition,
ORX_PHOTONS_SLABS): the ctypes mirror matches the C layout (compiled probe), the new argument checks happen
before the first HIP call (so they are testable without a device), the three new entry points are exported and
declared, and integration/standalone_group.cpp takes --photons rows|slabs."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from oppositerenderer_amd import _abi, renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oppositerenderer_amd", "standalone_group")
NEW_SYMBOLS = ("orx_slab_plan", "orx_group_slab_plan", "orx_group_debug_all_to_all")


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


def create(n, devices, cfg=None, **gcfg):
    lib = renderer.load_library()
    h = C.c_void_p(0xDEAD)
    devs = (C.c_int * len(devices))(*devices)
    c = _abi.default_config(photon_launch_width=16, photon_launch_height=16, seed=1, **(cfg or {}))
    gc = _abi.default_group_config(**gcfg)
    st = lib.orx_create_group(n, devs, C.byref(c), C.byref(gc), C.byref(h))
    return st, h


def test_group_config_layout_matches_c():
    probe = r"""
#include <stdio.h>
#include <stddef.h>
#include "orx.h"
int main(void){
 printf("%zu %zu %zu %zu %d %d\n", sizeof(orx_group_config), offsetof(orx_group_config, pipeline),
        offsetof(orx_group_config, photon_partition), offsetof(orx_group_config, reserved),
        (int)ORX_PHOTONS_ROWS, (int)ORX_PHOTONS_SLABS);
 return 0;}
"""
    d = tempfile.mkdtemp()
    c = os.path.join(d, "g.c")
    exe = os.path.join(d, "g")
    open(c, "w").write(probe)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    vals = [int(v) for v in subprocess.check_output([exe]).split()]
    G = _abi.OrxGroupConfig
    assert vals == [32, 12, 16, 20, 0, 1]
    assert vals == [C.sizeof(G), G.pipeline.offset, G.photon_partition.offset, G.reserved.offset, _abi.PHOTONS_ROWS,
                    _abi.PHOTONS_SLABS]


def test_default_photon_partition_is_rows():
    lib = renderer.load_library()
    c = _abi.OrxGroupConfig()
    C.memset(C.byref(c), 0xFF, C.sizeof(c))
    lib.orx_default_group_config(C.byref(c))
    assert c.photon_partition == _abi.PHOTONS_ROWS == 0
    assert bytes(c) == bytes(_abi.default_group_config())


@pytest.mark.parametrize("value", [2, 0xFFFFFFFF])
def test_create_rejects_unknown_photon_partition(value):
    st, h = create(2, [0, 0], partition=_abi.GROUP_ROWS, photon_partition=value)
    assert st == _abi.ORX_ERR_INVALID_ARGUMENT and not h.value
    assert renderer.load_library().orx_group_last_error(None)


@pytest.mark.parametrize("n", [1, 2])
def test_batch_with_slabs_is_invalid(n):
    st, h = create(n, [0] * n, partition=_abi.GROUP_BATCH, photon_partition=_abi.PHOTONS_SLABS)
    assert st == _abi.ORX_ERR_INVALID_ARGUMENT and not h.value


@pytest.mark.parametrize("photon_map", [1, 2])
def test_slabs_need_the_uniform_grid(photon_map):
    st, h = create(2, [0, 0], cfg={"photon_map": photon_map}, partition=_abi.GROUP_ROWS,
                   photon_partition=_abi.PHOTONS_SLABS)
    assert st == _abi.ORX_ERR_UNSUPPORTED and not h.value
    assert renderer.load_library().orx_group_last_error(None)


def test_valid_slabs_config_without_device_is_device_error():
    if has_gpu():
        pytest.skip("a GPU is present")
    for n in (1, 2, 8):
        st, h = create(n, [0] * n, partition=_abi.GROUP_ROWS, comm=_abi.COMM_LOCAL, photon_partition=_abi.PHOTONS_SLABS)
        assert st == _abi.ORX_ERR_DEVICE and not h.value


def test_new_symbols_registered():
    assert set(NEW_SYMBOLS) <= set(renderer.EXPORTED_SYMBOLS)
    lib = renderer.load_library()
    hdr = open(os.path.join(ROOT, "include", "orx.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and f"{s}(" in hdr, s


def test_null_group_calls_are_invalid():
    lib = renderer.load_library()
    axis = C.c_uint32()
    buf = (C.c_uint8 * 1024)()
    counts = (C.c_uint64 * 1)()
    f = (C.c_float * 9)()
    assert lib.orx_group_slab_plan(None, C.byref(axis), buf, counts) == _abi.ORX_ERR_INVALID_ARGUMENT
    assert lib.orx_group_debug_all_to_all(None, f, counts, f) == _abi.ORX_ERR_INVALID_ARGUMENT


def test_standalone_group_rejects_unknown_photons():
    r = subprocess.run([binary(), "--photons", "foo"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "error:" in r.stderr and "--photons" in r.stderr


def test_standalone_group_slabs_no_device_fails_cleanly():
    if has_gpu():
        pytest.skip("a GPU is present")
    r = subprocess.run([binary(), "--ranks", "2", "--partition", "rows", "--photons", "slabs", "--comm", "local",
                        "--out", os.devnull], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "error:" in r.stderr
