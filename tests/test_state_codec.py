"""The checkpoint blob's codec on the CPU (oppositerenderer_amd/csrc/orx_state.cpp; include/orx.h, "Checkpoint /
resume").  No device is needed: orx_state_info_read / _packed_bytes / _pack / _unpack and orx_scene_key are pure.

1. round trip through liborx.so for a 4x2 frame (rng 4x2) and a 5x3 frame with rng 7x4;
2. the packed 4x2 blob of fixed inputs equals tests/golden/state_v1_tiny.bin, which pins format version 1
   (the offsets documented in orx.h are checked against the same bytes);
3. every prefix, a wrong magic, version 2, a flipped byte in the header, in each section and in each checksum,
   sizes whose product overflows 64 bits and a total beyond `bytes` give ORX_ERR_INVALID_ARGUMENT;
4. tests/state_codec_check.cpp runs the same sweep and a mutation fuzz as a program of its own, built with
   orx_state.cpp alone under AddressSanitizer + UndefinedBehaviorSanitizer;
5. the scene key of a scene is the same from two separately built ABI copies and differs between scenes."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from oppositerenderer_amd import _abi, renderer, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oppositerenderer_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "state_v1_tiny.bin")
INVALID = _abi.ORX_ERR_INVALID_ARGUMENT


def fnv1a64(data: bytes) -> int:
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def make_info(W, H, RW, RH, **kw):
    info = _abi.OrxStateInfo()
    info.kind = _abi.STATE_KIND_FRAME
    info.flags = _abi.STATE_FLAG_VCM_ESTIMATED
    info.width, info.height, info.rng_width, info.rng_height = W, H, RW, RH
    info.photon_launch_width, info.photon_launch_height = RW, RH
    info.method = _abi.VCM_BIDIRECTIONAL_PATH_TRACING
    info.ppm_radius = 0.25
    info.iteration_number = 7
    info.local_iteration_number = 6
    info.scene_key = 0x1122334455667788
    for k, v in kw.items():
        setattr(info, k, v)
    return info


def pack(info, words, floats):
    lib = renderer.load_library()
    n = lib.orx_state_packed_bytes(C.byref(info))
    assert n == 128 + words.nbytes + floats.nbytes
    buf = C.create_string_buffer(n)
    assert lib.orx_state_pack(C.byref(info), words.ctypes.data, floats.ctypes.data, buf, n - 1) == INVALID
    assert lib.orx_state_pack(C.byref(info), words.ctypes.data, floats.ctypes.data, buf, n) == _abi.ORX_OK
    return buf.raw


def read(blob: bytes, nbytes=None):
    """(status, info) of orx_state_info_read on a buffer of exactly the bytes given"""
    lib = renderer.load_library()
    nbytes = len(blob) if nbytes is None else nbytes
    buf = (C.c_uint8 * max(nbytes, 1)).from_buffer_copy(blob[:nbytes] if nbytes else b"\0")
    info = _abi.OrxStateInfo()
    st = lib.orx_state_info_read(buf, nbytes, C.byref(info))
    rng, out = C.c_void_p(), C.c_void_p()
    assert lib.orx_state_unpack(buf, nbytes, C.byref(rng), C.byref(out)) == st
    return st, info


def tiny_blob():
    """the fixed 4x2 frame of the format pin"""
    words = (np.arange(4 * 2 * 6, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    floats = (np.arange(4 * 2 * 3, dtype=np.float32) * np.float32(0.375) - np.float32(2.0)).astype(np.float32)
    return pack(make_info(4, 2, 4, 2), words, floats), words, floats


def with_header_sum(blob: bytearray) -> bytes:
    blob[120:128] = struct.pack("<Q", fnv1a64(bytes(blob[:120])))
    return bytes(blob)


@pytest.mark.parametrize("W,H,RW,RH", [(4, 2, 4, 2), (5, 3, 7, 4)])
def test_round_trip(W, H, RW, RH):
    lib = renderer.load_library()
    rng = np.random.default_rng(W * 100 + H)
    words = rng.integers(0, 1 << 32, RW * RH * 6, dtype=np.uint64).astype(np.uint32)
    floats = rng.standard_normal(W * H * 3).astype(np.float32)
    floats[0] = np.float32("nan")  # words, not values: a NaN's bits survive
    info = make_info(W, H, RW, RH)
    blob = pack(info, words, floats)
    st, got = read(blob)
    assert st == _abi.ORX_OK
    for name, _ in _abi.OrxStateInfo._fields_:
        want = {"version": 1, "total_bytes": len(blob), "world": 0, "calls": 0}.get(name, getattr(info, name))
        assert getattr(got, name) == want, name
    assert renderer.state_info(blob).total_bytes == len(blob)
    buf = C.create_string_buffer(blob, len(blob))
    p_rng, p_out = C.c_void_p(), C.c_void_p()
    assert lib.orx_state_unpack(buf, len(blob), C.byref(p_rng), C.byref(p_out)) == _abi.ORX_OK
    base = C.addressof(buf)
    assert p_rng.value == base + 128 and p_out.value == base + 128 + words.nbytes
    assert blob[128:128 + words.nbytes] == words.tobytes()
    assert blob[128 + words.nbytes:] == floats.tobytes()


def test_format_version_1_is_pinned():
    blob, words, floats = tiny_blob()
    with open(GOLDEN, "rb") as f:
        golden = f.read()
    assert len(golden) == 128 + 4 * 2 * 24 + 4 * 2 * 12 == 416
    assert blob == golden
    # the offsets of include/orx.h, read off the same bytes
    assert golden[:8] == b"ORXSTATE"
    assert struct.unpack_from("<IIQII", golden, 8) == (1, 128, 416, 0, 1)
    assert struct.unpack_from("<6I", golden, 32) == (4, 2, 4, 2, 4, 2)
    assert struct.unpack_from("<ifQQQ", golden, 56) == (1, 0.25, 7, 6, 0x1122334455667788)
    assert struct.unpack_from("<IIQ", golden, 88) == (0, 0, 0)
    assert struct.unpack_from("<3Q", golden, 104) == (fnv1a64(words.tobytes()), fnv1a64(floats.tobytes()),
                                                      fnv1a64(golden[:120]))


def test_rejections():
    blob, words, floats = tiny_blob()
    assert read(blob)[0] == _abi.ORX_OK
    for n in range(len(blob)):  # every prefix
        assert read(blob, n)[0] == INVALID, n
    for at in range(len(blob)):  # header, RNG section, output section, the three checksums
        bad = bytearray(blob)
        bad[at] ^= 0x10
        assert read(bytes(bad))[0] == INVALID, at
    bad = bytearray(blob)
    bad[0:8] = b"ORXSTATS"
    assert read(with_header_sum(bad))[0] == INVALID
    bad = bytearray(blob)
    struct.pack_into("<I", bad, 8, 2)  # version 2
    assert read(with_header_sum(bad))[0] == INVALID
    bad = bytearray(blob)
    struct.pack_into("<Q", bad, 16, len(blob) + 1)  # a total beyond the bytes given
    assert read(with_header_sum(bad))[0] == INVALID
    for total in (len(blob), (1 << 64) - 1, 128):  # rng (2^32 - 1)^2 slots: times 24 overflows 64 bits
        bad = bytearray(blob)
        struct.pack_into("<II", bad, 40, 0xFFFFFFFF, 0xFFFFFFFF)
        struct.pack_into("<Q", bad, 16, total)
        assert read(with_header_sum(bad))[0] == INVALID
    bad = bytearray(blob)
    struct.pack_into("<4I", bad, 32, *([0xFFFFFFFF] * 4))
    assert read(with_header_sum(bad))[0] == INVALID
    with pytest.raises(renderer.OrxError) as e:
        renderer.state_info(blob[:-1])
    assert e.value.status == INVALID
    lib = renderer.load_library()
    huge = make_info(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert lib.orx_state_packed_bytes(C.byref(huge)) == 0
    assert lib.orx_state_packed_bytes(C.byref(make_info(4, 2, 3, 2))) == 0


def test_codec_under_sanitizers(tmp_path):
    exe = str(tmp_path / "state_codec_check")
    # the sanitizer runtimes are linked into the program, as tests/test_slab_plan.py does
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "state_codec_check.cpp"),
                           os.path.join(CSRC, "orx_state.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-4000:]
    assert "all checks passed" in run.stdout


def test_scene_key_depends_on_contents_only():
    lib = renderer.load_library()
    a, b = scenes.cornell().to_abi(), scenes.cornell().to_abi()  # two deep copies at other addresses
    ka, kb = lib.orx_scene_key(C.byref(a)), lib.orx_scene_key(C.byref(b))
    assert ka == kb and ka != 0
    small = scenes.cornell_small().to_abi()
    assert lib.orx_scene_key(C.byref(small)) != ka
    assert lib.orx_scene_key(None) == 0
