"""Convergence estimate and display resolve, the parts that need no GPU: the float32 restatement of the
statistics (tests/convergence_ref.py) against float64, the ABI of the new calls, their argument checks
without a device, orx_display_convert against a host probe built from include/orx_display.h and against
numpy.power, and the host code under the sanitizers as a program of its own (tests/post_host_check.cpp)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import convergence_ref as cref
from oppositerenderer_amd import _abi, renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oppositerenderer_amd", "csrc")
f32 = np.float32
INVALID, STATE = _abi.ORX_ERR_INVALID_ARGUMENT, _abi.ORX_ERR_STATE


# ---- the restatement against float64 ----

def synthetic_sums(n, sigma, seed, npx=4096):
    """n running sums of npx pixels: a per-pixel colour times a lognormal(0, sigma) factor per iteration and
    a per-channel jitter; a quarter of the pixels receive zero every third iteration; accumulated in float32"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.05, 2.0, (npx, 3))
    S = np.zeros((npx, 3), f32)
    sums = []
    for i in range(n):
        v = (base * rng.lognormal(0.0, sigma, (npx, 1)) * rng.uniform(0.8, 1.25, (npx, 3))).astype(f32)
        if i % 3 == 2:
            v[:npx // 4] = 0
        S = (S + v).astype(f32)
        sums.append(S.copy())
    return sums


@pytest.mark.parametrize("sigma", [0.01, 0.5, 2.0])
@pytest.mark.parametrize("n", [2, 6, 8, 64, 1000])
def test_restatement_against_float64(n, sigma):
    """|M2_32 - M2_64| <= 1e-3 (M2_64 + (n mean)^2 2^-23) and |A_32 - A_64| <= 1e-5 A_64 against a float64
    two-pass variance of the same fp32 sums.  Observed with this generator: at most 2.2e-4 for M2 (n = 2,
    sigma 0.01) and 2.1e-6 for A (n = 1000): the bounds are about 5x over those."""
    sums = synthetic_sums(n, sigma, n * 10 + int(sigma * 100))
    prev, A, M2 = cref.window(sums)
    assert prev.tobytes() == sums[-1].tobytes()
    S64 = np.array(sums, np.float64)
    d = np.diff(np.concatenate([np.zeros((1,) + S64.shape[1:]), S64]), axis=0)
    y = 0.2126 * d[..., 0] + 0.7152 * d[..., 1] + 0.0722 * d[..., 2]
    A64, mean = y.sum(0), y.mean(0)
    M64 = ((y - mean) ** 2).sum(0)
    rm = np.abs(M2 - M64) / (M64 + (n * mean) ** 2 * 2.0 ** -23)
    ra = np.abs(A - A64) / A64
    print(f"n {n} sigma {sigma}: M2 {rm.max():.3e} A {ra.max():.3e}")
    assert rm.max() <= 1e-3
    assert ra.max() <= 1e-5
    # a window on a base: the same statistics of the later iterations alone
    if n >= 6:
        p2, A2, M22 = cref.window(sums[3:], base=sums[2])
        y2 = y[3:]
        assert np.abs(A2 - y2.sum(0)).max() <= 1e-5 * np.abs(y2.sum(0)).max() + 1e-5 * S64[-1].max()
        assert p2.tobytes() == sums[-1].tobytes()


def test_error_plane_and_tiles_by_hand():
    A = np.array([6.0, 0.0, 3.0], f32)
    M2 = np.array([6.0, 0.0, 0.0], f32)
    e, m = cref.error_plane(A, M2, 3, 0.5)
    assert m.tolist() == [2.0, 0.0, 1.0]
    assert e[0] == f32(np.sqrt(f32(1.0))) / f32(2.0) and e[1] == 0.0 and e[2] == 0.0
    e, m = cref.error_plane(np.full(37 * 21, 2.0, f32), np.full(37 * 21, 8.0, f32), 2, 1e-3)
    t = cref.tile_stats(e, m, 37, 21, 0.5)
    assert (t["tiles_x"], t["tiles_y"]) == (3, 2) and np.allclose(t["tiles"], 2.0) and t["pixels_above"] == 37 * 21
    assert t["mean_luminance"] == 1.0


# ---- ABI ----

def test_struct_layout_and_enums_match_c():
    probe = r"""
#include <stdio.h>
#include <stddef.h>
#include "orx.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu ", sizeof(orx_convergence), offsetof(orx_convergence, iterations),
        offsetof(orx_convergence, tiles_x), offsetof(orx_convergence, tiles_y), offsetof(orx_convergence, pixels_above),
        offsetof(orx_convergence, max_tile), offsetof(orx_convergence, mean_error),
        offsetof(orx_convergence, max_tile_error), offsetof(orx_convergence, mean_luminance),
        offsetof(orx_convergence, reserved));
 printf("%d %d %d %d %d %d %d %d %zu %zu %u\n", (int)ORX_BUF_CONV_PREV, (int)ORX_BUF_CONV_SUM, (int)ORX_BUF_CONV_M2,
        (int)ORX_BUF_CONV_ERROR, (int)ORX_PASS_CONVERGENCE, (int)ORX_PASS_COUNT, (int)ORX_DISPLAY_RGBA8,
        (int)ORX_DISPLAY_BGRA8, sizeof(orx_config), sizeof(orx_stats), (unsigned)ORX_ABI_VERSION);
 return 0;}
"""
    d = tempfile.mkdtemp()
    src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
    open(src, "w").write(probe)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    vals = [int(v) for v in subprocess.check_output([exe]).split()]
    K = _abi.OrxConvergence
    assert vals[0] == C.sizeof(K) == 44
    assert vals[1:10] == [K.iterations.offset, K.tiles_x.offset, K.tiles_y.offset, K.pixels_above.offset,
                          K.max_tile.offset, K.mean_error.offset, K.max_tile_error.offset, K.mean_luminance.offset,
                          K.reserved.offset] == [0, 4, 8, 12, 16, 20, 24, 28, 32]
    assert vals[10:14] == [_abi.BUF_CONV_PREV, _abi.BUF_CONV_SUM, _abi.BUF_CONV_M2, _abi.BUF_CONV_ERROR] == [21, 22, 23, 24]
    assert vals[14] == _abi.PASS_CONVERGENCE == 13 and vals[15] == 14
    assert vals[16:18] == [_abi.DISPLAY_RGBA8, _abi.DISPLAY_BGRA8] == [0, 1]
    assert vals[18] == 64 and vals[19] == C.sizeof(_abi.OrxStats) and vals[20] == 1
    assert len(_abi.PASS_NAMES) == 11 and _abi.PASS_CONVERGENCE < len(_abi.OrxStats().pass_ms)


NEW_SYMBOLS = ("orx_set_convergence", "orx_get_convergence", "orx_display_convert", "orx_get_display",
               "orx_group_set_convergence", "orx_group_get_convergence", "orx_group_get_display")


def test_new_symbols_exported():
    lib = renderer.load_library()
    for name in NEW_SYMBOLS:
        assert name in renderer.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None


def test_null_and_bad_arguments_without_a_device():
    lib = renderer.load_library()
    out = _abi.OrxConvergence()
    px = (C.c_uint8 * 16)()
    for prefix in ("orx", "orx_group"):
        assert getattr(lib, prefix + "_set_convergence")(None, 1) == INVALID
        assert getattr(lib, prefix + "_get_convergence")(None, 1e-3, 0.1, C.byref(out), None, 0) == INVALID
        assert getattr(lib, prefix + "_get_display")(None, 1.0, 1.0, 0, px, 16) == INVALID
    one = (C.c_float * 3)(1, 1, 1)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.orx_display_convert(one, 1, bad, 1.0, 0, px) == INVALID
        assert lib.orx_display_convert(one, 1, 1.0, bad, 0, px) == INVALID
    for fmt in (-1, 2, 7):
        assert lib.orx_display_convert(one, 1, 1.0, 1.0, fmt, px) == INVALID
    assert lib.orx_display_convert(None, 1, 1.0, 1.0, 0, px) == INVALID
    assert lib.orx_display_convert(one, 1, 1.0, 1.0, 0, None) == INVALID
    assert lib.orx_display_convert(one, 1, 1.0, 1.0, 1, px) == _abi.ORX_OK
    with pytest.raises(renderer.OrxError) as e:
        renderer.display_convert(np.ones((2, 3), f32), 0.0)
    assert e.value.status == INVALID


# ---- orx_display_convert ----

PROBE = r"""
#include "orx_display.h"
void probe(const float* c, int n, float inv_it, float inv_gamma, unsigned char* out) {
    for (int i = 0; i < n; i++) out[i] = (unsigned char)orx_display_byte(c[i], inv_it, inv_gamma);
}
void probe_g(const float* c, int n, float inv_it, float inv_gamma, float* g) {
    for (int i = 0; i < n; i++) g[i] = orx_powf(c[i] * inv_it, inv_gamma) * 255.0f;
}
"""


@pytest.fixture(scope="module")
def probe():
    d = tempfile.mkdtemp()
    c, so = os.path.join(d, "probe.c"), os.path.join(d, "libprobe.so")
    open(c, "w").write(PROBE)
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           c, "-o", so, "-lm"])
    lib = C.CDLL(so)
    for f in (lib.probe, lib.probe_g):
        f.argtypes, f.restype = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p], None
    return lib


def display_values(probe):
    rng = np.random.default_rng(20261021)
    vals = rng.uniform(0.0, 4.0, 100_000).astype(f32)
    special = np.array([0.0, -1.0, np.nan, np.inf, 1e-30, 1.0, -np.inf, -0.0, 4.0], f32)
    # values whose g = pow(v, 1/2.2) * 255 lies within 1e-4 of an integer: start at (k / 255)^2.2 and walk the
    # neighbouring floats
    k = np.arange(1, 256, dtype=np.float64)
    near = np.power(k / 255.0, 2.2).astype(f32)
    cand = np.concatenate([np.nextafter(near, f32(0)), near, np.nextafter(near, f32(8))])
    g = np.empty(cand.size, f32)
    probe.probe_g(cand.ctypes.data, cand.size, C.c_float(1.0), C.c_float(1.0 / 2.2), g.ctypes.data)
    close = cand[np.abs(g - np.rint(g)) < 1e-4]
    assert close.size >= 100
    vals = np.concatenate([special, close, vals])
    pad = (-vals.size) % 3
    return np.concatenate([vals, np.zeros(pad, f32)]).reshape(-1, 3)


@pytest.mark.parametrize("inv_it,inv_gamma", [(1.0, 1.0 / 2.2), (1.0 / 7.0, 1.0 / 2.2), (0.5, 1.0)])
def test_display_convert_matches_probe_and_numpy(probe, inv_it, inv_gamma):
    src = display_values(probe)
    if inv_it != 1.0:  # keep the near-integer values near-integer after the division
        src = (src / f32(inv_it)).astype(f32)
    want = np.empty(src.size, np.uint8)
    probe.probe(src.ctypes.data, src.size, C.c_float(inv_it), C.c_float(inv_gamma), want.ctypes.data)
    want = want.reshape(-1, 3)
    rgba = renderer.display_convert(src, inv_it, inv_gamma, _abi.DISPLAY_RGBA8)
    bgra = renderer.display_convert(src, inv_it, inv_gamma, _abi.DISPLAY_BGRA8)
    assert rgba.shape == bgra.shape == (src.shape[0], 4) and rgba.dtype == np.uint8
    assert (rgba[:, 3] == 255).all() and (bgra[:, 3] == 255).all()
    assert np.array_equal(rgba[:, :3], want)                       # bytes equal, R G B A
    assert np.array_equal(bgra[:, :3], want[:, ::-1])              # B G R A
    ref = cref.display_bytes64(src, inv_it, inv_gamma)
    assert np.abs(rgba[:, :3].astype(np.int32) - ref.astype(np.int32)).max() <= 1
    # the special values at the front: 0, -1, NaN | inf, 1e-30, 1 | -inf, -0, 4
    if inv_it == 1.0:
        assert rgba[0, :3].tolist() == [0, 0, 0]
        assert rgba[1, 0] == 255 and rgba[1, 1] == 0 and rgba[1, 2] == 255
        assert rgba[2, :3].tolist() == [0, 0, 255]


def test_display_convert_shapes():
    img = np.linspace(0, 2, 5 * 7 * 3, dtype=f32).reshape(5, 7, 3)
    out = renderer.display_convert(img, 1.0)
    assert out.shape == (5, 7, 4)
    assert renderer.display_convert(np.zeros((0, 3), f32), 1.0).shape == (0, 4)


# ---- the host code under the sanitizers, as a program of its own ----

def test_post_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "post_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "post_host_check.cpp"),
                           os.path.join(CSRC, "orx_post_host.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-4000:]
    assert "all checks passed" in run.stdout
