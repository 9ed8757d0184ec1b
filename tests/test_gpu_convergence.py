"""Convergence statistics, the estimate and the display resolve on the device (include/orx.h
orx_set_convergence / orx_get_convergence / orx_get_display, csrc/orx_post.hip) (TEST: GPU).

Cornell small, seed 1645301512, photon launch 64x64, image 37x21: 3x2 tiles partial in both axes, 777 pixels
= 12 waves and a partial one, 194 four-pixel groups and a ragged pixel.  Six iterations, the running sum read
after each; tests/convergence_ref.py restates the statistics in float32 from those sums, and the device's
planes must equal it bit for bit (a NaN, which only a negative M2 could produce, equal to any NaN)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import convergence_ref as cref
from oppositerenderer_amd import _abi, multigpu, scenes
from oppositerenderer_amd.group import OptixRendererGroup
from oppositerenderer_amd.renderer import OptixRenderer, OrxError, RenderRequestDetails, display_convert

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1645301512
W, H, P, N = 37, 21, 64, 6
FLOOR = 1e-3
METHODS = {"ppm": _abi.PROGRESSIVE_PHOTON_MAPPING, "vcm": _abi.VCM_BIDIRECTIONAL_PATH_TRACING, "pt": _abi.PATH_TRACING}
# case -> (method, set_iteration_pipelining, vcm_merging)
CASES = {"pt": ("pt", -1, 0), "ppm_serial": ("ppm", 0, 0), "ppm_pipelined": ("ppm", 1, 0),
         "vcm_overlapped": ("vcm", 1, 0), "vcm_merging": ("vcm", 1, 1)}
PLANES = (_abi.BUF_CONV_PREV, _abi.BUF_CONV_SUM, _abi.BUF_CONV_M2)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def request(scene, method, w=W, h=H):
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(w) / np.float32(h)))
    return RenderRequestDetails(cam, scene.name, METHODS[method], w, h)


def config(**kw):
    return _abi.default_config(seed=SEED, photon_launch_width=P, photon_launch_height=P, **kw)


def make(case, scene, convergence=True):
    method, pipe, merging = CASES[case]
    r = OptixRenderer(config(vcm_merging=merging))
    r.initialize(0)
    r.initScene(scene)
    r.set_iteration_pipelining(pipe)
    if convergence:
        r.setConvergence(True)
    return r


def iterate(r, scene, det, its, read=True):
    """its: (iteration, local iteration) pairs; the radius follows the iteration number.  Returns the running
    sums read after each (read=False: none is read, nothing drains the pipeline)."""
    radii = multigpu.radius_sequence(scene.initial_ppm_radius(), max(i for i, _ in its) + 1)
    sums = []
    for i, local in its:
        r.renderNextIteration(i, local, radii[i], True, det)
        if read:
            sums.append(r.getOutputBuffer().copy())
    return sums


def planes(r):
    return [r.read_buffer(b).copy() for b in PLANES]


def check_planes(got, sums, base=None, rows=None):
    want = cref.window(sums, base)
    for name, g, w in zip(("prev", "A", "M2"), got, want):
        w = w.reshape(H if rows is None else -1, W, -1)
        assert same_bits(g, w), f"{name}: {int((g.ravel().view(np.uint32) != w.ravel().view(np.uint32)).sum())} words differ"
    return want


@functools.lru_cache(maxsize=None)
def straight(case):
    """six iterations of a case with the sum read after each, then one query at the restated plane's median"""
    scene = scenes.cornell_small()
    r = make(case, scene)
    det = request(scene, CASES[case][0])
    sums = iterate(r, scene, det, [(i, i) for i in range(N)])
    out = {"sums": sums, "pipelined": r.pipelined(), "planes": planes(r)}
    _, A, M2 = cref.window(sums)
    e, m = cref.error_plane(A, M2, N, FLOOR)
    out["e"], out["m"] = e, m
    out["threshold"] = float(np.median(e[np.isfinite(e)]))
    out["conv"], out["tiles"] = r.getConvergence(FLOOR, out["threshold"], tiles=True)
    out["error"] = r.read_buffer(_abi.BUF_CONV_ERROR).copy()
    out["pass_ms"] = r.stats().pass_ms[_abi.PASS_CONVERGENCE]
    r.destroy()
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_planes_bit_for_bit(case):
    s = straight(case)
    assert s["pipelined"] == (case in ("ppm_pipelined", "vcm_overlapped"))
    assert all(np.isfinite(x).all() for x in s["sums"]) and s["sums"][-1].mean() > 0
    check_planes(s["planes"], s["sums"])
    assert s["planes"][2].max() > 0  # the iterations differ: there is a variance to estimate
    print(f"{case}: NaN in e {int(np.isnan(s['e']).sum())}, threshold {s['threshold']:.4g}, pass_ms {s['pass_ms']:.4f}")
    assert same_bits(s["error"], s["e"])
    assert s["conv"].iterations == N
    assert s["conv"].pixels_above == int((s["e"] > np.float32(s["threshold"])).sum())
    assert 0.3 * W * H < s["conv"].pixels_above < 0.7 * W * H
    assert s["pass_ms"] > 0


def test_undrained_pipeline():
    """the same render without the per-iteration reads: only the last read drains, so the update is ordered by
    the streams and not by the test's reads"""
    scene = scenes.cornell_small()
    r = make("ppm_pipelined", scene)
    iterate(r, scene, request(scene, "ppm"), [(i, i) for i in range(N)], read=False)
    assert r.pipelined()
    got = planes(r)
    want = straight("ppm_pipelined")
    for g, w in zip(got, want["planes"]):
        assert same_bits(g, w)
    check_planes(got, want["sums"])
    r.destroy()


@pytest.mark.parametrize("case", ["ppm_pipelined", "pt"])
def test_tile_map_and_frame_numbers(case):
    """against float64 NumPy over the restated error plane at relative 3e-5: a 256-term sum of non-negative
    fp32 terms in any order is off by at most 255 * 2^-24 = 1.5e-5, the divide adds one rounding, and the
    frame means are finished in double"""
    check_estimate(straight(case)["conv"], straight(case)["tiles"], straight(case)["e"], straight(case)["m"], W, H,
                   straight(case)["threshold"])


def check_estimate(conv, tiles, e, m, w, h, threshold):
    TOL = 3e-5
    ref = cref.tile_stats(e, m, w, h, threshold)
    assert (conv.tiles_x, conv.tiles_y) == (ref["tiles_x"], ref["tiles_y"]) == (-(-w // 16), -(-h // 16))
    assert tiles.shape == ref["tiles"].shape
    assert np.isfinite(ref["tiles"]).all()
    assert np.abs(tiles - ref["tiles"]).max() <= TOL * ref["tiles"].max()
    assert (np.abs(tiles - ref["tiles"]) <= TOL * ref["tiles"]).all()
    assert abs(conv.mean_error - ref["mean_error"]) <= TOL * ref["mean_error"]
    assert abs(conv.mean_luminance - ref["mean_luminance"]) <= TOL * ref["mean_luminance"]
    assert abs(conv.max_tile_error - ref["max_tile_error"]) <= TOL * ref["max_tile_error"]
    assert conv.pixels_above == ref["pixels_above"]
    order = np.sort(ref["tiles"].ravel())
    if order.size < 2 or order[-1] - order[-2] > TOL * order[-1]:
        assert conv.max_tile == ref["max_tile"]
    else:  # the two largest tiles within the tolerance: either
        assert conv.max_tile in np.argsort(ref["tiles"].ravel())[-2:]
    assert conv.mean_error > 0 and conv.mean_luminance > 0


# ---- window restarts ----

def test_restart_at_local_iteration_zero():
    scene = scenes.cornell_small()
    r = make("ppm_pipelined", scene)
    sums = iterate(r, scene, request(scene, "ppm"), [(0, 0), (1, 1), (2, 2), (3, 0), (4, 1), (5, 2)])
    check_planes(planes(r), sums[3:])
    assert r.getConvergence(FLOOR, 0.1).iterations == 3
    r.destroy()


def test_restart_at_resize():
    scene = scenes.cornell_small()
    r = make("ppm_pipelined", scene)
    det = request(scene, "ppm")
    iterate(r, scene, det, [(0, 0), (1, 1), (2, 2)])
    small = iterate(r, scene, request(scene, "ppm", 16, 16), [(3, 3)])
    assert r.read_buffer(_abi.BUF_CONV_SUM).size == 256 and small[0].shape == (16, 16, 3)
    with pytest.raises(OrxError) as e:  # one iteration in the window
        r.getConvergence(FLOOR, 0.1)
    assert e.value.status == _abi.ORX_ERR_STATE
    sums = iterate(r, scene, det, [(4, 4), (5, 5), (6, 6)])  # the resize cleared the sum
    check_planes(planes(r), sums)
    r.destroy()


def test_restart_when_switched_off_and_on():
    scene = scenes.cornell_small()
    r = make("ppm_pipelined", scene)
    det = request(scene, "ppm")
    first = iterate(r, scene, det, [(0, 0), (1, 1), (2, 2)])
    r.setConvergence(False)
    with pytest.raises(OrxError) as e:
        r.read_buffer(_abi.BUF_CONV_SUM)
    assert e.value.status == _abi.ORX_ERR_STATE
    r.setConvergence(True)
    sums = iterate(r, scene, det, [(3, 3), (4, 4), (5, 5)])
    assert same_bits(sums[-1], straight("ppm_pipelined")["sums"][-1])  # the render itself went on undisturbed
    check_planes(planes(r), sums, base=first[-1])
    assert r.getConvergence(FLOOR, 0.1).iterations == 3
    r.destroy()


def test_restart_at_restore():
    scene = scenes.cornell_small()
    det = request(scene, "ppm")
    a = make("ppm_pipelined", scene)
    first = iterate(a, scene, det, [(0, 0), (1, 1), (2, 2)])
    blob = a.saveState()
    a.destroy()
    b = make("ppm_pipelined", scene)  # statistics on before the restore
    b.restoreState(blob)
    assert same_bits(b.read_buffer(_abi.BUF_CONV_PREV), first[-1])
    sums = iterate(b, scene, det, [(3, 3), (4, 4), (5, 5)])
    check_planes(planes(b), sums, base=first[-1])
    b.destroy()


# ---- off is off ----

def test_off_is_off():
    scene = scenes.cornell_small()
    r = make("ppm_pipelined", scene, convergence=False)
    iterate(r, scene, request(scene, "ppm"), [(i, i) for i in range(N)], read=False)
    for b in PLANES + (_abi.BUF_CONV_ERROR,):
        with pytest.raises(OrxError) as e:
            r.read_buffer(b)
        assert e.value.status == _abi.ORX_ERR_STATE
    with pytest.raises(OrxError) as e:
        r.getConvergence(FLOOR, 0.1)
    assert e.value.status == _abi.ORX_ERR_STATE
    assert r.stats().pass_ms[_abi.PASS_CONVERGENCE] == 0
    off = r.getOutputBuffer().copy()
    r.destroy()
    assert off.tobytes() == straight("ppm_pipelined")["sums"][-1].tobytes()  # byte-equal with the feature on


def test_query_argument_checks():
    scene = scenes.cornell_small()
    r = make("pt", scene)
    with pytest.raises(OrxError) as e:  # before the first frame
        r.getDisplayBuffer(1.0)
    assert e.value.status == _abi.ORX_ERR_STATE
    iterate(r, scene, request(scene, "pt"), [(0, 0), (1, 1)], read=False)
    for floor, thr in ((0.0, 0.1), (-1.0, 0.1), (float("inf"), 0.1), (float("nan"), 0.1), (1e-3, float("nan"))):
        with pytest.raises(OrxError) as e:
            r.getConvergence(floor, thr)
        assert e.value.status == _abi.ORX_ERR_INVALID_ARGUMENT
    out = _abi.OrxConvergence()
    small = np.empty(5, np.float32)  # 6 tiles
    assert r._lib.orx_get_convergence(r._h, 1e-3, 0.1, out, small.ctypes.data, small.nbytes) == _abi.ORX_ERR_INVALID_ARGUMENT
    assert r._lib.orx_get_convergence(r._h, 1e-3, 0.1, None, None, 0) == _abi.ORX_ERR_INVALID_ARGUMENT
    for args in ((0.0, 1.0, 0), (1.0, float("nan"), 0), (1.0, 1.0, 2)):
        with pytest.raises(OrxError) as e:
            r.getDisplayBuffer(*args)
        assert e.value.status == _abi.ORX_ERR_INVALID_ARGUMENT
    r.destroy()


# ---- display ----

@pytest.mark.parametrize("w,h", [(W, H), (1, 1)])
def test_display_equals_host_convert(w, h):
    scene = scenes.cornell_small()
    r = make("ppm_pipelined", scene, convergence=False)
    iterate(r, scene, request(scene, "ppm", w, h), [(0, 0), (1, 1), (2, 2)], read=False)
    out = r.getOutputBuffer().copy()
    for fmt in (_abi.DISPLAY_RGBA8, _abi.DISPLAY_BGRA8):
        got = r.getDisplayBuffer(1.0 / 3.0, 1.0 / 2.2, fmt)
        want = display_convert(out, 1.0 / 3.0, 1.0 / 2.2, fmt)
        assert got.shape == (h, w, 4) and got.tobytes() == want.tobytes()
    assert (want[..., 3] == 255).all() and (w == 1 or 0 < want[..., :3].mean() < 255)
    r.destroy()


# ---- ROWS group ----

def make_group(world, partition, scene, pipeline=1):
    g = OptixRendererGroup(config(), _abi.default_group_config(partition=partition, comm=_abi.COMM_LOCAL, pipeline=pipeline))
    g.initialize([0] * world)
    g.initScene(scene)
    return g


@pytest.mark.parametrize("method", ["ppm", "pt"])
def test_rows_group(method):
    """world 3, image 37x22: local rows 8, 7, 7"""
    world, h = 3, 22
    scene = scenes.cornell_small()
    g = make_group(world, _abi.GROUP_ROWS, scene)
    g.setConvergence(True)
    det = request(scene, method, W, h)
    radii = multigpu.radius_sequence(scene.initial_ppm_radius(), N)
    sums = []
    for i in range(N):
        g.renderNextIteration(i, i, radii[i], True, det)
        sums.append(g.getOutputBuffer().copy())
    assert g.pipelined() == (method == "ppm")
    prev, A, M2 = cref.window(sums)
    prev, A, M2 = prev.reshape(h, W, 3), A.reshape(h, W), M2.reshape(h, W)
    for k in range(world):
        r = g.renderer(k)
        got = [r.read_buffer(b) for b in PLANES]
        assert got[1].size == len(range(k, h, world)) * W
        for name, gk, wk in zip(("prev", "A", "M2"), got, (prev[k::world], A[k::world], M2[k::world])):
            assert same_bits(gk, wk), (k, name)
        with pytest.raises(OrxError) as e:  # a shard holds part of a frame: the group answers
            r.getConvergence(FLOOR, 0.1)
        assert e.value.status == _abi.ORX_ERR_STATE
    e, m = cref.error_plane(A.ravel(), M2.ravel(), N, FLOOR)
    threshold = float(np.median(e[np.isfinite(e)]))
    conv, tiles = g.getConvergence(FLOOR, threshold, tiles=True)
    assert conv.iterations == N
    check_estimate(conv, tiles, e, m, W, h, threshold)
    # the display image of the merged frame
    for fmt in (_abi.DISPLAY_RGBA8, _abi.DISPLAY_BGRA8):
        got = g.getDisplayBuffer(1.0 / N, 1.0 / 2.2, fmt)
        assert got.tobytes() == display_convert(sums[-1], 1.0 / N, 1.0 / 2.2, fmt).tobytes()
    g.destroy()


def test_batch_group_has_display_but_no_statistics():
    scene = scenes.cornell_small()
    g = make_group(2, _abi.GROUP_BATCH, scene)
    with pytest.raises(OrxError) as e:
        g.setConvergence(True)
    assert e.value.status == _abi.ORX_ERR_UNSUPPORTED
    det = request(scene, "pt")
    for i in range(4):
        g.renderNextIteration(i, i, 1.0, True, det)
    out = g.getOutputBuffer().copy()
    assert g.getDisplayBuffer(0.25).tobytes() == display_convert(out, 0.25).tobytes()
    with pytest.raises(OrxError) as e:
        g.getConvergence(FLOOR, 0.1)
    assert e.value.status == _abi.ORX_ERR_STATE
    g.destroy()


# ---- the stand-alone hosts ----

def run_bin(name, *args):
    exe = os.path.join(ROOT, "oppositerenderer_amd", name)
    return subprocess.run([exe, *args], check=True, stdout=subprocess.PIPE, text=True, timeout=120).stdout


def test_standalone_until_error_and_display(tmp_path):
    common = ["--method", "pt", "--width", "32", "--height", "32", "--iterations", "12"]
    out = run_bin("standalone_cornell", *common, "--until-error", "1e9")
    assert "iterations 2 mean_error" in out
    raw, disp = str(tmp_path / "o.f32"), str(tmp_path / "o.bgra")
    out = run_bin("standalone_cornell", *common, "--until-error", "0", "--out", raw, "--display", disp)
    assert "iterations 12 mean_error" in out
    img = np.fromfile(raw, np.float32).reshape(32, 32, 3)
    px = np.fromfile(disp, np.uint8)
    assert px.size == 32 * 32 * 4
    assert px.tobytes() == display_convert(img, np.float32(1.0) / np.float32(12), np.float32(1.0) / np.float32(2.2),
                                           _abi.DISPLAY_BGRA8).tobytes()
    out = run_bin("standalone_group", "--ranks", "3", "--partition", "rows", "--comm", "local", *common,
                  "--until-error", "1e9", "--display", disp)
    assert "iterations 2 mean_error" in out and np.fromfile(disp, np.uint8).size == 32 * 32 * 4
