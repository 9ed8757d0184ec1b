"""Vertex merging on the device (orx_config.vcm_merging, csrc/orx_vcm_merge.hip) against the NumPy
brute force of tests/vcm_merge_ref.py, which reads the device's own light- and camera-vertex buffers.

Bars: the accepted-pair count per pixel is exact (the accept test is restated in float32); the merging
colour is within rel-L2 1e-5 of the float64 brute force, the project's bar for summed estimates
(fp32 summation order only)."""
import ctypes as C

import numpy as np
import pytest

import vcm_merge_ref
from oppositerenderer_amd import _abi, scenes
from oppositerenderer_amd.group import OptixRendererGroup
from oppositerenderer_amd.renderer import OptixRenderer, OrxError, RenderRequestDetails, load_library, next_ppm_radius

pytestmark = pytest.mark.gpu
SEED = 1645301512
VCM = _abi.VCM_BIDIRECTIONAL_PATH_TRACING


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b * b).sum(), 1e-300)))


def cornell_glossy_floor():
    sc = scenes.cornell()
    sc.name = "CornellGlossyFloor"
    sc.quad_mat[0] = sc.add_material(scenes.Glossy((0.5, 0.5, 0.5), (0.3, 0.3, 0.3), 20.0))
    return sc


SCENES = {"Cornell": scenes.cornell, "CornellGlossyFloor": cornell_glossy_floor,
          "CornellSmall": lambda: scenes.scene_by_name("CornellSmall")}


def make(scene, merging=1, seed=SEED, **cfg):
    gpu = OptixRenderer(_abi.default_config(seed=seed, photon_launch_width=32, photon_launch_height=32,
                                            vcm_merging=merging, **cfg))
    gpu.initialize(0)
    gpu.initScene(scene)
    return gpu


def request(scene, method, W, H):
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
    return RenderRequestDetails(cam, scene.name, method, W, H)


def check_against_brute_force(gpu, scene, W, H, radius):
    """The last iteration's merge buffers against the brute force over its vertex buffers.
    Returns the total accepted pairs."""
    npx = W * H
    K = gpu._cfg.vcm_max_path_length
    lv = gpu.read_buffer(_abi.BUF_VCM_VERTICES).reshape(9, npx, 16)
    lc = gpu.read_buffer(_abi.BUF_VCM_VERTEX_COUNT, np.uint32)
    cv = gpu.read_buffer(_abi.BUF_VCM_CAMERA_VERTICES).reshape(K, npx, 16)
    cc = gpu.read_buffer(_abi.BUF_VCM_CAMERA_VERTEX_COUNT, np.uint32)
    merge = gpu.read_buffer(_abi.BUF_VCM_MERGE).reshape(npx, 3)
    count = gpu.read_buffer(_abi.BUF_VCM_MERGE_COUNT, np.uint32)
    cand = gpu.read_buffer(_abi.BUF_VCM_MERGE_CANDIDATES, np.uint32)
    assert cc.max() <= K and lc.sum() > 0 and cc.sum() > 0
    ref_color, ref_count = vcm_merge_ref.merge_reference(lv, lc, cv, cc, scene.materials, W, H, radius)
    total = int(ref_count.sum())
    err = rel_l2(merge, ref_color) if total else 0.0
    print(f"merge {scene.name} {W}x{H} r={radius}: light vertices {int(np.minimum(lc, 9).sum())}, camera vertices "
          f"{int(cc.sum())}, accepted pairs {total}, candidates {int(cand.sum())}, rel-L2 {err:.3e}")
    assert np.array_equal(count.astype(np.int64), ref_count)
    assert (cand >= count).all()
    assert np.isfinite(merge).all()
    if total == 0:
        assert not merge.any()
    else:
        assert err <= 1e-5
    return total


@pytest.mark.parametrize("radius", [30.0, 1e-3, 300.0])
@pytest.mark.parametrize("scene_name,W,H", [("Cornell", 32, 32), ("Cornell", 48, 40), ("CornellGlossyFloor", 32, 32)])
def test_merge_matches_brute_force(scene_name, W, H, radius):
    """48x40: W is no multiple of 8 and the light-vertex count no multiple of 64.  r = 30: a window of a few
    cells; 1e-3: no pair at all; 300: one cell, the window clamped on every side, nearly every pair accepted."""
    scene = SCENES[scene_name]()
    gpu = make(scene)
    det = request(scene, VCM, W, H)
    for i in range(2):
        gpu.renderNextIteration(i, i, radius, True, det)
    assert not gpu.pipelined()
    total = check_against_brute_force(gpu, scene, W, H, radius)
    if W == 48:
        assert int(np.minimum(gpu.read_buffer(_abi.BUF_VCM_VERTEX_COUNT, np.uint32), 9).sum()) % 64 != 0
    if radius == 30.0:
        assert total >= 1000
    elif radius == 1e-3:
        assert total == 0
    else:  # the radius exceeds the scene: one cell, so every camera vertex tests every light vertex
        lc = np.minimum(gpu.read_buffer(_abi.BUF_VCM_VERTEX_COUNT, np.uint32), 9).astype(np.int64).sum()
        cc = gpu.read_buffer(_abi.BUF_VCM_CAMERA_VERTEX_COUNT, np.uint32).astype(np.int64).sum()
        assert int(gpu.read_buffer(_abi.BUF_VCM_MERGE_CANDIDATES, np.uint32).astype(np.int64).sum()) == lc * cc
        assert total >= 1000
    st = gpu.stats()
    assert st.pass_ms[_abi.PASS_VCM_GRID] > 0 and st.pass_ms[_abi.PASS_VCM_MERGE] > 0
    gpu.destroy()


def test_merging_leaves_the_walks_unchanged():
    """Merging draws no random numbers and changes only dVC (plane C.w) of the light vertices."""
    scene = scenes.cornell()
    W = H = 32
    npx = W * H
    bufs = []
    for merging in (0, 1):
        gpu = make(scene, merging)
        det = request(scene, VCM, W, H)
        for i in range(2):
            gpu.renderNextIteration(i, i, 30.0, True, det)
        b = {"rng": gpu.read_buffer(_abi.BUF_RNG, np.uint32), "count": gpu.read_buffer(_abi.BUF_VCM_VERTEX_COUNT, np.uint32),
             "verts": gpu.read_buffer(_abi.BUF_VCM_VERTICES).reshape(9, npx, 16).view(np.uint32)}
        if merging:
            cam = gpu.read_buffer(_abi.BUF_VCM_CAMERA).astype(np.float64)
            mrg = gpu.read_buffer(_abi.BUF_VCM_MERGE).astype(np.float64)
            assert np.isfinite(cam - mrg).all() and mrg.any()
        bufs.append(b)
        gpu.destroy()
    off, on = bufs
    assert np.array_equal(off["rng"], on["rng"])
    assert np.array_equal(off["count"], on["count"])
    valid = np.arange(9)[:, None] < np.minimum(off["count"], 9)[None, :]
    assert valid.any()
    same = [w for w in range(16) if w != 11]  # everything but C.w = dVC
    assert np.array_equal(off["verts"][valid][:, same], on["verts"][valid][:, same])
    assert (off["verts"][valid][:, 11] != on["verts"][valid][:, 11]).any()


def test_merging_is_deterministic():
    """No float atomics in the merge: two fresh renderers give the same merging colour, camera colour
    (connections + merging) and output bit for bit.  The output also holds the light-tracing splats, whose
    hardware atomics add in no fixed order: should two runs' splat images differ in a last bit, the output
    is held to that difference instead."""
    scene = scenes.scene_by_name("CornellSmall")
    W, H = 40, 32
    runs = []
    for _ in range(2):
        gpu = make(scene)
        det = request(scene, VCM, W, H)
        # the scene's own initial radius (1.7e-4 of a 2.5-unit room) finds no pair among 1280 subpaths
        r = 0.15
        splats = []
        for i in range(3):
            gpu.renderNextIteration(i, i, r, True, det)
            splats.append(gpu.read_buffer(_abi.BUF_VCM_SPLAT).copy())
            r = next_ppm_radius(r, i)
        runs.append((gpu.read_buffer(_abi.BUF_VCM_MERGE).copy(), gpu.read_buffer(_abi.BUF_VCM_CAMERA).copy(),
                     gpu.getOutputBuffer().copy(), np.stack(splats)))
        gpu.destroy()
    (m0, c0, o0, s0), (m1, c1, o1, s1) = runs
    assert np.isfinite(m0).all() and m0.any() and np.isfinite(o0).all()
    assert m0.tobytes() == m1.tobytes()
    assert c0.tobytes() == c1.tobytes()
    if s0.tobytes() == s1.tobytes():
        assert o0.tobytes() == o1.tobytes()
    else:  # a last-bit splat difference per iteration and the rounding of the three accumulations it shifts
        assert np.abs(s0.astype(np.float64) - s1).max() <= 2.0 ** -22 * np.abs(s0).max()
        np.testing.assert_allclose(o0, o1, rtol=1e-6, atol=0)


def _mean_luminance(scene, merging, seed, W=64, H=64, iters=32):
    gpu = make(scene, merging, seed=seed)
    det = request(scene, VCM, W, H)
    r = 4.0 * scene.initial_ppm_radius()
    for i in range(iters):
        gpu.renderNextIteration(i, i, r, True, det)
        r = next_ppm_radius(r, i)
    out = gpu.getOutputBuffer().astype(np.float64) / iters
    gpu.destroy()
    assert np.isfinite(out).all()
    return float((out @ np.array([0.2126, 0.7152, 0.0722])).mean())


def test_merging_conserves_energy():
    """Cornell 64x64, 32 iterations, radii from 4 x the initial PPM radius: the image-mean luminance with
    merging on differs from merging off (same seed) by no more than 3 x the largest difference between
    three merging-off runs with different seeds.  The factor 3 allows for the small kernel bias of
    merging; a missing normalisation or misVm left at 0 changes the brightness by tens of percent.

    Measured on an MI355X: on/off difference 0.2334 % (mean luminance 0.155245 on, 0.154884 off),
    largest seed-to-seed difference 0.2116 % (0.154884, 0.154579, 0.154557)."""
    scene = scenes.cornell()
    off = [_mean_luminance(scene, 0, s) for s in (SEED, SEED + 1, SEED + 2)]
    on = _mean_luminance(scene, 1, SEED)
    noise = max(abs(a - b) / b for a in off for b in off)
    diff = abs(on - off[0]) / off[0]
    print(f"energy: mean luminance off {off}, on {on}: on/off difference {diff:.4%}, seed-to-seed {noise:.4%}")
    assert noise > 0
    assert diff <= 3.0 * noise


def test_interface_errors():
    lib = load_library()
    scene = scenes.cornell()
    det = request(scene, VCM, 32, 32)
    gpu = make(scene, 0)
    gpu.renderNextIteration(0, 0, 30.0, True, det)
    for buf in (_abi.BUF_VCM_CAMERA_VERTEX_COUNT, _abi.BUF_VCM_CAMERA_VERTICES, _abi.BUF_VCM_MERGE,
                _abi.BUF_VCM_MERGE_COUNT):
        with pytest.raises(OrxError) as e:
            gpu.read_buffer(buf)
        assert e.value.status == _abi.ORX_ERR_STATE
    gpu.destroy()
    h = C.c_void_p()
    cfg = _abi.default_config(vcm_merging=2)
    assert lib.orx_create(0, C.byref(cfg), C.byref(h)) == _abi.ORX_ERR_INVALID_ARGUMENT and not h.value
    # the pair counts are debug counters
    gpu = make(scene, 1, debug_counters=0)
    gpu.renderNextIteration(0, 0, 30.0, True, det)
    assert gpu.read_buffer(_abi.BUF_VCM_MERGE).any()
    with pytest.raises(OrxError) as e:
        gpu.read_buffer(_abi.BUF_VCM_MERGE_COUNT)
    assert e.value.status == _abi.ORX_ERR_STATE
    gpu.destroy()
    # a rank of a row partition would need every rank's light vertices
    gpu = make(scene, 1)
    gpu.set_shard(0, 2)
    lib.orx_vcm_local_light.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_float, C.c_void_p]
    lib.orx_vcm_local_light.restype = C.c_int
    req = det.to_abi()
    assert lib.orx_vcm_local_light(gpu._h, 0, 0, 30.0, C.byref(req)) == _abi.ORX_ERR_UNSUPPORTED
    assert b"single-device" in lib.orx_last_error(gpu._h)
    gpu.destroy()


def test_one_rank_rows_group_matches_the_renderer():
    scene = scenes.cornell()
    W, H = 48, 40
    det = request(scene, VCM, W, H)
    cfg = dict(seed=SEED, photon_launch_width=32, photon_launch_height=32, vcm_merging=1)
    gpu = make(scene)
    g = OptixRendererGroup(_abi.default_config(**cfg),
                           _abi.default_group_config(partition=_abi.GROUP_ROWS, comm=_abi.COMM_LOCAL))
    g.initialize([0])
    g.initScene(scene)
    r = scene.initial_ppm_radius()
    rank = g.renderer(0)
    splats_equal = True
    for i in range(3):
        gpu.renderNextIteration(i, i, r, True, det)
        g.renderNextIteration(i, i, r, True, det)
        # everything the merge and the connections compute is bit-equal, iteration by iteration
        for buf in (_abi.BUF_VCM_MERGE, _abi.BUF_VCM_CAMERA, _abi.BUF_VCM_CAMERA_VERTEX_COUNT, _abi.BUF_VCM_MERGE_COUNT):
            assert gpu.read_buffer(buf).tobytes() == rank.read_buffer(buf).tobytes()
        splats_equal &= gpu.read_buffer(_abi.BUF_VCM_SPLAT).tobytes() == rank.read_buffer(_abi.BUF_VCM_SPLAT).tobytes()
        r = next_ppm_radius(r, i)
    assert gpu.read_buffer(_abi.BUF_VCM_MERGE).any()
    a, b = gpu.getOutputBuffer(), g.getOutputBuffer()
    assert a.any()
    # the output also sums the light-tracing splats, float atomics in every mode: bit for bit whenever
    # the two runs' splat images are, to their last-bit differences otherwise
    if splats_equal:
        assert a.tobytes() == b.tobytes()
    else:
        np.testing.assert_allclose(a, b, rtol=1e-6, atol=0)
    g.destroy()
    gpu.destroy()


@pytest.mark.parametrize("method", [_abi.PATH_TRACING, _abi.PROGRESSIVE_PHOTON_MAPPING])
def test_other_methods_are_unaffected(method):
    scene = scenes.cornell()
    det = request(scene, method, 32, 32)
    outs = []
    for merging in (0, 1):
        gpu = make(scene, merging)
        r = scene.initial_ppm_radius()
        for i in range(2):
            gpu.renderNextIteration(i, i, r, True, det)
            r = next_ppm_radius(r, i)
        outs.append(gpu.getOutputBuffer().copy())
        gpu.destroy()
    assert outs[0].any()
    # PT is bit-exact; the PPM gather sums a cell's photons in atomic-rank order (tests/test_gpu_parity.py)
    if method == _abi.PATH_TRACING:
        assert outs[0].tobytes() == outs[1].tobytes()
    else:
        assert rel_l2(outs[1], outs[0]) <= 1e-5


def test_resize_reallocates_the_caches():
    scene = scenes.cornell()
    gpu = make(scene)
    gpu.renderNextIteration(0, 0, 30.0, True, request(scene, VCM, 32, 32))
    check_against_brute_force(gpu, scene, 32, 32, 30.0)
    gpu.renderNextIteration(1, 0, 30.0, True, request(scene, VCM, 48, 40))
    assert check_against_brute_force(gpu, scene, 48, 40, 30.0) >= 1000
    gpu.renderNextIteration(2, 0, 30.0, True, request(scene, VCM, 32, 32))
    check_against_brute_force(gpu, scene, 32, 32, 30.0)
    gpu.destroy()


def test_texture_vertices_merge():
    """Texture materials keep their texel colour beside the 64-B records (the TEX walks and the fifth
    plane): the pair counts equal the brute force's, and the merging colour is finite, non-zero and the
    same bits in two fresh renderers.  (The colour itself has no reference here: the texel colours are not
    part of the readable vertex buffers.)"""
    from oppositerenderer_amd import synthetic
    scene = synthetic.textured_room()
    W, H = 56, 48
    det = request(scene, VCM, W, H)
    radius = 0.05 * float(np.max(np.asarray(scene.aabb_max) - np.asarray(scene.aabb_min)))
    merges = []
    for _ in range(2):
        gpu = make(scene)
        for i in range(2):
            gpu.renderNextIteration(i, i, radius, True, det)
        merges.append(gpu.read_buffer(_abi.BUF_VCM_MERGE).copy())
        if len(merges) == 1:
            npx = W * H
            want = vcm_merge_ref.accepted_pairs(
                gpu.read_buffer(_abi.BUF_VCM_VERTICES).reshape(9, npx, 16), gpu.read_buffer(_abi.BUF_VCM_VERTEX_COUNT, np.uint32),
                gpu.read_buffer(_abi.BUF_VCM_CAMERA_VERTICES).reshape(-1, npx, 16),
                gpu.read_buffer(_abi.BUF_VCM_CAMERA_VERTEX_COUNT, np.uint32), radius)
            got = gpu.read_buffer(_abi.BUF_VCM_MERGE_COUNT, np.uint32)
            print(f"texture merge: accepted pairs {int(want.sum())}")
            assert np.array_equal(got.astype(np.int64), want) and want.sum() >= 1000
        gpu.destroy()
    assert np.isfinite(merges[0]).all() and merges[0].any()
    assert merges[0].tobytes() == merges[1].tobytes()
