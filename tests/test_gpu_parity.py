"""GPU parity: liborx.so (HIP, gfx950) against the CPU oracle on identical seeds.

Bar (north_star): output within 1e-4 relative L2; every integer/index
quantity (RNG states, grid offsets, photon-to-cell assignment) and every
control-flow-derived value (hit points, photon deposits, direct light) must be
bit-exact.  The only fp32 values allowed to differ are sums whose order the
GPU changes: the gather accumulates a cell's photons in atomic-rank order
instead of the stable-sort order.
"""
import numpy as np
import pytest

import oracle_lib
from oppositerenderer_amd import _abi, scenes
from oppositerenderer_amd.renderer import OptixRenderer, RenderRequestDetails, next_ppm_radius

pytestmark = pytest.mark.gpu
SEED = 1645301512  # DEBUG_RANDOM_SEED (config.h:50)


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    den = np.sqrt((b * b).sum())
    return float(np.sqrt(((a - b) ** 2).sum()) / max(den, 1e-30))


def make_pair(scene, W, H, P, method, **cfg):
    c = _abi.default_config(seed=SEED, photon_launch_width=P, photon_launch_height=P, **cfg)
    gpu = OptixRenderer(c)
    gpu.initialize(0)
    gpu.initScene(scene)
    cfg.pop("gather_variant", None)
    c2 = _abi.default_config(seed=SEED, photon_launch_width=P, photon_launch_height=P, **cfg)
    ora = oracle_lib.OracleRenderer(c2)
    ora.init_scene(scene)
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
    det = RenderRequestDetails(cam, scene.name, method, W, H)
    return gpu, ora, det


def cell_multisets(photons, offsets):
    """photons: [n,9] grid-ordered; returns per-cell lexicographically sorted rows."""
    rows = photons.view(np.uint32).reshape(-1, 9)
    out = []
    for c in range(len(offsets) - 1):
        a, b = offsets[c], offsets[c + 1]
        if b > a:
            seg = rows[a:b]
            out.append(seg[np.lexsort(seg.T[::-1])])
    return out


def check_ppm_iteration(gpu, ora):
    # bit-exact: RNG, hitpoints, offsets, direct
    for buf, dt in ((_abi.BUF_RNG, np.uint32), (_abi.BUF_HITPOINTS, np.uint32), (_abi.BUF_GRID_OFFSETS, np.uint32),
                    (_abi.BUF_DIRECT, np.uint32), (_abi.BUF_DEBUG_VISITED, np.uint32)):
        g = gpu.read_buffer(buf, dt)
        o = ora.read_buffer(buf, dt)
        assert g.shape == o.shape, buf
        mism = np.count_nonzero(g != o)
        assert mism == 0, f"buffer {buf}: {mism} of {g.size} words differ"
    gs, os_ = gpu.stats(), ora.stats()
    assert list(gs.grid_size) == list(os_.grid_size)
    assert np.float32(gs.cell_size) == np.float32(os_.cell_size)
    assert gs.valid_photons == os_.valid_photons
    assert gs.photons_visited == os_.photons_visited
    # photon grid: same photons in every cell
    off = gpu.read_buffer(_abi.BUF_GRID_OFFSETS, np.uint32)
    gp = gpu.read_buffer(_abi.BUF_PHOTONS).reshape(-1, 9)
    op = ora.read_buffer(_abi.BUF_PHOTONS).reshape(-1, 9)
    assert gp.shape == op.shape
    for a, b in zip(cell_multisets(gp, off), cell_multisets(op, off)):
        assert np.array_equal(a, b)
    # indirect: only summation order differs
    gi = gpu.read_buffer(_abi.BUF_INDIRECT)
    oi = ora.read_buffer(_abi.BUF_INDIRECT)
    assert rel_l2(gi, oi) < 1e-5
    np.testing.assert_allclose(gi, oi, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("gather_variant", [0, 1, 2])
@pytest.mark.parametrize("scene_name,W,H,P", [("Cornell", 64, 64, 128), ("Cornell", 96, 80, 64),
                                              ("CornellSmall", 64, 64, 128)])
def test_ppm_parity(scene_name, W, H, P, gather_variant):
    scene = scenes.scene_by_name(scene_name)
    gpu, ora, det = make_pair(scene, W, H, P, _abi.PROGRESSIVE_PHOTON_MAPPING, gather_variant=gather_variant)
    radius = scene.initial_ppm_radius()
    req = det.to_abi()
    for it in range(3):
        gpu.renderNextIteration(it, it, radius, True, det)
        ora.render_next_iteration(it, it, radius, req)
        check_ppm_iteration(gpu, ora)
        radius = next_ppm_radius(radius, it)
    g = gpu.getOutputBuffer()
    o = ora.output()
    assert rel_l2(g, o) < 1e-4, rel_l2(g, o)
    gpu.destroy()
    ora.close()


@pytest.mark.parametrize("radius", [None, 5000.0])
def test_ppm_union_weight_forms(radius):
    """The union gather evaluates its weight polynomial in d^2 with per-launch coefficients c_k / r^(2k)
    divided through by c_4 / r^8 (launch_ppm_gather), falling back to the polynomial in u = d^2 / r^2 where
    that scale leaves [1e-20, 1e20]: a 5000-unit radius over the 550-unit Cornell box takes the fallback
    (c_4 / r^8 ~ 2e-31; every photon is a candidate of every pixel).  Both forms against the oracle
    (accepted sets exact), and the u form forced (ORX_GATHER_DFORM=0) in a child process."""
    import subprocess, sys, os, json
    if radius is None:
        code = r'''
import json, sys
sys.path.insert(0, "tests")
import test_gpu_parity as t
from oppositerenderer_amd import _abi, scenes
from oppositerenderer_amd.renderer import next_ppm_radius
scene = scenes.scene_by_name("Cornell")
gpu, ora, det = t.make_pair(scene, 64, 48, 64, _abi.PROGRESSIVE_PHOTON_MAPPING)
r = scene.initial_ppm_radius()
for it in range(2):
    gpu.renderNextIteration(it, it, r, True, det)
    ora.render_next_iteration(it, it, r, det.to_abi())
    t.check_ppm_iteration(gpu, ora)
    r = next_ppm_radius(r, it)
print(json.dumps({"err": t.rel_l2(gpu.getOutputBuffer(), ora.output())}))
'''
        env = dict(os.environ, ORX_GATHER_DFORM="0")
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=110,
                             cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        assert out.returncode == 0, out.stderr[-2000:]
        assert json.loads(out.stdout.strip().splitlines()[-1])["err"] < 1e-4
        return
    scene = scenes.scene_by_name("Cornell")
    gpu, ora, det = make_pair(scene, 48, 40, 64, _abi.PROGRESSIVE_PHOTON_MAPPING)
    req = det.to_abi()
    for it in range(2):
        gpu.renderNextIteration(it, it, radius, True, det)
        ora.render_next_iteration(it, it, radius, req)
        check_ppm_iteration(gpu, ora)
    assert rel_l2(gpu.getOutputBuffer(), ora.output()) < 1e-4
    gpu.destroy()
    ora.close()


@pytest.mark.parametrize("scene_name,W,H", [("Cornell", 64, 64), ("CornellSmallLargeSphere", 48, 48),
                                            ("CornellSmallSmallSpheres", 48, 40)])
def test_pt_parity(scene_name, W, H):
    scene = scenes.scene_by_name(scene_name)
    gpu, ora, det = make_pair(scene, W, H, 64, _abi.PATH_TRACING)
    req = det.to_abi()
    for it in range(3):
        gpu.renderNextIteration(it, it, 1.0, True, det)
        ora.render_next_iteration(it, it, 1.0, req)
        g = gpu.read_buffer(_abi.BUF_RNG, np.uint32)
        o = ora.read_buffer(_abi.BUF_RNG, np.uint32)
        assert np.array_equal(g, o)
    g = gpu.getOutputBuffer()
    o = ora.output()
    # no order-dependent sums in PT: bit-exact
    assert np.array_equal(g.view(np.uint32), o.view(np.uint32)), rel_l2(g, o)
    gpu.destroy()
    ora.close()


def test_ppm_specular_scenes_parity():
    """Mirror + glass spheres and a point light (Glass.cu, Mirror.cu, PhotonGenerator.cu point branch)."""
    for name in ("CornellSmallLargeSphere", "CornellSmallSmallSpheres", "CornellSmallPointDistant"):
        scene = scenes.scene_by_name(name)
        gpu, ora, det = make_pair(scene, 48, 48, 96, _abi.PROGRESSIVE_PHOTON_MAPPING)
        radius = scene.initial_ppm_radius()
        req = det.to_abi()
        for it in range(2):
            gpu.renderNextIteration(it, it, radius, True, det)
            ora.render_next_iteration(it, it, radius, req)
            check_ppm_iteration(gpu, ora)
            radius = next_ppm_radius(radius, it)
        assert rel_l2(gpu.getOutputBuffer(), ora.output()) < 1e-4
        gpu.destroy()
        ora.close()


def test_resize_reinitialises_rng():
    """A width/height change re-seeds the RNG buffer (OptixRenderer.cpp:534-537, :828-848)."""
    scene = scenes.cornell()
    gpu, ora, det = make_pair(scene, 32, 32, 32, _abi.PATH_TRACING)
    gpu.renderNextIteration(0, 0, 1.0, True, det)
    det.width, det.height = 40, 24
    gpu.renderNextIteration(1, 0, 1.0, True, det)
    ora.render_next_iteration(1, 0, 1.0, det.to_abi())
    assert gpu.getWidth() == 40 and gpu.getHeight() == 24
    assert np.array_equal(gpu.getOutputBuffer().view(np.uint32), ora.output().view(np.uint32))
    gpu.destroy()


def test_error_paths():
    from oppositerenderer_amd.renderer import OrxError
    r = OptixRenderer(_abi.default_config(seed=SEED))
    with pytest.raises(OrxError):
        r.initScene(scenes.cornell())  # before initialize
    r.initialize(0)
    with pytest.raises(OrxError):
        r.initialize(0)  # Multiple OptixRenderer::initialize
    sc = scenes.cornell()
    sc.lights = []
    with pytest.raises(OrxError):
        r.initScene(sc)  # No lights exists in this scene.
    r.destroy()


def test_photon_stack_error_is_a_status():
    """A photon pass whose deep-stack buffer does not cover the launch returns ORX_ERR_STATE through
    the ABI (the reference throws, OptixRenderer.cpp:816-820) instead of aborting the host process;
    the renderer recovers at the next resize."""
    import ctypes as C

    from oppositerenderer_amd.renderer import OrxError
    scene = scenes.cornell()
    W, H, P = 32, 24, 32
    r = OptixRenderer(_abi.default_config(seed=SEED, photon_launch_width=P, photon_launch_height=P))
    r.initialize(0)
    r.initScene(scene)
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
    det = RenderRequestDetails(cam, scene.name, _abi.PROGRESSIVE_PHOTON_MAPPING, W, H)
    radius = scene.initial_ppm_radius()
    r.renderNextIteration(0, 0, radius, False, det)
    f = r._lib.orx_debug_limit_photon_stack
    f.argtypes, f.restype = [C.c_void_p, C.c_uint32], C.c_int
    assert f(r._h, 64) == 0
    with pytest.raises(OrxError, match="traversal-stack"):
        r.renderNextIteration(1, 1, radius, False, det)
    det2 = RenderRequestDetails(cam, scene.name, _abi.PROGRESSIVE_PHOTON_MAPPING, W + 8, H)
    r.renderNextIteration(0, 0, radius, True, det2)  # a resize sizes the buffer again
    assert r.getOutputBuffer().sum() > 0
    r.destroy()


@pytest.mark.parametrize("method", [_abi.PROGRESSIVE_PHOTON_MAPPING, _abi.PATH_TRACING])
def test_mesh_bvh_parity(method):
    """Synthetic Sponza-class hall (261k triangles, smooth normals): the device
    SAH BVH and the oracle's median-split BVH must report the same closest hits."""
    from oppositerenderer_amd import synthetic
    scene = synthetic.synthetic_hall()
    gpu, ora, det = make_pair(scene, 80, 45, 96, method)
    radius = scene.initial_ppm_radius()
    req = det.to_abi()
    for it in range(2):
        gpu.renderNextIteration(it, it, radius, True, det)
        ora.render_next_iteration(it, it, radius, req)
        if method == _abi.PROGRESSIVE_PHOTON_MAPPING:
            check_ppm_iteration(gpu, ora)
        else:
            assert np.array_equal(gpu.read_buffer(_abi.BUF_RNG, np.uint32), ora.read_buffer(_abi.BUF_RNG, np.uint32))
        radius = next_ppm_radius(radius, it)
    g, o = gpu.getOutputBuffer(), ora.output()
    if method == _abi.PATH_TRACING:
        assert np.array_equal(g.view(np.uint32), o.view(np.uint32)), rel_l2(g, o)
    else:
        assert rel_l2(g, o) < 1e-4
    gpu.destroy()
    ora.close()


def check_vcm_iteration(gpu, ora):
    """Bit-exact: RNG, per-subpath vertex counts, every stored light vertex,
    each pixel's camera-subpath colour.  Order-dependent: the light-tracing
    splats (atomic adds from any light subpath into any pixel)."""
    for buf in (_abi.BUF_RNG, _abi.BUF_VCM_VERTEX_COUNT, _abi.BUF_VCM_CAMERA):
        g = gpu.read_buffer(buf, np.uint32)
        o = ora.read_buffer(buf, np.uint32)
        assert g.shape == o.shape, buf
        mism = np.count_nonzero(g != o)
        assert mism == 0, f"buffer {buf}: {mism} of {g.size} words differ"
    cnt = gpu.read_buffer(_abi.BUF_VCM_VERTEX_COUNT, np.uint32)
    gv = gpu.read_buffer(_abi.BUF_VCM_VERTICES, np.uint32).reshape(9, -1, 16)
    ov = ora.read_buffer(_abi.BUF_VCM_VERTICES, np.uint32).reshape(9, -1, 16)
    valid = np.arange(9)[:, None] < np.minimum(cnt, 9)[None, :]
    assert np.array_equal(gv[valid], ov[valid])
    gs = gpu.read_buffer(_abi.BUF_VCM_SPLAT)
    os_ = ora.read_buffer(_abi.BUF_VCM_SPLAT)
    assert rel_l2(gs, os_) < 1e-5, rel_l2(gs, os_)
    np.testing.assert_allclose(gs, os_, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("scene_name,W,H", [("Cornell", 64, 64), ("CornellSmall", 48, 40),
                                            ("CornellSmallLargeSphere", 48, 48),
                                            ("CornellSmallSmallSpheres", 40, 40),
                                            ("CornellSmallPointDistant", 40, 32),
                                            ("CornellSmallLightUpwards", 32, 32)])
def test_vcm_parity(scene_name, W, H):
    """VCM light + camera passes (vcm/VCMLightPass.cu, VCMCameraPass.cu), including
    the first iteration's subpath-length estimate launch (OptixRenderer.cpp:699-763)."""
    scene = scenes.scene_by_name(scene_name)
    gpu, ora, det = make_pair(scene, W, H, 64, _abi.VCM_BIDIRECTIONAL_PATH_TRACING)
    radius = scene.initial_ppm_radius()
    req = det.to_abi()
    for it in range(3):
        gpu.renderNextIteration(it, it, radius, True, det)
        ora.render_next_iteration(it, it, radius, req)
        check_vcm_iteration(gpu, ora)
        radius = next_ppm_radius(radius, it)
    g, o = gpu.getOutputBuffer(), ora.output()
    assert np.isfinite(g).all()
    assert rel_l2(g, o) < 1e-4, rel_l2(g, o)
    gpu.destroy()
    ora.close()


def test_vcm_mesh_parity():
    """VCM on the triangle-mesh hall (BVH traversal for subpaths, shadow and connection rays)."""
    from oppositerenderer_amd import synthetic
    scene = synthetic.synthetic_hall()
    gpu, ora, det = make_pair(scene, 64, 36, 64, _abi.VCM_BIDIRECTIONAL_PATH_TRACING)
    radius = scene.initial_ppm_radius()
    req = det.to_abi()
    for it in range(2):
        gpu.renderNextIteration(it, it, radius, True, det)
        ora.render_next_iteration(it, it, radius, req)
        check_vcm_iteration(gpu, ora)
        radius = next_ppm_radius(radius, it)
    assert rel_l2(gpu.getOutputBuffer(), ora.output()) < 1e-4
    gpu.destroy()
    ora.close()


def test_vcm_resize_reruns_estimate():
    """resizeBuffers clears m_lightVertexCountEstimated (OptixRenderer.cpp:847): the
    estimate launch runs again and advances the RNG; pixelSizeFactor follows the size."""
    scene = scenes.scene_by_name("CornellSmall")
    gpu, ora, det = make_pair(scene, 32, 32, 32, _abi.VCM_BIDIRECTIONAL_PATH_TRACING)
    for it, (w, h) in enumerate([(32, 32), (32, 32), (40, 24)]):
        det.width, det.height = w, h
        gpu.renderNextIteration(it, it, 0.05, True, det)
        ora.render_next_iteration(it, it, 0.05, det.to_abi())
        check_vcm_iteration(gpu, ora)
    assert rel_l2(gpu.getOutputBuffer(), ora.output()) < 1e-4
    gpu.destroy()
    ora.close()


@pytest.mark.parametrize("method", [_abi.PROGRESSIVE_PHOTON_MAPPING, _abi.PATH_TRACING,
                                    _abi.VCM_BIDIRECTIONAL_PATH_TRACING])
def test_texture_parity(method):
    """Texture material (material/Texture.cu): bilinear wrap sampling of the
    diffuse map, normal mapping with interpolated tangents, the photon program's
    0.01 cutoffs and VCM Lambertian(texel) vertices, on the TexturedRoom mesh."""
    from oppositerenderer_amd import synthetic
    scene = synthetic.textured_room()
    gpu, ora, det = make_pair(scene, 56, 48, 64, method)
    radius = scene.initial_ppm_radius()
    req = det.to_abi()
    for it in range(3):
        gpu.renderNextIteration(it, it, radius, True, det)
        ora.render_next_iteration(it, it, radius, req)
        if method == _abi.PROGRESSIVE_PHOTON_MAPPING:
            check_ppm_iteration(gpu, ora)
        elif method == _abi.VCM_BIDIRECTIONAL_PATH_TRACING:
            check_vcm_iteration(gpu, ora)
        else:
            assert np.array_equal(gpu.read_buffer(_abi.BUF_RNG, np.uint32), ora.read_buffer(_abi.BUF_RNG, np.uint32))
        radius = next_ppm_radius(radius, it)
    g, o = gpu.getOutputBuffer(), ora.output()
    assert np.isfinite(g).all() and g.mean() > 0
    if method == _abi.PATH_TRACING:
        assert np.array_equal(g.view(np.uint32), o.view(np.uint32)), rel_l2(g, o)
    else:
        assert rel_l2(g, o) < 1e-4, rel_l2(g, o)
    gpu.destroy()
    ora.close()


@pytest.mark.parametrize("method", [_abi.PATH_TRACING, _abi.PROGRESSIVE_PHOTON_MAPPING])
def test_device_bvh_matches_host_bvh(method, monkeypatch):
    """The on-device binned-SAH build (orx_bvh.hip) and the host builder give
    different trees but identical closest hits: bit-identical PT output and PPM
    hitpoints / deposits on the hall mesh."""
    from oppositerenderer_amd import synthetic
    scene = synthetic.synthetic_hall()
    outs, stats = [], []
    for host in ("0", "1"):
        monkeypatch.setenv("ORX_BVH_HOST", host)
        c = _abi.default_config(seed=SEED, photon_launch_width=96, photon_launch_height=96)
        gpu = OptixRenderer(c)
        gpu.initialize(0)
        gpu.initScene(scene)
        cam = scene.default_camera.set_aspect_ratio(float(np.float32(80) / np.float32(45)))
        det = RenderRequestDetails(cam, scene.name, method, 80, 45)
        radius = scene.initial_ppm_radius()
        for it in range(2):
            gpu.renderNextIteration(it, it, radius, True, det)
            radius = next_ppm_radius(radius, it)
        bufs = [gpu.read_buffer(_abi.BUF_RNG, np.uint32)]
        if method == _abi.PROGRESSIVE_PHOTON_MAPPING:
            bufs += [gpu.read_buffer(_abi.BUF_HITPOINTS, np.uint32), gpu.read_buffer(_abi.BUF_GRID_OFFSETS, np.uint32)]
        outs.append((gpu.getOutputBuffer(), bufs))
        stats.append(gpu.stats().bvh_stack_entries)
        gpu.destroy()
    (g0, b0), (g1, b1) = outs
    for a, b in zip(b0, b1):
        assert np.array_equal(a, b)
    if method == _abi.PATH_TRACING:
        assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
    else:
        assert rel_l2(g0, g1) < 1e-5
    assert 0 < stats[0] <= 96


@pytest.mark.gpu
def test_wire_server_packet_matches_oracle():
    """A render server's packet (wire.render_request on the HIP renderer: a run of iterations with
    the client's radii, local iteration numbers 0..n-1, output = sum over the run) equals the
    oracle's for the same request, and survives the reference framing bit for bit."""
    from oppositerenderer_amd import wire
    scene = scenes.scene_by_name("Cornell")
    W, H, P = 48, 40, 64
    gpu, ora, det = make_pair(scene, W, H, P, _abi.PROGRESSIVE_PHOTON_MAPPING)
    d = wire.RenderServerRenderRequestDetails.from_camera(det.camera, scene.name, det.render_method, W, H)
    gen = wire.RequestGenerator(scene.initial_ppm_radius(), d)
    gen.next_request(2)  # this server's run starts at iteration 2
    req = wire.RenderServerRenderRequest.decode(gen.next_request(3).encode())
    pkt = wire.RenderResultPacket.decode(wire.render_request(gpu, req, det).encode())
    for i, (it, r) in enumerate(zip(req.iteration_numbers, req.ppm_radii)):
        ora.render_next_iteration(it, i, r, det.to_abi())
    ref = ora.output().reshape(-1)
    assert pkt.iteration_numbers == [2, 3, 4] and pkt.output.shape == ref.shape
    assert rel_l2(pkt.output, ref) < 1e-4
    rx = wire.RenderResultPacketReceiver(_abi.PROGRESSIVE_PHOTON_MAPPING)
    assert rx.onRenderResultPacketReceived(pkt, gen.sequence_number)
    assert rx.next_expected_iteration() == 0 and rx.getBackBufferNumIterations() == 3  # waits for 0..1
    gpu.destroy()
    ora.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name,W,H,P", [("Cornell", 64, 48, 64), ("CornellSmall", 48, 48, 32)])
def test_stochastic_hash_parity(scene_name, W, H, P):
    """photon_map = 1 (ACCELERATION_STRUCTURE_STOCHASTIC_HASH): uncapped deposits, the hash table
    (counts and the photon each entry keeps), the 27-cell gather and the output are bit-exact."""
    scene = scenes.scene_by_name(scene_name)
    gpu, ora, det = make_pair(scene, W, H, P, _abi.PROGRESSIVE_PHOTON_MAPPING,
                              photon_map=_abi.PHOTON_MAP_STOCHASTIC_HASH)
    radius = scene.initial_ppm_radius()
    for it in range(3):
        gpu.renderNextIteration(it, it, radius, True, det)
        ora.render_next_iteration(it, it, radius, det.to_abi())
        for buf, dt in ((_abi.BUF_RNG, np.uint32), (_abi.BUF_HITPOINTS, np.uint32), (_abi.BUF_GRID_OFFSETS, np.uint32),
                        (_abi.BUF_PHOTONS, np.uint32), (_abi.BUF_INDIRECT, np.uint32), (_abi.BUF_DIRECT, np.uint32),
                        (_abi.BUF_DEBUG_VISITED, np.uint32)):
            g, o = gpu.read_buffer(buf, dt), ora.read_buffer(buf, dt)
            assert g.shape == o.shape, buf
            assert np.count_nonzero(g != o) == 0, f"buffer {buf} differs (iteration {it})"
        gs, os_ = gpu.stats(), ora.stats()
        assert list(gs.grid_size) == list(os_.grid_size) and gs.cell_size == os_.cell_size
        assert gs.valid_photons == os_.valid_photons == ora.read_buffer(_abi.BUF_GRID_OFFSETS, np.uint32).sum()
        assert gs.num_cells == P * P * 4
        radius = next_ppm_radius(radius, it)
    g, o = gpu.getOutputBuffer(), ora.output()
    assert np.array_equal(g.view(np.uint32), o.view(np.uint32))
    assert g.mean() > 0
    gpu.destroy()
    ora.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name,W,H,P", [("Cornell", 64, 48, 64), ("CornellSmall", 48, 48, 32),
                                              ("Cornell", 32, 32, 256)])
def test_kdtree_parity(scene_name, W, H, P):
    """photon_map = 2 (ACCELERATION_STRUCTURE_KD_TREE_CPU, built on the device): RNG, hit points,
    photons and direct light are bit-exact; the device tree is a valid balanced kd-tree of the
    reference's shape (median = (start+end)/2 at every node) over exactly the valid photons; the
    indirect estimate matches within fp32 summation order.  Where several photons share a split
    coordinate, select.h's sequential partition decides which go left on the CPU and the slot
    order does here, so the subtrees below such a split hold different photons and the visit
    counters differ slightly; the search is exact in both, so every pixel accepts the same photons."""
    from test_kdtree import check_tree, read_tree

    scene = scenes.scene_by_name(scene_name)
    gpu, ora, det = make_pair(scene, W, H, P, _abi.PROGRESSIVE_PHOTON_MAPPING, photon_map=_abi.PHOTON_MAP_KD_TREE)
    radius = scene.initial_ppm_radius()
    for it in range(3):
        gpu.renderNextIteration(it, it, radius, True, det)
        ora.render_next_iteration(it, it, radius, det.to_abi())
        for buf in (_abi.BUF_RNG, _abi.BUF_HITPOINTS, _abi.BUF_DIRECT):
            g, o = gpu.read_buffer(buf, np.uint32), ora.read_buffer(buf, np.uint32)
            assert g.shape == o.shape and np.count_nonzero(g != o) == 0, f"buffer {buf} differs (iteration {it})"
        gs_, os_ = gpu.read_buffer(_abi.BUF_PHOTON_SLOTS).reshape(-1, 9), ora.read_buffer(_abi.BUF_PHOTON_SLOTS).reshape(-1, 9)
        valid = os_[:, 0:3].max(1) > 0
        assert np.array_equal(gs_[valid].view(np.uint32), os_[valid].view(np.uint32))
        gph, gax = read_tree(gpu)
        oph, oax = read_tree(ora)
        assert gph.shape == oph.shape
        idx = check_tree(gph, gax, os_[valid])
        assert np.array_equal(idx, check_tree(oph, oax, os_[valid]))
        gst, ost = gpu.stats(), ora.stats()
        assert gst.valid_photons == ost.valid_photons == int(valid.sum())
        assert gst.num_cells == ost.num_cells == gph.shape[0]
        assert abs(int(gst.photons_visited) - int(ost.photons_visited)) <= 0.05 * ost.photons_visited
        assert rel_l2(gpu.read_buffer(_abi.BUF_INDIRECT), ora.read_buffer(_abi.BUF_INDIRECT)) < 1e-5
        radius = next_ppm_radius(radius, it)
    g, o = gpu.getOutputBuffer(), ora.output()
    assert rel_l2(g, o) < 1e-5 and g.mean() > 0
    gpu.destroy()
    ora.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline,photon_map,large,gasync", [
    ("1", 0, False, "0"), ("0", 0, False, "0"), ("1", 1, False, "0"), ("1", 2, False, "0"), ("1", 1, True, "0"),
    ("1", 0, True, "0"), ("1", 0, False, "1"), ("1", 0, True, "1"), ("1", 0, False, "auto")])
def test_ppm_back_to_back_iterations(pipeline, photon_map, large, gasync, monkeypatch):
    """Iterations issued back to back with no read in between: with pipelining on (default) the
    gather + output of iteration i run beside the eye/photon/grid passes of i+1 on another
    buffer set; the running sum after five iterations (and a resolution change in between)
    matches the oracle as the serial schedule does.  gasync = "1": the grid build of i runs on a
    stream of its own beside the photon pass of i+1 (ORX_GRID_ASYNC=1, photon outputs alternate);
    "auto" (the default, ORX_GRID_ASYNC unset): the renderer times its first pipelined iteration and
    chooses, choosing again after the resize -- the images still match the oracle."""
    import subprocess, sys, os, json
    code = r'''
import json, sys, numpy as np
sys.path.insert(0, "tests")
import oracle_lib
from oppositerenderer_amd import _abi, scenes
from oppositerenderer_amd.renderer import OptixRenderer, RenderRequestDetails, next_ppm_radius
scene = scenes.cornell()
pm, large = int(sys.argv[1]), sys.argv[2] == "1"
P = 256 if large else (64 if pm == 1 else 96)  # the hash table needs a power-of-two deposit count
# 1080p-class rows; 100x30 leaves photon blocks right of the pixels in the shared rows (the
# photons the pipelined schedule launches before the eye pass: rows >= 30 and columns >= 128)
sizes = ((1920, 24, 4), (1280, 16, 2), (100, 30, 3)) if large else ((64, 48, 5), (40, 40, 3))
sched = []
cfg = _abi.default_config(seed=1645301512, photon_launch_width=P, photon_launch_height=P, photon_map=pm)
gpu = OptixRenderer(cfg); gpu.initialize(0); gpu.initScene(scene)
ora = oracle_lib.OracleRenderer(_abi.default_config(seed=1645301512, photon_launch_width=P, photon_launch_height=P,
                                                    photon_map=pm))
ora.init_scene(scene)
errs = []
for W, H, n in sizes:
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
    det = RenderRequestDetails(cam, scene.name, _abi.PROGRESSIVE_PHOTON_MAPPING, W, H)
    r = scene.initial_ppm_radius()
    for it in range(n):
        gpu.renderNextIteration(it, it, r, True, det)
        ora.render_next_iteration(it, it, r, det.to_abi())
        r = next_ppm_radius(r, it)
    sched.append(gpu.grid_schedule()[0])
    g, o = gpu.getOutputBuffer().astype(np.float64), ora.output().astype(np.float64)
    errs.append(float(np.sqrt(((g - o) ** 2).sum() / (o ** 2).sum())))
print(json.dumps({"errs": errs, "pipelined": gpu.pipelined(), "sched": sched}))
'''
    env = dict(os.environ, ORX_PIPELINE=pipeline, ORX_GRID_ASYNC=gasync)
    if gasync == "auto":
        env.pop("ORX_GRID_ASYNC")
    out = subprocess.run([sys.executable, "-c", code, str(photon_map), "1" if large else "0"], env=env,
                         capture_output=True, text=True, timeout=110,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert all(e < 1e-5 for e in res["errs"]), res
    assert res["pipelined"] == (pipeline == "1"), res  # no silent fallback to the serial schedule
    if gasync == "auto":  # chosen within each size's iterations (the first pipelined one is timed)
        assert all(m in (0, 1) for m in res["sched"]), res
    elif pipeline == "1" and photon_map == 0:
        assert res["sched"] == [int(gasync)] * len(res["sched"]), res


_VCM_CHILD = r'''
import json, sys, numpy as np
sys.path.insert(0, "tests")
import oracle_lib
from oppositerenderer_amd import _abi, scenes
from oppositerenderer_amd.renderer import OptixRenderer, RenderRequestDetails, next_ppm_radius
scene = scenes.scene_by_name("CornellSmall")
W, H = 96, 72
cfg = _abi.default_config(seed=1645301512, photon_launch_width=64, photon_launch_height=64)
gpu = OptixRenderer(cfg); gpu.initialize(0); gpu.initScene(scene)
ora = oracle_lib.OracleRenderer(_abi.default_config(seed=1645301512, photon_launch_width=64, photon_launch_height=64))
ora.init_scene(scene)
cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
det = RenderRequestDetails(cam, scene.name, _abi.VCM_BIDIRECTIONAL_PATH_TRACING, W, H)
r = scene.initial_ppm_radius()
for it in range(3):
    gpu.renderNextIteration(it, it, r, True, det)
    ora.render_next_iteration(it, it, r, det.to_abi())
    r = next_ppm_radius(r, it)
bad = {}
for buf, name in ((_abi.BUF_RNG, "rng"), (_abi.BUF_VCM_CAMERA, "camera"), (_abi.BUF_VCM_VERTEX_COUNT, "counts")):
    g, o = gpu.read_buffer(buf, np.uint32), ora.read_buffer(buf, np.uint32)
    bad[name] = int(np.count_nonzero(g != o))
g, o = gpu.getOutputBuffer().astype(np.float64), ora.output().astype(np.float64)
st = gpu.stats()
print(json.dumps({"bad": bad, "err": float(np.sqrt(((g - o) ** 2).sum() / (o ** 2).sum())), "mean": float(g.mean()),
                  "rays": int(st.vcm_shadow_rays), "overflow": int(st.vcm_shadow_overflow),
                  "lconn": int(st.vcm_light_connections), "linplace": int(st.vcm_light_inplace)}))
'''


@pytest.mark.gpu
@pytest.mark.parametrize("defer", ["16", "0", "1"])
def test_vcm_camera_shadow_modes(defer):
    """The VCM camera pass's connection shadow rays (vcm.h:315-400, connectLightSourceS1 :406-488):
    deferred to k_vcm_shadow with the colours summed by k_vcm_accum in the reference's order (the
    default, ORX_VCM_DEFER=16 entries per pixel; ~6.5 rays per pixel on the hall), traced in place
    inside the camera kernel (ORX_VCM_DEFER=0), and
    deferred into a list too small for them (1 per pixel: the walk overflows, walks on without entries,
    and the resolve's last kernel reruns the colours from the saved RNG start words).  Camera colours, RNG and vertex counts bit-exact against the oracle, three
    iterations back to back (the overlapped schedule cycles both entry lists and light images and
    reruns each overflow after the previous iteration's colours), and the overflow flag as expected."""
    import subprocess, sys, os, json
    env = dict(os.environ, ORX_VCM_DEFER=defer)
    out = subprocess.run([sys.executable, "-c", _VCM_CHILD], env=env, capture_output=True, text=True, timeout=110,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert all(v == 0 for v in res["bad"].values()), res
    assert res["err"] < 1e-5 and res["mean"] > 0, res
    if defer == "16":
        assert res["rays"] > 0 and res["overflow"] == 0, res
    elif defer == "1":
        assert res["overflow"] == 1, res  # the rerun path ran
        # with the light pass's camera connections deferred into the same resolve: the rerun reads the
        # light image those splats land in, so it must follow k_vcm_light_shadow (it runs in the resolve,
        # in stream order after it)
        assert res["lconn"] > 0, res

@pytest.mark.gpu
@pytest.mark.parametrize("ldefer", ["4", "1", "0"])
def test_vcm_light_connection_modes(ldefer):
    """The light pass's camera connections (connectCameraT1, vcm.h:52-150) deferred to the overlapped
    resolve (ORX_VCM_LIGHT_DEFER=4 per subpath, the default), into a list too small for them (1: the
    waves whose queue does not fit trace it in place and fill their reserved entries with inert ones),
    and traced in the light pass (0).  Three iterations back to back; RNG, camera colours and vertex
    counts bit-exact, the output (light-image splats are float atomics in every mode) within 1e-5."""
    import subprocess, sys, os, json
    env = dict(os.environ, ORX_VCM_LIGHT_DEFER=ldefer)
    out = subprocess.run([sys.executable, "-c", _VCM_CHILD], env=env, capture_output=True, text=True, timeout=110,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert all(v == 0 for v in res["bad"].values()), res
    assert res["err"] < 1e-5 and res["mean"] > 0, res
    if ldefer == "4":
        assert res["lconn"] > 0 and res["linplace"] == 0, res
    elif ldefer == "1":
        assert res["lconn"] > 0 and res["linplace"] > 0, res  # both paths ran
    else:
        assert res["lconn"] == 0 and res["linplace"] == 0, res


@pytest.mark.gpu
def test_vcm_resolve_bounds_stale_lists():
    """The VCM resolve driven with stale list state (orx_debug_vcm_stale_resolve): an entry count past
    the list's capacity, every odd pixel's list head past the entries, and light-connection entries whose
    pixel offsets lie past the light image -- what a walk or light pass that did not write the set's
    control words would leave (the round-5 timing variant that faulted in k_vcm_accum).
    The resolve must complete: even pixels' colours bit-identical to the real resolve (their lists are
    intact), odd pixels' colours at most the real ones (the sum stops at the bad head), all finite."""
    import ctypes as C
    scene = scenes.scene_by_name("CornellSmall")
    W, H = 96, 72
    r = OptixRenderer(_abi.default_config(seed=SEED, photon_launch_width=64, photon_launch_height=64))
    r.initialize(0)
    r.initScene(scene)
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
    det = RenderRequestDetails(cam, scene.name, _abi.VCM_BIDIRECTIONAL_PATH_TRACING, W, H)
    radius = scene.initial_ppm_radius()
    for it in range(2):
        r.renderNextIteration(it, it, radius, True, det)
    before = r.read_buffer(_abi.BUF_VCM_CAMERA, np.float32).reshape(-1, 3).copy()
    assert r.stats().vcm_light_connections > 0
    f = r._lib.orx_debug_vcm_stale_resolve
    f.argtypes, f.restype = [C.c_void_p], C.c_int
    assert f(r._h) == 0, r._lib.orx_last_error(r._h)
    after = r.read_buffer(_abi.BUF_VCM_CAMERA, np.float32).reshape(-1, 3)
    assert np.isfinite(after).all() and np.isfinite(r.getOutputBuffer()).all()
    assert np.array_equal(after[0::2], before[0::2])
    assert (after[1::2] <= before[1::2]).all()
    assert (after[1::2] < before[1::2]).any()  # the bad heads were read and stopped the sums
    r.destroy()


@pytest.mark.gpu
def test_method_switches_without_reads():
    """PPM (pipelined), PT and VCM iterations issued back to back with no read in between: the
    deferred PPM gather/output is ordered before the next method's passes, the RNG chain runs
    through all of them, and the final image matches the oracle running the same sequence."""
    scene = scenes.cornell()
    W, H, P = 48, 40, 64
    gpu, ora, _ = make_pair(scene, W, H, P, _abi.PROGRESSIVE_PHOTON_MAPPING)
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
    seq = [(_abi.PROGRESSIVE_PHOTON_MAPPING, 0), (_abi.PROGRESSIVE_PHOTON_MAPPING, 1), (_abi.PATH_TRACING, 0),
           (_abi.PATH_TRACING, 1), (_abi.VCM_BIDIRECTIONAL_PATH_TRACING, 0), (_abi.PROGRESSIVE_PHOTON_MAPPING, 0),
           (_abi.PROGRESSIVE_PHOTON_MAPPING, 1), (_abi.PROGRESSIVE_PHOTON_MAPPING, 2)]
    radius = scene.initial_ppm_radius()
    for it, (method, local) in enumerate(seq):
        det = RenderRequestDetails(cam, scene.name, method, W, H)
        gpu.renderNextIteration(it, local, radius, True, det)
        ora.render_next_iteration(it, local, radius, det.to_abi())
        radius = next_ppm_radius(radius, it)
    g, o = gpu.getOutputBuffer(), ora.output()
    assert rel_l2(g, o) < 1e-5 and g.mean() > 0
    assert gpu.pipelined()
    gpu.destroy()
    ora.close()


@pytest.mark.gpu
def test_vcm_shadow_overlap_schedules():
    """VCM's deferred shadow rays and colours of iteration i run beside the light pass and camera
    subpaths of i+1 (the light images and entry lists alternate, orx_host_vcm.hip vcm_camera): overlapped
    iterations, a serial stretch (orx_set_iteration_pipelining(0)), overlap again, a PPM iteration in
    between and VCM once more, every camera colour and RNG word bit-exact and the output matching the
    oracle after each step."""
    scene = scenes.cornell()
    W, H, P = 48, 40, 64
    gpu, ora, _ = make_pair(scene, W, H, P, _abi.VCM_BIDIRECTIONAL_PATH_TRACING)
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
    radius = scene.initial_ppm_radius()
    seen = []
    steps = [(_abi.VCM_BIDIRECTIONAL_PATH_TRACING, 0, -1), (_abi.VCM_BIDIRECTIONAL_PATH_TRACING, 1, -1),
             (_abi.VCM_BIDIRECTIONAL_PATH_TRACING, 2, -1), (_abi.VCM_BIDIRECTIONAL_PATH_TRACING, 3, 0),
             (_abi.VCM_BIDIRECTIONAL_PATH_TRACING, 4, 1), (_abi.PROGRESSIVE_PHOTON_MAPPING, 0, -1),
             (_abi.VCM_BIDIRECTIONAL_PATH_TRACING, 0, -1), (_abi.VCM_BIDIRECTIONAL_PATH_TRACING, 1, -1)]
    for it, (method, local, mode) in enumerate(steps):
        gpu.set_iteration_pipelining(mode)
        det = RenderRequestDetails(cam, scene.name, method, W, H)
        gpu.renderNextIteration(it, local, radius, True, det)
        ora.render_next_iteration(it, local, radius, det.to_abi())
        seen.append(gpu.pipelined())
        if method == _abi.VCM_BIDIRECTIONAL_PATH_TRACING:
            for buf in (_abi.BUF_RNG, _abi.BUF_VCM_CAMERA):
                g, o = gpu.read_buffer(buf, np.uint32), ora.read_buffer(buf, np.uint32)
                assert np.array_equal(g, o), (it, buf, int(np.count_nonzero(g != o)))
        g, o = gpu.getOutputBuffer(), ora.output()
        assert rel_l2(g, o) < 1e-5 and g.mean() > 0, (it, rel_l2(g, o))
        radius = next_ppm_radius(radius, it)
    assert seen == [True, True, True, False, True, True, True, True], seen
    gpu.destroy()
    ora.close()


@pytest.mark.gpu
def test_pipelining_starts_after_other_methods():
    """The second buffer set of PPM pipelining is allocated on the first pipelined iteration, not
    at the resize: PT first (no second set), then PPM at the same size pipelines, then a serial
    stretch (orx_set_iteration_pipelining(0)) and pipelining again, all matching the oracle."""
    scene = scenes.cornell()
    W, H, P = 48, 40, 64
    gpu, ora, _ = make_pair(scene, W, H, P, _abi.PATH_TRACING)
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
    radius = scene.initial_ppm_radius()
    seen = []
    for it, (method, local, mode) in enumerate([(_abi.PATH_TRACING, 0, -1), (_abi.PROGRESSIVE_PHOTON_MAPPING, 0, -1),
                                                (_abi.PROGRESSIVE_PHOTON_MAPPING, 1, -1),
                                                (_abi.PROGRESSIVE_PHOTON_MAPPING, 2, 0),
                                                (_abi.PROGRESSIVE_PHOTON_MAPPING, 3, 1),
                                                (_abi.PROGRESSIVE_PHOTON_MAPPING, 4, 1)]):
        gpu.set_iteration_pipelining(mode)
        det = RenderRequestDetails(cam, scene.name, method, W, H)
        gpu.renderNextIteration(it, local, radius, True, det)
        ora.render_next_iteration(it, local, radius, det.to_abi())
        seen.append(gpu.pipelined())
        radius = next_ppm_radius(radius, it)
    assert seen == [False, True, True, False, True, True], seen
    g, o = gpu.getOutputBuffer(), ora.output()
    assert rel_l2(g, o) < 1e-5 and g.mean() > 0
    gpu.destroy()
    ora.close()


@pytest.mark.fresh_process
@pytest.mark.parametrize("order", [8, 3])
def test_gather_tile_order(order, tmp_path):
    """The super-tile gather order (orx_host_ppm.hip gather_order; on by default from 4M pixels) on an
    image whose 13 x 10 tiles are multiples of neither 8 nor 3: the local gather and the three-shard
    external gather against the oracle in a fresh process with ORX_GATHER_ORDER set
    (tests/gather_order_child.py).  No lit pixel may be left dark (a skipped tile)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ORX_GATHER_ORDER=str(order))
    out = subprocess.run([sys.executable, "-u", os.path.join(root, "tests", "gather_order_child.py")], env=env,
                         capture_output=True, text=True, timeout=150, cwd=root)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["order"] == str(order)
    assert res["lit_pixels"] > 1000, res
    assert res["dark_pixels"] == 0, res
    assert res["local_indirect_rel_l2"] < 1e-5, res
    assert res["local_output_rel_l2"] < 1e-4, res
    assert res["rows3_output_rel_l2"] < 1e-5, res
