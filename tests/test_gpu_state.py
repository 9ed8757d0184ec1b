"""Checkpoint / resume on one renderer (include/orx.h orx_save_state / orx_restore_state,
csrc/orx_host_state.hip) (TEST: GPU).

"straight" is N iterations on one fresh renderer; "resumed" is k iterations, saveState, destroy, then a fresh
renderer with initScene, restoreState and N - k more.  Seed 1645301512, radii from multigpu.radius_sequence.
The frame is 40x25 with a 32x34 photon launch: rng 40x34, so there are RNG slots only pixels use (x >= 32),
slots only photon threads use (y >= 25) and slots nothing uses (x >= 32, y >= 25).

Bars: RNG and per-iteration buffers bit-equal to the straight render (the chain of every slot continues where
it stopped); running sums against the ORACLE's straight render at the bars of tests/test_gpu_steady_state.py
(indirect rel-L2 <= 1e-5, output <= 1e-4: fp32 summation order only); PT bit-equal to both."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib
from oppositerenderer_amd import _abi, multigpu, scenes
from oppositerenderer_amd.renderer import OptixRenderer, OrxError, RenderRequestDetails, state_info

pytestmark = pytest.mark.gpu
SEED = 1645301512
W, H, PW, PH = 40, 25, 32, 34
METHODS = {"ppm": _abi.PROGRESSIVE_PHOTON_MAPPING, "vcm": _abi.VCM_BIDIRECTIONAL_PATH_TRACING, "pt": _abi.PATH_TRACING}


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b * b).sum()), 1e-30))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def request(scene, method, w=W, h=H):
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(w) / np.float32(h)))
    return RenderRequestDetails(cam, scene.name, METHODS[method], w, h)


def config(pw=PW, ph=PH, **kw):
    return _abi.default_config(seed=kw.pop("seed", SEED), photon_launch_width=pw, photon_launch_height=ph, **kw)


def renderer(cfg, scene=None, pipe=-1):
    r = OptixRenderer(cfg)
    r.initialize(0)
    if scene is not None:
        r.initScene(scene)
    r.set_iteration_pipelining(pipe)
    return r


def run(r, scene, det, first, count, total):
    radii = multigpu.radius_sequence(scene.initial_ppm_radius(), total)
    for i in range(first, first + count):
        r.renderNextIteration(i, i, radii[i], True, det)


def snapshot(r, buffers):
    out = {"output": r.getOutputBuffer().copy()}
    for b in buffers:
        out[b] = r.read_buffer(b, np.uint32).copy()
    for v in out.values():
        v.setflags(write=False)
    return out


BUFS = {"ppm": (_abi.BUF_RNG, _abi.BUF_HITPOINTS, _abi.BUF_INDIRECT),
        "vcm": (_abi.BUF_RNG, _abi.BUF_VCM_VERTEX_COUNT, _abi.BUF_VCM_CAMERA),
        "pt": (_abi.BUF_RNG,)}


@functools.lru_cache(maxsize=None)
def straight(scene_name, method, n, pw, ph, photon_map, pipe):
    scene = scenes.scene_by_name(scene_name)
    r = renderer(config(pw, ph, photon_map=photon_map), scene, pipe)
    run(r, scene, request(scene, method), 0, n, n)
    snap = snapshot(r, BUFS[method])
    r.destroy()
    return snap


def resumed(scene_name, method, n, k, pw, ph, photon_map, pipe):
    scene = scenes.scene_by_name(scene_name)
    det = request(scene, method)
    a = renderer(config(pw, ph, photon_map=photon_map), scene, pipe)
    run(a, scene, det, 0, k, n)
    blob = a.saveState()
    a.destroy()
    info = state_info(blob)
    radii = multigpu.radius_sequence(scene.initial_ppm_radius(), n)
    assert (info.kind, info.width, info.height, info.rng_width, info.rng_height) == (0, W, H, max(pw, W), max(ph, H))
    assert (info.photon_launch_width, info.photon_launch_height, info.method) == (pw, ph, METHODS[method])
    assert (info.iteration_number, info.local_iteration_number) == (k - 1, k - 1)
    assert info.ppm_radius == np.float32(radii[k - 1]) and len(blob) == info.total_bytes
    b = renderer(config(pw, ph, photon_map=photon_map), scene, pipe)
    b.restoreState(blob)
    assert (b.getWidth(), b.getHeight()) == (W, H)
    assert b.saveState() == blob  # a restore leaves exactly the saved state
    run(b, scene, det, k, n - k, n)
    snap = snapshot(b, BUFS[method])
    b.destroy()
    return snap


@functools.lru_cache(maxsize=None)
def oracle(scene_name, method, n, pw, ph, photon_map=0):
    """the oracle's straight render: computed once per configuration, read-only"""
    scene = scenes.scene_by_name(scene_name)
    ora = oracle_lib.OracleRenderer(config(pw, ph, photon_map=photon_map))
    ora.init_scene(scene)
    req = request(scene, method).to_abi()
    radii = multigpu.radius_sequence(scene.initial_ppm_radius(), n)
    for i in range(n):
        ora.render_next_iteration(i, i, radii[i], req)
    out = {"output": ora.output().copy(), _abi.BUF_RNG: ora.read_buffer(_abi.BUF_RNG, np.uint32)}
    if method == "ppm":
        out[_abi.BUF_INDIRECT] = ora.read_buffer(_abi.BUF_INDIRECT)
    ora.close()
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("pipe,photon_map,pw,ph", [(1, 0, PW, PH), (0, 0, PW, PH), (1, 1, 32, 32), (1, 2, PW, PH)])
def test_ppm_resumes(pipe, photon_map, pw, ph):
    """the stochastic hash needs a power-of-two launch: 32x32 with the default 4 deposits, as test_stochastic_hash.py"""
    n, k = 6, 3
    ref = straight("Cornell", "ppm", n, pw, ph, photon_map, pipe)
    got = resumed("Cornell", "ppm", n, k, pw, ph, photon_map, pipe)
    ora = oracle("Cornell", "ppm", n, pw, ph, photon_map)
    e_ind = rel_l2(got[_abi.BUF_INDIRECT].view(np.float32), ora[_abi.BUF_INDIRECT])
    e_out = rel_l2(got["output"], ora["output"])
    print(f"ppm pipe {pipe} map {photon_map}: indirect rel-L2 {e_ind:.3e}, output {e_out:.3e}, "
          f"output vs straight {rel_l2(got['output'], ref['output']):.3e}")
    assert np.array_equal(got[_abi.BUF_RNG], ref[_abi.BUF_RNG])
    assert np.array_equal(got[_abi.BUF_RNG], ora[_abi.BUF_RNG])
    assert np.array_equal(got[_abi.BUF_HITPOINTS], ref[_abi.BUF_HITPOINTS])
    assert ora["output"].mean() > 0
    assert e_ind <= 1e-5, e_ind
    assert e_out <= 1e-4, e_out


@pytest.mark.parametrize("pipe", [1, 0])
def test_vcm_resumes(pipe):
    """fails when the restore replays the subpath-length estimate (every RNG slot advances once more) or leaves
    the pixel size factor at its default (the light-tracing splats land elsewhere)"""
    n, k = 4, 2
    ref = straight("Cornell", "vcm", n, PW, PH, 0, pipe)
    got = resumed("Cornell", "vcm", n, k, PW, PH, 0, pipe)
    ora = oracle("Cornell", "vcm", n, PW, PH)
    for b, name in ((_abi.BUF_RNG, "rng"), (_abi.BUF_VCM_VERTEX_COUNT, "vertex counts"), (_abi.BUF_VCM_CAMERA, "camera")):
        assert np.array_equal(got[b], ref[b]), f"{name}: {np.count_nonzero(got[b] != ref[b])} of {got[b].size} words differ"
    err = rel_l2(got["output"], ora["output"])
    print(f"vcm overlap {pipe}: output rel-L2 {err:.3e}")
    assert ora["output"].mean() > 0
    assert err <= 1e-4, err


def test_pt_resumes_bit_equal():
    n, k, name = 4, 2, "CornellSmallSmallSpheres"
    ref = straight(name, "pt", n, PW, PH, 0, 1)
    got = resumed(name, "pt", n, k, PW, PH, 0, 1)
    ora = oracle(name, "pt", n, PW, PH)
    assert ref["output"].mean() > 0
    for other in (ref, ora):
        assert np.array_equal(bits(got["output"]), bits(other["output"]))
        assert np.array_equal(got[_abi.BUF_RNG], other[_abi.BUF_RNG])


def test_save_is_inert():
    """six PPM iterations with a save after the third equal six without one.  The save only synchronises and
    reads, as the output read of tests/test_gpu_group.py does, and the passes' sums do not depend on the
    schedule: the issue's rel-L2 <= 1e-5 bar for the output is held as bit equality."""
    scene = scenes.cornell()
    det = request(scene, "ppm")
    ref = straight("Cornell", "ppm", 6, PW, PH, 0, 1)
    r = renderer(config(), scene, 1)
    run(r, scene, det, 0, 3, 6)
    blob = r.saveState()
    assert r.saveState() == blob
    run(r, scene, det, 3, 3, 6)
    got = snapshot(r, BUFS["ppm"])
    r.destroy()
    assert np.array_equal(got[_abi.BUF_RNG], ref[_abi.BUF_RNG])
    assert np.array_equal(got[_abi.BUF_HITPOINTS], ref[_abi.BUF_HITPOINTS])
    err = rel_l2(got["output"], ref["output"])
    print(f"save in the middle: output rel-L2 {err:.3e}, bit-equal {np.array_equal(bits(got['output']), bits(ref['output']))}")
    assert err <= 1e-5, err
    assert np.array_equal(bits(got["output"]), bits(ref["output"]))


def test_restart_after_restore_keeps_rng_and_clears_sum():
    """local iteration 0 after a restore clears the sum, as ever, and keeps the restored RNG; a request of
    another size resizes and seeds again"""
    scene = scenes.cornell()
    det = request(scene, "pt")
    a = renderer(config(), scene)
    run(a, scene, det, 0, 2, 3)
    blob = a.saveState()
    a.renderNextIteration(2, 0, 0.1, True, det)  # the same restart without a save and restore
    want = snapshot(a, BUFS["pt"])
    a.destroy()
    b = renderer(config(), scene)
    b.restoreState(blob)
    b.renderNextIteration(2, 0, 0.1, True, det)
    got = snapshot(b, BUFS["pt"])
    assert np.array_equal(got[_abi.BUF_RNG], want[_abi.BUF_RNG])
    assert np.array_equal(bits(got["output"]), bits(want["output"]))
    small = request(scene, "pt", 24, 16)
    b.renderNextIteration(0, 0, 0.1, True, small)
    fresh = renderer(config(), scene)
    fresh.renderNextIteration(0, 0, 0.1, True, small)
    assert np.array_equal(b.read_buffer(_abi.BUF_RNG, np.uint32), fresh.read_buffer(_abi.BUF_RNG, np.uint32))
    assert np.array_equal(bits(b.getOutputBuffer()), bits(fresh.getOutputBuffer()))
    b.destroy()
    fresh.destroy()


def status_of(fn, *args):
    with pytest.raises(OrxError) as e:
        fn(*args)
    return e.value.status, str(e.value)


def test_refusals():
    scene = scenes.cornell()
    det = request(scene, "ppm")
    a = renderer(config(), scene)
    assert status_of(a.saveState)[0] == _abi.ORX_ERR_STATE  # no frame yet
    run(a, scene, det, 0, 1, 1)
    blob = a.saveState()
    a.destroy()

    b = renderer(config())
    assert status_of(b.restoreState, blob)[0] == _abi.ORX_ERR_STATE  # before initScene
    b.initScene(scenes.cornell_small())
    st, msg = status_of(b.restoreState, blob)
    assert st == _abi.ORX_ERR_INVALID_ARGUMENT  # another scene; both keys named
    small_abi = scenes.cornell_small().to_abi()
    small_key = b._lib.orx_scene_key(C.byref(small_abi))
    assert f"{state_info(blob).scene_key:016x}" in msg and f"{small_key:016x}" in msg, msg
    b.destroy()

    c = renderer(config(PW, 32), scene)
    st, msg = status_of(c.restoreState, blob)
    assert st == _abi.ORX_ERR_INVALID_ARGUMENT and "32 x 34" in msg and "32 x 32" in msg  # another photon launch
    assert status_of(c.restoreState, blob[:-1])[0] == _abi.ORX_ERR_INVALID_ARGUMENT
    damaged = bytearray(blob)
    damaged[200] ^= 1
    assert status_of(c.restoreState, bytes(damaged))[0] == _abi.ORX_ERR_INVALID_ARGUMENT
    c.destroy()

    medium = scenes.cornell_medium()
    d = renderer(config(enable_media=1), medium)
    run(d, medium, request(medium, "ppm"), 0, 1, 1)
    assert status_of(d.saveState)[0] == _abi.ORX_ERR_UNSUPPORTED
    d.destroy()

    e = renderer(config(), scene)
    run(e, scene, det, 0, 1, 1)
    e.set_shard(0, 2)
    assert status_of(e.saveState)[0] == _abi.ORX_ERR_UNSUPPORTED
    assert status_of(e.restoreState, blob)[0] == _abi.ORX_ERR_UNSUPPORTED
    e.destroy()


def test_clock_seeded_render_resumes_exactly():
    scene = scenes.cornell()
    det = request(scene, "ppm")
    a = renderer(config(seed=0), scene)
    run(a, scene, det, 0, 2, 3)
    blob = a.saveState()
    a.destroy()
    rngs = []
    for _ in range(2):
        b = renderer(config(seed=0), scene)
        b.restoreState(blob)
        run(b, scene, det, 2, 1, 3)
        rngs.append(b.read_buffer(_abi.BUF_RNG, np.uint32).copy())
        b.destroy()
    assert np.array_equal(rngs[0], rngs[1])
    assert not np.array_equal(rngs[0], np.frombuffer(blob, np.uint32, rngs[0].size, 128))  # and it did advance


def test_render_manager_save_and_resume(tmp_path):
    """StandaloneRenderManager.save / resume: the iteration number and the radius go on from the header"""
    from oppositerenderer_amd.renderer import StandaloneRenderManager

    def manager():
        return StandaloneRenderManager(renderer(config()), scenes.cornell(), METHODS["ppm"], W, H)

    full = manager()
    for _ in range(4):
        full.render_next_iteration()
    want = snapshot(full.renderer, BUFS["ppm"])
    a = manager()
    a.render_next_iteration()
    a.render_next_iteration()
    a.save(tmp_path / "state.bin")
    b = manager()
    b.resume(tmp_path / "state.bin")
    # the header holds the radius as the renderer got it, a float: the schedule goes on from its rounding
    assert b.iteration == 2 and abs(b.radius - a.radius) <= 2.0 ** -23 * a.radius
    b.render_next_iteration()
    b.render_next_iteration()
    got = snapshot(b.renderer, BUFS["ppm"])
    assert b.iteration == full.iteration and abs(b.radius - full.radius) <= 2.0 ** -23 * full.radius
    assert np.array_equal(got[_abi.BUF_RNG], want[_abi.BUF_RNG])
    assert np.array_equal(got[_abi.BUF_HITPOINTS], want[_abi.BUF_HITPOINTS])
    assert rel_l2(got["output"], want["output"]) <= 1e-5
    for m in (full, a, b):
        m.renderer.destroy()
